// launch_host.hpp -- the host side of the launch layer: how a dmt_render* call becomes work on the device.  The kernel
// tables, the fold check behind dmt_sync, the tile grid of a region, the plan of a launch (host arithmetic only) and its
// enqueue, the wavefront form, adaptive rounds, the counting launches, the layer's settings and the event-pair timing.  The
// layer's state and its rules are in launch_state.hpp, its device code in launch_device.hpp.
//
// Part of dmt_hip.hip's translation unit, included once after surface_host.hpp and baseParams and before
// denoise_host.hpp: it uses resolveFeatures, checkFeatures, baseParams, requireTree, reserveOverflow, bvhView and
// motionParams and SceneState::matIdOutside; denoise_host.hpp and probes.hpp call checkErrorFlag, and camera_host.hpp's
// dmt_download_film reaches it through a forward declaration.
#pragma once

namespace {

// kernel tables: {mask, kernel} per row of the device-side lists; a mask without a row has no kernel (nullptr)
template <class Fn>
struct KernelRow { uint32_t mask; Fn fn; };
template <class Fn, size_t N>
Fn kernelOf(KernelRow<Fn> const (&rows)[N], uint32_t mask) {
  for (KernelRow<Fn> const& r : rows) if (r.mask == mask) return r.fn;
  return nullptr;
}
int noKernel(dmt_ctx* ctx, char const* what, uint32_t mask) {
  ctx->err = std::string(what) + ": no kernel is compiled for this combination of scene features (mask " + std::to_string(mask) + ")";
  return DMT_ERR_STATE;
}
typedef void (*MegakernelFn)(RenderParams);
typedef void (*WfKernelFn)(RenderParams, WfParams);
#define DMT_MEGAKERNEL_ROW(suffix, mask, waves, body) {mask, k_megakernel##suffix},
#define DMT_WF_SHADE_ROW(suffix, mask, waves) {mask, k_wf_shade##suffix},
KernelRow<MegakernelFn> const kMegakernels[] = {DMT_MEGAKERNELS(DMT_MEGAKERNEL_ROW) DMT_STATS_MEGAKERNELS(DMT_MEGAKERNEL_ROW)};
KernelRow<WfKernelFn> const kWfShadeKernels[] = {DMT_WF_SHADE_KERNELS(DMT_WF_SHADE_ROW)};

MegakernelFn megakernelOf(uint32_t mask) { return kernelOf(kMegakernels, mask); }
// resident 256-thread blocks per CU of a kernel (cached per context)
int blocksPerCuOf(dmt_ctx* c, MegakernelFn kernel) {
  void const* const fn = reinterpret_cast<void const*>(kernel);
  for (auto const& e : c->launch.occupancy)
    if (e.first == fn) return e.second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, 0) != hipSuccess || n <= 0) n = 1;
  c->launch.occupancy.emplace_back(fn, n);
  return n;
}

// the scheduler's diagnostic words as the device holds them; the caller has synchronised as far as it means to
int readSchedDiag(dmt_ctx* ctx, unsigned long long (&d)[kSchedDiagWords]) {
  HIP_TRY(ctx, hipMemcpy(d, ctx->launch.sched.diag.get(), sizeof(d), hipMemcpyDeviceToHost));
  return DMT_OK;
}

// After the stream has drained: every work item of every past launch must have been folded into the film exactly once
// (item_complete / fold_chain count their folds).  Anything else means the hand-over protocol lost or duplicated a sample
// chunk and the film is not the ordered fold the contract promises.
int checkErrorFlag(dmt_ctx* ctx) {
  LaunchState& S = ctx->launch;
  unsigned long long d[kSchedDiagWords] = {};
  if (int const rc = readSchedDiag(ctx, d)) return rc;
  unsigned long long const folds = d[SD_FOLDS];
  // a wave left a launch with parked hits in its queue: their samples are missing.  Reported once per difference; the
  // device counters stay as they are for dmt_ggx_batch_diag
  if (d[SD_GGX_PARKED] - d[SD_GGX_RESUMED] != S.ggx.lostReported) {
    char msg[200];
    snprintf(msg, sizeof(msg), "GGX batching: %llu hits were parked, %llu were taken back: the film is invalid", d[SD_GGX_PARKED],
             d[SD_GGX_RESUMED]);
    S.ggx.lostReported = d[SD_GGX_PARKED] - d[SD_GGX_RESUMED];
    return fail(ctx, DMT_ERR_HIP, msg);
  }
  if (folds != S.sched.expectedFolds) {
    char msg[200];
    snprintf(msg, sizeof(msg), "in-launch ordering: %llu sample chunks were folded into the film, %llu were launched: the film is invalid",
             folds, S.sched.expectedFolds);
    S.sched.expectedFolds = folds;  // report once
    return fail(ctx, DMT_ERR_HIP, msg);
  }
  return DMT_OK;
}

// ---- what renderImpl and dmt_render_adaptive ask first, each under its own name --------------------
int requireScene(dmt_ctx* ctx, char const* caller) {
  if (ctx->scene.haveTris && ctx->scene.haveBsdfs && ctx->lights.list.have && ctx->camera.have) return DMT_OK;
  ctx->err = std::string(caller) + ": upload triangles, bsdfs, lights and set the camera first";
  return DMT_ERR_STATE;
}
// A pixel rectangle clamped to the film, the 8x8 tiles it touches, and the share of them this context's rank owns: region
// tile j (row-major from the region's first tile) belongs to rank j % world, as item_geom, k_adaptive_mask and wf_pixel
// (wavefront.hpp) decode it.
struct TileGrid {
  int x0, y0, x1, y1, rank, world;
  int tx0 = 0, ty0 = 0, rtx = 0;   // origin (in tiles) and tiles per row
  uint32_t tiles = 0, owned = 0;
  TileGrid(dmt_ctx const* c, int ax0, int ay0, int ax1, int ay1)
      : x0(std::max(ax0, 0)), y0(std::max(ay0, 0)), x1(std::min(ax1, c->film.w)), y1(std::min(ay1, c->film.h)), rank(c->launch.rank), world(c->launch.world) {
    if (empty()) return;
    tx0 = x0 / 8, ty0 = y0 / 8, rtx = (x1 + 7) / 8 - tx0;
    tiles = uint32_t(rtx) * uint32_t((y1 + 7) / 8 - ty0);
    owned = tiles > uint32_t(rank) ? (tiles - uint32_t(rank) + uint32_t(world) - 1) / uint32_t(world) : 0;
  }
  bool empty() const { return x1 <= x0 || y1 <= y0; }
  // the nine fields RenderParams and AdaptiveArgs share
  template <class Args>
  void put(Args& a) const {
    a.x0 = x0, a.y0 = y0, a.x1 = x1, a.y1 = y1, a.tx0 = tx0, a.ty0 = ty0, a.rtx = rtx, a.rank = rank, a.world = world;
  }
  // pixels of the owned tiles inside the region
  uint64_t ownedPixels() const {
    uint64_t pixels = 0;
    for (uint32_t item = 0; item < owned; ++item) {
      uint32_t const j = uint32_t(rank) + item * uint32_t(world);
      int const px0 = (tx0 + int(j % uint32_t(rtx))) * 8, py0 = (ty0 + int(j / uint32_t(rtx))) * 8;
      int const w = std::min(px0 + 8, x1) - std::max(px0, x0), hgt = std::min(py0 + 8, y1) - std::max(py0, y0);
      if (w > 0 && hgt > 0) pixels += uint64_t(w) * uint64_t(hgt);
    }
    return pixels;
  }
};

// the 16 counters of a counting launch: reserved, zeroed on the stream, and P.stats points at them
int armStats(dmt_ctx* ctx, RenderParams& P) {
  HIP_TRY(ctx, ctx->launch.sched.stats.reserve(16));
  HIP_TRY(ctx, hipMemsetAsync(ctx->launch.sched.stats.get(), 0, 16 * sizeof(unsigned long long), ctx->stream));
  P.stats = ctx->launch.sched.stats.get();
  return DMT_OK;
}

// Wavefront form of a BVH launch (wavefront.hpp): passes over (owned tiles, sample range), each pass a fixed sequence of
// kernels on the context's stream.  G = the tiles this rank renders; P carries region / partition / film.
// `shade` = the k_wf_shade* row of the launch's mask.
int launchWavefront(dmt_ctx* ctx, RenderParams P, TileGrid const& G, uint32_t sample_offset, uint32_t spp, WfKernelFn shade, uint64_t* stats,
                    int nstats) {
  LaunchState::Wavefront& wf = ctx->launch.wf;
  uint32_t const cuCount = uint32_t(ctx->launch.cuCount);
  uint32_t const iters = uint32_t(ctx->maxDepth) + 2u;  // closest rays at depth 0..maxDepth, + one trailing shadow ray
  size_t const target = wf.targetPaths < 4096 ? 4096 : wf.targetPaths;
  uint32_t const tilesPerPass = uint32_t(std::min<size_t>(G.owned, std::max<size_t>(1, target / 64)));
  uint32_t n = uint32_t(std::max<size_t>(1, target / (size_t(tilesPerPass) * 64)));
  if (n > spp) n = spp;
  size_t const slotsMax = size_t(tilesPerPass) * 64 * n;
  HIP_TRY(ctx, wf.state.reserve(size_t(WF_PLANES) * slotsMax));
  HIP_TRY(ctx, wf.queue.reserve(2 * slotsMax));
  size_t const nCounts = 2 * (size_t(iters) + 2);
  HIP_TRY(ctx, wf.counts.reserve(nCounts));
  if (wf.blocksTrace == 0) {
    int a = 0, b = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, reinterpret_cast<void const*>(k_wf_trace), 256, 0);
    // one shade grid for every variant: sized by the one with the most registers
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<void const*>(k_wf_shade_env_area), 256, 0);
    wf.blocksTrace = a > 0 ? a : 1, wf.blocksShade = b > 0 ? b : 1;
  }
  uint32_t const traceBlocks = cuCount * uint32_t(stats ? 4 : wf.blocksTrace);
  uint32_t const shadeBlocks = cuCount * uint32_t(stats ? 2 : wf.blocksShade);
  HIP_TRY(ctx, reserveOverflow(ctx, size_t(traceBlocks) * 256));
  P.bvh = bvhView(ctx, size_t(traceBlocks) * 256);
  if (stats) {
    if (int const rc = armStats(ctx, P)) return rc;
  }
  WfKernelFn const trace = stats ? k_wf_trace_stats : k_wf_trace;
  WfParams W{};
  W.state = wf.state.get();
  W.queue[0] = wf.queue.get(), W.queue[1] = wf.queue.get() + slotsMax;
  W.counts = wf.counts.get(), W.cursors = wf.counts.get() + (iters + 2);
  for (uint32_t tile0 = 0; tile0 < G.owned; tile0 += tilesPerPass) {
    uint32_t const tiles = std::min(tilesPerPass, G.owned - tile0);
    for (uint32_t s = 0; s < spp; s += n) {
      W.tile0 = tile0, W.pixelSlots = tiles * 64u, W.s0 = sample_offset + s, W.n = std::min(n, spp - s);
      W.slots = W.pixelSlots * W.n;
      HIP_TRY(ctx, hipMemsetAsync(wf.counts.get(), 0, nCounts * sizeof(uint32_t), ctx->stream));
      uint32_t const genBlocks = std::min<uint32_t>((W.slots + 255u) / 256u, cuCount * 8u);
      W.it = 0;
      hipLaunchKernelGGL(k_wf_generate, dim3(genBlocks), dim3(256), 0, ctx->stream, P, W);
      for (uint32_t it = 0; it < iters; ++it) {
        W.it = it;
        // a persistent grid no larger than the pass: small passes do not pay for 2 048 idle blocks per launch
        uint32_t const tb = std::min<uint32_t>(traceBlocks, (W.slots + 255u) / 256u);
        uint32_t const sb = std::min<uint32_t>(shadeBlocks, (W.slots + 255u) / 256u);
        hipLaunchKernelGGL(trace, dim3(tb), dim3(256), 0, ctx->stream, P, W);
        hipLaunchKernelGGL(shade, dim3(sb), dim3(256), 0, ctx->stream, P, W);
      }
      if (!stats) hipLaunchKernelGGL(k_wf_fold, dim3((W.pixelSlots + 255u) / 256u), dim3(256), 0, ctx->stream, P, W);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  if (stats) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> h(16, 0);
    HIP_TRY(ctx, hipMemcpy(h.data(), ctx->launch.sched.stats.get(), 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    h[0] = G.ownedPixels() * spp;  // samples (the kernels count rays, visits and bounces)
    for (int k = 0; k < nstats && k < 16; ++k) stats[k] = h[size_t(k)];
  }
  return DMT_OK;
}

// the tiles of an adaptive round (dmt_render_adaptive): `count` region tiles in `list`, their pixel masks in `mask`
struct TileSelection {
  uint32_t const* list;
  unsigned long long const* mask;
  uint32_t count;
};

// What a dmt_render* call puts on the stream, worked out before anything is allocated or enqueued: host arithmetic over the
// context's settings, the tile grid and the sample count.
struct LaunchPlan {
  uint32_t F = 0;                                 // the feature mask of the launch, without kFeatStats
  MegakernelFn kernel = nullptr;
  WfKernelFn wfShade = nullptr;                   // the k_wf_shade* row of the mask (counting: of mask | kFeatStats), if it has one
  bool wavefront = false, parksGgx = false;       // parksGgx: the row that parks GGX hits, one queue per wave
  int blocksPerCu = 0;
  uint32_t subShift = 0, numItems = 0;            // tile items: owned tiles, or the selected tiles of an adaptive round, << subShift
  uint32_t chunkSpp = 0, numChunks = 0, blocks = 0;
  SamplerTablePlan tab;
  uint32_t sliceChunks = 0;                       // chunks per megakernel launch of the call: tab.sliceChunks, or all of them without a table
  size_t busyWords = 0, linkWords = 0;            // the two parts of sched.words
  uint64_t folds = 0;                             // every item is folded exactly once (checkErrorFlag)
};
// The plan of a launch over the owned tiles of G (at least one) with the kernel of mask F (it has one).  `counting`:
// dmt_render_stats / dmt_render_profile.  Refuses a launch of more than 2^31 - 1 work items.
int planLaunch(dmt_ctx* ctx, uint32_t F, TileGrid const& G, uint32_t spp, bool counting, TileSelection const* sel, LaunchPlan& L) {
  LaunchState const& S = ctx->launch;
  L.F = F, L.kernel = megakernelOf(F);
  L.numItems = sel ? sel->count : G.owned;  // (count > 0: checked by the caller)
  // BVH launches run as the megakernel unless the wavefront form (wavefront.hpp) is asked for: on the measured scenes
  // the megakernel is faster (1 M triangles: 489 vs 378 Msamples/s), so "automatic" means megakernel
  // (BVH masks without textures, blends or a light tree have a k_wf_shade* row)
  L.wfShade = kernelOf(kWfShadeKernels, counting ? F | kFeatStats : F);
  L.wavefront = S.wf.strategy == 2 && L.wfShade != nullptr && !sel;  // (adaptive rounds: always the megakernel)
  L.blocksPerCu = blocksPerCuOf(ctx, L.kernel);
  {  // fewer owned tiles than ~4 per resident wave: schedule row bands of the tiles instead of whole tiles
    uint32_t const waves = uint32_t(S.cuCount) * uint32_t(L.blocksPerCu) * 4u;
    L.subShift = S.subShift >= 0 ? uint32_t(S.subShift) : 0u;
    if (S.subShift < 0)
      while (L.subShift < 2u && (uint64_t(L.numItems) << L.subShift) < 4ull * waves) ++L.subShift;
    L.numItems <<= L.subShift;
  }
  // samples per work item: automatic = 16 per 64 pixels (1 024 path samples per item); bounded so the staging
  // area (768 B per sample index per resident wave and slot) stays small
  L.chunkSpp = S.chunkSpp ? S.chunkSpp : (16u << L.subShift);
  if (L.chunkSpp > spp) L.chunkSpp = spp;
  if (L.chunkSpp > kMaxChunkSpp) L.chunkSpp = kMaxChunkSpp;
  L.numChunks = (spp + L.chunkSpp - 1) / L.chunkSpp;
  if (uint64_t(L.numItems) * L.numChunks > 0x7FFFFFFFull)
    return fail(ctx, DMT_ERR_INVALID, "dmt_render: too many work items (tiles x sample chunks); raise dmt_set_chunk or split the pass");
  // Sampler table: for plain megakernel launches only.  Counting launches are not timed, the wavefront form prepares its
  // samples per pass, and an adaptive round's live pixel count is on the device.  The owned pixels are counted in whole tiles.
  if (!counting && !L.wavefront && !sel && !(F & kFeatMotion))  // (motion launches compute their samples: the table has no time plane)
    L.tab = samplerTablePlan(ctx->film.w, ctx->film.h, uint64_t(G.owned) * 64u, spp, L.chunkSpp, S.tab.budget, S.tab.mode,
                             ctx->camera.lensR > 0.f ? kSamTabLensEntryBytes : kSamTabEntryBytes);
  uint32_t const wavesWanted = L.numItems * L.numChunks < L.numItems ? L.numItems : L.numItems * L.numChunks;
  L.blocks = uint32_t(S.cuCount) * uint32_t(L.blocksPerCu);
  uint32_t const blocksNeeded = (wavesWanted + 3) / 4;
  if (L.blocks > blocksNeeded) L.blocks = blocksNeeded;
  if (L.blocks == 0) L.blocks = 1;
  L.parksGgx = S.ggx.batchT != 0u && F == 0u && !counting && !L.wavefront;
  // A call with a sampler table runs as tab.slices consecutive sample slices, each a table fill and a megakernel launch
  // over a whole number of chunks, all inside the one event pair; the film is bit-identical under any split of the
  // sample range.  Without a table the call is one slice.
  L.sliceChunks = L.tab.use ? L.tab.sliceChunks : L.numChunks;
  L.busyWords = size_t(L.blocks) * 4u * size_t(kSlabsPerWave);
  L.linkWords = L.sliceChunks > 1 ? size_t(L.numItems) * size_t(L.sliceChunks) : 0;
  L.folds = uint64_t(L.numItems) * L.numChunks;
  return DMT_OK;
}

// Grows the buffers a planned launch reads, points P at them, and zeroes the scheduler's words on the stream.
int growLaunchBuffers(dmt_ctx* ctx, LaunchPlan const& L, uint32_t spp, RenderParams& P) {
  LaunchState& S = ctx->launch;
  {  // staging slabs of finished samples, kSlabsPerWave per wave of the launch
    size_t const floats = size_t(L.blocks) * 4u * size_t(kSlabsPerWave) * size_t(L.chunkSpp) * 192u;
    HIP_TRY(ctx, S.sched.stage.reserve(floats));
    P.stage = S.sched.stage.get();
  }
  if (L.parksGgx) {
    HIP_TRY(ctx, S.ggx.queue.reserve(size_t(L.blocks) * size_t(kLdsThreads / 64) * size_t(kGgxFields) * size_t(kGgxQueueCap)));  // (wave_index)
    P.ggxQueue = S.ggx.queue.get(), P.ggxBatchT = S.ggx.batchT;
  }
  {  // slab-busy marks + one hand-over word per (chunk, tile item), all zero at launch
    HIP_TRY(ctx, S.sched.words.reserve(L.busyWords + L.linkWords));
    P.slabBusy = S.sched.words.get(), P.link = S.sched.words.get() + L.busyWords;
    HIP_TRY(ctx, hipMemsetAsync(S.sched.words.get(), 0, (L.busyWords + L.linkWords) * sizeof(uint32_t), ctx->stream));
  }
  if (L.tab.use) {
    size_t const sliceEntries = size_t(std::min<uint64_t>(uint64_t(L.sliceChunks) * L.chunkSpp, spp)) * L.tab.pw * L.tab.ph;
    HIP_TRY(ctx, S.tab.vals.reserve(2 * sliceEntries));
    HIP_TRY(ctx, S.tab.jit.reserve(sliceEntries));
    P.samTab = S.tab.vals.get(), P.samTabJit = S.tab.jit.get(), P.samTabPw = L.tab.pw, P.samTabPh = L.tab.ph;
    if (ctx->camera.lensR > 0.f) {
      HIP_TRY(ctx, S.tab.lens.reserve(sliceEntries));
      P.samTabLens = S.tab.lens.get();
    } else if (ctx->camera.projKind == DMT_PROJECTION_PERSPECTIVE) {
      P.camTail = 0.f;  // a pixel filter alone: the jitter plane holds the warped jitter, the main path needs no tail
    }  // (another projection keeps its tail, which recomputes the jitter by tail_jitter: the jitter plane's bits)
  }
  return DMT_OK;
}

// The megakernel launches of a call: one per sample slice, each after its table fill.
int enqueueSlices(dmt_ctx* ctx, LaunchPlan const& L, RenderParams& P, uint32_t sample_offset, uint32_t spp) {
  LaunchState& S = ctx->launch;
  for (uint32_t c0 = 0; c0 < L.numChunks; c0 += L.sliceChunks) {
    uint32_t const first = c0 * P.chunkSpp;  // of the call's samples
    uint32_t const n = std::min<uint64_t>(uint64_t(L.sliceChunks) * P.chunkSpp, spp - first);
    P.sampleOffset = sample_offset + first, P.spp = n, P.numChunks = (n + P.chunkSpp - 1) / P.chunkSpp;
    if (c0 > 0) {  // the link words and the counter start every slice at zero, as they start every launch
      HIP_TRY(ctx, hipMemsetAsync(S.sched.words.get(), 0, (L.busyWords + L.linkWords) * sizeof(uint32_t), ctx->stream));
      HIP_TRY(ctx, hipMemsetAsync(S.sched.counter.get(), 0, sizeof(uint32_t), ctx->stream));
    }
    if (L.tab.use) {
      P.samTabS0 = P.sampleOffset;
      uint32_t const entries = n * L.tab.pw * L.tab.ph;
      hipLaunchKernelGGL(k_sampler_table, dim3((entries + 255u) / 256u), dim3(256), 0, ctx->stream, P.sp, P.samTabS0, n, L.tab.pw, L.tab.ph,
                         S.tab.vals.get(), S.tab.jit.get(), const_cast<float2*>(P.samTabLens), P.filtKnots, P.filtR);
      HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(L.kernel, dim3(L.blocks), dim3(256), 0, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
  }
  return DMT_OK;
}

// Grows what the plan needs and puts the launch on the stream, inside one event pair (the counting launches return before
// the pair is closed: they are not timed).
int enqueueLaunch(dmt_ctx* ctx, LaunchPlan const& L, TileGrid const& G, uint32_t sample_offset, uint32_t spp, uint64_t* stats6, int nstats,
                  TileSelection const* sel) {
  LaunchState& S = ctx->launch;
  RenderParams P = baseParams(ctx, 0);
  P.mean = ctx->film.mean, P.m2 = ctx->film.m2, P.counter = S.sched.counter.get();
  P.width = ctx->film.w, P.height = ctx->film.h;
  G.put(P);
  P.numItems = L.numItems, P.subShift = L.subShift, P.chunkSpp = L.chunkSpp, P.numChunks = L.numChunks;
  P.sampleOffset = sample_offset, P.spp = spp;
  if (sel) P.tileList = sel->list, P.tileMask = sel->mask;
  P.schedDiag = S.sched.diag.get();
  if (S.timing.used == S.timing.events.size()) {
    hipEvent_t a, b;
    HIP_TRY(ctx, hipEventCreate(&a));
    HIP_TRY(ctx, hipEventCreate(&b));
    S.timing.events.emplace_back(a, b);
  }
  auto& ev = S.timing.events[S.timing.used];
  if (int const rc = growLaunchBuffers(ctx, L, spp, P)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(S.sched.counter.get(), 0, sizeof(uint32_t), ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ev.first, ctx->stream));
  if (L.wavefront) {
    if (int const rcT = requireTree(ctx, "dmt_render")) return rcT;
    int const rcW = launchWavefront(ctx, P, G, sample_offset, spp, L.wfShade, stats6, nstats);
    if (rcW) return rcW;
    if (stats6) return DMT_OK;
  } else if (ctx->accel == DMT_ACCEL_BVH) {
    if (int const rcT = requireTree(ctx, "dmt_render")) return rcT;
    HIP_TRY(ctx, reserveOverflow(ctx, size_t(S.cuCount) * size_t(std::max(L.blocksPerCu, ctx->ac.blocksPerCUBvh)) * 256));
    P.bvh = bvhView(ctx, size_t(L.blocks) * 256);
    if (stats6) {  // the megakernel's counting launch: synchronous, not timed
      if (int const rc = armStats(ctx, P)) return rc;
      hipLaunchKernelGGL(megakernelOf(L.F | kFeatStats), dim3(L.blocks), dim3(256), 0, ctx->stream, P);
      HIP_TRY(ctx, hipGetLastError());
      S.sched.expectedFolds += L.folds;
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipMemcpy(stats6, S.sched.stats.get(), size_t(nstats) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      return DMT_OK;
    }
  }
  if (int const rcM = motionParams(ctx, L.F, P)) return rcM;
  if (!L.wavefront) {
    if (int const rc = enqueueSlices(ctx, L, P, sample_offset, spp)) return rc;
    S.sched.expectedFolds += L.folds;
  }
  HIP_TRY(ctx, hipEventRecord(ev.second, ctx->stream));
  ++S.timing.used;
  return DMT_OK;
}

int renderImpl(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1, uint64_t* stats6, int nstats,
               TileSelection const* sel = nullptr) {
  if (!ctx) return DMT_ERR_INVALID;
  if (stats6) memset(stats6, 0, size_t(nstats) * sizeof(uint64_t));
  if (int const rc = requireScene(ctx, "dmt_render")) return rc;
  // the Halton index sample * stride must stay inside int32 (CC/private/rng.cu:229)
  uint64_t const stride = uint64_t(ctx->camera.sp.scale0) * uint64_t(ctx->camera.sp.scale1);
  if ((uint64_t(sample_offset) + spp + 1) * stride > 0x7FFFFFFFull)
    return fail(ctx, DMT_ERR_INVALID, "dmt_render: sample index overflows the 32-bit Halton index");
  // every material index must address an uploaded BSDF (the kernel gathers bsdfs[matId])
  if (ctx->scene.matIdOutside())
    return fail(ctx, DMT_ERR_INVALID, "dmt_render: a triangle's material index is outside the BSDF array");
  TileGrid const G(ctx, x0, y0, x1, y1);
  if (spp == 0 || G.empty()) return DMT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t F = 0;
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  if (int const rc = checkFeatures(ctx, stats6 ? F | kFeatStats : F)) return rc;
  if (!megakernelOf(F)) return noKernel(ctx, "dmt_render", F);
  if (G.owned == 0) return DMT_OK;
  LaunchPlan L;
  if (int const rc = planLaunch(ctx, F, G, spp, stats6 != nullptr, sel, L)) return rc;
  return enqueueLaunch(ctx, L, G, sample_offset, spp, stats6, nstats, sel);
}

}  // namespace

extern "C" {

int dmt_render(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1) {
  return renderImpl(ctx, sample_offset, spp, x0, y0, x1, y1, nullptr, 0);
}

// Adaptive sampling: rounds of step_spp samples; before each round k_adaptive_mask decides which pixels go on (stopping rule
// at adaptive_active) and lists the tiles that have any, and the round is an ordinary megakernel launch over those tiles.
int dmt_render_adaptive(dmt_ctx* ctx, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, float threshold, int x0, int y0,
                        int x1, int y1, uint32_t* rounds, uint64_t* samples) {
  if (!ctx) return DMT_ERR_INVALID;
  if (rounds) *rounds = 0;
  if (samples) *samples = 0;
  if (step_spp == 0 || max_spp == 0) return fail(ctx, DMT_ERR_INVALID, "dmt_render_adaptive: step_spp and max_spp must be positive");
  if (max_spp > (1u << 24)) return fail(ctx, DMT_ERR_INVALID, "dmt_render_adaptive: max_spp above 2^24 (the sample count must stay exact in fp32)");
  if (!std::isfinite(threshold) || threshold < 0.f) return fail(ctx, DMT_ERR_INVALID, "dmt_render_adaptive: threshold must be finite and >= 0");
  if (int const rc = requireScene(ctx, "dmt_render_adaptive")) return rc;
  TileGrid const G(ctx, x0, y0, x1, y1);
  if (G.empty()) return DMT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (G.owned == 0) return DMT_OK;
  LaunchState::Adaptive& ad = ctx->launch.adaptive;
  AdaptiveArgs A{};
  A.mean = ctx->film.mean, A.m2 = ctx->film.m2, A.width = ctx->film.w;
  G.put(A);
  A.owned = G.owned;
  A.minSpp = min_spp, A.maxSpp = max_spp, A.threshold = threshold;
  size_t const filmTiles = size_t((ctx->film.w + 7) / 8) * size_t((ctx->film.h + 7) / 8);  // >= tiles of any region
  HIP_TRY(ctx, ad.mask.reserve(filmTiles));
  HIP_TRY(ctx, ad.list.reserve(filmTiles));
  HIP_TRY(ctx, ad.count.reserve(2));
  A.mask = ad.mask.get(), A.list = ad.list.get(), A.counters = ad.count.get();
  for (uint32_t offset = 0; offset < max_spp;) {
    A.offset = offset;
    HIP_TRY(ctx, hipMemsetAsync(A.counters, 0, 2 * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_adaptive_mask, dim3((A.owned + 3u) / 4u), dim3(256), 0, ctx->stream, A);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t h[2] = {0, 0};  // listed tiles, active pixels
    HIP_TRY(ctx, hipMemcpyAsync(h, A.counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int const rc = checkErrorFlag(ctx)) return rc;  // the previous round lost or duplicated a fold
    if (h[0] == 0) break;
    uint32_t const n = std::min(step_spp, max_spp - offset);
    TileSelection const sel{A.list, A.mask, h[0]};
    if (int const rc = renderImpl(ctx, offset, n, G.x0, G.y0, G.x1, G.y1, nullptr, 0, &sel)) return rc;
    if (rounds) ++*rounds;
    if (samples) *samples += uint64_t(h[1]) * n;
    offset += n;
  }
  return DMT_OK;
}

// the two counting launches: `n` counters each
static int countingRender(dmt_ctx* ctx, char const* refusal, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1, uint64_t* stats, int n) {
  if (!ctx || !stats) return DMT_ERR_INVALID;
  if (ctx->accel != DMT_ACCEL_BVH) return fail(ctx, DMT_ERR_STATE, refusal);
  return renderImpl(ctx, sample_offset, spp, x0, y0, x1, y1, stats, n);
}
int dmt_render_stats(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1, uint64_t* stats6) {
  return countingRender(ctx, "dmt_render_stats: only the BVH path has device counters", sample_offset, spp, x0, y0, x1, y1, stats6, 6);
}
int dmt_render_profile(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1, uint64_t* stats16) {
  return countingRender(ctx, "dmt_render_profile: only the BVH path has device counters", sample_offset, spp, x0, y0, x1, y1, stats16, 16);
}

int dmt_sync(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return checkErrorFlag(ctx);
}

int dmt_sched_diag(dmt_ctx* ctx, uint64_t* out8, int reset) {
  if (!ctx || !out8) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long d[kSchedDiagWords] = {};
  if (int const rc = readSchedDiag(ctx, d)) return rc;
  for (int i = 0; i < 8; ++i) out8[i] = i < kSchedDiagWords ? d[i] : 0;
  out8[6] = ctx->launch.sched.expectedFolds;
  out8[7] = uint64_t(kSlabsPerWave);
  if (reset) {
    HIP_TRY(ctx, hipMemset(ctx->launch.sched.diag.get(), 0, sizeof(d)));  // (the GGX batching words too: read dmt_ggx_batch_diag first)
    ctx->launch.sched.expectedFolds = 0, ctx->launch.ggx.lostReported = 0;
  }
  return DMT_OK;
}

int dmt_set_ggx_batch(dmt_ctx* ctx, uint32_t batch) {
  if (!ctx) return DMT_ERR_INVALID;
  if (batch > kGgxQueueCap) return fail(ctx, DMT_ERR_INVALID, "dmt_set_ggx_batch: a batch is at most 64 hits (the queue's capacity)");
  ctx->launch.ggx.batchT = batch;
  return DMT_OK;
}

int dmt_ggx_batch_diag(dmt_ctx* ctx, uint64_t* out5) {
  if (!ctx || !out5) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long d[kSchedDiagWords] = {};
  if (int const rc = readSchedDiag(ctx, d)) return rc;
  out5[0] = d[SD_GGX_PARKED], out5[1] = d[SD_GGX_RESUMED], out5[2] = d[SD_GGX_PASSES], out5[3] = d[SD_GGX_FULL], out5[4] = ctx->launch.ggx.batchT;
  return DMT_OK;
}

int dmt_set_chunk(dmt_ctx* ctx, uint32_t samples_per_item) {
  if (!ctx) return DMT_ERR_INVALID;
  ctx->launch.chunkSpp = samples_per_item;
  return DMT_OK;
}

int dmt_set_sampler_table(dmt_ctx* ctx, int mode, uint64_t budget_bytes) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_SAMPLER_TABLE_OFF && mode != DMT_SAMPLER_TABLE_AUTO && mode != DMT_SAMPLER_TABLE_FORCE)
    return fail(ctx, DMT_ERR_INVALID, "dmt_set_sampler_table: unknown mode");
  ctx->launch.tab.mode = mode;
  ctx->launch.tab.budget = budget_bytes ? budget_bytes : kSamTabDefaultBudget;
  return DMT_OK;
}

int dmt_sampler_table_plan(int width, int height, uint64_t owned_pixels, uint32_t spp, uint32_t chunk_spp, uint64_t budget_bytes, int mode,
                           dmt_sampler_table_plan_record* out, uint32_t* slice_spp, uint32_t slice_cap) {
  if (!out || width <= 0 || height <= 0 || (slice_cap && !slice_spp)) return DMT_ERR_INVALID;
  if (mode != DMT_SAMPLER_TABLE_OFF && mode != DMT_SAMPLER_TABLE_AUTO && mode != DMT_SAMPLER_TABLE_FORCE) return DMT_ERR_INVALID;
  if (chunk_spp > spp) chunk_spp = spp;
  SamplerTablePlan const p = samplerTablePlan(width, height, owned_pixels, spp, chunk_spp, budget_bytes ? budget_bytes : kSamTabDefaultBudget, mode);
  *out = dmt_sampler_table_plan_record{};
  out->use = p.use ? 1 : 0, out->period_width = p.pw, out->period_height = p.ph, out->entry_bytes = kSamTabEntryBytes;
  if (!p.use) return DMT_OK;
  out->slices = p.slices;
  uint64_t const sliceSamples = uint64_t(p.sliceChunks) * chunk_spp;
  out->slice_bytes = std::min<uint64_t>(sliceSamples, spp) * p.pw * p.ph * kSamTabEntryBytes;
  for (uint32_t k = 0; k < p.slices && k < slice_cap; ++k)
    slice_spp[k] = uint32_t(std::min<uint64_t>(sliceSamples, spp - k * sliceSamples));
  return DMT_OK;
}

int dmt_set_bvh_strategy(dmt_ctx* ctx, int strategy, uint64_t paths_per_pass) {
  if (!ctx) return DMT_ERR_INVALID;
  if (strategy < 0 || strategy > 2) return fail(ctx, DMT_ERR_INVALID, "dmt_set_bvh_strategy: 0 = automatic, 1 = megakernel, 2 = wavefront");
  ctx->launch.wf.strategy = strategy;
  if (paths_per_pass) ctx->launch.wf.targetPaths = size_t(paths_per_pass);
  return DMT_OK;
}

int dmt_set_partition(dmt_ctx* ctx, int rank, int world) {
  if (!ctx) return DMT_ERR_INVALID;
  if (world < 1 || rank < 0 || rank >= world) return fail(ctx, DMT_ERR_INVALID, "dmt_set_partition: bad rank/world");
  ctx->launch.rank = rank, ctx->launch.world = world;
  return DMT_OK;
}

int dmt_kernel_time(dmt_ctx* ctx, double* total_ms, uint64_t* launches, int reset) {
  if (!ctx) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int const rc = checkErrorFlag(ctx)) return rc;  // a time measured on an invalid film is not reported
  LaunchState::Timing& T = ctx->launch.timing;
  for (size_t i = 0; i < T.used; ++i) {
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, T.events[i].first, T.events[i].second));
    T.ms += double(ms);
    ++T.launches;
  }
  T.used = 0;
  if (total_ms) *total_ms = T.ms;
  if (launches) *launches = T.launches;
  if (reset) T.ms = 0.0, T.launches = 0;
  return DMT_OK;
}

int dmt_kernel_info(dmt_ctx* ctx, int* vgprs, int* sgprs, int* lds_bytes, int* blocks_per_cu, int* cu_count) {
  if (!ctx) return DMT_ERR_INVALID;
  uint32_t F = 0;  // facts of the kernel dmt_render would launch now
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  MegakernelFn const kernel = megakernelOf(F);
  if (!kernel) return noKernel(ctx, "dmt_kernel_info", F);
  hipFuncAttributes attr{};
  HIP_TRY(ctx, hipFuncGetAttributes(&attr, reinterpret_cast<void const*>(kernel)));
  if (vgprs) *vgprs = attr.numRegs;
  if (sgprs) *sgprs = 0;
  if (lds_bytes) *lds_bytes = int(attr.sharedSizeBytes);
  if (blocks_per_cu) *blocks_per_cu = blocksPerCuOf(ctx, kernel);
  if (cu_count) *cu_count = ctx->launch.cuCount;
  return DMT_OK;
}

// scratch (private segment) bytes per lane of the kernel dmt_render would launch now: 0 = no register spills, no stack
int dmt_kernel_scratch(dmt_ctx* ctx, int* scratch_bytes) {
  if (!ctx || !scratch_bytes) return DMT_ERR_INVALID;
  uint32_t F = 0;
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  MegakernelFn const kernel = megakernelOf(F);
  if (!kernel) return noKernel(ctx, "dmt_kernel_scratch", F);
  hipFuncAttributes attr{};
  HIP_TRY(ctx, hipFuncGetAttributes(&attr, reinterpret_cast<void const*>(kernel)));
  *scratch_bytes = int(attr.localSizeBytes);
  return DMT_OK;
}

}  // extern "C"
