// launch_device.hpp -- the device side of the launch layer: how the waves of a megakernel launch pick up, trace, complete and
// fold work items (sample chunk x tile item), with the staging slabs and hand-over words that keep the film an ordered fold.
// The layer's state is in launch_state.hpp, its helpers and entry points in launch_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once, inside its anonymous namespace, between the sample preparation and
// the GGX batching code: it uses KArgs, PathState, Sampler and the film helpers of pt_device.hpp, and megakernel_body(_bvh)
// and ggx_park / ggx_resume use what it defines.  The host reads kMaxChunkSpp, kSlabsPerWave, kSchedDiagWords and the SD_* words.
#pragma once

#ifndef DMT_MIN_WAVES_PER_SIMD
#define DMT_MIN_WAVES_PER_SIMD 4
#endif
#ifndef DMT_MIN_WAVES_PER_SIMD_BVH
#define DMT_MIN_WAVES_PER_SIMD_BVH 3
#endif
constexpr uint32_t kMaxChunkSpp = 512;  // staging: 384 KB per slab at most
#ifndef DMT_SLABS_PER_WAVE
#define DMT_SLABS_PER_WAVE 4
#endif
constexpr int kSlabsPerWave = DMT_SLABS_PER_WAVE;  // staging slabs per wave: two live items + two handed over
#ifndef DMT_PREP_THRESHOLD
#define DMT_PREP_THRESHOLD 64
#endif
struct TileArgs {  // what a wave needs when it picks up a new work item
  float4* mean;
  float4* m2;
  uint32_t* counter;
  int width, x0, y0, x1, y1, tx0, ty0, rtx;
  uint32_t numItems, subShift, sampleOffset, spp, chunkSpp, numChunks;
  uint32_t* link;
  uint32_t* slabBusy;
  float* stage;
  int rank, world;
};
DMT_DEV TileArgs load_tile_args(KArgs k) {
  k = kargs(k);
  TileArgs t;
  t.mean = k->mean, t.m2 = k->m2, t.counter = k->counter, t.width = k->width;
  t.x0 = k->x0, t.y0 = k->y0, t.x1 = k->x1, t.y1 = k->y1, t.tx0 = k->tx0, t.ty0 = k->ty0, t.rtx = k->rtx;
  t.numItems = k->numItems, t.subShift = k->subShift, t.sampleOffset = k->sampleOffset, t.spp = k->spp, t.rank = k->rank, t.world = k->world;
  t.chunkSpp = k->chunkSpp, t.numChunks = k->numChunks, t.link = k->link, t.slabBusy = k->slabBusy, t.stage = k->stage;
  return t;
}

// ---- work items ------------------------------------------------------------------------------------
// Work item = (sample chunk c, owned tile t), handed out chunk-major from one atomic counter: all tiles
// of chunk 0, then chunk 1, ...  An item is n samples x 64 pixels = up to 64 n UNITS (pixel, sample).
//
// * Lanes are not tied to pixels.  A lane that needs work takes the item's next unit (wave-wide ballot +
//   prefix count on a wave-uniform cursor; unit u -> pixel u mod 64, sample u div 64, so a batch of 64
//   requests is one sample of every pixel).  Path lengths differ between pixels (glass vs wall) and between
//   samples; with lane == pixel every item ran at the pace of its slowest pixel, now the wave stays full
//   until the item runs out of units.
// * A finished sample's radiance goes to one of the wave's kSlabsPerWave staging SLABS in global memory
//   ([sample][pixel] float3, written through so that any wave can read it back).  The film is the reference's
//   Welford update (SMEMLayout::updateSample, T/megakernel/megakernel.cuh:59-79) applied to a pixel's samples
//   IN INDEX ORDER, so chunk c of a tile must be folded after chunk c-1 -- while chunks c and c+1 are traced
//   CONCURRENTLY by different waves (a small frame, or one GPU's share of a frame split eight ways, still fills
//   the machine).  Nobody waits for that order; the fold is HANDED OVER instead (item_complete):
//     - every (chunk, tile) has one hand-over word `link`, zero at launch.  Exactly two parties touch it, each
//       with ONE atomic exchange: the wave that finishes tracing chunk c writes "slab + 1", the wave that has
//       put chunk c-1 into the film writes kFoldReady.  Exchanges on one word are totally ordered, so exactly
//       one of the two sees the other's value, and that one folds chunk c: the finisher if the predecessor was
//       already in the film, else the predecessor's folder, which then goes on to chunk c+1 the same way
//       (fold_chain).  Chunk 0 is folded by its finisher.
//     - a slab that was handed over stays busy until its folder clears `slabBusy`; its owner meanwhile uses
//       another of its slabs.
//   The film is therefore bit-identical for every chunk size and schedule, and no wave ever spins on another
//   wave's progress while it holds work: the only wait left is a wave with NO live item whose slabs are all
//   handed over and not folded yet (sched_retire) -- it holds nothing anybody needs, polls for a bounded wall
//   clock time and then EXITS (the remaining items are fetched by the other waves; counted in schedDiag).
//   Round 2's protocol had the finisher spin on a per-tile completion counter instead.  That is deadlock-free
//   only if every wave that has fetched an item keeps running; it gave up (error flag, 71 s per step) when four
//   processes' persistent kernels shared one GPU (DESIGN.md 7 has the record).
// * A wave holds up to TWO live items (sequence numbers cur and cur+1, LDS slots seq & 1): when item cur has
//   no units left, free lanes draw from item cur+1 (fetched at that moment) while the last paths of cur drain;
//   when cur's last sample is staged the wave completes it (lane i folds pixel i; whatever lane i is tracing
//   meanwhile stays in its registers).  Small items are therefore cheap, which keeps the end-of-launch tail
//   short when a frame is split over 8 GPUs.
__shared__ uint32_t s_desc[kLdsThreads / 64][2][8];  // per wave, per slot: chunk, tile item, px0, py0, s0, first float of the slab, nInside, slab
__shared__ int32_t s_pixbase[2 * kLdsThreads];       // per slot, per pixel: Halton pixel base, -1 = outside the region
__shared__ uint32_t s_pixmap[2 * kLdsThreads];       // per slot: j-th pixel inside the region

constexpr uint32_t kSlotBit = 0x80000000u;  // staging index = slot bit | (sample * 64 + pixel)
constexpr uint32_t kFoldReady = 0xFFFFFFFFu;  // link word: the tile's previous chunk is in the film
// The Halton index of the sample a lane is tracing (the *_medium rows: medium_device.hpp), from its staging index alone:
// slot, sample k of the chunk and pixel name the chunk's first sample (s_desc word 4) and the pixel's base index
// (s_pixbase), both of which outlive every sample of their item.  No state of its own: the brute-force rows have 32 bytes
// of LDS left per block at four blocks per CU.
DMT_DEV uint32_t medium_h(KArgs k, PathState const& st) {
  uint32_t const slot = st.sidx >> 31, ks = (st.sidx & ~kSlotBit) >> 6, pixel = st.sidx & 63u;
  k = kargs(k);
  int32_t const base = s_pixbase[slot * kLdsThreads + (threadIdx.x & ~63u) + pixel];
  return uint32_t(base + int32_t(s_desc[threadIdx.x >> 6][slot][4] + ks) * (k->sp.scale0 * k->sp.scale1));
}
#ifndef DMT_SLAB_WAIT_MS
#define DMT_SLAB_WAIT_MS 250  // a wave without a live item and without a free slab polls this long, then exits
#endif
constexpr int kSchedDiagWords = 12;  // folds, handed over, folded for another wave, stalls, early exits, max stall ticks; 8-11: GGX batching

// wave-level bookkeeping (all wave-uniform)
struct WaveSched {
  uint32_t cur = 0, fetched = 0;          // live items are [cur, fetched), at most two
  uint32_t alloc = 0;                     // item units are drawn from
  uint32_t nextUnit = 0, totalUnits = 0;  // cursor / size of item `alloc`
  bool exhausted = false;                 // the launch has no more items
  uint32_t slabFree = (1u << kSlabsPerWave) - 1u;  // own slabs that are free
  uint32_t slabPend = 0;                           // own slabs handed over, not known to be folded yet
};
// launch diagnostics (dmt_sched_diag; the host checks folds == items): one atomic per EVENT, from lane 0 -- an event is at
// most once per work item (~10^3 path samples), and counters kept in the wave's registers cost spills in the hot loop
enum { SD_FOLDS = 0, SD_HANDED = 1, SD_CHAINED = 2, SD_STALLS = 3, SD_EXITS = 4, SD_MAXSTALL = 5,
       SD_GGX_PARKED = 8, SD_GGX_RESUMED = 9, SD_GGX_PASSES = 10, SD_GGX_FULL = 11 };
DMT_DEV void sched_count(unsigned long long* D, int lane, int what, unsigned long long n = 1ull) {
  if (lane == 0) atomicAdd(&D[what], n);
}
// per-lane bookkeeping
struct LaneSched {
  bool prepared = false;  // a unit is waiting in s_prep
  bool prepSlot = false;  // ... of the item in this slot
};

// pixel origin and row count of a tile item (an owned tile is scheduled as 1 << subShift bands of 8 >> subShift
// rows: more, smaller items when this GPU has fewer tiles than resident waves; lanes beyond the band are "outside").
// Adaptive launches (tileList set; wave-uniform) take the tile from the list and keep only the lanes whose pixel bit is
// set in the tile's mask word: pixel (x, y) of the tile is bit y * 8 + x, so lane i of band b is bit b * rows * 8 + i.
// The two pointers are read from the kernel arguments here, not kept in TileArgs (SGPRs held across the hot loop).
struct ItemGeom {
  int px0, py0;
  uint32_t rows;
  unsigned long long live;  // bit i: lane i's pixel is traced (all ones without a tile list)
};
DMT_DEV ItemGeom item_geom(TileArgs const& T, uint32_t item) {
  uint32_t const band = item & ((1u << T.subShift) - 1u);
  uint32_t const rows = 8u >> T.subShift;
  uint32_t j;
  unsigned long long live = ~0ull;
  KArgs const k = kargs(kargs_base());
  if (uint32_t const* const list = k->tileList) {
    j = list[item >> T.subShift];
    live = kargs(k)->tileMask[j] >> (band * rows * 8u);
  } else {
    j = uint32_t(T.rank) + (item >> T.subShift) * uint32_t(T.world);
  }
  return {(T.tx0 + int(j % uint32_t(T.rtx))) * 8, (T.ty0 + int(j / uint32_t(T.rtx))) * 8 + int(band * rows), rows, live};
}
DMT_DEV bool item_lane_inside(TileArgs const& T, ItemGeom const& g, int lane) {
  int const px = g.px0 + (lane & 7), py = g.py0 + (lane >> 3);
  // (g.live is wave-uniform and bit i belongs to lane i: it IS the lane mask -- no per-lane shift, no VGPRs)
  return uint32_t(lane >> 3) < g.rows && px >= T.x0 && px < T.x1 && py >= T.y0 && py < T.y1 &&
         __builtin_amdgcn_inverse_ballot_w64(g.live);
}
DMT_DEV uint32_t chunk_samples(TileArgs const& T, uint32_t chunk) {
  uint32_t const s0 = chunk * T.chunkSpp;
  return s0 + T.chunkSpp < T.spp ? T.chunkSpp : T.spp - s0;
}

// index of this wave in the launch, as a value the compiler knows to be wave-uniform (gtid >> 6 lives in a VGPR; slab
// bookkeeping derived from it would be treated as divergent: VALU bit scans, exec-masked branches around item_fetch)
DMT_DEV uint32_t wave_index(uint32_t) { return blockIdx.x * (kLdsThreads / 64) + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6))); }

// which of the wave's handed-over slabs have been folded meanwhile?
DMT_DEV void slab_refresh(TileArgs const& T, uint32_t gtid, int lane, WaveSched& W) {
  if (W.slabPend == 0u) return;
  bool const mine = lane < kSlabsPerWave && ((W.slabPend >> lane) & 1u) != 0u;
  uint32_t busy = 1u;
  if (mine) busy = __hip_atomic_load(&T.slabBusy[wave_index(gtid) * kSlabsPerWave + uint32_t(lane)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t const freed = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(__ballot(mine && busy == 0u)))));
  W.slabFree |= freed, W.slabPend &= ~freed;
}

// fetch the next work item into slot seq & 1; false = the launch has no more items.  The caller has checked that the
// wave has a free slab (W.slabFree != 0; slab_refresh runs in sched_retire only, to keep it out of the hot loop).
DMT_DEV bool item_fetch(KArgs Pk, uint32_t gtid, int lane, uint32_t seq, WaveSched& W, uint32_t& units) {
  TileArgs const T = load_tile_args(Pk);
  uint32_t work = 0;
  if (lane == 0) work = atomicAdd(T.counter, 1u);
  work = uint32_t(__builtin_amdgcn_readfirstlane(int(work)));
  if (work >= T.numItems * T.numChunks) return false;
  uint32_t const slabK = uint32_t(__builtin_ctz(W.slabFree));
  W.slabFree &= ~(1u << slabK);
  uint32_t const chunk = work / T.numItems;
  uint32_t const item = work - chunk * T.numItems;
  ItemGeom const g = item_geom(T, item);
  int const px = g.px0 + (lane & 7), py = g.py0 + (lane >> 3);
  bool const inside = item_lane_inside(T, g, lane);
  uint32_t const s0 = T.sampleOffset + chunk * T.chunkSpp;
  uint32_t const n = chunk_samples(T, chunk);
  uint32_t const slot = seq & 1u;
  unsigned long long const insideMask = __ballot(inside);
  uint32_t const nInside = uint32_t(__popcll(insideMask));
  uint32_t* const d = s_desc[threadIdx.x >> 6][slot];  // wave-uniform values: every lane stores the same words
  d[0] = chunk, d[1] = item, d[2] = uint32_t(g.px0), d[3] = uint32_t(g.py0), d[4] = s0, d[6] = nInside;
  d[7] = wave_index(gtid) * kSlabsPerWave + slabK;
  d[5] = d[7] * T.chunkSpp * 192u;  // first float of the slab (< 2^32: at most 16 384 slabs of kMaxChunkSpp * 192 floats)
  uint32_t const wbase = slot * kLdsThreads + (threadIdx.x & ~63u);
  s_pixbase[wbase + lane] = inside ? halton_pixel_base(load_cold_args(Pk).sp, px, py) : -1;
  if (inside) s_pixmap[wbase + uint32_t(__popcll(insideMask & ((1ull << lane) - 1ull)))] = uint32_t(lane);
  units = nInside * n;
  return true;
}

// Staged radiance goes to the wave's slab with PLAIN stores (they merge in this XCD's L2; the owner folds its own slab
// from there).  Only when a slab is handed over is it made visible to the other XCDs (slab_publish).
DMT_DEV void stage_sample(KArgs Pk, uint32_t sidx, f3 L) {
  uint32_t const first = s_desc[threadIdx.x >> 6][sidx >> 31][5];
  float* const p = kargs(Pk)->stage + (first + (sidx & ~kSlotBit) * 3u);
  p[0] = L.x, p[1] = L.y, p[2] = L.z;
}
// Hand-over: the folder may run on another XCD, whose L2 is a different one, and this XCD's L2 holds the slab as dirty
// lines.  Writing back the whole L2 (release fence = buffer_wbl2) would cost far more than the slab is worth, so the
// owner re-stores its n x 64 x 3 floats with agent-scope stores (global_store ... sc1: written through to memory), lane i
// the samples of pixel i; the folder reads them with agent-scope loads.  48 loads + 48 stores per lane for 16 samples,
// paid only by chunks that finish before their predecessor (none on a frame with more tiles than resident waves).
DMT_DEV void slab_publish(TileArgs const& T, int lane, uint32_t slab, uint32_t n) {
  float* p = T.stage + size_t(slab) * size_t(T.chunkSpp) * 192u + uint32_t(lane) * 3u;
#pragma unroll 4
  for (uint32_t k = 0; k < n; ++k, p += 192) {
    float const x = p[0], y = p[1], z = p[2];
    uint32_t* const q = reinterpret_cast<uint32_t*>(p);
    __hip_atomic_store(q + 0, __float_as_uint(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, __float_as_uint(y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 2, __float_as_uint(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// prepare unit u of item `seq` in this lane's s_prep
template <bool MOTION = false, bool PROJ = true>
DMT_DEV void prepare_unit(KArgs Pk, uint32_t seq, uint32_t u, LaneSched& Ls) {
  uint32_t const slot = seq & 1u;
  uint32_t const* const d = s_desc[threadIdx.x >> 6][slot];
  uint32_t const nInside = d[6];
  uint32_t k, j;
  if (nInside == 64u) k = u >> 6, j = u & 63u;
  else k = u / nInside, j = u - k * nInside;
  uint32_t const wbase = slot * kLdsThreads + (threadIdx.x & ~63u);
  uint32_t const pixel = s_pixmap[wbase + j];
  prepare_sample<MOTION, PROJ>(Pk, int(d[2]) + int(pixel & 7u), int(d[3]) + int(pixel >> 3), s_pixbase[wbase + pixel], d[4] + k);
  s_prep[14 * kLdsThreads + threadIdx.x] = __uint_as_float((slot << 31) | (k * 64u + pixel));
  Ls.prepared = true, Ls.prepSlot = slot != 0u;
}

// Film words that another wave of this launch may read or have written (the tile's previous / next chunk) are
// moved with agent-scope relaxed atomics (global_load/store ... sc1: coherent across the XCDs' L2s) and
// ordered against the hand-over word by s_waitcnt.  The obvious alternative, plain accesses between
// acquire/release FENCES, costs a buffer_inv / buffer_wbl2 of the XCD's whole L2 per item.
DMT_DEV float4 film_load(float4 const* p) {
  unsigned long long const* const q = reinterpret_cast<unsigned long long const*>(p);
  unsigned long long const a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long const b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_float4(__uint_as_float(uint32_t(a)), __uint_as_float(uint32_t(a >> 32)), __uint_as_float(uint32_t(b)),
                     __uint_as_float(uint32_t(b >> 32)));
}
DMT_DEV void film_store(float4* p, float4 v) {
  unsigned long long* const q = reinterpret_cast<unsigned long long*>(p);
  __hip_atomic_store(q, (unsigned long long)__float_as_uint(v.x) | ((unsigned long long)__float_as_uint(v.y) << 32),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, (unsigned long long)__float_as_uint(v.z) | ((unsigned long long)__float_as_uint(v.w) << 32),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One sample into a pixel's running statistics: SMEMLayout::updateSample, T/megakernel/megakernel.cuh:59-79.  ONE function
// for every fold in this library (megakernel items, wavefront passes), so that every path to the film rounds alike.
DMT_DEV void welford_update(f3& mean, f3& M2, float& N, f3 L) {
  N = N + 1.0f;
  f3 const delta = L - mean;
  mean = mean + delta / N;
  f3 const delta2 = L - mean;
  M2 = M2 + delta * delta2;
}

// Put chunk `chunk` of tile item `item` (staged in `slab`) into the film -- the caller knows that chunk - 1 is there --
// and then every directly following chunk that has already been handed over.  Lane i folds pixel i of the tile.
DMT_DEV void fold_chain(TileArgs const& T, unsigned long long* D, uint32_t gtid, int lane, uint32_t item, uint32_t chunk, uint32_t slab) {
  ItemGeom const g = item_geom(T, item);
  bool const inside = item_lane_inside(T, g, lane);
  size_t const pidx = size_t(g.px0 + (lane & 7)) + size_t(g.py0 + (lane >> 3)) * size_t(T.width);
  f3 mean = mk3(0, 0, 0), M2 = mk3(0, 0, 0);
  float N = 0.f;
  uint32_t folded = 0;
  if (inside) {
    float4 const m = film_load(T.mean + pidx);  // SMEMLayout::startSample, megakernel.cuh:45-57
    float4 const v = film_load(T.m2 + pidx);
    mean = mk3(m.x, m.y, m.z), M2 = mk3(v.x, v.y, v.z), N = v.w;
  }
  for (;;) {
    uint32_t const n = chunk_samples(T, chunk);
    bool const own = slab / kSlabsPerWave == wave_index(gtid);  // wave-uniform
    float const* p = T.stage + size_t(slab) * size_t(T.chunkSpp) * 192u + uint32_t(lane) * 3u;
    if (inside) {
      if (own) {
#pragma unroll 4
        for (uint32_t k = 0; k < n; ++k, p += 192) welford_update(mean, M2, N, mk3(p[0], p[1], p[2]));
      } else {  // another wave's slab: read it where it was written through to
#pragma unroll 2
        for (uint32_t k = 0; k < n; ++k, p += 192) {
          uint32_t const* const q = reinterpret_cast<uint32_t const*>(p);
          uint32_t const x = __hip_atomic_load(q + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          uint32_t const y = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          uint32_t const z = __hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          welford_update(mean, M2, N, mk3(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z)));
        }
      }
      film_store(T.mean + pidx, make_float4(mean.x, mean.y, mean.z, 0.f));  // endSample, megakernel.cuh:81-85
      film_store(T.m2 + pidx, make_float4(M2.x, M2.y, M2.z, N));
    }
    ++folded;
    if (++chunk == T.numChunks) {  // (a foreign slab of the last chunk still has to be released)
      if (!own) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(&T.slabBusy[slab], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      break;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // slab read, film stores written through -> release the slab, publish
    uint32_t next = 0;
    if (lane == 0) {
      if (!own) __hip_atomic_store(&T.slabBusy[slab], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      next = __hip_atomic_exchange(&T.link[size_t(chunk) * T.numItems + item], kFoldReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    next = uint32_t(__builtin_amdgcn_readfirstlane(int(next)));
    if (next == 0u) break;  // chunk not finished yet: its finisher will find kFoldReady and fold it
    slab = next - 1u;       // finished and handed over: this wave folds it (the running statistics are in registers)
  }
  sched_count(D, lane, SD_FOLDS, folded);
  if (folded > 1u) sched_count(D, lane, SD_CHAINED, folded - 1u);
}

// Item `seq` of this wave is completely staged: fold it, or hand it over to the folder of the tile's previous chunk.
DMT_DEV void item_complete(KArgs Pk, uint32_t gtid, int lane, uint32_t seq, WaveSched& W) {
  TileArgs const T = load_tile_args(Pk);
  uint32_t const* const d = s_desc[threadIdx.x >> 6][seq & 1u];
  uint32_t const chunk = uint32_t(__builtin_amdgcn_readfirstlane(int(d[0])));
  uint32_t const item = uint32_t(__builtin_amdgcn_readfirstlane(int(d[1])));
  uint32_t const slab = uint32_t(__builtin_amdgcn_readfirstlane(int(d[7])));
  uint32_t const slabBit = 1u << (slab - wave_index(gtid) * kSlabsPerWave);
  if (chunk > 0u) {
    // Is the previous chunk in the film already (the usual case when the frame has more tiles than resident waves)?
    // Then this wave folds, and nothing has to be published.  A stale "no" only costs an unnecessary publish.
    uint32_t seen = 0;
    if (lane == 0) seen = __hip_atomic_load(&T.link[size_t(chunk) * T.numItems + item], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen = uint32_t(__builtin_amdgcn_readfirstlane(int(seen)));
    if (seen != kFoldReady) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own staging stores have landed (in this XCD's L2)
      slab_publish(T, lane, slab, chunk_samples(T, chunk));
      if (lane == 0) __hip_atomic_store(&T.slabBusy[slab], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slab is in memory and marked busy -> offer it
      uint32_t old = 0;
      if (lane == 0) old = __hip_atomic_exchange(&T.link[size_t(chunk) * T.numItems + item], slab + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      old = uint32_t(__builtin_amdgcn_readfirstlane(int(old)));
      if (old != kFoldReady) {  // the previous chunk is not in the film yet: its folder takes this slab
        W.slabPend |= slabBit;
        sched_count(kargs(Pk)->schedDiag, lane, SD_HANDED);
        return;
      }
    }  // (kFoldReady seen or received: nobody else touches this word any more)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own staging stores have landed
  fold_chain(T, kargs(Pk)->schedDiag, gtid, lane, item, chunk, slab);
  W.slabFree |= slabBit;
}

// Hand the next units of the wave's items to the lanes that ask for one (`want`) and prepare them.  This is the ONE place
// where work items are fetched (item_fetch is large, and the kernel already fills most of the instruction cache): a wave
// starts with no item, and a wave whose last live item was retired comes here because all its lanes are starving.
template <bool MOTION = false, bool PROJ = true>
DMT_DEV void sched_draw(KArgs Pk, uint32_t gtid, int lane, WaveSched& W, LaneSched& Ls, bool want) {
  if (__builtin_expect(W.nextUnit == W.totalUnits, 0)) {  // the item units are drawn from is used up (or there is none yet): fetch the next if there is room
    if (!W.exhausted && W.fetched - W.cur < 2u && W.slabFree != 0u) {
      uint32_t units = 0;
      if (item_fetch(Pk, gtid, lane, W.fetched, W, units)) W.alloc = W.fetched, ++W.fetched, W.nextUnit = 0, W.totalUnits = units;
      else W.exhausted = true;
    }
  }
  uint32_t const avail = W.totalUnits - W.nextUnit;
  if (avail == 0u) return;
  unsigned long long const m = __ballot(want);
  uint32_t const rank = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
  uint32_t const cnt = uint32_t(__popcll(m));
  if (want && rank < avail) prepare_unit<MOTION, PROJ>(Pk, W.alloc, W.nextUnit + rank, Ls);
  W.nextUnit += cnt < avail ? cnt : avail;
}

// item cur: all units drawn and none of them still in a lane -> complete it; false = the wave leaves the launch
DMT_DEV bool sched_retire(KArgs Pk, uint32_t gtid, int lane, WaveSched& W) {
  item_complete(Pk, gtid, lane, W.cur, W);
  ++W.cur;
  if (W.slabPend != 0u) slab_refresh(load_tile_args(Pk), gtid, lane, W);  // once per completed item: which handed-over slabs are back?
  if (W.cur == W.fetched) {  // no live item: the next sched_draw fetches one
    if (W.exhausted) return false;
    if (W.slabFree == 0u) {
      // Every slab of this wave is handed over and waits for a folder.  The wave holds nothing anybody needs; in a
      // healthy launch a slab comes back within one item's tracing time.  Poll for a bounded WALL CLOCK time, then leave:
      // the other waves fetch the remaining items, and a free wave slot lets a switched-out wave run again.
      TileArgs const T = load_tile_args(Pk);
      unsigned long long* const D = kargs(Pk)->schedDiag;
      sched_count(D, lane, SD_STALLS);
      unsigned long long const t0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz
      unsigned long long waited = 0;
      do {
        __builtin_amdgcn_s_sleep(64);
        slab_refresh(T, gtid, lane, W);
        waited = __builtin_amdgcn_s_memrealtime() - t0;
      } while (W.slabFree == 0u && waited <= (unsigned long long)(DMT_SLAB_WAIT_MS) * 100000ull);
      if (lane == 0) atomicMax(&D[SD_MAXSTALL], waited);
      if (W.slabFree == 0u) {
        sched_count(D, lane, SD_EXITS);
        return false;
      }
    }
  }
  return true;
}
// does this lane still hold a sample of the item in slot `curSlot`?
DMT_DEV bool lane_holds(PathState const& st, LaneSched const& Ls, bool curSlot) {
  return (st.active && ((st.sidx >> 31) != 0u) == curSlot) || (Ls.prepared && Ls.prepSlot == curSlot) ||
         (st.finPending && ((get_finIdx() >> 31) != 0u) == curSlot);
}
