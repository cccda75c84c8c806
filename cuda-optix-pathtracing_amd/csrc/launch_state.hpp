// launch_state.hpp -- what a context keeps for the launch layer: how a dmt_render* call becomes work on the device.  The
// scheduler's buffers and fold accounting, the GGX batching queues, the sampler table and its plan, the adaptive rounds'
// tile lists, the wavefront form's buffers, the event pairs of dmt_kernel_time, and the settings that shape a launch.  The
// layer's device code is in launch_device.hpp (wavefront.hpp), its helpers and entry points in launch_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, kSchedDiagWords, kGgxQueueCap,
// DMT_GGX_BATCH_T and the DMT_SAMPLER_TABLE_* modes.
//
// Buffers.  allocate() makes the two that every launch reads, zeroed: sched.counter and sched.diag.  Every other buffer is
// grown on demand (DevBuf::reserve: never shrunk, contents not kept) by the call that needs it, so a context that has seen a
// large launch serves every smaller one without allocating:
//
//   buffer                          grown by                          zeroed
//   sched.counter                   allocate()                        on the stream, per launch and per table slice
//   sched.words                     growLaunchBuffers                 on the stream, per launch and per table slice
//   sched.stage                     growLaunchBuffers                 never: a slab is written before it is read
//   sched.stats                     armStats (the counting launches)  on the stream, per counting launch
//   sched.diag                      allocate()                        dmt_sched_diag(reset) only: it accumulates over launches
//   ggx.queue                       growLaunchBuffers, for the row    never: a queue is read only as far as it was written
//                                   that parks hits
//   tab.vals, tab.jit, tab.lens     growLaunchBuffers, for a launch   never: k_sampler_table fills a slice before the
//                                   with a table (lens: with a lens)  megakernel reads it
//   adaptive.mask, .list            dmt_render_adaptive               never: k_adaptive_mask writes what a round reads
//   adaptive.count                  dmt_render_adaptive               on the stream, per round
//   wf.state, wf.queue, wf.counts   launchWavefront                   counts: on the stream, per pass
//
// Settings are sticky: each holds until its setter is called again, across uploads, launches of every kind and refused
// calls.  fromEnv() seeds five of them at context creation:
//
//   setting                   setter                  environment variable
//   wf.strategy               dmt_set_bvh_strategy    DMT_BVH_STRATEGY (0 automatic, 1 megakernel, 2 wavefront; else 0)
//   wf.targetPaths            dmt_set_bvh_strategy    DMT_WF_PATHS (>= 4096)
//   tab.mode                  dmt_set_sampler_table   DMT_SAMPLER_TABLE (0 off, 2 force, else automatic)
//   tab.budget                dmt_set_sampler_table   --
//   ggx.batchT                dmt_set_ggx_batch       DMT_GGX_BATCH (<= 0 off; at most the queue's capacity)
//   subShift                  --                      DMT_SUB_SHIFT (< 0 automatic; at most 2)
//   chunkSpp                  dmt_set_chunk           --
//   rank, world               dmt_set_partition       --
//
// dmt_sched_diag(reset) zeroes sched.diag (the GGX batching words with it) and with it sched.expectedFolds and
// ggx.lostReported, the host's two views of those words; nothing else.  dmt_kernel_time folds the used event pairs into
// timing.ms / timing.launches and, with reset, zeroes those two.
#pragma once

namespace {

// ---- sampler table: the host's plan ----------------------------------------------------------------
constexpr uint32_t kSamTabEntryBytes = 40;                  // 8 dimension values (two float4) + the film jitter (one float2)
constexpr uint32_t kSamTabLensEntryBytes = 48;              // launches with a lens: + the lens values (one float2)
constexpr uint64_t kSamTabDefaultBudget = 512ull << 20;
// Automatic mode uses the table when the launch's owned pixels are at least this many periods: the fill costs one
// period's worth of sampler arithmetic per sample, the compute path `ratio` periods' worth, so the table saves
// (1 - 1/ratio) of it and pays three loads per prepared sample.  Measured on Cornell frames of 2 048 spp, table forced
// against off: ratio 1 (128 x 128) +10.7 %, 1.56 +3.1 %, 2.25 -2.7 %, 4 (256 x 256) -9.5 %, 9 -15.7 %, 16 -16.7 %
// ("Sampler table").  The break-even is near 2; 4 keeps a margin for launches that own only part of their
// tiles' pixels (regions off the tile grid) and for every committed workload it is a gain.
constexpr uint64_t kSamTabMinRatio = 4;
struct SamplerTablePlan {
  bool use = false;
  uint32_t pw = 0, ph = 0;      // the frame's Halton period in pixels: min(width, 128) x min(height, 128)
  uint32_t slices = 0;          // fill + megakernel pairs of the call
  uint32_t sliceChunks = 0;     // sample chunks per slice (the last slice has what is left)
};
// Pure host arithmetic (dmt_sampler_table_plan exposes it).  chunkSpp: samples per work item of the launch, <= spp.
SamplerTablePlan samplerTablePlan(int width, int height, uint64_t ownedPixels, uint32_t spp, uint32_t chunkSpp, uint64_t budget, int mode,
                                  uint32_t entryBytes = kSamTabEntryBytes) {
  SamplerTablePlan p;
  if (width <= 0 || height <= 0) return p;
  p.pw = uint32_t(width < 128 ? width : 128), p.ph = uint32_t(height < 128 ? height : 128);
  if (mode == DMT_SAMPLER_TABLE_OFF || spp == 0 || chunkSpp == 0) return p;
  if (chunkSpp > spp) chunkSpp = spp;
  uint64_t const period = uint64_t(p.pw) * p.ph;
  if (mode != DMT_SAMPLER_TABLE_FORCE && ownedPixels < kSamTabMinRatio * period) return p;
  uint64_t const chunkEntries = uint64_t(chunkSpp) * period;
  uint64_t maxChunks = budget / (chunkEntries * entryBytes);
  uint64_t const maxChunksByIndex = 0x7FFFFFFFull / chunkEntries;  // entry indices are 32-bit on the device
  if (maxChunks > maxChunksByIndex) maxChunks = maxChunksByIndex;
  if (maxChunks == 0) return p;  // not even one chunk fits: the launch computes its samples
  uint64_t const numChunks = (uint64_t(spp) + chunkSpp - 1) / chunkSpp;
  uint64_t const k = (numChunks + maxChunks - 1) / maxChunks;
  p.sliceChunks = uint32_t((numChunks + k - 1) / k);  // equal chunk counts, <= maxChunks
  p.slices = uint32_t((numChunks + p.sliceChunks - 1) / p.sliceChunks);
  p.use = true;
  return p;
}

struct LaunchState {
  // the work-item scheduler (launch_device.hpp) and the fold accounting dmt_sync checks
  struct Sched {
    DevBuf<uint32_t> counter, words;        // the work counter; [waves * kSlabsPerWave] slab-busy marks, then [numChunks][numItems] hand-over words
    DevBuf<unsigned long long> diag;        // kSchedDiagWords counters over all launches (dmt_sched_diag)
    unsigned long long expectedFolds = 0;   // work items launched so far: what diag[SD_FOLDS] must read once the stream has drained
    DevBuf<float> stage;                    // staging slabs of finished samples, [wave][kSlabsPerWave][chunkSpp][64] float3
    DevBuf<unsigned long long> stats;       // 16 device counters of dmt_render_stats / dmt_render_profile
  } sched;
  // GGX batching (ggx_park / ggx_resume)
  struct Ggx {
    DevBuf<float> queue;                    // the queues of parked hits, [wave][kGgxFields][kGgxQueueCap]
    uint32_t batchT = DMT_GGX_BATCH_T;      // 0 = off
    unsigned long long lostReported = 0;    // parked - taken back that checkErrorFlag has reported already (0 in a healthy context)
  } ggx;
  // sampler table of a launch (samplerTablePlan, k_sampler_table): refilled by every dmt_render call that uses it
  struct Table {
    DevBuf<float4> vals;
    DevBuf<float2> jit, lens;               // (lens: launches with a lens only)
    int mode = DMT_SAMPLER_TABLE_AUTO;
    uint64_t budget = kSamTabDefaultBudget;  // bytes of table memory a launch may use; larger tables are filled in sample slices
  } tab;
  // dmt_render_adaptive: per tile of the film's tile grid a mask word, the list of tiles with active pixels, two counters
  struct Adaptive {
    DevBuf<unsigned long long> mask;
    DevBuf<uint32_t> list, count;
  } adaptive;
  // wavefront form of the BVH path (wavefront.hpp)
  struct Wavefront {
    int strategy = 0;                       // 0 = automatic (by launch size), 1 = megakernel, 2 = wavefront
    size_t targetPaths = size_t(1) << 22;   // path slots per pass
    DevBuf<float> state;
    DevBuf<uint32_t> queue, counts;         // two queues; counts + cursors
    int blocksTrace = 0, blocksShade = 0;   // resident blocks per CU of the trace and shade kernels (0: not asked yet)
  } wf;
  // one event pair around every timed launch since the last dmt_kernel_time
  struct Timing {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    double ms = 0.0;
    uint64_t launches = 0;
  } timing;
  // the shape of a launch
  uint32_t chunkSpp = 0;                    // samples per work item, 0 = automatic
  int subShift = -1;                        // row bands per tile (log2); -1 = choose per launch
  int rank = 0, world = 1;                  // the tiles of a region this context renders: tile j with j % world == rank
  int cuCount = 0;
  std::vector<std::pair<void const*, int>> occupancy;  // megakernel variant -> resident 256-thread blocks per CU

  // the settings the environment seeds at context creation (the table above): experiments, A/B runs and tests
  void fromEnv() {
    auto env = [](char const* name, long long& v) {
      char const* const e = std::getenv(name);
      if (e) v = std::atoll(e);
      return e != nullptr;
    };
    long long v = 0;
    if (env("DMT_BVH_STRATEGY", v)) wf.strategy = v < 0 || v > 2 ? 0 : int(v);
    if (env("DMT_WF_PATHS", v) && v >= 4096) wf.targetPaths = size_t(v);
    if (env("DMT_SAMPLER_TABLE", v)) tab.mode = v == 0 ? DMT_SAMPLER_TABLE_OFF : v == 2 ? DMT_SAMPLER_TABLE_FORCE : DMT_SAMPLER_TABLE_AUTO;
    if (env("DMT_GGX_BATCH", v)) ggx.batchT = v <= 0 ? 0u : uint32_t(std::min<long long>(v, kGgxQueueCap));
    if (env("DMT_SUB_SHIFT", v)) subShift = v < 0 ? -1 : (v > 2 ? 2 : int(v));  // (results do not depend on it)
  }

  // the two buffers every launch reads, zeroed (dmt_ctx_create, on the context's device)
  hipError_t allocate() {
    hipError_t e = sched.counter.reserve(2);
    if (e == hipSuccess) e = hipMemset(sched.counter.get(), 0, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = sched.diag.reserve(kSchedDiagWords);
    if (e == hipSuccess) e = hipMemset(sched.diag.get(), 0, kSchedDiagWords * sizeof(unsigned long long));
    return e;
  }
};

}  // namespace
