// dmt_hip.hip -- gfx950 megakernel + C ABI (include/dmt_hip.h).
//
// Kernel design (MI355X-first, not a translation of T/megakernel/megakernel.cu):
//   * work item = one 8x8-pixel tile x all samples of the pass; waves pull items from a global
//     atomic counter (persistent threads + work stealing) instead of a static grid-stride loop;
//   * one lane = one pixel; when a lane's path ends it folds the radiance into its Welford
//     registers and immediately regenerates the next sample of the same pixel, so a wave never
//     waits for its longest path (the reference reconverges the warp after every sample);
//   * everything the reference does between two ray casts (BSDF prepare, light sample, NEE
//     weight, BSDF sample, Russian roulette) is evaluated BEFORE the shadow ray is traced, so the
//     shadow ray of bounce k and the closest-hit ray of bounce k+1 go through ONE pass over the
//     triangle array: two independent Moeller-Trumbore chains per lane (ILP) and each triangle is
//     fetched once.  Radiance is still accumulated in the reference's order.
//   * brute-force mode keeps the reference's "loop over every triangle" semantics: the loop
//     index is wave-uniform, so triangle records arrive through scalar loads (s_load_dwordx4)
//     and live in SGPRs -- no LDS or VGPR traffic in the hot loop.
//   * film state (mean, M2, N) stays in registers for the whole item; one 32-byte read and one
//     32-byte write per pixel per pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/dmt_hip.h"
#include "pt_device.hpp"
#include "medium.hpp"
#include "medium_grid.hpp"
#include "bvh_device.hpp"
#include "bvh_gpu_build.hpp"
#include "devbuf.hpp"
#include "envmap.hpp"
#include "light_tree.hpp"
#include "light_tree_ref.hpp"
#include "emitter_tree.hpp"
#include "cull_plan.hpp"

using namespace dmt;

namespace {

// Culled clusters of the brute-force pass: the record (CullCluster), the plan's limits and the host planners are in
// cull_plan.hpp; what follows is the device's view of a plan (brute_clusters).
constexpr uint32_t kCullGroup = 4;         // the device takes the clusters kCullGroup at a time
typedef uint32_t CullWords __attribute__((ext_vector_type(8)));  // a CullCluster's first eight words: b[0..5], box, count
struct CullRec {                           // 12 B, the block's LDS copy of what a compacted task needs
  uint32_t first, countSlot, magic;        // countSlot = count | slot << 16
};
struct CullView {
  TriIsect const* always;         // the triangles every ray is tested against; == scene.tris when clusterCount == 0
  uint32_t const* alwaysIdx;      // [alwaysCount] original index of always[i] (clusterCount > 0 only)
  CullCluster const* clusters;    // [kCullMaxClusters]
  float const* tri9;              // [9][kCullMaxTris] p0, e0, e1 of the culled triangles, field-major
  uint32_t alwaysCount, clusterCount;
};

struct VtxNormalRec;  // vnormals.hpp
struct OpacityRec;    // opacity.hpp

struct RenderParams {
  SceneView scene;
  CullView cull;
  BvhView bvh;
  CameraXf cam;
  SamplerParams sp;
  float4* __restrict__ mean;
  float4* __restrict__ m2;
  uint32_t* __restrict__ counter;
  int width, height;
  int x0, y0, x1, y1;     // pixel region
  int tx0, ty0, rtx;      // tile grid of the region: origin (in tiles) and tiles per row
  uint32_t numItems;      // owned tiles << subShift
  uint32_t subShift;      // an owned 8x8 tile is scheduled as 1 << subShift row bands (1, 2 or 4)
  int rank, world;
  uint32_t sampleOffset, spp;
  uint32_t chunkSpp;       // samples per work item
  uint32_t numChunks;      // ceil(spp / chunkSpp)
  float* stage;            // staging slabs of finished samples: [wave][kSlabsPerWave][chunkSpp][64] float3
  uint32_t* link;          // [numChunks][numItems] hand-over word of (chunk, tile): 0, kFoldReady or slab + 1 (item_complete)
  uint32_t* slabBusy;      // [wave][kSlabsPerWave] 1 while a handed-over slab waits for its folder
  // adaptive sampling (dmt_render_adaptive; both null otherwise): the launch's tiles are tileList[0 .. numItems >> subShift),
  // region tile indices (rank + k * world), and a lane renders its pixel only if the pixel's bit of tileMask[tile] is set
  uint32_t const* tileList;
  unsigned long long const* tileMask;
  unsigned long long* schedDiag;  // kSchedDiagWords counters, accumulated over launches (dmt_sched_diag)
  // sampler table of the launch (k_sampler_table; samTab null: prepare_sample computes): the sampler's values depend on
  // (px % 128, py % 128, sample) only, so they are tabulated once over the frame's period samTabPw x samTabPh for the
  // samples from samTabS0 on and shared by every pixel congruent modulo 128.  Key [sample - samTabS0][py & 127][px & 127].
  float4 const* samTab;      // two float4 per entry: the 8 dimension values
  float2 const* samTabJit;   // one float2 per entry: pixel2d, the film jitter
  float2 const* samTabLens;  // launches with a lens only: one float2 per entry, lens_values (u10, u11)
  uint32_t samTabS0, samTabPw, samTabPh;
  float camTail, lensD;      // camTail: non-zero when prepare_sample's cold tail has work (a lens, or a pixel filter the sampler table
                             // does not already carry); the lens radius itself is lensRad, below.  lensD: the focus distance
  int maxDepth;
  int shadeThreshold;         // BVH megakernel: shade when this many lanes of the wave have finished their rays (bvhShadeThreshold)
  EnvView env;                // A18 env map (w == 0: none); read by the *_env kernels only
  // SURVEY 8f-3 emissive triangles; read by the *_area kernels only
  uint32_t const* areaOf;     // [triCount] index into areaTri / areaLe, 0xFFFFFFFF = not emissive
  uint32_t const* areaTri;    // [areaCount] ORIGINAL triangle index
  float const* areaLe;        // [areaCount] rgb radiance
  uint32_t areaCount;
  // SURVEY 8f-1 image textures; read by the *_tex kernels only (layout: dmt_upload_textures)
  uint32_t const* texRgba;    // RGBA8 texels of every texture, back to back
  int32_t const* texDesc;     // [texture] {first texel, width, height}
  uint32_t const* matTex;     // [bsdf] {diffuse, roughness, normal texture or 0xFFFFFFFF, anisotropy as float bits}
  float const* triUv;         // [triangle] {u0, v0, u1, v1, u2, v2}
  LightTreeNode const* lightTree;  // light BVH over `lights` (light_tree.hpp); read by the *_ltree kernels only
  LightTreeRefNode const* lightTreeRef;  // the reference-semantics tree (light_tree_ref.hpp); read by the *_ltree2 kernels only
  unsigned long long* stats;  // stats build only: samples, closest rays, shadow rays, node visits, triangle tests, bounces
  // first-hit texture filtering (DMT_TEXFILTER_REFERENCE); read by the *_texf kernels only.  Camera footprint as
  // dmt_texture_footprint returns it, and the MIP levels above 0 of every texture (layout: buildMipChain)
  float texCfr[12];           // camera-from-render, row-major 3x4
  float texMinDx[3], texMinDy[3];  // smallest direction differentials, in the frame of the camera ray
  float texSppScale;          // max(1/8, 1/sqrt(frame spp))
  uint32_t const* texMip;     // RGBA8 texels of levels 1.. of every texture, back to back
  int32_t const* texMipDesc;  // [texture] {levels, first texel of level 1 in texMip}
  // motion blur (dmt_set_motion); read by the *_motion kernels only, which also get the motion tree in `bvh`.  Last, so that
  // no other field moves
  MotionView motion;
  // smooth shading (dmt_upload_vertex_normals): [triangle] three octahedral normals and a flags word; read by the *_vn
  // kernels only, at the hit.  After `motion`, so that no other field moves
  VtxNormalRec const* vtxNormals;
  // alpha cutouts (dmt_upload_opacity): [triangle] the cutout record and the cutoff in byte units; read by the *_cut kernels
  // only, at candidate hits.  After `vtxNormals`, so that no other field moves
  OpacityRec const* opacity;
  float opacityCutoff8;
  // GGX batching (dmt_set_ggx_batch; ggx_park / ggx_resume): the waves' queues of parked hits, [wave][kGgxFields][kGgxQueueCap],
  // and the batch size T (0: off, the queue is then not read).  Read by k_megakernel only.  After
  // `opacityCutoff8`, so that no other field moves
  uint32_t ggxBatchT;
  float* ggxQueue;
  // material kind per triangle (SurfaceState::Kind): bit i of word i >> 5 is set when ORIGINAL triangle i has a GGX material,
  // i.e. when ggx_park parks its hits.  Soups of at most 64 triangles carry the table in the arguments themselves
  // (triKindInline; triKindBits is then null), larger ones in device memory.  Read by k_megakernel only.  After `ggxQueue`, so
  // that no other field moves
  uint32_t const* triKindBits;
  uint32_t triKindInline[2];
  // the participating medium (dmt_set_medium; medium.hpp): sigmaT == 0 without one.  Read by the *_medium kernels only.
  // After `triKindInline`, so that no other field moves
  MediumParams medium;
  // its density grid (dmt_set_medium_grid; medium_grid.hpp): density == nullptr without one.  Read by the *_medium_grid
  // kernels only.  After `medium`, so that no other field moves
  MediumGridParams mediumGrid;
  // its spectrum (dmt_set_medium_spectrum; medium.hpp): read by the *_rgb kernels only, whose `medium.sigmaT` is the
  // reference channel's extinction.  After `mediumGrid`, so that no other field moves
  MediumSpectrumParams mediumSpectrum;
  // the emitter tree (dmt_set_emitter_sampling; emitter_tree.hpp) over `lights` and the emissive triangles: its nodes and, per
  // emitter, the bit trail of its leaf.  Read by the *_etree kernels only.  After `mediumSpectrum`, so that no other field moves
  EmitterNode const* emitterTree;
  EmitterTrail const* emitterTrails;
  // camera-side state read where a camera ray is made: the thin lens's radius (dmt_set_lens; 0: pinhole) and the pixel filter
  // (dmt_set_pixel_filter; filtKnots null: box 0.5, no warp).  After `emitterTrails`, so that no other field moves
  float lensRad, filtR;
  FilterBin const* filtKnots;
  // one-record light lists through the scalar path (LightState::uniformPath; DMT_UNIFORM_LIGHTS=0 at context creation clears
  // it): non-zero lets path_shade read lights[0] / infLights[0] by s_load where the pick runs over one record.  After
  // `filtKnots`, so that no other field moves
  uint32_t uniformLights;
  // the camera's projection (dmt_set_projection): projKind 0 is the perspective camera, projA the model's
  // host-made factor and projW x projH the film's size as floats (camera_ray_projection).  Read by prepare_sample's cold
  // tail, the feature pass and the probes.  After `uniformLights`, so that no other field moves
  int projKind;
  float projA, projW, projH;
};

// Per-lane state.  A lane carries (a) the path it is currently extending and (b) at most one
// pending shadow ray.  The shadow ray normally belongs to the current path, but when a path ends
// with its last shadow ray still untraced the lane parks that sample's radiance in Lfin and starts
// the NEXT sample at once: the old shadow ray and the new camera ray share the next triangle pass,
// and the parked sample is finalised (in order) right after it.
// All kernels that trace paths take a RenderParams as their FIRST by-value argument, i.e. at offset 0 of
// the kernarg segment.  Device code never touches that parameter object directly: it reads the fields it
// needs, where it needs them, through the kernarg pointer behind an opaque barrier (`kargs`).  Left to
// itself the compiler hoists all ~90 argument dwords to the top of the kernel and keeps them in SGPRs
// across the triangle loop; that overflows the 102-SGPR file and the spill code lands INSIDE the hot
// loop (measured: 97 ms -> 160 ms per launch).  An s_load from the scalar cache at the point of use
// costs nothing next to the ~2-3k instructions of a shading step.
typedef RenderParams const DMT_CONST_AS* KArgs;
DMT_DEV KArgs kargs_base() { return (KArgs)__builtin_amdgcn_kernarg_segment_ptr(); }
DMT_DEV KArgs kargs(KArgs p) {
  asm volatile("" : "+s"(p));
  return p;
}
DMT_DEV CameraExtra load_camera_extra(KArgs k) {  // at the point of use, like the cold arguments
  k = kargs(k);
  return CameraExtra{k->lensRad, k->lensD, k->filtKnots, k->filtR, k->projKind, k->projA, k->projW, k->projH};
}
DMT_DEV SceneView load_scene(KArgs k) {
  k = kargs(k);
  SceneView s;
  s.tris = k->scene.tris, s.post = k->scene.post, s.bsdfs = k->scene.bsdfs, s.lights = k->scene.lights;
  s.infLights = k->scene.infLights, s.triCount = k->scene.triCount, s.bsdfCount = k->scene.bsdfCount;
  s.lightCount = k->scene.lightCount, s.infLightCount = k->scene.infLightCount;
  return s;
}
DMT_DEV BvhView load_bvh(KArgs k) {
  k = kargs(k);
  BvhView b;
  b.nodes = k->bvh.nodes, b.pairs = k->bvh.pairs, b.overflow = k->bvh.overflow, b.overflowStride = k->bvh.overflowStride;
  return b;
}

DMT_DEV EnvView load_env(KArgs k) {
  k = kargs(k);
  EnvView e;
  e.func = k->env.func, e.cdf = k->env.cdf, e.rowInt = k->env.rowInt, e.mFunc = k->env.mFunc, e.mCdf = k->env.mCdf;
  e.rgb = k->env.rgb, e.mInt = k->env.mInt, e.w = k->env.w, e.h = k->env.h;
  e.qx = k->env.qx, e.qy = k->env.qy, e.qz = k->env.qz, e.qw = k->env.qw;
  return e;
}

// Diagnostic build only (make variant DEFS=-DDMT_SECTION_TIMING=1): wave-level shader-clock cycles spent in each section of
// the brute-force megakernel, summed over all waves; read back with dmt_diag_section_cycles (tools/diag_sections.py).
#ifndef DMT_SECTION_TIMING
#define DMT_SECTION_TIMING 0
#endif
#if DMT_SECTION_TIMING
__device__ unsigned long long g_sect[16];
__shared__ unsigned long long s_sectLast[kLdsThreads / 64];
__shared__ unsigned long long s_sectAcc[kLdsThreads / 64][16];
#endif
DMT_DEV void sect_mark(int i) {  // everything since the previous mark belongs to section i
#if DMT_SECTION_TIMING
  unsigned long long const now = __builtin_readcyclecounter();
  unsigned long long const m = __ballot(1);
  if (int(__ffsll((long long)m)) - 1 == int(threadIdx.x & 63u)) {
    uint32_t const w = threadIdx.x >> 6;
    s_sectAcc[w][i] += now - s_sectLast[w];
    s_sectLast[w] = now;
  }
#endif
}
struct PathState {
  RayPair rp;       // .x = current path's ray, .y = pending shadow ray
  f3 beta, L;
  int depth;
  bool lastT;
  bool active;      // has a closest-hit ray to trace
  bool hasShadow;   // shadow ray / smax / C valid
  bool finPending;  // the pending shadow ray belongs to the finished sample parked in Lfin
  float smax;
  Sampler rng;
  uint32_t sidx;    // where the current sample's radiance goes (staging index, megakernel only)
  float lastPdf;    // env-map kernels only: pdf / delta flag of the bounce that produced the current ray
  bool lastSpecular;
};
// GGX batching (k_megakernel): a lane that has just taken a parked hit back (ggx_resume) carries the
// path's depth as its complement, i.e. negative, until it shades (ggx_park puts it back).  Such a lane traces no closest
// ray in that pass: rp.d*.x is the hit's ray direction and rp.o*.x hold tri, bu, bv as bits.  No state of its own: a
// flag per lane cost the kernel a register.
DMT_DEV bool ggx_resumed(PathState const& st) { return st.depth < 0; }
// cold per-lane values in LDS, [field][thread]: pending NEE contribution C (0..2) and the parked
// radiance Lfin of a finished sample (3..5) with its staging index (6); each is touched once per ray pass at most
__shared__ float s_cold[7 * kLdsThreads];
DMT_DEV void put_C(f3 v) {
  float* const c = s_cold + threadIdx.x;
  c[0 * kLdsThreads] = v.x, c[1 * kLdsThreads] = v.y, c[2 * kLdsThreads] = v.z;
}
DMT_DEV f3 get_C() {
  float const* const c = s_cold + threadIdx.x;
  return mk3(c[0 * kLdsThreads], c[1 * kLdsThreads], c[2 * kLdsThreads]);
}
DMT_DEV void put_Lfin(f3 v) {
  float* const c = s_cold + threadIdx.x;
  c[3 * kLdsThreads] = v.x, c[4 * kLdsThreads] = v.y, c[5 * kLdsThreads] = v.z;
}
DMT_DEV f3 get_Lfin() {
  float const* const c = s_cold + threadIdx.x;
  return mk3(c[3 * kLdsThreads], c[4 * kLdsThreads], c[5 * kLdsThreads]);
}
// emitter-tree kernels only (kFeatEmitterTree): the surface vertex the current path ray left, position (0..2) and geometric
// normal (3..5) exactly as et_select saw them, for et_pmf when the ray hits an emissive triangle.  Written once per bounce,
// read once per emitter hit; an array of its own, so that only the kernels that use it allocate it
__shared__ float s_prev[6 * kLdsThreads];
DMT_DEV void put_prev_vertex(f3 p, f3 n) {
  float* const c = s_prev + threadIdx.x;
  c[0 * kLdsThreads] = p.x, c[1 * kLdsThreads] = p.y, c[2 * kLdsThreads] = p.z;
  c[3 * kLdsThreads] = n.x, c[4 * kLdsThreads] = n.y, c[5 * kLdsThreads] = n.z;
}
DMT_DEV void get_prev_vertex(f3& p, f3& n) {
  float const* const c = s_prev + threadIdx.x;
  p = mk3(c[0 * kLdsThreads], c[1 * kLdsThreads], c[2 * kLdsThreads]);
  n = mk3(c[3 * kLdsThreads], c[4 * kLdsThreads], c[5 * kLdsThreads]);
}
DMT_DEV void put_finIdx(uint32_t i) { s_cold[6 * kLdsThreads + threadIdx.x] = __uint_as_float(i); }
DMT_DEV uint32_t get_finIdx() { return __float_as_uint(s_cold[6 * kLdsThreads + threadIdx.x]); }
DMT_DEV f3 ray_dir(PathState const& st) { return mk3(st.rp.dx.x, st.rp.dy.x, st.rp.dz.x); }
DMT_DEV f3 ray_org(PathState const& st) { return mk3(st.rp.ox.x, st.rp.oy.x, st.rp.oz.x); }
DMT_DEV f3 shadow_dir(PathState const& st) { return mk3(st.rp.dx.y, st.rp.dy.y, st.rp.dz.y); }  // the pending shadow ray (set_shadow_ray)
DMT_DEV f3 shadow_org(PathState const& st) { return mk3(st.rp.ox.y, st.rp.oy.y, st.rp.oz.y); }
DMT_DEV void swap_rays(PathState& st) {  // path ray <-> pending shadow ray (megakernel_body_bvh)
  auto sw = [](v2f& p) { float const t = p.x; p.x = p.y, p.y = t; };
  sw(st.rp.ox), sw(st.rp.oy), sw(st.rp.oz), sw(st.rp.dx), sw(st.rp.dy), sw(st.rp.dz);
}
DMT_DEV void set_ray(PathState& st, f3 o, f3 d) {
  st.rp.ox.x = o.x, st.rp.oy.x = o.y, st.rp.oz.x = o.z;
  st.rp.dx.x = d.x, st.rp.dy.x = d.y, st.rp.dz.x = d.z;
}
DMT_DEV void set_shadow_ray(PathState& st, f3 o, f3 d) {
  st.rp.ox.y = o.x, st.rp.oy.y = o.y, st.rp.oz.y = o.z;
  st.rp.dx.y = d.x, st.rp.dy.y = d.y, st.rp.dz.y = d.z;
}

DMT_DEV void path_begin(PathState& st, CameraXf const& cam, SamplerParams const& sp, int px, int py,
                        int32_t pixBase, uint32_t s, CameraExtra const& extra) {
  int32_t const hidx = pixBase + int32_t(s) * (sp.scale0 * sp.scale1);
  st.rng.start(uint32_t(hidx));
  Ray const r = camera_ray_any(cam, sp, px, py, hidx, extra);
  set_ray(st, r.o, r.d);
  st.beta = mk3(1, 1, 1);
  st.L = mk3(0, 0, 0);
  st.depth = 0;
  st.lastT = false;
  st.active = true;
}

// Everything between two ray casts (T/megakernel/megakernel.cu:135-295).  Returns true when the
// path ends.  May leave a pending shadow ray (st.hasShadow) whose contribution st.C is added once
// visibility is known.
#include "surface_device.hpp"

template <bool CULL = true>
DMT_DEV void trace_pair_brute(KArgs k, PathState const& st, bool doC, bool doS, int& bestTri, float& bu, float& bv, bool& occluded);

#include "motion.hpp"
#include "vnormals.hpp"

// Optional parts of the path-tracing code, one bit each: the template argument F of path_shade, lane_finish, lane_step,
// megakernel_body(_bvh) and wf_shade_body.  featuresOf (host) computes a context's mask; DMT_MEGAKERNELS and
// DMT_WF_SHADE_KERNELS list the masks that have a kernel.
constexpr uint32_t kFeatBvh = 1u << 0;           // BVH traversal instead of the brute-force triangle pass
constexpr uint32_t kFeatStats = 1u << 1;         // per-lane work counters (dmt_render_stats; never on the timed path)
constexpr uint32_t kFeatEnv = 1u << 2;           // A18 env-map light
constexpr uint32_t kFeatArea = 1u << 3;          // SURVEY 8f-3 emissive triangles
constexpr uint32_t kFeatTex = 1u << 4;           // SURVEY 8f-1 image textures
constexpr uint32_t kFeatBlend = 1u << 5;         // image textures + fractional "metallic" (BS_GGX_BLEND record pairs)
constexpr uint32_t kFeatLightTree = 1u << 6;     // SURVEY 8f-4 light tree (light_tree.hpp)
constexpr uint32_t kFeatLightTreeRef = 1u << 7;  // the reference-semantics light tree (light_tree_ref.hpp)
constexpr uint32_t kFeatTexFilter = 1u << 8;     // first-hit MIP / EWA texture filtering; with kFeatTex or kFeatBlend only
constexpr uint32_t kFeatMotion = 1u << 9;        // motion blur: triangles at the sample's time (motion.hpp); plain and env-map rows only
constexpr uint32_t kFeatCutout = 1u << 11;       // alpha cutouts: candidate hits filtered by an opacity texture (opacity.hpp); the texture rows only
constexpr uint32_t kFeatVtxNormals = 1u << 10;   // smooth shading: ns interpolated from per-vertex normals (vnormals.hpp); plain, env, tex rows
constexpr uint32_t kFeatMedium = 1u << 12;       // participating medium: free flight and scatter vertices between two ray casts (medium_device.hpp); plain and env-map rows only
constexpr uint32_t kFeatMediumGrid = 1u << 13;   // the medium's extinction from a density grid, marched voxel by voxel (medium_grid.hpp); set together with kFeatMedium
constexpr uint32_t kFeatEmitterTree = 1u << 15;  // NEE picks among lights and emissive triangles by the emitter tree (emitter_tree.hpp); with kFeatArea, the four *_area rows only
constexpr uint32_t kFeatMediumSpectrum = 1u << 14;  // per-channel extinction and emission: one-sample MIS over the channels' free flights (medium.hpp); set together with kFeatMedium

// the post-hit record path_shade works on: the uploaded one, or under kFeatMotion the triangle at the sample's time
template <uint32_t F>
DMT_DEV Hit shade_hit(KArgs k, SceneView const& sc, int tri, float bu, float bv, f3 rd) {
  if constexpr (F & kFeatMotion) return hit_finish(motion_post(k, sc.post[tri], tri, motion_time()), bu, bv, rd);
  else return hit_finish(sc.post[tri], bu, bv, rd);
}

#include "medium_device.hpp"

// One-record light lists through the scalar path (RenderParams::uniformLights): the rows of path_shade that carry the two
// scalar arms.  Every row whose pick is the uniform one does, but for the nine masks under which a kernel gains scratch from the
// arms and the plain BVH row, which measured slower with them ("Shading: scalar light records"; profiles/shade_loads/kernel_resources_*.txt); those keep the parent's
// code, and run the lane's pick for every list.  The tree rows pick by their trees and are left alone in the hit arm.
// The list is read off one compiler's register allocation and nothing re-derives it by itself: after a change to path_shade
// or a new compiler, return true here, run `make asm` on that and on the commit before, and diff the two tables of
// tools/kernel_resources.py over EVERY line -- the megakernel rows and the `void k_test_trace<F>` probes, which instantiate
// the same masks, alike (first column: everything before the last seven fields).  A mask any of whose kernels gains scratch
// bytes or loses a wave goes on the list; then build again and diff again, since the masks taken out return to the parent's
// figures.
constexpr bool uniform_lights_row(uint32_t F) {
  uint32_t const row = F & ~kFeatStats;
  return row != (kFeatBvh | kFeatEnv) && row != (kFeatBvh | kFeatEnv | kFeatMedium) && row != (kFeatBvh | kFeatEnv | kFeatTex) &&
         row != (kFeatBvh | kFeatEnv | kFeatTex | kFeatVtxNormals) && row != (kFeatBvh | kFeatTex) && row != (kFeatEnv | kFeatArea) &&
         row != (kFeatEnv | kFeatMotion) && row != (kFeatBvh | kFeatBlend) && row != (kFeatEnv | kFeatTex | kFeatTexFilter) &&
         row != kFeatBvh;  // (no scratch, one more VGPR: measured 0.3 % slower on 1 M triangles with the arms, six runs each)
}

template <uint32_t F>
DMT_DEV bool path_shade(KArgs k, PathState& st, int bestTri, float bu, float bv) {
  static_assert(!((F & kFeatLightTree) && (F & kFeatLightTreeRef)), "one light tree at a time");
  static_assert(!(F & kFeatEmitterTree) || ((F & kFeatArea) && !(F & ~(kFeatEmitterTree | kFeatArea | kFeatBvh | kFeatEnv))), "emitter tree: the emissive-triangle rows only");
  static_assert(!((F & kFeatTex) && (F & kFeatBlend)), "kFeatBlend carries the texture code itself");
  static_assert(!(F & kFeatTexFilter) || (F & (kFeatTex | kFeatBlend)), "the texture filter needs the texture code");
  static_assert(!(F & kFeatMotion) || !(F & ~(kFeatMotion | kFeatBvh | kFeatEnv)), "motion: the plain and env-map rows only");
  static_assert(!(F & kFeatCutout) || ((F & kFeatTex) && !(F & ~(kFeatCutout | kFeatBvh | kFeatEnv | kFeatTex))), "cutouts: the texture rows only");
  static_assert(!(F & kFeatVtxNormals) || !(F & ~(kFeatVtxNormals | kFeatBvh | kFeatEnv | kFeatTex)), "vertex normals: the plain, env-map and texture rows only");
  // the medium has the plain and env-map rows only: each of its bits implies kFeatMedium and nothing outside kMediumRow
  constexpr uint32_t kMediumRow = kFeatBvh | kFeatEnv | kFeatMedium | kFeatMediumGrid | kFeatMediumSpectrum;
  constexpr bool mediumRowOk = (F & kFeatMedium) && !(F & ~kMediumRow);
  static_assert(!(F & kFeatMedium) || mediumRowOk, "medium: the plain and env-map rows only");
  static_assert(!(F & kFeatMediumGrid) || mediumRowOk, "medium grid: with the medium, on the plain and env-map rows only");
  static_assert(!(F & kFeatMediumSpectrum) || mediumRowOk, "medium spectrum: with the medium, on the plain and env-map rows only");
  constexpr bool kUniformRow = uniform_lights_row(F);
  SceneView const sc = load_scene(k);
  int const maxDepth = kargs(k)->maxDepth;
  if constexpr (F & kFeatMedium) {  // a collision inside the box replaces the surface hit or the miss
    int const mv = medium_vertex<F>(k, st, sc, bestTri, bu, bv);
    if (mv != MV_THROUGH) return mv == MV_ENDED;
  }
  if constexpr (F & kFeatEnv) {
    if (bestTri < 0) {  // A18: the env map seen by a path ray, MIS against NEE (core-render.cpp:154-163)
      EnvView const env = load_env(k);
      float pdfLight = 0.f;
      f3 const Le = env_eval_dir(env, ray_dir(st), pdfLight);
      if (st.depth == 0 || st.lastSpecular)
        st.L = st.L + st.beta * Le;
      else
        st.L = st.L + st.beta * (st.lastPdf / (st.lastPdf + pdfLight)) * Le;
      return true;
    }
  }
  if (bestTri < 0) {  // miss: constant environment, no MIS (megakernel.cu:135-151)
    if (sc.infLightCount > 0) {
      if constexpr (kUniformRow) {
        // one infinite light: pick_index(u, 1) is 0 for every u, so the record is wave-uniform and comes by s_load; its type
        // test is a scalar branch and the arm has no vector load.  The draw stays: the dimension counter advances as before
        float const uInf = st.rng.get1D();
        float const pmf = 1.f / float(sc.infLightCount);
        if (sc.infLightCount == 1u && kargs(k)->uniformLights) {
          Rec32 const light = load_rec0_uniform(sc.infLights);
          if (light_type(light) == LT_ENV) st.L = st.L + st.beta * light_intensity(light) / pmf;
        } else {
          Rec32 const light = sc.infLights[pick_index(uInf, sc.infLightCount)];
          if (light_type(light) == LT_ENV) st.L = st.L + st.beta * light_intensity(light) / pmf;
        }
      } else {
        uint32_t const li = pick_index(st.rng.get1D(), sc.infLightCount);
        Rec32 const light = sc.infLights[li];
        float const pmf = 1.f / float(sc.infLightCount);
        if (light_type(light) == LT_ENV) st.L = st.L + st.beta * light_intensity(light) / pmf;
      }
    }
    sect_mark(4);
    return true;
  }
  f3 const rd = ray_dir(st);
  Hit const hit = shade_hit<F>(k, sc, bestTri, bu, bv, rd);
  uint32_t nAll = sc.lightCount;  // lights the NEE chooses among
  if constexpr (F & kFeatArea) {
    KArgs const ka = kargs(k);
    nAll += ka->areaCount;
    uint32_t const ai = ka->areaOf[bestTri];
    if (ai != 0xFFFFFFFFu) {  // emitted radiance of the surface the path ray hit
      f3 const o = mk3(st.rp.ox.x, st.rp.oy.x, st.rp.oz.x);
      float const pl = area_pdf(sc.post[bestTri], rd, dot(hit.pos - o, rd));
      if (pl > 0.f) {
        f3 const Le = mk3(ka->areaLe[3 * ai], ka->areaLe[3 * ai + 1], ka->areaLe[3 * ai + 2]);
        if (st.depth == 0 || st.lastSpecular) {
          st.L = st.L + st.beta * Le;
        } else {
          float const a = st.lastPdf;
          float b;  // pl x the probability with which NEE at the vertex the ray left picks this triangle
          if constexpr (F & kFeatEmitterTree) {
            f3 pp, pn;
            get_prev_vertex(pp, pn);
            b = pl * ((F & kFeatEnv) ? 0.5f : 1.f) *
                et_pmf(ka->emitterTree, ka->emitterTrails[sc.lightCount + ai], pp.x, pp.y, pp.z, pn.x, pn.y, pn.z);
          } else {
            b = pl * ((F & kFeatEnv) ? 0.5f : 1.f) / float(nAll);
          }
          st.L = st.L + st.beta * Le * ((a * a) / (a * a + b * b));
        }
      }
    }
  }
  sect_mark(4);
  if (st.depth >= maxDepth) return true;  // :154-158

  f3 const wo = -rd;
  Rec32 rec = sc.bsdfs[hit.matId];
  f3 ns = hit.normal;  // shading normal: the geometric one unless vertex normals or a normal map say otherwise
  if constexpr (F & kFeatVtxNormals) ns = shading_normal_at(k, bestTri, bu, bv, hit.normal);
  // fractional "metallic" (BS_GGX_BLEND, JSON scenes): both lobes of the material are prepared, evaluated and sampled and the
  // results blended as the reference's CPU renderer does (core-material.cpp:275-286, :383-394).  kFeatBlend instantiations only.
  Rec32 rec2{};
  float mix = 0.f;
  bool blend = false;
  constexpr bool FILT = (F & kFeatTexFilter) != 0;
  TexDiff td{0.f, 0.f, 0.f, 0.f};  // UV differentials of the camera ray's hit; zero at every later hit (core-render.cpp:264-268)
  if constexpr (FILT) {
    if (st.depth == 0) td = tex_footprint(k, bestTri, hit.pos, hit.normal);
  }
  if constexpr (F & kFeatBlend) {
    if (hi16(rec.w[1]) == BS_GGX_BLEND) {
      mix = blend_metallic<FILT>(k, rec, hit.matId, bestTri, bu, bv, td);
      rec.w[1] = (rec.w[1] & 0x0000FFFFu) | (uint32_t(BS_GGX_DIEL) << 16);
      rec2 = sc.bsdfs[hit.matId + 1u];
      if (mix >= 1.f) rec = rec2;  // :273  the conductor alone
      else blend = mix > 0.f;      // :272  metallic <= 0: the dielectric alone
    }
  }
  if constexpr (F & (kFeatTex | kFeatBlend)) {
    if (!(F & kFeatBlend) || kargs(k)->matTex != nullptr) {
      ns = apply_material_textures<FILT>(k, rec, hit.matId, bestTri, bu, bv, ns, td);  // (ns: hit.normal, or the smooth normal the map perturbs)
      if (blend) (void)apply_material_textures<FILT>(k, rec2, hit.matId + 1u, bestTri, bu, bv, hit.normal, td);  // same roughness map
    }
  }
#if DMT_SECTION_TIMING
  {  // material mix of the lanes that shade in this pass: [11] passes with a GGX lane, [12] GGX lanes, [13] passes, [14] lanes
    bool const ggx = hi16(rec.w[1]) != BS_OREN;
    unsigned long long const all = __ballot(1), mg = __ballot(ggx);
    if (int(__ffsll((long long)all)) - 1 == int(threadIdx.x & 63u)) {
      unsigned long long* const acc = s_sectAcc[threadIdx.x >> 6];
      acc[11] += mg ? 1u : 0u, acc[12] += uint32_t(__popcll(mg)), acc[13] += 1u, acc[14] += uint32_t(__popcll(all));
    }
  }
#endif
  Bsdf const b = bsdf_prepare(rec, ns, wo);  // :165-166
  Bsdf b2{};
  if constexpr (F & kFeatBlend) {
    if (blend) b2 = bsdf_prepare(rec2, ns, wo);
  }
  // f * weight and pdf of the material towards wi.  Blend: f = lerp(fD, fC, metallic), the RGB overload (a, b, t) of
  // cudautils-color.cuh:112-114; pdf = lerp(pdfD, pdfC, metallic) resolves to the FLOAT overload dmt::lerp(float x, float a,
  // float b) = (1 - x) a + x b (cudautils-vecmath.cuh:750-752), i.e. the reference computes (1 - pdfD) pdfC + pdfD metallic.
  // Kept as written, on the sampling side too (core-material.cpp:282).
  auto blend_pdf = [&](float pdfD, float pdfC) { return (1.f - pdfD) * pdfC + pdfD * mix; };
  auto eval_material = [&](f3 wi, float& pdf) {
    f3 f = eval_bsdf(b, wo, wi, ns, hit.normal, pdf) * b.weight;
    if constexpr (F & kFeatBlend) {
      if (blend) {
        float pdfC = 0.f;
        f3 const fC = eval_bsdf(b2, wo, wi, ns, hit.normal, pdfC) * b2.weight;
        f = f * (1.f - mix) + fC * mix;
        pdf = blend_pdf(pdf, pdfC);
      }
    }
    return f;
  };
  sect_mark(5);

  // next-event estimation (:170-241)
  float uLight = st.rng.get1D();
  f2 const uLight2 = st.rng.get2D();
  bool envNee = false;
  if constexpr (F & kFeatEnv) {  // A18: env map with probability 1/2, the light list otherwise (core-render.cpp:290-299)
    envNee = uLight < 0.5f;
    uLight = envNee ? uLight : (uLight - 0.5f) * 2.f;
    if (envNee) {
      EnvView const env = load_env(k);
      EnvSampleDev const es = env_sample(env, uLight2);
      if (es.ok) {
        float bsdfPdf = 0.f;
        f3 const f = eval_material(es.wi, bsdfPdf);
        f3 const Le = env_eval_uv(env, es.uv);
        if (!is_zero(f) && max3(Le) > 0.f) {  // core-render.cpp:357-369: Le f / (pdfLight pmf + pdfBsdf), pmf = 1/2
          put_C(st.beta * (Le * f / (es.pdf * 0.5f + bsdfPdf)));
          set_shadow_ray(st, offset_ray_origin(hit.pos, hit.error, hit.normal, es.wi), es.wi);
          st.smax = kInf;
          st.hasShadow = true;
        }
      }
    }
  }
  bool areaNee = false;
  [[maybe_unused]] int etSel = -1;  // kFeatEmitterTree: the emitter the tree picked at this vertex (-1: none) and its probability
  [[maybe_unused]] float etPmf = 0.f;
  if constexpr (F & kFeatArea) {
    uint32_t li;
    if constexpr (F & kFeatEmitterTree) {
      // one walk at (hit.pos, hit.normal), the vertex a later emitter hit evaluates et_pmf at: kept bit for bit (put_prev_vertex)
      put_prev_vertex(hit.pos, hit.normal);
      if (!envNee) {
        KArgs const ka = kargs(k);
        etSel = et_select(ka->emitterTree, hit.pos.x, hit.pos.y, hit.pos.z, hit.normal.x, hit.normal.y, hit.normal.z, uLight, etPmf);
      }
      li = etSel >= 0 ? uint32_t(etSel) : 0u;
      areaNee = etSel >= 0 && li >= sc.lightCount;
    } else {
      li = pick_index(uLight, nAll);
      areaNee = !envNee && li >= sc.lightCount;
    }
    if (areaNee) {
      KArgs const ka = kargs(k);
      uint32_t const ai = li - sc.lightCount;
      AreaSampleDev const as = area_sample(sc.post[ka->areaTri[ai]], hit.pos, uLight2);
      if (as.ok) {
        float bsdfPdf = 0.f;
        f3 const f = eval_material(as.wi, bsdfPdf);
        if (!is_zero(f)) {
          f3 const Le = mk3(ka->areaLe[3 * ai], ka->areaLe[3 * ai + 1], ka->areaLe[3 * ai + 2]);
          float a;
          if constexpr (F & kFeatEmitterTree) a = as.pdf * ((F & kFeatEnv) ? 0.5f : 1.f) * etPmf;
          else a = as.pdf * ((F & kFeatEnv) ? 0.5f : 1.f) / float(nAll);
          float const bb = bsdfPdf;
          put_C(st.beta * (Le * f * (((a * a) / (a * a + bb * bb)) / a)));
          set_shadow_ray(st, offset_ray_origin(hit.pos, hit.error, hit.normal, as.wi), as.wi);
          st.smax = as.dist * 0.999f;
          st.hasShadow = true;
        }
      }
    }
  }
  bool treeNee = false;
  if constexpr (F & kFeatLightTreeRef) {
    // The reference's light tree with its own semantics (light_tree_ref.hpp): a cut of up to FOUR tree nodes, one light drawn
    // below each, one shadow ray per light (core-render.cpp:296-370).  This loop carries one pending shadow ray per lane, so
    // all but the LAST contributing light are tested for visibility right here (a whole any-hit traversal per ray; the
    // lane's traversal stack is free while it shades) and added in the reference's order; the last one rides with the next
    // closest-hit ray as usual.  Opt-in mode: the divergence of these in-line traversals is its price.
    treeNee = !envNee && sc.lightCount > 1;
    if (treeNee) {
      LightTreeRefSelection const sel = ltr_select(kargs(k)->lightTreeRef, hit.pos.x, hit.pos.y, hit.pos.z, hit.normal.x, hit.normal.y,
                                                   hit.normal.z, uLight, (F & kFeatEnv) ? 0.5f : 1.f);
      bool pending = false;
      f3 pendC = mk3(0, 0, 0), pendO = mk3(0, 0, 0), pendD = mk3(0, 0, 0);
      float pendMax = 0.f;
      for (uint32_t i = 0; i < sel.count; ++i) {
        Rec32 const light = sc.lights[sel.indices[i]];
        float const pmf = sel.pmfs[i];
        LightSample const ls = sample_light(light, hit.pos, uLight2, st.lastT, hit.normal);
        if (!ls.valid()) continue;
        float bsdfPdf = 0.f;
        f3 const f = eval_material(ls.direction, bsdfPdf);
        if (is_zero(f)) continue;
        f3 const Le = eval_light(light, ls);
        f3 C;
        if (ls.delta) {
          C = st.beta * Le * f / pmf;
        } else {
          float const w = sqr(pmf * ls.pdf) / sqr(pmf * ls.pdf + bsdfPdf);
          C = Le * f * st.beta * w;
        }
        if (pending) {  // an earlier light is waiting: resolve it now, keep this one pending
          bool occ;
          if constexpr (F & kFeatBvh) {
            occ = bvh_any(load_bvh(k), true, pendO, pendD, pendMax, blockIdx.x * blockDim.x + threadIdx.x);
          } else {
            PathState tmp = st;
            set_shadow_ray(tmp, pendO, pendD);
            tmp.smax = pendMax;
            int bt;
            float tu, tvv;
            trace_pair_brute<false>(k, tmp, false, true, bt, tu, tvv, occ);  // divergent here: the plain loop over every triangle
          }
          if (!occ) st.L = st.L + pendC;
        }
        pending = true, pendC = C, pendMax = ls.distance;
        pendO = offset_ray_origin(hit.pos, hit.error, hit.normal, ls.direction), pendD = ls.direction;
      }
      if (pending) {
        put_C(pendC);
        set_shadow_ray(st, pendO, pendD);
        st.smax = pendMax;
        st.hasShadow = true;
      }
    }
  }
  if (!envNee && !areaNee && !treeNee && sc.lightCount > 0) {
    uint32_t li = 0;
    float pmf = 0.f;
    bool picked = true;
    if constexpr (F & kFeatLightTree) {  // importance-driven choice (light_tree.hpp) instead of the uniform pick
      float treePmf = 0.f;
      int const sel = lt_select(kargs(k)->lightTree, hit.pos.x, hit.pos.y, hit.pos.z, hit.normal.x, hit.normal.y, hit.normal.z, uLight, treePmf);
      picked = sel >= 0;
      li = picked ? uint32_t(sel) : 0u;
      pmf = ((F & kFeatEnv) ? 0.5f : 1.f) * treePmf;
    } else if constexpr (F & kFeatEmitterTree) {  // the walk above returned a record of the light list, or nothing
      picked = etSel >= 0;
      li = picked ? uint32_t(etSel) : 0u;
      pmf = ((F & kFeatEnv) ? 0.5f : 1.f) * etPmf;
    } else {
      li = pick_index(uLight, (F & kFeatArea) ? nAll : sc.lightCount);
      pmf = ((F & kFeatEnv) ? 0.5f : 1.f) / float((F & kFeatArea) ? nAll : sc.lightCount);
    }
    // The uniform pick over ONE record returns 0 for every draw, so the record is wave-uniform: it comes by s_load, and the
    // type switches and the decoding of sample_light and eval_light run on scalar registers, each in a copy of its own so
    // that no word of the record merges with a lane's.  Only the sample meets the lane's path again.  Any other count, and
    // the tree rows, run the lane's pick
    constexpr bool kUniformArm = kUniformRow && !(F & (kFeatLightTree | kFeatEmitterTree | kFeatLightTreeRef));
    [[maybe_unused]] bool uniformRec = false;
    [[maybe_unused]] Rec32 light{};
    LightSample ls;
    if constexpr (kUniformArm) {
      uniformRec = ((F & kFeatArea) ? nAll : sc.lightCount) == 1u && kargs(k)->uniformLights;
      if (uniformRec) ls = sample_light(load_rec0_uniform(sc.lights), hit.pos, uLight2, st.lastT, hit.normal);
      else ls = sample_light(sc.lights[li], hit.pos, uLight2, st.lastT, hit.normal);
    } else {
      light = sc.lights[li];
      ls = sample_light(light, hit.pos, uLight2, st.lastT, hit.normal);
    }
    sect_mark(6);
    if (picked && ls.valid()) {
      float bsdfPdf = 0.f;
      f3 const f = eval_material(ls.direction, bsdfPdf);
      if (!is_zero(f)) {
        f3 Le;
        if constexpr (kUniformArm)  // (the record again, where it is used: its words are not held across the material's evaluation)
          Le = uniformRec ? eval_light(load_rec0_uniform(sc.lights), ls) : eval_light(sc.lights[li], ls);
        else
          Le = eval_light(light, ls);
        if (ls.delta) {
          put_C(st.beta * Le * f / pmf);
        } else {  // power heuristic, no division by the light pdf (:233-238)
          float const w = sqr(pmf * ls.pdf) / sqr(pmf * ls.pdf + bsdfPdf);
          put_C(Le * f * st.beta * w);
        }
        set_shadow_ray(st, offset_ray_origin(hit.pos, hit.error, hit.normal, ls.direction), ls.direction);
        st.smax = ls.distance;
        st.hasShadow = true;
      }
      // f == 0: the reference traces the shadow ray and then adds nothing; not traced here
    }
  }

  if constexpr (F & kFeatMedium) {  // the NEE just left pending, times the transmittance of its shadow segment
    if (st.hasShadow) medium_attenuate_pending<F>(k, st);
  }
  // bounce (:247-295); get2D before get1D = left-to-right argument evaluation
  sect_mark(7);
  f2 const u2 = st.rng.get2D();
  float const uc = st.rng.get1D();
  BsdfSample bs = sample_bsdf(b, wo, ns, hit.normal, u2, uc);
  if constexpr (F & kFeatBlend) {
    if (blend) {  // core-material.cpp:275-286: both lobes sampled with the same numbers; direction and flags of the conductor's
      BsdfSample sC = sample_bsdf(b2, wo, ns, hit.normal, u2, uc);
      sC.f = bs.f * (1.f - mix) + sC.f * mix;
      sC.pdf = blend_pdf(bs.pdf, sC.pdf);
      sC.eta = 1.f;
      bs = sC;
    }
  }
  sect_mark(8);
  if (!bs.valid()) return true;
  st.lastT = bs.refract;
  if constexpr (F & (kFeatEnv | kFeatArea)) st.lastPdf = bs.pdf, st.lastSpecular = bs.delta;
  set_ray(st, offset_ray_origin(hit.pos, hit.error, hit.normal, bs.wi), bs.wi);
  st.beta = st.beta * (bs.f * fabsf(dot(bs.wi, hit.normal)) / bs.pdf);
  float const rrBeta = max3(st.beta * bs.eta);
  if (rrBeta < 1 && st.depth > 1) {
    float const q = fmaxf(0.f, 1.f - rrBeta);
    if (st.rng.get1D() < q) return true;
    st.beta = st.beta / (1 - q);
  }
  ++st.depth;
  sect_mark(9);
  return false;
}

DMT_DEV TriS load_tri(TriIsect const DMT_CONST_AS* tris, uint32_t i) {
  TriS T;
  T.p0x = tris[i].p0x, T.p0y = tris[i].p0y, T.p0z = tris[i].p0z;
  T.e0x = tris[i].e0x, T.e0y = tris[i].e0y, T.e0z = tris[i].e0z;
  T.e1x = tris[i].e1x, T.e1y = tris[i].e1y, T.e1z = tris[i].e1z;
  return T;
}

// One pass over the triangle array for the lane's ray pair: closest hit for .x, any-hit for .y.
// Brute force = the reference's semantics.  The loop index is wave-uniform and the array is read
// through the constant address space, so each triangle arrives by s_load into SGPRs, prefetched one
// triangle ahead in a two-register ping-pong (no SGPR copies), and the VALU work is packed fp32 over the
// two rays: no VGPR, LDS or vector-memory traffic in the loop.
struct BruteHit {
  float bt, bu, bv;
  int tri;
  bool occluded;
};
// nine named scalars per triangle (never a struct, see mt_core9)
#define DMT_TRI_DECL(P) float P##0, P##1, P##2, P##3, P##4, P##5, P##6, P##7, P##8
#define DMT_TRI_LOAD(P, idx)                                                                          \
  P##0 = tris[idx].p0x, P##1 = tris[idx].p0y, P##2 = tris[idx].p0z, P##3 = tris[idx].e0x, P##4 = tris[idx].e0y, \
  P##5 = tris[idx].e0z, P##6 = tris[idx].e1x, P##7 = tris[idx].e1y, P##8 = tris[idx].e1z
#define DMT_TRI_TEST(P, idx)                                                                                   \
  do {                                                                                                         \
    MTPair m;                                                                                                  \
    mt_core9<v2f>(P##0, P##1, P##2, P##3, P##4, P##5, P##6, P##7, P##8, st.rp.ox, st.rp.oy, st.rp.oz, st.rp.dx, \
                  st.rp.dy, st.rp.dz, m.det, m.t, m.u, m.v);                                                   \
    bool const v1 = mt_valid(m.det.x, m.t.x, m.u.x, m.v.x);                                                    \
    bool const v2 = mt_valid(m.det.y, m.t.y, m.u.y, m.v.y);                                                    \
    if (doC && v1 && m.t.x < h.bt) { /* strict <: lowest index wins ties (megakernel.cu:126) */                 \
      h.bt = m.t.x;                                                                                            \
      h.tri = int(idx);                                                                                        \
      h.bu = m.u.x;                                                                                            \
      h.bv = m.v.x;                                                                                            \
    }                                                                                                          \
    if (doS && v2 && m.t.y < st.smax) h.occluded = true; /* :210-211 */                                        \
  } while (0)

// LDS of the culled clusters: the block's copy of their triangles and task records (cull_stage), and per wave the bound
// hits of one group of kCullGroup clusters and the per-lane results of the compacted tests (brute_clusters).  5 856 B per block.
__shared__ float s_cullTri[9 * kCullMaxTris];                         // [field][slot]
__shared__ CullRec s_cullRec[kCullMaxClusters];
__shared__ unsigned long long s_cullKey[kLdsThreads];                 // closest ray: min of (t bits << 32 | original index << 6 | slot)
__shared__ unsigned long long s_cullOcc[kLdsThreads / 64];            // shadow rays: bit `lane` = some culled triangle occludes it
__shared__ uint8_t s_cullOwner[kLdsThreads / 64][kCullGroup][128];   // per cluster of the group: lane | 64 * shadow of every bound hit
constexpr float kCullTSlack = 1.0f + 1.0f / 256;  // the bound test's segment ends this much beyond smax / the best t so far
constexpr float kCullRel = 1.0f / 16384;          // ... and a sphere's radius grows by this fraction of the squared ray extent
constexpr float kCullTLo = 1e-4f * (1.0f - 1.0f / 256);  // box bounds: the segment starts this far below mt_valid's t > 1e-4

#ifndef DMT_CULL_COUNTS
#define DMT_CULL_COUNTS 0
#endif
#if DMT_CULL_COUNTS
// Diagnostic build only (make variant DEFS=-DDMT_CULL_COUNTS=1): the work of brute_clusters summed over all waves, read back
// with dmt_diag_cull_counts (tools/diag_cull_counts.py).  [0] calls per wave, [1] / [2] closest / shadow rays, [3] task passes,
// [4 + kind] bound hits of closest rays, [6 + kind] of shadow rays, [8 + kind] compacted tasks; kind 0 = sphere, 1 = box.
__device__ unsigned long long g_cullCount[16];
#endif

// Every thread of a block that traces with trace_pair_brute<true> runs this once before its first trace (the kernels
// whose body can call it: brute-force megakernels, k_test_trace, k_test_closest).  Any block size up to kLdsThreads.
DMT_DEV void cull_stage(KArgs k) {
  k = kargs(k);
  if (k->cull.clusterCount == 0) return;  // uniform: nobody waits at the barrier
  float const* const t9 = k->cull.tri9;
  for (uint32_t i = threadIdx.x; i < 9 * kCullMaxTris; i += blockDim.x) s_cullTri[i] = t9[i];
  CullCluster const* const cl = k->cull.clusters;
  for (uint32_t i = threadIdx.x; i < kCullMaxClusters; i += blockDim.x)
    s_cullRec[i] = CullRec{cl[i].first, cl[i].count | cl[i].slot << 16, cl[i].magic};
  __syncthreads();
}

// ---- the box bound (device: brute_clusters; host: dmt_cull_box_test runs the same functions) ----
// A box record holds centre c and half-width h per axis.  With A = 1 / d and B = -(o A), the ray meets the axis' two planes
// at mid -+ h |A|, mid = c A + B: no compare orders the two.  Per ray (cull_ray): A, B, E2 (|A| the compiler forms again
// at every box, 6 v_and: packed fmas take no abs).  Per box and axis (cull_box_axis): three fmas.  Per ray and box
// (cull_box_accept): max3, min3, two clamps, one fma and max(near_xyz, kCullTLo) <= min(far_xyz, tmax) * kCullTSlack + E2.
//
// |d| is raised to kCullDirFloor = 2^-60 before the reciprocal, so A, B and E2 stay finite for coordinates below 2^60 (with
// a floor of FLT_MIN, o A overflows for |o| >= 4 and c A + B is inf - inf).  A smaller component becomes one of that size
// and the same sign: the ray leans into the slab it lies in, and an origin on a face gives mid -+ h |A| = 0 on that face up
// to E2 -- a hit, never a miss.  Raising |d| shrinks the axis' interval towards t = 0; a ray that meets the vertex box with
// such a component starts within 2^-60 t of its slab and at least m inside the record's, whose far plane then lies beyond
// 2^60 m, past every t the other axes allow.
//
// Conservativeness.  Let R = [c - h, c + h] in exact arithmetic; the planner makes R hold its inflated box.
// u = 2^-24.  The three roundings of an axis bound, near' = fl(fl(c A - fl(o A)) -+ h |A|):
//   fl(o A):        at most u |B|;
//   the mid fma:    at most u |mid'| <= u (|c| |A| + |B|);
//   the bound fma:  at most u (|mid'| + h |A|) <= u ((|c| + h) |A| + |B|);
// in all at most 3 u |B| + u (2 |c| + h) |A| (second-order terms are 2^-22 of that).  The second term is the plane moved by
// at most u (2 |c| + h) <= 2^-23 (extent + |coordinate|_max) = m / 16 in space: the computed bounds are those of a box R-
// that still holds the vertex box inflated by 15/16 m, which is what remains for what m was sized for (mt_valid's slack,
// the float edges, Moeller-Trumbore's rounding across the ray: a margin of about 7.5 instead of 8).  The first term has no
// bound relative to a small t -- an origin near a plane, a camera far from the scene -- and is covered by
// E = kCullErrK max(|Bx|, |By|, |Bz|) per ray, kCullErrK = 2^-21 = 8 u: every bound is within 3/8 E of R-'s, so
// max near' <= max near + 3/8 E <= min far + 3/8 E <= min far' + 3/4 E, and the two clamps are exact.  The test adds
// E2 = 2 E: of the 5/4 E to spare, 2^-8 (3/8 E) goes to the slack factor multiplying a far' that is 3/8 E low, the rest is
// margin (a factor 8/3 on the rounding terms).  A is the reciprocal instruction's, within 1 ulp of 1 / d: a relative error
// of every t of the axis, which kCullTSlack covers with room, as it covers the rounding of the t that mt_core9 computes.
// Flushed denormals move a bound by at most 2^-126, far below 2^-8 kCullTLo.
constexpr float kCullDirFloor = 0x1p-60f;
constexpr float kCullErrK = 0x1p-21f;
DMT_HD float cull_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DMT_HD v2f cull_fma(float a, v2f b, v2f c) { return __builtin_elementwise_fma(v2f{a, a}, b, c); }
DMT_HD float cull_abs(float a) { return __builtin_fabsf(a); }
DMT_HD v2f cull_abs(v2f a) { return __builtin_elementwise_abs(a); }
DMT_HD float cull_max(float a, float b) { return __builtin_fmaxf(a, b); }
DMT_HD v2f cull_max(v2f a, v2f b) { return __builtin_elementwise_max(a, b); }
// the direction component whose reciprocal the caller takes (device: v_rcp_f32, host: a division)
DMT_HD float cull_dir(float d) { return __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d), kCullDirFloor), d); }
template <class T>
struct CullRay {
  T ax, ay, az;  // A
  T rx, ry, rz;  // |A|
  T bx, by, bz;  // B
  T e2;          // 2 E
};
template <class T>
DMT_HD CullRay<T> cull_ray(T ox, T oy, T oz, T ax, T ay, T az) {
  CullRay<T> r;
  r.ax = ax, r.ay = ay, r.az = az;
  r.rx = cull_abs(ax), r.ry = cull_abs(ay), r.rz = cull_abs(az);
  r.bx = -(ox * ax), r.by = -(oy * ay), r.bz = -(oz * az);
  r.e2 = (2.0f * kCullErrK) * cull_max(cull_max(cull_abs(r.bx), cull_abs(r.by)), cull_abs(r.bz));
  return r;
}
template <class T>
DMT_HD void cull_box_axis(float c, float h, T a, T r, T b, T& near, T& far) {
  T const mid = cull_fma(c, a, b);
  near = cull_fma(-h, r, mid), far = cull_fma(h, r, mid);
}
// tmax: the segment's end times kCullTSlack
DMT_HD bool cull_box_accept(float nx, float ny, float nz, float fx, float fy, float fz, float tmax, float e2) {
  float const n = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(nx, ny), nz), kCullTLo);
  float const f = __builtin_fminf(__builtin_fminf(__builtin_fminf(fx, fy), fz), tmax);
  return n <= cull_fma(f, kCullTSlack, e2);
}
DMT_DEV float slab_rcp(float d) { return rcp_(cull_dir(d)); }

// The culled clusters for the lane's ray pair, after the packed loop has run over the always list (h holds its result,
// with the always list's position in h.tri).  The clusters are taken kCullGroup at a time, which bounds the owner lists.  For
// each cluster of a group a packed bound test of both rays, over [0 or kCullTLo, smax] for the shadow ray and up to the best
// t so far for the closest ray, with slack: segment-sphere for sphere bounds, slabs for box bounds.  Then the (ray, triangle)
// tests of the rays that touched a bound are spread over the wave's active lanes, nAct per pass; a lane decodes (cluster,
// owner lane, kind, triangle), fetches the owner's ray with ds_bpermute and runs the scalar mt_core9 + mt_valid, which are
// bit-identical to the packed loop's halves.  Closest hits meet in a ds_min_u64 of (t bits, original index, slot) per owner,
// shadow hits in an OR.  After a group the closest ray's segment shrinks to the best culled hit so far.  The merge takes the
// lexicographic minimum with the loop's result: the same (tri, u, v, occluded) as one loop over every triangle in index order
// with a strict < (valid t > 1e-4, so float bits order like the floats; no two triangles share an original index).
DMT_DEV void brute_clusters(KArgs k, PathState const& st, bool doC, bool doS, BruteHit& h) {
  k = kargs(k);
  uint32_t const nc = k->cull.clusterCount;
  auto const* const cls = to_const_as(k->cull.clusters);
  if (h.tri >= 0) h.tri = int(k->cull.alwaysIdx[h.tri]);
  uint32_t const lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long const act = __ballot(1);
  uint32_t const nAct = uint32_t(__popcll(act));
  uint32_t const rank = __builtin_amdgcn_mbcnt_hi(uint32_t(act >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(act), 0u));
  s_cullKey[threadIdx.x] = ~0ull;
  s_cullOcc[w] = 0;
  float tmaxC = h.bt * kCullTSlack;
  float const tmaxS = st.smax * kCullTSlack;
  // the rays' constants of the two bound tests, once per call.  Unconditional: a uniform branch on the kinds of cluster
  // the plan has would cost a select per register, and the optimiser had hoisted the sphere test's pair out of the
  // loop for every plan before.
  CullRay<v2f> const cr = cull_ray(st.rp.ox, st.rp.oy, st.rp.oz, v2f{slab_rcp(st.rp.dx.x), slab_rcp(st.rp.dx.y)},
                                   v2f{slab_rcp(st.rp.dy.x), slab_rcp(st.rp.dy.y)}, v2f{slab_rcp(st.rp.dz.x), slab_rcp(st.rp.dz.y)});
  v2f const dd = st.rp.dx * st.rp.dx + st.rp.dy * st.rp.dy + st.rp.dz * st.rp.dz;
  v2f const idd = rcp_(dd);
  unsigned long long const mDoC = __ballot(doC), mDoS = __ballot(doS);  // the lanes with a ray of each kind, once per call
#if DMT_CULL_COUNTS
  unsigned long long cnt[16] = {};
  cnt[0] = 1, cnt[1] = __popcll(mDoC), cnt[2] = __popcll(mDoS);
#endif
  for (uint32_t c0 = 0; c0 < nc; c0 += kCullGroup) {
    uint32_t pre[kCullGroup + 1];  // first task of each cluster of the group (uniform)
    pre[0] = 0;
#pragma unroll
    for (uint32_t q = 0; q < kCullGroup; ++q) {
      uint32_t tasks = 0;
      if (c0 + q < nc) {
        // the record's first eight words in one scalar load (c0 + q is uniform): the bound, its kind and the count.  Volatile
        // keeps it one load at this place: a plain one is sunk into the two arms below, behind their arithmetic
        CullWords const rw = *reinterpret_cast<CullWords const volatile DMT_CONST_AS*>(cls + (c0 + q));
        CullCluster cl;
        for (int i = 0; i < 6; ++i) cl.b[i] = __uint_as_float(rw[i]);
        cl.box = rw[6], cl.count = rw[7];
        // The verdicts are balloted inside each arm, each ballot of ONE compare, and meet the rays' masks (mDoC, mDoS) in
        // scalar registers.  A ballot of anything but a compare -- a lane boolean merged across this branch, an `and` of
        // two -- is lowered through a VGPR: v_cndmask 0, 1 and v_cmp_ne 0, two expensive instructions per vote, four
        // votes per cluster.  The lane's own bit comes back from the mask for free.
        unsigned long long mC, mS;
        if (cl.box) {
          // slabs: per axis the entry and the exit, near = max over the entries and the segment start, far = min over the
          // exits and the segment end (see cull_ray for the arithmetic and what keeps it conservative)
          v2f nx, ny, nz, fx, fy, fz;
          cull_box_axis(cl.b[0], cl.b[3], cr.ax, cr.rx, cr.bx, nx, fx);
          cull_box_axis(cl.b[1], cl.b[4], cr.ay, cr.ry, cr.by, ny, fy);
          cull_box_axis(cl.b[2], cl.b[5], cr.az, cr.rz, cr.bz, nz, fz);
          // (both verdicts first, then the masks: behind a short-circuit && the test sits in a branch of its own, where
          // the compiler quiets every min / max input again)
          bool const aC = cull_box_accept(nx.x, ny.x, nz.x, fx.x, fy.x, fz.x, tmaxC, cr.e2.x);
          bool const aS = cull_box_accept(nx.y, ny.y, nz.y, fx.y, fy.y, fz.y, tmaxS, cr.e2.y);
          mC = __ballot(aC) & mDoC, mS = __ballot(aS) & mDoS;
        } else {
          v2f const wx = cl.b[0] - st.rp.ox, wy = cl.b[1] - st.rp.oy, wz = cl.b[2] - st.rp.oz;
          v2f const ww = wx * wx + wy * wy + wz * wz;
          v2f tc = (wx * st.rp.dx + wy * st.rp.dy + wz * st.rp.dz) * idd;
          tc.x = fminf(fmaxf(tc.x, 0.f), tmaxC);
          tc.y = fminf(fmaxf(tc.y, 0.f), tmaxS);
          v2f const ex = wx - tc * st.rp.dx, ey = wy - tc * st.rp.dy, ez = wz - tc * st.rp.dz;
          v2f const ee = ex * ex + ey * ey + ez * ez;
          v2f const lim = cl.b[3] + kCullRel * (ww + tc * tc * dd);
          mC = __ballot(ee.x <= lim.x) & mDoC, mS = __ballot(ee.y <= lim.y) & mDoS;
        }
        bool const hitC = __builtin_amdgcn_inverse_ballot_w64(mC), hitS = __builtin_amdgcn_inverse_ballot_w64(mS);
        uint32_t const nC = uint32_t(__popcll(mC)), nS = uint32_t(__popcll(mS));
        if (hitC) s_cullOwner[w][q][__builtin_amdgcn_mbcnt_hi(uint32_t(mC >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mC), 0u))] = uint8_t(lane);
        if (hitS)
          s_cullOwner[w][q][nC + __builtin_amdgcn_mbcnt_hi(uint32_t(mS >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mS), 0u))] =
              uint8_t(lane | 64u);
        tasks = (nC + nS) * cl.count;
#if DMT_CULL_COUNTS
        if (cl.box) cnt[5] += nC, cnt[7] += nS, cnt[9] += tasks;
        else cnt[4] += nC, cnt[6] += nS, cnt[8] += tasks;
#endif
      }
      pre[q + 1] = pre[q] + tasks;
    }
    uint32_t const total = pre[kCullGroup];
#if DMT_CULL_COUNTS
    cnt[3] += (total + nAct - 1) / nAct;
#endif
    asm volatile("" ::: "memory");  // one wave's LDS operations complete in order: only the compiler must not reorder them
    for (uint32_t base = 0; base < total; base += nAct) {
      uint32_t const g = min(base + rank, total - 1u);
      uint32_t q = 0, first = 0;
#pragma unroll
      for (uint32_t p = 1; p < kCullGroup; ++p)
        if (g >= pre[p]) q = p, first = pre[p];
      CullRec const rec = s_cullRec[c0 + q];
      uint32_t const count = rec.countSlot & 0xFFFFu, slot0 = rec.countSlot >> 16;
      uint32_t const local = g - first;
      uint32_t const e = __umulhi(local, rec.magic);  // local / count, exact for local < 2^32 / count^2
      uint32_t const j = local - e * count;
      uint32_t const own = s_cullOwner[w][q][e];
      bool const shadow = own >= 64u;
      int const src = int(own & 63u) << 2;
      auto pull = [&](v2f v) {
        float const a = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(v.x)));
        float const b = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(v.y)));
        return shadow ? b : a;
      };
      float const ox = pull(st.rp.ox), oy = pull(st.rp.oy), oz = pull(st.rp.oz);
      float const dx = pull(st.rp.dx), dy = pull(st.rp.dy), dz = pull(st.rp.dz);
      float const smax = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(st.smax)));
      float const* const T = s_cullTri + slot0 + j;
      float det, t, u, v;
      mt_core9<float>(T[0 * kCullMaxTris], T[1 * kCullMaxTris], T[2 * kCullMaxTris], T[3 * kCullMaxTris], T[4 * kCullMaxTris],
                      T[5 * kCullMaxTris], T[6 * kCullMaxTris], T[7 * kCullMaxTris], T[8 * kCullMaxTris], ox, oy, oz, dx, dy, dz,
                      det, t, u, v);
      if (base + rank < total && mt_valid(det, t, u, v)) {
        if (shadow) {
          if (t < smax) atomicOr(&s_cullOcc[w], 1ull << (own & 63u));
        } else if (t < kInf) {
          atomicMin(&s_cullKey[w * 64u + own],
                    (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | ((rec.first + j) << kCullSlotBits) | (slot0 + j));
        }
      }
    }
    asm volatile("" ::: "memory");
    if (c0 + kCullGroup < nc) {  // the next group's closest segment ends at the best culled hit so far
      unsigned long long const kc = s_cullKey[threadIdx.x];
      if (kc != ~0ull) tmaxC = fminf(tmaxC, __uint_as_float(uint32_t(kc >> 32)) * kCullTSlack);
    }
  }
#if DMT_CULL_COUNTS
  if (rank == 0)
    for (int i = 0; i < 10; ++i) atomicAdd(&g_cullCount[i], cnt[i]);
#endif
  if (doC) {
    unsigned long long const kc = s_cullKey[threadIdx.x];
    if (kc < ((static_cast<unsigned long long>(__float_as_uint(h.bt)) << 32) | (uint32_t(h.tri) << kCullSlotBits))) {
      float const* const T = s_cullTri + (uint32_t(kc) & ((1u << kCullSlotBits) - 1u));
      float det, t, u, v;  // the winner's u, v: the scalar form of the test again, on the lane's own ray
      mt_core9<float>(T[0 * kCullMaxTris], T[1 * kCullMaxTris], T[2 * kCullMaxTris], T[3 * kCullMaxTris], T[4 * kCullMaxTris],
                      T[5 * kCullMaxTris], T[6 * kCullMaxTris], T[7 * kCullMaxTris], T[8 * kCullMaxTris], st.rp.ox.x, st.rp.oy.x,
                      st.rp.oz.x, st.rp.dx.x, st.rp.dy.x, st.rp.dz.x, det, t, u, v);
      h.bt = __uint_as_float(uint32_t(kc >> 32)), h.tri = int(uint32_t(kc) >> kCullSlotBits), h.bu = u, h.bv = v;
    }
  }
  if (doS && ((s_cullOcc[w] >> lane) & 1ull)) h.occluded = true;
}

// CULL = false: the plain loop over every triangle (callers in divergent code or outside a staged block).
template <bool CULL>
DMT_DEV void trace_pair_brute(KArgs k, PathState const& st, bool doC, bool doS, int& bestTri, float& bu,
                              float& bv, bool& occluded) {
  BruteHit h{kInf, 0.f, 0.f, -1, false};
  k = kargs(k);
  auto const* tris = to_const_as(CULL ? k->cull.always : k->scene.tris);
  uint32_t const n = CULL ? k->cull.alwaysCount : k->scene.triCount;
  uint32_t const last = n ? n - 1 : 0;
  DMT_TRI_DECL(a);
  DMT_TRI_DECL(b);
  DMT_TRI_LOAD(a, 0);  // the array always holds >= 1 record (DevBuf::assign)
  for (uint32_t i = 0; i < n;) {
    uint32_t const ib = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD(b, ib);
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch s_loads above the arithmetic
    DMT_TRI_TEST(a, i);
    if (++i >= n) break;
    uint32_t const ia = i + 1 < last ? i + 1 : last;
    DMT_TRI_LOAD(a, ia);
    __builtin_amdgcn_sched_barrier(0);
    DMT_TRI_TEST(b, i);
    ++i;
  }
  if constexpr (CULL) {
    if (kargs(k)->cull.clusterCount != 0) brute_clusters(k, st, doC, doS, h);
  }
  bestTri = h.tri, bu = h.bu, bv = h.bv, occluded = h.occluded;
}

#include "opacity.hpp"

struct LaneStats {  // stats build only
  uint32_t samples = 0, closest = 0, shadow = 0, bounces = 0;
  TraversalCounters tc;
  // loop profile of the BVH kernel: wave-level iterations (counted by every lane, /64 on the host) and the lanes
  // that did useful work in them
  uint32_t itNode = 0, itLeaf = 0, itShade = 0, itOuter = 0, itPrep = 0, lanesLeaf = 0, lanesShade = 0, lanesPrep = 0;
};
template <bool STATS = false>
DMT_DEV void trace_pair_bvh(KArgs k, PathState const& st, bool doC, bool doS, uint32_t gtid, int& bestTri,
                            float& bu, float& bv, bool& occluded, LaneStats* ls = nullptr) {
  BvhView const bvh = load_bvh(k);
  float bt;
  if constexpr (STATS) ls->closest += doC ? 1u : 0u, ls->shadow += doS ? 1u : 0u;
  bvh_closest<STATS>(bvh, doC, mk3(st.rp.ox.x, st.rp.oy.x, st.rp.oz.x), mk3(st.rp.dx.x, st.rp.dy.x, st.rp.dz.x),
                     gtid, bestTri, bt, bu, bv, STATS ? &ls->tc : nullptr);
  occluded = bvh_any<STATS>(bvh, doS, mk3(st.rp.ox.y, st.rp.oy.y, st.rp.oz.y),
                            mk3(st.rp.dx.y, st.rp.dy.y, st.rp.dz.y), st.smax, gtid, STATS ? &ls->tc : nullptr);
}
// the same two traversals through the motion tree (`bvh` of a motion launch), each ray at its own time.  bt (optional): the
// closest hit's t
DMT_DEV void trace_pair_bvh_motion(KArgs k, PathState const& st, bool doC, bool doS, v2f time, uint32_t gtid, int& bestTri, float& bu,
                                   float& bv, bool& occluded, float* btOut = nullptr) {
  BvhView const bvh = load_bvh(k);
  TriPairDelta const* const delta = kargs(k)->motion.pairDelta;
  float bt;
  bvh_closest<false>(bvh, doC, mk3(st.rp.ox.x, st.rp.oy.x, st.rp.oz.x), mk3(st.rp.dx.x, st.rp.dy.x, st.rp.dz.x), gtid, bestTri, bt, bu, bv,
                     nullptr, LeafMotion{delta, time.x});
  occluded = bvh_any<false>(bvh, doS, mk3(st.rp.ox.y, st.rp.oy.y, st.rp.oz.y), mk3(st.rp.dx.y, st.rp.dy.y, st.rp.dz.y), st.smax, gtid,
                            nullptr, LeafMotion{delta, time.y});
  if (btOut) *btOut = bt;
}

// One "ray pass" of a lane: trace (closest + pending shadow), resolve the shadow ray, shade.
// sink(L, sidx) is called once per completed sample with the index the sample was started with.
// park(doC, bestTri, bu, bv) (GGX batching, megakernel_body): called by every lane of the pass between the shadow resolve and
// the shading; returns whether the lane still shades in this pass.  NoPark: every lane with a closest ray does.
struct NoPark {};
template <uint32_t F, class Sink, class Park = NoPark>
DMT_DEV void lane_finish(KArgs k, PathState& st, bool doC, bool doS, int bestTri, float bu, float bv, bool occluded,
                         Sink&& sink, Park&& park = Park{});

template <uint32_t F, class Sink, class Park = NoPark>
DMT_DEV void lane_step(KArgs k, uint32_t gtid, PathState& st, Sink&& sink, LaneStats* ls = nullptr, Park&& park = Park{}) {
  constexpr bool PARK = !std::is_same<typename std::decay<Park>::type, NoPark>::value;
  bool const doC = st.active;
  bool const doS = st.hasShadow;
  int bestTri;
  float bu, bv;
  bool occluded;
  if constexpr (PARK) {
    // a lane that has taken a parked hit back shades it in this pass and traces no closest ray (its shadow ray, if it has
    // one, is traced as usual): the hit comes from the closest-ray half of rp, which such a lane does not need (ggx_resume)
    static_assert(F == 0, "GGX batching: the plain brute-force row only");
    trace_pair_brute(k, st, doC && !ggx_resumed(st), doS, bestTri, bu, bv, occluded);
    if (ggx_resumed(st)) bestTri = __float_as_int(st.rp.ox.x), bu = st.rp.oy.x, bv = st.rp.oz.x;
    sect_mark(2);
    lane_finish<F>(k, st, doC, doS, bestTri, bu, bv, occluded, sink, park);
    return;
  }
  if constexpr ((F & kFeatCutout) && (F & kFeatBvh))
    trace_pair_bvh_cut(k, st, doC, doS, gtid, bestTri, bu, bv, occluded);
  else if constexpr (F & kFeatCutout)
    trace_pair_brute_cut(k, st, doC, doS, bestTri, bu, bv, occluded);
  else if constexpr ((F & kFeatMotion) && (F & kFeatBvh))
    trace_pair_bvh_motion(k, st, doC, doS, v2f{motion_time(), motion_time_shadow()}, gtid, bestTri, bu, bv, occluded);
  else if constexpr (F & kFeatMotion)
    trace_pair_brute_motion(k, st, doC, doS, v2f{motion_time(), motion_time_shadow()}, bestTri, bu, bv, occluded);
  else if constexpr (F & kFeatBvh)
    trace_pair_bvh<(F & kFeatStats) != 0>(k, st, doC, doS, gtid, bestTri, bu, bv, occluded, ls);
  else
    trace_pair_brute(k, st, doC, doS, bestTri, bu, bv, occluded);
  sect_mark(2);
  if constexpr (F & kFeatStats) ls->bounces += (doC && bestTri >= 0 && st.depth < kargs(k)->maxDepth) ? 1u : 0u;
  lane_finish<F & ~kFeatStats>(k, st, doC, doS, bestTri, bu, bv, occluded, sink);
}

// Second half of a ray pass: resolve the shadow ray (in the reference's accumulation order), then shade.
template <uint32_t F, class Sink, class Park>
DMT_DEV void lane_finish(KArgs k, PathState& st, bool doC, bool doS, int bestTri, float bu, float bv, bool occluded,
                         Sink&& sink, Park&& park) {
  if (doS) {
    st.hasShadow = false;
    if (st.finPending) {  // the shadow ray of an already finished sample
      f3 Lfin = get_Lfin();
      if (!occluded) Lfin = Lfin + get_C();
      st.finPending = false;
      sink(Lfin, get_finIdx());
    } else if (!occluded) {
      st.L = st.L + get_C();  // NEE of the previous bounce, added before anything of this bounce
    }
  }
  sect_mark(3);
  // (the path's own shadow ray is resolved: a hit that parks here parks no shadow state)
  if constexpr (!std::is_same<typename std::decay<Park>::type, NoPark>::value) doC = park(doC, bestTri, bu, bv);
  if (doC) {
    if (path_shade<F>(k, st, bestTri, bu, bv)) {
      st.active = false;
      if (st.hasShadow) {  // last NEE still untraced: park the sample, the lane may start the next
        put_Lfin(st.L);
        put_finIdx(st.sidx);
        st.finPending = true;
      } else {
        sink(st.L, st.sidx);
      }
    }
  }
  if constexpr (F & kFeatMotion) {
    if (st.hasShadow) motion_park_shadow();  // made by the bounce just shaded (an older one was resolved above): the current sample's
  }
  sect_mark(10);
}

// the lane's NEXT sample, prepared ahead of need (sampler values + camera ray), [field][thread]
__shared__ float s_prep[15 * kLdsThreads];  // 0-7 sampler values, 8-13 camera ray, 14 staging index

// Starting a sample costs ~2k instructions (8 scrambled radical inverses + camera ray).  Paths end at
// different times, so doing it on demand would run that code for a handful of lanes on almost every
// pass.  Instead every lane keeps its next sample PREPARED in LDS; a finished lane swaps it in (a few
// LDS moves) and the preparation of the following one is batched: it runs when at least half the wave
// needs one, or when some lane would otherwise starve.  Sample values are pure functions of
// (pixel, sample), so preparing early changes nothing.
// Cold kernel arguments (camera matrices, sampler parameters: 38 dwords) are only needed here, once per
// sample.  Left to itself the compiler hoists their kernarg loads to the top of the kernel and keeps
// them in SGPRs across the triangle loop, which overflows the SGPR file and spills INTO the hot loop.
// Reading them through an opaque copy of the kernarg pointer keeps the s_loads at the point of use.
struct ColdArgs {
  CameraXf cam;
  SamplerParams sp;
};
DMT_DEV ColdArgs load_cold_args(KArgs Pk) {
  Pk = kargs(Pk);
  ColdArgs c;
#pragma unroll
  for (int i = 0; i < 16; ++i) c.cam.cfr[i] = Pk->cam.cfr[i], c.cam.rfc[i] = Pk->cam.rfc[i];
  c.sp.scale0 = Pk->sp.scale0, c.sp.scale1 = Pk->sp.scale1, c.sp.exp0 = Pk->sp.exp0, c.sp.exp1 = Pk->sp.exp1;
  c.sp.inv0 = Pk->sp.inv0, c.sp.inv1 = Pk->sp.inv1;
  return c;
}

// With a sampler table (RenderParams::samTab, wave-uniform) the 8 values and the film jitter are loaded -- three independent
// aligned vector loads per sample -- instead of computed: ~60 scrambled digits, a run-time division and a base-3 radical
// inverse per lane, repeated for every pixel congruent modulo 128.  The table holds what the code below computes, written by
// the same functions (k_sampler_table), so both paths prepare bit-identical samples.  The table's pointers and geometry are
// read from the kernel arguments here, like the cold arguments, and so is the lens (dmt_set_lens): a second wave-uniform
// branch, which makes the sample's ray a lens ray (prepare_lens_ray) and changes nothing else about the sample.
// The lens ray of a prepared sample, over the pinhole ray in s_prep[8..13].  It runs after the lens-free code instead of
// branching inside it, and reads everything it needs from the kernel arguments again, so that the code and the live ranges
// of a launch without a lens stay the parent's.  Measured with -Rpass-analysis=kernel-resource-usage: a
// branch inside the lens-free code, or this tail laid out in line, cost k_megakernel_bvh_env a spilled VGPR (8 bytes of
// scratch), and a noinline function gave eight rows a stack frame (and cannot take the opaque kernarg pointer); as an
// unlikely tail no row gains scratch.
// Under a pixel filter (dmt_set_pixel_filter) this is also where the jitter is warped: the one cold tail for
// lens and filter.  A table's jitter plane already holds the warped jitter, so a tabulated launch gets here only for a lens.
// Without a lens the tail forms the pinhole ray through camera_ray_jittered, the function the tabulated main path calls.
// Its form is the measured one again: jitter, then lens values, then one choice between the two ray
// functions.  A tail split into a lens branch and a filter branch cost k_megakernel_env_tex 4 bytes of scratch, and a lower
// clamp on filter_warp's bin index, or two 4-byte loads per axis from the knots themselves, cost forty rows a VGPR.
// The sample's film jitter as the tail needs it when no table supplies it: pixel2d, warped under a pixel filter.
DMT_DEV f2 tail_jitter(KArgs Pk, int32_t hidx) {
  KArgs const k = kargs(Pk);
  SamplerParams sp;
  sp.scale0 = k->sp.scale0, sp.scale1 = k->sp.scale1, sp.exp0 = k->sp.exp0, sp.exp1 = k->sp.exp1, sp.inv0 = k->sp.inv0, sp.inv1 = k->sp.inv1;
  f2 jit = pixel2d(sp, hidx);
  if (FilterBin const* const knots = kargs(Pk)->filtKnots) {
    float const fr = kargs(Pk)->filtR;
    jit.x = filter_warp(knots, fr, jit.x);
    jit.y = filter_warp(knots, fr, jit.y);
  }
  return jit;
}
// The ray of another projection than the perspective one (dmt_set_projection; never with a lens), over the
// ray prepare_lens_ray has just stored: the last step of the cold tail, after the perspective code and not a branch inside
// it.  It recomputes the jitter by tail_jitter (the bits a table's jitter plane holds) and reads the matrices from the kernel
// arguments once more, so that nothing of the perspective tail stays live for it.  Measured: where this
// block sits -- here, as a sibling branch in prepare_sample, merged into the choice between the two ray functions, or ahead of
// the lens code -- changes no row's resources; what does is the literal constants of its sine and cosine, which the compiler
// hoists out of the sample loop into registers that then live across the shading code (sincos_cold, pt_device.hpp).
DMT_DEV void prepare_projection_ray(KArgs Pk, int px, int py, int32_t pixBase, uint32_t s) {
  float* const prep = s_prep + threadIdx.x;
  int32_t const hidx = pixBase + int32_t(s) * (kargs(Pk)->sp.scale0 * kargs(Pk)->sp.scale1);
  f2 const jit = tail_jitter(Pk, hidx);
  KArgs const kp = kargs(Pk);
  CameraXf cam;
#pragma unroll
  for (int i = 0; i < 16; ++i) cam.cfr[i] = kp->cam.cfr[i], cam.rfc[i] = kp->cam.rfc[i];
  Ray const q = camera_ray_projection(cam, film_coord(jit.x, px), film_coord(jit.y, py), kp->projKind, kp->projA, kp->projW, kp->projH);
  prep[8 * kLdsThreads] = q.o.x, prep[9 * kLdsThreads] = q.o.y, prep[10 * kLdsThreads] = q.o.z;
  prep[11 * kLdsThreads] = q.d.x, prep[12 * kLdsThreads] = q.d.y, prep[13 * kLdsThreads] = q.d.z;
}
template <bool PROJ>  // PROJ: the row carries the projection's ray (projection_row)
DMT_DEV void prepare_lens_ray(KArgs Pk, int px, int py, int32_t pixBase, uint32_t s) {
  float* const prep = s_prep + threadIdx.x;
  f2 jit;
  LensU lu{0.f, 0.f};
  float const lensR = kargs(Pk)->lensRad;
  if (float2 const* const tab = kargs(Pk)->samTabLens) {  // launches with a table and a lens: its jitter (warped already) and lens planes
    KArgs const k = kargs(Pk);
    uint32_t const e = ((s - k->samTabS0) * k->samTabPh + (uint32_t(py) & 127u)) * k->samTabPw + (uint32_t(px) & 127u);
    float2 const j = k->samTabJit[e], u = tab[e];
    jit = mk2(j.x, j.y), lu = LensU{u.x, u.y};
  } else {  // computed: a lens, a pixel filter, or both
    int32_t const hidx = pixBase + int32_t(s) * (kargs(Pk)->sp.scale0 * kargs(Pk)->sp.scale1);
    jit = tail_jitter(Pk, hidx);
    if (lensR > 0.f) lu = lens_values(uint32_t(hidx));
  }
  CameraXf cam;
  KArgs const kc = kargs(Pk);
#pragma unroll
  for (int i = 0; i < 16; ++i) cam.cfr[i] = kc->cam.cfr[i], cam.rfc[i] = kc->cam.rfc[i];
  Ray const r = lensR > 0.f ? camera_ray_lens(cam, px, py, jit, lensR, kc->lensD, lu) : camera_ray_jittered(cam, px, py, jit);
  prep[8 * kLdsThreads] = r.o.x, prep[9 * kLdsThreads] = r.o.y, prep[10 * kLdsThreads] = r.o.z;
  prep[11 * kLdsThreads] = r.d.x, prep[12 * kLdsThreads] = r.d.y, prep[13 * kLdsThreads] = r.d.z;
  if constexpr (PROJ) {
    if (__builtin_expect(kargs(Pk)->projKind != 0, 0)) prepare_projection_ray(Pk, px, py, pixBase, s);
  }
}
#ifndef DMT_LENS_EARLY
#define DMT_LENS_EARLY 1  // variant builds for A/B runs: 0 reads the lens radius after the sample's LDS stores
#endif
// The rows whose cold tail carries the projection's ray: all but k_megakernel_env and k_megakernel_bvh_env_ltree.  Host and
// device read the same function (checkFeatures).
constexpr bool projection_row(uint32_t F) {
  uint32_t const row = F & ~kFeatStats;
  return row != kFeatEnv && row != (kFeatBvh | kFeatEnv | kFeatLightTree);
}
// PROJ: the cold tail ends with the projection's ray.  Two rows are compiled without it (projection_row): with it, in every
// shape of the tail that was measured, they spill one VGPR more than they did; without it their code is what
// it was, and dmt_render refuses another projection than the perspective one for them.
template <bool MOTION = false, bool PROJ = true>  // MOTION: the sample's time is prepared with it (motion.hpp)
DMT_DEV void prepare_sample(KArgs Pk, int px, int py, int32_t pixBase, uint32_t s) {
  float* const prep = s_prep + threadIdx.x;
  Ray r;
#if DMT_LENS_EARLY
  float const lensR = kargs(Pk)->camTail;  // lens or filter; with the table pointer, so that the compare below finds it ready
#endif
  if (float4 const* const tab = kargs(Pk)->samTab) {
    KArgs const k = kargs(Pk);
    uint32_t const e = ((s - k->samTabS0) * k->samTabPh + (uint32_t(py) & 127u)) * k->samTabPw + (uint32_t(px) & 127u);
    float4 const a = tab[2 * size_t(e)], b = tab[2 * size_t(e) + 1];
    float2 const jit = k->samTabJit[e];
    prep[0 * kLdsThreads] = a.x, prep[1 * kLdsThreads] = a.y, prep[2 * kLdsThreads] = a.z, prep[3 * kLdsThreads] = a.w;
    prep[4 * kLdsThreads] = b.x, prep[5 * kLdsThreads] = b.y, prep[6 * kLdsThreads] = b.z, prep[7 * kLdsThreads] = b.w;
    CameraXf cam;
    {
      KArgs const kc = kargs(Pk);
#pragma unroll
      for (int i = 0; i < 16; ++i) cam.cfr[i] = kc->cam.cfr[i], cam.rfc[i] = kc->cam.rfc[i];
    }
    r = camera_ray_jittered(cam, px, py, mk2(jit.x, jit.y));
  } else {
    ColdArgs const cold = load_cold_args(Pk);
    int32_t const hidx = pixBase + int32_t(s) * (cold.sp.scale0 * cold.sp.scale1);
    sampler_values(uint32_t(hidx), prep);
    r = camera_ray(cold.cam, cold.sp, px, py, hidx);
  }
  prep[8 * kLdsThreads] = r.o.x, prep[9 * kLdsThreads] = r.o.y, prep[10 * kLdsThreads] = r.o.z;
  prep[11 * kLdsThreads] = r.d.x, prep[12 * kLdsThreads] = r.d.y, prep[13 * kLdsThreads] = r.d.z;
#if !DMT_LENS_EARLY
  float const lensR = kargs(Pk)->camTail;
#endif
  if (__builtin_expect(lensR > 0.f, 0)) prepare_lens_ray<PROJ>(Pk, px, py, pixBase, s);  // lens, filter or projection: wave-uniform, laid out of line
  if constexpr (MOTION) motion_set_prepared(motion_sample_time(Pk, pixBase, s));
}
template <bool MOTION = false>
DMT_DEV void path_begin_prepared(PathState& st) {
  float const* const prep = s_prep + threadIdx.x;
  float* const u = s_sampler_u + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) u[k * kLdsThreads] = prep[k * kLdsThreads];
  set_ray(st, mk3(prep[8 * kLdsThreads], prep[9 * kLdsThreads], prep[10 * kLdsThreads]),
          mk3(prep[11 * kLdsThreads], prep[12 * kLdsThreads], prep[13 * kLdsThreads]));
  st.rng.dim = 2;
  st.beta = mk3(1, 1, 1);
  st.L = mk3(0, 0, 0);
  st.depth = 0;
  st.lastT = false;
  st.active = true;
  st.sidx = __float_as_uint(prep[14 * kLdsThreads]);
  if constexpr (MOTION) motion_begin_prepared();
}

#include "launch_device.hpp"

// ---- GGX batching (k_megakernel; dmt_set_ggx_batch) ---------------------------------------------------------------
// The GGX branches of bsdf_prepare, eval_bsdf and sample_bsdf run for the whole wave whenever one lane of a pass has hit
// a GGX material: on Cornell in more than half of the passes, for one or two lanes.  With a batch size T > 0 such a hit
// is PARKED instead of shaded: the lane writes the path into the wave's queue in global memory and is free, so it starts
// its next prepared sample in the next pass like a lane whose path has ended -- a parked path keeps no lane idle.  When the
// queue holds T records, lanes that are free take them back and shade them together, in one pass, through the same
// path_shade call as every other lane.  Entering path_shade for a hit is a pure function of what the record holds (no
// emission is added at a hit in these rows), every sample draws the same sampler dimensions, and the film is folded per
// chunk in sample-index order from the staging slab: films do not depend on T.
// Queue: a LIFO per wave, [field][slot] floats, written and read with plain accesses by its own wave only (one wave's
// vector memory operations on an address complete in order).  Invariants, all wave-uniform:
//   (1) records in the queue == parked0 + parked1 <= kGgxQueueCap; a hit that finds the queue full is shaded at once;
//   (2) a parked path belongs to its item: item `cur` is not retired while the parked count of its slot is non-zero
//       (megakernel_body), so a slot's descriptor and slab outlive every record that names them;
//   (3) when item cur has no units left and has parked paths, free lanes take records back whatever T is, before they
//       start a sample of the next item (megakernel_body): paths end, so lanes fall free and the count reaches zero;
//   (4) hence a wave leaves the loop only with an empty queue: it leaves with no live item, and (2) held for each.
#ifndef DMT_GGX_BATCH_T
#define DMT_GGX_BATCH_T 32  // a context's batch size until dmt_set_ggx_batch / DMT_GGX_BATCH say otherwise (DESIGN.md 4.1 has the sweep)
#endif
constexpr uint32_t kGgxQueueCap = 64;  // records per wave
constexpr uint32_t kGgxFields = 24;    // beta, L, ray direction, tri, bu, bv, depth, staging index, (14 unused), dim | lastT, 8 sampler values
// Wave-uniform state, four scalars.  The hits taken back are not counted on their own: a record leaves the queue only by
// being taken back, so a wave has taken back what it parked minus what its queue holds when it leaves -- which is what
// dmt_sync checks (a wave that left with records in its queue).
struct GgxBatch {
  uint32_t parked = 0;                             // parked paths of the items in slot 0 (low half) and slot 1 (high half)
  uint32_t nParked = 0, nPasses = 0, nFull = 0;    // dmt_ggx_batch_diag: flushed once, when the wave leaves
  DMT_DEV uint32_t queued() const { return (parked & 0xFFFFu) + (parked >> 16); }
  DMT_DEV uint32_t of_slot(uint32_t slot) const { return (parked >> (slot * 16u)) & 0xFFFFu; }
};
DMT_DEV float* ggx_queue(KArgs Pk, uint32_t gtid, uint32_t slot) {
  return kargs(Pk)->ggxQueue + (size_t(wave_index(gtid)) * (kGgxFields * kGgxQueueCap) + slot);
}
DMT_DEV uint32_t lane_rank(unsigned long long m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}
// Called by every lane of a pass after the shadow resolve (lane_finish): parks the lane's hit if it is a GGX hit below the
// bounce cap and the queue has room.  Returns whether the lane shades in this pass.
DMT_DEV bool ggx_park(KArgs Pk, uint32_t gtid, PathState& st, GgxBatch& G, bool doC, int bestTri, float bu, float bv) {
  if (kargs(Pk)->ggxBatchT == 0u) return doC;  // wave-uniform: off (nothing was ever parked, no lane has resumed)
  // The votes of this function are wave masks, each the ballot of ONE compare, combined in scalar registers; a lane takes its
  // own bit back from a mask where it needs it (inverse ballot).  A ballot of anything else -- an `and` of conditions, a lane
  // boolean merged across one of the uniform branches below -- is lowered through a VGPR: v_cndmask 0, 1 and v_cmp_ne 0.
  unsigned long long const mDoC = __ballot(doC);
  // (the compare intrinsic: st.depth < 0 has another use below, and a ballot folds only a compare that is its own)
  unsigned long long const mResumed = __builtin_amdgcn_sicmp(st.depth, 0, 40 /* signed < */) & mDoC;  // (ggx_resumed)
  if (st.depth < 0) st.depth = ~st.depth;
  // Whether the hit's material is a GGX one is a bit of the per-triangle table made at upload (SurfaceState::Kind): from the
  // kernel arguments for soups of at most 64 triangles -- scalar loads, no vector memory -- and one load from the array
  // otherwise (wave-uniform branch).  Neither the triangle's record nor the material's is read before path_shade, and
  // nothing here waits for the staging store the shadow resolve has just issued.  (tri: a lane without a hit reads
  // triangle 0's word; the array holds >= 1 word.)
  uint32_t const tri = uint32_t(bestTri < 0 ? 0 : bestTri);
  unsigned long long m = mDoC & ~mResumed & __ballot(bestTri >= 0) & __ballot(st.depth < kargs(Pk)->maxDepth);
  {
    KArgs const k = kargs(Pk);
    if (uint32_t const* const bits = k->triKindBits) {
      m &= __ballot(((bits[tri >> 5] >> (tri & 31u)) & 1u) != 0u);
    } else {
      uint32_t w0 = k->triKindInline[0], w1 = k->triKindInline[1];
      asm volatile("" : "+s"(w0), "+s"(w1));  // both words by scalar load: a select of the two addresses becomes a vector load
      uint32_t const word = (tri & 32u) != 0u ? w1 : w0;
      m &= __ballot(((word >> (tri & 31u)) & 1u) != 0u);
    }
  }
  unsigned long long mPark = 0ull;
  if (m != 0ull) {
    uint32_t const q = G.queued();
    uint32_t const room = kGgxQueueCap - q;  // invariant (1): q <= kGgxQueueCap
    uint32_t const want = uint32_t(__popcll(m));
    uint32_t const n = want < room ? want : room;
    uint32_t const rank = lane_rank(m);
    mPark = m & __ballot(rank < room);  // queue full: shade now
    if (__builtin_amdgcn_inverse_ballot_w64(mPark)) {
      float* const r = ggx_queue(Pk, gtid, q + rank);  // slot q + rank < q + room == kGgxQueueCap
      float const* const u = s_sampler_u + threadIdx.x;
      r[0 * kGgxQueueCap] = st.beta.x, r[1 * kGgxQueueCap] = st.beta.y, r[2 * kGgxQueueCap] = st.beta.z;
      r[3 * kGgxQueueCap] = st.L.x, r[4 * kGgxQueueCap] = st.L.y, r[5 * kGgxQueueCap] = st.L.z;
      r[6 * kGgxQueueCap] = st.rp.dx.x, r[7 * kGgxQueueCap] = st.rp.dy.x, r[8 * kGgxQueueCap] = st.rp.dz.x;
      r[9 * kGgxQueueCap] = __int_as_float(bestTri), r[10 * kGgxQueueCap] = bu, r[11 * kGgxQueueCap] = bv;
      r[12 * kGgxQueueCap] = __int_as_float(st.depth), r[13 * kGgxQueueCap] = __uint_as_float(st.sidx);
      r[15 * kGgxQueueCap] = __uint_as_float(uint32_t(st.rng.dim) | (st.lastT ? 0x100u : 0u));
#pragma unroll
      for (uint32_t d = 0; d < 8; ++d) r[(16 + d) * kGgxQueueCap] = u[d * kLdsThreads];
      st.active = false;  // the lane is free: it starts its prepared sample in the next pass
    }
    uint32_t const n1 = uint32_t(__popcll(mPark & __ballot((st.sidx >> 31) != 0u)));
    G.parked += (n - n1) + (n1 << 16), G.nParked += n, G.nFull += want - n;  // want - n hits found the queue full
  }
  if ((mResumed | (m & ~mPark)) != 0ull) ++G.nPasses;  // a pass that runs the GGX branches
  return __builtin_amdgcn_inverse_ballot_w64(mDoC & ~mPark);  // (as `doC && !park` of lane booleans the kernel spills 17 VGPRs)
}
// Free lanes take the newest records of the queue back (the caller has decided that they should): a lane restores the
// path and shades the hit in this pass without tracing a closest ray (lane_step).
DMT_DEV void ggx_resume(KArgs Pk, uint32_t gtid, PathState& st, GgxBatch& G) {
  uint32_t const q = G.queued();
  unsigned long long const m = __ballot(!st.active);
  if (m == 0ull) return;
  uint32_t const have = uint32_t(__popcll(m));
  uint32_t const n = have < q ? have : q;
  uint32_t const rank = lane_rank(m);
  unsigned long long const mPop = m & __ballot(rank < q);  // (a mask, like ggx_park's votes)
  if (__builtin_amdgcn_inverse_ballot_w64(mPop)) {
    float const* const r = ggx_queue(Pk, gtid, q - 1u - rank);  // slot in [q - n, q), q <= kGgxQueueCap
    float* const u = s_sampler_u + threadIdx.x;
    st.beta = mk3(r[0 * kGgxQueueCap], r[1 * kGgxQueueCap], r[2 * kGgxQueueCap]);
    st.L = mk3(r[3 * kGgxQueueCap], r[4 * kGgxQueueCap], r[5 * kGgxQueueCap]);
    st.rp.dx.x = r[6 * kGgxQueueCap], st.rp.dy.x = r[7 * kGgxQueueCap], st.rp.dz.x = r[8 * kGgxQueueCap];
    st.rp.ox.x = r[9 * kGgxQueueCap], st.rp.oy.x = r[10 * kGgxQueueCap], st.rp.oz.x = r[11 * kGgxQueueCap];  // tri (as bits), bu, bv
    st.depth = ~__float_as_int(r[12 * kGgxQueueCap]);  // the mark of a lane that has resumed
    st.sidx = __float_as_uint(r[13 * kGgxQueueCap]);
    uint32_t const flags = __float_as_uint(r[15 * kGgxQueueCap]);
    st.rng.dim = int(flags & 0xFFu), st.lastT = (flags & 0x100u) != 0u;
#pragma unroll
    for (uint32_t d = 0; d < 8; ++d) u[d * kLdsThreads] = r[(16 + d) * kGgxQueueCap];
    st.active = true;
  }
  uint32_t const n1 = uint32_t(__popcll(mPop & __ballot((st.sidx >> 31) != 0u)));
  G.parked -= (n - n1) + (n1 << 16);
}

template <bool STATS>
DMT_DEV void flush_stats(KArgs Pk, LaneStats const& ls) {
  if constexpr (STATS) {
    unsigned long long* const stats = kargs(Pk)->stats;
    atomicAdd(&stats[0], (unsigned long long)ls.samples);
    atomicAdd(&stats[1], (unsigned long long)ls.closest);
    atomicAdd(&stats[2], (unsigned long long)ls.shadow);
    atomicAdd(&stats[3], (unsigned long long)ls.tc.nodes);
    atomicAdd(&stats[4], (unsigned long long)ls.tc.tris);
    atomicAdd(&stats[5], (unsigned long long)ls.bounces);
    atomicAdd(&stats[6], (unsigned long long)ls.itNode);
    atomicAdd(&stats[7], (unsigned long long)ls.itLeaf);
    atomicAdd(&stats[8], (unsigned long long)ls.itShade);
    atomicAdd(&stats[9], (unsigned long long)ls.itOuter);
    atomicAdd(&stats[10], (unsigned long long)ls.itPrep);
    atomicAdd(&stats[11], (unsigned long long)ls.lanesLeaf);
    atomicAdd(&stats[12], (unsigned long long)ls.lanesShade);
    atomicAdd(&stats[13], (unsigned long long)ls.lanesPrep);
    atomicAdd(&stats[14], (unsigned long long)ls.tc.deadNodes);
    atomicAdd(&stats[15], (unsigned long long)ls.tc.overflowPushes);
  }
}

template <uint32_t F>
DMT_DEV void megakernel_body() {
  static_assert(!(F & kFeatBvh), "BVH kernels run megakernel_body_bvh");
  constexpr bool STATS = (F & kFeatStats) != 0;
  constexpr bool MOTION = (F & kFeatMotion) != 0;
  KArgs const Pk = kargs_base();
  LaneStats ls;
  int const lane = int(threadIdx.x) & 63;
  uint32_t const gtid = blockIdx.x * blockDim.x + threadIdx.x;
  WaveSched W;
  LaneSched Ls;
  PathState st{};
  auto sink = [&](f3 L, uint32_t sidx) { stage_sample(Pk, sidx, L); };
#if DMT_SECTION_TIMING
  if (lane == 0) s_sectLast[threadIdx.x >> 6] = __builtin_readcyclecounter();  // (LDS is not zeroed: without this, start-up holds what the block before left there)
#endif
  if constexpr (!MOTION && !(F & kFeatCutout)) cull_stage(Pk);  // (the motion pass is the plain loop: the clusters' bounds are of key 0; so is the cutout pass)
#if DMT_SECTION_TIMING
  if (lane < 16) s_sectAcc[threadIdx.x >> 6][lane] = 0;
  sect_mark(15);
#endif
  // GGX batching: the plain row only.  (k_megakernel_env could park its hits as well -- lastPdf and lastSpecular would ride in
  // the record -- but with the code it needs 44 bytes of scratch instead of 16, so it is compiled as it was)
  constexpr bool BATCH = F == 0;
  GgxBatch G;
  {
    for (;;) {
      if constexpr (BATCH) {
        // Free lanes take parked hits back BEFORE they start a sample: when the queue holds a batch, or (invariant 3)
        // when item cur has no units left and still has parked paths -- those are drained whatever T is, so that cur
        // can be retired; records of item cur + 1 that lie above them in the LIFO come back with them.  The same when
        // the item units are drawn from has none left: a free lane would have nothing else to start.
        uint32_t const q = G.queued();
        if (q != 0u) {  // (never with T == 0)
          uint32_t const ofCur = G.of_slot(W.cur & 1u);
          bool const drain = W.nextUnit == W.totalUnits || (W.alloc != W.cur && ofCur != 0u);
          if (drain || q >= kargs(Pk)->ggxBatchT) ggx_resume(Pk, gtid, st, G);
        }
      }
      bool const needPrep = !Ls.prepared;
      bool const starving = !st.active && needPrep;
      if (__any(starving) || __popcll(__ballot(needPrep)) >= DMT_PREP_THRESHOLD) {
        if constexpr (BATCH) {
          // The lane index goes through an opaque copy: item_fetch forms an LDS address from it (s_pixbase + lane) that is
          // otherwise hoisted out of this loop and kept in a VGPR across it, the one register the kernel does not have
          // (make asm: 8 bytes of scratch, that address spilled at kernel start).  The copy is one move per call.
          int l = lane;
          asm volatile("" : "+v"(l));
          sched_draw<MOTION, projection_row(F)>(Pk, gtid, l, W, Ls, needPrep);
        } else {
          sched_draw<MOTION, projection_row(F)>(Pk, gtid, lane, W, Ls, needPrep);
        }
      }
      if (W.cur == W.fetched) break;  // nothing live and nothing fetched: the launch has no more items (invariant 4: nothing parked)
      if (!st.active && Ls.prepared) {
        path_begin_prepared<MOTION>(st);
        Ls.prepared = false;
        if constexpr (STATS) ++ls.samples;
      }
      sect_mark(0);
      if (W.alloc != W.cur || W.nextUnit == W.totalUnits) {  // item cur has no units left: is it complete?
        // (invariant 2: not while one of its paths is parked -- that path's sample is not staged yet)
        // Spelled twice on purpose.  With one statement and the parked term in its condition -- as `!held && !__any(..)` or as
        // `!__any(held || ..)`, `held` a constant false in the other rows -- every brute-force row that does not batch changed
        // its register allocation (make asm: k_megakernel_tex 40 -> 84 bytes of scratch, k_megakernel_area 4 -> 12 spilled
        // SGPRs); with the parent's statement kept as it is they compile as before.  An edit to one copy belongs in the other.
        if constexpr (BATCH) {
          if (G.of_slot(W.cur & 1u) == 0u && !__any(lane_holds(st, Ls, (W.cur & 1u) != 0u))) {
            bool const more = sched_retire(Pk, gtid, lane, W);
            sect_mark(1);
            if (!more) break;
            continue;
          }
        } else if (!__any(lane_holds(st, Ls, (W.cur & 1u) != 0u))) {
          bool const more = sched_retire(Pk, gtid, lane, W);  // fold it, or hand it over (never waits for another wave's item)
          sect_mark(1);
          if (!more) break;
          continue;
        }
      }
      sect_mark(1);
      if constexpr (BATCH)
        lane_step<F>(Pk, gtid, st, sink, nullptr, [&](bool doC, int tri, float bu, float bv) {
          return ggx_park(Pk, gtid, st, G, doC, tri, bu, bv);
        });
      else
        lane_step<F>(Pk, gtid, st, sink, STATS ? &ls : nullptr);
    }
  }
  if constexpr (BATCH) {  // (both exits of the loop are taken with no live item: the queue is empty)
    unsigned long long* const D = kargs(Pk)->schedDiag;
    int const first = int(lane_rank(~0ull));  // 0 in lane 0; formed here, so that nothing of it is live across the loop
    if (G.nParked != 0u) sched_count(D, first, SD_GGX_PARKED, G.nParked), sched_count(D, first, SD_GGX_RESUMED, G.nParked - G.queued());
    if (G.nPasses != 0u) sched_count(D, first, SD_GGX_PASSES, G.nPasses);
    if (G.nFull != 0u) sched_count(D, first, SD_GGX_FULL, G.nFull);
  }
#if DMT_SECTION_TIMING
  if (lane < 16) atomicAdd(&g_sect[lane], s_sectAcc[threadIdx.x >> 6][lane]);
#endif
  flush_stats<STATS>(Pk, ls);
}

#ifndef DMT_BVH_NODE_WEIGHT
#define DMT_BVH_NODE_WEIGHT 1  // a node step is chosen when nNode * NODE_WEIGHT >= nLeaf * LEAF_WEIGHT: a leaf step (one
#define DMT_BVH_LEAF_WEIGHT 2  // pair test) costs about half a node step, so it pays from half as many lanes (measured best)
#endif
#ifndef DMT_BVH_SHADE_THRESHOLD
#define DMT_BVH_SHADE_THRESHOLD 32
#endif
// BVH flavour of the megakernel.  Same items, same sample order, same film as megakernel_body, but the
// traversal is asynchronous per lane (bvh_device.hpp: trav_step): every loop iteration advances each
// traversing lane by one node or leaf, lanes that have finished both of their rays wait for shading, and
// shading runs for all waiting lanes at once when at least DMT_BVH_SHADE_THRESHOLD of them are waiting (or
// nobody is traversing).  Incoherent rays take very different numbers of steps; with a pass-synchronous
// loop the wave ran at 14 % lane utilisation.
#ifndef DMT_BVH_DUMMY_LDS
#define DMT_BVH_DUMMY_LDS 0  // occupancy experiments: extra LDS bytes per block (fewer resident blocks per CU)
#endif
template <uint32_t F>
DMT_DEV void megakernel_body_bvh() {
  static_assert((F & kFeatBvh) != 0, "brute-force kernels run megakernel_body");
  constexpr bool STATS = (F & kFeatStats) != 0;
  constexpr bool MOTION = (F & kFeatMotion) != 0;
  KArgs const Pk = kargs_base();
#if DMT_BVH_DUMMY_LDS > 0
  __shared__ volatile char s_dummy[DMT_BVH_DUMMY_LDS];
  if (threadIdx.x == 0) s_dummy[blockIdx.x % DMT_BVH_DUMMY_LDS] = 1;
#endif
  LaneStats ls;
  int const lane = int(threadIdx.x) & 63;
  uint32_t const gtid = blockIdx.x * blockDim.x + threadIdx.x;
  WaveSched W;
  LaneSched Ls;
  PathState st{};
  auto sink = [&](f3 L, uint32_t sidx) { stage_sample(Pk, sidx, L); };
  Traversal tv{};
  tv.phase = TR_IDLE;
  if constexpr (STATS) tv.stack.ovfCount = &ls.tc.overflowPushes;
  {
    for (;;) {
      // A. draw + prepare units, start samples (only lanes between rounds start one)
      bool const idle = tv.phase == TR_IDLE;
      bool const needPrep = !Ls.prepared;
      bool const starving = idle && !st.active && needPrep;
      if (__any(starving) || __popcll(__ballot(needPrep)) >= DMT_PREP_THRESHOLD) {
        if constexpr (STATS) ++ls.itPrep, ls.lanesPrep += needPrep ? 1u : 0u;
        sched_draw<MOTION, projection_row(F)>(Pk, gtid, lane, W, Ls, needPrep);
      }
      if (W.cur == W.fetched) break;  // nothing live and nothing fetched: the launch has no more items
      if constexpr (STATS) ++ls.itOuter;
      if (idle && !st.active && Ls.prepared) {
        path_begin_prepared<MOTION>(st);
        Ls.prepared = false;
        if constexpr (STATS) ++ls.samples;
      }
      // B. start a round: pending shadow ray first, then the closest-hit ray.  The ray being traversed is ALWAYS st.rp's
      //    .x half (the traversal keeps no copy of it): a round with a shadow ray swaps the halves, and swaps them back when
      //    the shadow ray is done, so that the closest-hit ray is in .x again when the lane shades.
      if (idle && (st.active || st.hasShadow)) {
        // (what the round consists of is st.active / st.hasShadow themselves: nothing changes them before the lane shades)
        tv.bestTri = -1, tv.bu = 0.f, tv.bv = 0.f;
        if (st.hasShadow) {
          tv.phase = TR_SHADOW;
          swap_rays(st);
        } else {
          tv.phase = TR_CLOSEST;
        }
        trav_set_ray(tv, ray_org(st), ray_dir(st), st.hasShadow ? st.smax : kInf);
        if constexpr (STATS) ls.closest += st.active ? 1u : 0u, ls.shadow += st.hasShadow ? 1u : 0u;
      }
      // R. item cur has no units left: is it complete?
      if (W.alloc != W.cur || W.nextUnit == W.totalUnits) {
        if (!__any(lane_holds(st, Ls, (W.cur & 1u) != 0u))) {
          if (!sched_retire(Pk, gtid, lane, W)) break;
          continue;
        }
      }
      // C. traversal.  Lanes sit on an inner node, on a leaf, or have finished their ray.  Each iteration runs ONE
      //    kind of step -- node or leaf, whichever serves more lanes per instruction (a leaf step costs about half a
      //    node step) -- so a step always serves a good share of the traversing lanes (a plain while-while loop kept running node steps for the last few lanes
      //    that were still descending: 11 % lane utilisation in node steps).  The loop ends when enough lanes
      //    wait for shading.
      BvhView const bvh = load_bvh(Pk);
      // motion rows: a leaf is tested at the time of the ray being traversed -- the pending shadow ray's own while the lane is
      // in its shadow phase -- read from LDS at the leaf step; nothing of it is live across node steps or shading
      auto const leafMotion = [&]() {
        if constexpr (MOTION) return LeafMotion{kargs(Pk)->motion.pairDelta, tv.phase == TR_SHADOW ? motion_time_shadow() : motion_time()};
        else if constexpr (F & kFeatCutout) return LeafCutout{load_cutout(Pk)};  // cutout rows: fetched at the leaf step, live nowhere else
        else return NoMotion{};
      };
      int const shadeThreshold = kargs(Pk)->shadeThreshold > 1 ? kargs(Pk)->shadeThreshold : 1;  // (0 would never let the wave traverse)
      // The words of the node a lane stands on are fetched AHEAD: when a step leaves the lane on an inner node, its loads are
      // issued right there, and the step selection, the other kind of step for the other lanes and the loop overhead run
      // under their latency (1 M triangles: 488 -> 517 Msamples/s, 16 M: 440 -> 466).  Fetched anew here for every lane on a
      // node, so that nothing of it is live while the wave shades.  Measured and lost: a leaf's pair words ahead as well (430 in
      // shared registers, 384 in registers of their own) and the hit nearest child ahead of the stack round trip (449); DESIGN 4.2.5.
      NodeWords nd{};
      if ((tv.phase == TR_CLOSEST || tv.phase == TR_SHADOW) && !(tv.cur & kBvhLeafFlag)) nd = node_fetch(bvh, tv.cur);
      for (;;) {
        bool traversing = tv.phase == TR_CLOSEST || tv.phase == TR_SHADOW;
        if (traversing && tv.cur == kBvhEmpty) {  // ray finished: next ray of the round, or done
          if (tv.phase == TR_SHADOW) {
            swap_rays(st);         // .x = the closest-hit ray again
            st.smax = tv.tlim;     // the shadow ray's verdict (negative = occluded) outlives the closest-hit traversal here
          }
          if (tv.phase == TR_SHADOW && st.active) {
            tv.phase = TR_CLOSEST;
            trav_set_ray(tv, ray_org(st), ray_dir(st), kInf);
            nd = node_fetch(bvh, tv.cur);  // the root
          } else {
            tv.phase = TR_DONE;
            traversing = false;
          }
        }
        bool const onNode = traversing && !(tv.cur & kBvhLeafFlag);
        bool const onLeaf = traversing && (tv.cur & kBvhLeafFlag) != 0u;  // cur != kBvhEmpty here
        int const nNode = __popcll(__ballot(onNode)), nLeaf = __popcll(__ballot(onLeaf));
        if (nNode + nLeaf == 0) break;
        if (__popcll(__ballot(tv.phase == TR_DONE)) >= shadeThreshold) break;
        // (parking a found leaf and carrying on with node steps, Aila & Laine's speculative traversal, was measured here in
        //  round 2 and removed: 8 % fewer wave iterations but 5 % slower, the extra dependent LDS pop lengthens every node step)
#ifdef DMT_BVH_BOTH_STEPS  // experiment: every traversing lane advances every iteration (node and leaf code both run)
        if constexpr (STATS) ++ls.itNode, ++ls.itLeaf, ls.lanesLeaf += onLeaf ? 1u : 0u;
        if (onNode) trav_node<STATS>(bvh, tv, STATS ? &ls.tc : nullptr);
        if (onLeaf) trav_leaf<STATS>(bvh, tv, ray_org(st), ray_dir(st), STATS ? &ls.tc : nullptr, leafMotion());
#else
        if (nNode * DMT_BVH_NODE_WEIGHT >= nLeaf * DMT_BVH_LEAF_WEIGHT) {
          if constexpr (STATS) ++ls.itNode;
          if (onNode) {
            trav_node<STATS>(bvh, tv, nd, STATS ? &ls.tc : nullptr);
            if (!(tv.cur & kBvhLeafFlag)) nd = node_fetch(bvh, tv.cur);
          }
        } else {
          if constexpr (STATS) ++ls.itLeaf, ls.lanesLeaf += onLeaf ? 1u : 0u;
          if (onLeaf) {
            trav_leaf<STATS>(bvh, tv, ray_org(st), ray_dir(st), STATS ? &ls.tc : nullptr, leafMotion());
            if (!(tv.cur & kBvhLeafFlag)) nd = node_fetch(bvh, tv.cur);
          }
        }
#endif
      }
      // D. resolve + shade every lane that has finished its round
      if constexpr (STATS) ++ls.itShade, ls.lanesShade += tv.phase == TR_DONE ? 1u : 0u;
      if (tv.phase == TR_DONE) {
        if constexpr (STATS) ls.bounces += (st.active && tv.bestTri >= 0 && st.depth < kargs(Pk)->maxDepth) ? 1u : 0u;
        lane_finish<F & ~kFeatStats>(Pk, st, st.active, st.hasShadow, tv.bestTri, tv.bu, tv.bv, st.smax < 0.f, sink);
        tv.phase = TR_IDLE;
      }
    }
  }
  flush_stats<STATS>(Pk, ls);
}

// The megakernels, one per feature mask a launch can need: (name suffix, mask, minimum waves per SIMD, body).  The kernel
// calls its body directly (one more inlined level in between changes the generated code).  Separate kernels, so that one
// combination's register allocation never touches another's.  No suffix: brute force, the reference's semantics; _bvh: 16 KB
// more LDS per block for the traversal stacks; _blend: a second prepared BSDF per lane, one wave per SIMD fewer than _tex.
// _vn: the parent row's body and bounds with a shading normal of its own (three more live VGPRs through path_shade, as the
// _tex rows already carry); _env_vn and _bvh_env_vn run one wave per SIMD fewer than _env / _bvh_env, which is what keeps
// them within their parents' scratch.
// _cut: the parent _tex row's body with the cutout trace, one wave per SIMD fewer than the parent: at the parents' bounds
// (where the parents themselves spill) the rows would spill VGPRs; at these they do not.
// _medium: the static twin's body with the medium's code in path_shade.  _bvh_medium and _bvh_env_medium keep their twins'
// bounds; _medium and _env_medium run one wave per SIMD fewer than theirs: at four they spill 8 and 15 VGPRs (36 and 48
// bytes of scratch, where k_megakernel has none).
// _medium_grid: the _medium twin's body with the voxel march in place of the closed forms.  Three rows keep their twins'
// bounds; _bvh_env_medium_grid runs one wave per SIMD fewer than _bvh_env_medium: at three it spills 2 VGPRs (8 bytes of
// scratch).
// _rgb: the grey twin's body with the spectrum's event and per-channel transmittances (medium.hpp).  Seven rows keep their
// twins' bounds; _bvh_env_medium_rgb runs one wave per SIMD fewer than _bvh_env_medium: at three it spills 1 VGPR (8 bytes
// of scratch).
// _etree: the _area twin's body with the emitter tree's walk in path_shade (et_select at the hit, et_pmf at an emitter hit)
// and the previous vertex in 6 KB more LDS per block (s_prev).  The walk holds both children of a level, six quads, in
// flight: 13 to 28 more VGPRs than the twin (149 / 181 / 156 / 188 against 128 / 168 / 128 / 168).  At the twins' bounds
// (4 / 3) the compiler cannot fit that without spilling and misses the bound instead; each row runs one wave per SIMD
// fewer (3 / 2), where it uses no scratch.
#define DMT_MEGAKERNELS(X)                                                          \
  X(, 0, DMT_MIN_WAVES_PER_SIMD, megakernel_body)                                   \
  X(_bvh, kFeatBvh, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh)                \
  X(_env, kFeatEnv, 4, megakernel_body)                                             \
  X(_bvh_env, kFeatBvh | kFeatEnv, 3, megakernel_body_bvh)                          \
  X(_area, kFeatArea, 4, megakernel_body)                                           \
  X(_bvh_area, kFeatBvh | kFeatArea, 3, megakernel_body_bvh)                        \
  X(_env_area, kFeatEnv | kFeatArea, 4, megakernel_body)                            \
  X(_bvh_env_area, kFeatBvh | kFeatEnv | kFeatArea, 3, megakernel_body_bvh)         \
  X(_tex, kFeatTex, 4, megakernel_body)                                             \
  X(_bvh_tex, kFeatBvh | kFeatTex, 3, megakernel_body_bvh)                          \
  X(_env_tex, kFeatEnv | kFeatTex, 4, megakernel_body)                              \
  X(_bvh_env_tex, kFeatBvh | kFeatEnv | kFeatTex, 3, megakernel_body_bvh)           \
  X(_blend, kFeatBlend, 3, megakernel_body)                                         \
  X(_bvh_blend, kFeatBvh | kFeatBlend, 2, megakernel_body_bvh)                      \
  X(_env_blend, kFeatEnv | kFeatBlend, 3, megakernel_body)                          \
  X(_bvh_env_blend, kFeatBvh | kFeatEnv | kFeatBlend, 2, megakernel_body_bvh)       \
  X(_area_etree, kFeatArea | kFeatEmitterTree, 3, megakernel_body)                  \
  X(_bvh_area_etree, kFeatBvh | kFeatArea | kFeatEmitterTree, 2, megakernel_body_bvh) \
  X(_env_area_etree, kFeatEnv | kFeatArea | kFeatEmitterTree, 3, megakernel_body)   \
  X(_bvh_env_area_etree, kFeatBvh | kFeatEnv | kFeatArea | kFeatEmitterTree, 2, megakernel_body_bvh) \
  X(_ltree, kFeatLightTree, 4, megakernel_body)                                     \
  X(_bvh_ltree, kFeatBvh | kFeatLightTree, 3, megakernel_body_bvh)                  \
  X(_env_ltree, kFeatEnv | kFeatLightTree, 4, megakernel_body)                      \
  X(_bvh_env_ltree, kFeatBvh | kFeatEnv | kFeatLightTree, 3, megakernel_body_bvh)   \
  X(_ltree2, kFeatLightTreeRef, 3, megakernel_body)                                 \
  X(_bvh_ltree2, kFeatBvh | kFeatLightTreeRef, 2, megakernel_body_bvh)              \
  X(_env_ltree2, kFeatEnv | kFeatLightTreeRef, 3, megakernel_body)                  \
  X(_bvh_env_ltree2, kFeatBvh | kFeatEnv | kFeatLightTreeRef, 2, megakernel_body_bvh)   \
  X(_texf, kFeatTex | kFeatTexFilter, 2, megakernel_body)                           \
  X(_bvh_texf, kFeatBvh | kFeatTex | kFeatTexFilter, 2, megakernel_body_bvh)        \
  X(_env_texf, kFeatEnv | kFeatTex | kFeatTexFilter, 2, megakernel_body)            \
  X(_bvh_env_texf, kFeatBvh | kFeatEnv | kFeatTex | kFeatTexFilter, 2, megakernel_body_bvh) \
  X(_blendf, kFeatBlend | kFeatTexFilter, 2, megakernel_body)                       \
  X(_bvh_blendf, kFeatBvh | kFeatBlend | kFeatTexFilter, 2, megakernel_body_bvh)    \
  X(_env_blendf, kFeatEnv | kFeatBlend | kFeatTexFilter, 2, megakernel_body)        \
  X(_bvh_env_blendf, kFeatBvh | kFeatEnv | kFeatBlend | kFeatTexFilter, 2, megakernel_body_bvh) \
  X(_motion, kFeatMotion, 4, megakernel_body)                                       \
  X(_bvh_motion, kFeatBvh | kFeatMotion, 3, megakernel_body_bvh)                    \
  X(_env_motion, kFeatEnv | kFeatMotion, 4, megakernel_body)                        \
  X(_bvh_env_motion, kFeatBvh | kFeatEnv | kFeatMotion, 3, megakernel_body_bvh)      \
  X(_vn, kFeatVtxNormals, DMT_MIN_WAVES_PER_SIMD, megakernel_body)                  \
  X(_bvh_vn, kFeatBvh | kFeatVtxNormals, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh) \
  X(_env_vn, kFeatEnv | kFeatVtxNormals, 3, megakernel_body)                        \
  X(_bvh_env_vn, kFeatBvh | kFeatEnv | kFeatVtxNormals, 2, megakernel_body_bvh)     \
  X(_tex_vn, kFeatTex | kFeatVtxNormals, 4, megakernel_body)                        \
  X(_bvh_tex_vn, kFeatBvh | kFeatTex | kFeatVtxNormals, 3, megakernel_body_bvh)     \
  X(_env_tex_vn, kFeatEnv | kFeatTex | kFeatVtxNormals, 4, megakernel_body)         \
  X(_bvh_env_tex_vn, kFeatBvh | kFeatEnv | kFeatTex | kFeatVtxNormals, 3, megakernel_body_bvh) \
  X(_tex_cut, kFeatTex | kFeatCutout, 3, megakernel_body)                           \
  X(_bvh_tex_cut, kFeatBvh | kFeatTex | kFeatCutout, 2, megakernel_body_bvh)        \
  X(_env_tex_cut, kFeatEnv | kFeatTex | kFeatCutout, 3, megakernel_body)            \
  X(_bvh_env_tex_cut, kFeatBvh | kFeatEnv | kFeatTex | kFeatCutout, 2, megakernel_body_bvh) \
  X(_medium, kFeatMedium, 3, megakernel_body)                                       \
  X(_bvh_medium, kFeatBvh | kFeatMedium, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh) \
  X(_env_medium, kFeatEnv | kFeatMedium, 3, megakernel_body)                        \
  X(_bvh_env_medium, kFeatBvh | kFeatEnv | kFeatMedium, 3, megakernel_body_bvh) \
  X(_medium_grid, kFeatMedium | kFeatMediumGrid, 3, megakernel_body)                \
  X(_bvh_medium_grid, kFeatBvh | kFeatMedium | kFeatMediumGrid, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh) \
  X(_env_medium_grid, kFeatEnv | kFeatMedium | kFeatMediumGrid, 3, megakernel_body) \
  X(_bvh_env_medium_grid, kFeatBvh | kFeatEnv | kFeatMedium | kFeatMediumGrid, 2, megakernel_body_bvh) \
  X(_medium_rgb, kFeatMedium | kFeatMediumSpectrum, 3, megakernel_body)             \
  X(_bvh_medium_rgb, kFeatBvh | kFeatMedium | kFeatMediumSpectrum, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh) \
  X(_env_medium_rgb, kFeatEnv | kFeatMedium | kFeatMediumSpectrum, 3, megakernel_body) \
  X(_bvh_env_medium_rgb, kFeatBvh | kFeatEnv | kFeatMedium | kFeatMediumSpectrum, 2, megakernel_body_bvh) \
  X(_medium_grid_rgb, kFeatMedium | kFeatMediumGrid | kFeatMediumSpectrum, 3, megakernel_body) \
  X(_bvh_medium_grid_rgb, kFeatBvh | kFeatMedium | kFeatMediumGrid | kFeatMediumSpectrum, DMT_MIN_WAVES_PER_SIMD_BVH, megakernel_body_bvh) \
  X(_env_medium_grid_rgb, kFeatEnv | kFeatMedium | kFeatMediumGrid | kFeatMediumSpectrum, 3, megakernel_body) \
  X(_bvh_env_medium_grid_rgb, kFeatBvh | kFeatEnv | kFeatMedium | kFeatMediumGrid | kFeatMediumSpectrum, 2, megakernel_body_bvh)
// the same bodies with per-lane work counters (node visits, triangle tests, rays, bounces): they feed the
// algorithmic-bytes model of the BVH path (dmt_render_stats) and are never on the timed path
#define DMT_STATS_MEGAKERNELS(X)                                                    \
  X(_bvh_stats, kFeatBvh | kFeatStats, 2, megakernel_body_bvh)                      \
  X(_bvh_stats_env, kFeatBvh | kFeatStats | kFeatEnv, 2, megakernel_body_bvh)

#define DMT_DEFINE_MEGAKERNEL(suffix, mask, waves, body) \
  __global__ void __launch_bounds__(256, waves) k_megakernel##suffix(RenderParams P) { body<mask>(); }
DMT_MEGAKERNELS(DMT_DEFINE_MEGAKERNEL)
DMT_STATS_MEGAKERNELS(DMT_DEFINE_MEGAKERNEL)

// Fills the sampler table of a launch (RenderParams::samTab): one thread per entry (sample s0 + k, period pixel (x, y)),
// with the functions prepare_sample's compute path calls, so that a loaded sample is the computed one bit for bit.
// `lens` (null without a lens): the third plane, lens_values of the entry's Halton index.  `knots` (null without a pixel
// filter): the jitter is warped by the filter before it is stored.
__global__ void __launch_bounds__(256) k_sampler_table(SamplerParams sp, uint32_t s0, uint32_t n, uint32_t pw, uint32_t ph,
                                                       float4* vals, float2* jit, float2* lens, FilterBin const* knots, float filtR) {
  uint32_t const e = blockIdx.x * 256u + threadIdx.x;  // (entries < 2^31: samplerTablePlan)
  if (e >= n * pw * ph) return;
  uint32_t const x = e % pw, row = e / pw, y = row % ph, k = row / ph;
  int32_t const hidx = halton_pixel_base(sp, int(x), int(y)) + int32_t(s0 + k) * (sp.scale0 * sp.scale1);
  float* const u = s_sampler_u + threadIdx.x;
  sampler_values(uint32_t(hidx), u);
  vals[2 * size_t(e)] = make_float4(u[0 * kLdsThreads], u[1 * kLdsThreads], u[2 * kLdsThreads], u[3 * kLdsThreads]);
  vals[2 * size_t(e) + 1] = make_float4(u[4 * kLdsThreads], u[5 * kLdsThreads], u[6 * kLdsThreads], u[7 * kLdsThreads]);
  f2 p = pixel2d(sp, hidx);
  if (knots) p = f2{filter_warp(knots, filtR, p.x), filter_warp(knots, filtR, p.y)};  // the jitter plane holds the warped jitter
  jit[e] = make_float2(p.x, p.y);
  if (lens) {
    LensU const u = lens_values(uint32_t(hidx));
    lens[e] = make_float2(u.x, u.y);
  }
}

// ---- adaptive sampling (dmt_render_adaptive) --------------------------------------------------------
// Stopping rule, fp32: a pixel with N = M2.w samples has the relative standard error of its mean
//   err = sqrt((M2.x + M2.y + M2.z) / (N (N - 1))) / max(mean.x + mean.y + mean.z, 1e-3)     (+inf for N < 2)
// and takes part in the round that starts at sample `offset` iff
//   N == offset && N < maxSpp && (N < minSpp || err > threshold).
// N == offset: a pixel is traced only while it holds exactly samples [0, offset), so it drops out for good and a film
// that was not cleared is never counted twice; its film then equals a uniform film of N samples bit for bit.
DMT_DEV bool adaptive_active(float4 m, float4 v, uint32_t offset, uint32_t minSpp, uint32_t maxSpp, float threshold) {
  float const N = v.w;
  if (N != float(offset) || !(N < float(maxSpp))) return false;
  if (N < float(minSpp) || N < 2.f) return true;
  float const err = sqrtf((v.x + v.y + v.z) / (N * (N - 1.f))) / fmaxf(m.x + m.y + m.z, 1e-3f);
  return err > threshold;
}
struct AdaptiveArgs {
  float4 const* mean;
  float4 const* m2;
  unsigned long long* mask;  // [region tile] the tile's active pixels, bit y * 8 + x
  uint32_t* list;            // [k < counters[0]] region tiles with at least one active pixel, in no particular order
  uint32_t* counters;        // {listed tiles, active pixels}, zero at launch
  int width, x0, y0, x1, y1, tx0, ty0, rtx;
  uint32_t owned;            // tiles of the region this partition owns
  int rank, world;
  uint32_t offset, minSpp, maxSpp;
  float threshold;
};
// one wave per owned tile (region tile j = rank + w * world, as item_geom), lane = pixel
__global__ void __launch_bounds__(256) k_adaptive_mask(AdaptiveArgs A) {
  uint32_t const w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= A.owned) return;  // whole waves
  int const lane = int(threadIdx.x) & 63;
  uint32_t const j = uint32_t(A.rank) + w * uint32_t(A.world);
  int const px = (A.tx0 + int(j % uint32_t(A.rtx))) * 8 + (lane & 7), py = (A.ty0 + int(j / uint32_t(A.rtx))) * 8 + (lane >> 3);
  bool active = false;
  if (px >= A.x0 && px < A.x1 && py >= A.y0 && py < A.y1) {
    size_t const pidx = size_t(px) + size_t(py) * size_t(A.width);
    active = adaptive_active(film_load(A.mean + pidx), film_load(A.m2 + pidx), A.offset, A.minSpp, A.maxSpp, A.threshold);
  }
  unsigned long long const word = __ballot(active);
  if (lane == 0) {
    A.mask[j] = word;
    if (word != 0ull) {
      A.list[atomicAdd(&A.counters[0], 1u)] = j;
      atomicAdd(&A.counters[1], uint32_t(__popcll(word)));
    }
  }
}

#include "wavefront.hpp"
#include "denoise.hpp"
#include "display.hpp"

}  // namespace

// =============================================================================================
// host side of the C ABI
// =============================================================================================
#include "scene_state.hpp"
#include "camera_state.hpp"
#include "accel_state.hpp"
#include "surface_state.hpp"
#include "medium_state.hpp"
#include "light_state.hpp"
#include "launch_state.hpp"

struct dmt_ctx {
  int device = 0;
  hipStream_t ownStream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  // the scene layer: the triangle soup with its host copy, the BSDF records (scene_state.hpp, scene_host.hpp)
  SceneState scene;
  // the camera layer: the camera and the sampler set-up, the thin lens, the pixel filter; and the film, the context's own or
  // the caller's after dmt_film_bind (camera_state.hpp, camera_host.hpp)
  CameraState camera;
  FilmState film;
  // the acceleration layer: the static and the motion tree, builder and update policy, key 1, the cull tables of the
  // brute-force pass (accel_state.hpp, accel_host.hpp, cull_plan.hpp)
  AccelState ac;
  // the light layer: the light list, the light tree over it and the env map (light_state.hpp, light_host.hpp)
  LightState lights;
  // the surface-attribute layer: textures and UVs, the texture filter, vertex normals, opacity records, emissive triangles
  // (surface_state.hpp, surface_host.hpp)
  SurfaceState surf;
  // the medium layer: the participating medium, its density grid and its spectrum (medium_state.hpp, medium_host.hpp)
  MediumState medium;
  // the launch layer: the scheduler's buffers and fold accounting, GGX batching, the sampler table, adaptive rounds, the
  // wavefront form, timing, and the settings that shape a launch (launch_state.hpp, launch_host.hpp)
  LaunchState launch;
  // the image-space layer: feature planes, the filter's scratch, the temporal history (denoise.hpp, denoise_host.hpp)
  DenoiseState dn;
  // the display transform: its scratch planes, the bloom pyramid, the record of the last call (display.hpp, display_host.hpp)
  DisplayState disp;
  int maxDepth = 32;
  int accel = DMT_ACCEL_BRUTE_FORCE;
};

namespace {

std::string g_createError;

#define HIP_TRY(ctx, call)                                                                 \
  do {                                                                                     \
    hipError_t const e__ = (call);                                                         \
    if (e__ != hipSuccess) {                                                               \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorName(e__) + " - " +              \
                   hipGetErrorString(e__);                                                 \
      return DMT_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

int fail(dmt_ctx* ctx, int code, char const* msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// The feature mask (kFeat*) of what a launch of this context needs.  The light and the medium layer give their own bits; the
// light tree applies to plain surfaces only: textured or emissive-triangle scenes keep the uniform pick.
bool plainSurfaces(dmt_ctx const* c) { return c->surf.area.count == 0 && c->surf.tex.count == 0 && !c->scene.hasBlend; }
uint32_t featuresOf(dmt_ctx const* c) {
  uint32_t F = 0;
  if (c->accel == DMT_ACCEL_BVH) F |= kFeatBvh;
  if (c->surf.area.count > 0) F |= kFeatArea;
  if (c->scene.hasBlend) F |= kFeatBlend;  // the blend kernels carry the texture code too
  else if (c->surf.tex.count > 0) F |= kFeatTex;
  if (c->surf.texFilter == DMT_TEXFILTER_REFERENCE && (F & (kFeatTex | kFeatBlend))) F |= kFeatTexFilter;
  if (c->ac.haveMotion) F |= kFeatMotion;
  if (c->surf.vn.have) F |= kFeatVtxNormals;
  if (c->surf.op.have) F |= kFeatCutout;
  return F | c->lights.features(plainSurfaces(c)) | c->lights.emitterFeatures(c->surf.area.count) | c->medium.features();
}
int ensureLightTree(dmt_ctx* ctx);
int ensureEmitterTree(dmt_ctx* ctx);
// featuresOf once the light tree it asks for is built: a tree deeper than the walk's guard switches the context back to the
// uniform pick (LightState::Tree::tooDeep), which changes the kernel, its occupancy and the launch shape
int resolveFeatures(dmt_ctx* ctx, uint32_t* mask) {
  if (featuresOf(ctx) & (kFeatLightTree | kFeatLightTreeRef)) {
    if (int const rc = ensureLightTree(ctx)) return rc;
  }
  if (featuresOf(ctx) & kFeatEmitterTree) {  // too deep: the bit goes and the *_area rows run
    if (int const rc = ensureEmitterTree(ctx)) return rc;
  }
  *mask = featuresOf(ctx);
  return DMT_OK;
}
// what another projection than the perspective one (dmt_set_projection) refuses of a feature mask: dmt_render*
// (checkFeatures) and the trace probes, which shade with the same bodies
int checkProjection(dmt_ctx* ctx, uint32_t F) {
  if (!projection_row(F) && ctx->camera.projKind != DMT_PROJECTION_PERSPECTIVE)  // the two rows compiled without the projection's tail
    return fail(ctx, DMT_ERR_STATE, (F & kFeatBvh) ? "dmt_render: another projection than the perspective one (dmt_set_projection) together with an env map, the BVH and the light tree is not supported (use the uniform light pick)"
                                                   : "dmt_render: another projection than the perspective one (dmt_set_projection) together with an env map needs the BVH (dmt_set_accel) unless the scene has textures, emissive triangles, motion, vertex normals or a medium");
  if ((F & kFeatTexFilter) && ctx->camera.projKind != DMT_PROJECTION_PERSPECTIVE)  // its footprints are the pinhole's differentials
    return fail(ctx, DMT_ERR_STATE, "dmt_render: the first-hit texture filter together with another projection than the perspective one (dmt_set_projection) is not supported");
  return DMT_OK;
}
// the combinations dmt_render refuses (mask | kFeatStats for dmt_render_stats / dmt_render_profile)
int checkFeatures(dmt_ctx* ctx, uint32_t F) {
  if (int const rc = checkProjection(ctx, F)) return rc;
  if (F & kFeatMedium) {  // the medium has the plain and env-map megakernel rows
    if (F & kFeatStats) return fail(ctx, DMT_ERR_STATE, "dmt_render_stats / dmt_render_profile: a participating medium (dmt_set_medium) has no counting kernels");
    if (F & kFeatArea) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with emissive triangles is not supported");
    if (F & kFeatCutout) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with opacity textures is not supported");
    if (F & kFeatTexFilter) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with the first-hit texture filter is not supported");
    if (F & (kFeatTex | kFeatBlend)) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with image textures or blend materials is not supported");
    if (F & (kFeatLightTree | kFeatLightTreeRef)) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with a light tree is not supported");
    if (F & kFeatMotion) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with motion blur is not supported");
    if (F & kFeatVtxNormals) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with vertex normals is not supported");
    if ((F & kFeatBvh) && ctx->launch.wf.strategy == 2) return fail(ctx, DMT_ERR_STATE, "dmt_render: a participating medium (dmt_set_medium) together with the wavefront BVH strategy is not supported");
  }
  if (F & kFeatCutout) {  // alpha cutouts have the four texture megakernel rows; the rest is refused as for those rows
    if (F & kFeatBlend) return fail(ctx, DMT_ERR_STATE, "dmt_render: opacity textures (dmt_upload_opacity) together with blend materials are not supported");
    if (F & kFeatTexFilter) return fail(ctx, DMT_ERR_STATE, "dmt_render: opacity textures (dmt_upload_opacity) together with the first-hit texture filter are not supported");
    if (F & kFeatVtxNormals) return fail(ctx, DMT_ERR_STATE, "dmt_render: opacity textures (dmt_upload_opacity) together with vertex normals are not supported");
  }
  if (F & kFeatVtxNormals) {  // smooth shading has the plain, env-map and texture megakernel rows
    if (F & kFeatStats) return fail(ctx, DMT_ERR_STATE, "dmt_render_stats / dmt_render_profile: vertex normals (dmt_upload_vertex_normals) have no counting kernels");
    if (F & kFeatMotion) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with motion blur are not supported");
    if (F & kFeatTexFilter) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with the first-hit texture filter are not supported");
    if (F & kFeatBlend) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with blend materials are not supported");
    if (F & kFeatArea) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with emissive triangles are not supported");
    if (F & (kFeatLightTree | kFeatLightTreeRef)) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with a light tree are not supported");
    if ((F & kFeatBvh) && ctx->launch.wf.strategy == 2) return fail(ctx, DMT_ERR_STATE, "dmt_render: vertex normals (dmt_upload_vertex_normals) together with the wavefront BVH strategy are not supported");
  }
  if (F & kFeatMotion) {  // motion blur has the plain and env-map megakernel rows
    if (F & kFeatStats) return fail(ctx, DMT_ERR_STATE, "dmt_render_stats / dmt_render_profile: motion blur (dmt_set_motion) has no counting kernels");
    if (F & kFeatTexFilter) return fail(ctx, DMT_ERR_STATE, "dmt_render: motion blur (dmt_set_motion) together with the first-hit texture filter is not supported");
    if (F & (kFeatTex | kFeatBlend)) return fail(ctx, DMT_ERR_STATE, "dmt_render: motion blur (dmt_set_motion) together with image textures or blend materials is not supported");
    if (F & kFeatArea) return fail(ctx, DMT_ERR_STATE, "dmt_render: motion blur (dmt_set_motion) together with emissive triangles is not supported");
    if (F & (kFeatLightTree | kFeatLightTreeRef)) return fail(ctx, DMT_ERR_STATE, "dmt_render: motion blur (dmt_set_motion) together with a light tree is not supported");
    if ((F & kFeatBvh) && ctx->launch.wf.strategy == 2) return fail(ctx, DMT_ERR_STATE, "dmt_render: motion blur (dmt_set_motion) together with the wavefront BVH strategy is not supported");
  }
  if ((F & kFeatEmitterTree) && (F & kFeatBvh) && ctx->launch.wf.strategy == 2)
    return fail(ctx, DMT_ERR_STATE, "dmt_render: the emitter tree (dmt_set_emitter_sampling) together with the wavefront BVH strategy is not supported");
  if ((F & kFeatEmitterTree) && (F & kFeatStats))
    return fail(ctx, DMT_ERR_STATE, "dmt_render_stats / dmt_render_profile: the emitter tree (dmt_set_emitter_sampling) has no counting kernels");
  if ((F & kFeatStats) && (F & (kFeatTex | kFeatBlend | kFeatArea | kFeatLightTree | kFeatLightTreeRef)))
    return fail(ctx, DMT_ERR_STATE, "dmt_render_stats / dmt_render_profile: the counting kernels exist for the plain and env-map BVH kernels only; "
                                    "with textures, blended materials, emissive triangles or a light tree they would describe a different kernel");
  if ((F & kFeatBlend) && (F & kFeatArea)) return fail(ctx, DMT_ERR_STATE, "dmt_render: fractional-metallic materials together with emissive triangles are not supported");
  if ((F & kFeatTex) && (F & kFeatArea)) return fail(ctx, DMT_ERR_STATE, "dmt_render: image textures together with emissive triangles are not supported");
  if (!ctx->surf.texturesMatch(ctx->scene.bsdfCount, ctx->scene.triCount))
    return fail(ctx, DMT_ERR_STATE, "dmt_render: texture tables do not match the uploaded BSDFs / triangles (upload textures last)");
  return DMT_OK;
}

}  // namespace

// the camera layer's helpers and entry points: the camera and sampler set-up math that the headers below use, the film, the
// thin lens, the pixel filter
#include "camera_host.hpp"

// the acceleration layer: the trees, their builders and updates, key 1 of the motion, the cull tables and the entry points
// that show a cull plan; the helpers below, scene_host.hpp, denoise_host.hpp and probes.hpp call into it
#include "accel_host.hpp"

// the scene layer's helpers and entry points: the records of a soup, dmt_upload_triangles, dmt_upload_bsdfs
#include "scene_host.hpp"

// the surface-attribute layer's helpers and entry points: textures, the texture filter, vertex normals, opacity records,
// emissive triangles, and the first-hit variant chooser that denoise_host.hpp and probes.hpp use
#include "surface_host.hpp"

// the medium layer's helpers and entry points: the medium, its density grid and its spectrum, and the checks and call
// records that probes.hpp uses
#include "medium_host.hpp"

// the light layer's helpers and entry points: the light list, the sampling mode, the one builder of the two light trees
// and the lazy build that resolveFeatures calls, the env map
#include "light_host.hpp"

namespace {

// the layers' parts of the argument struct and the limits (what the path-tracing device code reads)
RenderParams baseParams(dmt_ctx const* c, size_t threads) {
  RenderParams P{};
  c->scene.fill(P);
  P.cull = cullView(c);
  P.bvh = bvhView(c, threads);
  c->camera.fill(P);
  P.maxDepth = c->maxDepth;
  P.shadeThreshold = shadeThresholdFor(c, c->ac.tree.nodeCount);
  c->lights.fill(P, plainSurfaces(c));
  c->lights.fillEmitters(P, c->surf.area.count);
  c->medium.fill(P);
  c->surf.fill(P);
  return P;
}

int finishTest(dmt_ctx* ctx) {
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DMT_OK;
}

}  // namespace

// the launch layer's helpers and entry points: the kernel tables, the plan and the enqueue of a dmt_render* call, the fold
// check (checkErrorFlag) that denoise_host.hpp and probes.hpp use, timing
#include "launch_host.hpp"

// the image-space layer's entry points and the rules of its state; it uses the helpers above
#include "denoise_host.hpp"

// the display transform's entry points and host twins; of the context they read the camera's size, the film and the stream
#include "display_host.hpp"

extern "C" {

int dmt_ctx_create(int device_ordinal, dmt_ctx** out) {
  if (!out) return DMT_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    g_createError = "no HIP device available (the HIP path has no CPU fallback)";
    return DMT_ERR_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= count) {
    g_createError = "device ordinal out of range";
    return DMT_ERR_INVALID;
  }
  std::unique_ptr<dmt_ctx> ctx(new (std::nothrow) dmt_ctx());
  if (!ctx) return DMT_ERR_INVALID;
  ctx->device = device_ordinal;
  hipError_t e = hipSetDevice(device_ordinal);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->ownStream, hipStreamNonBlocking);
  hipDeviceProp_t prop{};
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device_ordinal);
  if (e == hipSuccess) e = ctx->launch.allocate();
  int bpcBvh = 0;
  if (e == hipSuccess)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpcBvh, reinterpret_cast<void const*>(k_megakernel_bvh), 256, 0);
  if (e != hipSuccess) {
    g_createError = std::string("dmt_ctx_create: ") + hipGetErrorString(e);
    if (ctx->ownStream) (void)hipStreamDestroy(ctx->ownStream);
    return DMT_ERR_HIP;
  }
  ctx->stream = ctx->ownStream;
  ctx->launch.cuCount = prop.multiProcessorCount;
  ctx->ac.blocksPerCUBvh = bpcBvh > 0 ? bpcBvh : 1;
  ctx->launch.fromEnv();
  if (char const* e5 = std::getenv("DMT_BVH_SHADE_THRESHOLD")) {  // tuning runs (shadeThresholdFor)
    int const v = std::atoi(e5);
    ctx->ac.shadeThresholdEnv = v < 1 ? 0 : (v > 64 ? 64 : v);
  }
  if (char const* e6 = std::getenv("DMT_BRUTE_CULL")) {  // A/B runs and tests
    int const v = std::atoi(e6);
    ctx->ac.bruteCull = v == 0 ? 0 : v == 1 ? 1 : 2;
  }
  if (char const* e7 = std::getenv("DMT_TRI_KIND_INLINE")) ctx->surf.kind.allowInline = std::atoi(e7) != 0;  // tests (SurfaceState::Kind)
  if (char const* e8 = std::getenv("DMT_UNIFORM_LIGHTS")) ctx->lights.uniformPath = std::atoi(e8) != 0;  // A/B runs and tests (LightState)
  *out = ctx.release();
  return DMT_OK;
}

int dmt_ctx_destroy(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& ev : ctx->launch.timing.events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  if (ctx->ownStream) (void)hipStreamDestroy(ctx->ownStream);
  delete ctx;  // the device buffers free themselves
  return DMT_OK;
}

const char* dmt_last_error(const dmt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int dmt_set_limits(dmt_ctx* ctx, int max_depth) {
  if (!ctx) return DMT_ERR_INVALID;
  if (max_depth < 0) return fail(ctx, DMT_ERR_INVALID, "dmt_set_limits: max_depth < 0");
  ctx->maxDepth = max_depth;
  return DMT_OK;
}

int dmt_set_stream(dmt_ctx* ctx, void* hip_stream) {
  if (!ctx) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->ownStream;
  return DMT_OK;
}

#if DMT_CULL_COUNTS
extern "C" int dmt_diag_cull_counts(unsigned long long* out16, int reset) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_cullCount), 16 * sizeof(unsigned long long));
  if (e == hipSuccess && reset) {
    unsigned long long z[16] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_cullCount), z, sizeof(z));
  }
  return e == hipSuccess ? 0 : -1;
}
#endif
#if DMT_SECTION_TIMING
extern "C" int dmt_diag_section_cycles(unsigned long long* out16, int reset) {
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sect), 16 * sizeof(unsigned long long));
  if (e == hipSuccess && reset) {
    unsigned long long z[16] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_sect), z, sizeof(z));
  }
  return e == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"

// the device probes: the k_test_* kernels and the dmt_test_* entry points
#include "probes.hpp"
