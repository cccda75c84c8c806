// probes.hpp -- the device probes: the k_test_* kernels and the dmt_test_* entry points (include/dmt_hip.h) that run one
// device function over arrays of cases, which is how the tests compare the device code with the oracle function by function.
//
// Part of dmt_hip.hip's translation unit, included once at its end: it uses the device code, dmt_ctx, HIP_TRY, fail,
// baseParams, resolveFeatures / kernelOf and finishTest defined there, accel_host.hpp's requireTree, reserveOverflow and
// motionParams, surface_host.hpp's firstHitVariant, camera_host.hpp's computeSamplerParams, CameraState::extra,
// SceneState::matIdOutside, and denoise_host.hpp's makeProjXf.  A probe: a kernel with one lane per case, an entry point staging its arrays (probe_stage.hpp).
#pragma once

#include "probe_stage.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// dmt_test_trace_samples: the radiance of single samples, shaded by the body of the megakernel row `F` (one instantiation
// per row of DMT_MEGAKERNELS; the BVH rows trace each ray to completion instead of stepping the wave's traversal)
template <uint32_t F>
__global__ void k_test_trace(RenderParams P, int n, int32_t const* pxs, int32_t const* pys, int32_t const* ss, float* L3) {
  KArgs const k = kargs_base();
  if constexpr (!(F & (kFeatBvh | kFeatMotion | kFeatCutout))) cull_stage(k);
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  PathState st{};
  if (i < n) {
    ColdArgs const c = load_cold_args(k);
    path_begin(st, c.cam, c.sp, pxs[i], pys[i], halton_pixel_base(c.sp, pxs[i], pys[i]), uint32_t(ss[i]), load_camera_extra(k));
    if constexpr (F & kFeatMotion) motion_set_time(motion_sample_time(k, halton_pixel_base(c.sp, pxs[i], pys[i]), uint32_t(ss[i])));
    if constexpr (F & kFeatMedium) {  // medium_h: the lane's sample is sample 0 of "pixel" lane of slot 0, whose base is the sample's own index
      st.sidx = threadIdx.x & 63u;
      s_pixbase[threadIdx.x] = halton_pixel_base(c.sp, pxs[i], pys[i]) + ss[i] * (c.sp.scale0 * c.sp.scale1);
      s_desc[threadIdx.x >> 6][0][4] = 0u;
    }
  }
  auto store = [&](f3 L, uint32_t) { L3[3 * i] = L.x, L3[3 * i + 1] = L.y, L3[3 * i + 2] = L.z; };
  uint32_t const gtid = blockIdx.x * blockDim.x + threadIdx.x;
  while (__any(st.active || st.hasShadow)) lane_step<F>(k, gtid, st, store);
}

// first-hit texture filter probes: the lookup of texture `tex` at (tri, bu, bv) by the *_texf kernels' device code, as at a
// hit of depth `depth` (0: the camera ray's, filtered; otherwise level 0)
__global__ void k_test_texfilter(RenderParams P, int n, int32_t const* tri, float const* bu, float const* bv, int32_t const* tex,
                                 int32_t const* depth, float* rgb3, int32_t* branch, float* lod) {
#pragma clang fp contract(off)  // (s, t) rounded as a plain float restatement rounds them
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  TriPost const T = load_scene(k).post[tri[i]];
  Hit const hit = hit_finish(T, bu[i], bv[i], mk3(0.f, 0.f, 1.f));
  TexDiff td{0.f, 0.f, 0.f, 0.f};
  if (depth[i] == 0) td = tex_footprint(k, tri[i], hit.pos, hit.normal);
  float const* const uv = kargs(k)->triUv + 6 * size_t(tri[i]);
  float const w0 = 1.f - bu[i] - bv[i];
  float const s = w0 * uv[0] + bu[i] * uv[2] + bv[i] * uv[4], t = w0 * uv[1] + bu[i] * uv[3] + bv[i] * uv[5];
  TexProbe pr{0, 0.f};
  f3 const c = tex_filtered<true>(k, tex[i], s, t, false, td, &pr);
  rgb3[3 * i] = c.x, rgb3[3 * i + 1] = c.y, rgb3[3 * i + 2] = c.z;
  branch[i] = pr.branch, lod[i] = pr.lod;
}

// A18 probes: env-map sampling (u2 -> wi, pdf, uv, Le by uv) and evaluation by direction (wi -> Le, pdf)
__global__ void k_test_envmap(EnvView env, int n, float const* u2, float const* wiIn, float* wi3, float* pdf, float* uv2,
                              float* Le3, int32_t* ok, float* LeDir3, float* pdfDir) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  EnvSampleDev const es = env_sample(env, f2{u2[2 * i], u2[2 * i + 1]});
  f3 const Le = env_eval_uv(env, es.uv);
  wi3[3 * i] = es.wi.x, wi3[3 * i + 1] = es.wi.y, wi3[3 * i + 2] = es.wi.z;
  pdf[i] = es.pdf, uv2[2 * i] = es.uv.x, uv2[2 * i + 1] = es.uv.y;
  Le3[3 * i] = Le.x, Le3[3 * i + 1] = Le.y, Le3[3 * i + 2] = Le.z;
  ok[i] = es.ok ? 1 : 0;
  float p = 0.f;
  f3 const Ld = env_eval_dir(env, mk3(wiIn[3 * i], wiIn[3 * i + 1], wiIn[3 * i + 2]), p);
  LeDir3[3 * i] = Ld.x, LeDir3[3 * i + 1] = Ld.y, LeDir3[3 * i + 2] = Ld.z;
  pdfDir[i] = p;
}

// single path with a per-bounce log, one record per closest-hit ray (at most cap, *nOut written):
//   rec12 = {tri (-1: miss), pos3, beta3, L3 before the bounce is shaded, depth, sampler dimension}
template <bool MOTION, bool VN = false, bool CUT = false>
DMT_DEV void test_trace_log_body(int px, int py, int smp, float* rec12, int cap, int* nOut, float* L3) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  KArgs const k = kargs_base();
  SceneView const sc = load_scene(k);
  PathState st{};
  {
    ColdArgs const c = load_cold_args(k);
    path_begin(st, c.cam, c.sp, px, py, halton_pixel_base(c.sp, px, py), uint32_t(smp), load_camera_extra(k));
    if constexpr (MOTION) motion_set_time(motion_sample_time(k, halton_pixel_base(c.sp, px, py), uint32_t(smp)));
  }
  int n = 0;
  for (;;) {
    bool const doC = st.active, doS = st.hasShadow;
    int bestTri;
    float bu, bv;
    bool occluded;
    if constexpr (MOTION)  // one sample: its shadow rays share its time
      trace_pair_brute_motion(k, st, doC, doS, v2f{motion_time(), motion_time()}, bestTri, bu, bv, occluded);
    else if constexpr (CUT)  // every ray of the path sees the cutouts
      trace_pair_brute_cut(k, st, doC, doS, bestTri, bu, bv, occluded);
    else
      trace_pair_brute<false>(k, st, doC, doS, bestTri, bu, bv, occluded);  // one thread: the plain loop
    if (doS) {
      if (!occluded) st.L = st.L + get_C();
      st.hasShadow = false;
    }
    bool ended = true;
    if (doC) {
      if (n < cap) {
        float* r = rec12 + 12 * n++;
        f3 pos = mk3(0, 0, 0);
        if (bestTri >= 0) pos = shade_hit<MOTION ? kFeatMotion : 0u>(k, sc, bestTri, bu, bv, ray_dir(st)).pos;
        r[0] = float(bestTri), r[1] = pos.x, r[2] = pos.y, r[3] = pos.z;
        r[4] = st.beta.x, r[5] = st.beta.y, r[6] = st.beta.z, r[7] = st.L.x, r[8] = st.L.y, r[9] = st.L.z;
        r[10] = float(st.depth), r[11] = float(st.rng.dim);
      }
      ended = path_shade<MOTION ? kFeatMotion : VN ? kFeatVtxNormals : 0u>(k, st, bestTri, bu, bv);
      if (ended) st.active = false;
    }
    if (ended && !st.hasShadow) break;
  }
  *nOut = n;
  L3[0] = st.L.x, L3[1] = st.L.y, L3[2] = st.L.z;
}
__global__ void k_test_trace_log(RenderParams P, int px, int py, int smp, float* rec12, int cap, int* nOut,
                                 float* L3) {
  test_trace_log_body<false>(px, py, smp, rec12, cap, nOut, L3);
}
__global__ void k_test_trace_log_motion(RenderParams P, int px, int py, int smp, float* rec12, int cap, int* nOut, float* L3) {
  test_trace_log_body<true>(px, py, smp, rec12, cap, nOut, L3);
}

__global__ void k_test_trace_log_vn(RenderParams P, int px, int py, int smp, float* rec12, int cap, int* nOut, float* L3) {
  test_trace_log_body<false, true>(px, py, smp, rec12, cap, nOut, L3);
}

__global__ void k_test_trace_log_cut(RenderParams P, int px, int py, int smp, float* rec12, int cap, int* nOut, float* L3) {
  test_trace_log_body<false, false, true>(px, py, smp, rec12, cap, nOut, L3);
}

// dmt_test_shading_normal: shading_normal_at of triangle tri[i] at (bu, bv) for a ray of direction rd3[i]; ngFacing is
// the stored normal flipped against the ray as hit_finish flips it
// MAPPED (dmt_test_shading_normal_mapped): then the material's normal map around it, as path_shade's *_tex_vn rows apply it
template <bool MAPPED>
__global__ void k_test_shading_normal(RenderParams P, int n, int32_t const* tri, float const* bu, float const* bv, float const* rd3, float* ns3) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  SceneView const sc = load_scene(k);
  TriPost const T = sc.post[tri[i]];
  f3 ng = mk3(T.nx, T.ny, T.nz);
  if (dot(mk3(rd3[3 * i], rd3[3 * i + 1], rd3[3 * i + 2]), ng) > 0) ng = -ng;
  f3 ns = shading_normal_at(k, tri[i], bu[i], bv[i], ng);
  if constexpr (MAPPED) {
    Rec32 rec = sc.bsdfs[T.matId];
    ns = apply_material_textures<false>(k, rec, T.matId, tri[i], bu[i], bv[i], ns);
  }
  ns3[3 * i] = ns.x, ns3[3 * i + 1] = ns.y, ns3[3 * i + 2] = ns.z;
}

__global__ void k_test_tri(float const* xs, float const* ys, float const* zs, uint32_t n, f3 o, f3 d,
                           int32_t* hit, float* t, float* pos3, float* nrm3, float* err3) {
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f3 const p0 = mk3(xs[4 * i], ys[4 * i], zs[4 * i]);
  f3 const p1 = mk3(xs[4 * i + 1], ys[4 * i + 1], zs[4 * i + 1]);
  f3 const p2 = mk3(xs[4 * i + 2], ys[4 * i + 2], zs[4 * i + 2]);
  f3 const e0 = mk3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z);
  f3 const e1 = mk3(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
  Ray const ray{o, d};
  MTResult const r = mt_test(p0, e0, e1, ray);
  hit[i] = r.valid ? 1 : 0;
  float const inf = kInf;
  t[i] = r.valid ? r.t : inf;
  f3 pos = mk3(0, 0, 0), nrm = mk3(0, 0, 0), err = mk3(0, 0, 0);
  if (r.valid) {
    TriPost P;
    P.p0x = p0.x, P.p0y = p0.y, P.p0z = p0.z, P.p1x = p1.x, P.p1y = p1.y, P.p1z = p1.z;
    P.p2x = p2.x, P.p2y = p2.y, P.p2z = p2.z;
    f3 const nn = normalize(cross(e1, e0));
    P.nx = nn.x, P.ny = nn.y, P.nz = nn.z;
    P.matId = 0;
    Hit const h = hit_finish(P, r.u, r.v, mk3(0, 0, 0));  // zero direction: normal not flipped
    pos = h.pos, nrm = h.normal, err = h.error;
  }
  pos3[3 * i] = pos.x, pos3[3 * i + 1] = pos.y, pos3[3 * i + 2] = pos.z;
  nrm3[3 * i] = nrm.x, nrm3[3 * i + 1] = nrm.y, nrm3[3 * i + 2] = nrm.z;
  err3[3 * i] = err.x, err3[3 * i + 1] = err.y, err3[3 * i + 2] = err.z;
}

__global__ void k_test_sampler(SamplerParams sp, int n, int32_t const* pxs, int32_t const* pys,
                               int32_t const* ss, int ndims, int32_t* hidx, float* pix2, float* dims) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  int32_t const h = halton_pixel_base(sp, pxs[i], pys[i]) + ss[i] * (sp.scale0 * sp.scale1);
  hidx[i] = h;
  f2 const p = pixel2d(sp, h);
  pix2[2 * i] = p.x, pix2[2 * i + 1] = p.y;
  Sampler r;
  r.start(uint32_t(h));
  for (int d = 0; d < ndims; ++d) dims[size_t(i) * ndims + d] = r.get1D();
}

// the rays the render kernels trace (lens rays for lensR > 0), or with lens2 the sample's lens values alone
__global__ void k_test_camera(CameraXf cam, SamplerParams sp, CameraExtra extra, int n, int32_t const* pxs,
                              int32_t const* pys, int32_t const* ss, float* o3, float* d3, float* lens2) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  int32_t const h = halton_pixel_base(sp, pxs[i], pys[i]) + ss[i] * (sp.scale0 * sp.scale1);
  if (lens2) {
    LensU const u = lens_values(uint32_t(h));
    lens2[2 * i] = u.x, lens2[2 * i + 1] = u.y;
    return;
  }
  Ray const r = camera_ray_any(cam, sp, pxs[i], pys[i], h, extra);
  o3[3 * i] = r.o.x, o3[3 * i + 1] = r.o.y, o3[3 * i + 2] = r.o.z;
  d3[3 * i] = r.d.x, d3[3 * i + 1] = r.d.y, d3[3 * i + 2] = r.d.z;
}

// the film positions the camera-ray code forms: the jitter, warped under a pixel filter (knots non-null), plus the pixel
__global__ void k_test_film_positions(SamplerParams sp, FilterBin const* knots, float filtR, int n, int32_t const* pxs, int32_t const* pys,
                                      int32_t const* ss, float* xy2) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  int32_t const h = halton_pixel_base(sp, pxs[i], pys[i]) + ss[i] * (sp.scale0 * sp.scale1);
  f2 r = pixel2d(sp, h);
  if (knots) r = f2{filter_warp(knots, filtR, r.x), filter_warp(knots, filtR, r.y)};
  xy2[2 * i] = film_coord(r.x, pxs[i]), xy2[2 * i + 1] = film_coord(r.y, pys[i]);
}

// The BSDF probes' body: one lane per case of record `rec`, shading normal ns3[i], geometric normal ng3[i] (kOwnNg) or the
// shading normal again (a compile-time choice: a second load of the normal through ng3 = ns3 would change k_test_bsdf's code).
// Output layouts:
//   prepared12 = bsdf_prepare: {weight3, Oren-Nayar ms3 | 0, GGX escale | 0, type, GGX ax, ay, phi0 | 0, dielectric eta | 0}
//   sample10   = sample_bsdf(u2, uc): {wi3, f3, pdf, eta, delta, refract} (flags as 0 / 1)
//   eval4      = eval_bsdf(wi_eval): {f3 * weight, pdf}
template <bool kOwnNg>
DMT_DEV void test_bsdf_body(Rec32 rec, int n, float const* ns3, float const* ng3, float const* wo3, float const* u2,
                            float const* uc, float const* wi3, float* prep12, float* samp10, float* eval4) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  f3 const ns = mk3(ns3[3 * i], ns3[3 * i + 1], ns3[3 * i + 2]);
  f3 const ng = kOwnNg ? mk3(ng3[3 * i], ng3[3 * i + 1], ng3[3 * i + 2]) : ns;
  f3 const wo = mk3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
  Bsdf const b = bsdf_prepare(rec, ns, wo);
  float* p = prep12 + 12 * size_t(i);
  p[0] = b.weight.x, p[1] = b.weight.y, p[2] = b.weight.z;
  bool const oren = b.type == BS_OREN, ggx = b.type == BS_GGX_DIEL || b.type == BS_GGX_COND;  // the two kinds share registers (Bsdf)
  p[3] = oren ? b.ms.x : 0.f, p[4] = oren ? b.ms.y : 0.f, p[5] = oren ? b.ms.z : 0.f;
  p[6] = ggx ? b.escale : 0.f, p[7] = float(b.type), p[8] = ggx ? b.ax : 0.f, p[9] = ggx ? b.ay : 0.f, p[10] = ggx ? b.phi0 : 0.f;
  p[11] = b.type == BS_GGX_DIEL ? b.eta : 0.f;
  BsdfSample const s = sample_bsdf(b, wo, ns, ng, mk2(u2[2 * i], u2[2 * i + 1]), uc[i]);
  float* o = samp10 + 10 * size_t(i);
  o[0] = s.wi.x, o[1] = s.wi.y, o[2] = s.wi.z, o[3] = s.f.x, o[4] = s.f.y, o[5] = s.f.z;
  o[6] = s.pdf, o[7] = s.eta, o[8] = s.delta ? 1.f : 0.f, o[9] = s.refract ? 1.f : 0.f;
  float pdf = 0.f;
  f3 const f = eval_bsdf(b, wo, mk3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), ns, ng, pdf) * b.weight;
  float* e = eval4 + 4 * size_t(i);
  e[0] = f.x, e[1] = f.y, e[2] = f.z, e[3] = pdf;
}

// the geometric normal is the shading normal
__global__ void k_test_bsdf(Rec32 rec, int n, float const* ns3, float const* wo3, float const* u2, float const* uc, float const* wi3,
                            float* prep12, float* samp10, float* eval4) {
  test_bsdf_body<false>(rec, n, ns3, nullptr, wo3, u2, uc, wi3, prep12, samp10, eval4);
}

// a geometric normal of its own: the render kernels hand a normal-mapped ns and hit.normal as ng to sample_bsdf / eval_bsdf,
// wo . ns <= 0 < wo . ng included
__global__ void k_test_bsdf_ng(Rec32 rec, int n, float const* ns3, float const* ng3, float const* wo3, float const* u2,
                               float const* uc, float const* wi3, float* prep12, float* samp10, float* eval4) {
  test_bsdf_body<true>(rec, n, ns3, ng3, wo3, u2, uc, wi3, prep12, samp10, eval4);
}

// The material of triangle tri[i] at (bu, bv) as path_shade patches it before bsdf_prepare (level-0 lookups): the record
// after apply_material_textures and the shading normal it returns for the geometric normal ng3[i].  A BS_GGX_BLEND
// material also gives its conductor record, patched the same way, and the metallic fraction; the dielectric record keeps
// the blend tag.  Other materials leave rec2 zero and mix 0.
__global__ void k_test_material(RenderParams P, int n, int32_t const* tri, float const* bu, float const* bv, float const* ng3,
                                uint32_t* rec8, float* ns3, uint32_t* rec2_8, float* mixOut) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  SceneView const sc = load_scene(k);
  uint32_t const matId = sc.post[tri[i]].matId;
  f3 const ng = mk3(ng3[3 * i], ng3[3 * i + 1], ng3[3 * i + 2]);
  Rec32 rec = sc.bsdfs[matId], rec2{};
  float mix = 0.f;
  bool const blend = hi16(rec.w[1]) == BS_GGX_BLEND && matId + 1u < sc.bsdfCount;  // a pair: its conductor follows
  if (blend) {
    mix = blend_metallic<false>(k, rec, matId, tri[i], bu[i], bv[i]);
    rec.w[1] = (rec.w[1] & 0x0000FFFFu) | (uint32_t(BS_GGX_DIEL) << 16);  // patched as the dielectric it is shaded as
    rec2 = sc.bsdfs[matId + 1u];
  }
  f3 ns = ng;
  if (kargs(k)->matTex != nullptr) {
    ns = apply_material_textures<false>(k, rec, matId, tri[i], bu[i], bv[i], ng);
    if (blend) (void)apply_material_textures<false>(k, rec2, matId + 1u, tri[i], bu[i], bv[i], ng);
  }
  if (blend) rec.w[1] = (rec.w[1] & 0x0000FFFFu) | (uint32_t(BS_GGX_BLEND) << 16);
  for (int w = 0; w < 8; ++w) rec8[8 * size_t(i) + w] = rec.w[w], rec2_8[8 * size_t(i) + w] = rec2.w[w];
  ns3[3 * i] = ns.x, ns3[3 * i + 1] = ns.y, ns3[3 * i + 2] = ns.z;
  mixOut[i] = mix;
}

// sample_light at (pos3, nrm3) with draw u2, then eval_light of the sample:
//   out14 = {pLight3, direction3, pdf, delta, distance, factor, Le3, valid} (flags as 0 / 1)
__global__ void k_test_light(Rec32 rec, int n, float const* pos3, float const* nrm3, float const* u2,
                             int32_t const* hadT, float* out14) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  LightSample const s = sample_light(rec, mk3(pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2]),
                                     mk2(u2[2 * i], u2[2 * i + 1]), hadT[i] != 0,
                                     mk3(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2]));
  f3 const Le = eval_light(rec, s);
  float* o = out14 + 14 * size_t(i);
  o[0] = s.pLight.x, o[1] = s.pLight.y, o[2] = s.pLight.z;
  o[3] = s.direction.x, o[4] = s.direction.y, o[5] = s.direction.z;
  o[6] = s.pdf, o[7] = float(s.delta), o[8] = s.distance, o[9] = s.factor;
  o[10] = Le.x, o[11] = Le.y, o[12] = Le.z, o[13] = s.valid() ? 1.f : 0.f;
}

__global__ void k_test_half(int n, float const* fin, uint16_t* hout, uint16_t const* hin, float* fout) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  if (fin && hout) hout[i] = uint16_t(f2h(fin[i]));
  if (hin && fout) fout[i] = h2f(hin[i]);
}

__global__ void k_test_closest(RenderParams P, bool useBvh, int n, float const* o3, float const* d3, int32_t* tri,
                               float* tOut) {
  KArgs const k = kargs_base();
  if (!useBvh) cull_stage(k);
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  bool const alive = i < n;
  PathState st{};
  if (alive)
    set_ray(st, mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]));
  st.active = alive;
  int best;
  float bu, bv, bt = kInf;
  bool occluded;
  if (useBvh)
    trace_pair_bvh(k, st, alive, false, blockIdx.x * blockDim.x + threadIdx.x, best, bu, bv, occluded);
  else
    trace_pair_brute(k, st, alive, false, best, bu, bv, occluded);
  if (alive && best >= 0) {  // t of the winning triangle (same arithmetic as the loops)
    TriS const T = load_tri(to_const_as(load_scene(k).tris), uint32_t(best));
    bt = mt_pair(T, st.rp).t.x;
  }
  if (alive) tri[i] = best, tOut[i] = bt;
}

// dmt_test_trace_pair: one call of the render kernels' trace for the pair (closest ray i, shadow ray i) of every lane, full
// waves of pairs as the megakernel traces them: what the brute-force pass's culled clusters see of both kinds of ray
__global__ void k_test_trace_pair(RenderParams P, bool useBvh, int n, float const* o3, float const* d3, float const* so3, float const* sd3,
                                  float const* smax, int32_t* tri, float* uv2, uint8_t* occ) {
  KArgs const k = kargs_base();
  if (!useBvh) cull_stage(k);
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  bool const alive = i < n;
  PathState st{};
  if (alive) {
    set_ray(st, mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]));
    set_shadow_ray(st, mk3(so3[3 * i], so3[3 * i + 1], so3[3 * i + 2]), mk3(sd3[3 * i], sd3[3 * i + 1], sd3[3 * i + 2]));
    st.smax = smax[i];
  }
  st.active = alive, st.hasShadow = alive;
  int best;
  float bu, bv;
  bool occluded;
  if (useBvh)
    trace_pair_bvh(k, st, alive, alive, blockIdx.x * blockDim.x + threadIdx.x, best, bu, bv, occluded);
  else
    trace_pair_brute(k, st, alive, alive, best, bu, bv, occluded);
  if (alive) {
    tri[i] = best, occ[i] = occluded ? 1 : 0;
    uv2[2 * i] = best >= 0 ? bu : 0.f, uv2[2 * i + 1] = best >= 0 ? bv : 0.f;
  }
}

// dmt_test_closest_hit_at: the closest hit of ray i against the scene at time[i], by the motion rows' trace of the accel mode
__global__ void k_test_closest_at(RenderParams P, bool useBvh, int n, float const* o3, float const* d3, float const* time, int32_t* tri,
                                  float* tOut, float* uv2) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  bool const alive = i < n;
  PathState st{};
  if (alive)
    set_ray(st, mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]));
  st.active = alive;
  float const tm = alive ? time[i] : 0.f;
  int best;
  float bu, bv, bt = kInf;
  bool occluded;
  if (useBvh)
    trace_pair_bvh_motion(k, st, alive, false, v2f{tm, tm}, blockIdx.x * blockDim.x + threadIdx.x, best, bu, bv, occluded, &bt);
  else
    trace_pair_brute_motion(k, st, alive, false, v2f{tm, tm}, best, bu, bv, occluded, &bt);
  if (alive) {
    tri[i] = best, tOut[i] = best >= 0 ? bt : kInf;
    if (uv2) uv2[2 * i] = best >= 0 ? bu : 0.f, uv2[2 * i + 1] = best >= 0 ? bv : 0.f;
  }
}

// dmt_test_opacity: alpha8 and the pass decision of triangle tri[i] at (bu, bv), by the record and the lookup the cutout rows
// use (an opaque triangle: 255, passes)
__global__ void k_test_opacity(RenderParams P, int n, int32_t const* tri, float const* bu, float const* bv, float* alpha8, uint8_t* pass) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  CutoutView const cv = load_cutout(k);
  OpacityRec const R = cv.recs[tri[i]];
  float const a = R.wh == 0u ? 255.f : opacity_alpha8_at(cv.rgba, R, bu[i], bv[i]);
  alpha8[i] = a;
  pass[i] = (R.wh == 0u || a >= cv.cutoff8) ? 1 : 0;
}

// dmt_test_closest_hit_opacity: ray i as a closest-hit ray and as a shadow ray of length tmax[i] at once, by the cutout rows'
// trace of the accel mode
__global__ void k_test_closest_cut(RenderParams P, bool useBvh, int n, float const* o3, float const* d3, float const* tmax, int32_t* tri,
                                   float* tOut, float* uv2, uint8_t* occ) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  bool const alive = i < n;
  PathState st{};
  if (alive) {
    f3 const o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
    set_ray(st, o, d), set_shadow_ray(st, o, d);
    st.smax = tmax[i];
  }
  st.active = alive, st.hasShadow = alive;
  int best;
  float bu, bv, bt = kInf;
  bool occluded;
  if (useBvh)
    trace_pair_bvh_cut(k, st, alive, alive, blockIdx.x * blockDim.x + threadIdx.x, best, bu, bv, occluded, &bt);
  else
    trace_pair_brute_cut(k, st, alive, alive, best, bu, bv, occluded, &bt);
  if (alive) {
    tri[i] = best, tOut[i] = best >= 0 ? bt : kInf;
    if (uv2) uv2[2 * i] = best >= 0 ? bu : 0.f, uv2[2 * i + 1] = best >= 0 ? bv : 0.f;
    if (occ) occ[i] = occluded ? 1 : 0;
  }
}

// dmt_test_shutter_times: shutter_time of the samples, as the motion rows compute it
__global__ void k_test_shutter(SamplerParams sp, float open, float close, int n, int32_t const* pxs, int32_t const* pys, int32_t const* ss,
                               float* t) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  int32_t const h = halton_pixel_base(sp, pxs[i], pys[i]) + ss[i] * (sp.scale0 * sp.scale1);
  t[i] = shutter_time(uint32_t(h), open, close);
}

// dmt_test_medium: the device versions of what the *_medium rows compute between two ray casts
__global__ void k_test_medium(MediumParams m, int n, float const* o3, float const* d3, float const* tHit, uint32_t const* h, uint32_t const* depth,
                              float const* cosine, float const* u2, float* seg2, int32_t* hit, float* values3, float* eval, float* wi3, float* pdf) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  float t0, t1;
  bool const ok = medium_segment(o3 + 3 * i, d3 + 3 * i, tHit[i], m.lo, m.hi, &t0, &t1);
  seg2[2 * i] = t0, seg2[2 * i + 1] = t1, hit[i] = ok ? 1 : 0;
  float const u = medium_u(h[i], depth[i]);
  values3[3 * i] = u, values3[3 * i + 1] = medium_free_flight(m.sigmaT, u), values3[3 * i + 2] = medium_transmittance(m.sigmaT, ok ? t1 - t0 : 0.f);
  eval[i] = hg_eval(m.g, cosine[i]);
  float const wo[3] = {-d3[3 * i], -d3[3 * i + 1], -d3[3 * i + 2]};
  hg_sample(m.g, wo, u2[2 * i], u2[2 * i + 1], wi3 + 3 * i, pdf + i);
}

// dmt_test_medium_grid: medium_grid_march on the device, one ray per thread
__global__ void k_test_medium_grid(MediumParams m, MediumGridParams g, int n, float const* o3, float const* d3, float const* tEnd,
                                   float const* tauTarget, float* tau, float* ts, int32_t* collided, int32_t* steps) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  MediumGridMarch const r = medium_grid_march(o3 + 3 * i, d3 + 3 * i, tEnd[i], tauTarget[i], m.sigmaT, m.lo, m.hi, g);
  tau[i] = r.tau, ts[i] = r.ts, collided[i] = r.collided, steps[i] = r.steps;
}

// dmt_test_medium_spectrum: medium_spectrum_event on the device, one case per thread
__global__ void k_test_medium_spectrum(MediumSpectrumParams sp, int n, float const* beta3, uint32_t const* h, uint32_t const* depth,
                                       float const* tauSeg, int32_t* channel, int32_t* collided, float* tauAt, float* weight3) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  float const beta[3] = {beta3[3 * i], beta3[3 * i + 1], beta3[3 * i + 2]};
  MediumSpectrumEvent const ev = medium_spectrum_event(sp.q, beta, h[i], depth[i], tauSeg[i]);
  channel[i] = ev.channel, collided[i] = ev.collided, tauAt[i] = ev.tauAt;
  weight3[3 * i] = ev.w[0], weight3[3 * i + 1] = ev.w[1], weight3[3 * i + 2] = ev.w[2];
}

// dmt_camera_project (project_point) on the device
__global__ void k_test_project(ProjXf c, int n, float const* p3, float* xy2, float* depth) {
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  Proj const o = project_point(c, p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]);
  xy2[2 * i] = o.fx, xy2[2 * i + 1] = o.fy, depth[i] = o.depth;
}

// dmt_test_light_tree: the light choice of a bounce at (pos3, nrm3) with the random number u, by the function the rows of the
// context's tree call on the tree they read.  REF: ltr_select's cut of up to four lights (*_ltree2); otherwise lt_select's one
// light, its probability formed as path_shade forms it (*_ltree).  Slots past counts[i] hold -1 / 0.
template <bool REF>
__global__ void k_test_light_tree(RenderParams P, int n, float const* pos3, float const* nrm3, float const* u, float startPmf,
                                  int32_t* idx4, float* pmf4, int32_t* counts) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  LightTreeRefSelection sel{};
  if constexpr (REF) {
    sel = ltr_select(kargs(k)->lightTreeRef, pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2], nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2],
                     u[i], startPmf);
  } else {
    float treePmf = 0.f;
    int const li = lt_select(kargs(k)->lightTree, pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2], nrm3[3 * i], nrm3[3 * i + 1],
                             nrm3[3 * i + 2], u[i], treePmf);
    if (li >= 0) sel.indices[0] = uint32_t(li), sel.pmfs[0] = startPmf * treePmf, sel.count = 1u;
  }
  counts[i] = int32_t(sel.count);
  for (uint32_t s = 0; s < uint32_t(kLightTreeMaxSplitSize); ++s)
    idx4[4 * i + s] = s < sel.count ? int32_t(sel.indices[s]) : -1, pmf4[4 * i + s] = s < sel.count ? sel.pmfs[s] : 0.f;
}

// dmt_test_emitter_tree: the emitter choice of a bounce at (pos3, nrm3) with the random number u, one lane per case: et_select
// on the tree the *_etree rows read, its probability formed as path_shade forms it, and et_pmf along the selected emitter's
// trail as an emitter hit forms it
__global__ void k_test_emitter_tree(RenderParams P, int n, float const* pos3, float const* nrm3, float const* u, float startPmf,
                                    int32_t* idx, float* pmf, float* pmfTrail) {
  KArgs const k = kargs_base();
  int const i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  EmitterNode const* const nodes = kargs(k)->emitterTree;
  float const px = pos3[3 * i], py = pos3[3 * i + 1], pz = pos3[3 * i + 2], nx = nrm3[3 * i], ny = nrm3[3 * i + 1], nz = nrm3[3 * i + 2];
  float treePmf = 0.f;
  int const e = et_select(nodes, px, py, pz, nx, ny, nz, u[i], treePmf);
  idx[i] = e, pmf[i] = e >= 0 ? startPmf * treePmf : 0.f;
  pmfTrail[i] = e >= 0 ? startPmf * et_pmf(nodes, kargs(k)->emitterTrails[e], px, py, pz, nx, ny, nz) : 0.f;
}

typedef void (*TestTraceFn)(RenderParams, int, int32_t const*, int32_t const*, int32_t const*, float*);
#define DMT_TEST_TRACE_ROW(suffix, mask, waves, body) {mask, k_test_trace<mask>},
KernelRow<TestTraceFn> const kTestTraceKernels[] = {DMT_MEGAKERNELS(DMT_TEST_TRACE_ROW)};

// ---------------------------------------------------------------------------------------------
// host side: what the entry points share
// ---------------------------------------------------------------------------------------------
int probeError(dmt_ctx* ctx, Probe const& p) {
  ctx->err = std::string(p.call) + ": " + hipGetErrorName(p.err) + " - " + hipGetErrorString(p.err);
  return DMT_ERR_HIP;
}

// after the launch: the kernel's own error, then every output the caller asked for
int finishProbe(dmt_ctx* ctx, Probe& p) {
  if (int const rc = finishTest(ctx)) return rc;
  return p.fetch() == hipSuccess ? DMT_OK : probeError(ctx, p);
}

// What the probes that walk the uploaded scene check first, reported under the entry point's name `who`: the whole scene
// and the camera set (wholeScene), and every material index inside the BSDF array.
int sceneReady(dmt_ctx* ctx, char const* who, bool wholeScene) {
  if (wholeScene && !(ctx->scene.haveTris && ctx->scene.haveBsdfs && ctx->lights.list.have && ctx->camera.have))
    return fail(ctx, DMT_ERR_STATE, (std::string(who) + ": scene/camera not set").c_str());
  if (ctx->scene.matIdOutside())
    return fail(ctx, DMT_ERR_INVALID, (std::string(who) + ": material index outside the BSDF array").c_str());
  return DMT_OK;
}

// dmt_test_bsdf (ng3 null: k_test_bsdf) and dmt_test_bsdf_ng behind their own argument checks
int probeBsdf(dmt_ctx* ctx, void const* bsdf32, int n, float const* ns3, float const* ng3, float const* wo3, float const* u2,
              float const* uc, float const* wi_eval3, float* prepared12, float* sample10, float* eval4) {
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dns(p, ns3, 3), dng(p, ng3, 3), dwo(p, wo3, 3), du2(p, u2, 2), duc(p, uc, 1), dwi(p, wi_eval3, 3);
  ProbeOut<float> dp(p, prepared12, 12), ds(p, sample10, 10), de(p, eval4, 4);
  if (p.err != hipSuccess) return probeError(ctx, p);
  Rec32 rec;
  memcpy(&rec, bsdf32, 32);
  if (ng3)
    hipLaunchKernelGGL(k_test_bsdf_ng, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, rec, n, dns.get(), dng.get(), dwo.get(), du2.get(),
                       duc.get(), dwi.get(), dp.get(), ds.get(), de.get());
  else
    hipLaunchKernelGGL(k_test_bsdf, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, rec, n, dns.get(), dwo.get(), du2.get(), duc.get(),
                       dwi.get(), dp.get(), ds.get(), de.get());
  return finishProbe(ctx, p);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C entry points (include/dmt_hip.h): arguments checked, arrays staged, one launch on the context's stream, outputs copied back
// ---------------------------------------------------------------------------------------------
extern "C" {

int dmt_test_envmap(dmt_ctx* ctx, int n, const float* u2, const float* wi_in3, float* wi3, float* pdf, float* uv2, float* Le3,
                    int32_t* ok, float* Le_dir3, float* pdf_dir) {
  if (!ctx || n <= 0 || !u2 || !wi_in3 || !wi3 || !pdf || !uv2 || !Le3 || !ok || !Le_dir3 || !pdf_dir) return DMT_ERR_INVALID;
  if (ctx->lights.env.view.w <= 0) return fail(ctx, DMT_ERR_STATE, "dmt_test_envmap: no env map uploaded");
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> du(p, u2, 2), dwin(p, wi_in3, 3);
  ProbeOut<float> dwi(p, wi3, 3), dpdf(p, pdf, 1), duv(p, uv2, 2), dLe(p, Le3, 3), dLd(p, Le_dir3, 3), dpd(p, pdf_dir, 1);
  ProbeOut<int32_t> dok(p, ok, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_envmap, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, ctx->lights.env.view, n, du.get(), dwin.get(), dwi.get(),
                     dpdf.get(), duv.get(), dLe.get(), dok.get(), dLd.get(), dpd.get());
  return finishProbe(ctx, p);
}

int dmt_test_sampler_table(dmt_ctx* ctx, int width, int height, uint32_t s0, uint32_t n, float* out_vals, float* out_jitter) {
  if (!ctx || width <= 0 || height <= 0 || !out_vals || !out_jitter) return DMT_ERR_INVALID;
  uint32_t const pw = uint32_t(width < 128 ? width : 128), ph = uint32_t(height < 128 ? height : 128);
  SamplerParams const sp = computeSamplerParams(width, height);
  if (uint64_t(n) * pw * ph > 0x7FFFFFFFull || (uint64_t(s0) + n + 1) * uint64_t(sp.scale0) * uint64_t(sp.scale1) > 0x7FFFFFFFull)
    return fail(ctx, DMT_ERR_INVALID, "dmt_test_sampler_table: too many entries, or the sample index overflows the 32-bit Halton index");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n) * pw * ph);  // one case per table entry
  ProbeOut<float4> dv(p, out_vals, 2);
  ProbeOut<float2> dj(p, out_jitter, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_sampler_table, dim3(p.blocks(256)), dim3(256), 0, ctx->stream, sp, s0, n, pw, ph, dv.get(), dj.get(),
                     static_cast<float2*>(nullptr), ctx->camera.filt.view(), ctx->camera.filt.radius);  // the lens-free table; the jitter warped under a pixel filter
  return finishProbe(ctx, p);
}

int dmt_test_triangle_intersect(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs, size_t count, const float* o3,
                                const float* d3, int32_t* hit, float* t, float* pos3, float* nrm3, float* err3) {
  if (!ctx || !xs || !ys || !zs || !o3 || !d3 || !hit) return DMT_ERR_INVALID;
  if (count == 0) return DMT_OK;
  Probe p(ctx->device, count);
  ProbeIn<float> dx(p, xs, 4), dy(p, ys, 4), dz(p, zs, 4);
  ProbeOut<int32_t> dh(p, hit, 1);
  ProbeOut<float> dt(p, t, 1), dp(p, pos3, 3), dn(p, nrm3, 3), de(p, err3, 3);  // optional: null is not copied back
  if (p.err != hipSuccess) return probeError(ctx, p);
  uint32_t const n = uint32_t(count);
  hipLaunchKernelGGL(k_test_tri, dim3(p.blocks(256)), dim3(256), 0, ctx->stream, dx.get(), dy.get(), dz.get(), n,
                     f3{o3[0], o3[1], o3[2]}, f3{d3[0], d3[1], d3[2]}, dh.get(), dt.get(), dp.get(), dn.get(), de.get());
  return finishProbe(ctx, p);
}

int dmt_test_sampler(dmt_ctx* ctx, int width, int height, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss,
                     int ndims, int32_t* halton_index, float* pixel2d_out, float* dims) {
  if (!ctx || n < 0 || ndims < 0 || !pxs || !pys || !ss || !halton_index || !pixel2d_out || !dims || width <= 0 || height <= 0)
    return DMT_ERR_INVALID;
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<int32_t> dh(p, halton_index, 1);
  ProbeOut<float> dp2(p, pixel2d_out, 2), dd(p, dims, size_t(ndims));  // ndims == 0: empty, nothing copied back
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_sampler, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, computeSamplerParams(width, height), n, dpx.get(),
                     dpy.get(), dss.get(), ndims, dh.get(), dp2.get(), dd.get());
  return finishProbe(ctx, p);
}

int dmt_test_camera_rays(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* o3, float* d3) {
  if (!ctx || n < 0 || !pxs || !pys || !ss || !o3 || !d3) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_camera_rays: set the camera first");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<float> dO(p, o3, 3), dD(p, d3, 3);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_camera, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, ctx->camera.xf, ctx->camera.sp, ctx->camera.extra(), n, dpx.get(),
                     dpy.get(), dss.get(), dO.get(), dD.get(), static_cast<float*>(nullptr));
  return finishProbe(ctx, p);
}

int dmt_test_lens_values(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* lens2) {
  if (!ctx || n < 0 || !pxs || !pys || !ss || !lens2) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_lens_values: set the camera first");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<float> dL(p, lens2, 2);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_camera, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, ctx->camera.xf, ctx->camera.sp, ctx->camera.extra(), n, dpx.get(),
                     dpy.get(), dss.get(), static_cast<float*>(nullptr), static_cast<float*>(nullptr), dL.get());
  return finishProbe(ctx, p);
}

int dmt_test_film_positions(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* xy2) {
  if (!ctx || n < 0 || !pxs || !pys || !ss || !xy2) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_film_positions: set the camera first");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<float> dXy(p, xy2, 2);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_film_positions, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, ctx->camera.sp, ctx->camera.filt.view(), ctx->camera.filt.radius, n,
                     dpx.get(), dpy.get(), dss.get(), dXy.get());
  return finishProbe(ctx, p);
}

int dmt_test_camera_project(dmt_ctx* ctx, int n, const float* p3, float* xy2, float* depth) {
  if (!ctx || n < 0 || !p3 || !xy2 || !depth) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_camera_project: set the camera first");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dP(p, p3, 3);
  ProbeOut<float> dXy(p, xy2, 2), dD(p, depth, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_project, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, makeProjXf(ctx->camera.cam), n, dP.get(), dXy.get(), dD.get());
  return finishProbe(ctx, p);
}

int dmt_test_bsdf(dmt_ctx* ctx, const void* bsdf32, int n, const float* ns3, const float* wo3, const float* u2, const float* uc,
                  const float* wi_eval3, float* prepared12, float* sample10, float* eval4) {
  if (!ctx || n < 0 || !bsdf32 || !ns3 || !wo3 || !u2 || !uc || !wi_eval3 || !prepared12 || !sample10 || !eval4) return DMT_ERR_INVALID;
  return probeBsdf(ctx, bsdf32, n, ns3, nullptr, wo3, u2, uc, wi_eval3, prepared12, sample10, eval4);
}

int dmt_test_bsdf_ng(dmt_ctx* ctx, const void* bsdf32, int n, const float* ns3, const float* ng3, const float* wo3, const float* u2,
                     const float* uc, const float* wi_eval3, float* prepared12, float* sample10, float* eval4) {
  if (!ctx || n < 0 || !bsdf32 || !ns3 || !ng3 || !wo3 || !u2 || !uc || !wi_eval3 || !prepared12 || !sample10 || !eval4)
    return DMT_ERR_INVALID;
  return probeBsdf(ctx, bsdf32, n, ns3, ng3, wo3, u2, uc, wi_eval3, prepared12, sample10, eval4);
}

int dmt_test_material(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* ng3, void* rec32,
                      float* ns3, void* rec2_32, float* mix) {
  if (!ctx || n < 0 || !tri || !bu || !bv || !ng3 || !rec32 || !ns3 || !rec2_32 || !mix) return DMT_ERR_INVALID;
  if (!(ctx->scene.haveTris && ctx->scene.haveBsdfs)) return fail(ctx, DMT_ERR_STATE, "dmt_test_material: triangles and BSDFs first");
  if (int const rc = sceneReady(ctx, "dmt_test_material", false)) return rc;
  if (!ctx->surf.texturesMatch(ctx->scene.bsdfCount, ctx->scene.triCount))
    return fail(ctx, DMT_ERR_STATE, "dmt_test_material: texture tables do not match the uploaded BSDFs / triangles (upload textures last)");
  for (int i = 0; i < n; ++i)
    if (tri[i] < 0 || size_t(tri[i]) >= ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "dmt_test_material: triangle index out of range");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dTri(p, tri, 1);
  ProbeIn<float> dBu(p, bu, 1), dBv(p, bv, 1), dNg(p, ng3, 3);
  ProbeOut<uint32_t> dRec(p, rec32, 8), dRec2(p, rec2_32, 8);
  ProbeOut<float> dNs(p, ns3, 3), dMix(p, mix, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_material, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), n, dTri.get(),
                     dBu.get(), dBv.get(), dNg.get(), dRec.get(), dNs.get(), dRec2.get(), dMix.get());
  return finishProbe(ctx, p);
}

int dmt_test_light(dmt_ctx* ctx, const void* light32, int n, const float* pos3, const float* nrm3, const float* u2,
                   const int32_t* had_transmission, float* out14) {
  if (!ctx || n < 0 || !light32 || !pos3 || !nrm3 || !u2 || !had_transmission || !out14) return DMT_ERR_INVALID;
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dp(p, pos3, 3), dn(p, nrm3, 3), du(p, u2, 2);
  ProbeIn<int32_t> dh(p, had_transmission, 1);
  ProbeOut<float> dout(p, out14, 14);
  if (p.err != hipSuccess) return probeError(ctx, p);
  Rec32 rec;
  memcpy(&rec, light32, 32);
  hipLaunchKernelGGL(k_test_light, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, rec, n, dp.get(), dn.get(), du.get(), dh.get(),
                     dout.get());
  return finishProbe(ctx, p);
}

int dmt_test_light_tree(dmt_ctx* ctx, int n, const float* pos3, const float* nrm3, const float* u, float start_pmf, int32_t* indices4,
                        float* pmfs4, int32_t* counts) {
  if (!ctx || n < 0 || !pos3 || !nrm3 || !u || !indices4 || !pmfs4 || !counts) return DMT_ERR_INVALID;
  uint32_t F = 0;  // the tree dmt_render would read, built first
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  switch (ctx->lights.why(plainSurfaces(ctx))) {  // where a launch runs the uniform rows there is no tree to walk
    case LightState::Pick::NoList: return fail(ctx, DMT_ERR_STATE, "dmt_test_light_tree: upload lights first");
    case LightState::Pick::UniformMode: return fail(ctx, DMT_ERR_STATE, "dmt_test_light_tree: the context picks its lights uniformly (dmt_set_light_sampling first)");
    case LightState::Pick::OneLight: return fail(ctx, DMT_ERR_STATE, "dmt_test_light_tree: a tree needs more than one light; the uniform pick is used");
    case LightState::Pick::TooDeep: return fail(ctx, DMT_ERR_STATE, ("dmt_test_light_tree: the light tree is too deep for the walk's guard (" +
                                                std::to_string(ctx->lights.tree.depth) + " levels); the uniform pick is used instead").c_str());
    case LightState::Pick::NotTreeable: return fail(ctx, DMT_ERR_STATE, "dmt_test_light_tree: this scene keeps the uniform pick (a light tree takes point and spot lights, "
                                                                        "without emissive triangles, image textures or blend materials)");
    case LightState::Pick::Tree: break;
  }
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dP(p, pos3, 3), dN(p, nrm3, 3), dU(p, u, 1);
  ProbeOut<int32_t> dI(p, indices4, 4), dC(p, counts, 1);
  ProbeOut<float> dPmf(p, pmfs4, 4);
  if (p.err != hipSuccess) return probeError(ctx, p);
  RenderParams const P = baseParams(ctx, p.threads(64));
  bool const ref = (F & kFeatLightTreeRef) != 0;
  if (!(ref ? static_cast<void const*>(P.lightTreeRef) : static_cast<void const*>(P.lightTree)))
    return fail(ctx, DMT_ERR_STATE, "dmt_test_light_tree: no light tree on the device");
  hipLaunchKernelGGL(ref ? k_test_light_tree<true> : k_test_light_tree<false>, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, P, n, dP.get(),
                     dN.get(), dU.get(), start_pmf, dI.get(), dPmf.get(), dC.get());
  return finishProbe(ctx, p);
}

int dmt_test_emitter_tree(dmt_ctx* ctx, int n, const float* pos3, const float* nrm3, const float* u, float start_pmf, int32_t* index_out,
                          float* pmf_out, float* pmf_by_trail_out) {
  if (!ctx || n < 0 || !pos3 || !nrm3 || !u || !index_out || !pmf_out || !pmf_by_trail_out) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t F = 0;  // the tree dmt_render would read, built first
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  switch (ctx->lights.whyEmitters(ctx->surf.area.count)) {  // where a launch runs the uniform rows there is no tree to walk
    case LightState::EmitterPick::UniformMode: return fail(ctx, DMT_ERR_STATE, "dmt_test_emitter_tree: the context picks its emitters uniformly (dmt_set_emitter_sampling first)");
    case LightState::EmitterPick::NoTriangles: return fail(ctx, DMT_ERR_STATE, "dmt_test_emitter_tree: no emissive triangles (dmt_upload_area_lights); the emitter tree is not used");
    case LightState::EmitterPick::NotTreeable: return fail(ctx, DMT_ERR_STATE, "dmt_test_emitter_tree: the light list holds a directional light; the uniform pick is used");
    case LightState::EmitterPick::TooDeep: return fail(ctx, DMT_ERR_STATE, ("dmt_test_emitter_tree: the emitter tree is too deep for the walk's guard (" +
                                                       std::to_string(ctx->lights.emitters.depth) + " levels); the uniform pick is used instead").c_str());
    case LightState::EmitterPick::Tree: break;
  }
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dP(p, pos3, 3), dN(p, nrm3, 3), dU(p, u, 1);
  ProbeOut<int32_t> dI(p, index_out, 1);
  ProbeOut<float> dPmf(p, pmf_out, 1), dTrail(p, pmf_by_trail_out, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  RenderParams const P = baseParams(ctx, p.threads(64));
  if (!P.emitterTree || !P.emitterTrails) return fail(ctx, DMT_ERR_STATE, "dmt_test_emitter_tree: no emitter tree on the device");
  hipLaunchKernelGGL(k_test_emitter_tree, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, P, n, dP.get(), dN.get(), dU.get(), start_pmf,
                     dI.get(), dPmf.get(), dTrail.get());
  return finishProbe(ctx, p);
}

int dmt_test_half(dmt_ctx* ctx, int n, const float* f_in, uint16_t* h_out, const uint16_t* h_in, float* f_out) {
  if (!ctx || n < 0) return DMT_ERR_INVALID;
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));  // either direction may be absent: its buffers stay empty (null)
  ProbeIn<float> dfi(p, f_in, 1);
  ProbeOut<uint16_t> dho(p, h_out, f_in && h_out ? 1 : 0);
  ProbeIn<uint16_t> dhi(p, h_in, 1);
  ProbeOut<float> dfo(p, f_out, h_in && f_out ? 1 : 0);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_half, dim3(p.blocks(256)), dim3(256), 0, ctx->stream, n, dfi.get(), dho.get(), dhi.get(), dfo.get());
  return finishProbe(ctx, p);
}

int dmt_test_trace_samples(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* L3) {
  if (!ctx || n < 0 || !pxs || !pys || !ss || !L3) return DMT_ERR_INVALID;
  if (int const rc = sceneReady(ctx, "dmt_test_trace_samples", true)) return rc;
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<float> dL(p, L3, 3);
  if (p.err != hipSuccess) return probeError(ctx, p);
  uint32_t F = 0;  // the shading body dmt_render would run
  if (int const rc = resolveFeatures(ctx, &F)) return rc;
  if (int const rc = checkProjection(ctx, F)) return rc;  // as dmt_render
  TestTraceFn const kernel = kernelOf(kTestTraceKernels, F);
  if (!kernel) return noKernel(ctx, "dmt_test_trace_samples", F);
  if (F & kFeatBvh) {
    if (int const rcT = requireTree(ctx, "dmt_test_trace_samples")) return rcT;
    HIP_TRY(ctx, reserveOverflow(ctx, p.threads(64)));
  }
  RenderParams P = baseParams(ctx, p.threads(64));
  if (int const rc = motionParams(ctx, F, P)) return rc;
  hipLaunchKernelGGL(kernel, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, P, n, dpx.get(), dpy.get(),
                     dss.get(), dL.get());
  return finishProbe(ctx, p);
}

int dmt_test_texture_filter(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const int32_t* tex,
                            const int32_t* depth, float* rgb3, int32_t* branch, float* lod) {
  if (!ctx || n < 0 || !tri || !bu || !bv || !tex || !depth || !rgb3 || !branch || !lod) return DMT_ERR_INVALID;
  if (!(ctx->scene.haveTris && ctx->camera.have) || ctx->surf.tex.count == 0 || ctx->surf.tex.triUvCount != ctx->scene.triCount)
    return fail(ctx, DMT_ERR_STATE, "dmt_test_texture_filter: triangles, camera and textures (with one UV triple per triangle) first");
  for (int i = 0; i < n; ++i)
    if (tri[i] < 0 || size_t(tri[i]) >= ctx->scene.triCount || tex[i] < 0 || uint32_t(tex[i]) >= ctx->surf.tex.count)
      return fail(ctx, DMT_ERR_INVALID, "dmt_test_texture_filter: triangle or texture index out of range");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dTri(p, tri, 1), dTex(p, tex, 1), dDepth(p, depth, 1);
  ProbeIn<float> dBu(p, bu, 1), dBv(p, bv, 1);
  ProbeOut<float> dRgb(p, rgb3, 3), dLod(p, lod, 1);
  ProbeOut<int32_t> dBranch(p, branch, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_texfilter, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), n, dTri.get(),
                     dBu.get(), dBv.get(), dTex.get(), dDepth.get(), dRgb.get(), dBranch.get(), dLod.get());
  return finishProbe(ctx, p);
}

int dmt_test_trace_log(dmt_ctx* ctx, int px, int py, int s, float* rec12, int cap, int* n_out, float* L3) {
  if (!ctx || !rec12 || cap <= 0 || !n_out || !L3) return DMT_ERR_INVALID;
  if (int const rc = sceneReady(ctx, "dmt_test_trace_log", true)) return rc;
  int variant = 0;
  if (int const rc = firstHitVariant(ctx, "dmt_test_trace_log", &variant)) return rc;
  Probe p(ctx->device, 1);  // one path, walked by one lane
  ProbeOut<float> dr(p, rec12, 12 * size_t(cap)), dL(p, L3, 3);
  ProbeOut<int> dn(p, n_out, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  RenderParams P = baseParams(ctx, p.threads(64));
  if (int const rc = motionParams(ctx, ctx->ac.haveMotion ? kFeatMotion : 0u, P)) return rc;  // (brute force: no tree)
  decltype(&k_test_trace_log) const kernels[4] = {k_test_trace_log, k_test_trace_log_vn, k_test_trace_log_motion, k_test_trace_log_cut};  // by firstHitVariant
  hipLaunchKernelGGL(kernels[variant], dim3(p.blocks(64)), dim3(64), 0, ctx->stream, P, px, py, s,
                     dr.get(), cap, dn.get(), dL.get());
  return finishProbe(ctx, p);
}

int dmt_test_closest_hit(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, int32_t* tri_index, float* t) {
  if (!ctx || nrays < 0 || !o3 || !d3 || !tri_index || !t) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_test_closest_hit: upload triangles first");
  if (nrays == 0) return DMT_OK;
  Probe p(ctx->device, size_t(nrays));
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3);
  ProbeOut<int32_t> di(p, tri_index, 1);
  ProbeOut<float> dt(p, t, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  bool const useBvh = ctx->accel == DMT_ACCEL_BVH;
  if (useBvh) {
    if (int const rcT = requireTree(ctx, "dmt_test_closest_hit")) return rcT;
    HIP_TRY(ctx, reserveOverflow(ctx, p.threads(64)));
  }
  hipLaunchKernelGGL(k_test_closest, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), useBvh, nrays,
                     dO.get(), dD.get(), di.get(), dt.get());
  return finishProbe(ctx, p);
}

int dmt_test_trace_pair(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* so3, const float* sd3, const float* smax,
                        int32_t* tri_index, float* uv2, uint8_t* occluded) {
  if (!ctx || nrays < 0 || !o3 || !d3 || !so3 || !sd3 || !smax || !tri_index || !uv2 || !occluded) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_test_trace_pair: upload triangles first");
  if (nrays == 0) return DMT_OK;
  Probe p(ctx->device, size_t(nrays));
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3), dSO(p, so3, 3), dSD(p, sd3, 3), dM(p, smax, 1);
  ProbeOut<int32_t> di(p, tri_index, 1);
  ProbeOut<float> duv(p, uv2, 2);
  ProbeOut<uint8_t> docc(p, occluded, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  bool const useBvh = ctx->accel == DMT_ACCEL_BVH;
  if (useBvh) {
    if (int const rcT = requireTree(ctx, "dmt_test_trace_pair")) return rcT;
    HIP_TRY(ctx, reserveOverflow(ctx, p.threads(64)));
  }
  hipLaunchKernelGGL(k_test_trace_pair, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), useBvh, nrays,
                     dO.get(), dD.get(), dSO.get(), dSD.get(), dM.get(), di.get(), duv.get(), docc.get());
  return finishProbe(ctx, p);
}

int dmt_test_closest_hit_at(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* time, int32_t* tri_index, float* t,
                            float* uv2) {
  if (!ctx || nrays < 0 || !o3 || !d3 || !time || !tri_index || !t) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_test_closest_hit_at: upload triangles first");
  if (!ctx->ac.haveMotion) return fail(ctx, DMT_ERR_STATE, "dmt_test_closest_hit_at: no key 1 (dmt_set_motion first)");
  for (int i = 0; i < nrays; ++i)
    if (!std::isfinite(time[i])) return fail(ctx, DMT_ERR_INVALID, "dmt_test_closest_hit_at: a time is not finite");
  if (nrays == 0) return DMT_OK;
  Probe p(ctx->device, size_t(nrays));
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3), dT(p, time, 1);
  ProbeOut<int32_t> di(p, tri_index, 1);
  ProbeOut<float> dt(p, t, 1), duv(p, uv2, 2);  // uv2 optional: null is not copied back
  if (p.err != hipSuccess) return probeError(ctx, p);
  bool const useBvh = ctx->accel == DMT_ACCEL_BVH;
  if (useBvh) HIP_TRY(ctx, reserveOverflow(ctx, p.threads(64)));
  RenderParams P = baseParams(ctx, p.threads(64));
  if (int const rc = motionParams(ctx, kFeatMotion | (useBvh ? kFeatBvh : 0u), P)) return rc;
  hipLaunchKernelGGL(k_test_closest_at, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, P, useBvh, nrays, dO.get(), dD.get(), dT.get(), di.get(),
                     dt.get(), duv.get());
  return finishProbe(ctx, p);
}

static int probeShadingNormal(dmt_ctx* ctx, bool mapped, int n, const int32_t* tri, const float* bu, const float* bv, const float* rd3, float* ns3) {
  if (!ctx || n < 0 || !tri || !bu || !bv || !rd3 || !ns3) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_test_shading_normal: upload triangles first");
  if (!ctx->surf.vn.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_shading_normal: no vertex normals (dmt_upload_vertex_normals first)");
  if (mapped) {
    if (int const rc = sceneReady(ctx, "dmt_test_shading_normal_mapped", false)) return rc;
    if (!ctx->scene.haveBsdfs || ctx->surf.tex.count == 0 || !ctx->surf.texturesMatch(ctx->scene.bsdfCount, ctx->scene.triCount))
      return fail(ctx, DMT_ERR_STATE, "dmt_test_shading_normal_mapped: BSDFs and textures (matching the uploaded BSDFs / triangles) first");
  }
  for (int i = 0; i < n; ++i)
    if (tri[i] < 0 || size_t(tri[i]) >= ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "dmt_test_shading_normal: triangle index out of range");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dTri(p, tri, 1);
  ProbeIn<float> dBu(p, bu, 1), dBv(p, bv, 1), dRd(p, rd3, 3);
  ProbeOut<float> dNs(p, ns3, 3);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(mapped ? k_test_shading_normal<true> : k_test_shading_normal<false>, dim3(p.blocks(64)), dim3(64), 0, ctx->stream,
                     baseParams(ctx, p.threads(64)), n, dTri.get(), dBu.get(), dBv.get(), dRd.get(), dNs.get());
  return finishProbe(ctx, p);
}
int dmt_test_shading_normal(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* rd3, float* ns3) {
  return probeShadingNormal(ctx, false, n, tri, bu, bv, rd3, ns3);
}
int dmt_test_shading_normal_mapped(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* rd3, float* ns3) {
  return probeShadingNormal(ctx, true, n, tri, bu, bv, rd3, ns3);
}

int dmt_test_opacity(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, float* alpha8, uint8_t* pass) {
  if (!ctx || n < 0 || !tri || !bu || !bv || !alpha8 || !pass) return DMT_ERR_INVALID;
  if (!ctx->surf.op.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_opacity: no opacity (dmt_upload_opacity first)");
  for (int i = 0; i < n; ++i)
    if (tri[i] < 0 || size_t(tri[i]) >= ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "dmt_test_opacity: triangle index out of range");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dTri(p, tri, 1);
  ProbeIn<float> dBu(p, bu, 1), dBv(p, bv, 1);
  ProbeOut<float> dA(p, alpha8, 1);
  ProbeOut<uint8_t> dP(p, pass, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_opacity, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), n, dTri.get(), dBu.get(),
                     dBv.get(), dA.get(), dP.get());
  return finishProbe(ctx, p);
}

int dmt_test_closest_hit_opacity(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* tmax, int32_t* tri_index, float* t,
                                 float* uv2, uint8_t* occluded) {
  if (!ctx || nrays < 0 || !o3 || !d3 || !tmax || !tri_index || !t) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_test_closest_hit_opacity: upload triangles first");
  if (!ctx->surf.op.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_closest_hit_opacity: no opacity (dmt_upload_opacity first)");
  if (nrays == 0) return DMT_OK;
  Probe p(ctx->device, size_t(nrays));
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3), dM(p, tmax, 1);
  ProbeOut<int32_t> di(p, tri_index, 1);
  ProbeOut<float> dt(p, t, 1), duv(p, uv2, 2);  // uv2, occluded optional: null is not copied back
  ProbeOut<uint8_t> docc(p, occluded, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  bool const useBvh = ctx->accel == DMT_ACCEL_BVH;
  if (useBvh) {
    if (int const rcT = requireTree(ctx, "dmt_test_closest_hit_opacity")) return rcT;
    HIP_TRY(ctx, reserveOverflow(ctx, p.threads(64)));
  }
  hipLaunchKernelGGL(k_test_closest_cut, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, baseParams(ctx, p.threads(64)), useBvh, nrays, dO.get(),
                     dD.get(), dM.get(), di.get(), dt.get(), duv.get(), docc.get());
  return finishProbe(ctx, p);
}

int dmt_test_medium(dmt_ctx* ctx, const float* medium8, int n, const float* o3, const float* d3, const float* t_hit, const uint32_t* h, const uint32_t* depth, const float* cosine, const float* u2, float* seg2, int32_t* hit,
                    float* values3, float* eval, float* wi3, float* pdf) {
  if (!ctx || !medium8 || n < 0 || !o3 || !d3 || !t_hit || !h || !depth || !cosine || !u2 || !seg2 || !hit || !values3 || !eval || !wi3 || !pdf) return DMT_ERR_INVALID;
  float const sigma_t = medium8[0], g = medium8[1], *const box_min3 = medium8 + 2, *const box_max3 = medium8 + 5;
  float const white[3] = {1.f, 1.f, 1.f};
  if (char const* const why = mediumArgsError(sigma_t, white, g, box_min3, box_max3)) return mediumRefused(ctx, "dmt_test_medium", why);
  if (!(sigma_t > 0.f)) return fail(ctx, DMT_ERR_INVALID, "dmt_test_medium: sigma_t must be > 0 (the free-flight distance divides by it)");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3), dT(p, t_hit, 1), dC(p, cosine, 1), dU(p, u2, 2);
  ProbeIn<uint32_t> dH(p, h, 1), dDepth(p, depth, 1);
  ProbeOut<float> dSeg(p, seg2, 2), dVal(p, values3, 3), dEval(p, eval, 1), dWi(p, wi3, 3), dPdf(p, pdf, 1);
  ProbeOut<int32_t> dHit(p, hit, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  MediumParams m{};
  m.sigmaT = sigma_t, m.g = g;
  for (int i = 0; i < 3; ++i) m.albedo[i] = 1.f, m.lo[i] = box_min3[i], m.hi[i] = box_max3[i];
  hipLaunchKernelGGL(k_test_medium, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, m, n, dO.get(), dD.get(), dT.get(), dH.get(), dDepth.get(), dC.get(),
                     dU.get(), dSeg.get(), dHit.get(), dVal.get(), dEval.get(), dWi.get(), dPdf.get());
  return finishProbe(ctx, p);
}

int dmt_test_medium_grid(dmt_ctx* ctx, const float* medium7, int nx, int ny, int nz, const float* density, int n, const float* o3, const float* d3,
                         const float* t_end, const float* tau_target, float* tau, float* ts, int32_t* collided, int32_t* steps) {
  if (!ctx || !medium7 || n < 0 || !o3 || !d3 || !t_end || !tau_target || !tau || !ts || !collided || !steps) return DMT_ERR_INVALID;
  float const sigma_t = medium7[0], *const box_min3 = medium7 + 1, *const box_max3 = medium7 + 4;
  MediumGridParams g;
  std::string why;
  if (char const* const e = mediumGridCallRecord(box_min3, box_max3, sigma_t, nx, ny, nz, density, g, why)) return mediumRefused(ctx, "dmt_test_medium_grid", e);
  if (n == 0) return DMT_OK;
  if (g.imin[0] > g.imax[0]) {  // no density > 0: nothing to march, as the host twin
    for (int i = 0; i < n; ++i) tau[i] = 0.f, ts[i] = 0.f, collided[i] = 0, steps[i] = 0;
    return DMT_OK;
  }
  Probe p(ctx->device, size_t(n));
  DevBuf<float> dGrid;
  p.ok(dGrid.assign(density, size_t(nx) * size_t(ny) * size_t(nz)), "hipMalloc + hipMemcpy (probe grid to device)");
  ProbeIn<float> dO(p, o3, 3), dD(p, d3, 3), dT(p, t_end, 1), dTarget(p, tau_target, 1);
  ProbeOut<float> dTau(p, tau, 1), dTs(p, ts, 1);
  ProbeOut<int32_t> dColl(p, collided, 1), dSteps(p, steps, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  g.density = dGrid.get();
  MediumParams m{};
  m.sigmaT = sigma_t;
  for (int i = 0; i < 3; ++i) m.albedo[i] = 1.f, m.lo[i] = box_min3[i], m.hi[i] = box_max3[i];
  hipLaunchKernelGGL(k_test_medium_grid, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, m, g, n, dO.get(), dD.get(), dT.get(), dTarget.get(),
                     dTau.get(), dTs.get(), dColl.get(), dSteps.get());
  return finishProbe(ctx, p);
}

int dmt_test_medium_spectrum(dmt_ctx* ctx, const float* k3, int n, const float* beta3, const uint32_t* h, const uint32_t* depth, const float* tau_seg,
                             int32_t* channel, int32_t* collided, float* tau_at, float* weight3) {
  if (!ctx || n < 0 || !beta3 || !h || !depth || !tau_seg || !channel || !collided || !tau_at || !weight3) return DMT_ERR_INVALID;
  MediumSpectrumParams sp{};
  if (char const* const why = mediumSpectrumCallRecord(k3, sp.q)) return mediumRefused(ctx, "dmt_test_medium_spectrum", why);
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<float> dBeta(p, beta3, 3), dTau(p, tau_seg, 1);
  ProbeIn<uint32_t> dH(p, h, 1), dDepth(p, depth, 1);
  ProbeOut<int32_t> dCh(p, channel, 1), dColl(p, collided, 1);
  ProbeOut<float> dAt(p, tau_at, 1), dW(p, weight3, 3);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_medium_spectrum, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, sp, n, dBeta.get(), dH.get(), dDepth.get(), dTau.get(),
                     dCh.get(), dColl.get(), dAt.get(), dW.get());
  return finishProbe(ctx, p);
}

int dmt_test_shutter_times(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* t) {
  if (!ctx || n < 0 || !pxs || !pys || !ss || !t) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_test_shutter_times: set the camera first");
  if (n == 0) return DMT_OK;
  Probe p(ctx->device, size_t(n));
  ProbeIn<int32_t> dpx(p, pxs, 1), dpy(p, pys, 1), dss(p, ss, 1);
  ProbeOut<float> dT(p, t, 1);
  if (p.err != hipSuccess) return probeError(ctx, p);
  hipLaunchKernelGGL(k_test_shutter, dim3(p.blocks(64)), dim3(64), 0, ctx->stream, ctx->camera.sp, ctx->ac.shutterOpen, ctx->ac.shutterClose, n, dpx.get(),
                     dpy.get(), dss.get(), dT.get());
  return finishProbe(ctx, p);
}

}  // extern "C"
