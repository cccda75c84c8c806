// denoise.hpp -- the image-space layer's device code and state: the feature pass (k_aov), the a-trous filter
// (k_denoise_init, k_atrous), temporal accumulation (k_temporal, project_point), and DenoiseState, what a context keeps for
// them.  DESIGN.md 4.11, 4.12.
//
// Part of dmt_hip.hip's translation unit, included once inside its anonymous namespace after wavefront.hpp: it uses the
// megakernel's device code (RenderParams, KArgs, tex_lookup, the closest-hit steps).  The entry points are in denoise_host.hpp.
#pragma once

// ---------------------------------------------------------------------------------------------
// denoiser (dmt_render_aovs, dmt_denoise)
// ---------------------------------------------------------------------------------------------
// Feature pass: camera samples 0 .. aovSpp-1 of every pixel of the frame, the film's own camera rays (lens rays under
// dmt_set_lens, so the features blur where the image blurs), closest hit as
// k_test_closest finds it.  Per pixel, summed in sample order over the samples whose ray hit a triangle ("hits"):
//   albedo   = (sum W / aovSpp, hits / aovSpp)     W = the record's fp16 weight after the level-0 texture patch;
//                                                   BS_GGX_BLEND: (1 - mix) W_diel + mix W_cond, mix clamped to [0, 1]
//   normal   = (normalize(sum ns) or 0 when |sum| < 1e-6, 0)   ns = hit_finish's face-forwarded or the normal-mapped normal
//   position = (sum pos / hits, sum t / hits), 0 without hits
//   surface  = (tri, bu, bv, 1) of the first sample that hit, tri the original index as a float; (-1, 0, 0, 0) without hits
struct AovArgs {
  float4* albedo;
  float4* normal;
  float4* position;
  float4* surface;
  int width;
  uint32_t pixels, aovSpp;
  bool useBvh;
};
DMT_DEV f3 rec_weight(Rec32 const& r) { return mk3(h2f(lo16(r.w[0])), h2f(hi16(r.w[0])), h2f(lo16(r.w[1]))); }
// The part of apply_material_textures (level 0) that W and the shading normal depend on: the albedo patch of Oren-Nayar
// records and the normal map, same expressions.  Its roughness patch is left out: nothing here reads it, and patching a
// word chosen by the record's type kept the record in scratch memory.
DMT_DEV f3 aov_textures(KArgs k, Rec32& rec, uint32_t matId, int tri, float bu, float bv, f3 ng) {
  KArgs const ka = kargs(k);
  uint32_t const* const m = ka->matTex + 4 * matId;
  int32_t const texD = int32_t(m[0]), texN = int32_t(m[2]);
  if (texD < 0 && texN < 0) return ng;
  float const* const uv = ka->triUv + 6 * size_t(tri);
  float const w0 = 1.f - bu - bv;
  float const s = w0 * uv[0] + bu * uv[2] + bv * uv[4], t = w0 * uv[1] + bu * uv[3] + bv * uv[5];
  if (texD >= 0 && hi16(rec.w[1]) == BS_OREN) {
    f3 const c = tex_lookup<false>(k, texD, s, t, false, TexDiff{});
    rec.w[0] = f2h(fmaxf(0.f, fminf(c.x, 1.f))) | (f2h(fmaxf(0.f, fminf(c.y, 1.f))) << 16);
    rec.w[1] = (rec.w[1] & 0xFFFF0000u) | f2h(fmaxf(0.f, fminf(c.z, 1.f)));
  }
  if (texN < 0) return ng;
  f3 n = tex_lookup<false>(k, texN, s, t, true, TexDiff{});
  auto quant = [](float v) { return float(int(v * 1023.f + 0.5f)) / 1023.f; };
  n = normalize(mk3(quant(n.x), quant(n.y), quant(n.z)));
  f3 tx, ty;
  gram_schmidt(ng, tx, ty);
  f3 const ns = tx * n.x + ty * n.y + ng * n.z;
  float const l2 = dot(ns, ns);
  return (l2 > 0.f && l2 < kInf) ? ns / sqrtf(l2) : ng;
}
// W and the shading normal at a camera ray's hit, as path_shade sees them at depth 0 (level-0 texture lookups).  VN: the
// smooth normal of the vertex-normal rows, under the normal map where there is one
template <bool VN = false>
DMT_DEV void aov_material(KArgs k, Hit const& hit, int tri, float bu, float bv, f3& W, f3& ns) {
  SceneView const sc = load_scene(k);
  bool const tex = kargs(k)->matTex != nullptr;
  Rec32 rec = sc.bsdfs[hit.matId];
  ns = hit.normal;
  if constexpr (VN) ns = shading_normal_at(k, tri, bu, bv, hit.normal);
  if (tex) ns = aov_textures(k, rec, hit.matId, tri, bu, bv, ns);
  if (hi16(rec.w[1]) == BS_GGX_BLEND) {  // GGX: the albedo patch never applies, to either record
    float const mix = fminf(fmaxf(blend_metallic(k, rec, hit.matId, tri, bu, bv), 0.f), 1.f);
    f3 Wd = rec_weight(rec);
    Wd.x = 1.f;  // the dielectric half keeps the metallic fraction where its W.x would be (makeGGXBlendDielectric)
    W = Wd * (1.f - mix) + rec_weight(sc.bsdfs[hit.matId + 1u]) * mix;
    return;
  }
  W = rec_weight(rec);
}
// one lane per pixel, row-major; whole waves stride over the frame (the BVH overflow stack is sized by the launch)
// MOTION (k_aov_motion, launched while key 1 is present): every sample is traced at its own time, as the film's is, so the
// planes blur where the film blurs; the post-hit record is the triangle's at that time.
// VN (k_aov_vn, launched while vertex normals are present): the normal plane accumulates the smooth shading normal.
// CUT (k_aov_cut, launched while opacity is present): the camera rays see through the holes, as the film's do, so the planes
// show what lies behind a cutout.
template <bool MOTION, bool VN = false, bool CUT = false>
DMT_DEV void aov_body(AovArgs const& A) {
  KArgs const k = kargs_base();
  if constexpr (!MOTION && !CUT) {
    if (!A.useBvh) cull_stage(k);
  }
  uint32_t const lane = threadIdx.x & 63u, gtid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t const waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t w = gtid >> 6; w * 64u < A.pixels; w += waves) {  // wave-uniform trip count
    uint32_t const i = w * 64u + lane;
    bool const alive = i < A.pixels;
    int const px = alive ? int(i % uint32_t(A.width)) : 0, py = alive ? int(i / uint32_t(A.width)) : 0;
    int32_t const base = halton_pixel_base(load_cold_args(k).sp, px, py);
    f3 sumW = mk3(0, 0, 0), sumN = mk3(0, 0, 0), sumP = mk3(0, 0, 0);
    float sumT = 0.f;
    uint32_t hits = 0;
    for (uint32_t s = 0; s < A.aovSpp; ++s) {
      PathState st{};
      // camera and sampler re-read from the kernel arguments at the point of use: held in SGPRs across the triangle pass
      // they would spill (see kargs)
      ColdArgs const c = load_cold_args(k);
      Ray const r = camera_ray_any(c.cam, c.sp, px, py, base + int32_t(s) * (c.sp.scale0 * c.sp.scale1), load_camera_extra(k));  // the film's rays: lens rays under a lens, filtered positions under a pixel filter
      set_ray(st, r.o, r.d);
      st.active = alive;
      int best;
      float bu, bv;
      bool occluded;
      float bt = kInf;
      if constexpr (MOTION) {
        float const tm = motion_sample_time(k, base, s);
        motion_set_time(tm);
        if (A.useBvh)
          trace_pair_bvh_motion(k, st, alive, false, v2f{tm, tm}, gtid, best, bu, bv, occluded, &bt);
        else
          trace_pair_brute_motion(k, st, alive, false, v2f{tm, tm}, best, bu, bv, occluded, &bt);
      } else if constexpr (CUT) {
        if (A.useBvh)
          trace_pair_bvh_cut(k, st, alive, false, gtid, best, bu, bv, occluded);
        else
          trace_pair_brute_cut(k, st, alive, false, best, bu, bv, occluded);
      } else {
        if (A.useBvh)
          trace_pair_bvh(k, st, alive, false, gtid, best, bu, bv, occluded);
        else
          trace_pair_brute(k, st, alive, false, best, bu, bv, occluded);
      }
      if (alive && best >= 0) {
        float t;
        if constexpr (MOTION) {
          t = bt;  // the trace's own
        } else {
          TriS const T = load_tri(to_const_as(load_scene(k).tris), uint32_t(best));
          t = mt_pair(T, st.rp).t.x;  // as k_test_closest reports it
        }
        Hit const hit = shade_hit<MOTION ? kFeatMotion : 0u>(k, load_scene(k), best, bu, bv, r.d);
        f3 W, ns;
        aov_material<VN>(k, hit, best, bu, bv, W, ns);
        sumW = sumW + W, sumN = sumN + ns, sumP = sumP + hit.pos, sumT += t;
        if (hits == 0) A.surface[i] = make_float4(float(best), bu, bv, 1.f);  // stored here: nothing more to keep across the loop
        ++hits;
      }
    }
    if (alive) {
      float const inv = 1.f / float(A.aovSpp);
      A.albedo[i] = make_float4(sumW.x * inv, sumW.y * inv, sumW.z * inv, float(hits) * inv);
      float const len = sqrtf(dot(sumN, sumN));
      f3 const n = len >= 1e-6f ? sumN / len : mk3(0, 0, 0);
      A.normal[i] = make_float4(n.x, n.y, n.z, 0.f);
      float const h = float(hits);
      A.position[i] = hits ? make_float4(sumP.x / h, sumP.y / h, sumP.z / h, sumT / h) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (!hits) A.surface[i] = make_float4(-1.f, 0.f, 0.f, 0.f);
    }
  }
}
__global__ void __launch_bounds__(256) k_aov(RenderParams P, AovArgs A) { aov_body<false>(A); }
__global__ void __launch_bounds__(256) k_aov_motion(RenderParams P, AovArgs A) { aov_body<true>(A); }
__global__ void __launch_bounds__(256) k_aov_vn(RenderParams P, AovArgs A) { aov_body<false, true>(A); }
__global__ void __launch_bounds__(256) k_aov_cut(RenderParams P, AovArgs A) { aov_body<false, false, true>(A); }

// A-trous passes (spatial SVGF).  Colour and variance travel together as one float4 (rgb, v) per pixel, ping-ponged
// between passes; the AOVs stay fp32 (no packing), so tests/denoise_ref.py restates the filter on the same numbers.
struct DenoiseArgs {
  float4 const* mean;      // k_denoise_init: the source film
  float4 const* m2;
  float4 const* albedo;    // k_atrous: the AOVs
  float4 const* normal;
  float4 const* position;
  float4 const* src;       // (rgb, variance) of pass i
  float4* dst;             // of pass i + 1 (k_denoise_init: pass 0)
  uint32_t* bad;           // k_denoise_init: pixels with N < 2 or a non-finite mean / M2
  int width, height;
  float theta;             // sensor height / (focal length * image height): one pixel's angle
  float sigmaN, sigmaX, sigmaA, sigmaL;
  float tapDist[25];       // s * sqrt(dx^2 + dy^2) of tap (dx, dy) at [5 (dy + 2) + dx + 2]
  int step;                // s = 2^i
};
// c0 = mean.xyz, v0 = (M2.x + M2.y + M2.z) / (3 N (N - 1)); counts the pixels the filter refuses
__global__ void __launch_bounds__(256) k_denoise_init(DenoiseArgs A) {
#pragma clang fp contract(off)
  uint32_t const i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t const pixels = uint32_t(A.width) * uint32_t(A.height);
  bool badPx = false;
  if (i < pixels) {
    float4 const m = A.mean[i], v = A.m2[i];
    float const N = v.w;
    badPx = !(N >= 2.f) || !__builtin_isfinite(N) || !__builtin_isfinite(m.x) || !__builtin_isfinite(m.y) ||
            !__builtin_isfinite(m.z) || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z);
    float const var = ((v.x + v.y) + v.z) / ((3.f * N) * (N - 1.f));
    A.dst[i] = make_float4(m.x, m.y, m.z, var);
  }
  unsigned long long const b = __ballot(badPx);
  if ((threadIdx.x & 63u) == 0u && b != 0ull) atomicAdd(A.bad, uint32_t(__popcll(b)));
}
DMT_DEV float luminance(float4 c) {
#pragma clang fp contract(off)
  return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
}
// one pass at step s: block = 64 x 4 pixels, a wave = 64 pixels of one row (tap loads coalesce); centre AOVs loaded once
__global__ void __launch_bounds__(256) k_atrous(DenoiseArgs A) {
#pragma clang fp contract(off)
  int const px = int(blockIdx.x) * 64 + int(threadIdx.x & 63u), py = int(blockIdx.y) * 4 + int(threadIdx.x >> 6);
  if (px >= A.width || py >= A.height) return;
  size_t const W = size_t(A.width);
  size_t const p = size_t(py) * W + size_t(px);
  float4 const cp = A.src[p];
  float4 const ap = A.albedo[p];
  if (!(ap.w > 0.f)) {  // background only: passes through and feeds no one
    A.dst[p] = cp;
    return;
  }
  float4 const np = A.normal[p], xp = A.position[p];
  float gs = 0.f, gw = 0.f;  // 3x3 [1/4, 1/2, 1/4] blur of the variance, normalised over the in-image taps
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      int const qx = px + dx, qy = py + dy;
      if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height) continue;
      float const kk = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      gs = gs + kk * A.src[size_t(qy) * W + size_t(qx)].w;
      gw = gw + kk;
    }
  }
  float const lp = luminance(cp);
  float const lden = A.sigmaL * sqrtf(gs / gw) + 1e-10f;
  float const xden = (A.sigmaX * xp.w) * A.theta;
  float const a2 = A.sigmaA * A.sigmaA;
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      int const qx = px + dx * A.step, qy = py + dy * A.step;
      if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height) continue;
      float const hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
      float const hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
      float w = hx * hy;
      float4 cq = cp;
      if (dx != 0 || dy != 0) {
        size_t const q = size_t(qy) * W + size_t(qx);
        float4 const aq = A.albedo[q];
        if (!(aq.w > 0.f)) continue;
        float4 const nq = A.normal[q], xq = A.position[q];
        cq = A.src[q];
        float const nd = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
        float const wn = powf(fmaxf(0.f, nd), A.sigmaN);
        float const pd = fabsf((np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y)) + np.z * (xq.z - xp.z));
        float const wx = expf(-pd / (xden * A.tapDist[5 * (dy + 2) + dx + 2]));
        float const ar = ap.x - aq.x, ag = ap.y - aq.y, ab = ap.z - aq.z;
        float const wa = expf(-((ar * ar + ag * ag) + ab * ab) / a2);
        float const wl = expf(-fabsf(lp - luminance(cq)) / lden);
        w = (((w * wn) * wx) * wa) * wl;
      }
      sw = sw + w;
      sr = sr + w * cq.x, sg = sg + w * cq.y, sb = sb + w * cq.z;
      sv = sv + (w * w) * cq.w;
    }
  }
  A.dst[p] = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// Temporal accumulation (dmt_denoise_temporal).
// World-to-film projection, the inverse of camera_ray's film-to-ray map: render-space point -> the continuous film
// coordinates camera_ray calls (fx, fy), and the camera-space depth.  fp32, no contraction, one order of operations for the
// host (dmt_camera_project) and the device; tests/temporal_ref.py restates it.
struct ProjXf {
  float right[3], up[3], fwd[3];  // rows of camera-from-render's rotation (the columns of CameraXf::rfc)
  float pos[3];
  float focal, tx, ty;            // cameraFromRaster: x_cam = fx / ipx + tx, y_cam = fy / ipy + ty at z_cam = focal
  float ipx, ipy;                 // 1 / psx, 1 / -psy
};
struct Proj {
  float fx, fy, depth;
};
// a / b: IEEE on the host; on the device v_rcp_f32 plus one residual step, which rounds as the host does except in rare
// half-way cases (the library's device `/` is the 2.5-ulp one, see the Makefile)
__host__ __device__ inline float proj_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float const r = __builtin_amdgcn_rcpf(b);
  float const q = a * r;
  return __builtin_fmaf(__builtin_fmaf(-q, b, a), r, q);
#else
  return a / b;
#endif
}
__host__ __device__ inline Proj project_point(ProjXf const& c, float x, float y, float z) {
#pragma clang fp contract(off)
  float const dx = x - c.pos[0], dy = y - c.pos[1], dz = z - c.pos[2];
  float const cx = (c.right[0] * dx + c.right[1] * dy) + c.right[2] * dz;
  float const cy = (c.up[0] * dx + c.up[1] * dy) + c.up[2] * dz;
  float const cz = (c.fwd[0] * dx + c.fwd[1] * dy) + c.fwd[2] * dz;
  float const s = proj_div(c.focal, cz);
  Proj o;
  o.fx = (cx * s - c.tx) * c.ipx;
  o.fy = (cy * s - c.ty) * c.ipy;
  o.depth = cz;
  return o;
}
// X = w0 p0 + bu p1 + bv p2, w0 = (1 - bu) - bv, left to right per component; v = the triangle's 9 raw floats
DMT_DEV f3 surface_point(float const* v, float bu, float bv) {
#pragma clang fp contract(off)
  float const w0 = (1.f - bu) - bv;
  return mk3((w0 * v[0] + bu * v[3]) + bv * v[6], (w0 * v[1] + bu * v[4]) + bv * v[7], (w0 * v[2] + bu * v[5]) + bv * v[8]);
}
struct TemporalArgs {
  float4 const* cur;        // (rgb, v0) of the current film: k_denoise_init's plane
  float4 const* albedo;     // the current AOVs
  float4 const* normal;
  float4 const* surface;
  float const* vertsCur;    // 9 floats per triangle: the current frame's, the history frame's (may be the same array)
  float const* vertsPrev;
  float4 const* histCv;     // the history: accumulated (rgb, v), length, and the normal / position planes of its frame
  float const* histLen;
  float4 const* histNormal;
  float4 const* histPos;
  float4* outCv;            // the new history (the other half of the ping-pong)
  float* outLen;
  uint32_t* counts;         // [0] pixels reprojected, [1] pixels reset
  ProjXf camCur, camPrev;
  int width, height;
  uint32_t triCount;
  int haveHistory;          // 0: every pixel is reset
  float alpha, normalThreshold, planeThreshold;
  float thetaPrev;          // one pixel's angle under the history frame's camera
};
// one lane per pixel; block = 64 x 4 pixels, a wave = 64 pixels of one row, as k_atrous
__global__ void __launch_bounds__(256) k_temporal(TemporalArgs A) {
#pragma clang fp contract(off)
  int const px = int(blockIdx.x) * 64 + int(threadIdx.x & 63u), py = int(blockIdx.y) * 4 + int(threadIdx.x >> 6);
  bool const inside = px < A.width && py < A.height;
  bool reproj = false, reset = false;
  if (inside) {
    size_t const W = size_t(A.width);
    size_t const p = size_t(py) * W + size_t(px);
    float4 const cc = A.cur[p];
    bool const covered = A.albedo[p].w > 0.f;
    float4 out = cc;
    float hOut = covered ? 1.f : 0.f;
    float4 const sf = A.surface[p];
    // the index test also turns away a NaN and anything outside the vertex arrays
    if (covered && A.haveHistory && sf.x >= 0.f && sf.x < float(A.triCount)) {
      size_t const tri = size_t(uint32_t(sf.x));
      f3 const Xc = surface_point(A.vertsCur + 9 * tri, sf.y, sf.z), Xp = surface_point(A.vertsPrev + 9 * tri, sf.y, sf.z);
      Proj const qc = project_point(A.camCur, Xc.x, Xc.y, Xc.z), qp = project_point(A.camPrev, Xp.x, Xp.y, Xp.z);
      float const u = float(px) + (qp.fx - qc.fx), v = float(py) + (qp.fy - qc.fy);
      // inside (-1, width) x (-1, height): some tap of the 2 x 2 footprint can be in the image; false for a NaN
      if (qp.depth > 0.f && u > -1.f && u < float(A.width) && v > -1.f && v < float(A.height)) {
        float const fu0 = floorf(u), fv0 = floorf(v);
        int const iu = int(fu0), iv = int(fv0);
        float const fu = u - fu0, fv = v - fv0;
        float4 const np = A.normal[p];
        float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sh = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          int const qx = iu + (t & 1), qy = iv + (t >> 1);
          float const w = ((t & 1) ? fu : 1.f - fu) * ((t >> 1) ? fv : 1.f - fv);
          if (!(w > 0.f) || qx < 0 || qx >= A.width || qy < 0 || qy >= A.height) continue;
          size_t const q = size_t(qy) * W + size_t(qx);
          float const hq = A.histLen[q];
          if (!(hq >= 1.f)) continue;
          float4 const nq = A.histNormal[q];
          float const nd = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
          if (!(nd >= A.normalThreshold)) continue;
          float4 const xq = A.histPos[q];
          float const pd = fabsf((nq.x * (Xp.x - xq.x) + nq.y * (Xp.y - xq.y)) + nq.z * (Xp.z - xq.z));
          if (!(pd <= (A.planeThreshold * xq.w) * A.thetaPrev)) continue;
          float4 const cq = A.histCv[q];
          sw = sw + w;
          sr = sr + w * cq.x, sg = sg + w * cq.y, sb = sb + w * cq.z;
          sv = sv + (w * w) * cq.w;
          sh = sh + w * hq;
        }
        if (sw > 0.f) {
          reproj = true;
          float const h = fminf(sh / sw + 1.f, 65536.f);
          float const a = fmaxf(A.alpha, 1.f / h);
          hOut = h;
          if (a < 1.f) {  // a = 1 is the current frame itself, bit for bit
            float const pr = sr / sw, pg = sg / sw, pb = sb / sw, pv = sv / (sw * sw);
            float const b = 1.f - a;
            out = make_float4(pr + a * (cc.x - pr), pg + a * (cc.y - pg), pb + a * (cc.z - pb), (b * b) * pv + (a * a) * cc.w);
          }
        }
      }
    }
    reset = covered && !reproj;
    A.outCv[p] = out;
    A.outLen[p] = hOut;
  }
  unsigned long long const br = __ballot(reproj), bs = __ballot(reset);
  if ((threadIdx.x & 63u) == 0u) {
    if (br != 0ull) atomicAdd(A.counts, uint32_t(__popcll(br)));
    if (bs != 0ull) atomicAdd(A.counts + 1, uint32_t(__popcll(bs)));
  }
}

// What a context keeps for this layer.  Its operations need nothing else of the context; the ones that do (the vertex mirror
// of the updates, prepareHistory) are in denoise_host.hpp.
struct DenoiseState {
  // denoiser (dmt_render_aovs / dmt_upload_aovs, dmt_denoise): the three feature planes and their size (0 x 0: none); the
  // filter's scratch: a copy of a host film (mean, then M2), two (rgb, variance) planes, the count of refused pixels
  DevBuf<float4> albedo, normal, pos;
  int aovW = 0, aovH = 0;
  DevBuf<float4> film, cv;
  DevBuf<uint32_t> bad;
  // temporal accumulation (dmt_denoise_temporal).  The surface plane belongs to the AOVs; everything else is
  // allocated by the first temporal call (temporalOn), never before
  DevBuf<float4> surface;
  bool aovSurface = false;          // the surface plane matches the three AOV planes
  bool temporalOn = false;          // a temporal call was made: the updates keep tvCur current
  DevBuf<float4> histCv[2];         // accumulated (rgb, v), ping-pong; thSlot is the history
  DevBuf<float> histLen[2];
  DevBuf<float4> histNormal, histPos;  // the planes of the history's frame
  DevBuf<uint32_t> counts;          // [0] reprojected, [1] reset
  DevBuf<float> tvCur, tvPrev;      // raw vertices, 9 per triangle: current, and the history frame's once they differ
  bool tvValid = false;             // tvCur holds the uploaded soup
  bool tvPrevIsCur = true;          // no update since the history's frame: tvCur serves as both
  int thSlot = 0, thW = 0, thH = 0;
  bool thValid = false;             // false: the next call resets every pixel
  ProjXf thCam{};                   // the camera of the history's frame, and its pixel angle
  float thTheta = 0.f;
  dmt_temporal_record thRecord{};

  // the next temporal call resets every pixel; without a history frame no frame's vertices are kept apart from tvCur
  void dropHistory() { thValid = false, tvPrevIsCur = true, thRecord.frames = 0; }
  // a new soup: tvCur is not its vertices, and the history's triangle indices are not its triangles
  void dropVertexMirror() { tvValid = false, dropHistory(); }
  size_t historyBytes() const {
    return (histCv[0].size() + histCv[1].size() + histNormal.size() + histPos.size()) * sizeof(float4) +
           (histLen[0].size() + histLen[1].size() + tvCur.size() + tvPrev.size()) * sizeof(float) + counts.size() * sizeof(uint32_t);
  }
};
