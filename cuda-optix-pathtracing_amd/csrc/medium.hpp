// medium.hpp -- the participating medium (dmt_set_medium): one homogeneous fog in an axis-aligned box, grey
// extinction, Henyey-Greenstein phase function, sampled in-path between two ray casts.  include/dmt_hip.h states the
// definition for callers.
//
// Part of dmt_hip.hip's translation unit, included once after pt_device.hpp.  This file is what the device and the host
// twins (dmt_medium_segment, dmt_medium_values, dmt_phase_hg) share, one body each, the way lens_ray_parts and motion_lerp
// are shared; medium_device.hpp holds the device code that the *_medium rows of path_shade call.
#pragma once

namespace dmt {

struct MediumParams {  // the tail of RenderParams; sigmaT == 0 in every launch without a medium
  float sigmaT, g;
  float albedo[3];
  float lo[3], hi[3];
};

// ---- shared by the device and the host ------------------------------------------------------------------------------
// 1 / d, correctly rounded on both sides: the quotient in double, rounded once more to float (innocuous for a quotient of
// floats: 53 >= 2 * 24 + 2).  The device's own fp32 division is a v_rcp_f32 (1 ulp); double division is IEEE everywhere.
// (The opaque copy keeps the compiler from narrowing the expression back into an fp32 division.)
__host__ __device__ inline float medium_rcp(float d) {
  double q = 1.0 / double(d);
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(q));
#endif
  return float(q);
}
constexpr float kMediumParallel = 0x1p-100f;  // |d| below this: the ray runs parallel to the axis' two planes

// The clip of the ray o + t d against the box [lo, hi], intersected with [0, tHit] (tHit may be +inf).  fp32, no
// contraction, one order of operations.  Per axis: a parallel ray (|d| < 2^-100) leaves the interval alone when
// lo <= o <= hi and empties it otherwise; else inv = medium_rcp(d), ta = (lo - o) * inv, tb = (hi - o) * inv, and the
// interval becomes [max(t0, min(ta, tb)), min(t1, max(ta, tb))].  Returns whether t0 < t1; *t0 and *t1 are written either way.
__host__ __device__ inline bool medium_segment(float const* o, float const* d, float tHit, float const* lo, float const* hi, float* t0out,
                                               float* t1out) {
#pragma clang fp contract(off)
  float t0 = 0.0f, t1 = tHit;
  bool outside = false;
  for (int a = 0; a < 3; ++a) {
    if (__builtin_fabsf(d[a]) < kMediumParallel) {
      outside = outside || o[a] < lo[a] || o[a] > hi[a];
    } else {
      float const inv = medium_rcp(d[a]);
      float const ta = (lo[a] - o[a]) * inv, tb = (hi[a] - o[a]) * inv;
      float const tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
      t0 = tn > t0 ? tn : t0;
      t1 = tf < t1 ? tf : t1;
    }
  }
  if (outside) t1 = t0;
  *t0out = t0, *t1out = t1;
  return t0 < t1;
}

// The free-flight number of the sample with Halton index h at path depth `depth`: a hash, not a low-discrepancy
// dimension (the sampler's eight cycling values are all spoken for), in [0, 1).
__host__ __device__ inline float medium_u(uint32_t h, uint32_t depth) {
  uint32_t const x = mix_bits32_c(h ^ mix_bits32_c(0x9E3779B9u * (depth + 1u)));
  return float(x >> 8) * 0x1p-24f;
}

// Henyey-Greenstein, pbrt's convention: c = dot(wo, wi) with wo pointing back along the arriving ray, so c = -1 is straight
// on.  1 + g^2 + 2 g c is formed as (1 - |g|)^2 + 2 |g| (1 + sign(g) c): every term is non-negative, so the peak of a
// strongly forward (or backward) lobe does not cancel.
__host__ __device__ inline float hg_eval(float g, float c) {
#pragma clang fp contract(off)
  float const a = __builtin_fabsf(g), oma = 1.0f - a;
  float const s = __builtin_fmaxf(g < 0.0f ? 1.0f - c : 1.0f + c, 0.0f);
  float const denom = oma * oma + (2.0f * a) * s;
  return 0.0795774715459476679f * ((oma * (1.0f + a)) / (denom * __builtin_sqrtf(denom)));
}
// the sampled c = dot(wo, wi) for the number u: pbrt's inversion, isotropic below |g| = 1e-3
__host__ __device__ inline float hg_cos_theta(float g, float u) {
#pragma clang fp contract(off)
  float c;
  if (__builtin_fabsf(g) < 1e-3f) {
    c = 1.0f - 2.0f * u;
  } else {
    float const t = (1.0f - g * g) / (1.0f + g - 2.0f * g * u);
    c = -(1.0f + g * g - t * t) / (2.0f * g);
  }
  return __builtin_fminf(__builtin_fmaxf(c, -1.0f), 1.0f);
}
// wi for (u.x, u.y) around the unit vector wo, and its pdf = hg_eval at the sampled cosine.  The frame is gram_schmidt's
// (common_math.cuh:453-465); the device takes its own sine, cosine and reciprocal square root, the host the library's.
__host__ __device__ inline void hg_sample(float g, float const* wo, float ux, float uy, float* wi, float* pdf) {
  float const c = hg_cos_theta(g, ux);
  float const s = __builtin_sqrtf(__builtin_fmaxf(1.0f - c * c, 0.0f));
  float const phi = 6.28318530717958647692f * uy;
  float sn, cs, a[3];
  if (__builtin_fabsf(wo[0] - wo[1]) > 1e-3f || __builtin_fabsf(wo[0] - wo[2]) > 1e-3f)
    a[0] = wo[2] - wo[1], a[1] = wo[0] - wo[2], a[2] = wo[1] - wo[0];
  else
    a[0] = wo[2] - wo[1], a[1] = wo[0] + wo[2], a[2] = -wo[1] - wo[0];
#if defined(__HIP_DEVICE_COMPILE__)
  dmt::sincos_bounded(phi, sn, cs);
  float const inv = dmt::rsqrt_ieee(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
#else
  sn = sinf(phi), cs = cosf(phi);
  float const inv = 1.0f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
#endif
  a[0] *= inv, a[1] *= inv, a[2] *= inv;
  float const b[3] = {wo[1] * a[2] - wo[2] * a[1], wo[2] * a[0] - wo[0] * a[2], wo[0] * a[1] - wo[1] * a[0]};
  for (int i = 0; i < 3; ++i) wi[i] = (s * cs) * a[i] + (s * sn) * b[i] + c * wo[i];
  *pdf = hg_eval(g, c);
}

}  // namespace dmt
