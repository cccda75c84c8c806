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

// ---- the medium's spectrum (dmt_set_medium_spectrum) ------------------------------------------------
// Channel extinctions k_c = sigma_t e_c and an emission.  Every clip and march runs once, in the reference channel m (the
// largest k; MediumParams::sigmaT holds k_m in a spectrum launch); the other channels' optical depths are q_c tau_m.
struct MediumSpectrumParams {  // the tail of RenderParams after MediumGridParams; read by the *_rgb rows only
  float q[3];   // k_c / k_m, correctly rounded on the host; q[m] == 1
  float le[3];  // emitted radiance
};
// the stream of the channel choice: medium_u(h, depth + kMediumChoiceStream).  dmt_set_limits admits every depth an int
// holds, so the offset is 2^31 and not 65536: depth + 1 and depth + 1 + 2^31 never meet below 2^31
constexpr uint32_t kMediumChoiceStream = 0x80000000u;
// q_c = k_c / k_m, correctly rounded (host): the quotient in double, rounded once more to float, as medium_rcp
inline float medium_spectrum_q(float k, float km) { return float(double(k) / double(km)); }

// -log(y) for y = 1 - u, u = medium_u(..): a multiple of 2^-24 in [2^-24, 1], so y is exact.  In double, by operations that
// are IEEE on both sides (no contraction, one division), rounded once to float: the device and the host get the same
// bits, which the library's log1pf does not promise.  y = 2^e m with m in (sqrt(1/2), sqrt(2)]; log m = 2 atanh(s),
// s = (m - 1) / (m + 1), |s| <= 0.1716, the series to s^13 (the next term is below 3e-12 of the sum).
__host__ __device__ inline double medium_neg_log(float y) {
#pragma clang fp contract(off)
  uint32_t bits;
  __builtin_memcpy(&bits, &y, 4);
  int e = int(bits >> 23) - 127;
  uint32_t const mant = (bits & 0x7FFFFFu) | 0x3F800000u;
  float mf;
  __builtin_memcpy(&mf, &mant, 4);
  if (mf > 1.41421356f) mf *= 0.5f, ++e;
  double const m = double(mf);
  double s = (m - 1.0) / (m + 1.0);
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(s));  // (as in medium_rcp: keeps the quotient in double)
#endif
  double const z = s * s;
  double const poly = 1.0 + z * (1.0 / 3.0 + z * (1.0 / 5.0 + z * (1.0 / 7.0 + z * (1.0 / 9.0 + z * (1.0 / 11.0 + z * (1.0 / 13.0))))));
  return 0.0 - (double(e) * 0.693147180559945309417 + (2.0 * s) * poly);
}

struct MediumSpectrumChoice {
  int channel;  // j; -1 when beta is all zero (the event is then a pass with weights 1)
  float T;      // the target optical depth in channel m, +inf when q_j == 0
  float p[3];   // the choice probabilities beta_c / (beta_0 + beta_1 + beta_2)
};
struct MediumSpectrumEvent {
  int channel, collided;
  float tauAt;  // channel-m optical depth at the event: T on a collision, tauSeg on a pass
  float w[3];   // the factors of beta
};
// Steps 1 and 2 of the event: the channel j with probability p_j by the second hash stream, and the target in channel m.
// The cumulative sums are compared without a division, so the choice is exact on both sides; a channel with beta == 0 is
// never chosen, whatever the last sum rounds to.  Nothing here indexes an array by j.
__host__ __device__ inline MediumSpectrumChoice medium_spectrum_choose(float const* q, float const* beta, uint32_t h, uint32_t depth) {
#pragma clang fp contract(off)
  MediumSpectrumChoice c;
  float const b0 = beta[0], b1 = beta[1], b2 = beta[2];
  float const s01 = b0 + b1, sum = s01 + b2;
  c.channel = -1, c.T = __builtin_huge_valf(), c.p[0] = c.p[1] = c.p[2] = 0.0f;
  if (!(sum > 0.0f) || !(sum < __builtin_huge_valf())) return c;
  float const x = medium_u(h, depth + kMediumChoiceStream) * sum;
  int j = x < b0 ? 0 : (x < s01 ? 1 : 2);
  if (j == 2 && !(b2 > 0.0f)) j = b1 > 0.0f ? 1 : 0;
  if (j == 1 && !(b1 > 0.0f)) j = 0;
  c.channel = j;
  c.p[0] = b0 / sum, c.p[1] = b1 / sum, c.p[2] = b2 / sum;
  float const qj = j == 0 ? q[0] : (j == 1 ? q[1] : q[2]);
  if (qj > 0.0f) {
    double t = medium_neg_log(1.0f - medium_u(h, depth)) / double(qj);
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(t));
#endif
    c.T = float(t);
  }
  return c;
}
// Steps 3 and 4: the one-sample balance heuristic over the three free-flight densities, at channel-m optical depth tauAt.
// Collision: w_c = q_c e^(-q_c T) / sum_i p_i q_i e^(-q_i T).  Pass: w_c = e^(-q_c tau) / sum_i p_i e^(-q_i tau).  A channel
// with q_c == 0 has optical depth 0 whatever tauAt is (+inf included).  The chosen channel's own term keeps the sum > 0.
__host__ __device__ inline MediumSpectrumEvent medium_spectrum_weights(float const* q, MediumSpectrumChoice const& c, bool collided, float tauAt) {
#pragma clang fp contract(off)
  MediumSpectrumEvent ev;
  ev.channel = c.channel, ev.collided = collided ? 1 : 0, ev.tauAt = tauAt;
  float n[3], sum = 0.0f;
  for (int i = 0; i < 3; ++i) {
    float const t = q[i] > 0.0f ? expf(-(q[i] * tauAt)) : 1.0f;
    n[i] = collided ? q[i] * t : t;
    sum += c.p[i] * n[i];
  }
  for (int i = 0; i < 3; ++i) ev.w[i] = c.channel < 0 ? 1.0f : n[i] / sum;
  return ev;
}
// The event of a path segment whose channel-m optical depth is tauSeg > 0 (+inf allowed): steps 1 to 4 in one body, which
// the homogeneous *_rgb rows, the probe dmt_test_medium_spectrum and the host twin dmt_medium_spectrum_event share.  The
// grid rows call its two halves around their march, which decides the collision (tau_target = T) and gives tauSeg.
__host__ __device__ inline MediumSpectrumEvent medium_spectrum_event(float const* q, float const* beta, uint32_t h, uint32_t depth, float tauSeg) {
  MediumSpectrumChoice const c = medium_spectrum_choose(q, beta, h, depth);
  bool const collided = c.channel >= 0 && c.T < tauSeg;
  return medium_spectrum_weights(q, c, collided, collided ? c.T : tauSeg);
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
