// surface_device.hpp -- the device code of the surface-attribute layer: what a triangle or a material carries beyond its
// position and its BSDF record.  Emissive triangles (sampling and pdf), image textures (the level-0 bilinear lookup), the
// first-hit texture filter (footprint, MIP chain, EWA) and the patch of a packed BSDF record from its material's textures.
// Per-vertex normals and opacity records have headers of their own (vnormals.hpp, opacity.hpp).  What a context keeps for
// the layer is in surface_state.hpp, its entry points in surface_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once inside its anonymous namespace, after path_begin and before
// motion.hpp: it uses pt_device.hpp's vector math and records, KArgs / kargs and TriPost.
#pragma once

// ---- emissive triangles.  No reference implementation exists; semantics are pbrt-v4's, which the
// reference's scenes/cornell-box.pbrt is written for: DiffuseAreaLight, one-sided on n = normalize(cross(p1 - p0,
// p2 - p0)); uniform point sampling (SampleUniformTriangle); light chosen uniformly among [point/spot lights...,
// emissive triangles...]; power-heuristic MIS between light and BSDF sampling; emission seen directly by camera rays
// and after delta bounces.
struct AreaSampleDev {
  f3 wi;
  float dist, pdf;
  bool ok;
};
DMT_DEV AreaSampleDev area_sample(TriPost const& P, f3 p, f2 u) {
  AreaSampleDev r;
  r.ok = false, r.dist = 0.f, r.pdf = 0.f, r.wi = mk3(0, 0, 0);
  f3 const p0 = mk3(P.p0x, P.p0y, P.p0z), p1 = mk3(P.p1x, P.p1y, P.p1z), p2 = mk3(P.p2x, P.p2y, P.p2z);
  float b0, b1;
  if (u.x < u.y) {
    b0 = u.x / 2;
    b1 = u.y - b0;
  } else {
    b1 = u.y / 2;
    b0 = u.x - b1;
  }
  f3 const q = b0 * p0 + b1 * p1 + (1 - b0 - b1) * p2;
  f3 const c = cross(p1 - p0, p2 - p0);
  float const len = sqrtf(dot(c, c));
  if (!(len > 0.f)) return r;
  f3 const d = q - p;
  float const d2 = dot(d, d);
  if (!(d2 > 0.f)) return r;
  r.dist = sqrtf(d2);
  r.wi = d / r.dist;
  float const cosL = -dot(c / len, r.wi);
  if (!(cosL > 0.f)) return r;  // one-sided
  r.pdf = d2 / (cosL * (0.5f * len));
  r.ok = true;
  return r;
}
DMT_DEV float area_pdf(TriPost const& P, f3 rayD, float t) {
  f3 const p0 = mk3(P.p0x, P.p0y, P.p0z), p1 = mk3(P.p1x, P.p1y, P.p1z), p2 = mk3(P.p2x, P.p2y, P.p2z);
  f3 const c = cross(p1 - p0, p2 - p0);
  float const len = sqrtf(dot(c, c));
  if (!(len > 0.f)) return 0.f;
  float const cosL = -dot(c / len, rayD);
  if (!(cosL > 0.f)) return 0.f;
  return (t * t) / (cosL * (0.5f * len));
}

// ---- image textures of JSON materials.  The reference's megakernel path has none; semantics follow its CPU
// renderer (src/core/private/core-material.cpp:20-56,180-240; core-texture.cu:895-915): bilinear lookup at MIP level 0
// (this path carries no ray differentials, and the reference's isotropic fallback picks level 0 when its differentials
// vanish), mirror wrap, byte / 255, normal maps through Frame::fromZ(ng) after 10-bit quantisation.  The sampled albedo
// / roughness PATCH the packed record exactly as the host packers would have built it (makeOrenNayar, ggxCommon), so a
// textured and an untextured material take the same route through bsdf_prepare.
DMT_DEV f3 tex_texel(uint32_t const* rgba, int32_t first, int32_t w, int32_t h, int s, int t) {
  auto mirror = [](int c, int size) {
    int const p = size * 2;
    c %= p;
    if (c < 0) c += p;
    return c < size ? c : (p - c - 1);
  };
  uint32_t const px = rgba[size_t(first) + size_t(mirror(t, h)) * size_t(w) + size_t(mirror(s, w))];
  return mk3(float(px & 0xFFu) / 255.f, float((px >> 8) & 0xFFu) / 255.f, float((px >> 16) & 0xFFu) / 255.f);
}
DMT_DEV f3 tex_bilinear(KArgs k, int32_t tex, float s, float t, bool isNormal) {
  KArgs const ka = kargs(k);
  int32_t const* const d = ka->texDesc + 3 * tex;
  int32_t const first = d[0], w = d[1], h = d[2];
  uint32_t const* const rgba = ka->texRgba;
  float const x = s * float(w) - 0.5f, y = t * float(h) - 0.5f;
  float const fx = floorf(x), fy = floorf(y);
  int const x0 = int(fx), y0 = int(fy);
  float const tx = x - fx, ty = y - fy;
  f3 const c00 = tex_texel(rgba, first, w, h, x0, y0), c10 = tex_texel(rgba, first, w, h, x0 + 1, y0);
  f3 const c01 = tex_texel(rgba, first, w, h, x0, y0 + 1), c11 = tex_texel(rgba, first, w, h, x0 + 1, y0 + 1);
  f3 const cx0 = c00 * (1.f - tx) + c10 * tx, cx1 = c01 * (1.f - tx) + c11 * tx;
  f3 c = cx0 * (1.f - ty) + cx1 * ty;
  if (isNormal) c.x = c.x * 2.f - 1.f, c.y = c.y * 2.f - 1.f;
  return c;
}
// ---- first-hit texture filtering (DMT_TEXFILTER_REFERENCE, *_texf kernels).  The reference's CPU renderer
// filters every image-texture lookup at the camera ray's first hit by the pixel's footprint and looks up MIP level 0 at
// every later hit (core-render.cpp:264-268).  Restated here, with the reference's lines:
//   footprint   approximate_dp_dxy (core-texture.cu:55-87) with the frame's smallest camera differentials
//               (minDifferentialsFromCamera, core-render.cpp:928-980; host side, dmt_texture_footprint);
//               dpdu / dpdv (core-render.cpp:209-226); duv_From_dp_dxy, the #else branch (core-texture.cu:123-258);
//               zeroed when |cross(dpdx, dpdy)| < 1e-6 (core-render.cpp:264-268)
//   lookup      sampleMippedTexture (core-material.cpp:83-175): isotropic trilinear when no derivative is near zero (the
//               condition the reference names validDiffs, inverted, kept as written), else two EWA lookups (EWAFormula,
//               core-texture.cu:664-748) at the level of the UNclamped minor axis (computeTextureLOD_from_dudv, :595-662)
// Where the reference is undefined:
//   [fix 1] levels where one axis has reached 0 get resolution max(1, ...) (buildMipChain);
//   [fix 2] the second lookup of a pair past the last level reads the last level;
//   [fix 3] EWA with a zero-length shorter axis takes the isotropic branch (the clamp would compute 0 * inf);
//   [fix 4] an EWA lookup tests at most kEwaMaxTexels texel positions: while the ellipse's box at the reference's level
//           holds more, the level is raised (each level quarters the box); a box still too large at the last level, or
//           at the second level of the pair, takes the single-texel fallback of EWAFormula;
//   [fix 5] a triangle whose UV determinant is exactly 0 gets zero differentials.
// With zero differentials the lookup is tex_bilinear itself: the reference's lerp returns its first argument at t <= 0.
// The differentials and the EWA level are evaluated in double (see tex_footprint, ewa_lod_minor); the lookups in float.
#include "../../include/dmt_ewa_lut.inc"
__constant__ float kEwaLut[DMT_EWA_LUT_SIZE] = {DMT_EWA_LUT_VALUES};
constexpr float kEwaMaxTexels = 1024.f;  // [fix 4] texel positions per EWA lookup
constexpr float kMaxAnisotropy = 8.f;    // core-texture.h:210

struct TexDiff {  // d(u, v) / d(x, y) of the hit; all zero: the level-0 bilinear lookup
  float dudx, dudy, dvdx, dvdy;
};
struct TexProbe {  // what dmt_test_texture_filter reports: 0 level 0, 1 trilinear, 2 EWA, 3 EWA at a level raised by [fix 4]
  int branch;
  float lod;
};
struct TexLevel {
  uint32_t const* rgba;
  int32_t first, w, h;
};
DMT_DEV TexLevel tex_level(KArgs k, int32_t tex, int l) {
  KArgs const ka = kargs(k);
  int32_t const* const d = ka->texDesc + 3 * tex;
  TexLevel L;
  L.w = d[1], L.h = d[2];
  if (l == 0) {
    L.rgba = ka->texRgba, L.first = d[0];
    return L;
  }
  int32_t first = ka->texMipDesc[2 * tex + 1];
  for (int i = 1; i < l; ++i) first += max(1, L.w >> i) * max(1, L.h >> i);
  L.rgba = ka->texMip, L.first = first, L.w = max(1, L.w >> l), L.h = max(1, L.h >> l);
  return L;
}
DMT_DEV f3 lerp_rgb(f3 a, f3 b, float t) { return t <= 0.f ? a : (t >= 1.f ? b : (1.f - t) * a + t * b); }  // cudautils-color.cuh:112-114
// sampleBilinearTexel (core-material.cpp:20-56) on one level
DMT_DEV f3 tex_bilinear_level(TexLevel const& L, float s, float t, bool isNormal) {
  float const x = s * float(L.w) - 0.5f, y = t * float(L.h) - 0.5f;
  float const fx = floorf(x), fy = floorf(y);
  int const x0 = int(fx), y0 = int(fy);
  float const tx = x - fx, ty = y - fy;
  f3 const c00 = tex_texel(L.rgba, L.first, L.w, L.h, x0, y0), c10 = tex_texel(L.rgba, L.first, L.w, L.h, x0 + 1, y0);
  f3 const c01 = tex_texel(L.rgba, L.first, L.w, L.h, x0, y0 + 1), c11 = tex_texel(L.rgba, L.first, L.w, L.h, x0 + 1, y0 + 1);
  f3 c = lerp_rgb(lerp_rgb(c00, c10, tx), lerp_rgb(c01, c11, tx), ty);
  if (isNormal) c.x = c.x * 2.f - 1.f, c.y = c.y * 2.f - 1.f;
  return c;
}
// EWAFormula's ellipse and box at one level (core-texture.cu:664-712)
struct EwaBox {
  float A, B, C;
  int sx, sy;
  float s0, s1, t0, t1;
  float count;  // texel positions in the box (the loop never runs when it exceeds kEwaMaxTexels or is not a number)
};
DMT_DEV EwaBox ewa_box(int w, int h, float s, float t, f2 d0, f2 d1) {
#pragma clang fp contract(off)
  EwaBox b;
  float const d0x = d0.x * float(w), d0y = d0.y * float(h), d1x = d1.x * float(w), d1y = d1.y * float(h);
  b.sx = int(s * float(w) - 0.5f), b.sy = int(t * float(h) - 0.5f);  // truncated, not floored (as written)
  float A = d0y * d0y + d1y * d1y + 1.f;
  float B = -2.f * (d0x * d0y + d1x * d1y);
  float C = d0x * d0x + d1x * d1x + 1.f;
  float const invF = 1.f / (A * C - 0.25f * B * B);
  A *= invF, B *= invF, C *= invF;
  float const invDet = 1.f / (A * C - 0.25f * B * B);
  float const uR = safe_sqrt(C * invDet), vR = safe_sqrt(A * invDet);
  b.A = A, b.B = B, b.C = C;
  b.s0 = ceilf(float(b.sx) - uR), b.s1 = floorf(float(b.sx) + uR);
  b.t0 = ceilf(float(b.sy) - vR), b.t1 = floorf(float(b.sy) + vR);
  b.count = (b.s1 - b.s0 + 1.f) * (b.t1 - b.t0 + 1.f);
  return b;
}
DMT_DEV f3 ewa_texel(TexLevel const& L, int s, int t, bool isNormal) {
  f3 c = tex_texel(L.rgba, L.first, L.w, L.h, s, t);
  if (isNormal) c.x = c.x * 2.f - 1.f, c.y = c.y * 2.f - 1.f;  // remapNormal per texel (core-texture.h:233-240)
  return c;
}
DMT_DEV f3 ewa_lookup(TexLevel const& L, float s, float t, f2 d0, f2 d1, bool isNormal) {
#pragma clang fp contract(off)
  EwaBox const b = ewa_box(L.w, L.h, s, t, d0, d1);
  f3 sum = mk3(0.f, 0.f, 0.f);
  float sumW = 0.f;
  if (b.count <= kEwaMaxTexels) {  // [fix 4]; false for NaN
    int const s0 = int(b.s0), s1 = int(b.s1), t0 = int(b.t0), t1 = int(b.t1);
    for (int ti = t0; ti <= t1; ++ti) {
      float const tt = float(ti) - float(b.sy);
      for (int si = s0; si <= s1; ++si) {
        float const ss = float(si) - float(b.sx);
        float const r2 = b.A * ss * ss + b.B * ss * tt + b.C * tt * tt;
        if (r2 < 1.f) {
          float const w = kEwaLut[int(fminf(r2 * float(DMT_EWA_LUT_SIZE), float(DMT_EWA_LUT_SIZE - 1)))];
          sum = sum + ewa_texel(L, si, ti, isNormal) * w;
          sumW += w;
        }
      }
    }
  }
  if (!(sumW > 0.f)) return ewa_texel(L, b.sx, b.sy, isNormal);  // floor(sx + 0.5) of an int
  return mk3(sum.x / sumW, sum.y / sumW, sum.z / sumW);
}
// computeTextureLOD_from_dudv's lod_minor (core-texture.cu:595-662), in double: the smaller eigenvalue is a difference of
// two nearly equal numbers when the footprint is long and thin, where float would leave little of it
DMT_DEV float ewa_lod_minor(TexDiff const& d, int w, int h) {
  double const a0 = double(d.dudx) * w, a1 = double(d.dvdx) * h, b0 = double(d.dudy) * w, b1 = double(d.dvdy) * h;
  double const E = a0 * a0 + a1 * a1, F = b0 * b0 + b1 * b1, G = a0 * b0 + a1 * b1;
  double const eps = 1e-12;
  double const trace = E + F;
  double det = E * F - G * G;
  if (det < 0.0 && det > -eps) det = 0.0;
  if (trace <= eps) return 0.f;
  double discr = trace * trace - 4.0 * det;
  if (discr < 0.0) discr = 0.0;
  double l2 = 0.5 * (trace - sqrt(discr));
  if (l2 < 0.0 && l2 > -eps) l2 = 0.0;
  double const sigma = l2 > 0.0 ? sqrt(l2) : 0.0;
  return sigma > 0.0 ? float(fmax(0.0, log2(sigma))) : 0.f;
}
// sampleMippedTexture (core-material.cpp:83-175) with [fix 2-4]
template <bool PROBE>
DMT_DEV f3 tex_filtered(KArgs k, int32_t tex, float s, float t, bool isNormal, TexDiff const& d, TexProbe* pr) {
#pragma clang fp contract(off)
  if (d.dudx == 0.f && d.dudy == 0.f && d.dvdx == 0.f && d.dvdy == 0.f) {
    if constexpr (PROBE) pr->branch = 0, pr->lod = 0.f;
    return tex_bilinear(k, tex, s, t, isNormal);
  }
  KArgs const ka = kargs(k);
  int32_t const* const desc = ka->texDesc + 3 * tex;
  int const w = desc[1], h = desc[2];
  int const levels = ka->texMipDesc[2 * tex];
  f2 const dx = mk2(d.dudx, d.dvdx), dy = mk2(d.dudy, d.dvdy);
  bool const dxLonger = dot(dx, dx) > dot(dy, dy);
  f2 const d0 = dxLonger ? dx : dy;
  f2 d1 = dxLonger ? dy : dx;
  float const shorterLen = sqrtf(dot(d1, d1)), longerLen = sqrtf(dot(d0, d0));
  auto nearZero = [](float x) { return fabsf(x) < __FLT_EPSILON__; };
  bool const someNearZero = nearZero(d.dudx) || nearZero(d.dudy) || nearZero(d.dvdx) || nearZero(d.dvdy);
  if (!someNearZero || shorterLen == 0.f) {  // isotropic trilinear ([fix 3]: also for a zero-length shorter axis)
    float const dud = fmaxf(fabsf(d.dudx), fabsf(d.dudy)), dvd = fmaxf(fabsf(d.dvdx), fabsf(d.dvdy));
    float const rho = fmaxf(dud * float(w), dvd * float(h));
    float const lod = fmaxf(log2f(fmaxf(rho, 1e-8f)), 0.f);
    int const ilod = min(max(int(floorf(lod)), 0), levels - 1);
    float const tl = lod - float(ilod);
    if constexpr (PROBE) pr->branch = 1, pr->lod = lod;
    f3 const c0 = tex_bilinear_level(tex_level(k, tex, ilod), s, t, isNormal);
    f3 const c1 = tex_bilinear_level(tex_level(k, tex, min(ilod + 1, levels - 1)), s, t, isNormal);  // [fix 2]
    return lerp_rgb(c0, c1, tl);
  }
  if (float const den = shorterLen * kMaxAnisotropy; den < longerLen) {
    float const scale = longerLen / den;
    d1.x *= scale, d1.y *= scale;
  }
  float const lambda = ewa_lod_minor(d, w, h);
  int ilod = min(max(int(floorf(lambda)), 0), levels - 1);
  float const tl = lambda - float(ilod);
  TexLevel L0 = tex_level(k, tex, ilod);
  bool raised = false;
  while (ilod < levels - 1 && !(ewa_box(L0.w, L0.h, s, t, d0, d1).count <= kEwaMaxTexels)) {  // [fix 4]
    ++ilod, raised = true;
    L0 = tex_level(k, tex, ilod);
  }
  if constexpr (PROBE) pr->branch = raised ? 3 : 2, pr->lod = float(ilod) + tl;
  f3 const c0 = ewa_lookup(L0, s, t, d0, d1, isNormal);
  f3 const c1 = ewa_lookup(tex_level(k, tex, min(ilod + 1, levels - 1)), s, t, d0, d1, isNormal);  // [fix 2]
  return lerp_rgb(c0, c1, tl);
}
// one texture lookup of a material: level-0 bilinear, or (FILT) filtered by the hit's UV differentials
template <bool FILT>
DMT_DEV f3 tex_lookup(KArgs k, int32_t tex, float s, float t, bool isNormal, TexDiff const& d) {
  if constexpr (FILT) return tex_filtered<false>(k, tex, s, t, isNormal, d, nullptr);
  else return tex_bilinear(k, tex, s, t, isNormal);
}
// The footprint of one hit, evaluated in double (once per camera-ray hit; the result is rounded to float): a derivative that
// should vanish -- a UV axis orthogonal to dpdx or dpdy -- then stays far below the FLT_EPSILON test that picks the EWA branch.
struct d3 {
  double x, y, z;
};
DMT_DEV d3 md3(double x, double y, double z) { return d3{x, y, z}; }
DMT_DEV d3 operator+(d3 a, d3 b) { return md3(a.x + b.x, a.y + b.y, a.z + b.z); }
DMT_DEV d3 operator-(d3 a, d3 b) { return md3(a.x - b.x, a.y - b.y, a.z - b.z); }
DMT_DEV d3 operator*(d3 a, double s) { return md3(a.x * s, a.y * s, a.z * s); }
DMT_DEV double dotd(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DMT_DEV d3 crossd(d3 a, d3 b) { return md3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
DMT_DEV double lend(d3 a) { return sqrt(dotd(a, a)); }
DMT_DEV d3 normd(d3 a) {
  double const l = lend(a);
  return md3(a.x / l, a.y / l, a.z / l);
}
DMT_DEV d3 mul3(double const m[9], d3 v) {  // column-major
  return md3(m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z);
}
DMT_DEV d3 mul3T(double const m[9], d3 v) {  // transpose(m) v
  return md3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z);
}
DMT_DEV void inv3(double const m[9], double r[9]) {  // Transform's mInv = inverse(m)
  double const c0 = m[4] * m[8] - m[7] * m[5], c1 = m[7] * m[2] - m[1] * m[8], c2 = m[1] * m[5] - m[4] * m[2];
  double const inv = 1.0 / (m[0] * c0 + m[3] * c1 + m[6] * c2);
  r[0] = c0 * inv, r[1] = c1 * inv, r[2] = c2 * inv;
  r[3] = (m[6] * m[5] - m[3] * m[8]) * inv, r[4] = (m[0] * m[8] - m[6] * m[2]) * inv, r[5] = (m[3] * m[2] - m[0] * m[5]) * inv;
  r[6] = (m[3] * m[7] - m[6] * m[4]) * inv, r[7] = (m[6] * m[1] - m[0] * m[7]) * inv, r[8] = (m[0] * m[4] - m[3] * m[1]) * inv;
}
// the UV differentials of a camera ray's hit at p on triangle `tri` with geometric normal ng (any orientation)
DMT_DEV TexDiff tex_footprint(KArgs k, int tri, f3 pf, f3 ngf) {
#pragma clang fp contract(off)
  KArgs const ka = kargs(k);
  TexDiff r{0.f, 0.f, 0.f, 0.f};
  // approximate_dp_dxy (core-texture.cu:55-87): tangent plane in camera space, rotated so that the hit lies down +z
  auto const& c = ka->texCfr;
  d3 const p = md3(pf.x, pf.y, pf.z), ng = md3(ngf.x, ngf.y, ngf.z);
  d3 const pC = md3(c[0] * p.x + c[1] * p.y + c[2] * p.z + c[3], c[4] * p.x + c[5] * p.y + c[6] * p.z + c[7],
                    c[8] * p.x + c[9] * p.y + c[10] * p.z + c[11]);
  double rfc[9];  // cameraFromRender's inverse: the renderFromCamera rotation
  for (int i = 0; i < 3; ++i) rfc[i] = ka->cam.rfc[i], rfc[3 + i] = ka->cam.rfc[4 + i], rfc[6 + i] = ka->cam.rfc[8 + i];
  d3 const from = normd(pC);
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // Transform::rotateFromTo(from, +z), cudautils-transform.cu:87-147
  double const cosT = from.z;
  if (cosT > 1.0 - 1e-6) {
    // case 1: already aligned
  } else if (cosT < -1.0 + 1e-6) {  // case 2: opposite (its literal is read column by column, as Matrix4f stores it)
    d3 o = md3(1, 0, 0);
    if (fabs(dotd(from, o)) > 0.99) o = md3(0, 1, 0);
    d3 const a = normd(crossd(from, o));
    double const x = a.x, y = a.y, z = a.z, cc = -1.0, tt = 1.0 - cc;
    double const lit[9] = {tt * x * x + cc, tt * x * y - z, tt * z * x + y, tt * x * y + z, tt * y * y + cc, tt * y * z - x,
                           tt * z * x - y, tt * y * z + x, tt * z * z + cc};
    for (int i = 0; i < 9; ++i) R[i] = lit[i];
  } else {  // Rodrigues: I + [v]x + [v]x^2 (1 - c) / s^2, v = from x z
    double const x = from.y, y = -from.x, z = 0.0;
    double const s = sqrt(x * x + y * y + z * z);
    double const kk = (1.0 - cosT) / (s * s);
    double const vx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    double const vx2[9] = {-y * y - z * z, x * y, x * z, x * y, -x * x - z * z, y * z, x * z, y * z, -x * x - y * y};
    int const at[9] = {0, 3, 6, 1, 4, 7, 2, 5, 8};  // row-major entry i -> column-major slot
    for (int i = 0; i < 9; ++i) R[at[i]] += vx[i] + vx2[i] * kk;
  }
  double Ri[9];
  inv3(R, Ri);
  d3 const pD = mul3(R, pC);
  d3 const nD = mul3T(Ri, mul3T(rfc, ng));  // normals: transpose of the inverse
  double const dd = nD.z * pD.z;
  d3 const xd = normd(md3(ka->texMinDx[0], ka->texMinDx[1], 1.0 + double(ka->texMinDx[2])));
  d3 const yd = normd(md3(ka->texMinDy[0], ka->texMinDy[1], 1.0 + double(ka->texMinDy[2])));
  double const tx = -(0.0 - dd) / dotd(nD, xd), ty = -(0.0 - dd) / dotd(nD, yd);  // the origin differentials are 0 (pinhole)
  double const sc = ka->texSppScale;
  d3 const dpdx = mul3(rfc, mul3(Ri, xd * tx - pD)) * sc, dpdy = mul3(rfc, mul3(Ri, yd * ty - pD)) * sc;
  if (!(lend(crossd(dpdx, dpdy)) >= 1e-6)) return r;  // core-render.cpp:264-268
  // dpdu / dpdv (core-render.cpp:209-226)
  TriPost const P = load_scene(k).post[tri];
  float const* const uv = ka->triUv + 6 * size_t(tri);
  d3 const p0 = md3(P.p0x, P.p0y, P.p0z), dp1 = md3(P.p1x, P.p1y, P.p1z) - p0, dp2 = md3(P.p2x, P.p2y, P.p2z) - p0;
  double const du1 = double(uv[2]) - uv[0], dv1 = double(uv[3]) - uv[1], du2 = double(uv[4]) - uv[0], dv2 = double(uv[5]) - uv[1];
  double const detUv = du1 * dv2 - dv1 * du2;
  if (detUv == 0.0) return r;  // [fix 5]
  double const invUv = 1.0 / detUv;
  d3 const dpdu = (dp1 * dv2 - dp2 * dv1) * invUv, dpdv = (dp2 * du1 - dp1 * du2) * invUv;
  // duv_From_dp_dxy (core-texture.cu:123-258, the #else branch)
  d3 rdpdy = dpdy;
  if (lend(dpdx - dpdy) < 1e-12 * fmax(1.0, lend(dpdx))) {
    d3 n = crossd(dpdu, dpdv);
    double nl = lend(n);
    if (nl < 1e-12) {
      n = crossd(dpdu, dpdx), nl = lend(n);
      if (nl < 1e-12) n = crossd(dpdv, dpdx), nl = lend(n);
    }
    if (nl < 1e-12) n = md3(0, 0, 1);
    rdpdy = dpdy + normd(n) * (1e-6 * fmax(1.0, lend(dpdx)));
  }
  double const a00 = dotd(dpdu, dpdu), a01 = dotd(dpdu, dpdv), a11 = dotd(dpdv, dpdv);
  double const b0x = dotd(dpdu, dpdx), b1x = dotd(dpdv, dpdx), b0y = dotd(dpdu, rdpdy), b1y = dotd(dpdv, rdpdy);
  double const det = a00 * a11 - a01 * a01;
  if (fabs(det) < 1e-8) return r;
  double dudx, dvdx, dudy, dvdy;
  if (!__builtin_isinf(det) && fabs(det) > 1e-12) {
    double const inv = 1.0 / det;
    dudx = (a11 * b0x - a01 * b1x) * inv, dvdx = (a00 * b1x - a01 * b0x) * inv;
    dudy = (a11 * b0y - a01 * b1y) * inv, dvdy = (a00 * b1y - a01 * b0y) * inv;
  } else {
    double const lambda = 1e-6 * fmax(1.0, fmax(a00, a11));
    double const r00 = a00 + lambda, r11 = a11 + lambda, r01 = a01;
    double const rdet = r00 * r11 - r01 * r01;
    if (!__builtin_isinf(rdet) && fabs(rdet) > 0.0) {
      double const inv = 1.0 / rdet;
      dudx = (r11 * b0x - r01 * b1x) * inv, dvdx = (r00 * b1x - r01 * b0x) * inv;
      dudy = (r11 * b0y - r01 * b1y) * inv, dvdy = (r00 * b1y - r01 * b0y) * inv;
    } else {  // geometric gradients
      d3 n = crossd(dpdu, dpdv);
      double nl = lend(n);
      if (nl < 1e-12) {
        n = crossd(dpdu, dpdx), nl = lend(n);
        if (nl < 1e-12) n = crossd(dpdv, dpdx), nl = lend(n);
      }
      n = nl < 1e-12 ? md3(0, 0, 1) : normd(n);
      d3 const gu = normd(crossd(n, dpdv)), gv = normd(crossd(dpdu, n));
      dudx = dotd(gu, dpdx), dvdx = dotd(gv, dpdx), dudy = dotd(gu, rdpdy), dvdy = dotd(gv, rdpdy);
    }
  }
  auto clampd = [](double v) { return __builtin_isinf(v) ? 0.f : float(fmin(fmax(v, -1e8), 1e8)); };
  r.dudx = clampd(dudx), r.dvdx = clampd(dvdx), r.dudy = clampd(dudy), r.dvdy = clampd(dvdy);
  return r;
}
// metallic fraction of a BS_GGX_BLEND material at the hit: the record's constant, or the material's 1-channel metallic map
// (core-material.cpp:209-216), whose index sits in the first texture slot of the pair's SECOND row
template <bool FILT = false>
DMT_DEV float blend_metallic(KArgs k, Rec32 const& rec, uint32_t matId, int tri, float bu, float bv, TexDiff const& td = TexDiff{}) {
  KArgs const ka = kargs(k);
  float m = h2f(lo16(rec.w[0]));
  if (ka->matTex != nullptr) {
    int32_t const texM = int32_t(ka->matTex[4 * (matId + 1u)]);
    if (texM >= 0) {
      float const* const uv = ka->triUv + 6 * size_t(tri);
      float const w0 = 1.f - bu - bv;
      m = tex_lookup<FILT>(k, texM, w0 * uv[0] + bu * uv[2] + bv * uv[4], w0 * uv[1] + bu * uv[3] + bv * uv[5], false, td).x;
    }
  }
  return m;
}
// patches `rec` from the material's textures at the hit and returns the shading normal (ng when there is no normal map)
template <bool FILT = false>
DMT_DEV f3 apply_material_textures(KArgs k, Rec32& rec, uint32_t matId, int tri, float bu, float bv, f3 ng, TexDiff const& td = TexDiff{}) {
  KArgs const ka = kargs(k);
  uint32_t const* const m = ka->matTex + 4 * matId;
  int32_t const texD = int32_t(m[0]), texR = int32_t(m[1]), texN = int32_t(m[2]);
  if (texD < 0 && texR < 0 && texN < 0) return ng;
  float const aniso = __uint_as_float(m[3]);
  float const* const uv = ka->triUv + 6 * size_t(tri);
  float const w0 = 1.f - bu - bv;
  float const s = w0 * uv[0] + bu * uv[2] + bv * uv[4], t = w0 * uv[1] + bu * uv[3] + bv * uv[5];
  uint32_t const type = hi16(rec.w[1]);
  if (texD >= 0 && type == BS_OREN) {
    f3 const c = tex_lookup<FILT>(k, texD, s, t, false, td);
    rec.w[0] = f2h(fmaxf(0.f, fminf(c.x, 1.f))) | (f2h(fmaxf(0.f, fminf(c.y, 1.f))) << 16);
    rec.w[1] = (rec.w[1] & 0xFFFF0000u) | f2h(fmaxf(0.f, fminf(c.z, 1.f)));
  }
  if (texR >= 0) {
    float const rough = fmaxf(0.f, fminf(tex_lookup<FILT>(k, texR, s, t, false, td).x, 1.f));
    if (type == BS_OREN) {  // makeOrenNayar, CC/private/bsdf.cu:817-844: terms derived from the STORED halves
      float const kk = (kPi / 2.f) - 2.f / 3.f;
      uint32_t const hr = f2h(fmaxf(0.f, fminf(rough, kPi / 2.f)));
      float const sigma = h2f(hr);
      uint32_t const ha = f2h(1.f / (kPi + kk * sigma));
      uint32_t const hb = f2h(h2f(ha) * sigma);
      rec.w[5] = hr | (ha << 16);
      rec.w[6] = (rec.w[6] & 0xFFFF0000u) | hb;
    } else if (type == BS_GGX_DIEL || type == BS_GGX_COND) {  // ggxCommon: alpha_y = roughness, alpha_x = anisotropy * roughness
      float const top = 65535.f;
      uint32_t const ax = uint32_t(fminf(fmaxf(aniso * rough * top, 0.f), top)), ay = uint32_t(fminf(fmaxf(rough * top, 0.f), top));
      rec.w[3] = (rec.w[3] & 0x0000FFFFu) | (ax << 16);
      rec.w[4] = (rec.w[4] & 0xFFFF0000u) | ay;
    }
  }
  if (texN < 0) return ng;
  f3 n = tex_lookup<FILT>(k, texN, s, t, true, td);
  auto quant = [](float v) { return float(int(v * 1023.f + 0.5f)) / 1023.f; };
  n = normalize(mk3(quant(n.x), quant(n.y), quant(n.z)));
  f3 tx, ty;
  gram_schmidt(ng, tx, ty);
  f3 const ns = tx * n.x + ty * n.y + ng * n.z;
  float const l2 = dot(ns, ns);
  return (l2 > 0.f && l2 < kInf) ? ns / sqrtf(l2) : ng;
}
