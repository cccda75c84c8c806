// =====================================================================================
// dmt_oracle.cpp -- CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE)
//
// A plain C++17 restatement, in IEEE fp32 on the host, of the reference's megakernel path
// tracer (alexoz12v2/cuda-optix-pathtracing, "dmt").  Only tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg may load this library; the shipped HIP path never does.
//
// Every function cites the reference file:line it follows (paths relative to
// /root/reference/examples/triangles/, abbreviated  T/ = examples/triangles/,
// CC/ = examples/triangles/cuda-core/).  Where the reference has a host branch and a device
// branch (#ifdef __CUDA_ARCH__), the HOST branch is followed: software fp16, software table
// lookup with (size-1) scaling, 1/sqrtf for rsqrtf, IEEE division for __frcp_rn.
//
// Parity pinning (see DESIGN.md "Oracle"): the reference cannot be compiled in this container
// without stand-in CUDA headers, so it is NOT built; the oracle is pinned by
//   (1) the reference's own known-answer test T/tests/triangle_intersect.cu:12-68,164-186
//       (device routine == host Moeller-Trumbore on its 65,536 generated triangles, rays A/B),
//   (2) the sanity anchors the survey stage recorded from the reference sources executed on
//       CPU: computeParams(512,512), Halton index of pixel (17,42) s=3,
//       film means of the 64x64x4spp and 128x128x16spp Cornell renders,
//   (3) the authors' published figure docs/notes.txt:36-37 (mean of the 8-bit standard-error image of the
//       256x256, 2048-spp CUDA render = 0.018148823657): reproduced to 2e-5 relative with left-to-right
//       argument evaluation (tests/golden/reference_pins.json).
// Anything not covered by those (per-function BSDF / light values) is "parity unpinned" beyond
// the end-to-end film anchors.  The later sections restate code that has NO reference-side vector at all and
// are parity unpinned: the CPU renderer's env-map light (A18, core-light.cpp / core-math.cu) and emissive
// triangles (pbrt-v4 semantics; the reference has no implementation).
//
// Unspecified-behaviour note: T/megakernel/megakernel.cu:247-249 passes get2D() and get1D() as
// two arguments of one call; C++ leaves their evaluation order unspecified.  `rtl_args` selects
// right-to-left (what g++ does, hence what produced the survey anchors); the default is
// left-to-right (clang / nvcc front ends), which is what the HIP kernel implements.
// =====================================================================================
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../include/dmt_ggx_tables.inc"

namespace {

// ------------------------------------------------------------------------------------
// small vector algebra -- expression order follows CC/public/cuda-core/common_math.cuh:261-476
// ------------------------------------------------------------------------------------
struct V2 {
  float x = 0.f, y = 0.f;
};
struct V3 {
  float x = 0.f, y = 0.f, z = 0.f;
};
struct V4 {
  float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
};

inline V3 v3(float x, float y, float z) { return V3{x, y, z}; }
inline V2 v2(float x, float y) { return V2{x, y}; }

inline V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
inline V3 operator*(V3 a, V3 b) { return v3(b.x * a.x, b.y * a.y, b.z * a.z); }  // :354
inline V3 operator*(V3 v, float a) { return v3(v.x * a, v.y * a, v.z * a); }
inline V3 operator*(float a, V3 v) { return v3(v.x * a, v.y * a, v.z * a); }
inline V3 operator/(V3 v, float a) { return v3(v.x / a, v.y / a, v.z / a); }
inline V3 operator/(V3 v, V3 a) { return v3(v.x / a.x, v.y / a.y, v.z / a.z); }
inline V3 operator+(float b, V3 a) { return v3(a.x + b, a.y + b, a.z + b); }
inline V3 operator+(V3 a, float b) { return v3(a.x + b, a.y + b, a.z + b); }
inline V3 operator-(V3 a, float b) { return v3(a.x - b, a.y - b, a.z - b); }
inline V3 operator-(float a, V3 b) { return v3(a - b.x, a - b.y, a - b.z); }
inline V3& operator+=(V3& a, V3 b) { return a = a + b; }
inline V3& operator*=(V3& a, V3 b) {
  a.x *= b.x, a.y *= b.y, a.z *= b.z;
  return a;
}
inline V3& operator*=(V3& a, float b) {
  a.x *= b, a.y *= b, a.z *= b;
  return a;
}
inline V3& operator/=(V3& a, float b) {
  a.x /= b, a.y /= b, a.z /= b;
  return a;
}
inline V3& operator/=(V3& a, V3 b) {
  a.x /= b.x, a.y /= b.y, a.z /= b.z;
  return a;
}
inline V2 operator+(V2 a, V2 b) { return v2(a.x + b.x, a.y + b.y); }
inline V2 operator-(V2 a, V2 b) { return v2(a.x - b.x, a.y - b.y); }

inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float dot(V2 a, V2 b) { return a.x * b.x + a.y * b.y; }
inline float length2(V3 a) { return dot(a, a); }
inline float length2(V2 a) { return dot(a, a); }
inline float length(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
inline V3 cross(V3 a, V3 b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// host rsqrtf(x) of the CUDA headers is 1/sqrt(x)                      common_math.cuh:297-300
inline float rsqrt_host(float x) { return 1.0f / sqrtf(x); }
inline V3 normalize(V3 a) {
  float const inv = rsqrt_host(a.x * a.x + a.y * a.y + a.z * a.z);
  return v3(a.x * inv, a.y * inv, a.z * inv);
}
inline V3 absv(V3 a) { return v3(fabsf(a.x), fabsf(a.y), fabsf(a.z)); }
inline V3 sqrtv(V3 a) { return v3(sqrtf(a.x), sqrtf(a.y), sqrtf(a.z)); }
inline float sqrf(float f) { return f * f; }
inline float safeSqrt(float a) { return sqrtf(fmaxf(a, 0.f)); }
inline float maxComponent(V3 v) { return fmaxf(v.x, fmaxf(v.y, v.z)); }
inline bool isZero(V3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }
inline bool nearZeroPos(V3 v, float tol) { return v.x < tol && v.y < tol && v.z < tol; }
inline float luminance(V3 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
inline float average(V3 a) { return (a.x + a.y + a.z) / 3.f; }
inline float lerpf(float a, float b, float t) {  // common_math.cuh:301-305
  float const omt = 1.f - t;
  return omt * a + t * b;
}
inline V3 lerp3(V3 a, V3 b, float t) {  // :416-420
  float const omt = 1.f - t;
  return omt * a + t * b;
}
inline float safeacos(float v) { return acosf(fminf(fmaxf(v, -1.f), 1.f)); }
inline float sin_from_cos(float c) { return safeSqrt(1.f - sqrf(c)); }
inline float sin_sqr_to_one_minus_cos(float s_sq) {  // :439-443
  return s_sq > 0.0004f ? 1.0f - safeSqrt(1.0f - s_sq) : 0.5f * s_sq;
}
// smoothstep(a,b,x): the clamp is written fmaxf(fminf(.,0),1), so t is always 1 -> returns 1
// (common_math.cuh:478-489); restated literally.
inline float smoothstep1(float x) {
  if (x <= 0.f) return 0.f;
  if (x >= 1.f) return 1.f;
  float const x2 = x * x;
  return 3.f * x2 - 2.f * x2 * x;
}
inline float smoothstep3(float a, float b, float x) {
  float const t = fmaxf(fminf((x - a) / (b - a), 0.f), 1.f);
  return smoothstep1(t);
}
inline void gramSchmidt(V3 n, V3* a, V3* b) {  // :453-465
  if (fabsf(n.x - n.y) > 1e-3f || fabsf(n.x - n.z) > 1e-3f)
    *a = v3(n.z - n.y, n.x - n.z, n.y - n.x);
  else
    *a = v3(n.z - n.y, n.x + n.z, -n.y - n.x);
  *a = normalize(*a);
  *b = cross(n, *a);
}
inline void orthonormalTangent(V3 n, V3 t, V3* a, V3* b) {  // :466-472
  *b = normalize(cross(n, t));
  *a = cross(*b, n);
}

constexpr float kPi = 3.14159265358979323846f;      // std::numbers::pi_v<float>
constexpr float kInvPi = 0.318309886183790671538f;  // std::numbers::inv_pi_v<float>

// ------------------------------------------------------------------------------------
// fp16 <-> fp32, software (host branch)                         CC/private/encoding.cu:65-157
// ------------------------------------------------------------------------------------
uint16_t f2h(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  uint32_t const sign = (u >> 16) & 0x8000u;
  int32_t exp = int32_t((u >> 23) & 0xFFu) - 127 + 15;
  uint32_t mant = u & 0x007FFFFFu;
  if (exp >= 31) return uint16_t(sign | 0x7C00u | (mant ? 0x200u : 0u));
  if (exp <= 0) {
    if (exp < -10) return uint16_t(sign);
    mant |= 0x00800000u;
    uint32_t const shift = uint32_t(14 - exp);
    uint32_t const rounded = (mant >> shift) + ((mant >> (shift - 1)) & 1u);
    return uint16_t(sign | uint16_t(rounded));
  }
  uint32_t rounded = mant + 0x00001000u;
  if (rounded & 0x00800000u) {
    rounded = 0;
    exp += 1;
    if (exp >= 31) return uint16_t(sign | 0x7C00u);
  }
  return uint16_t(sign | uint16_t(exp << 10) | uint16_t(rounded >> 13));
}
float h2f(uint16_t h) {
  uint32_t const sign = uint32_t(h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 0x1Fu;
  uint32_t mant = h & 0x03FFu;
  uint32_t out;
  if (exp == 0) {
    if (mant == 0) {
      out = sign;
    } else {
      exp = 127 - 15 + 1;
      while ((mant & 0x0400u) == 0) {
        mant <<= 1;
        exp--;
      }
      mant &= 0x03FFu;
      out = sign | (exp << 23) | (mant << 13);
    }
  } else if (exp == 31) {
    out = sign | 0x7F800000u | (mant << 13);
  } else {
    out = sign | ((exp + 127 - 15) << 23) | (mant << 13);
  }
  float f;
  memcpy(&f, &out, 4);
  return f;
}

// ------------------------------------------------------------------------------------
// octahedral direction codec                                     CC/private/encoding.cu:12-60
// (the encoder clamps to [0,1] BEFORE rounding, so each 16-bit component is 0 or 1 -- restated)
// ------------------------------------------------------------------------------------
inline float signf(float f) {
  bool const b = std::signbit(f);
  return b * -1.f + !b * 1.f;
}
inline uint32_t encodeOctaComponent(float f) {
  float const mx = 65535.f;
  return uint32_t(roundf(fmaxf(fminf((f + 1) * 0.5f * mx, 1.f), 0.f)));
}
uint32_t octaFromDir(V3 dir) {
  V3 const p = dir / (fabsf(dir.x) + fabsf(dir.y) + fabsf(dir.z));
  float x = p.x, y = p.y, z = p.z;
  bool const flip = z < 0.f;
  x = flip * (1.f - fabsf(y)) * signf(x) + !flip * x;
  y = flip * (1.f - fabsf(x)) * signf(y) + !flip * y;
  return encodeOctaComponent(y) << 16 | encodeOctaComponent(x);
}
V3 dirFromOcta(uint32_t octa) {
  float const mx = 65535.f;
  uint32_t const ox = octa & 0xFFFFu;
  uint32_t const oy = (octa >> 16) & 0xFFFFu;
  V2 const f = v2(float(ox) / mx * 2.f - 1.f, float(oy) / mx * 2.f - 1.f);
  V3 n = v3(f.x, f.y, 1.f - fabsf(f.x) - fabsf(f.y));
  float const nx = n.x, ny = n.y;
  bool const flip = n.z < 0.f;
  n.x = flip * (1.f - fabsf(ny)) * signf(nx) + !flip * nx;
  n.y = flip * (1.f - fabsf(nx)) * signf(ny) + !flip * ny;
  return normalize(n);
}

// ------------------------------------------------------------------------------------
// packed 32-byte records, byte-identical to CC/public/cuda-core/bsdf.cuh:18-73 and
// CC/public/cuda-core/light.cuh:10-49 (field offsets spelled out; accessed by memcpy)
// ------------------------------------------------------------------------------------
struct Rec32 {
  unsigned char b[32];
};
static_assert(sizeof(Rec32) == 32, "record size");
inline uint16_t rd16(Rec32 const& r, int off) {
  uint16_t v;
  memcpy(&v, r.b + off, 2);
  return v;
}
inline void wr16(Rec32& r, int off, uint16_t v) { memcpy(r.b + off, &v, 2); }
inline uint32_t rd32(Rec32 const& r, int off) {
  uint32_t v;
  memcpy(&v, r.b + off, 4);
  return v;
}
inline void wr32(Rec32& r, int off, uint32_t v) { memcpy(r.b + off, &v, 4); }
inline float rdf(Rec32 const& r, int off) {
  float v;
  memcpy(&v, r.b + off, 4);
  return v;
}
inline void wrf(Rec32& r, int off, float v) { memcpy(r.b + off, &v, 4); }
inline V3 rdh3(Rec32 const& r, int off) {
  return v3(h2f(rd16(r, off)), h2f(rd16(r, off + 2)), h2f(rd16(r, off + 4)));
}
inline void wrh3(Rec32& r, int off, V3 v) {
  wr16(r, off, f2h(v.x));
  wr16(r, off + 2, f2h(v.y));
  wr16(r, off + 4, f2h(v.z));
}
inline V3 rdf3(Rec32 const& r, int off) { return v3(rdf(r, off), rdf(r, off + 4), rdf(r, off + 8)); }
inline void wrf3(Rec32& r, int off, V3 v) {
  wrf(r, off, v.x);
  wrf(r, off + 4, v.y);
  wrf(r, off + 8, v.z);
}

// BSDF offsets
enum : int {
  B_WEIGHT = 0,   // 3 x fp16
  B_TYPE = 6,     // u16
  ON_ALBEDO = 8,  // 3 x fp16 (never written by the reference)
  ON_MS = 14,     // 3 x fp16 multiScatter
  ON_ROUGH = 20,  // fp16
  ON_A = 22,      // fp16
  ON_B = 24,      // fp16
  G_ESCALE = 8,   // f32
  G_PHI0 = 12,    // u16
  G_AX = 14,      // u16
  G_AY = 16,      // u16
  GD_ETA = 18,    // fp16
  GD_RT = 20,     // 3 x fp16
  GD_TT = 26,     // 3 x fp16
  GC_ETA = 18,    // 3 x fp16
  GC_K = 24,      // 3 x fp16
};
enum : uint16_t { BS_OREN = 0, BS_GGX_DIEL = 1, BS_GGX_COND = 2, BS_LAMBERT = 3,
                  // This build's own tag (the megakernel's packed format has no such record): a GGX dielectric record whose
                  // material is "metallic" by a fraction.  The record that FOLLOWS it in the array is the material's GGX
                  // conductor, and the first half of the (otherwise unused) weight field holds the metallic fraction as fp16.
                  // Semantics: the reference CPU renderer's blend, core-material.cpp:275-286 (sample) and :383-394 (eval).
                  BS_GGX_BLEND = 4 };
// Light offsets
enum : int {
  L_INT = 0,     // 3 x fp16
  L_TYPE = 6,    // u16
  LP_POS = 8,    // 3 x f32
  LP_RAD = 20,   // fp16
  LS_POS = 8,    // 3 x f32
  LS_DIR = 20,   // u32 octa
  LS_COS0 = 24,  // fp16
  LS_COSE = 26,  // fp16
  LS_RAD = 28,   // fp16
  LD_DIR = 8,    // u32 octa
  LD_OMC = 12,   // fp16
};
enum : uint16_t { LT_POINT = 0, LT_SPOT = 1, LT_ENV = 2, LT_DIR = 3 };

inline V3 bsdfWeight(Rec32 const& b) { return rdh3(b, B_WEIGHT); }
inline void bsdfSetWeight(Rec32& b, V3 w) { wrh3(b, B_WEIGHT, w); }
inline uint16_t bsdfType(Rec32 const& b) { return rd16(b, B_TYPE); }

// ------------------------------------------------------------------------------------
// makers                    CC/private/bsdf.cu:428-450,669-717,817-844; CC/private/light.cu:258-307
// ------------------------------------------------------------------------------------
void bsdfInit(Rec32& b, uint16_t type, V3 albedo) {
  wrh3(b, B_WEIGHT, albedo);
  wr16(b, B_TYPE, type);
}
void bsdfGGXCommon(Rec32& b, float ax, float ay, float phi0) {
  float const U16 = 65535.f;
  wr16(b, G_AX, uint16_t(fminf(fmaxf(ax * U16, 0.f), U16)));
  wr16(b, G_AY, uint16_t(fminf(fmaxf(ay * U16, 0.f), U16)));
  wrf(b, G_ESCALE, 1.f);
  wr16(b, G_PHI0, uint16_t(fminf(fmaxf(phi0 / (2.f * kPi) * U16, 0.f), U16)));
}
Rec32 makeLambert() {
  Rec32 b{};
  bsdfInit(b, BS_LAMBERT, v3(1, 1, 1));
  return b;
}
Rec32 makeOrenNayar(V3 color, float roughness) {
  float const piOver2Minus2Over3 = (kPi / 2.f) - 2.f / 3.f;
  V3 const albedo = v3(fmaxf(0, fminf(color.x, 1)), fmaxf(0, fminf(color.y, 1)),
                       fmaxf(0, fminf(color.z, 1)));
  Rec32 b{};
  bsdfInit(b, BS_OREN, albedo);
  wr16(b, ON_ROUGH, f2h(fmaxf(0, fminf(roughness, kPi / 2.f))));
  float const sigma = h2f(rd16(b, ON_ROUGH));
  wr16(b, ON_A, f2h(1.f / (kPi + piOver2Minus2Over3 * sigma)));
  float const a = h2f(rd16(b, ON_A));
  wr16(b, ON_B, f2h(a * sigma));
  wrh3(b, ON_MS, v3(1.f, 1.f, 1.f));
  return b;
}
Rec32 makeGGXDielectric(V3 rTint, V3 tTint, float phi0, float eta, float ax, float ay) {
  Rec32 b{};
  bsdfInit(b, BS_GGX_DIEL, v3(1, 1, 1));
  bsdfGGXCommon(b, ax, ay, phi0);
  wr16(b, GD_ETA, f2h(eta));
  wrh3(b, GD_RT, rTint);
  wrh3(b, GD_TT, tTint);
  return b;
}
Rec32 makeGGXConductor(V3 eta, V3 kappa, float phi0, float ax, float ay) {
  Rec32 b{};
  bsdfInit(b, BS_GGX_COND, v3(1, 1, 1));
  bsdfGGXCommon(b, ax, ay, phi0);
  wrh3(b, GC_ETA, eta);
  wrh3(b, GC_K, kappa);
  return b;
}
void packIntensity(Rec32& l, V3 color, uint16_t type) {
  wrh3(l, L_INT, color);
  wr16(l, L_TYPE, type);
}
Rec32 makePointLight(V3 color, V3 pos, float radius) {
  Rec32 l{};
  packIntensity(l, color, LT_POINT);
  wrf3(l, LP_POS, pos);
  wr16(l, LP_RAD, f2h(radius));
  return l;
}
Rec32 makeSpotLight(V3 color, V3 pos, V3 dir, float cos0, float cosE, float radius) {
  Rec32 l{};
  packIntensity(l, color, LT_SPOT);
  wrf3(l, LS_POS, pos);
  wr32(l, LS_DIR, octaFromDir(dir));
  wr16(l, LS_COS0, f2h(cos0));
  wr16(l, LS_COSE, f2h(cosE));
  wr16(l, LS_RAD, f2h(radius));
  return l;
}
Rec32 makeDirectionalLight(V3 color, V3 dir, float oneMinusCos) {
  Rec32 l{};
  packIntensity(l, color, LT_DIR);
  wr32(l, LD_DIR, octaFromDir(dir));
  wr16(l, LD_OMC, f2h(oneMinusCos));
  return l;
}
Rec32 makeEnvLight(V3 color) {
  Rec32 l{};
  packIntensity(l, color, LT_ENV);
  return l;
}

// ------------------------------------------------------------------------------------
// Transform (column-major 4x4 + cofactor inverse)   CC/private/common_math.cu:16-130
// ------------------------------------------------------------------------------------
struct Xform {
  float m[16];
  float mi[16];
};
Xform makeXform(float const* src) {
  Xform t;
  float* m = t.m;
  float* inv = t.mi;
  for (int i = 0; i < 16; ++i) m[i] = src[i];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] +
           m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] -
           m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] +
           m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] -
            m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] -
           m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] +
           m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] -
           m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] +
            m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] +
           m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] -
           m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] +
            m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] -
            m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] -
           m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] +
           m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] -
            m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] +
            m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  float const det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  float const invDet = 1.0f / det;
  for (int i = 0; i < 16; ++i) inv[i] *= invDet;
  return t;
}
V3 xformDir(Xform const& t, V3 v) {
  float const* m = t.m;
  return v3(m[0] * v.x + m[4] * v.y + m[8] * v.z, m[1] * v.x + m[5] * v.y + m[9] * v.z,
            m[2] * v.x + m[6] * v.y + m[10] * v.z);
}
V3 xformPoint(Xform const& t, V3 p) {
  float const* m = t.m;
  float x = m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12];
  float y = m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13];
  float z = m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14];
  float const w = m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15];
  if (w != 1.0f && w != 0.0f) {
    float const iw = 1.0f / w;
    x *= iw, y *= iw, z *= iw;
  }
  return v3(x, y, z);
}
// CC/private/extra_math.cu:43-58
Xform worldFromCamera(V3 camDir, V3 camPos) {
  V3 const fwd = normalize(camDir);
  V3 const right = normalize(cross(fwd, v3(0, 0, 1)));
  V3 const up = cross(right, fwd);
  float m[16];
  m[0] = right.x, m[4] = up.x, m[8] = fwd.x, m[12] = camPos.x;
  m[1] = right.y, m[5] = up.y, m[9] = fwd.y, m[13] = camPos.y;
  m[2] = right.z, m[6] = up.z, m[10] = fwd.z, m[14] = camPos.z;
  m[3] = 0.f, m[7] = 0.f, m[11] = 0.f, m[15] = 1.f;
  return makeXform(m);
}
// CC/private/extra_math.cu:60-90
Xform cameraFromRasterPerspective(float focal_mm, float sensorH_mm, uint32_t xRes,
                                  uint32_t yRes) {
  float const sensorW_mm = sensorH_mm * float(xRes) / float(yRes);
  float const MM = 0.001f;
  float const focal = focal_mm * MM;
  float const sh = sensorH_mm * MM;
  float const sw = sensorW_mm * MM;
  float const psx = sw / float(xRes);
  float const psy = sh / float(yRes);
  float const tx = -0.5f * sw + 0.5f * psx;
  float const ty = 0.5f * sh - 0.5f * psy;
  float const tz = focal;
  float m[16];
  m[0] = psx, m[4] = 0.f, m[8] = 0.f, m[12] = tx;
  m[1] = 0.f, m[5] = -psy, m[9] = 0.f, m[13] = ty;
  m[2] = 0.f, m[6] = 0.f, m[10] = 1.f, m[14] = tz;
  m[3] = 0.f, m[7] = 0.f, m[11] = 0.f, m[15] = 1.f;
  return makeXform(m);
}

// ------------------------------------------------------------------------------------
// Halton-Owen sampler                     CC/private/rng.cu:11-262, CC/public/cuda-core/rng.cuh
// ------------------------------------------------------------------------------------
constexpr int kNumPrimes = 10;
constexpr int kPrimes[kNumPrimes] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29};
constexpr int kMaxRes = 128;

struct HaltonParams {
  int32_t baseScales[2];
  int32_t baseExponents[2];
  int32_t multInvs[2];
};
int64_t multiplicativeInverse(int64_t a, int64_t n) {  // rng.cu:21-46
  int64_t t = 0, newt = 1, r = n, newr = a;
  while (newr != 0) {
    int64_t const q = r / newr;
    int64_t tmp = t - q * newt;
    t = newt, newt = tmp;
    tmp = r - q * newr;
    r = newr, newr = tmp;
  }
  if (t < 0) t += n;
  return t;
}
HaltonParams computeParams(int width, int height) {  // rng.cu:182-208
  HaltonParams p{};
  int const res[2] = {width, height};
  for (int i = 0; i < 2; ++i) {
    int32_t const base = kPrimes[i];
    p.baseScales[i] = 1;
    p.baseExponents[i] = 0;
    while (p.baseScales[i] < (res[i] < kMaxRes ? res[i] : kMaxRes)) {
      p.baseScales[i] *= base;
      ++p.baseExponents[i];
    }
  }
  p.multInvs[0] = int32_t(multiplicativeInverse(p.baseScales[1], p.baseScales[0]));
  p.multInvs[1] = int32_t(multiplicativeInverse(p.baseScales[0], p.baseScales[1]));
  return p;
}
inline int32_t inverseRadicalInverse(int32_t inverse, int32_t base, int32_t nDigits) {  // :48-59
  int32_t index = 0;
  for (int32_t i = 0; i < nDigits; ++i) {
    int32_t const digit = inverse % base;
    inverse /= base;
    index *= base;
    index += digit;
  }
  return index;
}
inline uint32_t mixBits32(uint32_t v) {  // :61-68
  v ^= v >> 16;
  v *= 0x7feb352dU;
  v ^= v >> 15;
  v *= 0x846ca68bU;
  v ^= v >> 16;
  return v;
}
inline float radicalInverse(uint32_t primeIndex, uint32_t index) {  // :70-94
  uint32_t const base = uint32_t(kPrimes[primeIndex]);
  float const invBase = 1.0f / float(base);  // __frcp_rn(__uint2float_rn(base))
  float result = 0.0f;
  float invBasePow = invBase;
  while (index > 0) {
    uint32_t const next = index / base;
    uint32_t const digit = index - next * base;
    result = fmaf(float(digit), invBasePow, result);
    invBasePow *= invBase;
    index = next;
  }
  return fminf(result, 0.99999994f);
}
// digit "permutation" = (digit + hash) % base, with 32-bit wraparound        :96-135
inline float owenScrambledRadicalInverse32(int primeIndex, uint32_t index, uint32_t seed) {
  uint32_t const base = uint32_t(kPrimes[primeIndex]);
  float const invBase = 1.0f / float(base);
  float result = 0.0f;
  float invBasePow = invBase;
  uint32_t revHash = 0;
  while (index > 0) {
    uint32_t const next = index / base;
    uint32_t const digit = index - next * base;
    uint32_t const scramble = mixBits32(seed ^ revHash);
    uint32_t const permuted = (digit + scramble) % base;
    result = fmaf(float(permuted), invBasePow, result);
    revHash = revHash * base + digit;
    invBasePow *= invBase;
    index = next;
  }
  return fminf(result, 0.99999994f);
}
inline float sampleDim(int dimension, int haltonIndex) {  // :175-178
  uint32_t const seed = mixBits32(1u + (uint32_t(dimension) << 4));
  return owenScrambledRadicalInverse32(dimension, uint32_t(haltonIndex), seed);
}
struct Sampler {  // one lane of DeviceHaltonOwen (rng.cuh:14-27)
  int haltonIndex = 0;
  int dimension = 0;
  void startPixelSample(HaltonParams const& p, int px, int py, int32_t sampleIndex,
                        int32_t dim = 0) {  // rng.cu:210-231
    int const stride = p.baseScales[0] * p.baseScales[1];
    haltonIndex = 0;
    int const pm[2] = {px % kMaxRes, py % kMaxRes};
    for (int i = 0; i < 2; ++i) {
      int32_t const dimOffset = inverseRadicalInverse(pm[i], kPrimes[i], p.baseExponents[i]);
      haltonIndex += dimOffset * (stride / p.baseScales[i]) * p.multInvs[i];
    }
    haltonIndex %= stride;
    haltonIndex += sampleIndex * stride;
    dimension = dim > 2 ? dim : 2;
  }
  float get1D() {  // :233-240
    if (dimension >= kNumPrimes) dimension = 2;
    int const dim = dimension++;
    return sampleDim(dim, haltonIndex);
  }
  V2 get2D() {  // :242-252
    if (dimension + 1 >= kNumPrimes) dimension = 2;
    int const dim = dimension;
    dimension += 2;
    return v2(sampleDim(dim, haltonIndex), sampleDim(dim + 1, haltonIndex));
  }
  V2 getPixel2D(HaltonParams const& p) const {  // :254-262
    return v2(radicalInverse(0, uint32_t(haltonIndex >> p.baseExponents[0])),
              radicalInverse(1, uint32_t(haltonIndex / p.baseScales[1])));
  }
};

// ------------------------------------------------------------------------------------
// camera                                                       CC/private/extra_math.cu:7-42
// ------------------------------------------------------------------------------------
struct Ray {
  V3 o, d;
};
inline V2 cameraSampleFilm(int px, int py, Sampler const& rng, HaltonParams const& p) {
  V2 const shift = rng.getPixel2D(p) - v2(0.5f, 0.5f);
  return shift + v2(0.5f, 0.5f) + v2(float(px), float(py));
}
inline Ray cameraRay(V2 pFilm, Xform const& cameraFromRaster, Xform const& renderFromCamera) {
  Ray r;
  V3 const pCamera = xformPoint(cameraFromRaster, v3(pFilm.x, pFilm.y, 0.0f));
  r.o = xformPoint(renderFromCamera, v3(0.f, 0.f, 0.f));
  r.d = normalize(xformDir(renderFromCamera, pCamera));
  return r;
}

// ------------------------------------------------------------------------------------
// triangle intersection                      CC/private/shapes.cu:5-57 (device routine) and
// :59-109 (host Moeller-Trumbore used by the reference's own test as expected value)
// ------------------------------------------------------------------------------------
struct Hit {
  V3 pos, normal, error;
  int32_t hit = 0;
  uint32_t matId = 0;
  float t = std::numeric_limits<float>::infinity();
  float u = 0.f, v = 0.f;  // barycentric weights of p1, p2 (texture coordinates of textured materials)
};
inline float gammaf(int n) {  // extra_math.cuh:21-29
  float const f = float(n) * std::numeric_limits<float>::epsilon() * 0.5f;
  return f / (1 - f);
}
inline V3 triError(float u, float v, V3 p0, V3 p1, V3 p2) {  // extra_math.cuh:31-34
  return gammaf(7) * (absv(u * p0) + absv(v * p1) + absv((1 - u - v) * p2));
}
constexpr float kMTTol = 1e-7f;
// x = {x0,x1,x2,pad}, y, z: one float4 per axis per triangle (types.cuh:119-129)
Hit triangleIntersect(float const* x, float const* y, float const* z, Ray ray) {
  Hit r;
  V3 const e0 = v3(x[1] - x[0], y[1] - y[0], z[1] - z[0]);
  V3 const e1 = v3(x[2] - x[0], y[2] - y[0], z[2] - z[0]);
  V3 const dxe1 = v3(ray.d.y * e1.z - ray.d.z * e1.y, ray.d.z * e1.x - ray.d.x * e1.z,
                     ray.d.x * e1.y - ray.d.y * e1.x);
  float const det = dxe1.x * e0.x + dxe1.y * e0.y + dxe1.z * e0.z;
  if (fabsf(det) < kMTTol) return r;
  float const invDet = 1.0f / det;
  V3 const ov = v3(ray.o.x - x[0], ray.o.y - y[0], ray.o.z - z[0]);
  V3 const txe0 = v3(ov.y * e0.z - ov.z * e0.y, ov.z * e0.x - ov.x * e0.z,
                     ov.x * e0.y - ov.y * e0.x);
  float const u = invDet * (dxe1.x * ov.x + dxe1.y * ov.y + dxe1.z * ov.z);
  float const v = invDet * (txe0.x * ray.d.x + txe0.y * ray.d.y + txe0.z * ray.d.z);
  float const t = invDet * (txe0.x * e1.x + txe0.y * e1.y + txe0.z * e1.z);
  bool const valid = (u >= -kMTTol && v >= -kMTTol && (u + v) <= 1 + kMTTol) && (t > 1e-4f);
  if (valid) {
    V3 const p0 = v3(x[0], y[0], z[0]);
    V3 const p1 = v3(x[1], y[1], z[1]);
    V3 const p2 = v3(x[2], y[2], z[2]);
    r.hit = 1;
    r.t = t;
    r.u = u, r.v = v;
    r.pos = p0 + u * e0 + v * e1;
    r.normal = normalize(cross(e1, e0));
    r.error = triError(u, v, p0, p1, p2);
  }
  return r;
}
Hit hostIntersectMT(V3 o, V3 d, V3 p0, V3 p1, V3 p2) {
  float const EPS = 1e-7f;
  Hit h;
  V3 const e0 = v3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z);
  V3 const e1 = v3(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
  V3 const p = v3(d.y * e1.z - d.z * e1.y, d.z * e1.x - d.x * e1.z, d.x * e1.y - d.y * e1.x);
  float const det = p.x * e0.x + p.y * e0.y + p.z * e0.z;
  if (fabs(det) < EPS) return h;
  float const invDet = 1.0f / det;
  V3 const t = v3(o.x - p0.x, o.y - p0.y, o.z - p0.z);
  float const u = invDet * (p.x * t.x + p.y * t.y + p.z * t.z);
  if (u < -EPS || u > 1 + EPS) return h;
  V3 const q = v3(t.y * e0.z - t.z * e0.y, t.z * e0.x - t.x * e0.z, t.x * e0.y - t.y * e0.x);
  float const v = invDet * (q.x * d.x + q.y * d.y + q.z * d.z);
  if (v < -EPS || u + v > 1 + EPS) return h;
  float const tHit = invDet * (q.x * e1.x + q.y * e1.y + q.z * e1.z);
  if (tHit > EPS) {
    h.hit = 1;
    h.t = tHit;
    h.pos = p0 + u * e0 + v * e1;
    h.normal = cross(e1, e0);
    h.error = triError(u, v, p0, p1, p2);
  }
  return h;
}
// extra_math.cuh:36-59
V3 offsetRayOrigin(V3 p, V3 error, V3 ng, V3 w) {
  float const inf = std::numeric_limits<float>::infinity();
  float const d = dot(absv(ng), error);
  V3 offset = ng * d;
  if (dot(w, ng) < 0.f) offset = -offset;
  V3 po = p + offset;
  po.x = nextafterf(po.x, offset.x > 0 ? inf : -inf);
  po.y = nextafterf(po.y, offset.y > 0 ? inf : -inf);
  po.z = nextafterf(po.z, offset.z > 0 ? inf : -inf);
  return po;
}

// ------------------------------------------------------------------------------------
// sampling helpers                                              CC/private/sampling.cu:51-187
// ------------------------------------------------------------------------------------
V2 sampleUniformDisk(V2 u) {  // :135-155  (note the 3pi/4 branch -- restated as written)
  float const a = 2.f * u.x - 1.f;
  float const b = 2.f * u.y - 1.f;
  float phi = 0.f, rho = 0.f;
  if (a == 0.f && b == 0.f) return V2{};
  if (fabsf(a) > fabsf(b)) {
    float const piOver4 = kPi / 4;
    rho = a;
    phi = piOver4 * (b / a);
  } else {
    float const threePiOver4 = 3 * kPi / 4;
    rho = b;
    phi = threePiOver4 * (a / b);
  }
  return v2(rho * cosf(phi), rho * sinf(phi));
}
V3 sampleCosHemisphere(V3 n, V2 u, float* pdf) {  // :157-167
  V2 const r = sampleUniformDisk(u);
  float const cosTheta = safeSqrt(1.f - length2(r));
  V3 T, B;
  gramSchmidt(n, &T, &B);
  if (pdf) *pdf = cosTheta * kInvPi;
  return r.x * T + r.y * B + cosTheta * n;
}
V3 sampleUniformSphere(V2 rnd) {  // :123-133
  float const z = 1.0f - 2.0f * rnd.x;
  float const r = safeSqrt(1.f - z * z);
  float const phi = 2 * kPi * rnd.y;
  return v3(r * cosf(phi), r * sinf(phi), z);
}
// :86-121 -- `xy *= s` ASSIGNS s to both components (common_math.cuh:349-353), restated
V3 sampleUniformCone(V3 N, float oneMinusCos, V2 rnd, float* cosTheta, float* pdf, int* delta) {
  if (oneMinusCos > 0) {
    V2 xy = sampleUniformDisk(rnd);
    float const r2 = length2(xy);
    *cosTheta = 1.0f - r2 * oneMinusCos;
    float const s = safeSqrt(r2 * oneMinusCos * (2.0f - r2 * oneMinusCos));
    xy.x = s;
    xy.y = s;
    float const denom = fmaxf(oneMinusCos, 1e-8f);
    *pdf = 0.5f / (kPi * denom);
    V3 T{}, B{};
    gramSchmidt(N, &T, &B);
    return xy.x * T + xy.y * B + *cosTheta * N;
  }
  *delta = true;
  *cosTheta = 1.0f;
  *pdf = 1.0f;
  return N;
}
bool raySphereIntersect(V3 rayO, V3 rayD, float tMin, float tMax, V3 C, float radius, V3* ip,
                        float* it) {  // :51-84
  V3 const dv = C - rayO;
  float const r_sq = radius * radius;
  float const d_sq = dot(dv, dv);
  float const dcos = dot(dv, rayD);
  if (d_sq > r_sq && dcos < 0.0f) return false;
  float const dsin_sq = length2(dv - dcos * rayD);
  if (dsin_sq > r_sq) return false;
  float const t = dcos - copysignf(sqrtf(r_sq - dsin_sq), d_sq - r_sq);
  if (t > tMin && t < tMax) {
    *it = t;
    *ip = rayO + rayD * t;
    return true;
  }
  return false;
}

// ------------------------------------------------------------------------------------
// lights                                                          CC/private/light.cu:13-332
// ------------------------------------------------------------------------------------
struct LightSample {
  V3 pLight, direction;
  float pdf = 0.f;
  int32_t delta = 0;
  float distance = 0.f;
  float factor = 0.f;
  bool valid() const {  // light.cuh:65-67
    return direction.x != 0 && direction.y != 0 && direction.z != 0 && pdf != 0;
  }
};
LightSample samplePointLight(Rec32 const& L, V3 position, V2 u, bool hadTransmission, V3 normal) {
  LightSample s{};
  s.factor = 1.0f;
  float const radius = h2f(rd16(L, LP_RAD));
  float const radiusSqr = sqrf(radius);
  V3 const lpos = rdf3(L, LP_POS);
  V3 lightN = position - lpos;
  float const distSqr = dot(lightN, lightN);
  float const dist = sqrtf(distSqr);
  lightN /= dist;
  bool const effectivelyDelta = (radius / dist) < 1e-3f;
  float cosTheta = 0.f;
  if (distSqr > radiusSqr) {
    float const omc = sin_sqr_to_one_minus_cos(radiusSqr / distSqr);
    s.direction = sampleUniformCone(-lightN, omc, u, &cosTheta, &s.pdf, &s.delta);
    if (effectivelyDelta || s.delta) {
      s.pdf = 1;
      s.delta = true;
    }
  } else {
    if (hadTransmission) {
      s.direction = sampleUniformSphere(u);
      s.pdf = 0.25f * kInvPi;
    } else {
      s.direction = sampleCosHemisphere(normal, u, &s.pdf);
    }
    cosTheta = -dot(s.direction, lightN);
  }
  s.distance = dist * cosTheta -
               copysignf(safeSqrt(radiusSqr - distSqr + distSqr * cosTheta * cosTheta),
                         distSqr - radiusSqr);
  s.pLight = position + s.direction * s.distance;
  return s;
}
Ray spotLightToLocal(V3 lightPos, V3 lightDir, Ray g) {  // :82-108
  V3 const fwd = normalize(lightDir);
  V3 up = (fabsf(fwd.z) < 0.999f) ? v3(0.f, 0.f, 1.f) : v3(0.f, 1.f, 0.f);
  V3 const right = normalize(cross(up, fwd));
  up = cross(fwd, right);
  V3 const o = v3(g.o.x - lightPos.x, g.o.y - lightPos.y, g.o.z - lightPos.z);
  Ray l;
  l.o = v3(dot(o, right), dot(o, up), dot(o, fwd));
  l.d = v3(dot(g.d, right), dot(g.d, up), dot(g.d, fwd));
  return l;
}
LightSample sampleSpotLight(Rec32 const& L, V3 position, V2 u, bool hadTransmission, V3 normal) {
  LightSample s{};
  s.distance = FLT_MAX;
  float const radius = h2f(rd16(L, LS_RAD));
  float const cosThetaE = h2f(rd16(L, LS_COSE));
  float const cosTheta0 = h2f(rd16(L, LS_COS0));
  V3 const spotDir = normalize(dirFromOcta(rd32(L, LS_DIR)));
  V3 const lpos = rdf3(L, LS_POS);
  float const radiusSqr = radius * radius;
  V3 lightN = position - lpos;
  float const distSqr = dot(lightN, lightN);
  float const dist = sqrtf(distSqr);
  lightN /= dist;
  bool const effectivelyDelta = (radius / dist) < 1e-3f;
  bool outside = false;
  float cosTheta = 0.f;
  if (distSqr > radiusSqr) {
    float const omcSpread = 1.f - cosThetaE;
    float const omcHalf = sin_sqr_to_one_minus_cos(radiusSqr / distSqr);
    if (omcHalf < omcSpread) {
      s.direction = sampleUniformCone(-lightN, omcHalf, u, &cosTheta, &s.pdf, &s.delta);
    } else {
      s.direction = sampleUniformCone(-spotDir, omcSpread, u, &cosTheta, &s.pdf, &s.delta);
      if (!raySphereIntersect(position, s.direction, 0.f, FLT_MAX, lpos, radius, &s.pLight,
                              &s.distance)) {
        outside = true;
        s.pdf = 0;
      }
    }
  } else {
    if (hadTransmission) {
      s.direction = sampleUniformSphere(u);
      s.pdf = 0.25f * kInvPi;
    } else {
      s.direction = sampleCosHemisphere(normal, u, &s.pdf);
    }
    cosTheta = -dot(s.direction, lightN);
  }
  Ray const local = spotLightToLocal(lpos, spotDir, Ray{position, -s.direction});
  if (!outside) {
    s.factor = smoothstep3(cosThetaE, cosTheta0, local.d.z);  // light.cuh:77-81
    if (s.factor <= 0.f) outside = true;
  }
  if (!outside) {
    if (s.distance == FLT_MAX) {
      // light.cu:176-179: product (not difference) with the copysign term -- restated; the value
      // is overwritten by the re-projection below
      s.distance = dist * cosTheta *
                   copysignf(safeSqrt(radiusSqr - distSqr + distSqr * cosTheta * cosTheta),
                             distSqr - radiusSqr);
    }
    if (effectivelyDelta) {
      s.pdf = 1.f;
      s.delta = true;
    }
    s.pLight = position + s.direction * s.distance;
    V3 const ng = normalize(s.pLight - lpos);
    s.pLight = ng * radius + lpos;
    V3 const newDir = s.pLight - position;
    float const distance = length(newDir);
    s.direction = newDir / distance;
    s.distance = distance;
  }
  return s;
}
LightSample sampleLight(Rec32 const& L, V3 position, V2 u, bool hadTransmission, V3 normal) {
  LightSample s{};
  switch (rd16(L, L_TYPE)) {  // light.cu:211-253
    case LT_POINT: s = samplePointLight(L, position, u, hadTransmission, normal); break;
    case LT_SPOT: s = sampleSpotLight(L, position, u, hadTransmission, normal); break;
    case LT_ENV:
      s.direction = sampleUniformSphere(u);
      s.pdf = 0.25f * kInvPi;
      s.factor = 1.f;
      s.pLight = s.direction;
      s.distance = FLT_MAX;
      break;
    case LT_DIR: {
      float unused{};
      s.pLight = sampleUniformCone(dirFromOcta(rd32(L, LD_DIR)), h2f(rd16(L, LD_OMC)), u, &unused,
                                   &s.pdf, &s.delta);
      s.direction = -s.pLight;
      s.factor = 1.f;
      s.delta = true;
      s.distance = FLT_MAX;
      break;
    }
  }
  return s;
}
V3 evalLight(Rec32 const& L, LightSample const& ls) {  // :309-320
  V3 Le = rdh3(L, L_INT) * ls.factor;
  uint16_t const t = rd16(L, L_TYPE);
  if (t == LT_POINT || t == LT_SPOT) Le /= (ls.distance * ls.distance);
  return Le;
}
V3 evalInfiniteLight(Rec32 const& L, V3 /*dir*/, float* pdf) {  // :322-332
  if (rd16(L, L_TYPE) != LT_ENV) {
    *pdf = 0;
    return v3(0, 0, 0);
  }
  *pdf = 0.25f * kPi;
  return rdh3(L, L_INT);
}

// ------------------------------------------------------------------------------------
// GGX energy tables (software lookup, host branch)     CC/private/extra_math.cu:95-126,
// CC/private/bsdf.cu:13-170,407-426
// ------------------------------------------------------------------------------------
const float kGgxE[DMT_GGX_E_ROWS * DMT_GGX_E_COLS] = {DMT_GGX_E_TABLE_VALUES};
const float kGgxEavg[DMT_GGX_EAVG_COUNT] = {DMT_GGX_EAVG_TABLE_VALUES};

float lookupTableRead(float const* table, float x, int32_t size) {
  x = fminf(fmaxf(x, 0.f), 1.f) * (size - 1);
  int32_t const index = int32_t(fminf(float(int32_t(x)), float(size - 1)));
  int32_t const nIndex = int32_t(fminf(float(index + 1), float(size - 1)));
  float const t = x - index;
  float const d0 = table[index];
  if (t == 0.f) return d0;
  float const d1 = table[nIndex];
  return (1.f - t) * d0 + t * d1;
}
float lookupTableRead2D(float const* table, float x, float y, int32_t sx, int32_t sy) {
  y = fminf(fmaxf(y, 0.f), 1.f) * (sy - 1);
  int32_t const index = int32_t(fminf(float(int32_t(y)), float(sy - 1)));
  int32_t const nIndex = int32_t(fminf(float(index + 1), float(sy - 1)));
  float const t = y - index;
  float const d0 = lookupTableRead(table + sx * index, x, sx);
  if (t == 0.f) return d0;
  float const d1 = lookupTableRead(table + sx * nIndex, x, sx);
  return (1.f - t) * d0 + t * d1;
}

// ------------------------------------------------------------------------------------
// BSDFs                       CC/public/cuda-core/bsdf.cuh:75-224, CC/private/bsdf.cu:278-1011
// ------------------------------------------------------------------------------------
struct BSDFSample {
  V3 wi, f;
  float pdf = 0.f;
  float eta = 0.f;
  bool delta = false;
  bool refract = false;
  bool valid() const { return wi.x != 0 && wi.y != 0 && wi.z != 0 && pdf != 0.f; }  // :83-85
};
float fresnelDielectric(float cosI, float eta, float* cosT_out) {  // bsdf.cuh:175-202
  cosI = fmaxf(-1.f, fminf(1.f, cosI));
  bool const entering = cosI > 0.f;
  if (!entering) {
    eta = 1.f / eta;
    cosI = fabsf(cosI);
  }
  float const sinI = safeSqrt(fmaxf(0.f, 1.f - cosI * cosI));
  float const sinT = sinI / eta;
  if (sinT >= 1.f) return 1.f;
  float const cosT = safeSqrt(fmaxf(0.f, 1.f - sinT * sinT));
  *cosT_out = cosT;
  float const rParl = ((eta * cosI) - (cosT)) / ((eta * cosI) + (cosT));
  float const rPerp = ((cosI) - (eta * cosT)) / ((cosI) + (eta * cosT));
  return (rParl * rParl + rPerp * rPerp) * 0.5f;
}
V3 fresnelConductor(float cosI, V3 eta, V3 k) {  // bsdf.cuh:204-224
  cosI = fmaxf(-1.f, fminf(1.f, cosI));
  float const c2 = cosI * cosI;
  float const s2 = 1.f - c2;
  V3 const eta2 = v3(eta.x * eta.x, eta.y * eta.y, eta.z * eta.z);
  V3 const k2 = v3(k.x * k.x, k.y * k.y, k.z * k.z);
  V3 const t0 = eta2 - k2 - s2;
  V3 const a2b2 = sqrtv(t0 * t0 + 4.f * eta2 * k2);
  V3 const t1 = a2b2 + c2;
  V3 const a = sqrtv(0.5f * (a2b2 + t0));
  V3 const t2 = 2.f * cosI * a;
  V3 const Rs = (t1 - t2) / (t1 + t2);
  V3 const t3 = c2 * a2b2 + s2 * s2;
  V3 const t4 = t2 * s2;
  V3 const Rp = Rs * (t3 - t4) / (t3 + t4);
  return 0.5f * (Rp + Rs);
}
void microfacetFresnel(Rec32 const& b, float cos_HO, float* cos_HI, V3* R, V3* T) {  // :331-354
  if (bsdfType(b) == BS_GGX_DIEL) {
    float const F = fresnelDielectric(cos_HO, h2f(rd16(b, GD_ETA)), cos_HI);
    *R = F * rdh3(b, GD_RT);
    *T = (1.f - F) * rdh3(b, GD_TT);
  } else {
    *R = fresnelConductor(cos_HO, rdh3(b, GC_ETA), rdh3(b, GC_K));
    *T = v3(0, 0, 0);
  }
}
inline V3 tangentFromPhi(V3 ns, float phi0) {  // :279-294
  V3 const ref = fabsf(ns.x) < 0.999f ? v3(1.0f, 0.0f, 0.0f) : v3(0.0f, 1.0f, 0.0f);
  V3 const t = normalize(cross(ref, ns));
  V3 const b = cross(ns, t);
  float const s = sinf(phi0);
  float const c = cosf(phi0);
  return c * t + s * b;
}
inline V3 faceForward(V3 n, V3 v) { return dot(n, v) < 0.0f ? -n : n; }
inline float ggxPhi0(Rec32 const& b) {  // bsdf.cuh:52-55
  return float(rd16(b, G_PHI0)) / 65535 * 2.f * kPi;
}
// Probes only (oracle_set_cos_nh_ulps; 0 everywhere else): cos_NH moves by this many fp32 ulps on its way into the
// distribution term D of sampleGGX / evalGGX, which is as far as a differently rounded half vector lands from this one.
// sampleGGX_VNDF's Nh.z, a sum of O(1) terms that it clamps at 0 and renormalises, moves by as many ulps of 1 (2^-24).
// The shading sweep's conditioning filter uses it to find the cases that this rounding decides.
static int g_cosNhUlps = 0;
inline float nudgeCosNH(float c) {
  float const to = g_cosNhUlps > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
  for (int k = 0; k < std::abs(g_cosNhUlps); ++k) c = nextafterf(c, to);
  return c;
}
V3 sampleGGX_VNDF(V3 wo, V2 u, float ax, float ay) {  // :303-329
  V3 const V = normalize(v3(ax * wo.x, ay * wo.y, wo.z));
  V3 T1, T2;
  float const lensq = V.x * V.x + V.y * V.y;
  if (lensq > 1e-7f) {
    float const invLen = rsqrt_host(lensq);
    T1 = v3(-V.y * invLen, V.x * invLen, 0.f);
    T2 = cross(V, T1);
  } else {
    T1 = v3(1, 0, 0);
    T2 = v3(0, 1, 0);
  }
  V2 t = sampleUniformDisk(u);
  t.y = lerpf(safeSqrt(1.f - t.x * t.x), t.y, 0.5f * (1.f + V.z));
  V3 Nh = t.x * T1 + t.y * T2 + safeSqrt(1.f - dot(t, t)) * V;
  Nh.z += float(g_cosNhUlps) * 5.9604645e-8f;  // (probes only; + 0 otherwise)
  Nh = normalize(v3(ax * Nh.x, ay * Nh.y, fmaxf(0.f, Nh.z)));
  return Nh;
}
inline V3 refractAngle(V3 inc, V3 n, float cosT, float invEta) {  // :358-364
  return (invEta * dot(n, inc) + cosT) * n - invEta * inc;
}
inline float ggxLambdaFrom(float x) { return 0.5f * (sqrtf(1.f + x) - 1.f); }
inline float ggx_D(float alpha2, float cos_NH) {
  float const c2 = fminf(cos_NH * cos_NH, 1.f);
  float const omc2 = 1.f - c2;
  return alpha2 / (kPi * sqrf(omc2 + alpha2 * c2));
}
inline float ggx_lambda(float alpha2, float cos_N) {
  return ggxLambdaFrom(alpha2 * fmaxf(0.f, 1.f / sqrf(cos_N)));
}
inline float ggx_aniso_D(float ax, float ay, V3 lH) {
  lH /= v3(ax, ay, 1.f);
  float const alpha2 = ax * ay;
  return kInvPi / (alpha2 * sqrf(dot(lH, lH)));
}
inline float ggx_aniso_lambda(float ax, float ay, V3 V) {
  return ggxLambdaFrom((sqrf(ax * V.x) + sqrf(ay * V.y)) / sqrf(V.z));
}
constexpr float kThroughputEps = 1e-6f;

BSDFSample sampleGGX(Rec32 const& b, V3 wo, V3 ns, V3 ng, V2 u, float uc) {  // :457-569
  BSDFSample s{};
  float const cos_NO = dot(ns, wo);
  uint16_t const axq = rd16(b, G_AX), ayq = rd16(b, G_AY);
  bool const isotropic = axq == ayq;
  float const ax = float(axq) / 65535;
  float const ay = float(ayq) / 65535;
  V3 const tangent = tangentFromPhi(ns, ggxPhi0(b));
  s.eta = 1.f;
  float invEta = 1.f;
  s.delta = fmaxf(ax, ay) < 1e-3f;
  V3 H{}, lH{}, lO{};
  if (s.delta) {
    H = ns;
  } else {
    V3 X{}, Y{};
    if (isotropic)
      gramSchmidt(ns, &X, &Y);
    else
      orthonormalTangent(ns, tangent, &X, &Y);
    lO = v3(dot(X, wo), dot(Y, wo), cos_NO);
    lH = sampleGGX_VNDF(lO, u, ax, ay);
    H = lH.x * X + lH.y * Y + lH.z * ns;
  }
  float const cos_HO = dot(H, wo);
  float cos_HI{};
  V3 R{}, T{};
  microfacetFresnel(b, cos_HO, &cos_HI, &R, &T);
  if (nearZeroPos(R, kThroughputEps) && nearZeroPos(T, kThroughputEps)) return s;
  float const pdfReflect = fminf(fmaxf(average(R) / average(R + T), 0.f), 1.f);
  s.refract = uc > pdfReflect;
  if (s.refract) invEta = 1.f / h2f(rd16(b, GD_ETA));
  s.wi = s.refract ? refractAngle(wo, H, cos_HI, invEta) : 2.f * cos_HO * H - wo;
  if (dot(ng, s.wi) <= 0 && !s.refract) {
    s.pdf = 0;
    return s;
  }
  if (s.refract) {
    s.f = T;
    s.pdf = 1.f - pdfReflect;
    s.delta |= fabsf(s.eta - 1.f) < 1e-4f;  // eta is still 1 here -> always delta (:531)
  } else {
    s.pdf = pdfReflect;
    // NOTE (:526-534): on reflection sample.f is left at its zero initialisation.
  }
  if (s.delta) {
    s.pdf *= 1e6f;
    s.f *= 1e6f;
  } else {
    float D{}, lamI{}, lamO{};
    if (isotropic || s.refract) {
      float const alpha2 = ax * ay;
      float const cos_NH = nudgeCosNH(lH.z);
      float const cos_NI = dot(ns, s.wi);
      D = ggx_D(alpha2, cos_NH);
      lamI = ggx_lambda(alpha2, cos_NI);
      lamO = ggx_lambda(alpha2, cos_NO);
    } else {
      V3 const lI = 2.f * cos_HO * lH - lO;
      D = ggx_aniso_D(ax, ay, v3(lH.x, lH.y, nudgeCosNH(lH.z)));
      lamI = ggx_aniso_lambda(ax, ay, lI);
      lamO = ggx_aniso_lambda(ax, ay, lO);
    }
    float const common =
        D / cos_NO * (s.refract ? fabsf(cos_HO * cos_HI) / sqrf(cos_HI + cos_HO * invEta) : 0.25f);
    s.pdf *= common / (1.f + lamO);
    s.f *= common / (1.f + lamO + lamI);
  }
  return s;
}
V3 evalGGX(Rec32 const& b, V3 wo, V3 wi, V3 ns, V3 ng, float* pdf) {  // :571-667
  float const energyScale = rdf(b, G_ESCALE);
  bool const conductor = bsdfType(b) == BS_GGX_COND;
  bool const hasReflection = conductor ? true : luminance(rdh3(b, GD_RT)) > kThroughputEps;
  bool const hasTransmission = conductor ? false : luminance(rdh3(b, GD_TT)) > kThroughputEps;
  float const ax = float(rd16(b, G_AX)) / 65535;
  float const ay = float(rd16(b, G_AY)) / 65535;
  bool const isotropic = ax == ay;
  float const cos_NO = dot(ns, wo);
  float const cos_NI = dot(ns, wi);
  float const cos_NgI = dot(ng, wi);
  bool const isTransmission = cos_NI < 0.f;
  float const ior = isTransmission ? h2f(rd16(b, GD_ETA)) : 1.f;
  bool const effSpecular = fmaxf(ax, ay) < 1e-3f;
  if (cos_NO <= 0.f || (cos_NgI < 0) != isTransmission || effSpecular ||
      (!hasReflection && cos_NgI > 0.f) || (!hasTransmission && cos_NgI < 0.f)) {
    *pdf = 0.f;
    return v3(0, 0, 0);
  }
  V3 H = isTransmission ? (ior * wi + wo) : (wi + wo);
  float const invLen_H = rsqrt_host(dot(H, H));
  H *= invLen_H;
  float const cos_HO = dot(H, wo);
  float unused{};
  V3 R{}, T{};
  microfacetFresnel(b, cos_HO, &unused, &R, &T);
  if (nearZeroPos(R, kThroughputEps) && nearZeroPos(T, kThroughputEps)) {
    *pdf = 0.f;
    return v3(0, 0, 0);
  }
  float const cos_NH = nudgeCosNH(dot(ns, H));
  float D{}, lamI{}, lamO{};
  if (isotropic || isTransmission) {
    float const alpha2 = ax * ay;
    D = ggx_D(alpha2, cos_NH);
    lamI = ggx_lambda(alpha2, cos_NI);
    lamO = ggx_lambda(alpha2, cos_NO);
  } else {
    V3 const tangent = tangentFromPhi(ns, ggxPhi0(b));
    V3 X{}, Y{};
    orthonormalTangent(ns, tangent, &X, &Y);
    V3 const lH = v3(dot(X, H), dot(Y, H), cos_NH);
    V3 const lO = v3(dot(X, wo), dot(Y, wo), cos_NO);
    V3 const lI = v3(dot(X, wi), dot(Y, wi), cos_NI);
    D = ggx_aniso_D(ax, ay, lH);
    lamI = ggx_aniso_lambda(ax, ay, lI);
    lamO = ggx_aniso_lambda(ax, ay, lO);
  }
  float const common =
      D / cos_NO * (isTransmission ? sqrf(ior * invLen_H) * fabsf(cos_HO * dot(H, wi)) : 0.25f);
  float const pdfReflect = average(R) / average(R + T);
  float const lobePdf = isTransmission ? 1.f - pdfReflect : pdfReflect;
  *pdf = lobePdf * common / (1.f + lamO);
  return energyScale * (isTransmission ? T : R) * common / (1.f + lamO + lamI);
}
BSDFSample sampleLambert(Rec32 const&, V3 /*wo*/, V3 ns, V3 ng, V2 u, float) {  // :719-733
  BSDFSample s{};
  s.eta = 1.f;
  s.wi = sampleCosHemisphere(ns, u, &s.pdf);
  if (dot(ng, s.wi) > 0.f)
    s.f = v3(s.pdf, s.pdf, s.pdf);
  else
    s.pdf = 0;
  return s;
}
V3 evalLambert(Rec32 const&, V3, V3 wi, V3 ns, V3, float* pdf) {  // :735-741
  float const cos_NI = fmaxf(dot(ns, wi), 0.f);
  *pdf = cos_NI * kInvPi;
  return v3(*pdf, *pdf, *pdf);
}
float orenNayar_G(float cosTheta) {  // :751-763
  float const piOver2 = kPi / 2;
  float const twoThirds = 2.f / 3.f;
  float const piOver2m = piOver2 - twoThirds;
  if (cosTheta < 1e-6f) return piOver2m - cosTheta;
  float const sinTheta = sin_from_cos(cosTheta);
  float const theta = safeacos(cosTheta);
  return sinTheta * (theta - twoThirds - sinTheta * cosTheta) +
         twoThirds * (sinTheta / cosTheta) * (1.f - sqrf(sinTheta) * sinTheta);
}
V3 orenNayarIntensity(Rec32 const& b, V3 n, V3 v, V3 l) {  // :765-788
  float const a = h2f(rd16(b, ON_A));
  float const bb = h2f(rd16(b, ON_B));
  V3 const ms = rdh3(b, ON_MS);
  float const nl = fmaxf(dot(n, l), 0.f);
  if (bb <= 0) {
    float const r = nl * kInvPi;
    return v3(r, r, r);
  }
  float const nv = fmaxf(dot(n, v), 0.f);
  float t = dot(l, v) - nl * nv;
  if (t > 0.f) t /= fmaxf(nl, nv) + FLT_MIN;
  float const single = a + bb * t;
  float const El = a * kPi + bb * orenNayar_G(nl);
  V3 const multi = ms * (1.f - El);
  return nl * (single + multi);
}
BSDFSample sampleOrenNayar(Rec32 const& b, V3 wo, V3 ns, V3 ng, V2 u, float) {  // :790-802
  BSDFSample s{};
  s.eta = 1.f;
  s.wi = sampleCosHemisphere(ns, u, &s.pdf);
  if (dot(ng, s.wi) > 0.f)
    s.f = orenNayarIntensity(b, ns, wo, s.wi);
  else
    s.pdf = 0;
  return s;
}
V3 evalOrenNayar(Rec32 const& b, V3 wo, V3 wi, V3 ns, V3, float* pdf) {  // :804-812
  float const cos_NI = dot(ns, wi);
  if (cos_NI > 0.f) {
    *pdf = cos_NI * kInvPi;
    return orenNayarIntensity(b, ns, wo, wi);
  }
  return v3(0, 0, 0);
}
BSDFSample sampleBsdf(Rec32 const& b, V3 wo, V3 ns, V3 ng, V2 u, float uc) {  // :851-880
  BSDFSample s{};
  if (dot(wo, ng) > 0.0f) {
    ns = faceForward(ns, ng);
    switch (bsdfType(b)) {
      case BS_OREN: s = sampleOrenNayar(b, wo, ns, ng, u, uc); break;
      case BS_GGX_DIEL:
      case BS_GGX_COND: s = sampleGGX(b, wo, ns, ng, u, uc); break;
      case BS_LAMBERT: s = sampleLambert(b, wo, ns, ng, u, uc); break;
    }
  }
  return s;
}
V3 evalBsdf(Rec32 const& b, V3 wo, V3 wi, V3 ns, V3 ng, float* pdf) {  // :882-907
  V3 f = v3(0, 0, 0);
  *pdf = 0;
  switch (bsdfType(b)) {
    case BS_OREN: f = evalOrenNayar(b, wo, wi, ns, ng, pdf); break;
    case BS_GGX_COND:
    case BS_GGX_DIEL: f = evalGGX(b, wo, wi, ns, ng, pdf); break;
    case BS_LAMBERT: f = evalLambert(b, wo, wi, ns, ng, pdf); break;
  }
  return f;
}
void energyPreservingGGXScale(Rec32& b, float alpha2, float cos_NO, V3 Fss) {  // :407-426
  float const E = lookupTableRead2D(kGgxE, alpha2, cos_NO, DMT_GGX_E_COLS, DMT_GGX_E_ROWS);
  float const Eavg = lookupTableRead(kGgxEavg, alpha2, DMT_GGX_EAVG_COUNT);
  float const missing = (1.f - E) / E;
  float const escale = 1.f + missing;
  wrf(b, G_ESCALE, escale);
  V3 const Fms = Fss * Eavg / (v3(1, 1, 1) - Fss * (1.f - Eavg));
  bsdfSetWeight(b, bsdfWeight(b) * (1.f + Fms * missing) / escale);
}
void prepareBSDF(Rec32* b, V3 ns, V3 wo, int /*transmissionCount*/) {  // :909-1011
  switch (bsdfType(*b)) {
    case BS_OREN: {
      float const a = h2f(rd16(*b, ON_A));
      float const bb = h2f(rd16(*b, ON_B));
      V3 const albedo = bsdfWeight(*b);
      float const nl = fmaxf(0.f, dot(ns, wo));
      float const Ev = a * kPi + bb * orenNayar_G(nl);
      V3 ms = albedo * (1.f - Ev);
      ms.x = fmaxf(ms.x, 0.f), ms.y = fmaxf(ms.y, 0.f), ms.z = fmaxf(ms.z, 0.f);
      wrh3(*b, ON_MS, ms);
      break;
    }
    case BS_GGX_DIEL:
    case BS_GGX_COND: {
      {
        float const cos_HO = fabsf(dot(wo, ns));
        float unused{};
        V3 R, T;
        microfacetFresnel(*b, cos_HO, &unused, &R, &T);
        bsdfSetWeight(*b, R + T);
      }
      V3 Fss{};
      if (bsdfType(*b) == BS_GGX_DIEL) {
        Fss = rdh3(*b, GD_TT);
      } else {
        V3 const eta = rdh3(*b, GC_ETA);
        V3 const kappa = rdh3(*b, GC_K);
        V3 const F0 = fresnelConductor(1.f, eta, kappa);
        V3 const F82 = fresnelConductor(1.f / 7.f, eta, kappa);
        V3 const B = (lerp3(F0, v3(1, 1, 1), 0.46266436f) - F82) * 17.651384f;
        Fss = lerp3(F0, v3(1, 1, 1), 1.f / 21.f) - B * (1.f / 126.f);
      }
      float const ax = float(rd16(*b, G_AX)) / 65535;
      float const ay = float(rd16(*b, G_AY)) / 65535;
      float const alpha2 = ax * ay;
      float const cos_NO = fmaxf(0.f, dot(ns, wo));
      energyPreservingGGXScale(*b, alpha2, cos_NO, Fss);
      break;
    }
    case BS_LAMBERT: break;
  }
}

// ------------------------------------------------------------------------------------
// scene + integrator                               T/megakernel/megakernel.cu:53-322
// ------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------
// A18: environment-map light of the reference's CPU renderer
//   PiecewiseConstant1D/2D       src/core/private/core-math.cu:385-675
//   EnvLight, sample, eval       src/core/private/core-light.cpp:84-117,394-491
//   MIS rules                    src/core/private/core-render.cpp:154-163,290-299,357-369
// Restated with the reference's quirks: the 1-D CDF is INCLUSIVE (cdf[i] = sum_{j<=i}) and is summed in the
// AVX2 block order of core-math.cu:440-485; sample() never returns the last bin and prices bin `off` with
// func[off] although the inclusive CDF puts u in bin off+1 (core-math.cu:566-595); the sampling direction
// uses phi = clamp(1 - 2 pi u, -pi, pi) and theta = pi v while evaluation by direction uses the flipped
// v = 1 - theta/pi (the #define sits in the middle of core-light.cpp, line 468); the light's scale factor is
// stored and never applied (core-light.cpp:115,444-452).  Quaternion products are glm's Hamilton product
// (dependency g-truc/glm, fetched by cmake/Dependencies.cmake:50-57, not vendored).
// ------------------------------------------------------------------------------------
struct Pc1D {
  std::vector<float> absf, cdf;  // both n entries
  float integral = 0.f;
};
inline void pc1dBuild(float const* f, uint32_t n, float mn, float mx, Pc1D& out) {
  out.absf.resize(n), out.cdf.resize(n);
  for (uint32_t i = 0; i < n; ++i) out.absf[i] = fabsf(f[i]);
  float const fac = (mx - mn) / float(n);
  float carry = 0.f;
  uint32_t const nb = n & ~7u;
  for (uint32_t b = 0; b < nb; b += 8) {  // core-math.cu:447-481: in-lane prefix sums, lane 0 total into lane 1, carry
    float x[8];
    for (int j = 0; j < 8; ++j) x[j] = f[b + uint32_t(j)] * fac;
    for (int l = 0; l < 8; l += 4) {
      float const a0 = x[l], a1 = x[l + 1] + x[l], a2 = x[l + 2] + x[l + 1], a3 = x[l + 3] + x[l + 2];
      x[l] = a0, x[l + 1] = a1, x[l + 2] = a2 + a0, x[l + 3] = a3 + a1;
    }
    float const lane0 = x[3];
    for (int j = 4; j < 8; ++j) x[j] = x[j] + lane0;
    for (int j = 0; j < 8; ++j) out.cdf[b + uint32_t(j)] = x[j] + carry;
    carry = out.cdf[b + 7];
  }
  for (uint32_t i = nb; i < n; ++i)  // core-math.cu:484-490 (unscaled; only n < 8 or non-multiples reach it)
    out.cdf[i] = (i ? out.cdf[i - 1] : 0.f) + f[i];
  out.integral = out.cdf[n - 1];
  bool const zero = fabsf(out.integral) <= std::numeric_limits<float>::epsilon();  // fl::nearZero
  float const fac2 = 1.0f / (zero ? float(n) : out.integral);                        // fl::rcp
  if (zero)
    for (uint32_t i = 0; i < n; ++i) out.cdf[i] = float(i) * fac2;
  else
    for (uint32_t i = 0; i < n; ++i) out.cdf[i] *= fac2;
}
inline int32_t findIntervalLessThan(int32_t sz, float const* cdf, float u) {  // core-math.cu:553-564
  int32_t size = sz - 2, first = 1;
  while (size > 0) {
    int32_t const half = size >> 1, middle = first + half;
    bool const pred = cdf[middle] <= u;
    first = pred ? middle + 1 : first;
    size = pred ? size - (half + 1) : half;
  }
  int32_t const r = first - 1;
  return r < 0 ? 0 : (r > sz - 2 ? sz - 2 : r);
}
inline float pc1dSample(float const* absf, float const* cdf, int32_t n, float integral, float u, float* pdf,
                        int32_t* offset) {  // core-math.cu:566-582, domain [0,1]
  int32_t const off = findIntervalLessThan(n, cdf, u);
  *offset = off;
  float du = u - cdf[off];
  if (cdf[off + 1] - cdf[off] > 0) du /= cdf[off + 1] - cdf[off];
  *pdf = integral > 0 ? absf[off] / integral : 0.f;
  float const delta = (float(off) + du) / float(n);
  return delta == 0.f ? 0.f : (1.f - 0.f) * delta + 0.f;  // fl::lerp(delta, min = 0, max = 1)
}
struct EnvMap {
  int w = 0, h = 0;
  float const* rgb = nullptr;       // h x w x 3
  std::vector<float> func, cdf;     // conditional rows, h x w each
  std::vector<float> rowInt;        // integral of each row
  Pc1D marginal;                    // over rows
  float q[4] = {0, 0, 0, 1};        // lightFromRender, normalised (x, y, z, w)
  float scale = 1.f;
};
inline void envBuild(float const* rgb, int w, int h, float const* quat, float scale, EnvMap& e) {
  e.w = w, e.h = h, e.rgb = rgb, e.scale = scale;
  e.func.resize(size_t(w) * h), e.cdf.resize(size_t(w) * h), e.rowInt.resize(size_t(h));
  std::vector<float> row(static_cast<size_t>(w), 0.f);
  for (int y = 0; y < h; ++y) {  // distributionFromImage: RGB::avg() per texel (core-light.cpp:84-103)
    for (int x = 0; x < w; ++x) {
      float const* p = rgb + 3 * (size_t(x) + size_t(y) * size_t(w));
      row[size_t(x)] = (p[0] + p[1] + p[2]) / 3.f;
    }
    Pc1D c;
    pc1dBuild(row.data(), uint32_t(w), 0.f, 1.f, c);
    memcpy(&e.func[size_t(y) * w], c.absf.data(), size_t(w) * 4);
    memcpy(&e.cdf[size_t(y) * w], c.cdf.data(), size_t(w) * 4);
    e.rowInt[size_t(y)] = c.integral;
  }
  pc1dBuild(e.rowInt.data(), uint32_t(h), 0.f, 1.f, e.marginal);
  float const len = sqrtf(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
  for (int i = 0; i < 4; ++i) e.q[i] = quat[i] / len;  // normalize(quat), core-light.cpp:110
}
struct Quat {
  float x, y, z, w;
};
inline Quat qmul(Quat p, Quat q) {  // glm::qua operator*
  return Quat{p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y, p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z,
              p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x, p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z};
}
inline float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
struct EnvSample {
  V3 wi;
  float pdf;
  V2 uv;
  bool ok;
};
inline EnvSample envSample(EnvMap const& e, V2 u) {  // envLightSampleFromContext, core-light.cpp:394-442
  EnvSample r{};
  float pdfs[2];
  int32_t iu, iv;
  float const d1 = pc1dSample(e.marginal.absf.data(), e.marginal.cdf.data(), e.h, e.marginal.integral, u.y, &pdfs[1], &iv);
  float const d0 = pc1dSample(&e.func[size_t(iv) * e.w], &e.cdf[size_t(iv) * e.w], e.w, e.rowInt[size_t(iv)], u.x, &pdfs[0], &iu);
  float const mapPdf = pdfs[0] * pdfs[1];
  r.uv = V2{d0, d1};
  if (mapPdf == 0.f) return r;
  float const kPi = 3.14159265358979323846f;
  float const phi = clampf(1.f - 2.f * kPi * d0, -kPi, kPi);
  float const theta = clampf(kPi * d1, 0.f, kPi);
  // cartesianFromSpherical(1, phi, theta), cudautils-numbers.cuh:15-25
  float const sp = sinf(phi), cp = cosf(phi), st = sinf(theta), ct = cosf(theta);
  Quat const wl{1.f * sp * ct, 1.f * sp * st, 1.f * cp, 0.f};
  Quat const q{e.q[0], e.q[1], e.q[2], e.q[3]};
  Quat const qc{-q.x, -q.y, -q.z, q.w};
  Quat const wi = qmul(qmul(qc, wl), q);
  r.wi = v3(wi.x, wi.y, wi.z);
  r.pdf = mapPdf / (4 * kPi);
  r.ok = true;
  return r;
}
inline V3 envEvalUv(EnvMap const& e, V2 uv) {  // envLightEval(light, sample), core-light.cpp:444-452
  int32_t const xi = int32_t(roundf(clampf(uv.x, 0.f, 1.f) * float(e.w - 1)));
  int32_t const yi = int32_t(roundf(clampf(uv.y, 0.f, 1.f) * float(e.h - 1)));
  float const* p = e.rgb + 3 * (size_t(xi) + size_t(yi) * size_t(e.w));
  return v3(p[0], p[1], p[2]);
}
inline float pc2dPdf(EnvMap const& e, V2 p) {  // PiecewiseConstant2D::pdf, core-math.cu:628-644
  int32_t iu = int32_t(p.x * float(e.w)), iv = int32_t(p.y * float(e.h));
  iu = iu < 0 ? 0 : (iu > e.w - 1 ? e.w - 1 : iu);
  iv = iv < 0 ? 0 : (iv > e.h - 1 ? e.h - 1 : iv);
  return e.func[size_t(iv) * e.w + size_t(iu)] / e.marginal.integral;
}
inline V3 envEvalDir(EnvMap const& e, V3 wi, float* pdf) {  // envLightEval(light, wi, pdf), core-light.cpp:454-491
  Quat const q{e.q[0], e.q[1], e.q[2], e.q[3]};
  Quat const qc{-q.x, -q.y, -q.z, q.w};
  Quat const wl = qmul(qmul(q, Quat{wi.x, wi.y, wi.z, 0.f}), qc);
  float const kPi = 3.14159265358979323846f;
  float const theta = acosf(clampf(wl.z, -1.f, 1.f));
  float const phi = atan2f(wl.y, wl.x);
  V2 const uv{0.5f * (1.f + phi / kPi), 1.f - theta / kPi};
  *pdf = pc2dPdf(e, uv) / (4.f * kPi);
  int32_t xi = int32_t(uv.x * float(e.w)), yi = int32_t(uv.y * float(e.h));
  xi = xi < 0 ? 0 : (xi > e.w - 1 ? e.w - 1 : xi);
  yi = yi < 0 ? 0 : (yi > e.h - 1 ? e.h - 1 : yi);
  float const* p = e.rgb + 3 * (size_t(xi) + size_t(yi) * size_t(e.w));
  return v3(p[0], p[1], p[2]);
}

struct Camera {  // CC/public/cuda-core/types.cuh:101-109 (44 bytes)
  float dir[3];
  float pos[3];
  int32_t width, height, spp;
  float focalLength, sensorSize;
};
static_assert(sizeof(Camera) == 44, "DeviceCamera layout");

struct LtNode;
struct LtrNode;
struct Scene {
  float const* xs;  // float4 per triangle
  float const* ys;
  float const* zs;
  uint32_t const* matId;
  uint64_t triCount;
  Rec32 const* lights;
  uint32_t lightCount;
  Rec32 const* infLights;
  uint32_t infLightCount;
  Rec32 const* bsdfs;
  uint32_t bsdfCount;
  EnvMap const* env = nullptr;  // A18: replaces the constant environment when set
  // emissive triangles (diffuse area lights).  areaOf[tri] = index into areaTri / areaLe or ~0u
  uint32_t const* areaOf = nullptr;
  uint32_t const* areaTri = nullptr;
  float const* areaLe = nullptr;  // rgb per area light
  uint32_t areaCount = 0;
  // image textures of JSON materials (no implementation on the reference's megakernel path; semantics follow
  // its CPU renderer, src/core/private/core-material.cpp:20-56,180-240).  texDesc[k] = {first texel, width, height} into
  // texRgba (RGBA8); matTex[bsdf] = {diffuse, roughness, normal texture index or -1, anisotropy as float bits};
  // triUv[tri] = {u0, v0, u1, v1, u2, v2}
  uint8_t const* texRgba = nullptr;
  int32_t const* texDesc = nullptr;
  uint32_t texCount = 0;
  uint32_t const* matTex = nullptr;
  float const* triUv = nullptr;
  // light tree (see "light tree" below); null = the megakernel's uniform pick
  LtNode const* lightTree = nullptr;
  LtrNode const* lightTreeRef = nullptr;  // lightSampling == 2: the reference's tree (cones, SAOH, cuts of up to four lights)
};

struct Stats {  // algorithmic work counters (SURVEY 8d byte model)
  uint64_t samples = 0, closestRays = 0, shadowRays = 0, triTests = 0, bounces = 0, hits = 0;
};

struct RenderCfg {
  HaltonParams hp;
  Xform cameraFromRaster, renderFromCamera;
  int width, height;
  int maxDepth;
  bool rtlArgs;
};

inline uint32_t pickIndex(float u, uint32_t count) {
  // min(static_cast<int>(u * count), count - 1) with CUDA's min(int, unsigned) -> unsigned
  uint32_t const a = uint32_t(int(u * float(count)));
  uint32_t const b = count - 1u;
  return a < b ? a : b;
}

// ---- emissive triangles (no reference implementation exists).  Semantics are pbrt-v4's, which the
// reference's scenes/cornell-box.pbrt is written for: DiffuseAreaLight, one-sided on the side of
// n = normalize(cross(p1 - p0, p2 - p0)); uniform point sampling (SampleUniformTriangle); light chosen uniformly among
// [point/spot lights..., emissive triangles...]; power-heuristic MIS between light and BSDF sampling; emission seen
// directly by camera rays and after delta bounces.
struct AreaSample {
  V3 wi;
  float dist, pdf;  // solid-angle pdf
  bool ok;
};
inline void areaTriangle(Scene const& sc, uint32_t tri, V3& p0, V3& p1, V3& p2) {
  float const *x = sc.xs + 4 * size_t(tri), *y = sc.ys + 4 * size_t(tri), *z = sc.zs + 4 * size_t(tri);
  p0 = v3(x[0], y[0], z[0]), p1 = v3(x[1], y[1], z[1]), p2 = v3(x[2], y[2], z[2]);
}
inline AreaSample areaSample(Scene const& sc, uint32_t tri, V3 p, V2 u) {
  AreaSample r{};
  V3 p0, p1, p2;
  areaTriangle(sc, tri, p0, p1, p2);
  float b0, b1;
  if (u.x < u.y) {
    b0 = u.x / 2;
    b1 = u.y - b0;
  } else {
    b1 = u.y / 2;
    b0 = u.x - b1;
  }
  V3 const q = b0 * p0 + b1 * p1 + (1 - b0 - b1) * p2;
  V3 const c = cross(p1 - p0, p2 - p0);
  float const len = sqrtf(dot(c, c));
  if (!(len > 0.f)) return r;
  V3 const n = c / len;
  V3 const d = q - p;
  float const d2 = dot(d, d);
  if (!(d2 > 0.f)) return r;
  r.dist = sqrtf(d2);
  r.wi = d / r.dist;
  float const cosL = -dot(n, r.wi);
  if (!(cosL > 0.f)) return r;  // one-sided
  r.pdf = d2 / (cosL * (0.5f * len));
  r.ok = true;
  return r;
}
// pdf (solid angle) of having sampled the point a ray hits on emissive triangle `tri`; 0 when seen from behind
inline float areaPdf(Scene const& sc, uint32_t tri, V3 rayD, float t) {
  V3 p0, p1, p2;
  areaTriangle(sc, tri, p0, p1, p2);
  V3 const c = cross(p1 - p0, p2 - p0);
  float const len = sqrtf(dot(c, c));
  if (!(len > 0.f)) return 0.f;
  float const cosL = -dot(c / len, rayD);
  if (!(cosL > 0.f)) return 0.f;
  return (t * t) / (cosL * (0.5f * len));
}

// one path; returns radiance L                                      megakernel.cu:103-297
// ---- light tree ------------------------------------------------------------------------------------
// Restates src/core/private/core-light-tree-builder.cpp (LightBounds :52-70, lbImportance :98-146, split cost :246-263,
// selection :496-539, per-light probability :541-557) with the differences the product documents in csrc/light_tree.hpp:
// every light omnidirectional (the megakernel's spot cone does not attenuate), one light per bounce, splits found by a
// sorted sweep over the node's own lights, bounding-sphere test on |centre - p|^2.  No reference-side vectors: unpinned.
struct LtNode {
  float lo[3];
  float phi;
  float hi[3];
  uint32_t ref;  // leaf: 0x80000000 | light; inner: left child (right = left + 1)
};
struct LtItem {
  V3 pos;
  float radius, phi;
  uint32_t index;
};
inline float ltImportance(LtNode const& nd, V3 p, V3 n) {
  V3 const c = v3(0.5f * (nd.lo[0] + nd.hi[0]), 0.5f * (nd.lo[1] + nd.hi[1]), 0.5f * (nd.lo[2] + nd.hi[2]));
  V3 const dg = v3(nd.hi[0] - nd.lo[0], nd.hi[1] - nd.lo[1], nd.hi[2] - nd.lo[2]);
  float const halfDiag = 0.5f * sqrtf(dg.x * dg.x + dg.y * dg.y + dg.z * dg.z);
  V3 const w = p - c;
  float const d2 = w.x * w.x + w.y * w.y + w.z * w.z;
  float const distSqr = fmaxf(fmaxf(d2, halfDiag), 1e-20f);  // floor: a zero-radius light at the shading point (as the product)
  float sinB = 0.f, cosB = -1.f;
  if (d2 >= halfDiag * halfDiag && d2 > 0.f) {
    float const s2 = (halfDiag * halfDiag) / d2;
    sinB = sqrtf(s2), cosB = sqrtf(fmaxf(0.f, 1.f - s2));
  }
  float cosI = 1.f;
  if (d2 > 0.f) cosI = fabsf((w.x * n.x + w.y * n.y + w.z * n.z) * (1.f / sqrtf(d2)));
  float const sinI = sqrtf(fmaxf(0.f, 1.f - cosI * cosI));
  float const cosIB = cosI > cosB ? 1.f : cosI * cosB + sinI * sinB;
  return fmaxf(nd.phi * cosIB / distSqr, 0.f);
}
inline int ltSelect(LtNode const* nodes, V3 p, V3 n, float u, float* pmf) {
  uint32_t at = 0;
  *pmf = 1.f;
  for (int guard = 0; guard < 64; ++guard) {
    LtNode const& nd = nodes[at];
    if (nd.ref & 0x80000000u) return int(nd.ref & 0x7FFFFFFFu);
    float const i0 = ltImportance(nodes[nd.ref], p, n), i1 = ltImportance(nodes[nd.ref + 1u], p, n);
    float const sum = i0 + i1;
    if (!(sum > 0.f)) return -1;
    float const p0 = i0 / sum;
    if (u < p0) {
      *pmf *= p0;
      u = fminf(u / p0, 0.99999994f);
      at = nd.ref;
    } else {
      *pmf *= 1.f - p0;
      u = fminf((u - p0) / (1.f - p0), 0.99999994f);
      at = nd.ref + 1u;
    }
  }
  return -1;
}
inline void ltBounds(std::vector<LtItem> const& it, size_t a, size_t b, float lo[3], float hi[3], float* phi) {
  *phi = 0.f;
  for (int k = 0; k < 3; ++k) lo[k] = std::numeric_limits<float>::infinity(), hi[k] = -std::numeric_limits<float>::infinity();
  for (size_t i = a; i < b; ++i) {
    float const q[3] = {it[i].pos.x, it[i].pos.y, it[i].pos.z};
    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], q[k] - it[i].radius), hi[k] = std::max(hi[k], q[k] + it[i].radius);
    *phi += it[i].phi;
  }
}
inline double ltArea(float const lo[3], float const hi[3]) {
  double const dx = double(hi[0]) - lo[0], dy = double(hi[1]) - lo[1], dz = double(hi[2]) - lo[2];
  return 2.0 * (dx * dy + dy * dz + dz * dx);
}
inline std::vector<LtNode> ltBuild(Rec32 const* lights, uint32_t count) {
  std::vector<LtItem> items;
  for (uint32_t i = 0; i < count; ++i) {
    uint16_t const type = rd16(lights[i], L_TYPE);
    if (type != LT_POINT && type != LT_SPOT) continue;
    V3 const c = rdh3(lights[i], L_INT);
    LtItem it;
    it.pos = rdf3(lights[i], LP_POS);
    it.radius = fmaxf(h2f(rd16(lights[i], type == LT_POINT ? LP_RAD : LS_RAD)), 0.f);
    it.phi = 4.f * 3.14159265358979323846f * fmaxf(0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z, 0.f);
    it.index = i;
    items.push_back(it);
  }
  std::vector<LtNode> nodes;
  if (items.empty()) return nodes;
  struct Work {
    uint32_t node;
    size_t a, b;
  };
  nodes.emplace_back();
  std::vector<Work> stack{{0u, 0, items.size()}};
  while (!stack.empty()) {
    Work const w = stack.back();
    stack.pop_back();
    LtNode nd{};
    ltBounds(items, w.a, w.b, nd.lo, nd.hi, &nd.phi);
    if (w.b - w.a == 1) {
      nd.ref = 0x80000000u | items[w.a].index;
      nodes[w.node] = nd;
      continue;
    }
    int axis = 0;
    for (int k = 1; k < 3; ++k)
      if (nd.hi[k] - nd.lo[k] > nd.hi[axis] - nd.lo[axis]) axis = k;
    auto coord = [axis](LtItem const& x) { return axis == 0 ? x.pos.x : (axis == 1 ? x.pos.y : x.pos.z); };
    std::stable_sort(items.begin() + long(w.a), items.begin() + long(w.b), [&](LtItem const& x, LtItem const& y) {
      return coord(x) < coord(y) || (coord(x) == coord(y) && x.index < y.index);
    });
    size_t const n = w.b - w.a;
    size_t best = n / 2;
    double bestCost = std::numeric_limits<double>::infinity();
    for (size_t k = 1; k < n; ++k) {
      float lo[3], hi[3], phiL, phiR;
      ltBounds(items, w.a, w.a + k, lo, hi, &phiL);
      double const cl = double(phiL) * ltArea(lo, hi);
      ltBounds(items, w.a + k, w.b, lo, hi, &phiR);
      double const cost = cl + double(phiR) * ltArea(lo, hi);
      if (cost < bestCost * (1.0 - 1e-9)) bestCost = cost, best = k;
    }
    uint32_t const left = uint32_t(nodes.size());
    nodes.emplace_back(), nodes.emplace_back();
    nd.ref = left;
    nodes[w.node] = nd;
    stack.push_back({left + 1u, w.a + best, w.b});
    stack.push_back({left, w.a, w.a + best});
  }
  return nodes;
}
inline void ltPmfs(std::vector<LtNode> const& nodes, V3 p, V3 n, float* out, uint32_t count) {
  for (uint32_t i = 0; i < count; ++i) out[i] = 0.f;
  if (nodes.empty()) return;
  std::vector<std::pair<uint32_t, float>> stack{{0u, 1.f}};
  while (!stack.empty()) {
    auto const w = stack.back();
    stack.pop_back();
    LtNode const& nd = nodes[w.first];
    if (nd.ref & 0x80000000u) {
      if ((nd.ref & 0x7FFFFFFFu) < count) out[nd.ref & 0x7FFFFFFFu] = w.second;
      continue;
    }
    float const i0 = ltImportance(nodes[nd.ref], p, n), i1 = ltImportance(nodes[nd.ref + 1u], p, n);
    if (!(i0 + i1 > 0.f)) continue;
    float const p0 = i0 / (i0 + i1);
    stack.push_back({nd.ref, w.second * p0});
    stack.push_back({nd.ref + 1u, w.second * (1.f - p0)});
  }
}

// ---- the reference's light tree with its own semantics (lightSampling == 2) --------------------------------------
// Restates src/core/private/core-light-tree-builder.cpp: directionConesUnion :5-49, lbUnion :52-69, cosSubClamped /
// sinSubClamped / sinCosThetaBoundsSubtended :77-96, lbImportance :98-146, makeLBFromLight :149-187,
// adaptiveSplittingHeuristic :190-232, lightTreeBounds_Kr / _Ma / _Momega and summedAreaOrientationHeuristic :235-283,
// lightTreeBuildRecursive :305-392, lightTreeComputeVariances :394-426, lightTreeAdaptiveSplit :448-491,
// selectLightsFromSplit :493-539 (sampleDiscrete: core-math.cu:366-392); constants core-light-tree-builder.h:62-65.
// Kept as written: cosTheta_e of a union = fmaxf (:63), distances clamped against the half diagonal's LENGTH (:112, :202),
// M_omega's "cosTheta_diff" being a sine (:254), twoSided = false, the pow(., 1/4).  Four places where the written code is
// undefined or defeats itself are corrected exactly as the product documents them (csrc/light_tree_ref.hpp, [fix 1..4]):
// bins filled from the node's own lights, split planes offset by the node's lower bound, both children always present with
// the bounds of their own lights, |centre - p|^2 in the bounding-sphere test.  evalFac = 1 / pi (core-light.h:134-140).
// Experimental and disabled in the reference, no output to compare with: PARITY UNPINNED.
struct LtrBounds {
  V3 lo, hi, w;
  float cosTheta_o, cosTheta_e, phi;
  bool empty;
};
struct LtrNode {
  LtrBounds lb;
  float varPhi = 0.f;
  uint32_t numEmitters = 0, left = 0, light = 0;  // light: 0x80000000 | index for a leaf
  bool leaf() const { return (light & 0x80000000u) != 0u; }
};
inline float ltrSafeSqrt(float x) { return sqrtf(fmaxf(0.f, x)); }
inline float ltrSafeAcos(float x) { return acosf(fminf(fmaxf(x, -1.f), 1.f)); }
inline LtrBounds ltrEmpty() {
  LtrBounds b{};
  b.lo = v3(INFINITY, INFINITY, INFINITY), b.hi = v3(-INFINITY, -INFINITY, -INFINITY), b.empty = true;
  return b;
}
inline LtrBounds ltrFromLight(Rec32 const& L) {  // :149-187
  float const evalFac = 1.f / kPi;
  V3 const c = rdh3(L, L_INT);
  float const strength = 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z;
  V3 const co = rdf3(L, LP_POS);
  LtrBounds b{};
  if (rd16(L, L_TYPE) == LT_POINT) {
    float const r = fmaxf(h2f(rd16(L, LP_RAD)), 0.f);
    b.lo = co - v3(r, r, r), b.hi = co + v3(r, r, r);
    b.phi = 4.f * kPi * strength * evalFac;
    b.w = v3(0, 0, 1), b.cosTheta_o = -1.f, b.cosTheta_e = 0.f;
  } else {
    float const r = fmaxf(h2f(rd16(L, LS_RAD)), 0.f);
    float const cos0 = fminf(fmaxf(h2f(rd16(L, LS_COS0)), -1.f), 1.f), cosE = fminf(fmaxf(h2f(rd16(L, LS_COSE)), -1.f), 1.f);
    b.lo = co - v3(r, r, r), b.hi = co + v3(r, r, r);
    b.phi = 2.f * kPi * (1.f - cosE) * evalFac * strength;
    b.cosTheta_e = cosf(ltrSafeAcos(cosE) - ltrSafeAcos(cos0));
    b.w = dirFromOcta(rd32(L, LS_DIR));
    b.cosTheta_o = cos0;
  }
  return b;
}
inline void ltrConesUnion(V3 w0, float c0, V3 w1, float c1, V3* w, float* c) {  // :5-49
  float const t0 = ltrSafeAcos(c0), t1 = ltrSafeAcos(c1);
  float const td = ltrSafeAcos(dot(w0, w1));  // angleBetween of two unit vectors
  auto all = [](V3 v) { return v.x != 0.f && v.y != 0.f && v.z != 0.f; };
  if ((std::isnan(td) && !all(w1)) || fminf(td + t1, kPi) <= t0) {
    *w = w0, *c = c0;
    return;
  }
  if ((std::isnan(td) && !all(w0)) || fminf(td + t0, kPi) <= t1) {
    *w = w1, *c = c1;
    return;
  }
  float const tc = (t0 + td + t1) * 0.5f;
  V3 r = cross(w0, w1);
  float const rl2 = dot(r, r);
  if (tc >= kPi || !(rl2 > 0.f)) {
    *w = v3(0, 0, 1), *c = -1.f;
    return;
  }
  r = r * (1.f / sqrtf(rl2));
  float const a = tc - t0, ca = cosf(a), sa = sinf(a);  // rotation of w0 about r by a (fromRadians + rotate)
  V3 const rxw = cross(r, w0);
  float const rdw = dot(r, w0);
  V3 const v = w0 * ca + rxw * sa + r * (rdw * (1.f - ca));
  *w = v * (1.f / sqrtf(dot(v, v)));
  *c = cosf(tc);
}
inline LtrBounds ltrUnion(LtrBounds const& a, LtrBounds const& b) {  // :52-69
  if (a.empty) return b;
  if (b.empty) return a;
  LtrBounds u{};
  u.lo = v3(fminf(a.lo.x, b.lo.x), fminf(a.lo.y, b.lo.y), fminf(a.lo.z, b.lo.z));
  u.hi = v3(fmaxf(a.hi.x, b.hi.x), fmaxf(a.hi.y, b.hi.y), fmaxf(a.hi.z, b.hi.z));
  ltrConesUnion(a.w, a.cosTheta_o, b.w, b.cosTheta_o, &u.w, &u.cosTheta_o);
  u.cosTheta_e = fmaxf(a.cosTheta_e, b.cosTheta_e);
  u.phi = a.phi + b.phi;
  return u;
}
inline float ltrArea(LtrBounds const& b) {
  V3 const d = b.hi - b.lo;
  return 2.f * (d.x * d.y + d.x * d.z + d.y * d.z);
}
inline float ltrMomega(float cosTheta_e, float cosTheta_o) {  // :247-263
  float const theta_e = ltrSafeAcos(cosTheta_e), theta_o = ltrSafeAcos(cosTheta_o);
  float const theta_w = fminf(theta_o + theta_e, kPi);
  float const sinTheta_o = sinf(theta_o);
  float const cosTheta_diff = sinf(theta_o - 2.f * theta_w);
  return 2.f * kPi * (1.f - cosTheta_o) + (kPi / 2.f) * (2.f * theta_w * sinTheta_o - cosTheta_diff - 2.f * theta_o * sinTheta_o + cosTheta_o);
}
inline float ltrCosSub(float sa, float ca, float sb, float cb) { return ca > cb ? 1.f : ca * cb + sa * sb; }
inline float ltrSinSub(float sa, float ca, float sb, float cb) { return ca > cb ? 0.f : sa * cb - ca * sb; }
inline float ltrImportance(LtrBounds const& lb, V3 p, V3 n) {  // :98-146
  V3 const pc = (lb.lo + lb.hi) / 2.f;
  V3 const d = p - pc;
  float const len2 = dot(d, d);
  V3 const wi = d * (1.f / sqrtf(len2));
  float const sinTheta_o = ltrSafeSqrt(1.f - lb.cosTheta_o * lb.cosTheta_o);
  V3 const e = lb.hi - lb.lo;
  float const distSqr = fmaxf(len2, sqrtf(dot(e, e)) * 0.5f);
  float const cosTheta_w = dot(wi, lb.w);
  float const sinTheta_w = ltrSafeSqrt(1.f - cosTheta_w * cosTheta_w);
  V3 const h = lb.hi - pc;
  float const radius2 = dot(h, h);
  float sinTheta_b = 0.f, cosTheta_b = -1.f;
  if (!(len2 < radius2)) {
    float const s2 = radius2 / len2;
    sinTheta_b = sqrtf(s2), cosTheta_b = ltrSafeSqrt(1.f - s2);
  }
  float const cosTheta_wo = ltrCosSub(sinTheta_w, cosTheta_w, sinTheta_o, lb.cosTheta_o);
  float const sinTheta_wo = ltrSinSub(sinTheta_w, cosTheta_w, sinTheta_o, lb.cosTheta_o);
  float const cosTheta_p = ltrCosSub(sinTheta_wo, cosTheta_wo, sinTheta_b, cosTheta_b);
  if (cosTheta_p <= lb.cosTheta_e) return 0.f;
  float const cosTheta_i = fabsf(dot(wi, n));
  float const sinTheta_i = ltrSafeSqrt(1.f - cosTheta_i * cosTheta_i);
  float const cosTheta_ib = ltrCosSub(sinTheta_i, cosTheta_i, sinTheta_b, cosTheta_b);
  return fmaxf(lb.phi * cosTheta_ib * cosTheta_p / distSqr, 0.f);
}
inline float ltrSplitHeuristic(LtrNode const& nd, V3 p) {  // :190-232
  if (nd.leaf()) return 1.f;
  V3 const pc = (nd.lb.lo + nd.lb.hi) / 2.f;
  V3 const d = p - pc, e = nd.lb.hi - nd.lb.lo;
  float const halfDiag = sqrtf(dot(e, e)) * 0.5f;
  float const dist = ltrSafeSqrt(fmaxf(dot(d, d), halfDiag));
  float const a = fmaxf(dist - halfDiag, 0.f), b = dist + halfDiag;
  float gExpected2 = 0.f, gVariance = 0.f;
  if (a > 0.f && b > 0.f) {
    float const a3 = a * a * a, b3 = b * b * b;
    float const a_minus_b = a - b;
    float const a3_minus_b3 = a_minus_b * (a * a + a * b + b * b);
    float const r = 1.f / (a * b);
    gExpected2 = r * r;
    gVariance = a3_minus_b3 / (3.f * a_minus_b * a3 * b3) - gExpected2;
  }
  float const n = float(nd.numEmitters);
  float const eMean = nd.lb.phi / n;
  float const eExpected2 = eMean * eMean, eVariance = nd.varPhi;
  float const sigma2 = (eVariance * gVariance + eVariance * gExpected2 + eExpected2 * gVariance) * (n * n);
  return sqrtf(sqrtf(fmaxf(1.f / (1.f + sqrtf(sigma2)), 0.f)));
}
inline std::vector<LtrNode> ltrBuild(Rec32 const* lights, uint32_t count) {  // :305-446
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < count; ++i)
    if (rd16(lights[i], L_TYPE) == LT_POINT || rd16(lights[i], L_TYPE) == LT_SPOT) order.push_back(i);
  std::vector<LtrNode> nodes;
  if (order.empty()) return nodes;
  auto rangeBounds = [&](size_t a, size_t b) {
    LtrBounds lb = ltrEmpty();
    for (size_t i = a; i < b; ++i) lb = ltrUnion(lb, ltrFromLight(lights[order[i]]));
    return lb;
  };
  struct Work {
    uint32_t node;
    size_t a, b;
    LtrBounds lb;
  };
  nodes.emplace_back();
  std::vector<Work> stack{{0u, 0, order.size(), rangeBounds(0, order.size())}};
  while (!stack.empty()) {
    Work const w = stack.back();
    stack.pop_back();
    nodes[w.node].lb = w.lb;
    size_t const n = w.b - w.a;
    nodes[w.node].numEmitters = uint32_t(n);
    if (n == 1) {
      nodes[w.node].light = 0x80000000u | order[w.a];
      continue;
    }
    V3 const d = w.lb.hi - w.lb.lo;
    int const axis = (d.x > d.y && d.x > d.z) ? 0 : (d.y > d.z ? 1 : 2);
    auto comp = [axis](V3 v) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); };
    float const splitLen = comp(d) / 32.f;
    float const Kr = fmaxf(d.x, fmaxf(d.y, d.z)) / comp(d);
    float const Ma = ltrArea(w.lb), Mo = ltrMomega(w.lb.cosTheta_e, w.lb.cosTheta_o);
    LtrBounds bestL = ltrEmpty(), bestR = ltrEmpty();
    float minSplitPos = 0.f, minCost = INFINITY;
    bool found = false;
    for (int i = 1; i < 31; ++i) {
      float const splitPos = comp(w.lb.lo) + float(i) * splitLen;
      LtrBounds L = ltrEmpty(), R = ltrEmpty();
      for (size_t k = w.a; k < w.b; ++k) {
        Rec32 const& light = lights[order[k]];
        if (comp(rdf3(light, LP_POS)) < splitPos) L = ltrUnion(L, ltrFromLight(light));
        else R = ltrUnion(R, ltrFromLight(light));
      }
      if (L.empty || R.empty) continue;
      float const cost = Kr * (L.phi * ltrArea(L) * ltrMomega(L.cosTheta_e, L.cosTheta_o) + R.phi * ltrArea(R) * ltrMomega(R.cosTheta_e, R.cosTheta_o)) / (Ma * Mo);
      if (cost < minCost) minCost = cost, minSplitPos = splitPos, bestL = L, bestR = R, found = true;
    }
    size_t mid;
    if (found) {
      mid = size_t(std::stable_partition(order.begin() + long(w.a), order.begin() + long(w.b),
                                         [&](uint32_t li) { return comp(rdf3(lights[li], LP_POS)) < minSplitPos; }) - order.begin());
    } else {
      mid = w.a + n / 2;
      bestL = rangeBounds(w.a, mid), bestR = rangeBounds(mid, w.b);
    }
    uint32_t const left = uint32_t(nodes.size());
    nodes.emplace_back(), nodes.emplace_back();
    nodes[w.node].left = left;
    stack.push_back({left + 1u, mid, w.b, bestR});
    stack.push_back({left, w.a, mid, bestL});
  }
  for (size_t i = 0; i < nodes.size(); ++i) {  // :394-426
    if (nodes[i].leaf()) continue;
    std::vector<float> phis;
    std::vector<uint32_t> st{uint32_t(i)};
    while (!st.empty()) {
      uint32_t const at = st.back();
      st.pop_back();
      if (nodes[at].leaf()) {
        phis.push_back(nodes[at].lb.phi);
        continue;
      }
      st.push_back(nodes[at].left + 1u), st.push_back(nodes[at].left);
    }
    float mean = 0.f, var = 0.f;
    for (float f : phis) mean += f;
    mean /= float(phis.size());
    for (float f : phis) var += (f - mean) * (f - mean);
    nodes[i].varPhi = var / float(phis.size() - 1);
  }
  return nodes;
}
struct LtrSelection {
  uint32_t indices[4];
  float pmfs[4];
  uint32_t count = 0;
};
inline LtrSelection ltrSelect(LtrNode const* nodes, V3 p, V3 n, float u, float startPMF, float precision = 0.5f) {
  // lightTreeAdaptiveSplit :448-491
  std::vector<uint32_t> cut;
  if (nodes[0].leaf()) {
    cut.push_back(0u);
  } else {
    std::vector<uint32_t> parentStack, siblingStack{0u};
    while ((!siblingStack.empty() || !parentStack.empty()) && cut.size() < 4) {
      if (!siblingStack.empty()) {
        uint32_t const sibling = siblingStack.back();
        siblingStack.pop_back();
        bool const enough = ltrSplitHeuristic(nodes[sibling], p) >= precision;
        if (cut.size() + 1 == 4 || enough) cut.push_back(sibling);
        else if (!nodes[sibling].leaf()) parentStack.push_back(sibling);
      } else {
        uint32_t const parent = parentStack.back();
        parentStack.pop_back();
        siblingStack.push_back(nodes[parent].left), siblingStack.push_back(nodes[parent].left + 1u);
      }
    }
  }
  // selectLightsFromSplit :493-539
  LtrSelection sel;
  uint32_t moreLights = uint32_t(cut.size()), splitIndex = 0;
  while (sel.count < cut.size() && moreLights && splitIndex < cut.size()) {
    uint32_t at = cut[splitIndex++];
    float pmf = startPMF;
    bool pathSampled = false;
    while (!pathSampled) {
      LtrNode const& nd = nodes[at];
      if (!nd.leaf()) {
        float const w[2] = {ltrImportance(nodes[nd.left].lb, p, n), ltrImportance(nodes[nd.left + 1u].lb, p, n)};
        if (w[0] == 0.f && w[1] == 0.f) {
          pathSampled = true;
        } else {  // sampleDiscrete, core-math.cu:366-392
          float const sumWeights = w[0] + w[1];
          float up = u * sumWeights;
          if (up == sumWeights) up = nextafterf(up, -INFINITY);
          int offset = 0;
          float sum = 0.f;
          while (offset < 1 && sum + w[offset] <= up) sum += w[offset], ++offset;
          pmf *= w[offset] / sumWeights;
          u = fminf((up - sum) / w[offset], 0.99999994f);
          at = nd.left + uint32_t(offset);
        }
      } else {
        pathSampled = true;
        --moreLights;
        if (ltrImportance(nd.lb, p, n) > 0.f) {
          sel.indices[sel.count] = nd.light & 0x7FFFFFFFu;
          sel.pmfs[sel.count] = pmf;
          ++sel.count;
        }
      }
    }
  }
  return sel;
}

// ---- image textures ------------------------------------------------------------------------------
// One texel: mirror wrap (the only mode the reference's material code asks for, core-material.cpp:114-116), byte / 255
// (core-texture.cu readRGB of ByteRGB).  core-texture.cu:895-915.
inline V3 texel(Scene const& sc, int32_t tex, int s, int t) {
  int32_t const* d = sc.texDesc + 3 * tex;
  auto mirror = [](int c, int size) {
    int const p = size * 2;
    c %= p;
    if (c < 0) c += p;
    return c < size ? c : (p - c - 1);
  };
  uint8_t const* px = sc.texRgba + 4 * (size_t(d[0]) + size_t(mirror(t, d[2])) * size_t(d[1]) + size_t(mirror(s, d[1])));
  return v3(float(px[0]) / 255.f, float(px[1]) / 255.f, float(px[2]) / 255.f);
}
// sampleBilinearTexel at MIP level 0, core-material.cpp:20-56 (the megakernel path carries no ray differentials; the
// reference's isotropic fallback selects level 0 whenever its differentials are near zero, :104-116)
inline V3 textureBilinear(Scene const& sc, int32_t tex, float s, float t, bool isNormal) {
  int32_t const* d = sc.texDesc + 3 * tex;
  float const x = s * float(d[1]) - 0.5f, y = t * float(d[2]) - 0.5f;
  int const x0 = int(floorf(x)), y0 = int(floorf(y));
  float const tx = x - float(x0), ty = y - float(y0);
  V3 const c00 = texel(sc, tex, x0, y0), c10 = texel(sc, tex, x0 + 1, y0), c01 = texel(sc, tex, x0, y0 + 1),
           c11 = texel(sc, tex, x0 + 1, y0 + 1);
  auto lerpc = [](V3 a, V3 b, float w) { return a * (1.f - w) + b * w; };
  V3 c = lerpc(lerpc(c00, c10, tx), lerpc(c01, c11, tx), ty);
  if (isNormal) c.x = c.x * 2.f - 1.f, c.y = c.y * 2.f - 1.f;  // z stays as stored (:49-52)
  return c;
}
// Applies the material's textures at a hit: patches the packed record the way the host packers build it
// (makeOrenNayar / bsdfGGXCommon above) from the sampled albedo / roughness, and returns the shading normal.
// metallic fraction of a BS_GGX_BLEND material at a hit: the record's constant, or the material's 1-channel metallic map
// (core-material.cpp:209-216; its index sits in the FIRST texture slot of the pair's second row, which a conductor
// record has no other use for)
inline float blendMetallic(Scene const& sc, Rec32 const& rec, uint32_t matId, int tri, float bu, float bv) {
  float m = h2f(rd16(rec, B_WEIGHT));
  if (sc.matTex && sc.triUv) {
    int32_t const texM = int32_t(sc.matTex[4 * (matId + 1)]);
    if (texM >= 0) {
      float const* uv = sc.triUv + 6 * size_t(tri);
      float const w0 = 1.f - bu - bv;
      float const s = w0 * uv[0] + bu * uv[2] + bv * uv[4], t = w0 * uv[1] + bu * uv[3] + bv * uv[5];
      m = textureBilinear(sc, texM, s, t, false).x;
    }
  }
  return m;
}
// lookupUlps (probes only): every texture lookup is moved by that many fp32 ulps before it is quantised, which is how far a
// differently rounded bilinear filter lands from this one -- oracle_material_at_hit finds the hits on a quantisation boundary with it
inline V3 applyMaterialTextures(Scene const& sc, Rec32& rec, uint32_t matId, int tri, float bu, float bv, V3 ng, int lookupUlps = 0) {
  if (!sc.matTex || !sc.triUv) return ng;
  auto textureBilinear = [lookupUlps](Scene const& scn, int32_t tex, float ss, float tt, bool isNormal) {
    V3 c = ::textureBilinear(scn, tex, ss, tt, isNormal);
    float const to = lookupUlps > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
    for (int k = 0; k < std::abs(lookupUlps); ++k) c = v3(nextafterf(c.x, to), nextafterf(c.y, to), nextafterf(c.z, to));
    return c;
  };
  uint32_t const* m = sc.matTex + 4 * matId;
  int32_t const texD = int32_t(m[0]), texR = int32_t(m[1]), texN = int32_t(m[2]);
  if (texD < 0 && texR < 0 && texN < 0) return ng;
  float aniso;
  memcpy(&aniso, &m[3], 4);
  float const* uv = sc.triUv + 6 * size_t(tri);
  float const w0 = 1.f - bu - bv;
  float const s = w0 * uv[0] + bu * uv[2] + bv * uv[4], t = w0 * uv[1] + bu * uv[3] + bv * uv[5];
  uint16_t const type = bsdfType(rec);
  if (texD >= 0 && type == BS_OREN) {
    V3 const c = textureBilinear(sc, texD, s, t, false);
    wrh3(rec, B_WEIGHT, v3(fmaxf(0, fminf(c.x, 1)), fmaxf(0, fminf(c.y, 1)), fmaxf(0, fminf(c.z, 1))));
  }
  if (texR >= 0) {
    float const rough = fmaxf(0.f, fminf(textureBilinear(sc, texR, s, t, false).x, 1.f));
    if (type == BS_OREN) {
      float const k = (kPi / 2.f) - 2.f / 3.f;
      wr16(rec, ON_ROUGH, f2h(fmaxf(0, fminf(rough, kPi / 2.f))));
      float const sigma = h2f(rd16(rec, ON_ROUGH));
      wr16(rec, ON_A, f2h(1.f / (kPi + k * sigma)));
      float const a = h2f(rd16(rec, ON_A));
      wr16(rec, ON_B, f2h(a * sigma));
    } else if (type == BS_GGX_DIEL || type == BS_GGX_COND) {  // alpha_y = roughness, alpha_x = anisotropy * roughness (:262-263)
      float const U16 = 65535.f;
      wr16(rec, G_AX, uint16_t(fminf(fmaxf(aniso * rough * U16, 0.f), U16)));
      wr16(rec, G_AY, uint16_t(fminf(fmaxf(rough * U16, 0.f), U16)));
    }
  }
  if (texN < 0) return ng;
  // core-material.cpp:188-200: sample, quantise to 10 bits and normalise, rotate out of Frame::fromZ(ng)
  V3 n = textureBilinear(sc, texN, s, t, true);
  auto quant = [](float v) { return float(int(v * 1023.f + 0.5f)) / 1023.f; };  // fl::quantize, cudautils-float.cuh:357-361
  n = normalize(v3(quant(n.x), quant(n.y), quant(n.z)));
  V3 tx, ty;
  gramSchmidt(ng, &tx, &ty);
  V3 const ns = tx * n.x + ty * n.y + ng * n.z;
  float const l2 = length2(ns);
  return (l2 > 0.f && std::isfinite(l2)) ? ns / sqrtf(l2) : ng;  // safeNormalizeFallback
}

struct PathLog {  // optional per-bounce record sink: {tri, pos3, beta3, L3, depth, dim} = 12 floats
  float* rec = nullptr;
  int cap = 0, n = 0;
  void push(int tri, V3 pos, V3 beta, V3 L, int depth, int dim) {
    if (!rec || n >= cap) return;
    float* r = rec + 12 * n++;
    r[0] = float(tri), r[1] = pos.x, r[2] = pos.y, r[3] = pos.z, r[4] = beta.x, r[5] = beta.y, r[6] = beta.z;
    r[7] = L.x, r[8] = L.y, r[9] = L.z, r[10] = float(depth), r[11] = float(dim);
  }
};

V3 tracePath(Scene const& sc, RenderCfg const& cfg, int px, int py, int s, Stats* st,
             PathLog* log = nullptr) {
  Sampler rng;
  rng.startPixelSample(cfg.hp, px, py, s);
  Rec32 bsdf{};
  int depth = 0;
  int transmissionCount = 0;
  bool lastBounceTransmission = false;
  V3 L = v3(0, 0, 0);
  V3 beta = v3(1, 1, 1);
  float lastBsdfPdf = 1.f;      // env map only: pdf / delta flag of the bounce that produced the current ray
  bool specularBounce = false;  // (core-render.cpp:139-143)
  Ray ray = cameraRay(cameraSampleFilm(px, py, rng, cfg.hp), cfg.cameraFromRaster,
                      cfg.renderFromCamera);
  if (st) st->samples++;
  while (true) {
    Hit hit;
    int hitTri = -1;
    if (st) st->closestRays++, st->triTests += sc.triCount;
    for (uint64_t tri = 0; tri < sc.triCount; ++tri) {
      Hit const r = triangleIntersect(sc.xs + 4 * tri, sc.ys + 4 * tri, sc.zs + 4 * tri, ray);
      if (r.hit && r.t < hit.t) {
        hit = r;
        hitTri = int(tri);
        hit.matId = sc.matId[tri];
        if (dot(ray.d, hit.normal) > 0) hit.normal *= -1.f;
      }
    }
    if (log) log->push(hitTri, hit.pos, beta, L, depth, rng.dimension);
    if (!hit.hit && sc.env) {  // A18: env map seen by a path ray, MIS against NEE (core-render.cpp:154-163)
      float pdfLight = 0.f;
      V3 const Le = envEvalDir(*sc.env, ray.d, &pdfLight);
      if (depth == 0 || specularBounce)
        L += beta * Le;
      else
        L += beta * (lastBsdfPdf / (lastBsdfPdf + pdfLight)) * Le;
      break;
    }
    if (!hit.hit) {
      if (sc.infLightCount > 0) {  // (reference reads out of bounds when the list is empty)
        uint32_t const li = pickIndex(rng.get1D(), sc.infLightCount);
        float const lightPMF = 1.f / sc.infLightCount;
        float pdf = 0;
        V3 const Le = evalInfiniteLight(sc.infLights[li], ray.d, &pdf);
        if (pdf) L += beta * Le / lightPMF;
      }
      break;
    }
    if (sc.areaCount > 0 && sc.areaOf[hitTri] != 0xFFFFFFFFu) {  // emitted radiance of the surface the path ray hit
      float const pl = areaPdf(sc, uint32_t(hitTri), ray.d, hit.t);
      if (pl > 0.f) {
        V3 const Le = v3(sc.areaLe[3 * sc.areaOf[hitTri]], sc.areaLe[3 * sc.areaOf[hitTri] + 1], sc.areaLe[3 * sc.areaOf[hitTri] + 2]);
        if (depth == 0 || specularBounce) {
          L += beta * Le;
        } else {
          float const a = lastBsdfPdf, b = pl * (sc.env ? 0.5f : 1.f) / float(sc.lightCount + sc.areaCount);
          L += beta * Le * ((a * a) / (a * a + b * b));
        }
      }
    }
    if (depth >= cfg.maxDepth) break;
    if (st) st->bounces++, st->hits++;
    bsdf = sc.bsdfs[hit.matId];
    // fractional "metallic" (BS_GGX_BLEND): both lobes of the material are prepared, evaluated and sampled, and blended
    // as the reference's CPU renderer does (core-material.cpp:275-286, :383-394)
    Rec32 bsdf2{};
    float mix = 0.f;
    bool blend = false;
    if (bsdfType(bsdf) == BS_GGX_BLEND) {
      mix = blendMetallic(sc, bsdf, hit.matId, hitTri, hit.u, hit.v);
      wr16(bsdf, B_TYPE, BS_GGX_DIEL);
      bsdf2 = sc.bsdfs[hit.matId + 1];
      if (mix >= 1.f) bsdf = bsdf2;                       // :273  metallic >= 1: the conductor alone
      else blend = mix > 0.f;                             // :272  metallic <= 0: the dielectric alone
    }
    V3 const ns = applyMaterialTextures(sc, bsdf, hit.matId, hitTri, hit.u, hit.v, hit.normal);  // = hit.normal without textures
    prepareBSDF(&bsdf, ns, -ray.d, transmissionCount);
    if (blend) {
      (void)applyMaterialTextures(sc, bsdf2, hit.matId + 1, hitTri, hit.u, hit.v, hit.normal);  // same roughness map, same normal
      prepareBSDF(&bsdf2, ns, -ray.d, transmissionCount);
    }
    // f * weight and pdf of the material towards wi.  Blend: result.f = lerp(fD, fC, metallic) with the RGB overload
    // (a, b, t) of cudautils-color.cuh:112-114; result.pdf = lerp(pdfD, pdfC, metallic) resolves to the FLOAT overload
    // dmt::lerp(float x, float a, float b) = (1 - x) a + x b (cudautils-vecmath.cuh:750-752), whose first argument is the
    // parameter: the reference computes (1 - pdfD) pdfC + pdfD metallic.  Kept as written (it decides pixels); the same
    // expression serves the sampling side (core-material.cpp:282).
    auto blendPdf = [&](float pdfD, float pdfC) { return (1.f - pdfD) * pdfC + pdfD * mix; };
    auto evalMaterial = [&](V3 wo, V3 wi, float* pdf) {
      V3 f = evalBsdf(bsdf, wo, wi, ns, hit.normal, pdf) * bsdfWeight(bsdf);
      if (blend) {
        float pdfC = 0;
        V3 const fC = evalBsdf(bsdf2, wo, wi, ns, hit.normal, &pdfC) * bsdfWeight(bsdf2);
        f = f * (1.f - mix) + fC * mix;
        *pdf = blendPdf(*pdf, pdfC);
      }
      return f;
    };

    float uLight = rng.get1D();
    V2 const uLight2 = rng.get2D();
    bool envNee = false;
    if (sc.env) {  // A18: env map with probability 1/2, the light list otherwise (core-render.cpp:290-299)
      envNee = uLight < 0.5f;
      uLight = envNee ? uLight : (uLight - 0.5f) * 2.f;
    }
    bool areaNee = false;
    uint32_t areaIdx = 0;
    float const listPmfScale = sc.env ? 0.5f : 1.f;  // the env map takes half of the NEE samples when present
    if (sc.areaCount > 0 && !envNee) {  // uniform choice among point/spot lights and emissive triangles
      uint32_t const li = pickIndex(uLight, sc.lightCount + sc.areaCount);
      areaNee = li >= sc.lightCount;
      areaIdx = areaNee ? li - sc.lightCount : 0u;
    }
    if (areaNee) {
      uint32_t const tri = sc.areaTri[areaIdx];
      AreaSample const as = areaSample(sc, tri, hit.pos, uLight2);
      if (as.ok) {
        Ray const shadow{offsetRayOrigin(hit.pos, hit.error, hit.normal, as.wi), as.wi};
        float const smax = as.dist * 0.999f;
        bool visible = true;
        if (st) st->shadowRays++;
        for (uint64_t t2 = 0; t2 < sc.triCount; ++t2) {
          if (st) st->triTests++;
          Hit const r = triangleIntersect(sc.xs + 4 * t2, sc.ys + 4 * t2, sc.zs + 4 * t2, shadow);
          if (r.hit && r.t < smax) {
            visible = false;
            break;
          }
        }
        if (visible) {
          float bsdfPdf = 0;
          V3 const f = evalMaterial(-ray.d, shadow.d, &bsdfPdf);
          if (!isZero(f)) {
            V3 const Le = v3(sc.areaLe[3 * areaIdx], sc.areaLe[3 * areaIdx + 1], sc.areaLe[3 * areaIdx + 2]);
            float const a = as.pdf * listPmfScale / float(sc.lightCount + sc.areaCount), b = bsdfPdf;
            L += beta * (Le * f * (((a * a) / (a * a + b * b)) / a));
          }
        }
      }
    } else if (envNee) {
      EnvSample const es = envSample(*sc.env, uLight2);
      if (es.ok) {
        Ray const shadow{offsetRayOrigin(hit.pos, hit.error, hit.normal, es.wi), es.wi};
        bool visible = true;
        if (st) st->shadowRays++;
        for (uint64_t tri = 0; tri < sc.triCount; ++tri) {
          if (st) st->triTests++;
          if (triangleIntersect(sc.xs + 4 * tri, sc.ys + 4 * tri, sc.zs + 4 * tri, shadow).hit) {
            visible = false;
            break;
          }
        }
        if (visible) {
          float bsdfPdf = 0;
          V3 const f = evalMaterial(-ray.d, shadow.d, &bsdfPdf);
          V3 const Le = envEvalUv(*sc.env, es.uv);
          // core-render.cpp:357-369: Le f / (pdfLight pmf + pdfBsdf), pmf = 1/2
          if (!isZero(f) && maxComponent(Le) > 0.f) L += beta * (Le * f / (es.pdf * 0.5f + bsdfPdf));
        }
      }
    } else if (sc.lightTreeRef && sc.lightCount > 1 && sc.areaCount == 0 && !sc.matTex) {
      // lightSampling == 2: a cut of up to four tree nodes, one light drawn below each, one shadow ray per light
      // (core-render.cpp:296-370); the contribution of each light is this path's own NEE term with the light's pmf
      LtrSelection const sel = ltrSelect(sc.lightTreeRef, hit.pos, hit.normal, uLight, sc.env ? 0.5f : 1.f);
      for (uint32_t i = 0; i < sel.count; ++i) {
        Rec32 const& light = sc.lights[sel.indices[i]];
        float const lightPMF = sel.pmfs[i];
        LightSample const ls = sampleLight(light, hit.pos, uLight2, lastBounceTransmission, hit.normal);
        if (!ls.valid()) continue;
        Ray const shadow{offsetRayOrigin(hit.pos, hit.error, hit.normal, ls.direction), ls.direction};
        bool doNEE = true;
        if (st) st->shadowRays++;
        for (uint64_t tri = 0; tri < sc.triCount; ++tri) {
          if (st) st->triTests++;
          Hit const r = triangleIntersect(sc.xs + 4 * tri, sc.ys + 4 * tri, sc.zs + 4 * tri, shadow);
          if (r.hit && r.t < ls.distance) {
            doNEE = false;
            break;
          }
        }
        if (!doNEE) continue;
        float bsdfPdf = 0;
        V3 const f = evalMaterial(-ray.d, shadow.d, &bsdfPdf);
        V3 const Le = evalLight(light, ls);
        if (isZero(f)) continue;
        if (ls.delta) {
          L += beta * Le * f / lightPMF;
        } else {
          float const w = sqrf(lightPMF * ls.pdf) / sqrf(lightPMF * ls.pdf + bsdfPdf);
          L += Le * f * beta * w;
        }
      }
    } else if (sc.lightCount > 0) {
      uint32_t li = sc.areaCount > 0 ? pickIndex(uLight, sc.lightCount + sc.areaCount) : pickIndex(uLight, sc.lightCount);
      float lightPMF = (sc.env ? 0.5f : 1.f) / float(sc.lightCount + sc.areaCount);
      bool picked = true;
      if (sc.lightTree && sc.lightCount > 1 && sc.areaCount == 0 && !sc.matTex) {  // same applicability rule as the product
        float treePmf = 0.f;
        int const sel = ltSelect(sc.lightTree, hit.pos, hit.normal, uLight, &treePmf);
        picked = sel >= 0;
        li = picked ? uint32_t(sel) : 0u;
        lightPMF = (sc.env ? 0.5f : 1.f) * treePmf;
      }
      Rec32 const& light = sc.lights[li];
      LightSample const ls = sampleLight(light, hit.pos, uLight2, lastBounceTransmission, hit.normal);
      if (picked && ls.valid()) {
        Ray const shadow{offsetRayOrigin(hit.pos, hit.error, hit.normal, ls.direction), ls.direction};
        bool doNEE = true;
        if (st) st->shadowRays++;
        for (uint64_t tri = 0; tri < sc.triCount; ++tri) {
          if (st) st->triTests++;
          Hit const r = triangleIntersect(sc.xs + 4 * tri, sc.ys + 4 * tri, sc.zs + 4 * tri, shadow);
          if (r.hit && r.t < ls.distance) {
            doNEE = false;
            break;
          }
        }
        if (doNEE) {
          float bsdfPdf = 0;
          V3 const f = evalMaterial(-ray.d, shadow.d, &bsdfPdf);
          V3 const Le = evalLight(light, ls);
          if (!isZero(f)) {
            if (ls.delta) {
              L += beta * Le * f / lightPMF;
            } else {
              float const w = sqrf(lightPMF * ls.pdf) / sqrf(lightPMF * ls.pdf + bsdfPdf);
              L += Le * f * beta * w;
            }
          }
        }
      }
    }
    V2 u2;
    float uc;
    if (cfg.rtlArgs) {
      uc = rng.get1D();
      u2 = rng.get2D();
    } else {
      u2 = rng.get2D();
      uc = rng.get1D();
    }
    BSDFSample bs = sampleBsdf(bsdf, -ray.d, ns, hit.normal, u2, uc);
    if (blend) {  // core-material.cpp:275-286: both lobes sampled with the same numbers; direction and flags of the conductor's
      BSDFSample sC = sampleBsdf(bsdf2, -ray.d, ns, hit.normal, u2, uc);
      sC.f = bs.f * (1.f - mix) + sC.f * mix;
      sC.pdf = blendPdf(bs.pdf, sC.pdf);
      sC.eta = 1.f;
      bs = sC;
    }
    if (!bs.valid()) break;
    transmissionCount += bs.refract;
    lastBounceTransmission = bs.refract;
    lastBsdfPdf = bs.pdf, specularBounce = bs.delta;
    ray.o = offsetRayOrigin(hit.pos, hit.error, hit.normal, bs.wi);
    ray.d = bs.wi;
    beta *= bs.f * fabsf(dot(bs.wi, hit.normal)) / bs.pdf;
    float const rrBeta = maxComponent(beta * bs.eta);
    if (rrBeta < 1 && depth > 1) {
      float const q = fmaxf(0.f, 1.f - rrBeta);
      if (rng.get1D() < q) break;
      beta /= 1 - q;
    }
    ++depth;
  }
  return L;
}

// Welford running mean / M2 per pixel           T/megakernel/megakernel.cuh:45-85
void renderPixel(Scene const& sc, RenderCfg const& cfg, int px, int py, int sampleOffset, int spp,
                 float* mean4, float* m24, Stats* st) {
  size_t const idx = size_t(px) + size_t(py) * size_t(cfg.width);
  V3 mean = v3(mean4[4 * idx + 0], mean4[4 * idx + 1], mean4[4 * idx + 2]);
  V3 M2 = v3(m24[4 * idx + 0], m24[4 * idx + 1], m24[4 * idx + 2]);
  float N = m24[4 * idx + 3];
  for (int sb = 0; sb < spp; ++sb) {
    V3 const L = tracePath(sc, cfg, px, py, sb + sampleOffset, st);
    float const num = ++N;
    V3 const delta = L - mean;
    mean += delta / num;
    V3 const delta2 = L - mean;
    M2 += delta * delta2;
  }
  mean4[4 * idx + 0] = mean.x, mean4[4 * idx + 1] = mean.y, mean4[4 * idx + 2] = mean.z;
  mean4[4 * idx + 3] = 0.f;
  m24[4 * idx + 0] = M2.x, m24[4 * idx + 1] = M2.y, m24[4 * idx + 2] = M2.z;
  m24[4 * idx + 3] = N;
}

RenderCfg makeCfg(Camera const& cam, int maxDepth, int rtl) {
  RenderCfg cfg;
  cfg.hp = computeParams(cam.width, cam.height);
  cfg.cameraFromRaster = cameraFromRasterPerspective(cam.focalLength, cam.sensorSize,
                                                     uint32_t(cam.width), uint32_t(cam.height));
  cfg.renderFromCamera = worldFromCamera(v3(cam.dir[0], cam.dir[1], cam.dir[2]),
                                         v3(cam.pos[0], cam.pos[1], cam.pos[2]));
  cfg.width = cam.width;
  cfg.height = cam.height;
  cfg.maxDepth = maxDepth;
  cfg.rtlArgs = rtl != 0;
  return cfg;
}

// ------------------------------------------------------------------------------------
// hard-coded scene                CC/private/host_scene.cu:7-119, CC/private/host_utils.cu:402-469
// ------------------------------------------------------------------------------------
struct Tri {
  V3 v0, v1, v2;
};
std::vector<Tri> generateSphereMesh(V3 c, float radius, int lat, int lon) {
  std::vector<Tri> out;
  V3 const top = c + v3(0, radius, 0);
  V3 const bottom = c + v3(0, -radius, 0);
  for (int i = 0; i < lat; ++i) {
    float const th0 = kPi * float(i) / lat;
    float const th1 = kPi * float(i + 1) / lat;
    float const y0 = radius * cosf(th0), y1 = radius * cosf(th1);
    float const r0 = radius * sinf(th0), r1 = radius * sinf(th1);
    for (int j = 0; j < lon; ++j) {
      float const ph0 = 2.f * kPi * float(j) / lon;
      float const ph1 = 2.f * kPi * float((j + 1) % lon) / lon;
      V3 const p00 = c + v3(r0 * cosf(ph0), y0, r0 * sinf(ph0));
      V3 const p01 = c + v3(r0 * cosf(ph1), y0, r0 * sinf(ph1));
      V3 const p10 = c + v3(r1 * cosf(ph0), y1, r1 * sinf(ph0));
      V3 const p11 = c + v3(r1 * cosf(ph1), y1, r1 * sinf(ph1));
      if (i == 0) {
        out.push_back({top, p10, p11});
      } else if (i == lat - 1) {
        out.push_back({p00, bottom, p01});
      } else {
        out.push_back({p00, p10, p01});
        out.push_back({p01, p10, p11});
      }
    }
  }
  return out;
}
std::vector<Tri> generatePlane(V3 center, V3 normal, float width, float height) {
  V3 const n = normalize(normal);
  V3 major;
  if (fabs(n.x) <= fabs(n.y) && fabs(n.x) <= fabs(n.z))
    major = v3(1, 0, 0);
  else if (fabs(n.y) <= fabs(n.x) && fabs(n.y) <= fabs(n.z))
    major = v3(0, 1, 0);
  else
    major = v3(0, 0, 1);
  V3 tangent = normalize(cross(major, n));
  V3 bitangent = cross(n, tangent);
  tangent *= width * 0.5f;
  bitangent *= height * 0.5f;
  V3 const p0 = center - tangent - bitangent;
  V3 const p1 = center + tangent - bitangent;
  V3 const p2 = center + tangent + bitangent;
  V3 const p3 = center - tangent + bitangent;
  return {Tri{p0, p2, p1}, Tri{p0, p3, p2}};
}

struct HostScene {
  std::vector<float> xs, ys, zs;
  std::vector<uint32_t> matId;
  std::vector<Rec32> bsdfs, lights, infLights;
  Camera cam;
};
HostScene cornellBox() {
  HostScene h;
  std::vector<Tri> tris;
  std::vector<uint32_t> nextMesh, meshMat;
  auto add = [&](std::vector<Tri> const& mesh, uint32_t mat) {
    tris.insert(tris.end(), mesh.begin(), mesh.end());
    nextMesh.push_back(uint32_t((nextMesh.empty() ? 0 : nextMesh.back()) + mesh.size()));
    meshMat.push_back(mat);
  };
  V3 const white = v3(0.9f, 170.f / 204.f, 160.f / 204.f);
  add(generateSphereMesh(v3(-1.2, 2, -0.25), 0.5f, 2, 4), 0);
  h.bsdfs.push_back(makeOrenNayar(v3(1.f, .7f, .3f), .7f));
  add(generateSphereMesh(v3(1.2, 2.4, -0.25), 0.5f, 2, 4), 1);
  h.bsdfs.push_back(makeGGXDielectric(v3(0.02f, 0.07f, 0.01f), v3(0.95f, 0.95f, 0.87f), 1.f, 1.44f,
                                      .5f, .7f));
  add(generatePlane(v3(0, 4, 0), v3(0, -1, 0), 4, 4), 2);
  h.bsdfs.push_back(makeOrenNayar(white, .5f));
  add(generatePlane(v3(0, 2, -.5f), v3(0, 0, 1), 4, 4), 3);
  h.bsdfs.push_back(makeOrenNayar(v3(1.f, .7f, .3f), .7f));
  add(generatePlane(v3(0, 2, 2), v3(0, 0, -1), 4, 4), 4);
  h.bsdfs.push_back(makeOrenNayar(white, .5f));
  add(generatePlane(v3(-2, 2, 0), v3(1, 0, 0), 4, 4), 5);
  h.bsdfs.push_back(makeOrenNayar(v3(1.f, 0.01f, 0.01f), .6f));
  add(generatePlane(v3(2, 2, 0), v3(-1, 0, 0), 4, 4), 6);
  h.bsdfs.push_back(makeOrenNayar(v3(0.01f, 1.f, 0.01f), .6f));
  h.lights.push_back(makeSpotLight(2.f * v3(1, 1, 1), v3(0, 1.8f, 1.7f), v3(0, 0, -1),
                                   cosf(kPi / 6), cosf(kPi / 3), 0.01f));
  h.infLights.push_back(makeEnvLight(v3(0.1f, 0.1f, 0.1f)));

  // SoA flatten with the material walk of host_utils.cu:139-172
  size_t const n = tris.size();
  h.xs.resize(4 * n), h.ys.resize(4 * n), h.zs.resize(4 * n), h.matId.resize(n);
  uint32_t matIdx = 0, meshIdx = 0, nextInc = nextMesh[0];
  for (size_t i = 0; i < n; ++i) {
    if (meshIdx + 1 < nextMesh.size() && i >= nextInc) {
      ++meshIdx;
      nextInc = nextMesh[meshIdx];
      matIdx = meshMat[meshIdx];
    }
    Tri const& t = tris[i];
    h.xs[4 * i + 0] = t.v0.x, h.xs[4 * i + 1] = t.v1.x, h.xs[4 * i + 2] = t.v2.x, h.xs[4 * i + 3] = 0;
    h.ys[4 * i + 0] = t.v0.y, h.ys[4 * i + 1] = t.v1.y, h.ys[4 * i + 2] = t.v2.y, h.ys[4 * i + 3] = 0;
    h.zs[4 * i + 0] = t.v0.z, h.zs[4 * i + 1] = t.v1.z, h.zs[4 * i + 2] = t.v2.z, h.zs[4 * i + 3] = 0;
    h.matId[i] = matIdx;
  }
  Camera c{};
  c.dir[0] = 0.f, c.dir[1] = 1.f, c.dir[2] = 0.f;
  c.pos[0] = c.pos[1] = c.pos[2] = 0.f;
  c.width = 256, c.height = 256, c.spp = 4;
  c.focalLength = 20.f, c.sensorSize = 36.f;
  h.cam = c;
  return h;
}

}  // namespace

// =====================================================================================
// C API (ctypes-friendly).  Everything is plain pointers and sizes.
// =====================================================================================
extern "C" {

struct OracleScene {  // mirrors include/dmt_hip.h's upload calls
  const float* xs;
  const float* ys;
  const float* zs;
  const uint32_t* matId;
  uint64_t triCount;
  const void* lights;
  uint32_t lightCount;
  const void* infLights;
  uint32_t infLightCount;
  const void* bsdfs;
  uint32_t bsdfCount;
  // A18 (optional): equirectangular RGB float image, h x w x 3, w == 2 h, powers of two; quaternion x,y,z,w
  const float* envRgb;
  int32_t envW, envH;
  float envQuat[4];
  float envScale;
  // emissive triangles -- triangle indices and rgb radiance per entry
  const uint32_t* areaTri;
  const float* areaLe;
  uint32_t areaCount;
  // image textures, see Scene
  const uint8_t* texRgba;
  const int32_t* texDesc;
  uint32_t texCount;
  const uint32_t* matTex;
  const float* triUv;
  int32_t lightSampling;  // 0 = uniform pick, 1 = light tree (reduced: one light), 2 = the reference's tree (cuts of up to four lights)
};

static Scene toScene(OracleScene const* s, EnvMap* envStorage = nullptr, std::vector<uint32_t>* areaStorage = nullptr,
                     std::vector<LtNode>* treeStorage = nullptr, std::vector<LtrNode>* refTreeStorage = nullptr) {
  Scene sc;
  if (areaStorage && s->areaCount > 0 && s->areaTri && s->areaLe) {
    areaStorage->assign(size_t(s->triCount), 0xFFFFFFFFu);
    for (uint32_t k = 0; k < s->areaCount; ++k)
      if (s->areaTri[k] < s->triCount) (*areaStorage)[s->areaTri[k]] = k;
    sc.areaOf = areaStorage->data(), sc.areaTri = s->areaTri, sc.areaLe = s->areaLe, sc.areaCount = s->areaCount;
  }
  if (envStorage && s->envRgb && s->envW > 0 && s->envH > 0) {
    envBuild(s->envRgb, s->envW, s->envH, s->envQuat, s->envScale, *envStorage);
    sc.env = envStorage;
  }
  sc.xs = s->xs, sc.ys = s->ys, sc.zs = s->zs, sc.matId = s->matId, sc.triCount = s->triCount;
  sc.lights = reinterpret_cast<Rec32 const*>(s->lights), sc.lightCount = s->lightCount;
  sc.infLights = reinterpret_cast<Rec32 const*>(s->infLights), sc.infLightCount = s->infLightCount;
  sc.bsdfs = reinterpret_cast<Rec32 const*>(s->bsdfs), sc.bsdfCount = s->bsdfCount;
  if (s->texCount > 0 && s->texRgba && s->texDesc && s->matTex && s->triUv)
    sc.texRgba = s->texRgba, sc.texDesc = s->texDesc, sc.texCount = s->texCount, sc.matTex = s->matTex, sc.triUv = s->triUv;
  if (treeStorage && s->lightSampling == 1 && s->lightCount > 1) {
    *treeStorage = ltBuild(sc.lights, sc.lightCount);
    if (!treeStorage->empty()) sc.lightTree = treeStorage->data();
  }
  if (refTreeStorage && s->lightSampling == 2 && s->lightCount > 1) {
    *refTreeStorage = ltrBuild(sc.lights, sc.lightCount);
    if (!refTreeStorage->empty()) sc.lightTreeRef = refTreeStorage->data();
  }
  return sc;
}

// per-light selection probability at (p, n) of the tree over `count` packed lights; also node count and depth-free checks
int oracle_light_tree_pmfs(const void* lights32, uint32_t count, const float* p3, const float* n3, float* out, int* nodeCount) {
  std::vector<LtNode> const nodes = ltBuild(reinterpret_cast<Rec32 const*>(lights32), count);
  ltPmfs(nodes, v3(p3[0], p3[1], p3[2]), v3(n3[0], n3[1], n3[2]), out, count);
  if (nodeCount) *nodeCount = int(nodes.size());
  return 0;
}

// the reference-semantics tree at n shading points: up to four (light index, pmf) pairs each, plus the tree's shape
int oracle_light_tree_ref_select(const void* lights32, uint32_t count, int n, const float* p3, const float* n3, const float* u, float startPMF,
                                 int32_t* indices4, float* pmfs4, int32_t* counts, int* nodeCount) {
  std::vector<LtrNode> const nodes = ltrBuild(reinterpret_cast<Rec32 const*>(lights32), count);
  if (nodeCount) *nodeCount = int(nodes.size());
  if (nodes.empty()) return -1;
  for (int i = 0; i < n; ++i) {
    LtrSelection const sel = ltrSelect(nodes.data(), v3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]), v3(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2]), u[i], startPMF);
    counts[i] = int32_t(sel.count);
    for (int k = 0; k < 4; ++k) indices4[4 * i + k] = k < int(sel.count) ? int32_t(sel.indices[k]) : -1, pmfs4[4 * i + k] = k < int(sel.count) ? sel.pmfs[k] : 0.f;
  }
  return 0;
}

// --- scene: cornellBox() -----------------------------------------------------------------
// two-call protocol: counts first (pass null arrays), then fill.
int oracle_cornell_box(float* xs, float* ys, float* zs, uint32_t* matId, uint64_t* triCount,
                       void* bsdfs, uint32_t* bsdfCount, void* lights, uint32_t* lightCount,
                       void* infLights, uint32_t* infCount, void* camera44) {
  HostScene const h = cornellBox();
  *triCount = h.matId.size();
  *bsdfCount = uint32_t(h.bsdfs.size());
  *lightCount = uint32_t(h.lights.size());
  *infCount = uint32_t(h.infLights.size());
  if (xs) memcpy(xs, h.xs.data(), h.xs.size() * 4);
  if (ys) memcpy(ys, h.ys.data(), h.ys.size() * 4);
  if (zs) memcpy(zs, h.zs.data(), h.zs.size() * 4);
  if (matId) memcpy(matId, h.matId.data(), h.matId.size() * 4);
  if (bsdfs) memcpy(bsdfs, h.bsdfs.data(), h.bsdfs.size() * 32);
  if (lights) memcpy(lights, h.lights.data(), h.lights.size() * 32);
  if (infLights) memcpy(infLights, h.infLights.data(), h.infLights.size() * 32);
  if (camera44) memcpy(camera44, &h.cam, sizeof(Camera));
  return 0;
}

// --- makers (write one 32-byte record) ---------------------------------------------------
void oracle_make_oren_nayar(const float* color3, float roughness, void* out32) {
  Rec32 r = makeOrenNayar(v3(color3[0], color3[1], color3[2]), roughness);
  memcpy(out32, &r, 32);
}
void oracle_make_ggx_dielectric(const float* r3, const float* t3, float phi0, float eta, float ax,
                                float ay, void* out32) {
  Rec32 r = makeGGXDielectric(v3(r3[0], r3[1], r3[2]), v3(t3[0], t3[1], t3[2]), phi0, eta, ax, ay);
  memcpy(out32, &r, 32);
}
void oracle_make_ggx_conductor(const float* eta3, const float* k3, float phi0, float ax, float ay,
                               void* out32) {
  Rec32 r = makeGGXConductor(v3(eta3[0], eta3[1], eta3[2]), v3(k3[0], k3[1], k3[2]), phi0, ax, ay);
  memcpy(out32, &r, 32);
}
void oracle_make_lambert(void* out32) {
  Rec32 r = makeLambert();
  memcpy(out32, &r, 32);
}
void oracle_make_point_light(const float* c3, const float* p3, float radius, void* out32) {
  Rec32 r = makePointLight(v3(c3[0], c3[1], c3[2]), v3(p3[0], p3[1], p3[2]), radius);
  memcpy(out32, &r, 32);
}
void oracle_make_spot_light(const float* c3, const float* p3, const float* d3, float cos0,
                            float cosE, float radius, void* out32) {
  Rec32 r = makeSpotLight(v3(c3[0], c3[1], c3[2]), v3(p3[0], p3[1], p3[2]),
                          v3(d3[0], d3[1], d3[2]), cos0, cosE, radius);
  memcpy(out32, &r, 32);
}
void oracle_make_directional_light(const float* c3, const float* d3, float omc, void* out32) {
  Rec32 r = makeDirectionalLight(v3(c3[0], c3[1], c3[2]), v3(d3[0], d3[1], d3[2]), omc);
  memcpy(out32, &r, 32);
}
void oracle_make_env_light(const float* c3, void* out32) {
  Rec32 r = makeEnvLight(v3(c3[0], c3[1], c3[2]));
  memcpy(out32, &r, 32);
}

// --- encodings ---------------------------------------------------------------------------
uint16_t oracle_float_to_half(float f) { return f2h(f); }
float oracle_half_to_float(uint16_t h) { return h2f(h); }
uint32_t oracle_octa_from_dir(const float* d3) { return octaFromDir(v3(d3[0], d3[1], d3[2])); }
void oracle_dir_from_octa(uint32_t o, float* out3) {
  V3 const d = dirFromOcta(o);
  out3[0] = d.x, out3[1] = d.y, out3[2] = d.z;
}

// --- sampler -----------------------------------------------------------------------------
void oracle_halton_params(int width, int height, int32_t* out6) {
  HaltonParams const p = computeParams(width, height);
  out6[0] = p.baseScales[0], out6[1] = p.baseScales[1];
  out6[2] = p.baseExponents[0], out6[3] = p.baseExponents[1];
  out6[4] = p.multInvs[0], out6[5] = p.multInvs[1];
}
// for each (px,py,s): haltonIndex, pixel2D (2 floats), then `ndims` successive get1D() values
void oracle_sampler_stream(int width, int height, int n, const int32_t* pxs, const int32_t* pys,
                           const int32_t* ss, int ndims, int32_t* haltonIndex, float* pixel2d,
                           float* dims) {
  HaltonParams const p = computeParams(width, height);
  for (int i = 0; i < n; ++i) {
    Sampler r;
    r.startPixelSample(p, pxs[i], pys[i], ss[i]);
    haltonIndex[i] = r.haltonIndex;
    V2 const px = r.getPixel2D(p);
    pixel2d[2 * i] = px.x, pixel2d[2 * i + 1] = px.y;
    for (int d = 0; d < ndims; ++d) dims[size_t(i) * ndims + d] = r.get1D();
  }
}
// raw sampleDim(dim, index)
float oracle_sample_dim(int dim, int index) { return sampleDim(dim, index); }

// --- camera ------------------------------------------------------------------------------
void oracle_camera_rays(const void* camera44, int n, const int32_t* pxs, const int32_t* pys,
                        const int32_t* ss, float* o3, float* d3) {
  Camera cam;
  memcpy(&cam, camera44, sizeof(Camera));
  RenderCfg const cfg = makeCfg(cam, 32, 0);
  for (int i = 0; i < n; ++i) {
    Sampler r;
    r.startPixelSample(cfg.hp, pxs[i], pys[i], ss[i]);
    Ray const ray = cameraRay(cameraSampleFilm(pxs[i], pys[i], r, cfg.hp), cfg.cameraFromRaster,
                              cfg.renderFromCamera);
    o3[3 * i] = ray.o.x, o3[3 * i + 1] = ray.o.y, o3[3 * i + 2] = ray.o.z;
    d3[3 * i] = ray.d.x, d3[3 * i + 1] = ray.d.y, d3[3 * i + 2] = ray.d.z;
  }
}
void oracle_camera_transforms(const void* camera44, float* cameraFromRaster32,
                              float* renderFromCamera32) {
  Camera cam;
  memcpy(&cam, camera44, sizeof(Camera));
  RenderCfg const cfg = makeCfg(cam, 32, 0);
  memcpy(cameraFromRaster32, &cfg.cameraFromRaster, 128);
  memcpy(renderFromCamera32, &cfg.renderFromCamera, 128);
}

// --- triangle intersection ---------------------------------------------------------------
// one ray vs n triangles: hit flag, t, pos, normal, error (device routine restatement)
void oracle_triangle_intersect(const float* xs, const float* ys, const float* zs, uint64_t n,
                               const float* o3, const float* d3, int32_t* hit, float* t, float* pos3,
                               float* nrm3, float* err3) {
  Ray const ray{v3(o3[0], o3[1], o3[2]), v3(d3[0], d3[1], d3[2])};
  for (uint64_t i = 0; i < n; ++i) {
    Hit const h = triangleIntersect(xs + 4 * i, ys + 4 * i, zs + 4 * i, ray);
    hit[i] = h.hit;
    if (t) t[i] = h.t;
    if (pos3) pos3[3 * i] = h.pos.x, pos3[3 * i + 1] = h.pos.y, pos3[3 * i + 2] = h.pos.z;
    if (nrm3) nrm3[3 * i] = h.normal.x, nrm3[3 * i + 1] = h.normal.y, nrm3[3 * i + 2] = h.normal.z;
    if (err3) err3[3 * i] = h.error.x, err3[3 * i + 1] = h.error.y, err3[3 * i + 2] = h.error.z;
  }
}
// the reference test's expected values: host Moeller-Trumbore hit flags
void oracle_host_intersect_mt(const float* xs, const float* ys, const float* zs, uint64_t n,
                              const float* o3, const float* d3, int32_t* hit) {
  for (uint64_t i = 0; i < n; ++i) {
    V3 const p0 = v3(xs[4 * i], ys[4 * i], zs[4 * i]);
    V3 const p1 = v3(xs[4 * i + 1], ys[4 * i + 1], zs[4 * i + 1]);
    V3 const p2 = v3(xs[4 * i + 2], ys[4 * i + 2], zs[4 * i + 2]);
    hit[i] = hostIntersectMT(v3(o3[0], o3[1], o3[2]), v3(d3[0], d3[1], d3[2]), p0, p1, p2).hit ? 1 : 0;
  }
}
// closest hit of n rays against a soup (brute force, lowest index on ties): index (-1 = miss), t
void oracle_closest_hit(const float* xs, const float* ys, const float* zs, uint64_t ntri, int nrays,
                        const float* o3, const float* d3, int32_t* triIdx, float* tOut) {
  for (int r = 0; r < nrays; ++r) {
    Ray const ray{v3(o3[3 * r], o3[3 * r + 1], o3[3 * r + 2]), v3(d3[3 * r], d3[3 * r + 1], d3[3 * r + 2])};
    float best = std::numeric_limits<float>::infinity();
    int32_t idx = -1;
    for (uint64_t i = 0; i < ntri; ++i) {
      Hit const h = triangleIntersect(xs + 4 * i, ys + 4 * i, zs + 4 * i, ray);
      if (h.hit && h.t < best) best = h.t, idx = int32_t(i);
    }
    triIdx[r] = idx;
    tOut[r] = best;
  }
}
void oracle_offset_ray_origin(const float* p3, const float* e3, const float* n3, const float* w3,
                              float* out3) {
  V3 const r = offsetRayOrigin(v3(p3[0], p3[1], p3[2]), v3(e3[0], e3[1], e3[2]),
                               v3(n3[0], n3[1], n3[2]), v3(w3[0], w3[1], w3[2]));
  out3[0] = r.x, out3[1] = r.y, out3[2] = r.z;
}

// --- BSDF: prepare + sample + eval over a lattice ----------------------------------------
// per case i: ns3, wo3, u2, uc, wi_eval3 -> out: prepared record (32 B), sample {wi3,f3,pdf,eta,
// delta,refract} (10 floats), eval {f3*weight, pdf} (4 floats)
void oracle_bsdf_cases(const void* bsdf32, int n, const float* ns3, const float* wo3, const float* u2,
                       const float* uc, const float* wiEval3, void* prepared32, float* sample10,
                       float* eval4) {
  for (int i = 0; i < n; ++i) {
    Rec32 b;
    memcpy(&b, bsdf32, 32);
    V3 const ns = v3(ns3[3 * i], ns3[3 * i + 1], ns3[3 * i + 2]);
    V3 const wo = v3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
    prepareBSDF(&b, ns, wo, 0);
    memcpy(static_cast<char*>(prepared32) + 32 * size_t(i), &b, 32);
    BSDFSample const s = sampleBsdf(b, wo, ns, ns, v2(u2[2 * i], u2[2 * i + 1]), uc[i]);
    float* o = sample10 + 10 * size_t(i);
    o[0] = s.wi.x, o[1] = s.wi.y, o[2] = s.wi.z, o[3] = s.f.x, o[4] = s.f.y, o[5] = s.f.z;
    o[6] = s.pdf, o[7] = s.eta, o[8] = s.delta ? 1.f : 0.f, o[9] = s.refract ? 1.f : 0.f;
    float pdf = 0;
    V3 const wi = v3(wiEval3[3 * i], wiEval3[3 * i + 1], wiEval3[3 * i + 2]);
    V3 const f = evalBsdf(b, wo, wi, ns, ns, &pdf) * bsdfWeight(b);
    float* e = eval4 + 4 * size_t(i);
    e[0] = f.x, e[1] = f.y, e[2] = f.z, e[3] = pdf;
  }
}

void oracle_set_cos_nh_ulps(int ulps) { g_cosNhUlps = ulps; }

// oracle_bsdf_cases with a geometric normal of its own per case (ng3): what the path tracer hands sampleBsdf / evalBsdf
// under a normal map, where ns != hit.normal
void oracle_bsdf_cases_ng(const void* bsdf32, int n, const float* ns3, const float* ng3, const float* wo3, const float* u2,
                          const float* uc, const float* wiEval3, void* prepared32, float* sample10, float* eval4) {
  for (int i = 0; i < n; ++i) {
    Rec32 b;
    memcpy(&b, bsdf32, 32);
    V3 const ns = v3(ns3[3 * i], ns3[3 * i + 1], ns3[3 * i + 2]);
    V3 const ng = v3(ng3[3 * i], ng3[3 * i + 1], ng3[3 * i + 2]);
    V3 const wo = v3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]);
    prepareBSDF(&b, ns, wo, 0);
    memcpy(static_cast<char*>(prepared32) + 32 * size_t(i), &b, 32);
    BSDFSample const s = sampleBsdf(b, wo, ns, ng, v2(u2[2 * i], u2[2 * i + 1]), uc[i]);
    float* o = sample10 + 10 * size_t(i);
    o[0] = s.wi.x, o[1] = s.wi.y, o[2] = s.wi.z, o[3] = s.f.x, o[4] = s.f.y, o[5] = s.f.z;
    o[6] = s.pdf, o[7] = s.eta, o[8] = s.delta ? 1.f : 0.f, o[9] = s.refract ? 1.f : 0.f;
    float pdf = 0;
    V3 const wi = v3(wiEval3[3 * i], wiEval3[3 * i + 1], wiEval3[3 * i + 2]);
    V3 const f = evalBsdf(b, wo, wi, ns, ng, &pdf) * bsdfWeight(b);
    float* e = eval4 + 4 * size_t(i);
    e[0] = f.x, e[1] = f.y, e[2] = f.z, e[3] = pdf;
  }
}

// The material of triangle tri[i] at (bu, bv) as tracePath patches it before prepareBSDF: the record after
// applyMaterialTextures and the shading normal it returns for the geometric normal ng3[i].  A BS_GGX_BLEND material also
// gives its conductor record, patched the same way, and the metallic fraction; its dielectric record keeps the blend tag.
int oracle_material_at_hit(const OracleScene* s, int n, const int32_t* tri, const float* bu, const float* bv, const float* ng3,
                           int lookupUlps, void* rec32, float* ns3, void* rec2_32, float* mixOut) {
  Scene const sc = toScene(s);
  for (int i = 0; i < n; ++i) {
    if (tri[i] < 0 || uint64_t(tri[i]) >= sc.triCount) return 1;
    uint32_t const matId = sc.matId[tri[i]];
    if (matId >= sc.bsdfCount) return 1;
    V3 const ng = v3(ng3[3 * i], ng3[3 * i + 1], ng3[3 * i + 2]);
    Rec32 bsdf = sc.bsdfs[matId], bsdf2{};
    float mix = 0.f;
    bool const blend = bsdfType(bsdf) == BS_GGX_BLEND;
    if (blend) {
      if (matId + 1 >= sc.bsdfCount) return 1;
      mix = blendMetallic(sc, bsdf, matId, tri[i], bu[i], bv[i]);
      wr16(bsdf, B_TYPE, BS_GGX_DIEL);
      bsdf2 = sc.bsdfs[matId + 1];
    }
    V3 const ns = applyMaterialTextures(sc, bsdf, matId, tri[i], bu[i], bv[i], ng, lookupUlps);
    if (blend) {
      (void)applyMaterialTextures(sc, bsdf2, matId + 1, tri[i], bu[i], bv[i], ng, lookupUlps);
      wr16(bsdf, B_TYPE, BS_GGX_BLEND);
    }
    memcpy(static_cast<char*>(rec32) + 32 * size_t(i), &bsdf, 32);
    memcpy(static_cast<char*>(rec2_32) + 32 * size_t(i), &bsdf2, 32);
    ns3[3 * i] = ns.x, ns3[3 * i + 1] = ns.y, ns3[3 * i + 2] = ns.z;
    mixOut[i] = mix;
  }
  return 0;
}

// --- lights: sample + eval ---------------------------------------------------------------
// out per case: {pLight3, dir3, pdf, delta, distance, factor, Le3, valid} = 14 floats
void oracle_light_cases(const void* light32, int n, const float* pos3, const float* nrm3,
                        const float* u2, const int32_t* hadTransmission, float* out14) {
  Rec32 L;
  memcpy(&L, light32, 32);
  for (int i = 0; i < n; ++i) {
    LightSample const s = sampleLight(L, v3(pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2]),
                                      v2(u2[2 * i], u2[2 * i + 1]), hadTransmission[i] != 0,
                                      v3(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2]));
    V3 const Le = evalLight(L, s);
    float* o = out14 + 14 * size_t(i);
    o[0] = s.pLight.x, o[1] = s.pLight.y, o[2] = s.pLight.z;
    o[3] = s.direction.x, o[4] = s.direction.y, o[5] = s.direction.z;
    o[6] = s.pdf, o[7] = float(s.delta), o[8] = s.distance, o[9] = s.factor;
    o[10] = Le.x, o[11] = Le.y, o[12] = Le.z, o[13] = s.valid() ? 1.f : 0.f;
  }
}

// --- full render ---------------------------------------------------------------------------
// Renders pixels [x0,x1) x [y0,y1) for samples [sampleOffset, sampleOffset+spp) into the
// row-major film (mean4 / m24: width*height float4 each, running Welford state, N in m2.w).
// threads <= 1: single thread.  Otherwise 32x32 tiles over a std::thread pool, the way the
// reference's CPU renderer schedules (src/core/private/core-render.cpp:484-485,565-597).
// stats6 (optional): samples, closestRays, shadowRays, triTests, bounces, hits.
int oracle_render(const OracleScene* s, const void* camera44, int maxDepth, int sampleOffset, int spp,
                  int x0, int y0, int x1, int y1, int threads, int rtlArgs, float* mean4, float* m24,
                  uint64_t* stats6) {
  Camera cam;
  memcpy(&cam, camera44, sizeof(Camera));
  EnvMap env;
  std::vector<uint32_t> areaOf;
  std::vector<LtNode> lightTree;
  std::vector<LtrNode> lightTreeRef;
  Scene const sc = toScene(s, &env, &areaOf, &lightTree, &lightTreeRef);
  RenderCfg const cfg = makeCfg(cam, maxDepth, rtlArgs);
  if (x0 < 0) x0 = 0;
  if (y0 < 0) y0 = 0;
  if (x1 > cam.width) x1 = cam.width;
  if (y1 > cam.height) y1 = cam.height;
  if (x1 <= x0 || y1 <= y0) return 0;
  int const T = 32;
  int const tx = (x1 - x0 + T - 1) / T, ty = (y1 - y0 + T - 1) / T;
  int const ntiles = tx * ty;
  std::atomic<int> next{0};
  int const nthreads = threads < 1 ? 1 : threads;
  std::vector<Stats> stats(static_cast<size_t>(nthreads), Stats{});
  auto worker = [&](int tid) {
    Stats* st = stats6 ? &stats[size_t(tid)] : nullptr;
    for (;;) {
      int const t = next.fetch_add(1);
      if (t >= ntiles) break;
      int const bx = x0 + (t % tx) * T, by = y0 + (t / tx) * T;
      for (int y = by; y < by + T && y < y1; ++y)
        for (int x = bx; x < bx + T && x < x1; ++x)
          renderPixel(sc, cfg, x, y, sampleOffset, spp, mean4, m24, st);
    }
  };
  if (nthreads == 1) {
    worker(0);
  } else {
    std::vector<std::thread> pool;
    for (int i = 0; i < nthreads; ++i) pool.emplace_back(worker, i);
    for (auto& th : pool) th.join();
  }
  if (stats6) {
    Stats tot;
    for (auto const& st : stats) {
      tot.samples += st.samples, tot.closestRays += st.closestRays, tot.shadowRays += st.shadowRays;
      tot.triTests += st.triTests, tot.bounces += st.bounces, tot.hits += st.hits;
    }
    stats6[0] = tot.samples, stats6[1] = tot.closestRays, stats6[2] = tot.shadowRays;
    stats6[3] = tot.triTests, stats6[4] = tot.bounces, stats6[5] = tot.hits;
  }
  return 0;
}

// radiance of individual (pixel, sample) paths (no film), for localising divergence
void oracle_trace_samples(const OracleScene* s, const void* camera44, int maxDepth, int n,
                          const int32_t* pxs, const int32_t* pys, const int32_t* ss, int rtlArgs,
                          float* L3) {
  Camera cam;
  memcpy(&cam, camera44, sizeof(Camera));
  EnvMap env;
  std::vector<uint32_t> areaOf;
  std::vector<LtNode> lightTree;
  std::vector<LtrNode> lightTreeRef;
  Scene const sc = toScene(s, &env, &areaOf, &lightTree, &lightTreeRef);
  RenderCfg const cfg = makeCfg(cam, maxDepth, rtlArgs);
  for (int i = 0; i < n; ++i) {
    V3 const L = tracePath(sc, cfg, pxs[i], pys[i], ss[i], nullptr);
    L3[3 * i] = L.x, L3[3 * i + 1] = L.y, L3[3 * i + 2] = L.z;
  }
}

// per-bounce log of one path: records of 12 floats {tri, pos3, beta3, L3 (before shading), depth, dim}
int oracle_trace_log(const OracleScene* s, const void* camera44, int maxDepth, int px, int py, int smp,
                     int rtlArgs, float* rec12, int cap, float* Lout3) {
  Camera cam;
  memcpy(&cam, camera44, sizeof(Camera));
  EnvMap env;
  std::vector<uint32_t> areaOf;
  std::vector<LtNode> lightTree;
  std::vector<LtrNode> lightTreeRef;
  Scene const sc = toScene(s, &env, &areaOf, &lightTree, &lightTreeRef);
  RenderCfg const cfg = makeCfg(cam, maxDepth, rtlArgs);
  PathLog log;
  log.rec = rec12, log.cap = cap;
  V3 const L = tracePath(sc, cfg, px, py, smp, nullptr, &log);
  Lout3[0] = L.x, Lout3[1] = L.y, Lout3[2] = L.z;
  return log.n;
}

// --- A18 env map: tables and per-function cases ---------------------------------------------
// func/cdf: h*w each; rowInt, mFunc, mCdf: h each; mInt: 1
void oracle_envmap_tables(const float* rgb, int w, int h, float* func, float* cdf, float* rowInt, float* mFunc,
                          float* mCdf, float* mInt) {
  float const q[4] = {0, 0, 0, 1};
  EnvMap e;
  envBuild(rgb, w, h, q, 1.f, e);
  memcpy(func, e.func.data(), e.func.size() * 4);
  memcpy(cdf, e.cdf.data(), e.cdf.size() * 4);
  memcpy(rowInt, e.rowInt.data(), e.rowInt.size() * 4);
  memcpy(mFunc, e.marginal.absf.data(), size_t(h) * 4);
  memcpy(mCdf, e.marginal.cdf.data(), size_t(h) * 4);
  *mInt = e.marginal.integral;
}
// sampling: per case u2 -> wi3, pdf, uv2, Le3 (Le by uv, as NEE uses it), ok
void oracle_envmap_sample(const float* rgb, int w, int h, const float* quat4, int n, const float* u2, float* wi3,
                          float* pdf, float* uv2, float* Le3, int32_t* ok) {
  EnvMap e;
  envBuild(rgb, w, h, quat4, 1.f, e);
  for (int i = 0; i < n; ++i) {
    EnvSample const es = envSample(e, V2{u2[2 * i], u2[2 * i + 1]});
    V3 const Le = envEvalUv(e, es.uv);
    wi3[3 * i] = es.wi.x, wi3[3 * i + 1] = es.wi.y, wi3[3 * i + 2] = es.wi.z;
    pdf[i] = es.pdf, uv2[2 * i] = es.uv.x, uv2[2 * i + 1] = es.uv.y;
    Le3[3 * i] = Le.x, Le3[3 * i + 1] = Le.y, Le3[3 * i + 2] = Le.z;
    ok[i] = es.ok ? 1 : 0;
  }
}
// evaluation by direction (what a path ray that leaves the scene sees): Le3, pdf
void oracle_envmap_eval(const float* rgb, int w, int h, const float* quat4, int n, const float* wi3, float* Le3,
                        float* pdf) {
  EnvMap e;
  envBuild(rgb, w, h, quat4, 1.f, e);
  for (int i = 0; i < n; ++i) {
    V3 const Le = envEvalDir(e, v3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), &pdf[i]);
    Le3[3 * i] = Le.x, Le3[3 * i + 1] = Le.y, Le3[3 * i + 2] = Le.z;
  }
}

// 8-bit quantisation of the writers            CC/private/host_utils.cu:475-497
void oracle_pixels_from_film(const float* mean4, const float* m24, uint64_t npix, uint8_t* meanRgb,
                             uint8_t* seRgb) {
  for (uint64_t i = 0; i < npix; ++i) {
    for (int c = 0; c < 3; ++c) {
      float const m = fminf(fmaxf(mean4[4 * i + c], 0.f) * 255.f, 255.f);
      meanRgb[3 * i + c] = uint8_t(m);
      float const se = fminf(fmaxf(safeSqrt(m24[4 * i + c]) / m24[4 * i + 3], 0.f) * 255.f, 255.f);
      seRgb[3 * i + c] = uint8_t(se);
    }
  }
}

int oracle_hardware_threads() { return int(std::thread::hardware_concurrency()); }

}  // extern "C"
