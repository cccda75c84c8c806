// vnormals.hpp -- smooth shading (dmt_upload_vertex_normals): the per-triangle record of three vertex
// normals, the shading normal interpolated from it at a hit, and the host side that makes the records and computes
// normals for soups that come without any (dmt_smooth_normals).
//
// Part of dmt_hip.hip's translation unit, included once after the kernel-argument accessors.  Only code instantiated
// with kFeatVtxNormals (the *_vn rows, their probes, k_aov_vn) calls shading_normal_at, so no other kernel gains a
// register or an instruction.
//
// The record: 16 bytes per triangle, fetched by one 16-byte load at the hit.  Words 0..2 are the normals at vertices
// 0, 1, 2 in the octahedral mapping of the light records (decoded by dir_from_octa, unchanged), word 3 holds flags
// (bit 0: smooth).  The reference's ENCODER cannot be used as it stands: encodeOctaComponent clamps to [0, 1] before it
// rounds (encoding.cu:17-21), so each 16-bit component comes out 0 or 1 -- kept bit for bit where a light direction is
// packed, because the reference renders with that, but useless for normals.  octa_from_dir_host below is that
// arithmetic with the clamp at 65535, i.e. what the decoder inverts; tests/vnormal_ref.py restates it.
#pragma once

struct VtxNormalRec {
  uint32_t n[3];   // octahedral words of the normals at vertices 0, 1, 2
  uint32_t flags;  // bit 0: smooth; 0: flat (the triangle keeps its geometric normal)
};
static_assert(sizeof(VtxNormalRec) == 16, "one 16-byte load per hit");
constexpr uint32_t kVtxNormalSmooth = 1u;

// The shading normal of triangle `tri` at the barycentrics (bu, bv) of vertices 1 and 2 (hit_finish's), for the geometric
// normal ngFacing already flipped against the ray: n = w0 n0 + bu n1 + bv n2 with w0 = 1 - bu - bv (the weighting of the
// UV interpolation), normalised, and negated where it leaves the hemisphere of ngFacing -- whichever way the file's
// normals and winding point, the shading normal faces the ray's side of the surface.  A flat triangle, and a sum whose
// squared length is not finite or below 1e-12, give ngFacing bit for bit.
DMT_DEV f3 shading_normal_at(KArgs k, int tri, float bu, float bv, f3 ngFacing) {
  uint4 const r = *reinterpret_cast<uint4 const*>(kargs(k)->vtxNormals + tri);
  if (!(r.w & kVtxNormalSmooth)) return ngFacing;
  f3 const n0 = dir_from_octa(r.x), n1 = dir_from_octa(r.y), n2 = dir_from_octa(r.z);
  float const w0 = 1.f - bu - bv;
  f3 n = w0 * n0 + bu * n1 + bv * n2;
  float const l2 = dot(n, n);
  if (!(l2 >= 1e-12f && l2 < kInf)) return ngFacing;
  n = n * rsqrt_ieee(l2);
  if (dot(n, ngFacing) < 0.f) n = -n;
  return n;
}

namespace vnormals {

// encoding.cu:26-37 with the component clamped to [0, 65535] (see the head of this file); fp32, one operation per step
inline uint32_t octa_component_host(float v) {
  float const s = (v + 1.f) * 0.5f * 65535.f;
  return uint32_t(roundf(fmaxf(fminf(s, 65535.f), 0.f)));
}
inline uint32_t octa_from_dir_host(float const d[3]) {
  float const l1 = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]);
  float const px = d[0] / l1, py = d[1] / l1, pz = d[2] / l1;
  float x = px, y = py;
  if (pz < 0.f) {  // the lower half folds over the diagonals
    x = (1.f - fabsf(py)) * (std::signbit(px) ? -1.f : 1.f);
    y = (1.f - fabsf(px)) * (std::signbit(py) ? -1.f : 1.f);
  }
  return octa_component_host(y) << 16 | octa_component_host(x);
}

// n9: 9 floats per triangle -> records.  Returns -1, or the index of the first triangle with a normal that is not finite
// or shorter than 1e-6 while the triangle is not all zero (= flat).  *smooth: the number of smooth records.
inline long long packRecords(float const* n9, size_t count, std::vector<VtxNormalRec>& out, uint64_t* smooth) {
  out.assign(count, VtxNormalRec{{0u, 0u, 0u}, 0u});
  uint64_t ns = 0;
  for (size_t i = 0; i < count; ++i) {
    float const* const v = n9 + 9 * i;
    bool allZero = true;
    for (int c = 0; c < 9; ++c) allZero = allZero && v[c] == 0.f;
    if (allZero) continue;
    for (int c = 0; c < 3; ++c) {
      float const* const n = v + 3 * c;
      if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2])) return (long long)i;
      double const len = std::sqrt(double(n[0]) * n[0] + double(n[1]) * n[1] + double(n[2]) * n[2]);
      if (!(len >= 1e-6)) return (long long)i;
      float const u[3] = {float(n[0] / len), float(n[1] / len), float(n[2] / len)};  // normalised on the host
      out[i].n[c] = octa_from_dir_host(u);
    }
    out[i].flags = kVtxNormalSmooth;
    ++ns;
  }
  *smooth = ns;
  return -1;
}

// dmt_smooth_normals: see include/dmt_hip.h.  Positions are welded bit for bit; face normals are TriPost's
// normalize(cross(e1, e0)) in fp32; sums and angles in double.
inline void smoothNormals(float const* xs, float const* ys, float const* zs, size_t count, float creaseDegrees, float* n9) {
  struct Key {
    uint32_t x, y, z;
    bool operator<(Key const& o) const { return x != o.x ? x < o.x : y != o.y ? y < o.y : z < o.z; }
  };
  auto bits = [](float f) {
    if (f == 0.f) f = 0.f;  // -0 welds with +0
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
  };
  struct Corner { uint32_t tri; double angle; };
  std::vector<float> fn(3 * count, 0.f);
  std::vector<char> valid(count, 0);
  std::map<Key, std::vector<Corner>> weld;
  for (size_t i = 0; i < count; ++i) {
    float p[3][3];
    for (int c = 0; c < 3; ++c) p[c][0] = xs[4 * i + c], p[c][1] = ys[4 * i + c], p[c][2] = zs[4 * i + c];
    float const e0[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    float const e1[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    float const cx = e1[1] * e0[2] - e1[2] * e0[1], cy = e1[2] * e0[0] - e1[0] * e0[2], cz = e1[0] * e0[1] - e1[1] * e0[0];
    float const l2 = (cx * cx + cy * cy) + cz * cz;
    if (!(l2 > 0.f) || !std::isfinite(l2)) continue;  // zero area: contributes nothing, comes out flat
    float const inv = 1.f / sqrtf(l2);
    fn[3 * i] = cx * inv, fn[3 * i + 1] = cy * inv, fn[3 * i + 2] = cz * inv;
    valid[i] = 1;
    for (int c = 0; c < 3; ++c) {  // the interior angle at corner c
      double a[3], b[3];
      for (int d = 0; d < 3; ++d) a[d] = double(p[(c + 1) % 3][d]) - p[c][d], b[d] = double(p[(c + 2) % 3][d]) - p[c][d];
      double const la = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      double const cs = (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) / (la * lb);
      weld[Key{bits(p[c][0]), bits(p[c][1]), bits(p[c][2])}].push_back(Corner{uint32_t(i), std::acos(std::min(1.0, std::max(-1.0, cs)))});
    }
  }
  double const cosCrease = std::cos(std::min(180.0, std::max(0.0, double(creaseDegrees))) * 3.14159265358979323846 / 180.0);
  for (size_t i = 0; i < count; ++i) {
    for (int c = 0; c < 9; ++c) n9[9 * i + c] = 0.f;
    if (!valid[i]) continue;
    double const own[3] = {fn[3 * i], fn[3 * i + 1], fn[3 * i + 2]};
    for (int c = 0; c < 3; ++c) {
      double s[3] = {0, 0, 0};
      for (Corner const& o : weld[Key{bits(xs[4 * i + c]), bits(ys[4 * i + c]), bits(zs[4 * i + c])}]) {
        double const f[3] = {fn[3 * o.tri], fn[3 * o.tri + 1], fn[3 * o.tri + 2]};
        if (o.tri != i && own[0] * f[0] + own[1] * f[1] + own[2] * f[2] < cosCrease - 1e-12) continue;
        s[0] += o.angle * f[0], s[1] += o.angle * f[1], s[2] += o.angle * f[2];
      }
      double const len = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
      float* const out = n9 + 9 * i + 3 * c;
      if (len > 1e-12) out[0] = float(s[0] / len), out[1] = float(s[1] / len), out[2] = float(s[2] / len);
      else out[0] = fn[3 * i], out[1] = fn[3 * i + 1], out[2] = fn[3 * i + 2];  // the contributions cancel: the face's own
    }
  }
}

}  // namespace vnormals
