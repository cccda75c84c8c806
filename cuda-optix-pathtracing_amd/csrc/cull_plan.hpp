// cull_plan.hpp -- the host planners of the brute-force pass's culled clusters: the cluster record the device
// reads, the limits the plan keeps to, planBruteCull (sphere bounds), planBruteCullBox (box bounds) and planCullClusters,
// which runs them by the DMT_BRUTE_CULL level.  The device side is brute_clusters in dmt_hip.hip; the tables of a plan and the
// entry points that show one (dmt_brute_cull_plan, dmt_brute_cull_box_*, dmt_cull_records) are in accel_host.hpp.
//
// Host-only and self-contained: standard headers only, so a plain host compiler takes it without hip_runtime.h (a
// stand-alone program can run the planners under a sanitizer).  dmt_hip.hip includes it once, at file scope before its own
// anonymous namespace, because CullView and the device code name CullCluster and the limits.
//
// Culled clusters of the brute-force pass (planBruteCull / planBruteCullBox on the host, brute_clusters on the device).  A
// cluster is a run of consecutive triangles of one material -- one mesh of the scene front-ends -- with a cheap bound: a small
// sphere (compact meshes) or a thin box (flat meshes such as walls); the pass tests its triangles only for the rays that touch
// the bound, compacted over the wave's lanes.  Everything else stays in the "always" list, which the packed SGPR loop tests
// for every ray as before.
#pragma once

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

constexpr uint32_t kCullMaxClusters = 12;  // sphere clusters first, then box clusters; the device takes them kCullGroup at a time
constexpr uint32_t kCullMaxTris = 44;      // LDS copy of the culled triangles, 36 B each (see the LDS budget in DESIGN.md 4.1)
constexpr uint32_t kCullSlotBits = 6;      // a closest-hit key holds (original index << 6 | LDS slot): kCullMaxTris <= 64
constexpr uint32_t kCullMaxIndex = 1u << (32 - kCullSlotBits);  // no culling for soups of more triangles
struct alignas(64) CullCluster {           // 64 B: the first 32 are what a bound test reads, in one aligned s_load_dwordx8
  float b[6];                              // sphere: centre xyz and squared inflated radius; box: centre xyz, half-width xyz
  uint32_t box;                            // 0: sphere bound, 1: box bound
  uint32_t count;                          // original triangle indices [first, first + count)
  uint32_t first;
  uint32_t slot, magic;                    // first slot of its triangles in the LDS copy; ceil(2^32 / count)
  uint32_t pad[5];
};
static_assert(offsetof(CullCluster, box) == 24 && offsetof(CullCluster, count) == 28, "CullWords: the record's first eight words");
static_assert(sizeof(CullCluster) == 64 && alignof(CullCluster) == 64 && offsetof(CullCluster, first) == 32, "CullCluster layout");

// a triangle soup as the C ABI passes it: four floats per triangle and axis (three vertices and a pad), one material id each
struct CullSoup {
  float const *xs, *ys, *zs;
  uint32_t const* mat;
  uint32_t n;
  double vtx(uint32_t t, int k, int a) const { return double((a == 0 ? xs : a == 1 ? ys : zs)[4 * size_t(t) + k]); }
};
struct CullBox {
  double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
};
// bounds of triangles [first, end): the scene box, and the vertex box of every run
CullBox cullBounds(CullSoup const& s, uint32_t first, uint32_t end) {
  CullBox b;
  for (uint32_t t = first; t < end; ++t)
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) b.lo[a] = std::fmin(b.lo[a], s.vtx(t, k, a)), b.hi[a] = std::fmax(b.hi[a], s.vtx(t, k, a));
  return b;
}
// body(first, end) for every maximal run of consecutive triangles with one material id, in index order while more() holds
template <class More, class Body>
void cullRuns(CullSoup const& s, More more, Body body) {
  for (uint32_t first = 0, end = 0; first < s.n && more(); first = end) {
    for (end = first + 1; end < s.n && s.mat[end] == s.mat[first];) ++end;
    body(first, end);
  }
}

// A candidate is a maximal run of consecutive triangles with one material id (one mesh of the scene front-ends) of at least
// kCullMinTris triangles.  Its bound is the sphere around the centre of its vertex box through the farthest vertex, inflated
// by 1/1024 of the radius plus 1e-6 of (|centre|_max + radius): far more than mt_valid's 1e-7 barycentric slack (1e-7 of an
// edge), the float rounding of the centre and of e0 / e1, and the squared radius is rounded up.  It is culled when that
// radius is at most kCullMaxRadiusFrac of the scene's bounding-box diagonal; in index order while at most kCullMaxSphereClusters
// clusters and kCullMaxSphereTris triangles are taken.  The device test adds a relative margin of its own
// (kCullRel) for the rounding of the segment-sphere test and of the Moeller-Trumbore hit point.
constexpr uint32_t kCullMinTris = 4;
constexpr double kCullMaxRadiusFrac = 0.125;
constexpr uint32_t kCullMaxSphereClusters = 4, kCullMaxSphereTris = 32;
std::vector<CullCluster> planBruteCull(CullSoup const& s, bool enable, std::vector<float>* radii) {
  std::vector<CullCluster> out;
  if (!enable || s.n == 0) return out;
  CullBox const sc = cullBounds(s, 0, s.n);
  double const diag = std::sqrt((sc.hi[0] - sc.lo[0]) * (sc.hi[0] - sc.lo[0]) + (sc.hi[1] - sc.lo[1]) * (sc.hi[1] - sc.lo[1]) + (sc.hi[2] - sc.lo[2]) * (sc.hi[2] - sc.lo[2]));
  if (!std::isfinite(diag)) return out;
  uint32_t culled = 0;
  cullRuns(s, [&] { return out.size() < kCullMaxSphereClusters; }, [&](uint32_t first, uint32_t end) {
    uint32_t const count = end - first;
    if (count < kCullMinTris || culled + count > kCullMaxSphereTris) return;
    CullBox const b = cullBounds(s, first, end);
    float const c[3] = {float(0.5 * (b.lo[0] + b.hi[0])), float(0.5 * (b.lo[1] + b.hi[1])), float(0.5 * (b.lo[2] + b.hi[2]))};
    double r2 = 0.0;
    for (uint32_t t = first; t < end; ++t)
      for (int k = 0; k < 3; ++k) {
        double const dx = s.vtx(t, k, 0) - c[0], dy = s.vtx(t, k, 1) - c[1], dz = s.vtx(t, k, 2) - c[2];
        r2 = std::fmax(r2, dx * dx + dy * dy + dz * dz);
      }
    double const cmax = std::fmax(std::fabs(double(c[0])), std::fmax(std::fabs(double(c[1])), std::fabs(double(c[2]))));
    double const r = std::sqrt(r2) * (1.0 + 1.0 / 1024) + 1e-6 * (cmax + std::sqrt(r2));
    if (!(r <= kCullMaxRadiusFrac * diag)) return;
    CullCluster cl{};
    cl.b[0] = c[0], cl.b[1] = c[1], cl.b[2] = c[2];
    cl.b[3] = std::nextafter(float(r * r), HUGE_VALF);
    cl.first = first, cl.count = count, cl.slot = culled;
    cl.magic = uint32_t(((uint64_t(1) << 32) + count - 1) / count);
    out.push_back(cl);
    if (radii) radii->push_back(float(r));
    culled += count;
  });
  return out;
}
// Box clusters: a maximal one-material run of at least kCullBoxMinTris triangles that planBruteCull did not take -- the sphere
// rule rejects flat meshes such as walls, whose sphere holds most of the scene.  Its bound is its vertex box with every face
// moved out by m = 2^-19 (extent + |coordinate|_max of the box), then rounded outward to float.  m covers, with a margin of
// about 8:
//  * mt_valid's slack: it accepts u, v >= -1e-7 and u + v <= 1 + 1e-7, i.e. points up to 1e-7 (|e0| + |e1|) <= 3.5e-7 extent
//    outside the triangle;
//  * e0 / e1 are stored as floats: the tested triangle's vertices are up to 2^-24 |e| <= 1.1e-7 extent off the soup's;
//  * the rounding of the Moeller-Trumbore arithmetic across the ray: a few ulps of the coordinates, 2^-22 |coordinate|_max.
// Along the ray the device allows for its own rounding: the segment runs from kCullTLo = (1 - 2^-8) 1e-4 to the end t
// times kCullTSlack = 1 + 2^-8, and the slab test keeps near <= far * kCullTSlack + 2 E (cull_ray: the error term of its
// centre / half-width arithmetic, which also takes m / 16 of the inflation).  A wall is 2m thick after inflation, m well
// below kCullTLo: a ray leaving it at more than ~m / 1e-4 rad to its plane (Cornell: 0.057) gets it again only through E.
// The record stores the box as centre and half-width, the half-width rounded up until [c - hw, c + hw] holds the box.
// A run becomes a cluster when its box (before inflation) has a surface area of at most kCullBoxMaxAreaFrac of the scene
// box's: a random line that meets the scene box meets a convex body inside it with probability S_body / S_scene (Cauchy),
// and a compacted test costs about 2.7 packed ones.  Cornell's walls are exactly 1/3.  Clusters are taken in
// index order while the total stays within kCullMaxClusters clusters and kCullMaxTris triangles (the LDS copy).
constexpr uint32_t kCullBoxMinTris = 2;  // the task decode needs count >= 2; a lone triangle costs about one bound test anyway
constexpr double kCullBoxMaxAreaFrac = 0.35;
std::vector<CullCluster> planBruteCullBox(CullSoup const& s, std::vector<CullCluster> const& spheres, std::vector<float>* planBox = nullptr) {
  std::vector<CullCluster> out;
  if (s.n == 0) return out;
  auto area = [](double const lo[3], double const hi[3]) {
    double const x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
    return 2.0 * (x * y + y * z + z * x);
  };
  CullBox const sc = cullBounds(s, 0, s.n);
  double const sceneArea = area(sc.lo, sc.hi);
  if (!std::isfinite(sceneArea) || !(sceneArea > 0.0)) return out;
  uint32_t culled = 0;
  for (CullCluster const& c : spheres) culled += c.count;
  size_t const taken = spheres.size();
  cullRuns(s, [&] { return taken + out.size() < kCullMaxClusters; }, [&](uint32_t first, uint32_t end) {
    uint32_t const count = end - first;
    if (count < kCullBoxMinTris || culled + count > kCullMaxTris) return;
    if (std::any_of(spheres.begin(), spheres.end(), [&](CullCluster const& c) { return c.first == first; })) return;
    CullBox const bx = cullBounds(s, first, end);
    double const *const blo = bx.lo, *const bhi = bx.hi;
    if (!(area(blo, bhi) <= kCullBoxMaxAreaFrac * sceneArea)) return;
    double ext = 0.0, cmax = 0.0;
    for (int a = 0; a < 3; ++a)
      ext = std::fmax(ext, bhi[a] - blo[a]), cmax = std::fmax(cmax, std::fmax(std::fabs(blo[a]), std::fabs(bhi[a])));
    double const m = 0x1p-19 * (ext + cmax);
    CullCluster cl{};
    float pl[3], ph[3];
    bool holds = true;
    for (int a = 0; a < 3; ++a) {
      float l = float(blo[a] - m), h = float(bhi[a] + m);
      if (double(l) > blo[a] - m) l = std::nextafter(l, -HUGE_VALF);
      if (double(h) < bhi[a] + m) h = std::nextafter(h, HUGE_VALF);
      pl[a] = l, ph[a] = h;
      // the record: centre and half-width with [c - hw, c + hw] holding [l, h] in exact arithmetic.  The doubles below
      // are within 2^-53 of the exact values, the float above them plus one more step is 2^-24 beyond.
      float const c = float(0.5 * (double(l) + double(h)));
      double const hd = std::fmax(double(c) - double(l), double(h) - double(c));
      float hw = float(hd);
      if (double(hw) < hd) hw = std::nextafter(hw, HUGE_VALF);
      hw = std::nextafter(hw, HUGE_VALF);
      holds = holds && std::isfinite(c) && std::isfinite(hw) && (long double)c - (long double)hw <= (long double)l &&
              (long double)c + (long double)hw >= (long double)h;
      cl.b[a] = c, cl.b[3 + a] = hw;
    }
    assert(holds);
    if (!holds) return;  // (NDEBUG builds) the run stays in the always list
    if (planBox) planBox->insert(planBox->end(), {pl[0], pl[1], pl[2], ph[0], ph[1], ph[2]});
    cl.box = 1;
    cl.first = first, cl.count = count, cl.slot = culled;
    cl.magic = uint32_t(((uint64_t(1) << 32) + count - 1) / count);
    out.push_back(cl);
    culled += count;
  });
  return out;
}

// the culled clusters of the brute-force pass for a soup, by the DMT_BRUTE_CULL level: 0 none, 1 sphere clusters, 2 both
std::vector<CullCluster> planCullClusters(int level, CullSoup const& s) {
  // a closest-hit key holds the original index in 26 bits: no culling for larger soups
  std::vector<CullCluster> clusters = planBruteCull(s, level >= 1 && s.n < kCullMaxIndex, nullptr);
  if (level >= 2 && s.n < kCullMaxIndex) {
    std::vector<CullCluster> const boxes = planBruteCullBox(s, clusters);
    clusters.insert(clusters.end(), boxes.begin(), boxes.end());
  }
  return clusters;
}

}  // namespace
