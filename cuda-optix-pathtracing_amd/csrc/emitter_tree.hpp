// emitter_tree.hpp -- a light BVH whose leaves are emissive triangles as well as point and spot lights: importance-sampled
// next-event estimation over `[uploaded lights..., emissive triangles...]` instead of the uniform pick among them
// (dmt_set_emitter_sampling).
//
// What it follows: the light BVH of pbrt-v4 as its book describes it (Pharr, Jakob, Humphreys, "Physically Based Rendering",
// 4th ed., 12.6.3, after Conty & Kulla 2018), restated here: bounds with a cone of emission directions, the importance of a
// cluster seen from a shading point, a binned split by flux x orientation x area, selection by walking down the tree with a
// remapped random number, and the probability of a given emitter as the product of the choices on its root path.  That is the
// source surface_device.hpp names for the emitters themselves.  It is NOT light_tree_ref.hpp, whose clamps are the reference
// project's "as written".  One deliberate difference from pbrt: the squared distance is clamped against the SQUARED half
// diagonal of the box (pbrt clamps a squared distance against a length, mixed units).
//
// Emitters.  Index i < lightCount is record i of the light list (point or spot), otherwise emissive triangle
// areaTri[i - lightCount]: the numbering path_shade's uniform pick already uses.
//   triangle   box of its corners, axis n = normalize(cross(p1 - p0, p2 - p0)) (the side area_sample emits to), cos theta_o = 1,
//              phi = pi * luminance(Le) * area; a zero-area or zero-radiance triangle has phi = 0: never selected, pmf 0
//   light      box = position +- radius, cos theta_o = -1 (every direction: the megakernel's spot light does not attenuate, see
//              light_tree.hpp), phi = 4 pi luminance(I) as light_tree::itemOf
// theta_e = pi / 2 for every emitter, a constant that is not stored.  Emission is one-sided.
//
// Node, 48 bytes, 16-byte aligned, three quads that the walk reads with one dwordx4 load each:
//   quad 0   lo.x lo.y lo.z phi
//   quad 1   hi.x hi.y hi.z ref     ref: leaf = kEmitterLeaf | emitter index; inner = index of the left child, right = left + 1
//   quad 2   axis.x axis.y axis.z cos theta_o    the cone axis as three floats: nothing is quantised, host and device read the
//                                                same bits, and the builder rounds cos theta_o DOWN so that the stored cone of
//                                                a node holds the stored cones of its children
// nodes[0] is the root.  The two children of a node are adjacent (96 bytes from a 16-byte aligned address): et_step issues
// their six dwordx4 loads together before the first use, and the chosen child's `ref` is among them, so a level costs ONE
// dependent round trip.  Beside the nodes, indexed by emitter: the bit trail of its leaf (bit k = the choice at level k from
// the root, 0 left, 1 right) and the trail's length, 16 bytes per emitter (EmitterTrail), which et_pmf follows.
//
// Shared by the host (builder, host-only calls, tests) and the device (et_select, et_pmf): plain functions.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "light_tree.hpp"      // light_tree::itemOf
#include "light_tree_ref.hpp"  // kLightTreeNumBins

#if defined(__HIPCC__)
#define DMT_ET_HD __host__ __device__ inline
#else
#define DMT_ET_HD inline
#endif

namespace dmt {

struct alignas(16) EmitterQuad {
  float x, y, z, w;
};
struct alignas(16) EmitterNode {  // 48 B
  EmitterQuad a;  // lo.xyz, phi
  EmitterQuad b;  // hi.xyz, ref (its bits: et_bits / et_float)
  EmitterQuad c;  // axis.xyz, cos theta_o
};
static_assert(sizeof(EmitterNode) == 48 && alignof(EmitterNode) == 16, "emitter tree node: three quads");
struct alignas(16) EmitterTrail {  // 16 B, one per emitter
  uint32_t lo, hi;                 // bits 0..31 and 32..63 of the trail
  uint32_t length;                 // levels below the root
  uint32_t pad;
};
static_assert(sizeof(EmitterTrail) == 16, "emitter trail record");
constexpr uint32_t kEmitterLeaf = 0x80000000u;
// The deepest tree (in levels, a lone leaf = 1) a context uploads: trails of at most 59 bits, and the walks' guard of 64
// iterations leaves four to spare, as lt_select's does.  A deeper tree keeps the uniform pick (light_state.hpp).
constexpr int kEmitterTreeMaxDepth = 60;
static_assert(kEmitterTreeMaxDepth <= 64, "a trail has 64 bits");

DMT_ET_HD uint32_t et_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
DMT_ET_HD float et_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// Importance of a node (its three quads) at shading point p with normal n.  See the header for the terms.
DMT_ET_HD float et_importance(EmitterQuad const a, EmitterQuad const b, EmitterQuad const c, float px, float py, float pz, float nx,
                              float ny, float nz) {
  float const cx = 0.5f * (a.x + b.x), cy = 0.5f * (a.y + b.y), cz = 0.5f * (a.z + b.z);
  float const dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  float const radius2 = 0.25f * (dx * dx + dy * dy + dz * dz);  // squared half diagonal
  float wx = px - cx, wy = py - cy, wz = pz - cz;
  float const len2 = wx * wx + wy * wy + wz * wz;
  float const d2 = fmaxf(fmaxf(len2, radius2), 1e-20f);  // squared against squared; the floor: ADVICE round 3
  float sinB = 0.f, cosB = -1.f;                         // p inside the bounding sphere: the cluster is all around
  if (len2 >= radius2 && len2 > 0.f) {
    float const s2 = radius2 / len2;
    sinB = sqrtf(s2), cosB = sqrtf(fmaxf(0.f, 1.f - s2));
  }
  float const inv = len2 > 0.f ? 1.f / sqrtf(len2) : 0.f;
  wx *= inv, wy *= inv, wz *= inv;
  float const cosW = c.x * wx + c.y * wy + c.z * wz;  // one-sided emission: no absolute value
  float const sinW = sqrtf(fmaxf(0.f, 1.f - cosW * cosW));
  float const cosO = c.w, sinO = sqrtf(fmaxf(0.f, 1.f - cosO * cosO));
  float cosX = 1.f, sinX = 0.f;  // theta_x = max(0, theta_w - theta_o)
  if (!(cosW > cosO)) cosX = cosW * cosO + sinW * sinO, sinX = sinW * cosO - cosW * sinO;
  float const cosP = cosX > cosB ? 1.f : cosX * cosB + sinX * sinB;  // theta' = max(0, theta_x - theta_b)
  if (!(cosP > 0.f)) return 0.f;                                    // beyond theta_e = pi / 2 (NaN too)
  float const cosI = fabsf(wx * nx + wy * ny + wz * nz);            // transmission reaches emitters behind the surface
  float const sinI = sqrtf(fmaxf(0.f, 1.f - cosI * cosI));
  float const cosIB = cosI > cosB ? 1.f : cosI * cosB + sinI * sinB;
  return fmaxf(a.w * cosP * cosIB / d2, 0.f);
}

// One level: the probability p0 of the left one of the two children at `left`, and both children's refs.  False when neither
// has importance here.  The six loads stand together ahead of the arithmetic.
DMT_ET_HD bool et_step(EmitterNode const* nodes, uint32_t left, float px, float py, float pz, float nx, float ny, float nz, float& p0,
                       uint32_t& refL, uint32_t& refR) {
  EmitterNode const* const q = nodes + left;
  EmitterQuad const a0 = q[0].a, b0 = q[0].b, c0 = q[0].c, a1 = q[1].a, b1 = q[1].b, c1 = q[1].c;
  refL = et_bits(b0.w), refR = et_bits(b1.w);
  float const i0 = et_importance(a0, b0, c0, px, py, pz, nx, ny, nz);
  float const i1 = et_importance(a1, b1, c1, px, py, pz, nx, ny, nz);
  float const sum = i0 + i1;
  p0 = 0.f;
  if (!(sum > 0.f)) return false;
  p0 = i0 / sum;
  return true;
}
// the root: its ref, and whether a lone leaf has importance at (p, n)
DMT_ET_HD uint32_t et_root(EmitterNode const* nodes, float px, float py, float pz, float nx, float ny, float nz, bool& lone) {
  EmitterQuad const a = nodes[0].a, b = nodes[0].b, c = nodes[0].c;
  uint32_t const ref = et_bits(b.w);
  lone = (ref & kEmitterLeaf) && et_importance(a, b, c, px, py, pz, nx, ny, nz) > 0.f;
  return ref;
}

// Walk from the root to one emitter, choosing a child in proportion to its importance, u remapped at every level.  Returns
// the emitter index and its probability, or -1 (pmf 0) where no emitter has importance, or where the guard ends the walk.
DMT_ET_HD int et_select(EmitterNode const* nodes, float px, float py, float pz, float nx, float ny, float nz, float u, float& pmf) {
  bool lone;
  uint32_t ref = et_root(nodes, px, py, pz, nx, ny, nz, lone);
  pmf = 1.f;
  if (ref & kEmitterLeaf) {
    if (lone) return int(ref & ~kEmitterLeaf);
    pmf = 0.f;
    return -1;
  }
  for (int guard = 0; guard < 64; ++guard) {
    float p0;
    uint32_t refL, refR;
    if (!et_step(nodes, ref, px, py, pz, nx, ny, nz, p0, refL, refR)) break;
    if (u < p0) {
      pmf *= p0;
      u = fminf(u / p0, 0.99999994f);
      ref = refL;
    } else {
      pmf *= 1.f - p0;
      u = fminf((u - p0) / (1.f - p0), 0.99999994f);
      ref = refR;
    }
    if (ref & kEmitterLeaf) return int(ref & ~kEmitterLeaf);
  }
  pmf = 0.f;
  return -1;
}

// The probability with which et_select returns the emitter whose trail this is, at (p, n): the same child probabilities
// multiplied in the same order, so for the emitter et_select returned it is the same float bit for bit.  0 where the trail
// does not end at a leaf.
DMT_ET_HD float et_pmf(EmitterNode const* nodes, EmitterTrail const trail, float px, float py, float pz, float nx, float ny, float nz) {
  bool lone;
  uint32_t ref = et_root(nodes, px, py, pz, nx, ny, nz, lone);
  if (ref & kEmitterLeaf) return lone && trail.length == 0u ? 1.f : 0.f;
  float pmf = 1.f;
  uint32_t const length = trail.length < 64u ? trail.length : 64u;
  for (uint32_t k = 0; k < length; ++k) {
    if (ref & kEmitterLeaf) return 0.f;
    float p0;
    uint32_t refL, refR;
    if (!et_step(nodes, ref, px, py, pz, nx, ny, nz, p0, refL, refR)) return 0.f;
    bool const right = (((k < 32u ? trail.lo : trail.hi) >> (k & 31u)) & 1u) != 0u;
    if (right) pmf *= 1.f - p0, ref = refR;
    else pmf *= p0, ref = refL;
  }
  return (ref & kEmitterLeaf) ? pmf : 0.f;
}

namespace emitter_tree {

struct Item {
  float lo[3], hi[3], phi, axis[3], cosO;
  uint32_t index;
};

// ---- direction cones, in double (the builder only) ----
struct Cone {
  double w[3] = {0, 0, 1};
  double theta = 0;  // half angle; >= pi: the whole sphere
  bool empty = true;
};
constexpr double kPi = 3.14159265358979323846;
inline double angleBetween(double const a[3], double const b[3]) {
  double const cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  return std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}
inline Cone coneOf(float const axis[3], float cosO) {
  Cone c;
  c.empty = false;
  for (int k = 0; k < 3; ++k) c.w[k] = axis[k];
  c.theta = cosO <= -1.f ? kPi : std::acos(std::min(1.0, double(cosO)));
  return c;
}
// pbrt's DirectionCone::Union: one holds the other, the two cover the sphere, or the smallest cone around both
inline Cone coneUnion(Cone const& a, Cone const& b) {
  if (a.empty) return b;
  if (b.empty) return a;
  if (a.theta >= kPi) return a;
  if (b.theta >= kPi) return b;
  double const d = angleBetween(a.w, b.w);
  if (std::min(d + b.theta, kPi) <= a.theta) return a;
  if (std::min(d + a.theta, kPi) <= b.theta) return b;
  Cone r;
  r.empty = false;
  double const theta = 0.5 * (a.theta + d + b.theta);
  double k[3] = {a.w[1] * b.w[2] - a.w[2] * b.w[1], a.w[2] * b.w[0] - a.w[0] * b.w[2], a.w[0] * b.w[1] - a.w[1] * b.w[0]};
  double const kl = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
  if (theta >= kPi || !(kl > 0.0)) {
    r.theta = kPi;
    return r;
  }
  for (double& v : k) v /= kl;
  double const t = theta - a.theta, ct = std::cos(t), st = std::sin(t);  // a.w turned by t towards b.w, about k (k is normal to a.w)
  r.w[0] = a.w[0] * ct + (k[1] * a.w[2] - k[2] * a.w[1]) * st;
  r.w[1] = a.w[1] * ct + (k[2] * a.w[0] - k[0] * a.w[2]) * st;
  r.w[2] = a.w[2] * ct + (k[0] * a.w[1] - k[1] * a.w[0]) * st;
  r.theta = theta;
  return r;
}
// the orientation factor of the split cost, theta_e = pi / 2
inline double orientationMeasure(Cone const& c) {
  if (c.empty) return 0.0;
  double const to = std::min(c.theta, kPi), tw = std::min(to + 0.5 * kPi, kPi), so = std::sin(to), co = std::cos(to);
  return 2.0 * kPi * (1.0 - co) + 0.5 * kPi * (2.0 * tw * so - std::cos(to - 2.0 * tw) - 2.0 * to * so + co);
}

// the item of a packed point or spot light record (false: another type)
template <class HalfToFloat>
inline bool lightItem(uint8_t const* rec32, uint32_t index, HalfToFloat half, Item& it) {
  light_tree::Item l;
  if (!light_tree::itemOf(rec32, index, half, l)) return false;
  for (int k = 0; k < 3; ++k) it.lo[k] = l.pos[k] - l.radius, it.hi[k] = l.pos[k] + l.radius;
  it.phi = l.phi, it.axis[0] = 0.f, it.axis[1] = 0.f, it.axis[2] = 1.f, it.cosO = -1.f, it.index = index;
  return true;
}
// the item of an emissive triangle with corners p0, p1, p2 and radiance le
inline void triangleItem(float const p0[3], float const p1[3], float const p2[3], float const le[3], uint32_t index, Item& it) {
  for (int k = 0; k < 3; ++k) it.lo[k] = std::min(p0[k], std::min(p1[k], p2[k])), it.hi[k] = std::max(p0[k], std::max(p1[k], p2[k]));
  float const e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  float const c[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
  float const len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  float const lum = 0.2126f * le[0] + 0.7152f * le[1] + 0.0722f * le[2];
  it.index = index, it.cosO = 1.f;
  if (len > 0.f && std::isfinite(len)) {
    it.axis[0] = c[0] / len, it.axis[1] = c[1] / len, it.axis[2] = c[2] / len;
    it.phi = 3.14159265358979323846f * std::fmax(lum, 0.f) * (0.5f * len);
  } else {
    it.axis[0] = 0.f, it.axis[1] = 0.f, it.axis[2] = 1.f, it.phi = 0.f;
  }
  if (!(it.phi >= 0.f) || !std::isfinite(it.phi)) it.phi = 0.f;
}

struct Tree {
  std::vector<EmitterNode> nodes;
  std::vector<EmitterTrail> trails;  // [emitter]
  int depth = 0;                     // levels; a lone leaf = 1
};

struct BinAcc {
  double lo[3], hi[3], phi = 0;
  Cone cone;
  size_t count = 0;
  BinAcc() {
    for (int k = 0; k < 3; ++k) lo[k] = INFINITY, hi[k] = -INFINITY;
  }
  void add(Item const& it) {
    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], double(it.lo[k])), hi[k] = std::max(hi[k], double(it.hi[k]));
    phi += it.phi, ++count;
    cone = coneUnion(cone, coneOf(it.axis, it.cosO));
  }
  void add(BinAcc const& o) {
    if (!o.count) return;
    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], o.lo[k]), hi[k] = std::max(hi[k], o.hi[k]);
    phi += o.phi, count += o.count;
    cone = coneUnion(cone, o.cone);
  }
  double cost() const {  // phi x M_omega x area (K_r is the caller's)
    double const dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return phi * orientationMeasure(cone) * 2.0 * (dx * dy + dy * dz + dz * dx);
  }
};
inline float centroid(Item const& it, int axis) { return 0.5f * (it.lo[axis] + it.hi[axis]); }
inline int binOf(float c, float cmin, float cmax) {
  int const b = int(float(kLightTreeNumBins) * ((c - cmin) / (cmax - cmin)));
  return b < 0 ? 0 : b >= kLightTreeNumBins ? kLightTreeNumBins - 1 : b;
}

// nodes[0] = root; no emitters -> an empty tree.  O(n log n): every node bins its emitters once per axis and partitions
// them in place.  Deterministic.  An explicit stack, no recursion; trails are recorded while the depth fits their 64 bits.
inline Tree build(std::vector<Item> items) {
  Tree T;
  if (items.empty()) return T;
  size_t const n = items.size();
  T.trails.assign(n, EmitterTrail{0u, 0u, 0u, 0u});
  T.nodes.reserve(2 * n - 1);
  struct Work {
    uint32_t node;
    size_t a, b;
    int depth;
    uint64_t trail;
  };
  T.nodes.emplace_back();
  std::vector<Work> stack{{0u, 0, n, 1, 0ull}};
  while (!stack.empty()) {
    Work const w = stack.back();
    stack.pop_back();
    T.depth = std::max(T.depth, w.depth);
    EmitterNode nd{};
    if (w.b - w.a == 1) {
      Item const& it = items[w.a];
      nd.a = {it.lo[0], it.lo[1], it.lo[2], it.phi};
      nd.b = {it.hi[0], it.hi[1], it.hi[2], et_float(kEmitterLeaf | it.index)};
      nd.c = {it.axis[0], it.axis[1], it.axis[2], it.cosO};
      T.nodes[w.node] = nd;
      if (it.index < n) T.trails[it.index] = EmitterTrail{uint32_t(w.trail), uint32_t(w.trail >> 32), uint32_t(w.depth - 1), 0u};
      continue;
    }
    // the node's box and flux now; its cone after the build, from its children's stored ones (below)
    float cmin[3], cmax[3], blo[3], bhi[3];
    double phi = 0;
    for (int k = 0; k < 3; ++k) blo[k] = INFINITY, bhi[k] = -INFINITY, cmin[k] = INFINITY, cmax[k] = -INFINITY;
    for (size_t i = w.a; i < w.b; ++i) {
      for (int k = 0; k < 3; ++k) {
        blo[k] = std::min(blo[k], items[i].lo[k]), bhi[k] = std::max(bhi[k], items[i].hi[k]);
        float const c = centroid(items[i], k);
        cmin[k] = std::min(cmin[k], c), cmax[k] = std::max(cmax[k], c);
      }
      phi += items[i].phi;
    }
    double const ext[3] = {double(bhi[0]) - blo[0], double(bhi[1]) - blo[1], double(bhi[2]) - blo[2]};
    double const maxExt = std::max(ext[0], std::max(ext[1], ext[2]));
    int bestAxis = -1, bestBin = -1;
    double bestCost = INFINITY;
    for (int axis = 0; axis < 3; ++axis) {
      if (!(cmax[axis] > cmin[axis]) || !std::isfinite(cmax[axis] - cmin[axis])) continue;  // no boundary separates the centroids
      BinAcc bins[kLightTreeNumBins];
      for (size_t i = w.a; i < w.b; ++i) bins[binOf(centroid(items[i], axis), cmin[axis], cmax[axis])].add(items[i]);
      double rightCost[kLightTreeNumBins];
      BinAcc acc;
      for (int b = kLightTreeNumBins - 1; b >= 1; --b) acc.add(bins[b]), rightCost[b] = acc.cost();
      double const kr = maxExt / ext[axis];
      BinAcc left;
      for (int b = 0; b + 1 < kLightTreeNumBins; ++b) {  // the split after bin b
        left.add(bins[b]);
        if (left.count == 0 || left.count == w.b - w.a) continue;
        double const cost = (left.cost() + rightCost[b + 1]) * kr;
        if (cost < bestCost * (1.0 - 1e-9)) bestCost = cost, bestAxis = axis, bestBin = b;  // first clearly better split wins
      }
    }
    size_t mid;
    if (bestAxis >= 0) {
      int const ax = bestAxis, bb = bestBin;
      float const lo = cmin[ax], hi = cmax[ax];
      mid = size_t(std::stable_partition(items.begin() + long(w.a), items.begin() + long(w.b),
                                         [=](Item const& it) { return binOf(centroid(it, ax), lo, hi) <= bb; }) - items.begin());
    } else {  // coincident centroids, or no cost that compares: the median in (centroid, index) order
      std::sort(items.begin() + long(w.a), items.begin() + long(w.b), [](Item const& x, Item const& y) {
        for (int k = 0; k < 3; ++k) {
          float const cx = centroid(x, k), cy = centroid(y, k);
          if (cx < cy) return true;
          if (cy < cx) return false;
        }
        return x.index < y.index;
      });
      mid = w.a + (w.b - w.a) / 2;
    }
    uint32_t const left = uint32_t(T.nodes.size());
    T.nodes.emplace_back(), T.nodes.emplace_back();
    nd.a = {blo[0], blo[1], blo[2], float(phi)};
    nd.b = {bhi[0], bhi[1], bhi[2], et_float(left)};
    nd.c = {0.f, 0.f, 1.f, -1.f};
    T.nodes[w.node] = nd;
    uint64_t const bit = w.depth - 1 < 64 ? 1ull << (w.depth - 1) : 0ull;
    stack.push_back({left + 1u, mid, w.b, w.depth + 1, w.trail | bit});
    stack.push_back({left, w.a, mid, w.depth + 1, w.trail});
  }
  // cones, children before parents (a child's index is above its parent's): the union of the children's STORED cones, its
  // axis rounded to float, then the half angle that holds both children about that rounded axis, its cosine rounded down
  for (size_t i = T.nodes.size(); i-- > 0;) {
    EmitterNode& nd = T.nodes[i];
    uint32_t const ref = et_bits(nd.b.w);
    if (ref & kEmitterLeaf) continue;
    EmitterNode const& l = T.nodes[ref];
    EmitterNode const& r = T.nodes[ref + 1u];
    float const la[3] = {l.c.x, l.c.y, l.c.z}, ra[3] = {r.c.x, r.c.y, r.c.z};
    Cone const cl = coneOf(la, l.c.w), cr = coneOf(ra, r.c.w);
    Cone const u = coneUnion(cl, cr);
    double const len = std::sqrt(u.w[0] * u.w[0] + u.w[1] * u.w[1] + u.w[2] * u.w[2]);
    nd.c = {float(u.w[0] / len), float(u.w[1] / len), float(u.w[2] / len), -1.f};
    if (u.theta < kPi) {
      double const ax[3] = {nd.c.x, nd.c.y, nd.c.z};
      double const theta = std::max(angleBetween(ax, cl.w) + cl.theta, angleBetween(ax, cr.w) + cr.theta);
      if (theta < kPi) {
        double const c = std::cos(theta);
        float f = float(c);
        if (double(f) > c) f = std::nextafter(f, -2.f);
        nd.c.w = std::max(f, -1.f);
      }
    }
  }
  return T;
}

// probability of every emitter at (p, n): et_pmf along its trail
inline void pmfs(Tree const& T, float const p[3], float const n[3], float* out) {
  for (size_t i = 0; i < T.trails.size(); ++i)
    out[i] = T.nodes.empty() ? 0.f : et_pmf(T.nodes.data(), T.trails[i], p[0], p[1], p[2], n[0], n[1], n[2]);
}

}  // namespace emitter_tree
}  // namespace dmt
