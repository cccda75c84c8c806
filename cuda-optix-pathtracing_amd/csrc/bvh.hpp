// bvh.hpp -- 4-wide BVH: node / leaf layout (shared host/device) and the host builder.
//
// Semantics follow the reference's only BVH, the CPU renderer's: binned-SAH splits,
// small leaves, wide nodes obtained by collapsing binary splits (src/core/private/core-bvh-builder.cpp:58-223
// builds an 8-ary tree the same way, 16-128 bins, leaves <= 7).  The LAYOUT is designed for what bounds per-lane
// traversal on gfx950: the vector-memory front end.  tools/ubench/gather.hip (a dependent per-lane gather like a
// traversal's) measures, chip-wide, for records served by L2:
//     128-byte record, 7 x 16-byte loads per lane     88 G lane-steps/s   (round 1's node)
//     128-byte record, 5 loads                       121                  (round 1's triangle pair)
//      64-byte slot, 4 loads                         214
//      64-byte slot, 3 loads                         290                  (this node)
//      80-byte record, 5 loads                       178                  (this triangle pair)
// i.e. a step costs ~max(0.7 x loads, 64-byte sectors touched x 64 / 26) clocks of the CU's L1 path, whatever the
// occupancy; round 1's kernel ran at 75 % of the first two rates.  So:
//   * Bvh4Node = 48 bytes of payload in a 64-byte slot (one sector, three loads): the children's boxes are
//     quantised to 8 bits per plane relative to the node's own box (origin + power-of-two scale per axis) and child
//     references are implicit (inner children contiguous from childBase, leaves contiguous from the pair leafRef names).
//   * TriPair = 80 bytes (five loads): two triangles interleaved component by component for packed math.
//
// Correctness contract (tests/test_parity_gpu.py::test_bvh_*): traversal returns exactly the brute-force closest hit
// -- same triangle (lowest ORIGINAL index on equal t) and bit-identical (t,u,v), because the same Moeller-Trumbore
// routine runs on the same fp32 triangle record -- and the same any-hit answer.  Boxes only cull: triangle boxes are
// padded so that a ray the triangle test accepts can never be culled, and quantisation only ever GROWS a box (lo rounded
// down, hi rounded up, in exact arithmetic: origin and scale are floats, q * scale is exact).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "lbvh.hpp"

namespace dmt {

constexpr uint32_t kBvhLeafFlag = 0x80000000u;
constexpr uint32_t kBvhEmpty = 0xFFFFFFFFu;
constexpr int kBvhMaxLeafTris = 2;   // one triangle pair per leaf: measured best (1 M random triangles: 405 vs 391 Msamples/s for 4)
constexpr int kBvhMaxDepth = 48;   // depth bound (binary levels, hence also 4-wide levels) enforced by the builder
#ifndef DMT_BVH_LDS_STACK
#define DMT_BVH_LDS_STACK 16  // tests build a variant with 2 so that every non-trivial traversal runs through the global overflow stack
#endif
constexpr int kBvhLdsStack = DMT_BVH_LDS_STACK;   // traversal stack entries kept in LDS per lane
constexpr int kBvhOverflowStack = 3 * kBvhMaxDepth - kBvhLdsStack;  // the rest, per lane, in global memory

// traversal-stack entry / current position: kBvhEmpty | inner node index | kBvhLeafFlag | pair index
inline uint32_t bvhLeafRef(uint32_t pair) { return kBvhLeafFlag | pair; }

// Leaf storage on the device: two triangles interleaved component by component, so that the 16-byte loads
// deliver (first, second) register pairs ready for packed math.  A leaf is ONE pair; a one-triangle leaf repeats its
// triangle (same original index, so the repeated test can never win the tie-break against itself).
struct TriPair {  // 80 B = five 16-byte loads
  float p0x[2], p0y[2], p0z[2], e0x[2], e0y[2], e0z[2], e1x[2], e1y[2], e1z[2];
  uint32_t orig[2];  // ORIGINAL triangle indices (brute-force tie-break, shading)
};
static_assert(sizeof(TriPair) == 80, "pair size");
// Motion blur (dmt_set_motion): D = B - A of a pair's nine float fields, A the key-0 pair and B the pair
// packed from the key-1 positions, in the same interleaving.  A leaf of the motion tree loads both records and tests
// fmaf(t, D, A).  Like the pair array it carries three guard records behind its end (buildBvhHost).
struct TriPairDelta {  // 80 B = five 16-byte loads
  float p0x[2], p0y[2], p0z[2], e0x[2], e0y[2], e0z[2], e1x[2], e1y[2], e1z[2];
  uint32_t pad[2];
};
static_assert(sizeof(TriPairDelta) == 80, "pair delta size");

// Inner node.  Child k (k < count) has the box  [origin + qlo_k * scale, origin + qhi_k * scale]  per axis, with
// scale_axis = 2^(exp_axis - 127) and the q's the k-th BYTES of the six plane words.  Children 0 .. inner-1 are the inner
// nodes childBase + k; children inner .. count-1 are the leaves (triangle pairs) with the REFERENCES leafRef + k, where
// leafRef = first pair - inner + kBvhLeafFlag (modulo 2^32): a slot's reference is one add from either base (bvh_device.hpp).
struct Bvh4Node {  // 64-byte slot, 48 bytes read (three 16-byte loads)
  float ox, oy, oz;       // quantisation origin = lower corner of the node's box
  uint32_t meta;          // byte 0-2: biased power-of-two exponent of the x / y / z scale; byte 3: inner | count << 4
  uint32_t childBase;     // first inner child
  uint32_t leafRef;       // flagged reference of leaf slot k, minus k:  first pair - inner + kBvhLeafFlag  (mod 2^32)
  uint32_t qlox, qhix;    // byte k: child k's quantised planes
  uint32_t qloy, qhiy, qloz, qhiz;
  uint32_t pad[4];
};
static_assert(sizeof(Bvh4Node) == 64, "node size");

inline int bvhNodeInner(Bvh4Node const& n) { return int((n.meta >> 24) & 0xFu); }
inline int bvhNodeCount(Bvh4Node const& n) { return int((n.meta >> 28) & 0xFu); }
inline float bvhNodeScale(Bvh4Node const& n, int axis) {
  uint32_t const bits = ((n.meta >> (8 * axis)) & 0xFFu) << 23;
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
// decoded box of child k (host side: validation and tests; the device never forms the planes, see bvh_device.hpp)
inline void bvhChildBox(Bvh4Node const& n, int k, float lo[3], float hi[3]) {
  uint32_t const ql[3] = {n.qlox, n.qloy, n.qloz}, qh[3] = {n.qhix, n.qhiy, n.qhiz};
  float const o[3] = {n.ox, n.oy, n.oz};
  for (int a = 0; a < 3; ++a) {
    float const s = bvhNodeScale(n, a);
    lo[a] = o[a] + float((ql[a] >> (8 * k)) & 0xFFu) * s;
    hi[a] = o[a] + float((qh[a] >> (8 * k)) & 0xFFu) * s;
  }
}

namespace bvh_build {

using Box = lbvh::Box;  // lbvh.hpp: the same reset / grow / area, usable in kernels

struct Node2 {  // binary build node
  Box box;
  int left = -1, right = -1;  // inner
  uint32_t first = 0, count = 0;  // leaf range in `order`
  bool leaf() const { return left < 0; }
};

struct Builder {
  std::vector<Box> triBox;
  std::vector<float> centroid;  // 3 per triangle
  std::vector<uint32_t> order;
  std::vector<Node2> nodes;

  static int ceilLog2(uint32_t v) {
    int l = 0;
    while ((1u << l) < v) ++l;
    return l;
  }

  // depthBudget: binary levels still allowed below this node (guarantees the 4-wide depth bound)
  int build(uint32_t first, uint32_t count, int depthBudget) {
    int const id = int(nodes.size());
    nodes.emplace_back();
    Box box, cbox;
    box.reset(), cbox.reset();
    for (uint32_t i = first; i < first + count; ++i) {
      box.grow(triBox[order[i]]);
      cbox.grow(&centroid[3 * order[i]]);
    }
    nodes[id].box = box;
    if (count <= uint32_t(kBvhMaxLeafTris)) {
      nodes[id].first = first, nodes[id].count = count;
      return id;
    }
    int axis = 0;
    float ext = cbox.hi[0] - cbox.lo[0];
    for (int a = 1; a < 3; ++a)
      if (cbox.hi[a] - cbox.lo[a] > ext) ext = cbox.hi[a] - cbox.lo[a], axis = a;
    uint32_t mid = first + count / 2;
    bool const mustBalance = ceilLog2((count + kBvhMaxLeafTris - 1) / kBvhMaxLeafTris) >= depthBudget;
    bool split = false;
    if (!mustBalance && ext > 0.f) {  // binned SAH, best of the three axes
      constexpr int B = 16;
      float bestCost = std::numeric_limits<float>::infinity();
      int bestSplit = -1, bestAxis = -1;
      float bestK = 0.f;
      for (int ax = 0; ax < 3; ++ax) {
        float const e = cbox.hi[ax] - cbox.lo[ax];
        if (!(e > 0.f)) continue;
        Box bb[B];
        uint32_t bc[B] = {};
        for (auto& b : bb) b.reset();
        float const k = float(B) * (1.f - 1e-6f) / e;
        for (uint32_t i = first; i < first + count; ++i) {
          int b = int((centroid[3 * order[i] + ax] - cbox.lo[ax]) * k);
          b = b < 0 ? 0 : (b >= B ? B - 1 : b);
          bb[b].grow(triBox[order[i]]);
          ++bc[b];
        }
        float rightArea[B];
        uint32_t rightCnt[B];
        Box acc;
        acc.reset();
        uint32_t c = 0;
        for (int b = B - 1; b > 0; --b) {
          acc.grow(bb[b]);
          c += bc[b];
          rightArea[b] = acc.area(), rightCnt[b] = c;
        }
        acc.reset();
        c = 0;
        for (int b = 0; b < B - 1; ++b) {
          acc.grow(bb[b]);
          c += bc[b];
          if (c == 0 || rightCnt[b + 1] == 0) continue;
          float const cost = acc.area() * float(c) + rightArea[b + 1] * float(rightCnt[b + 1]);
          if (cost < bestCost) bestCost = cost, bestSplit = b, bestAxis = ax, bestK = k;
        }
      }
      if (bestSplit >= 0) {
        int const ax = bestAxis;
        float const lo = cbox.lo[ax];
        auto it = std::partition(order.begin() + first, order.begin() + first + count, [&](uint32_t t) {
          int b = int((centroid[3 * t + ax] - lo) * bestK);
          b = b < 0 ? 0 : (b >= B ? B - 1 : b);
          return b <= bestSplit;
        });
        mid = uint32_t(it - order.begin());
        split = mid > first && mid < first + count;
      }
    }
    if (!split) {  // median split on the same axis (degenerate centroids, or depth budget exhausted)
      mid = first + count / 2;
      std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                       [&](uint32_t a, uint32_t b) {
                         float const ca = centroid[3 * a + axis], cb = centroid[3 * b + axis];
                         return ca < cb || (ca == cb && a < b);
                       });
    }
    int const l = build(first, mid - first, depthBudget - 1);
    int const r = build(mid, first + count - mid, depthBudget - 1);
    nodes[id].left = l, nodes[id].right = r;
    return id;
  }
};

struct Result {
  std::vector<Bvh4Node> nodes;
  std::vector<uint32_t> pairTris;  // two ORIGINAL triangle indices per leaf pair (the second repeats the first in a one-triangle leaf)
  int depth = 0;
};

// Quantise the boxes of `nk` children (inner children first) into node `nd`.  Exact-arithmetic guarantee: the decoded
// box encloses the given one.  __host__ __device__: the device builder (bvh_gpu_build.hip) encodes with the same
// arithmetic; every operation is exact or a correctly rounded fp64 division, so host and device give the same bytes.
DMT_HD inline void encodeNode(Bvh4Node& nd, Box const* kid, int nk, int nInner) {
  memset(&nd, 0, sizeof(nd));
  Box all;
  all.reset();
  for (int k = 0; k < nk; ++k) all.grow(kid[k]);
  uint32_t ebytes[3] = {127, 127, 127};
  float org[3] = {0, 0, 0};
  double scale[3] = {1, 1, 1};
  for (int a = 0; a < 3 && nk > 0; ++a) {
    org[a] = all.lo[a];
    double const ext = double(all.hi[a]) - double(all.lo[a]);
    int e = -60;  // floor of the scale: the traversal's slope a = scale * (1 / d) must never flush to zero (bvh_device.hpp)
    if (ext > 0.0) {
      int fe;
      (void)::frexp(ext / 255.0, &fe);  // ext / 255 = m * 2^fe, m in [0.5, 1)  ->  2^fe >= ext / 255
      e = fe;
    }
    e = e < -60 ? -60 : (e > 127 ? 127 : e);
    while (e < 127 && ::ldexp(255.0, e) < ext) ++e;
    ebytes[a] = uint32_t(e + 127);
    scale[a] = ::ldexp(1.0, e);
  }
  nd.ox = org[0], nd.oy = org[1], nd.oz = org[2];
  nd.meta = ebytes[0] | (ebytes[1] << 8) | (ebytes[2] << 16) | (uint32_t(nInner) << 24) | (uint32_t(nk) << 28);
  uint32_t* const qlo[3] = {&nd.qlox, &nd.qloy, &nd.qloz};
  uint32_t* const qhi[3] = {&nd.qhix, &nd.qhiy, &nd.qhiz};
  for (int k = 0; k < 4; ++k)
    for (int a = 0; a < 3; ++a) {
      uint32_t l = 255, h = 0;  // empty slot: inverted box; NOT masked by count on the device -- see buildBvh's guard pairs
      if (k < nk) {
        double const fl = ::floor((double(kid[k].lo[a]) - double(org[a])) / scale[a]);
        double const fh = ::ceil((double(kid[k].hi[a]) - double(org[a])) / scale[a]);
        // clamp as min(max(f, 0), 255) does (a NaN gives 0)
        l = uint32_t(!(fl > 0.0) ? 0.0 : (fl > 255.0 ? 255.0 : fl));
        h = uint32_t(!(fh > 0.0) ? 0.0 : (fh > 255.0 ? 255.0 : fh));
      }
      *qlo[a] |= l << (8 * k), *qhi[a] |= h << (8 * k);
    }
}

// xs/ys/zs: the reference's SoA (4 floats per triangle: c0, c1, c2, pad).
// xs1/ys1/zs1 (all or none): a second key of the same triangles (motion blur).  Every triangle's box is then
// the UNION of its boxes at both keys, padded as one box, and the padding scale is taken over both keys.  A vertex moves on
// the segment between its keys, so the exact triangle at any t in [0, 1] lies inside the union box.  What the device tests
// is fmaf(t, D, A) with D = fl(B - A): D is off by <= 2^-24 |B - A| <= 2^-23 m (m = the box's largest |coordinate|), the
// fmaf rounds once more (2^-24 m), and the edge records add their own subtraction (2^-24 of the triangle's extent) and the
// same two steps on extents: every tested vertex p0 + e is within ~6 * 2^-24 (extent + m) = 3.6e-7 (extent + m) of the exact
// one.  padBox adds 1e-5 extent + 4e-6 m: ten times that, on top of the terms the static tree needs.
inline Result build(float const* xs, float const* ys, float const* zs, uint32_t n, float const* xs1 = nullptr, float const* ys1 = nullptr,
                    float const* zs1 = nullptr) {
  static_assert(kBvhMaxLeafTris == 2, "a leaf is one triangle pair");
  Result out;
  Builder b;
  b.triBox.resize(n), b.centroid.resize(3 * size_t(n)), b.order.resize(n);
  // largest |coordinate| of the soup: the slab arithmetic of the traversal (bvh_device.hpp: t = q a + b with b = origin inv +
  // (-o inv), two separately rounded products) errs by a few ulp of the ORIGIN-SIDE magnitudes, ~1.2e-7 (|o| + |node origin|) in
  // space, whatever the triangle's own coordinates are -- a triangle near coordinate 0 seen from far away is the case the
  // per-triangle terms below do not cover (round-2 advisor).  Rays start on the scene's surfaces or at a camera; the padding
  // allows for origins up to 8x the scene's largest |coordinate| away from the axes' zero.
  float sceneMaxAbs = 0.f;
  for (size_t k = 0; k < size_t(n) * 4; ++k) {
    if ((k & 3) == 3) continue;  // the SoA's pad lane
    sceneMaxAbs = std::max(sceneMaxAbs, std::max(std::fabs(xs[k]), std::max(std::fabs(ys[k]), std::fabs(zs[k]))));
    if (xs1) sceneMaxAbs = std::max(sceneMaxAbs, std::max(std::fabs(xs1[k]), std::max(std::fabs(ys1[k]), std::fabs(zs1[k]))));
  }
  float const slabPad = lbvh::slabPadOf(sceneMaxAbs);
  for (uint32_t i = 0; i < n; ++i) {
    Box bx;
    bx.reset();
    for (int v = 0; v < 3; ++v) {
      float const p[3] = {xs[4 * size_t(i) + v], ys[4 * size_t(i) + v], zs[4 * size_t(i) + v]};
      bx.grow(p);
      if (xs1) {
        float const q[3] = {xs1[4 * size_t(i) + v], ys1[4 * size_t(i) + v], zs1[4 * size_t(i) + v]};
        bx.grow(q);
      }
    }
    lbvh::padBox(bx, slabPad);  // the padding terms live in lbvh.hpp: the device builder pads the same way
    b.triBox[i] = bx;
    for (int a = 0; a < 3; ++a) b.centroid[3 * size_t(i) + a] = 0.5f * (bx.lo[a] + bx.hi[a]);
    b.order[i] = i;
  }
  if (n == 0) {  // a root without children
    Bvh4Node root;
    encodeNode(root, nullptr, 0, 0);
    out.nodes.push_back(root);
    return out;
  }
  b.nodes.reserve(size_t(n));
  int const root2 = b.build(0, n, kBvhMaxDepth);

  // collapse binary splits into 4-wide nodes: repeatedly open the inner child of largest area.  A node's inner
  // children get CONSECUTIVE node indices (implicit child references), processed breadth-first so that index order
  // is also level order of each subtree's top.
  struct Wide {
    int kids[4];  // binary node ids, inner children first
    int nk = 0, nInner = 0;
    int depth = 1;
  };
  std::vector<Wide> wide;
  wide.emplace_back();
  std::vector<int> source;  // binary node each wide node came from
  source.push_back(root2);
  for (size_t w = 0; w < wide.size(); ++w) {
    int const node2 = source[w];
    int kids[4];
    int nk = 0;
    if (b.nodes[size_t(node2)].leaf()) {
      kids[nk++] = node2;
    } else {
      kids[nk++] = b.nodes[size_t(node2)].left;
      kids[nk++] = b.nodes[size_t(node2)].right;
      while (nk < 4) {
        int pick = -1;
        float bestA = -1.f;
        for (int k = 0; k < nk; ++k)
          if (!b.nodes[size_t(kids[k])].leaf() && b.nodes[size_t(kids[k])].box.area() > bestA) bestA = b.nodes[size_t(kids[k])].box.area(), pick = k;
        if (pick < 0) break;
        int const open = kids[pick];
        kids[pick] = b.nodes[size_t(open)].left;
        kids[nk++] = b.nodes[size_t(open)].right;
      }
    }
    Wide W = wide[w];
    W.nk = nk;
    W.nInner = 0;
    for (int k = 0; k < nk; ++k)
      if (!b.nodes[size_t(kids[k])].leaf()) W.kids[W.nInner++] = kids[k];
    int at = W.nInner;
    for (int k = 0; k < nk; ++k)
      if (b.nodes[size_t(kids[k])].leaf()) W.kids[at++] = kids[k];
    wide[w] = W;
    out.depth = std::max(out.depth, W.depth);
    for (int k = 0; k < W.nInner; ++k) {  // consecutive indices: size() .. size() + nInner - 1
      Wide c;
      c.depth = W.depth + 1;
      wide.push_back(c);
      source.push_back(W.kids[k]);
    }
  }
  // encode in index order; leaves of a node become consecutive pairs
  out.nodes.resize(wide.size());
  uint32_t nextChild = 1;
  for (size_t w = 0; w < wide.size(); ++w) {
    Wide const& W = wide[w];
    Box kb[4];
    for (int k = 0; k < W.nk; ++k) kb[k] = b.nodes[size_t(W.kids[k])].box;
    Bvh4Node nd;
    encodeNode(nd, kb, W.nk, W.nInner);
    nd.childBase = nextChild;
    nextChild += uint32_t(W.nInner);
    nd.leafRef = uint32_t(out.pairTris.size() / 2) - uint32_t(W.nInner) + kBvhLeafFlag;
    for (int k = W.nInner; k < W.nk; ++k) {
      Node2 const& c = b.nodes[size_t(W.kids[k])];
      uint32_t const t0 = b.order[c.first], t1 = b.order[c.first + (c.count > 1 ? 1 : 0)];
      out.pairTris.push_back(t0), out.pairTris.push_back(t1);
    }
    out.nodes[w] = nd;
  }
  return out;
}

// Walks any tree in this layout over the soup xs / ys / zs (dmt_bvh_validate, dmt_bvh_check): every triangle in exactly one
// leaf, every node reached exactly once, decoded child boxes contain their vertices and nest within a quantisation step of
// the parent's, counts in range, leaves of at most kBvhMaxLeafTris triangles, depth within kBvhMaxDepth.  pairTris: the two
// ORIGINAL indices of each pair.  *depth = 4-wide levels (0 for a root without children); *sahCost = sum over all child
// slots of the decoded child box's area, a leaf slot weighted by its triangle count, over the area of the union of the
// root's child boxes.
inline bool check(Bvh4Node const* nodes, size_t nNodes, uint32_t const* pairTris, size_t npairs, float const* xs, float const* ys,
                  float const* zs, size_t count, int* depth, int* maxLeafOut, double* sahCost) {
  std::vector<uint8_t> seen(count, 0);
  std::vector<uint8_t> nodeSeen(nNodes, 0);
  int maxLeaf = 0, maxDepth = 0;
  bool ok = nNodes > 0;
  struct Item {
    uint32_t node;
    int depth;
    float lo[3], hi[3];  // decoded box of the slot this node hangs in
  };
  std::vector<Item> stack;
  float const inf = std::numeric_limits<float>::infinity();
  double areaSum = 0.0;
  Box rootBox;
  rootBox.reset();
  if (ok) stack.push_back({0u, 1, {-inf, -inf, -inf}, {inf, inf, inf}});
  while (!stack.empty() && ok) {
    Item const it = stack.back();
    stack.pop_back();
    if (it.node >= nNodes || nodeSeen[it.node]++) { ok = false; break; }
    Bvh4Node const& n = nodes[it.node];
    int const inner = bvhNodeInner(n), cnt = bvhNodeCount(n);
    if (inner > cnt || cnt > 4 || (cnt == 0 && count > 0)) { ok = false; break; }
    if (cnt > 0) maxDepth = std::max(maxDepth, it.depth);
    for (int k = 0; k < cnt && ok; ++k) {
      Item c{};
      bvhChildBox(n, k, c.lo, c.hi);
      for (int a = 0; a < 3; ++a) {  // nested up to the parent's quantisation step (the child is re-quantised on a finer grid)
        float const step = bvhNodeScale(n, a);
        ok = ok && c.lo[a] <= c.hi[a] && c.lo[a] >= it.lo[a] - step && c.hi[a] <= it.hi[a] + step;
      }
      double const dx = double(c.hi[0]) - double(c.lo[0]), dy = double(c.hi[1]) - double(c.lo[1]), dz = double(c.hi[2]) - double(c.lo[2]);
      double const area = 2.0 * (dx * dy + dy * dz + dz * dx);
      if (it.node == 0) rootBox.grow(c.lo), rootBox.grow(c.hi);
      if (k < inner) {
        areaSum += area;
        c.node = n.childBase + uint32_t(k);
        c.depth = it.depth + 1;
        stack.push_back(c);
        continue;
      }
      size_t const pair = size_t(uint32_t(n.leafRef + uint32_t(k) - kBvhLeafFlag));  // the slot's reference without its flag
      if (pair >= npairs) { ok = false; break; }
      uint32_t const t0 = pairTris[2 * pair], t1 = pairTris[2 * pair + 1];
      maxLeaf = std::max(maxLeaf, t0 == t1 ? 1 : 2);
      areaSum += area * (t0 == t1 ? 1.0 : 2.0);
      for (int half = 0; half < (t0 == t1 ? 1 : 2) && ok; ++half) {  // a one-triangle leaf repeats its triangle
        uint32_t const t = half ? t1 : t0;
        if (t >= count || seen[t]++) { ok = false; break; }
        for (int v = 0; v < 3 && ok; ++v) {
          float const p[3] = {xs[4 * size_t(t) + v], ys[4 * size_t(t) + v], zs[4 * size_t(t) + v]};
          for (int a = 0; a < 3; ++a) ok = ok && p[a] >= c.lo[a] && p[a] <= c.hi[a];
        }
      }
    }
  }
  for (size_t i = 0; i < count && ok; ++i) ok = seen[i] == 1;
  for (size_t i = 0; i < nNodes && ok; ++i) ok = nodeSeen[i] == 1;
  if (depth) *depth = maxDepth;
  if (maxLeafOut) *maxLeafOut = maxLeaf;
  if (sahCost) {
    double const dx = double(rootBox.hi[0]) - double(rootBox.lo[0]), dy = double(rootBox.hi[1]) - double(rootBox.lo[1]),
                 dz = double(rootBox.hi[2]) - double(rootBox.lo[2]);
    double const rootArea = dx >= 0.0 ? 2.0 * (dx * dy + dy * dz + dz * dx) : 0.0;
    *sahCost = rootArea > 0.0 ? areaSum / rootArea : 0.0;
  }
  return ok && maxLeaf <= kBvhMaxLeafTris && maxDepth <= kBvhMaxDepth;
}

}  // namespace bvh_build

// ---- refit: same topology and pair order, every box recomputed from new positions ---------------------------------------------
// A pure function of (topology, new positions): nothing of the old boxes is read, only meta's inner | count nibbles,
// childBase and leafRef.  The kernels of bvh_gpu_build.hip (dmt_update_vertices under DMT_BVH_UPDATE_REFIT) and the serial
// restatement reference() below (dmt_bvh_refit_reference) run the same functions, so their nodes agree in all 64 bytes.
//   * padding: slabPadOf(largest |coordinate| of the NEW soup), as both builders take it
//   * pair box: primBox(t0), grown by primBox(t1) when the pair holds two triangles
//   * a node's exact box: the union of its children's exact fp32 boxes (never a decoded quantised box); children have
//     higher indices than their parent in both builders' output (childBase = 1 + the inner children of all nodes before),
//     so indices are walked downwards -- on the device one launch per 4-wide level, deepest first
//   * a node: encodeNode on the <= 4 gathered boxes, childBase and leafRef written back
// Refitting a tree with the soup it was built from reproduces it: min / max are exact and associative, so the union of the
// children's boxes IS the box the builder took (the union of the padded triangle boxes below), and encodeNode is the
// builders' own.
namespace refit {

using Box = lbvh::Box;

DMT_HD inline Box loadBox(float const* boxes, size_t i) {
  Box b;
  for (int a = 0; a < 3; ++a) b.lo[a] = boxes[6 * i + a], b.hi[a] = boxes[6 * i + 3 + a];
  return b;
}
DMT_HD inline void storeBox(float* boxes, size_t i, Box const& b) {
  for (int a = 0; a < 3; ++a) boxes[6 * i + a] = b.lo[a], boxes[6 * i + 3 + a] = b.hi[a];
}

// box of the pair with vertices v0 (and v1 when it holds two triangles)
DMT_HD inline Box pairBox(float const v0[9], float const v1[9], bool two, float slabPad) {
  Box b = lbvh::primBox(v0, slabPad);
  if (two) b.grow(lbvh::primBox(v1, slabPad));
  return b;
}

// one half of a pair record from a triangle's vertices: the builders' own subtractions
DMT_HD inline void packPairHalf(TriPair& P, int half, float const v[9], uint32_t orig) {
  P.p0x[half] = v[0], P.p0y[half] = v[1], P.p0z[half] = v[2];
  P.e0x[half] = v[3] - v[0], P.e0y[half] = v[4] - v[1], P.e0z[half] = v[5] - v[2];
  P.e1x[half] = v[6] - v[0], P.e1y[half] = v[7] - v[1], P.e1z[half] = v[8] - v[2];
  P.orig[half] = orig;
}

// the topology words of a node
DMT_HD inline int innerOf(uint32_t meta) { return int((meta >> 24) & 0xFu); }
DMT_HD inline int countOf(uint32_t meta) { return int((meta >> 28) & 0xFu); }
DMT_HD inline uint32_t pairOfSlot(uint32_t leafRef, int k) { return leafRef + uint32_t(k) - kBvhLeafFlag; }

// Refits node `self`: false (and nothing written) when its counts are out of range, a child index is not above its own or a
// reference leaves the arrays.  nodeBox / pairBox: 6 floats per node / pair, the children's already final.
DMT_HD inline bool refitNode(uint32_t self, uint32_t meta, uint32_t childBase, uint32_t leafRef, size_t nNodes, size_t nPairs, float* nodeBox,
                             float const* pairBoxes, Bvh4Node& out) {
  int const inner = innerOf(meta), cnt = countOf(meta);
  if (cnt > 4 || inner > cnt) return false;
  Box kb[4];
  for (int k = 0; k < cnt; ++k) {
    if (k < inner) {
      size_t const c = size_t(childBase) + size_t(k);
      if (c <= self || c >= nNodes) return false;
      kb[k] = loadBox(nodeBox, c);
    } else {
      size_t const p = pairOfSlot(leafRef, k);
      if (p >= nPairs) return false;
      kb[k] = loadBox(pairBoxes, p);
    }
  }
  bvh_build::encodeNode(out, kb, cnt, inner);
  out.childBase = childBase, out.leafRef = leafRef;
  Box all;
  all.reset();
  for (int k = 0; k < cnt; ++k) all.grow(kb[k]);
  storeBox(nodeBox, self, all);
  return true;
}

// decoded box of child k, as bvhChildBox (usable in kernels)
DMT_HD inline void childBox(Bvh4Node const& n, int k, float lo[3], float hi[3]) {
  uint32_t const ql[3] = {n.qlox, n.qloy, n.qloz}, qh[3] = {n.qhix, n.qhiy, n.qhiz};
  float const o[3] = {n.ox, n.oy, n.oz};
  for (int a = 0; a < 3; ++a) {
    uint32_t const bits = ((n.meta >> (8 * a)) & 0xFFu) << 23;
    float s;
    memcpy(&s, &bits, 4);
    lo[a] = o[a] + float((ql[a] >> (8 * k)) & 0xFFu) * s;
    hi[a] = o[a] + float((qh[a] >> (8 * k)) & 0xFFu) * s;
  }
}

// A node's term of bvh_build::check's SAH cost, in its fp64 arithmetic on the decoded boxes: the area of every child slot,
// a leaf slot weighted by its triangle count.  orig: the pairs' original indices, `stride` words from pair to pair.
DMT_HD inline double costTerm(Bvh4Node const& n, uint32_t const* orig, size_t stride, size_t nPairs) {
  int const inner = innerOf(n.meta), cnt = countOf(n.meta);
  double sum = 0.0;
  for (int k = 0; k < cnt && k < 4; ++k) {
    float lo[3], hi[3];
    childBox(n, k, lo, hi);
    double const dx = double(hi[0]) - double(lo[0]), dy = double(hi[1]) - double(lo[1]), dz = double(hi[2]) - double(lo[2]);
    double const area = 2.0 * (dx * dy + dy * dz + dz * dx);
    if (k < inner) {
      sum += area;
    } else {
      size_t const p = pairOfSlot(n.leafRef, k);
      bool const one = p >= nPairs || orig[p * stride] == orig[p * stride + 1];
      sum += area * (one ? 1.0 : 2.0);
    }
  }
  return sum;
}

// area of the union of the root's decoded child boxes: what check() divides the sum of the terms by (0: no cost)
inline double rootArea(Bvh4Node const& root) {
  Box rb;
  rb.reset();
  for (int k = 0; k < countOf(root.meta) && k < 4; ++k) {
    float lo[3], hi[3];
    childBox(root, k, lo, hi);
    rb.grow(lo), rb.grow(hi);
  }
  double const dx = double(rb.hi[0]) - double(rb.lo[0]), dy = double(rb.hi[1]) - double(rb.lo[1]), dz = double(rb.hi[2]) - double(rb.lo[2]);
  return dx >= 0.0 ? 2.0 * (dx * dy + dy * dz + dz * dx) : 0.0;
}

// first node of every 4-wide level of a tree laid out level by level (both builders'), then the node count: level l is
// [out[l], out[l + 1]).  Empty when the inner counts do not add up to the array.
inline std::vector<uint32_t> levelBounds(Bvh4Node const* nodes, size_t nNodes) {
  std::vector<uint32_t> out;
  size_t first = 0, count = nNodes ? 1 : 0;
  while (count > 0) {
    if (first + count > nNodes) return {};
    out.push_back(uint32_t(first));
    size_t inner = 0;
    for (size_t i = first; i < first + count; ++i) inner += size_t(innerOf(nodes[i].meta));
    first += count, count = inner;
  }
  if (first != nNodes) return {};
  out.push_back(uint32_t(nNodes));
  return out;
}

// The serial restatement: any tree in this layout and the NEW soup (the reference's SoA, 4 floats per triangle) -> the
// refitted nodes.  *sahCost (may be null): the sum of the nodes' terms over the root's area.  False: a child index not above
// its parent's, or a reference outside the arrays.
inline bool reference(Bvh4Node const* nodes, size_t nNodes, uint32_t const* pairTris, size_t npairs, float const* xs, float const* ys,
                      float const* zs, size_t count, Bvh4Node* out, double* sahCost) {
  if (nNodes == 0) return false;
  auto verts = [&](uint32_t i, float v[9]) {
    for (int c = 0; c < 3; ++c) v[3 * c] = xs[4 * size_t(i) + c], v[3 * c + 1] = ys[4 * size_t(i) + c], v[3 * c + 2] = zs[4 * size_t(i) + c];
  };
  uint32_t maxAbsBits = 0;  // non-negative floats order as their bit patterns
  for (size_t i = 0; i < count; ++i) {
    float v[9];
    verts(uint32_t(i), v);
    for (float f : v) {
      float const a = fabsf(f);
      uint32_t b;
      memcpy(&b, &a, 4);
      maxAbsBits = std::max(maxAbsBits, b);
    }
  }
  float sceneMaxAbs;
  memcpy(&sceneMaxAbs, &maxAbsBits, 4);
  float const slabPad = lbvh::slabPadOf(sceneMaxAbs);
  std::vector<float> pairBoxes(6 * npairs), nodeBox(6 * nNodes);
  for (size_t p = 0; p < npairs; ++p) {
    uint32_t const t0 = pairTris[2 * p], t1 = pairTris[2 * p + 1];
    if (t0 >= count || t1 >= count) return false;
    float v0[9], v1[9];
    verts(t0, v0), verts(t1, v1);
    storeBox(pairBoxes.data(), p, pairBox(v0, v1, t0 != t1, slabPad));
  }
  for (size_t i = nNodes; i-- > 0;)
    if (!refitNode(uint32_t(i), nodes[i].meta, nodes[i].childBase, nodes[i].leafRef, nNodes, npairs, nodeBox.data(), pairBoxes.data(), out[i]))
      return false;
  if (sahCost) {
    double sum = 0.0;
    for (size_t i = 0; i < nNodes; ++i) sum += costTerm(out[i], pairTris, 2, npairs);
    double const ra = rootArea(out[0]);
    *sahCost = ra > 0.0 ? sum / ra : 0.0;
  }
  return true;
}

}  // namespace refit

// ---- LBVH: what needs the node layout (the rest is lbvh.hpp) ----------------------------------------------------------------
namespace lbvh {

static_assert(kLeafFlag == kBvhLeafFlag, "lbvh.hpp restates the leaf flag");

// One 4-wide node made from binary ref `ref`, given where its inner children (childBase) and its leaves (firstPair) go
struct Entry {
  Bvh4Node node;
  uint32_t kids[4];      // binary refs, inner children first
  uint32_t pairTris[8];  // two ORIGINAL triangle indices per leaf, in slot order
  int nInner, nLeaf;
};
DMT_HD inline void layoutEntry(Tree2 const& T, uint32_t ref, uint32_t childBase, uint32_t firstPair, Entry& E) {
  int nk = 0;
  selectChildren(T, ref, E.kids, nk, E.nInner);
  E.nLeaf = nk - E.nInner;
  Box kb[4];
  for (int k = 0; k < nk; ++k) kb[k] = T.boxOf(E.kids[k]);
  bvh_build::encodeNode(E.node, kb, nk, E.nInner);
  E.node.childBase = childBase;
  E.node.leafRef = firstPair - uint32_t(E.nInner) + kBvhLeafFlag;
  for (int k = E.nInner; k < nk; ++k) leafTris(T, E.kids[k], E.pairTris[2 * (k - E.nInner)], E.pairTris[2 * (k - E.nInner) + 1]);
}

struct Reference {
  std::vector<Bvh4Node> nodes;
  std::vector<uint32_t> pairTris;
  int depth = 0;
  bool abandoned = false;  // the level loop would have passed maxDepth: no tree
};

// The serial restatement of the device builder: same functions, same order of levels, entries and slots.
// xs/ys/zs: the reference's SoA (4 floats per triangle: c0, c1, c2, pad)
inline Reference reference(float const* xs, float const* ys, float const* zs, uint32_t n, int maxDepth) {
  Reference out;
  if (n == 0) {  // a root without children
    Bvh4Node root;
    bvh_build::encodeNode(root, nullptr, 0, 0);
    out.nodes.push_back(root);
    return out;
  }
  auto verts = [&](uint32_t i, float v[9]) {
    for (int c = 0; c < 3; ++c) v[3 * c] = xs[4 * size_t(i) + c], v[3 * c + 1] = ys[4 * size_t(i) + c], v[3 * c + 2] = zs[4 * size_t(i) + c];
  };
  // 1. padding scale, centroid bounds
  uint32_t maxAbsBits = 0;  // non-negative floats order as their bit patterns
  for (uint32_t i = 0; i < n; ++i) {
    float v[9];
    verts(i, v);
    for (float f : v) {
      float const a = fabsf(f);
      uint32_t b;
      memcpy(&b, &a, 4);
      maxAbsBits = std::max(maxAbsBits, b);
    }
  }
  float sceneMaxAbs;
  memcpy(&sceneMaxAbs, &maxAbsBits, 4);
  float const slabPad = slabPadOf(sceneMaxAbs);
  uint32_t cbLoO[3] = {kNone, kNone, kNone}, cbHiO[3] = {0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    float v[9], c[3];
    verts(i, v);
    centroidOf(primBox(v, slabPad), c);
    for (int a = 0; a < 3; ++a) cbLoO[a] = std::min(cbLoO[a], orderedOfFloat(c[a])), cbHiO[a] = std::max(cbHiO[a], orderedOfFloat(c[a]));
  }
  float cbLo[3], cbHi[3];
  for (int a = 0; a < 3; ++a) cbLo[a] = floatOfOrdered(cbLoO[a]), cbHi[a] = floatOfOrdered(cbHiO[a]);
  // 2. keys, sorted (unique: a total order)
  std::vector<uint64_t> keys(n);
  for (uint32_t i = 0; i < n; ++i) {
    float v[9], c[3];
    verts(i, v);
    centroidOf(primBox(v, slabPad), c);
    keys[i] = keyOf(mortonOf(c, cbLo, cbHi), i);
  }
  std::sort(keys.begin(), keys.end());
  // 3. binary radix tree
  std::vector<uint32_t> left(n - 1), right(n - 1), parent(2 * size_t(n) - 1, kNone);
  for (uint32_t i = 0; i + 1 < n; ++i) {
    radixNode(keys.data(), n, i, left[i], right[i]);
    parent[left[i]] = i, parent[right[i]] = i;
  }
  // 4. boxes bottom-up: the first to arrive at a parent leaves, the second combines and goes on
  std::vector<float> box(6 * (2 * size_t(n) - 1));
  std::vector<uint8_t> arrived(n - 1, 0);
  auto storeBox = [&](uint32_t ref, Box const& b) {
    for (int a = 0; a < 3; ++a) box[6 * size_t(ref) + a] = b.lo[a], box[6 * size_t(ref) + 3 + a] = b.hi[a];
  };
  Tree2 const T{n, left.data(), right.data(), box.data(), keys.data()};
  for (uint32_t j = 0; j < n; ++j) {
    float v[9];
    verts(uint32_t(keys[j]), v);
    Box b = primBox(v, slabPad);
    uint32_t ref = n - 1 + j;
    storeBox(ref, b);
    for (uint32_t p = parent[ref]; p != kNone; p = parent[p]) {
      if (!arrived[p]++) break;
      b.grow(T.boxOf(left[p] == ref ? right[p] : left[p]));
      storeBox(p, b);
      ref = p;
    }
  }
  // 5. collapse, level by level
  std::vector<uint32_t> cur{0u}, next;
  uint32_t levelBase = 0, pairBase = 0;
  while (!cur.empty()) {
    if (out.depth + 1 > maxDepth) {  // 6. depth guard
      out.nodes.clear(), out.pairTris.clear(), out.depth = 0, out.abandoned = true;
      return out;
    }
    ++out.depth;
    uint32_t const nextBase = levelBase + uint32_t(cur.size());
    uint32_t innerOff = 0, leafOff = 0;
    next.clear();
    for (uint32_t ref : cur) {
      Entry E;
      layoutEntry(T, ref, nextBase + innerOff, pairBase + leafOff, E);
      out.nodes.push_back(E.node);
      out.pairTris.insert(out.pairTris.end(), E.pairTris, E.pairTris + 2 * E.nLeaf);
      next.insert(next.end(), E.kids, E.kids + E.nInner);
      innerOff += uint32_t(E.nInner), leafOff += uint32_t(E.nLeaf);
    }
    levelBase = nextBase, pairBase += leafOff;
    cur.swap(next);
  }
  return out;
}

}  // namespace lbvh

}  // namespace dmt
