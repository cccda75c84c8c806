// lbvh.hpp -- the arithmetic of the LBVH builder (Karras 2012, "Maximizing parallelism in the construction of BVHs,
// octrees, and k-d trees") in this project's node format, as __host__ __device__ functions.
//
// One set of functions serves three users, so that their outputs can be compared bit for bit:
//   * the kernels of csrc/bvh_gpu_build.hip (DMT_BVH_BUILD_DEVICE),
//   * the serial host restatement lbvh::reference() below (dmt_lbvh_reference),
//   * the host SAH builder of bvh.hpp, which takes its triangle padding and its node encoding from here.
// Everything is either integer work, min / max, or fp32 / fp64 expressions without contraction: the device side is
// compiled with -ffp-contract=off, IEEE division and no denormal flush (csrc/Makefile), the host side has no fused
// multiply-add to contract to.
//
// The pipeline (each step a function of the input alone, hence two builds give the same bytes):
//   1. per triangle: box padded as the host builder pads it (primBox), centroid of the padded box
//   2. key = 30-bit Morton code of the centroid on the centroid bounds << 32 | triangle index; sort
//   3. binary radix tree over the sorted keys (radixNode): n - 1 inner nodes, one leaf per triangle
//   4. boxes bottom-up
//   5. collapse to 4-wide level by level (selectChildren + layoutEntry): a binary node whose children are both triangles
//      IS a leaf (one pair), a lone triangle child is a one-triangle leaf; a node opens its non-leaf child of largest
//      area until it has four; per level an exclusive scan over (inner, leaf) counts gives childBase and the pair index
//   6. the level loop stops at maxDepth levels ("abandoned": the caller runs the host builder)
//
// References into the binary tree ("ref"): 0 .. n-2 = inner node, n-1 + j = the triangle at sorted position j.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define DMT_HD __host__ __device__
#else
#define DMT_HD
#endif

namespace dmt {

struct Bvh4Node;  // bvh.hpp

namespace lbvh {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLeafFlag = 0x80000000u;  // = kBvhLeafFlag (bvh.hpp; static_assert there)

struct Box {
  float lo[3], hi[3];
  DMT_HD void reset() {
    for (int a = 0; a < 3; ++a) lo[a] = __builtin_inff(), hi[a] = -__builtin_inff();
  }
  DMT_HD void grow(float const p[3]) {
    for (int a = 0; a < 3; ++a) lo[a] = p[a] < lo[a] ? p[a] : lo[a], hi[a] = hi[a] < p[a] ? p[a] : hi[a];
  }
  DMT_HD void grow(Box const& b) {
    for (int a = 0; a < 3; ++a) lo[a] = b.lo[a] < lo[a] ? b.lo[a] : lo[a], hi[a] = hi[a] < b.hi[a] ? b.hi[a] : hi[a];
  }
  DMT_HD float area() const {
    float const dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0.f)) return 0.f;
    return 2.f * (dx * dy + dy * dz + dz * dx);
  }
};

// slab padding of a soup whose largest |coordinate| is sceneMaxAbs (why: bvh.hpp, bvh_build::build)
DMT_HD inline float slabPadOf(float sceneMaxAbs) { return 2.5e-7f * 9.f * sceneMaxAbs; }

// grows the tight box of a triangle by the padding terms: far above the rounding of the triangle test (~1e-7 relative
// to the triangle) and of the slab tests (slabPad), far below anything that costs traversal work
DMT_HD inline void padBox(Box& bx, float slabPad) {
  for (int a = 0; a < 3; ++a) {
    float const al = fabsf(bx.lo[a]), ah = fabsf(bx.hi[a]);
    float const m = al < ah ? ah : al;
    float const pad = 1e-5f * (bx.hi[a] - bx.lo[a]) + 4e-6f * m + 1e-7f + slabPad;
    bx.lo[a] -= pad, bx.hi[a] += pad;
  }
}

// padded box of the triangle with vertices v[0..2], v[3..5], v[6..8]
DMT_HD inline Box primBox(float const v[9], float slabPad) {
  Box bx;
  bx.reset();
  bx.grow(v), bx.grow(v + 3), bx.grow(v + 6);
  padBox(bx, slabPad);
  return bx;
}

DMT_HD inline void centroidOf(Box const& bx, float c[3]) {
  for (int a = 0; a < 3; ++a) c[a] = 0.5f * (bx.lo[a] + bx.hi[a]);
}

// floats as unsigned integers of the same order (min / max reductions with integer atomics)
DMT_HD inline uint32_t orderedOfFloat(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DMT_HD inline float floatOfOrdered(uint32_t o) {
  uint32_t const b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

DMT_HD inline uint32_t spreadBits10(uint32_t v) {  // 10 bits -> every third bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

// 30-bit Morton code of centroid c on the centroid bounds; an axis of zero extent codes as 0
DMT_HD inline uint32_t mortonOf(float const c[3], float const cbLo[3], float const cbHi[3]) {
  uint32_t q[3];
  for (int a = 0; a < 3; ++a) {
    float const ext = cbHi[a] - cbLo[a];
    q[a] = 0;
    if (ext > 0.f) {
      float const v = (c[a] - cbLo[a]) * (1024.f / ext);
      q[a] = !(v >= 0.f) ? 0u : (v >= 1023.f ? 1023u : uint32_t(v));
    }
  }
  return (spreadBits10(q[0]) << 2) | (spreadBits10(q[1]) << 1) | spreadBits10(q[2]);
}

DMT_HD inline uint64_t keyOf(uint32_t morton, uint32_t tri) { return (uint64_t(morton) << 32) | tri; }

// common leading bits of keys i and j (keys are unique), -1 outside the array
DMT_HD inline int delta(uint64_t const* keys, uint32_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= int64_t(n)) return -1;
  return __builtin_clzll(keys[i] ^ keys[j]);
}

// children of inner node i (0 <= i < n - 1) of the binary radix tree over n sorted unique keys, as refs
DMT_HD inline void radixNode(uint64_t const* keys, uint32_t n, uint32_t i, uint32_t& left, uint32_t& right) {
  int64_t const I = int64_t(i);
  int const d = delta(keys, n, I, I + 1) - delta(keys, n, I, I - 1) < 0 ? -1 : 1;
  int const dmin = delta(keys, n, I, I - d);
  int64_t lmax = 2;
  while (delta(keys, n, I, I + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, n, I, I + (l + t) * d) > dmin) l += t;
  int64_t const j = I + l * d;
  int const dnode = delta(keys, n, I, j);
  int64_t s = 0;
  for (int64_t div = 2;; div *= 2) {
    int64_t const t = (l + div - 1) / div;  // ceil(l / 2), ceil(l / 4), ..., 1
    if (delta(keys, n, I, I + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  int64_t const gamma = I + s * d + (d < 0 ? -1 : 0);
  int64_t const first = I < j ? I : j, last = I < j ? j : I;
  left = first == gamma ? uint32_t(n - 1 + gamma) : uint32_t(gamma);
  right = last == gamma + 1 ? uint32_t(n - 1 + gamma + 1) : uint32_t(gamma + 1);
}

// the binary tree as the collapse reads it
struct Tree2 {
  uint32_t n;                 // triangles
  uint32_t const* left;       // [n - 1] refs
  uint32_t const* right;      // [n - 1]
  float const* box;           // [2 n - 1][6]: lo xyz, hi xyz of every ref
  uint64_t const* keys;       // [n] sorted; the low word is the ORIGINAL triangle index
  DMT_HD bool isTri(uint32_t ref) const { return ref >= n - 1; }
  DMT_HD bool isLeaf(uint32_t ref) const { return isTri(ref) || (isTri(left[ref]) && isTri(right[ref])); }
  DMT_HD uint32_t triOf(uint32_t ref) const { return uint32_t(keys[ref - (n - 1)]); }
  DMT_HD Box boxOf(uint32_t ref) const {
    Box b;
    for (int a = 0; a < 3; ++a) b.lo[a] = box[6 * size_t(ref) + a], b.hi[a] = box[6 * size_t(ref) + 3 + a];
    return b;
  }
};

// children of the 4-wide node made from binary ref `ref`: inner children first, each group in slot order.  The host
// builder's rule: while there are fewer than four, open the non-leaf child of largest box area, first of equals.
DMT_HD inline void selectChildren(Tree2 const& T, uint32_t ref, uint32_t kids[4], int& nk, int& nInner) {
  uint32_t k4[4];
  nk = 0;
  if (T.isLeaf(ref)) {
    k4[nk++] = ref;
  } else {
    k4[nk++] = T.left[ref];
    k4[nk++] = T.right[ref];
    while (nk < 4) {
      int pick = -1;
      float bestA = -1.f;
      for (int k = 0; k < nk; ++k)
        if (!T.isLeaf(k4[k])) {
          float const ar = T.boxOf(k4[k]).area();
          if (ar > bestA) bestA = ar, pick = k;
        }
      if (pick < 0) break;
      uint32_t const open = k4[pick];
      k4[pick] = T.left[open];
      k4[nk++] = T.right[open];
    }
  }
  nInner = 0;
  for (int k = 0; k < nk; ++k)
    if (!T.isLeaf(k4[k])) kids[nInner++] = k4[k];
  int at = nInner;
  for (int k = 0; k < nk; ++k)
    if (T.isLeaf(k4[k])) kids[at++] = k4[k];
}

// the two ORIGINAL triangle indices of leaf `ref` (a one-triangle leaf repeats its triangle)
DMT_HD inline void leafTris(Tree2 const& T, uint32_t ref, uint32_t& t0, uint32_t& t1) {
  if (T.isTri(ref)) t0 = t1 = T.triOf(ref);
  else t0 = T.triOf(T.left[ref]), t1 = T.triOf(T.right[ref]);
}

}  // namespace lbvh
}  // namespace dmt
