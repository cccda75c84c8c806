// bvh_gpu_build.hip -- DMT_BVH_BUILD_DEVICE: the LBVH of lbvh.hpp built on the device, into the node / pair layout of
// bvh.hpp.  A translation unit of its own: not render-hot, shares nothing with the megakernels, and compiled WITHOUT
// their fast-math flags (csrc/Makefile: no contraction, IEEE division, denormals kept), so that every kernel here
// computes what the serial restatement lbvh::reference() computes on the host, bit for bit
// (tests/test_bvh_gpu_build_gpu.py compares all 64 bytes of every node).
//
// Kernels, in stream order (one thread per element unless noted; nothing waits for another wave anywhere):
//   k_scene_max, k_centroid_bounds   reductions (grid-stride, one integer atomicMax per block and word)
//   k_keys                           Morton key << 32 | triangle index
//   rocprim::radix_sort_keys         on the 30 Morton bits; stable, so equal codes stay in index order = the order of the keys
//   k_radix_tree                     children + parent links of the n - 1 binary inner nodes
//   k_fit                            boxes bottom-up by arrival counting (the visibility protocol: at the kernel)
//   per 4-wide level: k_level_count, rocprim::exclusive_scan, k_level_emit; the host reads the level's totals
//   k_guard_pairs                    three copies of the last pair
//
// The second half, the refit (bvh.hpp namespace refit; dmt_update_vertices): same topology and pair order, new positions.
//   k_pack_records                   TriIsect / TriPost from 9 floats per triangle (dmt_update_vertices_device only)
//   k_scene_max                      the padding scale of the NEW soup
//   k_refit_pairs                    every pair rewritten from the new vertices, its box; the three guard pairs in the tail
//   k_refit_level                    one launch per 4-wide level, deepest first, one thread per node: gathers the <= 4
//                                    child boxes the launches before left, encodes, stores its own box.  Nothing crosses
//                                    workgroups inside a launch; kernel boundaries are the only ordering.
//   k_refit_cost, rocprim::reduce    one fp64 term per node (bvh_build::check's arithmetic), summed
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>  // before rocPRIM: its headers use memcpy without including it

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dmt_hip.h"
#include "bvh_gpu_build.hpp"

namespace dmt {
namespace lbvh_gpu {
namespace {

constexpr int kBlock = 256;
// the zeroed words of Scratch::words
enum : uint32_t {
  W_MAX_ABS = 0,   // bits of the soup's largest |coordinate|
  W_CB_LO = 1,     // ~ordered(centroid min) x, y, z (so that zero is the identity of max)
  W_CB_HI = 4,     // ordered(centroid max) x, y, z
  W_TOTALS = 8,    // per level: inner children, leaves
  W_OVERRUN = 10,  // set if a level would write past an array (cannot happen for a valid tree; checked, not assumed)
  W_COUNTERS = 16  // [n - 1] arrivals at the binary inner nodes
};

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

__device__ __forceinline__ uint32_t blockMax(uint32_t v) {
  __shared__ uint32_t part[kBlock / 64];
  for (int off = 32; off > 0; off >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), off, 64)));
  __syncthreads();  // `part` may still be read from the previous call
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = part[0];
  for (int w = 1; w < kBlock / 64; ++w) m = max(m, part[w]);
  return m;
}

__device__ __forceinline__ void loadVerts(float const* verts, uint32_t stride, uint32_t tri, float v[9]) {
  float const* p = verts + size_t(tri) * stride;
  for (int q = 0; q < 9; ++q) v[q] = p[q];
}

__device__ __forceinline__ float slabPadFrom(uint32_t const* words) {
  uint32_t const b = words[W_MAX_ABS];
  float m;
  memcpy(&m, &b, 4);
  return lbvh::slabPadOf(m);
}

__global__ void __launch_bounds__(kBlock) k_scene_max(float const* verts, uint32_t stride, uint32_t n, uint32_t* words) {
  uint32_t m = 0;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    float v[9];
    loadVerts(verts, stride, i, v);
    for (int q = 0; q < 9; ++q) {
      float const a = fabsf(v[q]);
      uint32_t b;
      memcpy(&b, &a, 4);
      m = max(m, b);  // non-negative floats order as their bit patterns
    }
  }
  m = blockMax(m);
  if (threadIdx.x == 0) atomicMax(&words[W_MAX_ABS], m);
}

__global__ void __launch_bounds__(kBlock) k_centroid_bounds(float const* verts, uint32_t stride, uint32_t n, uint32_t* words) {
  float const slabPad = slabPadFrom(words);
  uint32_t r[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    float v[9], c[3];
    loadVerts(verts, stride, i, v);
    lbvh::centroidOf(lbvh::primBox(v, slabPad), c);
    for (int a = 0; a < 3; ++a) {
      uint32_t const o = lbvh::orderedOfFloat(c[a]);
      r[a] = max(r[a], ~o), r[3 + a] = max(r[3 + a], o);
    }
  }
  for (int q = 0; q < 6; ++q) {
    uint32_t const m = blockMax(r[q]);
    if (threadIdx.x == 0) atomicMax(&words[W_CB_LO + q], m);
  }
}

__global__ void __launch_bounds__(kBlock) k_keys(float const* verts, uint32_t stride, uint32_t n, uint32_t const* words, uint64_t* keys) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float cbLo[3], cbHi[3];
  for (int a = 0; a < 3; ++a) cbLo[a] = lbvh::floatOfOrdered(~words[W_CB_LO + a]), cbHi[a] = lbvh::floatOfOrdered(words[W_CB_HI + a]);
  float v[9], c[3];
  loadVerts(verts, stride, i, v);
  lbvh::centroidOf(lbvh::primBox(v, slabPadFrom(words)), c);
  keys[i] = lbvh::keyOf(lbvh::mortonOf(c, cbLo, cbHi), i);
}

__global__ void __launch_bounds__(kBlock) k_radix_tree(uint64_t const* keys, uint32_t n, uint32_t* left, uint32_t* right, uint32_t* parent) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i + 1 >= n) return;
  uint32_t l, r;
  lbvh::radixNode(keys, n, i, l, r);
  left[i] = l, right[i] = r;
  parent[l] = i, parent[r] = i;  // every ref but the root has exactly one parent: no two threads write one word
}

// Boxes bottom-up.  One thread per triangle climbs from its leaf; at each parent the first arriver leaves, the second
// combines its box with its sibling's and goes on: nobody waits, and the climb is bounded by the tree's height.
// The hand-off between the two arrivers may cross workgroups and XCDs (private L2s, per-CU L1s), so:
//   * a box is written with agent-scope atomic stores of 8-byte granules (write-through, never a plain store),
//   * the writer drains them (s_waitcnt vmcnt(0)) before it touches the parent's counter,
//   * the counter is an agent-scope acq_rel fetch-add (words zeroed by a hipMemsetAsync before every build),
//   * the second arriver reads its sibling's box with agent-scope atomic loads, never a plain load of a line that
//     another workgroup wrote in this launch.
// Later kernels read the boxes with plain loads: a new launch sees everything the previous one wrote.
__device__ __forceinline__ void storeBoxAgent(uint64_t* box, uint32_t ref, lbvh::Box const& b) {
  gu64* const g = (gu64*)(box + 3 * size_t(ref));
  float const f[6] = {b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]};
  for (int q = 0; q < 3; ++q) {
    unsigned long long w;
    memcpy(&w, &f[2 * q], 8);
    __hip_atomic_store(g + q, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ lbvh::Box loadBoxAgent(uint64_t* box, uint32_t ref) {
  gu64* const g = (gu64*)(box + 3 * size_t(ref));
  float f[6];
  for (int q = 0; q < 3; ++q) {
    unsigned long long const w = __hip_atomic_load(g + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    memcpy(&f[2 * q], &w, 8);
  }
  lbvh::Box b;
  for (int a = 0; a < 3; ++a) b.lo[a] = f[a], b.hi[a] = f[3 + a];
  return b;
}

__global__ void __launch_bounds__(kBlock) k_fit(float const* verts, uint32_t stride, uint64_t const* keys, uint32_t n, uint32_t const* words,
                                                uint32_t const* left, uint32_t const* right, uint32_t const* parent, uint64_t* box,
                                                uint32_t* counters) {
  uint32_t const j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  float v[9];
  loadVerts(verts, stride, uint32_t(keys[j]), v);
  lbvh::Box b = lbvh::primBox(v, slabPadFrom(words));
  uint32_t ref = n - 1 + j;
  storeBoxAgent(box, ref, b);
  for (uint32_t p = parent[ref]; p != lbvh::kNone; p = parent[p]) {  // parent / left / right: written by the previous launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the box is out before the arrival is counted
    uint32_t const earlier = __hip_atomic_fetch_add((gu32*)(counters + p), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (earlier == 0) return;  // first at p: the sibling's thread will pick this box up
    b.grow(loadBoxAgent(box, left[p] == ref ? right[p] : left[p]));
    storeBoxAgent(box, p, b);
    ref = p;
  }
}

__device__ __forceinline__ lbvh::Tree2 treeOf(uint32_t n, uint32_t const* left, uint32_t const* right, uint64_t const* box, uint64_t const* keys) {
  return lbvh::Tree2{n, left, right, reinterpret_cast<float const*>(box), keys};
}

__global__ void __launch_bounds__(kBlock) k_level_count(uint32_t n, uint32_t const* left, uint32_t const* right, uint64_t const* box,
                                                        uint64_t const* keys, uint32_t const* level, uint32_t count, uint64_t* counts) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  uint32_t kids[4];
  int nk, nInner;
  lbvh::selectChildren(treeOf(n, left, right, box, keys), level[i], kids, nk, nInner);
  counts[i] = (uint64_t(uint32_t(nInner)) << 32) | uint32_t(nk - nInner);
}

struct EmitArgs {
  uint32_t n;
  uint32_t const *left, *right;
  uint64_t const *box, *keys;
  float const* verts;
  uint32_t stride;
  uint32_t const* level;
  uint32_t count;
  uint64_t const *counts, *offsets;
  uint32_t levelBase, pairBase;
  Bvh4Node* nodes;
  TriPair* pairs;
  uint32_t* next;
  uint32_t cap;  // nodes, pairs (without guards) and next-level entries allocated
  uint32_t* words;
};

__global__ void __launch_bounds__(kBlock) k_level_emit(EmitArgs A) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.count) return;
  uint32_t const innerOff = uint32_t(A.offsets[i] >> 32), leafOff = uint32_t(A.offsets[i]);
  uint32_t const nextBase = A.levelBase + A.count;
  lbvh::Entry E;
  lbvh::layoutEntry(treeOf(A.n, A.left, A.right, A.box, A.keys), A.level[i], nextBase + innerOff, A.pairBase + leafOff, E);
  if (i == A.count - 1) A.words[W_TOTALS] = innerOff + uint32_t(E.nInner), A.words[W_TOTALS + 1] = leafOff + uint32_t(E.nLeaf);
  if (A.levelBase + i >= A.cap || innerOff + uint32_t(E.nInner) > A.cap || A.pairBase + leafOff + uint32_t(E.nLeaf) > A.cap) {
    A.words[W_OVERRUN] = 1;
    return;
  }
  A.nodes[A.levelBase + i] = E.node;
  for (int k = 0; k < E.nInner; ++k) A.next[innerOff + uint32_t(k)] = E.kids[k];
  for (int k = 0; k < E.nLeaf; ++k) {
    TriPair P;
    for (int half = 0; half < 2; ++half) {
      uint32_t const t = E.pairTris[2 * k + half];
      float v[9];
      loadVerts(A.verts, A.stride, t, v);
      P.p0x[half] = v[0], P.p0y[half] = v[1], P.p0z[half] = v[2];
      P.e0x[half] = v[3] - v[0], P.e0y[half] = v[4] - v[1], P.e0z[half] = v[5] - v[2];
      P.e1x[half] = v[6] - v[0], P.e1y[half] = v[7] - v[1], P.e1z[half] = v[8] - v[2];
      P.orig[half] = t;
    }
    A.pairs[A.pairBase + leafOff + uint32_t(k)] = P;
  }
}

__global__ void k_guard_pairs(TriPair* pairs, uint32_t npairs) {
  if (threadIdx.x < 3 && npairs > 0) pairs[npairs + threadIdx.x] = pairs[npairs - 1];
}

// ---- refit ---------------------------------------------------------------------------------------------------------------
enum : uint32_t { W_REFIT_BAD = 1, W_REFIT_WORDS = 4 };  // RefitScratch::words: W_MAX_ABS, then "a reference left the arrays"

__global__ void __launch_bounds__(kBlock) k_pack_records(float const* verts9, uint32_t n, TriIsect* tris, TriPost* post) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float v[9];
  loadVerts(verts9, 9, i, v);
  TriIsect t;
  TriPost q;
  packTriangle(v, tris[i].matId, t, q);  // the material id: from the record already there
  tris[i] = t, post[i] = q;
}

// One thread per pair, and three more for the guard pairs (copies of the last pair, made from its indices: no thread reads
// what another writes -- orig[] of a real pair is never written).
__global__ void __launch_bounds__(kBlock) k_refit_pairs(float const* verts, uint32_t stride, uint32_t n, TriPair* pairs, uint32_t npairs,
                                                        uint32_t* words, float* pairBox) {
  uint32_t const p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npairs + 3) return;
  uint32_t const src = p < npairs ? p : npairs - 1;
  uint32_t const t0 = pairs[src].orig[0], t1 = pairs[src].orig[1];
  if (t0 >= n || t1 >= n) {
    words[W_REFIT_BAD] = 1;
    return;
  }
  float v0[9], v1[9];
  loadVerts(verts, stride, t0, v0), loadVerts(verts, stride, t1, v1);
  TriPair P;
  refit::packPairHalf(P, 0, v0, t0), refit::packPairHalf(P, 1, v1, t1);
  static_assert(offsetof(TriPair, orig) == 72, "the 18 floats of a pair come first");
  memcpy(static_cast<void*>(pairs + p), &P, offsetof(TriPair, orig));
  if (p >= npairs) {
    pairs[p].orig[0] = t0, pairs[p].orig[1] = t1;
    return;
  }
  refit::storeBox(pairBox, p, refit::pairBox(v0, v1, t0 != t1, slabPadFrom(words)));
}

__global__ void __launch_bounds__(kBlock) k_refit_level(Bvh4Node* nodes, uint32_t first, uint32_t count, uint32_t nNodes, uint32_t nPairs,
                                                        float* nodeBox, float const* pairBox, uint32_t* words) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  uint32_t const self = first + i;
  Bvh4Node const* const old = nodes + self;  // only meta, childBase and leafRef are read
  Bvh4Node nd;
  if (!refit::refitNode(self, old->meta, old->childBase, old->leafRef, nNodes, nPairs, nodeBox, pairBox, nd)) {
    words[W_REFIT_BAD] = 1;
    return;
  }
  nodes[self] = nd;
}

__global__ void __launch_bounds__(kBlock) k_refit_cost(Bvh4Node const* nodes, uint32_t nNodes, TriPair const* pairs, uint32_t nPairs, double* terms) {
  uint32_t const i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= nNodes) return;
  terms[i] = refit::costTerm(nodes[i], pairs[0].orig, sizeof(TriPair) / sizeof(uint32_t), nPairs);
}

unsigned blocksFor(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

size_t Scratch::bytes() const {
  return (keys.size() + keysSorted.size() + box.size() + counts.size() + offsets.size()) * 8 + sortTemp.size() +
         (left.size() + right.size() + parent.size() + words.size() + levelA.size() + levelB.size()) * 4 + nodes.size() * sizeof(Bvh4Node) +
         pairs.size() * sizeof(TriPair);
}

#define LBVH_TRY(step, call)             \
  do {                                   \
    hipError_t const e__ = (call);       \
    if (e__ != hipSuccess) {             \
      what = step;                       \
      return e__;                        \
    }                                    \
  } while (0)

namespace {
struct Events {  // destroyed on every exit path
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};
}  // namespace

hipError_t build(float const* verts, uint32_t strideFloats, uint32_t n, int maxDepth, hipStream_t stream, Scratch& S, Result& out,
                 std::string& what) {
  out = Result{};
  if (n == 0) {  // a root without children
    Bvh4Node root;
    bvh_build::encodeNode(root, nullptr, 0, 0);
    LBVH_TRY("uploading the empty root", out.nodes.assign(&root, 1));
    LBVH_TRY("allocating the pair array", out.pairs.assign(nullptr, 0));
    out.nodeCount = 1;
    out.levels = {0u, 1u};
    return hipSuccess;
  }
  // temporaries
  size_t sortBytes = 0, scanBytes = 0;
  LBVH_TRY("sizing the sort", rocprim::radix_sort_keys(nullptr, sortBytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                                          size_t(n), 32u, 62u, stream));
  LBVH_TRY("sizing the scan", rocprim::exclusive_scan(nullptr, scanBytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                                         uint64_t(0), size_t(n), rocprim::plus<uint64_t>(), stream));
  size_t const refs = 2 * size_t(n) - 1;
  char const* const allocStep = "allocating temporaries";
  LBVH_TRY(allocStep, S.keys.reserve(n));
  LBVH_TRY(allocStep, S.keysSorted.reserve(n));
  LBVH_TRY(allocStep, S.sortTemp.reserve(std::max<size_t>(std::max(sortBytes, scanBytes), 16)));
  LBVH_TRY(allocStep, S.left.reserve(n));
  LBVH_TRY(allocStep, S.right.reserve(n));
  LBVH_TRY(allocStep, S.parent.reserve(refs));
  LBVH_TRY(allocStep, S.box.reserve(3 * refs));
  LBVH_TRY(allocStep, S.words.reserve(W_COUNTERS + size_t(n)));
  LBVH_TRY(allocStep, S.levelA.reserve(n));
  LBVH_TRY(allocStep, S.levelB.reserve(n));
  LBVH_TRY(allocStep, S.counts.reserve(n));
  LBVH_TRY(allocStep, S.offsets.reserve(n));
  LBVH_TRY(allocStep, S.nodes.reserve(n));
  LBVH_TRY(allocStep, S.pairs.reserve(size_t(n) + 3));
  out.tempBytes = S.bytes();

  Events ev;
  LBVH_TRY("creating events", hipEventCreate(&ev.a));
  LBVH_TRY("creating events", hipEventCreate(&ev.b));
  LBVH_TRY("recording the start", hipEventRecord(ev.a, stream));

  uint32_t* const words = S.words.get();
  unsigned const all = blocksFor(n), some = std::min(all, 4096u);
  LBVH_TRY("zeroing counters", hipMemsetAsync(words, 0, (W_COUNTERS + size_t(n)) * sizeof(uint32_t), stream));
  LBVH_TRY("clearing parents", hipMemsetAsync(S.parent.get(), 0xFF, refs * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_scene_max, dim3(some), dim3(kBlock), 0, stream, verts, strideFloats, n, words);
  hipLaunchKernelGGL(k_centroid_bounds, dim3(some), dim3(kBlock), 0, stream, verts, strideFloats, n, words);
  hipLaunchKernelGGL(k_keys, dim3(all), dim3(kBlock), 0, stream, verts, strideFloats, n, words, S.keys.get());
  LBVH_TRY("launching the key kernels", hipGetLastError());
  size_t tempBytes = S.sortTemp.size();
  LBVH_TRY("sorting", rocprim::radix_sort_keys(S.sortTemp.get(), tempBytes, S.keys.get(), S.keysSorted.get(), size_t(n), 32u, 62u, stream));
  uint64_t const* const keys = S.keysSorted.get();
  if (n > 1) hipLaunchKernelGGL(k_radix_tree, dim3(blocksFor(n - 1)), dim3(kBlock), 0, stream, keys, n, S.left.get(), S.right.get(), S.parent.get());
  hipLaunchKernelGGL(k_fit, dim3(all), dim3(kBlock), 0, stream, verts, strideFloats, keys, n, words, S.left.get(), S.right.get(), S.parent.get(),
                     S.box.get(), words + W_COUNTERS);
  LBVH_TRY("launching the tree kernels", hipGetLastError());

  // collapse: one 4-wide level per round; the host reads the level's totals (at most maxDepth small synchronisations)
  EmitArgs A{};
  A.n = n, A.left = S.left.get(), A.right = S.right.get(), A.box = S.box.get(), A.keys = keys;
  A.verts = verts, A.stride = strideFloats;
  A.counts = S.counts.get(), A.offsets = S.offsets.get();
  A.nodes = S.nodes.get(), A.pairs = S.pairs.get(), A.cap = n, A.words = words;
  uint32_t* cur = S.levelA.get();
  uint32_t* next = S.levelB.get();
  LBVH_TRY("seeding the root level", hipMemsetAsync(cur, 0, sizeof(uint32_t), stream));  // ref 0: the root
  uint32_t count = 1;
  while (count > 0) {
    if (out.depth + 1 > maxDepth) {  // depth guard: the traversal stack is sized by the bound
      out.abandoned = true;
      break;
    }
    ++out.depth;
    hipLaunchKernelGGL(k_level_count, dim3(blocksFor(count)), dim3(kBlock), 0, stream, n, A.left, A.right, A.box, keys, cur, count, S.counts.get());
    tempBytes = S.sortTemp.size();
    LBVH_TRY("scanning a level", rocprim::exclusive_scan(S.sortTemp.get(), tempBytes, S.counts.get(), S.offsets.get(), uint64_t(0), size_t(count),
                                                            rocprim::plus<uint64_t>(), stream));
    A.level = cur, A.count = count, A.next = next;
    hipLaunchKernelGGL(k_level_emit, dim3(blocksFor(count)), dim3(kBlock), 0, stream, A);
    LBVH_TRY("launching a level", hipGetLastError());
    uint32_t h[3] = {0, 0, 0};  // inner children, leaves, overrun
    LBVH_TRY("reading a level's totals", hipMemcpyAsync(h, words + W_TOTALS, sizeof(h), hipMemcpyDeviceToHost, stream));
    LBVH_TRY("waiting for a level", hipStreamSynchronize(stream));
    if (h[2] != 0 || size_t(A.levelBase) + count + h[0] > n || size_t(A.pairBase) + h[1] > n) {
      what = "a level overran its arrays (inconsistent tree)";
      return hipErrorUnknown;
    }
    out.levels.push_back(A.levelBase);
    A.levelBase += count, A.pairBase += h[1];
    count = h[0];
    std::swap(cur, next);
  }
  if (!out.abandoned) {
    out.nodeCount = A.levelBase, out.pairCount = A.pairBase;
    out.levels.push_back(out.nodeCount);
    hipLaunchKernelGGL(k_guard_pairs, dim3(1), dim3(64), 0, stream, S.pairs.get(), out.pairCount);
    LBVH_TRY("launching the guard pairs", hipGetLastError());
    LBVH_TRY("allocating the node array", out.nodes.reserve(out.nodeCount));
    LBVH_TRY("allocating the pair array", out.pairs.reserve(size_t(out.pairCount) + 3));
    LBVH_TRY("copying the nodes", hipMemcpyAsync(out.nodes.get(), S.nodes.get(), size_t(out.nodeCount) * sizeof(Bvh4Node), hipMemcpyDeviceToDevice, stream));
    LBVH_TRY("copying the pairs", hipMemcpyAsync(out.pairs.get(), S.pairs.get(), (size_t(out.pairCount) + 3) * sizeof(TriPair), hipMemcpyDeviceToDevice, stream));
  } else {
    out.depth = 0;
    out.levels.clear();
  }
  LBVH_TRY("recording the end", hipEventRecord(ev.b, stream));
  LBVH_TRY("waiting for the build", hipEventSynchronize(ev.b));
  LBVH_TRY("reading the build time", hipEventElapsedTime(&out.ms, ev.a, ev.b));
  return hipSuccess;
}

// ---- refit, host side --------------------------------------------------------------------------------------------------
size_t RefitScratch::bytes() const {
  return (nodeBox.size() + pairBox.size()) * sizeof(float) + (terms.size() + sum.size()) * sizeof(double) + reduceTemp.size() +
         words.size() * sizeof(uint32_t);
}

hipError_t packRecords(float const* verts9, uint32_t n, TriIsect* tris, TriPost* post, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_records, dim3(blocksFor(n)), dim3(kBlock), 0, stream, verts9, n, tris, post);
  return hipGetLastError();
}

hipError_t refit(float const* verts, uint32_t strideFloats, uint32_t n, Bvh4Node* nodes, TriPair* pairs, uint32_t nodeCount, uint32_t pairCount,
                 std::vector<uint32_t> const& levels, hipStream_t stream, RefitScratch& S, std::string& what) {
  if (n == 0 || pairCount == 0 || nodeCount == 0 || levels.size() < 2 || levels.front() != 0 || levels.back() != nodeCount) {
    what = "no tree with level bounds to refit";
    return hipErrorInvalidValue;
  }
  for (size_t l = 0; l + 1 < levels.size(); ++l)
    if (levels[l] >= levels[l + 1]) {
      what = "level bounds out of order";
      return hipErrorInvalidValue;
    }
  char const* const allocStep = "allocating refit scratch";
  LBVH_TRY(allocStep, S.nodeBox.reserve(6 * size_t(nodeCount)));
  LBVH_TRY(allocStep, S.pairBox.reserve(6 * size_t(pairCount)));
  LBVH_TRY(allocStep, S.words.reserve(W_REFIT_WORDS));
  uint32_t* const words = S.words.get();
  LBVH_TRY("zeroing the refit words", hipMemsetAsync(words, 0, W_REFIT_WORDS * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_scene_max, dim3(std::min(blocksFor(n), 4096u)), dim3(kBlock), 0, stream, verts, strideFloats, n, words);
  hipLaunchKernelGGL(k_refit_pairs, dim3(blocksFor(pairCount + 3)), dim3(kBlock), 0, stream, verts, strideFloats, n, pairs, pairCount, words,
                     S.pairBox.get());
  LBVH_TRY("launching the pair kernels", hipGetLastError());
  for (size_t l = levels.size() - 1; l-- > 0;) {  // deepest level first
    uint32_t const first = levels[l], count = levels[l + 1] - first;
    hipLaunchKernelGGL(k_refit_level, dim3(blocksFor(count)), dim3(kBlock), 0, stream, nodes, first, count, nodeCount, pairCount, S.nodeBox.get(),
                       S.pairBox.get(), words);
  }
  LBVH_TRY("launching the level kernels", hipGetLastError());
  uint32_t bad = 0;
  LBVH_TRY("reading the refit flag", hipMemcpyAsync(&bad, words + W_REFIT_BAD, sizeof(bad), hipMemcpyDeviceToHost, stream));
  LBVH_TRY("waiting for the refit", hipStreamSynchronize(stream));
  if (bad) {
    what = "a reference of the tree left its arrays (inconsistent tree)";
    return hipErrorUnknown;
  }
  return hipSuccess;
}

hipError_t sahCost(Bvh4Node const* nodes, TriPair const* pairs, uint32_t nodeCount, uint32_t pairCount, hipStream_t stream, RefitScratch& S,
                   double& cost, std::string& what) {
  cost = 0.0;
  if (nodeCount == 0 || pairCount == 0) return hipSuccess;
  size_t reduceBytes = 0;
  LBVH_TRY("sizing the reduction", rocprim::reduce(nullptr, reduceBytes, static_cast<double*>(nullptr), static_cast<double*>(nullptr), 0.0,
                                                    size_t(nodeCount), rocprim::plus<double>(), stream));
  char const* const allocStep = "allocating cost scratch";
  LBVH_TRY(allocStep, S.terms.reserve(nodeCount));
  LBVH_TRY(allocStep, S.sum.reserve(1));
  LBVH_TRY(allocStep, S.reduceTemp.reserve(std::max<size_t>(reduceBytes, 16)));
  hipLaunchKernelGGL(k_refit_cost, dim3(blocksFor(nodeCount)), dim3(kBlock), 0, stream, nodes, nodeCount, pairs, pairCount, S.terms.get());
  LBVH_TRY("launching the cost kernel", hipGetLastError());
  size_t tempBytes = S.reduceTemp.size();
  LBVH_TRY("summing the cost terms", rocprim::reduce(S.reduceTemp.get(), tempBytes, S.terms.get(), S.sum.get(), 0.0, size_t(nodeCount),
                                                      rocprim::plus<double>(), stream));
  double sum = 0.0;
  Bvh4Node root;
  LBVH_TRY("reading the cost", hipMemcpyAsync(&sum, S.sum.get(), sizeof(sum), hipMemcpyDeviceToHost, stream));
  LBVH_TRY("reading the root", hipMemcpyAsync(&root, nodes, sizeof(root), hipMemcpyDeviceToHost, stream));
  LBVH_TRY("waiting for the cost", hipStreamSynchronize(stream));
  double const ra = refit::rootArea(root);
  cost = ra > 0.0 ? sum / ra : 0.0;
  return hipSuccess;
}

}  // namespace lbvh_gpu
}  // namespace dmt

// ---- host-only entry points (no GPU): the restatement and the tree checker -----------------------------------------------
using namespace dmt;

extern "C" {

int dmt_lbvh_reference(const float* xs, const float* ys, const float* zs, size_t count, int max_depth, void* nodes64, size_t node_cap,
                       uint32_t* pair_orig2, size_t pair_cap, uint32_t* node_count, uint32_t* pair_count, int* depth, int* abandoned) {
  if ((count && (!xs || !ys || !zs)) || count > 0x0FFFFFFFu) return DMT_ERR_INVALID;
  lbvh::Reference const r = lbvh::reference(xs, ys, zs, uint32_t(count), max_depth);
  size_t const npairs = r.pairTris.size() / 2;
  if (node_count) *node_count = uint32_t(r.nodes.size());
  if (pair_count) *pair_count = uint32_t(npairs);
  if (depth) *depth = r.depth;
  if (abandoned) *abandoned = r.abandoned ? 1 : 0;
  if (r.nodes.size() > node_cap || npairs > pair_cap || (!r.nodes.empty() && !nodes64) || (npairs && !pair_orig2)) return DMT_ERR_INVALID;
  if (!r.nodes.empty()) memcpy(nodes64, r.nodes.data(), r.nodes.size() * sizeof(Bvh4Node));
  if (npairs) memcpy(pair_orig2, r.pairTris.data(), r.pairTris.size() * sizeof(uint32_t));
  return DMT_OK;
}

int dmt_bvh_check(const void* nodes64, size_t node_count, const uint32_t* pair_orig2, size_t pair_count, const float* xs, const float* ys,
                  const float* zs, size_t count, int* depth, int* max_leaf, double* sah_cost) {
  if ((count && (!xs || !ys || !zs)) || count > 0x0FFFFFFFu || (node_count && !nodes64) || (pair_count && !pair_orig2)) return DMT_ERR_INVALID;
  bool const ok = bvh_build::check(static_cast<Bvh4Node const*>(nodes64), node_count, pair_orig2, pair_count, xs, ys, zs, count, depth, max_leaf,
                                   sah_cost);
  return ok ? DMT_OK : DMT_ERR_STATE;
}

int dmt_bvh_refit_reference(const void* nodes64, size_t node_count, const uint32_t* pair_orig2, size_t pair_count, const float* xs,
                            const float* ys, const float* zs, size_t count, void* nodes64_out) {
  if ((count && (!xs || !ys || !zs)) || count > 0x0FFFFFFFu || !node_count || !nodes64 || !nodes64_out || (pair_count && !pair_orig2))
    return DMT_ERR_INVALID;
  std::vector<Bvh4Node> out(node_count);  // the caller's array is written only on success
  if (!refit::reference(static_cast<Bvh4Node const*>(nodes64), node_count, pair_orig2, pair_count, xs, ys, zs, count, out.data(), nullptr))
    return DMT_ERR_STATE;
  memcpy(nodes64_out, out.data(), node_count * sizeof(Bvh4Node));
  return DMT_OK;
}

}  // extern "C"
