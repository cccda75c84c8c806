// bvh_gpu_build.hpp -- interface of the device LBVH builder (bvh_gpu_build.hip; the algorithm: lbvh.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

#include "bvh.hpp"
#include "devbuf.hpp"
#include "tri_records.hpp"

namespace dmt {
namespace lbvh_gpu {

// temporaries of a build; the context owns one and reuses it (arrays only ever grow)
struct Scratch {
  DevBuf<uint64_t> keys, keysSorted;   // [n]
  DevBuf<uint8_t> sortTemp;            // rocPRIM's temporary storage (sort and scan)
  DevBuf<uint32_t> left, right;        // [n - 1] children of the binary inner nodes, as refs
  DevBuf<uint32_t> parent;             // [2 n - 1] parent of every ref
  DevBuf<uint64_t> box;                // [2 n - 1][3] boxes of every ref: (lo x, lo y), (lo z, hi x), (hi y, hi z)
  DevBuf<uint32_t> words;              // zeroed per build: 16 reduction / total words, then [n - 1] arrival counters
  DevBuf<uint32_t> levelA, levelB;     // [n] refs of the current and the next level
  DevBuf<uint64_t> counts, offsets;    // [n] per entry: inner << 32 | leaves, and its exclusive scan
  DevBuf<Bvh4Node> nodes;              // [n] upper bounds; the result is copied out at its exact size
  DevBuf<TriPair> pairs;               // [n + 3]
  size_t bytes() const;
};

struct Result {
  DevBuf<Bvh4Node> nodes;  // exact size
  DevBuf<TriPair> pairs;   // pairCount + 3 guard pairs (bvh.hpp)
  uint32_t nodeCount = 0, pairCount = 0;
  int depth = 0;
  bool abandoned = false;  // the depth guard fired: no tree
  float ms = 0.f;          // HIP events around the build
  size_t tempBytes = 0;
  std::vector<uint32_t> levels;  // first node of every 4-wide level, then nodeCount (refit::levelBounds' form)
};

// Builds the tree of the n triangles at verts[i * strideFloats + 0 .. 8] (p0, p1, p2; device memory) on `stream` and
// waits for it.  Anything but hipSuccess: `what` names the step that failed.
hipError_t build(float const* verts, uint32_t strideFloats, uint32_t n, int maxDepth, hipStream_t stream, Scratch& S, Result& out,
                 std::string& what);

// ---- the refit (bvh.hpp namespace refit) ----
// scratch of a refit; the context owns one and reuses it (arrays only ever grow)
struct RefitScratch {
  DevBuf<float> nodeBox, pairBox;  // 6 floats (24 bytes) per node / per pair: the exact fp32 boxes
  DevBuf<double> terms, sum;       // one cost term per node; their sum
  DevBuf<uint8_t> reduceTemp;      // rocPRIM's temporary storage
  DevBuf<uint32_t> words;          // zeroed per refit: the padding scale, the inconsistency flag
  size_t bytes() const;
};

// TriIsect / TriPost of the n triangles at verts9[9 i .. 9 i + 8] (device memory), material ids kept; enqueued on `stream`
hipError_t packRecords(float const* verts9, uint32_t n, TriIsect* tris, TriPost* post, hipStream_t stream);
// Refits the tree in place to the vertices at verts[i * strideFloats + 0 .. 8]: pairs (and the three guard pairs) rewritten,
// every node re-encoded, level by level from the deepest.  levels: first node of every level, then nodeCount.  Waits for it.
hipError_t refit(float const* verts, uint32_t strideFloats, uint32_t n, Bvh4Node* nodes, TriPair* pairs, uint32_t nodeCount, uint32_t pairCount,
                 std::vector<uint32_t> const& levels, hipStream_t stream, RefitScratch& S, std::string& what);
// SAH cost of a tree on the device by bvh_build::check's definition (waits for it)
hipError_t sahCost(Bvh4Node const* nodes, TriPair const* pairs, uint32_t nodeCount, uint32_t pairCount, hipStream_t stream, RefitScratch& S,
                   double& cost, std::string& what);

}  // namespace lbvh_gpu
}  // namespace dmt
