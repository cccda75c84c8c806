// accel_state.hpp -- what a context keeps for the acceleration layer: the two trees, who builds them, what an update does to
// them, key 1 of the motion, and the cull tables of the brute-force pass.  The layer's helpers and entry points are in
// accel_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, the node and pair records of
// bvh.hpp, the record types of tri_records.hpp, CullCluster (cull_plan.hpp), the builder's scratch types and the two records
// of dmt_hip.h.
//
// What invalidates what.  "drop" frees a tree's arrays and zeroes its counts; nothing reads a dropped tree (requireTree,
// ensureMotionTree).  Under DMT_ACCEL_BVH a dropped tree is rebuilt before the call returns: the static tree by buildBvh,
// the motion tree by ensureMotionTree when key 1 exists.
//
//   call                                 static tree            motion tree + key 1    update record
//   dmt_upload_triangles                 drop (then rebuild)    drop both              counts and costs reset by the rebuild
//   dmt_update_vertices[_device], BVH    refit or drop+rebuild  drop both              filled; a rebuild resets counts and costs
//   the same under brute force           drop                   drop both              action NONE, update_ms
//   a refit that fails                   drop (half refitted)   (dropped already)      left as the failure found it
//   dmt_set_accel_build, other builder   drop (then rebuild)    kept: always the host  counts and costs reset by the rebuild
//                                                               builder's
//   dmt_set_motion                       kept                   drop both, new key 1,  kept
//                                                               (then rebuild)
//   dmt_clear_motion                     kept                   drop both              kept
//   dmt_set_accel(BVH)                   built if dropped       built if dropped       reset if the static tree was built
//
// The build record is of the static tree only and is rewritten by every build of it (adopt); without a static tree
// dmt_accel_build_info reports zero counts.  dmt_set_shutter, shadeThresholdEnv and the scratch buffers survive everything.
//
// The cull tables are of the soup's current positions: dmt_upload_triangles and both vertex updates plan them anew
// (planCullClusters, by bruteCull) and commit them with the records they were planned from; nothing else touches them.
// bruteCull is set once, from DMT_BRUTE_CULL when the context is created.
#pragma once

namespace {

// One 4-wide BVH on the device.  The static tree has no deltas; the motion tree has no level bounds (it is never refitted).
struct BvhTree {
  DevBuf<Bvh4Node> nodes;
  DevBuf<TriPair> pairs;            // leaf storage, + 3 guard records (packLeaves)
  DevBuf<TriPairDelta> deltas;      // motion tree: key 1 - key 0 of every pair, + 3 guard records
  uint32_t nodeCount = 0, pairCount = 0;
  int depth = 0;
  std::vector<uint32_t> levels;     // first node of every 4-wide level, then the node count (the refit's launches)
  double buildMs = 0.0;
  bool valid = false;
  void drop() { *this = BvhTree{}; }
};

// device tables of a cluster plan of the brute-force pass (uploadCullTables); clusterCount == 0: the pass tests every triangle
struct CullTables {
  DevBuf<TriIsect> always;
  DevBuf<uint32_t> idx;
  DevBuf<CullCluster> clusters;
  DevBuf<float> tri9;
  uint32_t alwaysCount = 0, clusterCount = 0;
};

struct AccelState {
  // the brute-force pass's culled clusters (cull_plan.hpp); none: the pass tests the soup's records for every ray
  int bruteCull = 2;  // DMT_BRUTE_CULL at context creation (A/B runs, tests): 0 no clusters, 1 sphere clusters only, unset both
  CullTables cull;
  BvhTree tree;                          // of the uploaded soup (key 0), built for DMT_ACCEL_BVH
  // motion blur (dmt_set_motion).  Key 0 is the context's soup; key 1 lives here and is dropped with it.  The
  // motion tree is a second tree beside the static one (which stays as it is: dmt_clear_motion restores every film byte
  // for byte), built by the host SAH builder over both keys' boxes.
  BvhTree motionTree;
  DevBuf<uint32_t> overflow;             // kBvhOverflowStack words per thread of the largest launch so far
  int shadeThresholdEnv = 0;             // DMT_BVH_SHADE_THRESHOLD from the environment, 0 = choose by tree size
  int blocksPerCUBvh = 0;
  int accelBuild = DMT_BVH_BUILD_HOST;   // dmt_set_accel_build: who builds the static tree
  dmt_accel_build_record buildRecord{};  // of the static tree (dmt_accel_build_info)
  lbvh_gpu::Scratch lbvhScratch;         // temporaries of the device builder, reused across builds
  // dmt_update_vertices: what an update does to the static tree (dmt_set_accel_update), the record of the last one
  int accelUpdate = DMT_BVH_UPDATE_REBUILD;
  double maxCostRatio = 0.0;             // DMT_BVH_UPDATE_AUTO's bound
  dmt_accel_update_record updateRecord{};
  bool costAtBuildKnown = false;         // updateRecord.sah_cost_at_build is of the current topology
  lbvh_gpu::RefitScratch refitScratch;   // boxes and cost terms of a refit, reused across updates
  bool haveMotion = false;
  float shutterOpen = 0.f, shutterClose = 1.f;  // dmt_set_shutter: survives scene uploads and dmt_set_camera, like the lens
  std::vector<float> h_xs1, h_ys1, h_zs1;       // key 1 (the motion tree's input)
  DevBuf<TriIsect> d_dtris;                     // D = B - A per triangle
  DevBuf<TriKey1> d_post1;                      // key-1 vertices
};

}  // namespace
