// accel_host.hpp -- the host side of the acceleration layer (accel_state.hpp): building, adopting, updating and dropping the
// two trees, key 1 of the motion, the cull tables of the brute-force pass, and the dmt_* entry points of all of these, the
// host-only ones that show a cull plan (cull_plan.hpp) among them.
//
// Part of dmt_hip.hip's translation unit, included once: after the host helpers it uses (dmt_ctx, HIP_TRY, fail, cull_plan.hpp's
// planners, camera_host.hpp's computeSamplerParams, resolutionOk and haltonIndices) and before scene_host.hpp, baseParams,
// denoise_host.hpp and probes.hpp, which call into it (soupArgsOk, uploadCullTables, dropMotion, buildBvh, bvhView, cullView,
// shadeThresholdFor, reserveOverflow, requireTree, motionParams).  The three calls the other way, packSoup of scene_host.hpp and
// the vertex updates into denoise_host.hpp's mirror, are the forward declarations below.
#pragma once

namespace {

void packSoup(float const* xs, float const* ys, float const* zs, uint32_t const* mat, size_t count, std::vector<TriIsect>& a, std::vector<TriPost>& b);  // scene_host.hpp
int mirrorHostUpdate(dmt_ctx* ctx);                                         // denoise_host.hpp
int mirrorDeviceUpdate(dmt_ctx* ctx, void const* d_verts9, size_t count);  // denoise_host.hpp

BvhView bvhView(dmt_ctx const* c, size_t threads) {
  BvhView b;
  b.nodes = c->ac.tree.nodes.get(), b.pairs = c->ac.tree.pairs.get(), b.overflow = c->ac.overflow.get();
  b.overflowStride = uint32_t(threads);
  return b;
}

// the brute-force pass's tables; without clusters the pass tests the soup's records for every ray
CullView cullView(dmt_ctx const* c) {
  CullView v{};
  if (c->ac.cull.clusterCount > 0) {
    v.always = c->ac.cull.always.get(), v.alwaysIdx = c->ac.cull.idx.get(), v.clusters = c->ac.cull.clusters.get();
    v.tri9 = c->ac.cull.tri9.get(), v.alwaysCount = c->ac.cull.alwaysCount, v.clusterCount = c->ac.cull.clusterCount;
  } else {
    v.always = c->scene.tris.get(), v.alwaysCount = c->scene.triCount;
  }
  return v;
}

// BVH megakernel: how many lanes of a wave must have finished their rays before the wave stops traversing and shades
// (megakernel_body_bvh, step C).  Traversing lanes idle while the wave shades and finished lanes idle while it traverses, so
// the best value follows the cost ratio of the two -- low where rays take hundreds of steps, high where the tree is shallow
// and shading dominates.  Measured on MI355X, Msamples/s by threshold (profiles/r03/shade_threshold_sweep.txt):
//   Cornell box, 6 nodes, depth 3             32: 1 923   48: 2 184   56: 2 266   60: 2 244   64: 2 053
//   sphere.fbx + veranda, 123 nodes, depth 5  32: 6 867   48: 7 416   56: 7 683   64: 7 800
//   tessellated sphere, 4 588 nodes, depth 10 32: 3 043   48: 3 381   52: 3 399   56: 3 365   64: 2 748
//   1 M random triangles, 300 k nodes         28: 490     32: 489     36: 485     40: 473     48: 452
//   16 M random triangles                     24: 435     28: 439     32: 437     36: 436
// The step between 16 k and 128 k nodes is interpolated, not measured.  DMT_BVH_SHADE_THRESHOLD in the environment overrides
// the choice (tuning runs).  Results do not depend on it.  nodeCount: of the tree the launch traverses, static or motion.
int shadeThresholdFor(dmt_ctx const* c, uint32_t nodeCount) {
  if (c->ac.shadeThresholdEnv > 0) return c->ac.shadeThresholdEnv;
  return nodeCount <= 1024u ? 56 : nodeCount <= 16384u ? 52 : nodeCount <= 131072u ? 40 : DMT_BVH_SHADE_THRESHOLD;
}

// BVH traversal-stack overflow area for `threads` threads
hipError_t reserveOverflow(dmt_ctx* ctx, size_t threads) { return ctx->ac.overflow.reserve(threads * size_t(kBvhOverflowStack)); }

// what every launch that traverses the static tree asks first
int requireTree(dmt_ctx* ctx, char const* caller) {
  if (ctx->ac.tree.valid) return DMT_OK;
  ctx->err = std::string(caller) + ": BVH not built";
  return DMT_ERR_STATE;
}

// a builder made a new topology: the update record counts refits from here, costs are of the tree before
void treeBuilt(dmt_ctx* ctx) {
  ctx->ac.updateRecord.updates_since_build = 0;
  ctx->ac.updateRecord.sah_cost = ctx->ac.updateRecord.sah_cost_at_build = 0.0;
  ctx->ac.costAtBuildKnown = false;
}

// A built tree becomes the static one, and the build record describes it.  Both builders' results come through here.
void adopt(dmt_ctx* ctx, BvhTree&& t, int builder, size_t tempBytes) {
  AccelState& A = ctx->ac;
  A.tree = std::move(t);
  A.tree.valid = true;
  treeBuilt(ctx);
  dmt_accel_build_record& R = A.buildRecord;
  R = dmt_accel_build_record{};
  R.builder = builder;
  R.triangles = ctx->scene.triCount, R.nodes = A.tree.nodeCount, R.pairs = A.tree.pairCount, R.depth = A.tree.depth;
  R.build_ms = A.tree.buildMs, R.temp_bytes = tempBytes;
}

// delta record = key-1 record - key-0 record over their n leading float fields, one fp32 subtraction per field; the words
// behind them (material id, pads) stay as D has them
static_assert(offsetof(TriIsect, matId) == 9 * sizeof(float), "TriIsect: nine floats, then the words");
static_assert(offsetof(TriPair, orig) == 18 * sizeof(float) && offsetof(TriPairDelta, pad) == 18 * sizeof(float), "pair records: eighteen floats, then the words");
template <class D, class R>
void deltaRecord(D& d, R const& b, R const& a, int n) {
  float* const fd = reinterpret_cast<float*>(&d);
  float const *const fb = reinterpret_cast<float const*>(&b), *const fa = reinterpret_cast<float const*>(&a);
  for (int k = 0; k < n; ++k) fd[k] = fb[k] - fa[k];
}

// Leaf storage of a host-built tree: the TriPair of every pair of `pairTris` from the key-0 soup -- edges are the reference's
// own subtractions (CC/private/shapes.cu:10-11) in IEEE fp32, refit::packPairHalf -- and, when there is a key 1, D = (key-1
// pair) - (key-0 pair) field by field: the numbers of d_tris / d_dtris in the pairs' interleaving.  key[a]: the soup's xs, ys,
// zs.  Each array ends in 3 guard records (copies of the last one).  An EMPTY child slot holds an inverted quantised box and
// no reference of its own; its slab test misses by itself except in one corner: a ray exactly parallel to an axis through a
// node that is flat on the remaining axes (255 quantisation steps below half an ulp of the plane distance), where near ==
// far.  The slot's implicit reference is then leafRef + slot, i.e. a pair of the NEXT node -- or, for the last node, up to
// three pairs past the array.  Testing some real triangle of the scene once more changes no result (the triangle test
// decides hits, and a scene triangle is a scene triangle); reading past the array would, hence the guards.
void packLeaves(std::vector<uint32_t> const& pairTris, float const* const key0[3], float const* const* key1, std::vector<TriPair>& pairs,
                std::vector<TriPairDelta>& deltas) {
  size_t const npairs = pairTris.size() / 2;
  pairs.assign(npairs ? npairs + 3 : 0, TriPair{});
  deltas.assign(key1 ? pairs.size() : 0, TriPairDelta{});
  auto verts = [](float const* const* key, uint32_t i, float v[9]) {
    for (int c = 0; c < 3; ++c) v[3 * c] = key[0][4 * size_t(i) + c], v[3 * c + 1] = key[1][4 * size_t(i) + c], v[3 * c + 2] = key[2][4 * size_t(i) + c];
  };
  for (size_t p = 0; p < npairs; ++p) {
    TriPair B{};
    for (int half = 0; half < 2; ++half) {
      uint32_t const i = pairTris[2 * p + size_t(half)];
      float v[9];
      verts(key0, i, v), refit::packPairHalf(pairs[p], half, v, i);
      if (key1) verts(key1, i, v), refit::packPairHalf(B, half, v, i);
    }
    if (key1) deltaRecord(deltas[p], B, pairs[p], 18);
  }
  for (size_t p = npairs; p < pairs.size(); ++p) {
    pairs[p] = pairs[npairs - 1];
    if (key1) deltas[p] = deltas[npairs - 1];
  }
}

// the host builder's result on the device: nodes, leaves (packLeaves), counts and depth of `t`; tooMany: the tree's own text
int uploadHostTree(dmt_ctx* ctx, bvh_build::Result const& r, float const* const key0[3], float const* const* key1, char const* tooMany, BvhTree& t) {
  if (r.pairTris.size() / 2 > 0x7FFFFFFFull || r.nodes.size() > 0x7FFFFFFFull) return fail(ctx, DMT_ERR_INVALID, tooMany);
  std::vector<TriPair> pairs;
  std::vector<TriPairDelta> deltas;
  packLeaves(r.pairTris, key0, key1, pairs, deltas);
  HIP_TRY(ctx, t.nodes.assign(r.nodes.data(), r.nodes.size()));
  HIP_TRY(ctx, t.pairs.assign(pairs.data(), pairs.size()));
  if (key1) HIP_TRY(ctx, t.deltas.assign(deltas.data(), deltas.size()));
  t.nodeCount = uint32_t(r.nodes.size()), t.pairCount = uint32_t(r.pairTris.size() / 2), t.depth = r.depth;
  return DMT_OK;
}

// (re)build the 4-wide BVH of the uploaded soup on the host and upload nodes + triangle pairs
int buildBvhHost(dmt_ctx* ctx, int builder) {
  auto const t0 = std::chrono::steady_clock::now();
  bvh_build::Result r = bvh_build::build(ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data(), ctx->scene.triCount);
  float const* const key0[3] = {ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data()};
  BvhTree t;
  if (int const rc = uploadHostTree(ctx, r, key0, nullptr, "BVH: too many nodes / triangle pairs", t)) return rc;
  t.levels = refit::levelBounds(r.nodes.data(), r.nodes.size());
  t.buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();  // build, pair packing, copies
  adopt(ctx, std::move(t), builder, 0);
  return DMT_OK;
}

// the tree of the uploaded soup, by the builder dmt_set_accel_build chose
int buildBvh(dmt_ctx* ctx) {
  AccelState& A = ctx->ac;
  if (A.accelBuild != DMT_BVH_BUILD_DEVICE) return buildBvhHost(ctx, DMT_BVH_BUILT_BY_HOST);
  static_assert(sizeof(TriPost) == 64 && offsetof(TriPost, p2z) == 32, "the device builder reads p0, p1, p2 as nine consecutive floats");
  lbvh_gpu::Result r;
  std::string what;
  hipError_t const e = lbvh_gpu::build(reinterpret_cast<float const*>(ctx->scene.post.get()), uint32_t(sizeof(TriPost) / sizeof(float)),
                                       ctx->scene.triCount, kBvhMaxDepth, ctx->stream, A.lbvhScratch, r, what);
  if (e != hipSuccess) {  // an error, not a silent host build
    ctx->err = "device BVH build: " + what + ": " + hipGetErrorName(e) + " - " + hipGetErrorString(e);
    return DMT_ERR_HIP;
  }
  if (r.abandoned) {  // the depth guard: the traversal stack is sized by kBvhMaxDepth
    int const rc = buildBvhHost(ctx, DMT_BVH_BUILT_BY_HOST_AFTER_DEVICE);
    if (rc == DMT_OK) A.buildRecord.build_ms = A.tree.buildMs += double(r.ms), A.buildRecord.temp_bytes = r.tempBytes;  // the lost attempt counts
    return rc;
  }
  if (r.pairCount > 0x7FFFFFFFull || r.nodeCount > 0x7FFFFFFFull) return fail(ctx, DMT_ERR_INVALID, "BVH: too many nodes / triangle pairs");
  BvhTree t;
  t.nodes = std::move(r.nodes), t.pairs = std::move(r.pairs);
  t.nodeCount = r.nodeCount, t.pairCount = r.pairCount, t.depth = r.depth;
  t.levels = std::move(r.levels);
  t.buildMs = double(r.ms);
  adopt(ctx, std::move(t), DMT_BVH_BUILT_BY_DEVICE, r.tempBytes);
  return DMT_OK;
}

// ---- motion blur: key 1 on the host side ----
void dropMotion(dmt_ctx* ctx) {  // the positions key 1 was a motion FROM are going away
  AccelState& A = ctx->ac;
  A.haveMotion = false, A.motionTree.drop();
  A.h_xs1.clear(), A.h_ys1.clear(), A.h_zs1.clear();
  A.d_dtris.reset(), A.d_post1.reset();
}
// The motion tree: the host SAH builder over every triangle's union box of both keys, whatever dmt_set_accel_build says (the
// device builder and the refit know one key).  Leaves: the key-0 pairs and their deltas (packLeaves).
int ensureMotionTree(dmt_ctx* ctx) {
  AccelState& A = ctx->ac;
  if (A.motionTree.valid) return DMT_OK;
  auto const t0 = std::chrono::steady_clock::now();
  float const* const key0[3] = {ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data()};
  float const* const key1[3] = {A.h_xs1.data(), A.h_ys1.data(), A.h_zs1.data()};
  bvh_build::Result r = bvh_build::build(key0[0], key0[1], key0[2], ctx->scene.triCount, key1[0], key1[1], key1[2]);
  BvhTree t;
  if (int const rc = uploadHostTree(ctx, r, key0, key1, "motion BVH: too many nodes / triangle pairs", t)) return rc;
  t.buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  t.valid = true;
  A.motionTree = std::move(t);
  return DMT_OK;
}
// What a launch of a *_motion kernel reads beside baseParams: the delta records, key 1, the shutter, and for a BVH mask the
// motion tree in place of the static one (after the caller has set P.bvh's overflow stack for its launch).
int motionParams(dmt_ctx* ctx, uint32_t F, RenderParams& P) {
  if (!(F & kFeatMotion)) return DMT_OK;
  AccelState const& A = ctx->ac;
  P.motion.dtris = A.d_dtris.get(), P.motion.post1 = A.d_post1.get();
  P.motion.open = A.shutterOpen, P.motion.close = A.shutterClose;
  if (F & kFeatBvh) {
    if (int const rc = ensureMotionTree(ctx)) return rc;
    P.bvh.nodes = A.motionTree.nodes.get(), P.bvh.pairs = A.motionTree.pairs.get(), P.motion.pairDelta = A.motionTree.deltas.get();
    P.shadeThreshold = shadeThresholdFor(ctx, A.motionTree.nodeCount);
  }
  return DMT_OK;
}

// ---- the brute-force pass's cluster tables ----
// what every call that takes a soup with its material ids checks first
bool soupArgsOk(float const* xs, float const* ys, float const* zs, uint32_t const* mat, size_t count) {
  return !((count && (!xs || !ys || !zs || !mat)) || count > 0x7FFFFFFFu);
}

// device tables of a cluster plan; a = the soup's TriIsect records (read only when there are clusters).  The caller adopts
// them when everything else of its call has succeeded: ctx->ac.cull = std::move(T)
int uploadCullTables(dmt_ctx* ctx, std::vector<CullCluster> const& clusters, TriIsect const* a, size_t count, CullTables& T) {
  T.alwaysCount = uint32_t(count), T.clusterCount = uint32_t(clusters.size());
  if (clusters.empty()) return DMT_OK;
  std::vector<uint8_t> culled(count, 0);
  std::vector<float> tri9(9 * kCullMaxTris, 0.f);
  for (CullCluster const& cl : clusters)
    for (uint32_t j = 0; j < cl.count; ++j) {
      TriIsect const& t = a[cl.first + j];
      float const f[9] = {t.p0x, t.p0y, t.p0z, t.e0x, t.e0y, t.e0z, t.e1x, t.e1y, t.e1z};
      for (int q = 0; q < 9; ++q) tri9[q * kCullMaxTris + cl.slot + j] = f[q];
      culled[cl.first + j] = 1;
    }
  std::vector<TriIsect> always;
  std::vector<uint32_t> idx;
  for (size_t i = 0; i < count; ++i)
    if (!culled[i]) always.push_back(a[i]), idx.push_back(uint32_t(i));
  std::vector<CullCluster> table(kCullMaxClusters, CullCluster{});
  std::copy(clusters.begin(), clusters.end(), table.begin());
  T.alwaysCount = uint32_t(always.size());
  HIP_TRY(ctx, T.always.assign(always.data(), always.size()));
  HIP_TRY(ctx, T.idx.assign(idx.data(), idx.size()));
  HIP_TRY(ctx, T.clusters.assign(table.data(), table.size()));
  HIP_TRY(ctx, T.tri9.assign(tri9.data(), tri9.size()));
  return DMT_OK;
}

// ---- dmt_update_vertices: timing and the update policy ----
int lbvhError(dmt_ctx* ctx, char const* stage, std::string const& what, hipError_t e) {
  ctx->err = std::string(stage) + ": " + what + ": " + hipGetErrorName(e) + " - " + hipGetErrorString(e);
  return DMT_ERR_HIP;
}
int treeCost(dmt_ctx* ctx, double& cost) {
  BvhTree const& t = ctx->ac.tree;
  std::string what;
  hipError_t const e = lbvh_gpu::sahCost(t.nodes.get(), t.pairs.get(), t.nodeCount, t.pairCount, ctx->stream, ctx->ac.refitScratch, cost, what);
  return e == hipSuccess ? DMT_OK : lbvhError(ctx, "BVH cost", what, e);
}

// The records, cull tables and host mirrors hold the new positions; T.a is recorded on the idle stream.  Applies
// dmt_set_accel_update's policy to the tree and fills the update record.
int finishUpdate(dmt_ctx* ctx, EventPair& T) {
  AccelState& A = ctx->ac;
  dmt_accel_update_record& U = A.updateRecord;
  bool const bvh = ctx->accel == DMT_ACCEL_BVH;
  bool const refitting = bvh && A.tree.valid && A.accelUpdate != DMT_BVH_UPDATE_REBUILD && A.tree.levels.size() >= 2;
  bool rebuild = bvh && !refitting;
  if (!bvh) A.tree.drop();  // as an upload does
  U.action = DMT_BVH_UPDATED_NONE;
  if (refitting) {
    if (!A.costAtBuildKnown) {  // the nodes still are the builder's: the refit has not run yet
      if (int const rc = treeCost(ctx, U.sah_cost_at_build)) return rc;
      A.costAtBuildKnown = true;
    }
    static_assert(sizeof(TriPost) == 64 && offsetof(TriPost, p2z) == 32, "the refit reads p0, p1, p2 as nine consecutive floats");
    std::string what;
    hipError_t const e = lbvh_gpu::refit(reinterpret_cast<float const*>(ctx->scene.post.get()), uint32_t(sizeof(TriPost) / sizeof(float)), ctx->scene.triCount,
                                         A.tree.nodes.get(), A.tree.pairs.get(), A.tree.nodeCount, A.tree.pairCount, A.tree.levels, ctx->stream,
                                         A.refitScratch, what);
    if (e != hipSuccess) {
      A.tree.drop();  // the tree may be half refitted
      return lbvhError(ctx, "BVH refit", what, e);
    }
    if (int const rc = treeCost(ctx, U.sah_cost)) return rc;
    U.action = DMT_BVH_UPDATED_REFIT;
    ++U.updates_since_build;
    rebuild = A.accelUpdate == DMT_BVH_UPDATE_AUTO && U.sah_cost > A.maxCostRatio * U.sah_cost_at_build;
  }
  HIP_TRY(ctx, hipEventRecord(T.b, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(T.b));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, T.a, T.b));
  U.update_ms = double(ms);
  if (rebuild) {
    A.tree.drop();  // a build that fails leaves no tree, not the old positions'
    if (int const rc = buildBvh(ctx)) return rc;  // resets updates_since_build and the costs
    U.action = refitting ? DMT_BVH_UPDATED_REBUILD_AFTER_REFIT : DMT_BVH_UPDATED_REBUILD;
    U.update_ms += A.buildRecord.build_ms;
    if (A.accelUpdate != DMT_BVH_UPDATE_REBUILD) {
      if (int const rc = treeCost(ctx, U.sah_cost)) return rc;
      U.sah_cost_at_build = U.sah_cost;
      A.costAtBuildKnown = true;
    }
  }
  U.temp_bytes = A.refitScratch.bytes();
  return DMT_OK;
}

// common entry of the two updates: argument and state checks, the stream drained, the timer started.  *done: nothing to do
int beginUpdate(dmt_ctx* ctx, char const* name, bool nullArray, size_t count, EventPair& T, bool* done) {
  *done = false;
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "update of vertices before any dmt_upload_triangles");
  if (count != ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "update of vertices: count differs from the uploaded triangle count");
  if (count && nullArray) {
    ctx->err = std::string(name) + ": null array";
    return DMT_ERR_INVALID;
  }
  if (count == 0) {
    *done = true;
    return DMT_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the old records
  HIP_TRY(ctx, hipEventCreate(&T.a));
  HIP_TRY(ctx, hipEventCreate(&T.b));
  HIP_TRY(ctx, hipEventRecord(T.a, ctx->stream));
  return DMT_OK;
}

bool shutterOk(float open, float close) { return std::isfinite(open) && std::isfinite(close) && 0.f <= open && open <= close && close <= 1.f; }

}  // namespace

extern "C" {

int dmt_update_vertices(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs, size_t count) {
  EventPair T;
  bool done = false;
  if (int const rc = beginUpdate(ctx, "dmt_update_vertices", !xs || !ys || !zs, count, T, &done)) return rc;
  if (done) return DMT_OK;
  dropMotion(ctx);  // key 1 was a motion from the positions being replaced
  ctx->lights.invalidateEmitters();  // and the emitter tree was built over them
  std::vector<TriIsect> a;
  std::vector<TriPost> b;
  packSoup(xs, ys, zs, ctx->scene.h_mat.data(), count, a, b);
  CullTables cull;
  if (int const rcC = uploadCullTables(ctx, planCullClusters(ctx->ac.bruteCull, CullSoup{xs, ys, zs, ctx->scene.h_mat.data(), uint32_t(count)}), a.data(), count, cull)) return rcC;
  HIP_TRY(ctx, hipMemcpy(ctx->scene.tris.get(), a.data(), count * sizeof(TriIsect), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->scene.post.get(), b.data(), count * sizeof(TriPost), hipMemcpyHostToDevice));
  ctx->ac.cull = std::move(cull);
  ctx->scene.h_xs.assign(xs, xs + 4 * count), ctx->scene.h_ys.assign(ys, ys + 4 * count), ctx->scene.h_zs.assign(zs, zs + 4 * count);
  if (int const rcT = mirrorHostUpdate(ctx)) return rcT;
  return finishUpdate(ctx, T);
}

int dmt_update_vertices_device(dmt_ctx* ctx, const void* d_verts9, size_t count) {
  EventPair T;
  bool done = false;
  if (int const rc = beginUpdate(ctx, "dmt_update_vertices_device", !d_verts9, count, T, &done)) return rc;
  if (done) return DMT_OK;
  dropMotion(ctx);  // key 1 was a motion from the positions being replaced
  ctx->lights.invalidateEmitters();  // and the emitter tree was built over them
  HIP_TRY(ctx, lbvh_gpu::packRecords(static_cast<float const*>(d_verts9), uint32_t(count), ctx->scene.tris.get(), ctx->scene.post.get(), ctx->stream));
  if (int const rcT = mirrorDeviceUpdate(ctx, d_verts9, count)) return rcT;
  // the host mirrors (the host builder's, the cull plan's and a later rebuild's input) from the records just made
  std::vector<TriPost> b(count);
  HIP_TRY(ctx, hipMemcpyAsync(b.data(), ctx->scene.post.get(), count * sizeof(TriPost), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < count; ++i) {
    TriPost const& q = b[i];
    ctx->scene.h_xs[4 * i] = q.p0x, ctx->scene.h_xs[4 * i + 1] = q.p1x, ctx->scene.h_xs[4 * i + 2] = q.p2x;
    ctx->scene.h_ys[4 * i] = q.p0y, ctx->scene.h_ys[4 * i + 1] = q.p1y, ctx->scene.h_ys[4 * i + 2] = q.p2y;
    ctx->scene.h_zs[4 * i] = q.p0z, ctx->scene.h_zs[4 * i + 1] = q.p1z, ctx->scene.h_zs[4 * i + 2] = q.p2z;
  }
  std::vector<CullCluster> const clusters = planCullClusters(ctx->ac.bruteCull, CullSoup{ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data(), ctx->scene.h_mat.data(), uint32_t(count)});
  std::vector<TriIsect> a;
  if (!clusters.empty()) {  // the cluster tables copy TriIsect records: the kernel's own
    a.resize(count);
    HIP_TRY(ctx, hipMemcpy(a.data(), ctx->scene.tris.get(), count * sizeof(TriIsect), hipMemcpyDeviceToHost));
  }
  CullTables cull;
  if (int const rcC = uploadCullTables(ctx, clusters, a.data(), count, cull)) return rcC;
  ctx->ac.cull = std::move(cull);
  return finishUpdate(ctx, T);
}

int dmt_set_accel_update(dmt_ctx* ctx, int mode, double max_cost_ratio) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_BVH_UPDATE_REBUILD && mode != DMT_BVH_UPDATE_REFIT && mode != DMT_BVH_UPDATE_AUTO)
    return fail(ctx, DMT_ERR_INVALID, "dmt_set_accel_update: unknown mode");
  if (mode == DMT_BVH_UPDATE_AUTO && !(std::isfinite(max_cost_ratio) && max_cost_ratio > 1.0))
    return fail(ctx, DMT_ERR_INVALID, "dmt_set_accel_update: DMT_BVH_UPDATE_AUTO needs a finite max_cost_ratio > 1");
  ctx->ac.accelUpdate = mode;
  if (mode == DMT_BVH_UPDATE_AUTO) ctx->ac.maxCostRatio = max_cost_ratio;
  return DMT_OK;
}

int dmt_accel_update_info(dmt_ctx* ctx, dmt_accel_update_record* out) {
  if (!ctx || !out) return DMT_ERR_INVALID;
  *out = ctx->ac.updateRecord;
  return DMT_OK;
}

int dmt_set_accel(dmt_ctx* ctx, int mode) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_ACCEL_BRUTE_FORCE && mode != DMT_ACCEL_BVH) return fail(ctx, DMT_ERR_INVALID, "dmt_set_accel: unknown mode");
  ctx->accel = mode;
  if (mode == DMT_ACCEL_BVH && ctx->scene.haveTris && !ctx->ac.tree.valid) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int const rc = buildBvh(ctx)) return rc;
  }
  if (mode == DMT_ACCEL_BVH && ctx->ac.haveMotion) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ensureMotionTree(ctx);
  }
  return DMT_OK;
}

int dmt_set_accel_build(dmt_ctx* ctx, int mode) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_BVH_BUILD_HOST && mode != DMT_BVH_BUILD_DEVICE) return fail(ctx, DMT_ERR_INVALID, "dmt_set_accel_build: unknown mode");
  if (mode == ctx->ac.accelBuild) return DMT_OK;
  ctx->ac.accelBuild = mode;
  ctx->ac.tree.drop();  // the current tree is the other builder's
  if (ctx->accel == DMT_ACCEL_BVH && ctx->scene.haveTris) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight still read the old tree
    return buildBvh(ctx);
  }
  return DMT_OK;
}

int dmt_accel_build_info(dmt_ctx* ctx, dmt_accel_build_record* out) {
  if (!ctx || !out) return DMT_ERR_INVALID;
  if (!ctx->ac.tree.valid) {  // no tree: the builder the next build will use, zero counts
    *out = dmt_accel_build_record{};
    out->builder = ctx->ac.accelBuild == DMT_BVH_BUILD_DEVICE ? DMT_BVH_BUILT_BY_DEVICE : DMT_BVH_BUILT_BY_HOST;
    return DMT_OK;
  }
  *out = ctx->ac.buildRecord;
  return DMT_OK;
}

int dmt_accel_download(dmt_ctx* ctx, void* nodes64, size_t node_cap, uint32_t* pair_orig2, size_t pair_cap) {
  if (!ctx) return DMT_ERR_INVALID;
  BvhTree const& t = ctx->ac.tree;
  if (!t.valid) return fail(ctx, DMT_ERR_STATE, "dmt_accel_download: no tree (set DMT_ACCEL_BVH and upload triangles first)");
  if (node_cap < t.nodeCount || pair_cap < t.pairCount || (t.nodeCount && !nodes64) || (t.pairCount && !pair_orig2))
    return fail(ctx, DMT_ERR_INVALID, "dmt_accel_download: arrays too small (see dmt_accel_build_info)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(nodes64, t.nodes.get(), size_t(t.nodeCount) * sizeof(Bvh4Node), hipMemcpyDeviceToHost));
  std::vector<TriPair> pairs(t.pairCount);
  if (!pairs.empty()) HIP_TRY(ctx, hipMemcpy(pairs.data(), t.pairs.get(), pairs.size() * sizeof(TriPair), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < pairs.size(); ++p) pair_orig2[2 * p] = pairs[p].orig[0], pair_orig2[2 * p + 1] = pairs[p].orig[1];
  return DMT_OK;
}

// Host-only: build the BVH of a soup and check its invariants (every triangle in exactly one leaf, every DECODED
// (quantised) child box encloses all vertices below it and lies inside its parent's decoded box up to one quantisation
// step, inner children first with consecutive indices, depth within the traversal-stack bound).
int dmt_bvh_validate(const float* xs, const float* ys, const float* zs, size_t count, int* node_count, int* depth,
                     int* max_leaf) {
  if ((count && (!xs || !ys || !zs)) || count > 0x0FFFFFFFu) return DMT_ERR_INVALID;
  bvh_build::Result const r = bvh_build::build(xs, ys, zs, uint32_t(count));
  if (node_count) *node_count = int(r.nodes.size());
  if (depth) *depth = r.depth;
  bool const ok = bvh_build::check(r.nodes.data(), r.nodes.size(), r.pairTris.data(), r.pairTris.size() / 2, xs, ys, zs, count, nullptr,
                                   max_leaf, nullptr);
  return ok && r.depth <= kBvhMaxDepth ? DMT_OK : DMT_ERR_STATE;
}

// ---- motion blur -------------------------------------------------------------------------
int dmt_set_motion(dmt_ctx* ctx, const float* xs1, const float* ys1, const float* zs1, size_t count) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_set_motion: before any dmt_upload_triangles");
  if (count != ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "dmt_set_motion: count differs from the uploaded triangle count");
  if (count && (!xs1 || !ys1 || !zs1)) return fail(ctx, DMT_ERR_INVALID, "dmt_set_motion: null array");
  for (size_t k = 0; k < 4 * count; ++k) {
    if ((k & 3) == 3) continue;  // the SoA's pad lane
    if (!std::isfinite(xs1[k]) || !std::isfinite(ys1[k]) || !std::isfinite(zs1[k])) return fail(ctx, DMT_ERR_INVALID, "dmt_set_motion: a position is not finite");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the old key 1
  std::vector<TriIsect> a, b;
  std::vector<TriPost> pa, pb;
  packSoup(ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data(), ctx->scene.h_mat.data(), count, a, pa);  // A: the records the context holds
  packSoup(xs1, ys1, zs1, ctx->scene.h_mat.data(), count, b, pb);
  std::vector<TriIsect> d(count);  // zeroed: the material id and the pads of a delta record
  std::vector<TriKey1> q(count);
  for (size_t i = 0; i < count; ++i) {  // D = B - A, component by component in fp32
    deltaRecord(d[i], b[i], a[i], 9);
    TriPost const& P = pb[i];
    q[i] = TriKey1{P.p0x, P.p0y, P.p0z, P.p1x, P.p1y, P.p1z, P.p2x, P.p2y, P.p2z, 0.f, 0.f, 0.f};
  }
  DevBuf<TriIsect> dd;
  DevBuf<TriKey1> dq;
  HIP_TRY(ctx, dd.assign(d.data(), count));
  HIP_TRY(ctx, dq.assign(q.data(), count));
  dropMotion(ctx);
  AccelState& A = ctx->ac;
  A.d_dtris = std::move(dd), A.d_post1 = std::move(dq);
  A.h_xs1.assign(xs1, xs1 + 4 * count), A.h_ys1.assign(ys1, ys1 + 4 * count), A.h_zs1.assign(zs1, zs1 + 4 * count);
  A.haveMotion = true;
  if (ctx->accel == DMT_ACCEL_BVH) return ensureMotionTree(ctx);
  return DMT_OK;
}

int dmt_clear_motion(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->ac.haveMotion) return DMT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read key 1
  dropMotion(ctx);
  return DMT_OK;
}

int dmt_set_shutter(dmt_ctx* ctx, float open, float close) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!shutterOk(open, close)) return fail(ctx, DMT_ERR_INVALID, "dmt_set_shutter: needs finite 0 <= open <= close <= 1");
  ctx->ac.shutterOpen = open, ctx->ac.shutterClose = close;
  return DMT_OK;
}

int dmt_motion_info(dmt_ctx* ctx, int* keys, float* open, float* close, uint32_t* tree_nodes, uint32_t* tree_pairs, double* tree_build_ms) {
  if (!ctx) return DMT_ERR_INVALID;
  AccelState const& A = ctx->ac;  // a dropped motion tree has zero counts and time
  if (keys) *keys = ctx->scene.haveTris ? (A.haveMotion ? 2 : 1) : 0;
  if (open) *open = A.shutterOpen;
  if (close) *close = A.shutterClose;
  if (tree_nodes) *tree_nodes = A.motionTree.nodeCount;
  if (tree_pairs) *tree_pairs = A.motionTree.pairCount;
  if (tree_build_ms) *tree_build_ms = A.motionTree.buildMs;
  return DMT_OK;
}

int dmt_shutter_times(int width, int height, float open, float close, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* t) {
  if (!resolutionOk(width, height) || n < 0 || !shutterOk(open, close)) return DMT_ERR_INVALID;
  if (n && (!pxs || !pys || !ss || !t)) return DMT_ERR_INVALID;
  std::vector<int32_t> hs;
  if (!haltonIndices(computeSamplerParams(width, height), width, height, n, pxs, pys, ss, hs)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) t[i] = shutter_time(uint32_t(hs[size_t(i)]), open, close);
  return DMT_OK;
}

int dmt_motion_positions(const float* xs0, const float* ys0, const float* zs0, const float* xs1, const float* ys1, const float* zs1, size_t count,
                         float t, float* xs, float* ys, float* zs) {
  if (!std::isfinite(t) || (count && (!xs0 || !ys0 || !zs0 || !xs1 || !ys1 || !zs1 || !xs || !ys || !zs))) return DMT_ERR_INVALID;
  for (size_t k = 0; k < 4 * count; ++k) {
    bool const pad = (k & 3) == 3;  // the SoA's pad lane: key 0's
    xs[k] = pad ? xs0[k] : motion_lerp(t, xs0[k], xs1[k]);
    ys[k] = pad ? ys0[k] : motion_lerp(t, ys0[k], ys1[k]);
    zs[k] = pad ? zs0[k] : motion_lerp(t, zs0[k], zs1[k]);
  }
  return DMT_OK;
}

int dmt_motion_bvh_validate(const float* xs0, const float* ys0, const float* zs0, const float* xs1, const float* ys1, const float* zs1,
                            size_t count, int* node_count, int* pair_count, int* depth) {
  if ((count && (!xs0 || !ys0 || !zs0 || !xs1 || !ys1 || !zs1)) || count > 0x0FFFFFFFu) return DMT_ERR_INVALID;
  bvh_build::Result const r = bvh_build::build(xs0, ys0, zs0, uint32_t(count), xs1, ys1, zs1);
  if (node_count) *node_count = int(r.nodes.size());
  if (pair_count) *pair_count = int(r.pairTris.size() / 2);
  if (depth) *depth = r.depth;
  // every decoded child box holds the vertices below it at key 0 and at key 1 (and every other invariant of a tree, twice)
  bool const ok0 = bvh_build::check(r.nodes.data(), r.nodes.size(), r.pairTris.data(), r.pairTris.size() / 2, xs0, ys0, zs0, count, nullptr, nullptr, nullptr);
  bool const ok1 = bvh_build::check(r.nodes.data(), r.nodes.size(), r.pairTris.data(), r.pairTris.size() / 2, xs1, ys1, zs1, count, nullptr, nullptr, nullptr);
  return ok0 && ok1 && r.depth <= kBvhMaxDepth ? DMT_OK : DMT_ERR_STATE;
}

// ---- the brute-force pass's cluster plan, host-only (cull_plan.hpp) ------------------------------
int dmt_brute_cull_plan(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int enable,
                        uint32_t* cluster_count, uint32_t* cluster_first_count, float* cluster_sphere) {
  if (!soupArgsOk(xs, ys, zs, mat_id, count) || !cluster_count) return DMT_ERR_INVALID;
  std::vector<float> radii;
  std::vector<CullCluster> const cl = planBruteCull(CullSoup{xs, ys, zs, mat_id, uint32_t(count)}, enable != 0, &radii);
  *cluster_count = uint32_t(cl.size());
  for (size_t k = 0; k < cl.size(); ++k) {
    if (cluster_first_count) cluster_first_count[2 * k] = cl[k].first, cluster_first_count[2 * k + 1] = cl[k].count;
    if (cluster_sphere) cluster_sphere[4 * k] = cl[k].b[0], cluster_sphere[4 * k + 1] = cl[k].b[1], cluster_sphere[4 * k + 2] = cl[k].b[2],
                        cluster_sphere[4 * k + 3] = radii[k];
  }
  return DMT_OK;
}

// cluster_box: the planner's inflated boxes (lo xyz, hi xyz); cluster_record: what the device reads (centre xyz, half-width xyz)
static int cullBoxPlan(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int enable,
                       uint32_t* cluster_count, uint32_t* cluster_first_count, float* cluster_box, float* cluster_record) {
  if (!soupArgsOk(xs, ys, zs, mat_id, count) || !cluster_count) return DMT_ERR_INVALID;
  std::vector<CullCluster> cl;
  std::vector<float> planBox;
  if (enable && count < kCullMaxIndex) {
    CullSoup const soup{xs, ys, zs, mat_id, uint32_t(count)};
    cl = planBruteCullBox(soup, planBruteCull(soup, true, nullptr), &planBox);
  }
  *cluster_count = uint32_t(cl.size());
  for (size_t k = 0; k < cl.size(); ++k) {
    if (cluster_first_count) cluster_first_count[2 * k] = cl[k].first, cluster_first_count[2 * k + 1] = cl[k].count;
    for (int a = 0; a < 6; ++a) {
      if (cluster_box) cluster_box[6 * k + size_t(a)] = planBox[6 * k + size_t(a)];
      if (cluster_record) cluster_record[6 * k + size_t(a)] = cl[k].b[a];
    }
  }
  return DMT_OK;
}

int dmt_brute_cull_box_plan(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int enable,
                            uint32_t* cluster_count, uint32_t* cluster_first_count, float* cluster_box) {
  return cullBoxPlan(xs, ys, zs, mat_id, count, enable, cluster_count, cluster_first_count, cluster_box, nullptr);
}

int dmt_brute_cull_box_records(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int enable,
                               uint32_t* cluster_count, float* cluster_box, float* cluster_record) {
  return cullBoxPlan(xs, ys, zs, mat_id, count, enable, cluster_count, nullptr, cluster_box, cluster_record);
}

int dmt_cull_records(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int level,
                     uint32_t* cluster_count, uint32_t* record_bytes, uint32_t* record_align, void* records) {
  if (!soupArgsOk(xs, ys, zs, mat_id, count) || !cluster_count) return DMT_ERR_INVALID;
  std::vector<CullCluster> const cl = planCullClusters(level, CullSoup{xs, ys, zs, mat_id, uint32_t(count)});
  *cluster_count = uint32_t(cl.size());
  if (record_bytes) *record_bytes = uint32_t(sizeof(CullCluster));
  if (record_align) *record_align = uint32_t(alignof(CullCluster));
  if (records && !cl.empty()) memcpy(records, cl.data(), cl.size() * sizeof(CullCluster));
  return DMT_OK;
}

// The device's box bound test on the host, ray by ray: cull_ray, cull_box_axis and cull_box_accept as brute_clusters calls
// them, with a division where the device has v_rcp_f32 (within 1 ulp of it) and denormals kept.
int dmt_cull_box_test(const float* record6, const float* origins, const float* dirs, const float* tmax, size_t count, uint8_t* accept) {
  if (!record6 || (count && (!origins || !dirs || !tmax || !accept))) return DMT_ERR_INVALID;
  for (size_t i = 0; i < count; ++i) {
    float const* const o = origins + 3 * i;
    float const* const d = dirs + 3 * i;
    CullRay<float> const cr = cull_ray(o[0], o[1], o[2], 1.0f / cull_dir(d[0]), 1.0f / cull_dir(d[1]), 1.0f / cull_dir(d[2]));
    float nx, ny, nz, fx, fy, fz;
    cull_box_axis(record6[0], record6[3], cr.ax, cr.rx, cr.bx, nx, fx);
    cull_box_axis(record6[1], record6[4], cr.ay, cr.ry, cr.by, ny, fy);
    cull_box_axis(record6[2], record6[5], cr.az, cr.rz, cr.bz, nz, fz);
    accept[i] = cull_box_accept(nx, ny, nz, fx, fy, fz, tmax[i] * kCullTSlack, cr.e2) ? 1 : 0;
  }
  return DMT_OK;
}

}  // extern "C"
