// light_host.hpp -- the host side of the light layer: the one builder over the two kinds of light tree, the lazy build of a
// context's tree, and the dmt_* entry points of the light list, the sampling mode, the host-only tree calls and the env map.
// The layer's state and its rules -- what each call keeps and invalidates, when a feature bit is set, the too-deep
// fall-back, which calls drain the stream -- are in light_state.hpp; the trees themselves in light_tree.hpp and
// light_tree_ref.hpp, the env map's tables and device code in envmap.hpp.
//
// Part of dmt_hip.hip's translation unit, included once after the host helpers it uses (dmt_ctx with SceneState's host copy
// of the soup, HIP_TRY, fail) and before
// launch_host.hpp and probes.hpp: resolveFeatures (dmt_hip.hip) calls ensureLightTree ahead of every launch and of
// dmt_test_light_tree.
#pragma once

namespace {

float h2f_host(uint16_t h) {  // exact fp16 -> fp32 (CC/private/encoding.cu:124-155)
  uint32_t const sgn = uint32_t(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu, out;
  if (e == 0) {
    if (m == 0) {
      out = sgn;
    } else {
      e = 113;
      while (!(m & 0x400u)) m <<= 1, --e;
      out = sgn | (e << 23) | ((m & 0x3FFu) << 13);
    }
  } else if (e == 31) {
    out = sgn | 0x7F800000u | (m << 13);
  } else {
    out = sgn | ((e + 112) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &out, 4);
  return f;
}
// octahedral decode on the host (CC/private/encoding.cu:39-60), as pt_device.hpp's dir_from_octa
void octa_host(uint32_t octa, float out[3]) {
  float const mx = 65535.f;
  float const fx = float(octa & 0xFFFFu) / mx * 2.f - 1.f, fy = float((octa >> 16) & 0xFFFFu) / mx * 2.f - 1.f;
  float n[3] = {fx, fy, 1.f - fabsf(fx) - fabsf(fy)};
  if (n[2] < 0.f) {
    n[0] = (1.f - fabsf(fy)) * (std::signbit(fx) ? -1.f : 1.f);
    n[1] = (1.f - fabsf(fx)) * (std::signbit(fy) ? -1.f : 1.f);
  }
  float const inv = 1.f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  out[0] = n[0] * inv, out[1] = n[1] * inv, out[2] = n[2] * inv;
}

// ---- the two kinds of light tree ---------------------------------------------------
// A kind: its node and item types, the item of a packed record, its builder, its walk's depth guard, its buffer in the state.
struct LightTreeKind {  // DMT_LIGHTS_TREE (light_tree.hpp)
  using Node = LightTreeNode;
  using Item = light_tree::Item;
  static constexpr int maxDepth = kLightTreeMaxDepth;
  static bool itemOf(uint8_t const* rec32, uint32_t i, Item& it) { return light_tree::itemOf(rec32, i, h2f_host, it); }
  static std::vector<Node> build(std::vector<Item> const& items, int* depth) { return light_tree::build(items, depth); }
  static DevBuf<Node>& buffer(LightState::Tree& t) { return t.nodes; }
};
struct LightTreeRefKind {  // DMT_LIGHTS_TREE_REFERENCE (light_tree_ref.hpp)
  using Node = LightTreeRefNode;
  using Item = light_tree_ref::Item;
  static constexpr int maxDepth = kLightTreeRefMaxDepth;
  static bool itemOf(uint8_t const* rec32, uint32_t i, Item& it) { return light_tree_ref::itemOf(rec32, i, h2f_host, octa_host, it); }
  static std::vector<Node> build(std::vector<Item> const& items, int* depth) { return light_tree_ref::build(items, depth); }
  static DevBuf<Node>& buffer(LightState::Tree& t) { return t.refNodes; }
};

// The tree of kind K over a packed light list: what a context uploads and what the host-only calls return.  False, and
// nothing written, when a record is neither a point nor a spot light.  depth (may be null) = levels.
template <class K>
bool buildLightTree(void const* lights32, uint32_t count, std::vector<typename K::Node>& nodes, int* depth) {
  std::vector<typename K::Item> items(count);
  for (uint32_t i = 0; i < count; ++i)
    if (!K::itemOf(static_cast<uint8_t const*>(lights32) + 32 * size_t(i), i, items[i])) return false;
  nodes = K::build(items, depth);
  return true;
}

// a tree deeper than the walks' guard (lights at geometrically growing spacing) would cut paths short: the context keeps the
// uniform pick and says so through dmt_last_error; the call that found out goes on
int keepUniformPick(dmt_ctx* ctx, int guard) {
  ctx->lights.tree.tooDeep = true;
  ctx->err = "light tree: its depth of " + std::to_string(ctx->lights.tree.depth) + " exceeds the walk's guard of " + std::to_string(guard) +
             " levels; the uniform pick is used instead";
  return DMT_OK;
}
// (re)build the tree of kind K from the host copy of the light records and upload it
template <class K>
int uploadLightTree(dmt_ctx* ctx) {
  LightState& L = ctx->lights;
  std::vector<typename K::Node> nodes;
  if (!buildLightTree<K>(L.list.host.data(), L.list.count, nodes, &L.tree.depth))
    return fail(ctx, DMT_ERR_STATE, "light tree: only point and spot lights can be in the light list");
  if (L.tree.depth > K::maxDepth) return keepUniformPick(ctx, K::maxDepth);
  HIP_TRY(ctx, K::buffer(L.tree).assign(nodes.data(), nodes.size()));
  L.tree.valid = true;
  return DMT_OK;
}
int ensureLightTree(dmt_ctx* ctx) {
  if (ctx->lights.tree.valid) return DMT_OK;
  return ctx->lights.tree.mode == DMT_LIGHTS_TREE_REFERENCE ? uploadLightTree<LightTreeRefKind>(ctx) : uploadLightTree<LightTreeKind>(ctx);
}

// dmt_light_tree_nodes for one kind
template <class K>
int lightTreeNodes(void const* lights32, uint32_t count, void* nodes_out, uint32_t cap, int* node_count, int* depth) {
  std::vector<typename K::Node> nodes;
  if (!buildLightTree<K>(lights32, count, nodes, depth)) return DMT_ERR_INVALID;
  if (node_count) *node_count = int(nodes.size());
  if (nodes.size() > cap) return DMT_ERR_INVALID;  // the counts are reported: ask again with room for them
  if (!nodes.empty()) memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(typename K::Node));
  return DMT_OK;
}

// ---- the emitter tree (emitter_tree.hpp) -------------------------------------------
// The one builder call: what a context uploads and what the host-only calls return.  Emitters are the packed lights and
// then the triangles area_tri of the soup xs / ys / zs (4 floats per triangle and axis).  False, and nothing written, when a
// record is neither a point nor a spot light or a triangle index lies outside the soup.
bool buildEmitterTree(void const* lights32, uint32_t count, float const* xs, float const* ys, float const* zs, uint64_t triCount,
                      uint32_t const* areaTri, float const* areaLe, uint32_t areaCount, emitter_tree::Tree& tree) {
  std::vector<emitter_tree::Item> items(size_t(count) + areaCount);
  for (uint32_t i = 0; i < count; ++i)
    if (!emitter_tree::lightItem(static_cast<uint8_t const*>(lights32) + 32 * size_t(i), i, h2f_host, items[i])) return false;
  for (uint32_t k = 0; k < areaCount; ++k) {
    size_t const t = areaTri[k];
    if (t >= triCount) return false;
    float const p0[3] = {xs[4 * t], ys[4 * t], zs[4 * t]}, p1[3] = {xs[4 * t + 1], ys[4 * t + 1], zs[4 * t + 1]};
    float const p2[3] = {xs[4 * t + 2], ys[4 * t + 2], zs[4 * t + 2]};
    emitter_tree::triangleItem(p0, p1, p2, areaLe + 3 * size_t(k), count + k, items[size_t(count) + k]);
  }
  tree = emitter_tree::build(std::move(items));
  return true;
}
// (re)build the emitter tree from the host copies of the light records, the emissive list and the soup, and upload it.  Too
// deep: the same kind of note as keepUniformPick's, and the call that found out goes on with the uniform rows
int ensureEmitterTree(dmt_ctx* ctx) {
  LightState::Emitters& E = ctx->lights.emitters;
  if (E.valid || E.tooDeep) return DMT_OK;
  SurfaceState::Emissive const& area = ctx->surf.area;
  emitter_tree::Tree tree;
  auto const t0 = std::chrono::steady_clock::now();
  if (!buildEmitterTree(ctx->lights.list.host.data(), ctx->lights.list.count, ctx->scene.h_xs.data(), ctx->scene.h_ys.data(), ctx->scene.h_zs.data(), ctx->scene.triCount,
                        area.hostTri.data(), area.hostLe.data(), area.count, tree))
    return fail(ctx, DMT_ERR_STATE, "emitter tree: only point and spot lights can be in the light list");
  E.buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  E.depth = tree.depth, E.emitters = uint32_t(tree.trails.size()), E.nodeCount = uint32_t(tree.nodes.size());
  if (tree.depth > kEmitterTreeMaxDepth) {
    E.tooDeep = true;
    ctx->err = "emitter tree: its depth of " + std::to_string(tree.depth) + " exceeds the walk's guard of " + std::to_string(kEmitterTreeMaxDepth) +
               " levels; the uniform pick is used instead";
    return DMT_OK;
  }
  HIP_TRY(ctx, E.nodes.assign(tree.nodes.data(), tree.nodes.size()));
  HIP_TRY(ctx, E.trails.assign(tree.trails.data(), tree.trails.size()));
  E.valid = true;
  return DMT_OK;
}
// the arguments the three host-only emitter-tree calls share
bool emitterSceneOk(void const* lights32, uint32_t count, float const* xs, float const* ys, float const* zs, uint64_t triCount,
                    uint32_t const* areaTri, float const* areaLe, uint32_t areaCount) {
  return !(count && !lights32) && !(triCount && (!xs || !ys || !zs)) && !(areaCount && (!areaTri || !areaLe));
}

// ---- the env map (envmap.hpp) -------------------------------------------------------
// what the tables take: powers of two, at least 8 (one AVX2 block of the reference's CDF)
bool envResolutionOk(int width, int height) { return width >= 8 && height >= 8 && !(width & (width - 1)) && !(height & (height - 1)); }

}  // namespace

extern "C" {

int dmt_upload_lights(dmt_ctx* ctx, const void* lights32, uint32_t count, const void* infinite32, uint32_t infinite_count) {
  if (!ctx) return DMT_ERR_INVALID;
  if ((count && !lights32) || (infinite_count && !infinite32))
    return fail(ctx, DMT_ERR_INVALID, "dmt_upload_lights: null array");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<Rec32> lights, inf;
  HIP_TRY(ctx, lights.assign(lights32, count));
  HIP_TRY(ctx, inf.assign(infinite32, infinite_count));
  LightState::List& l = ctx->lights.list;
  l.recs = std::move(lights), l.inf = std::move(inf);
  l.count = count, l.infCount = infinite_count, l.have = true;
  l.host.assign(static_cast<uint8_t const*>(lights32), static_cast<uint8_t const*>(lights32) + size_t(count) * 32);
  ctx->lights.invalidateTree(), ctx->lights.invalidateEmitters();
  l.treeable = count > 0;
  for (uint32_t i = 0; i < count; ++i) {  // a directional light in the list (PBRT "distant") has no position: such lists keep the uniform pick
    uint16_t type;
    memcpy(&type, l.host.data() + 32 * size_t(i) + 6, 2);
    if (type != 0 && type != 1) l.treeable = false;
  }
  return DMT_OK;
}

int dmt_set_light_sampling(dmt_ctx* ctx, int mode) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_LIGHTS_UNIFORM && mode != DMT_LIGHTS_TREE && mode != DMT_LIGHTS_TREE_REFERENCE)
    return fail(ctx, DMT_ERR_INVALID, "dmt_set_light_sampling: unknown mode");
  if (mode != ctx->lights.tree.mode) ctx->lights.invalidateTree();  // the two trees are different structures
  ctx->lights.tree.mode = mode;
  return DMT_OK;
}

int dmt_uniform_lights_info(dmt_ctx* ctx, int* enabled) {
  if (!ctx || !enabled) return DMT_ERR_INVALID;
  RenderParams P{};
  ctx->lights.fill(P, true);  // what a launch passes: the switch as it reaches the kernels
  *enabled = P.uniformLights != 0u;
  return DMT_OK;
}

int dmt_set_emitter_sampling(dmt_ctx* ctx, int mode) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_EMITTERS_UNIFORM && mode != DMT_EMITTERS_TREE) return fail(ctx, DMT_ERR_INVALID, "dmt_set_emitter_sampling: unknown mode");
  if (mode != ctx->lights.emitters.mode) ctx->lights.invalidateEmitters();
  ctx->lights.emitters.mode = mode;
  return DMT_OK;
}

int dmt_emitter_tree_info(dmt_ctx* ctx, int* mode, int* active, uint32_t* emitters, uint32_t* nodes, int* depth, double* build_ms) {
  if (!ctx) return DMT_ERR_INVALID;
  LightState& L = ctx->lights;
  uint32_t const areaCount = ctx->surf.area.count;
  if (L.emitterFeatures(areaCount)) {  // as a launch would: build it, which may find it too deep
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int const rc = ensureEmitterTree(ctx)) return rc;
  }
  bool const on = L.emitterFeatures(areaCount) != 0u && L.emitters.valid;
  bool const built = on || L.whyEmitters(areaCount) == LightState::EmitterPick::TooDeep;  // a too-deep build still reports what it found
  if (mode) *mode = L.emitters.mode;
  if (active) *active = on ? 1 : 0;
  if (emitters) *emitters = built ? L.emitters.emitters : 0u;
  if (nodes) *nodes = built ? L.emitters.nodeCount : 0u;
  if (depth) *depth = built ? L.emitters.depth : 0;
  if (build_ms) *build_ms = built ? L.emitters.buildMs : 0.0;
  return DMT_OK;
}

// host only: the emitter tree ensureEmitterTree uploads for this scene
int dmt_emitter_tree_nodes(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                           const uint32_t* area_tri, const float* area_le, uint32_t area_count, void* nodes_out, uint32_t cap,
                           uint64_t* trails_out, int32_t* lengths_out, int* node_count, int* depth) {
  if (!emitterSceneOk(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count)) return DMT_ERR_INVALID;
  emitter_tree::Tree T;
  if (!buildEmitterTree(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count, T)) return DMT_ERR_INVALID;
  if (node_count) *node_count = int(T.nodes.size());
  if (depth) *depth = T.depth;
  if (nodes_out) {
    if (T.nodes.size() > cap) return DMT_ERR_INVALID;  // the counts are reported: ask again with room for them
    if (!T.nodes.empty()) memcpy(nodes_out, T.nodes.data(), T.nodes.size() * sizeof(EmitterNode));
  }
  for (size_t i = 0; i < T.trails.size(); ++i) {
    if (trails_out) trails_out[i] = uint64_t(T.trails[i].lo) | (uint64_t(T.trails[i].hi) << 32);
    if (lengths_out) lengths_out[i] = int32_t(T.trails[i].length);
  }
  return DMT_OK;
}

// host only: et_select and et_pmf, the functions the *_etree kernels call, at n cases
int dmt_emitter_tree_select(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                            const uint32_t* area_tri, const float* area_le, uint32_t area_count, int n, const float* p3, const float* n3,
                            const float* u, float start_pmf, int32_t* index_out, float* pmf_out, float* pmf_by_trail_out) {
  if (!emitterSceneOk(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count) || n < 0 ||
      (n && (!p3 || !n3 || !u || !index_out || !pmf_out || !pmf_by_trail_out)))
    return DMT_ERR_INVALID;
  emitter_tree::Tree T;
  if (!buildEmitterTree(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count, T) || T.nodes.empty()) return DMT_ERR_INVALID;
  if (T.depth > kEmitterTreeMaxDepth) return DMT_ERR_STATE;  // its trails do not fit: a context keeps the uniform pick
  for (int i = 0; i < n; ++i) {
    float pmf = 0.f;
    int const e = et_select(T.nodes.data(), p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], n3[3 * i], n3[3 * i + 1], n3[3 * i + 2], u[i], pmf);
    index_out[i] = e, pmf_out[i] = e >= 0 ? start_pmf * pmf : 0.f;
    pmf_by_trail_out[i] = e >= 0 ? start_pmf * et_pmf(T.nodes.data(), T.trails[size_t(e)], p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], n3[3 * i],
                                                      n3[3 * i + 1], n3[3 * i + 2])
                                 : 0.f;
  }
  return DMT_OK;
}

// host only: et_pmf of every emitter at (p, n)
int dmt_emitter_tree_pmfs(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                          const uint32_t* area_tri, const float* area_le, uint32_t area_count, const float* p3, const float* n3,
                          float* pmf_out) {
  if (!emitterSceneOk(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count) || !p3 || !n3 || !pmf_out) return DMT_ERR_INVALID;
  emitter_tree::Tree T;
  if (!buildEmitterTree(lights32, count, xs, ys, zs, tri_count, area_tri, area_le, area_count, T)) return DMT_ERR_INVALID;
  if (T.depth > kEmitterTreeMaxDepth) return DMT_ERR_STATE;
  emitter_tree::pmfs(T, p3, n3, pmf_out);
  return DMT_OK;
}

// host only: the probability with which the light tree built from `lights32` picks each light at (p, n)
int dmt_light_tree_pmfs(const void* lights32, uint32_t count, const float* p3, const float* n3, float* pmf_out, int* node_count,
                        int* depth) {
  if ((count && !lights32) || !p3 || !n3 || !pmf_out) return DMT_ERR_INVALID;
  std::vector<LightTreeNode> nodes;
  if (!buildLightTree<LightTreeKind>(lights32, count, nodes, depth)) return DMT_ERR_INVALID;
  light_tree::pmfs(nodes, p3, n3, pmf_out, count);
  if (node_count) *node_count = int(nodes.size());
  return DMT_OK;
}

// host only: cut + selection of the reference-semantics tree at n shading points (light_tree_ref.hpp's ltr_select, the
// function the *_ltree2 kernels call)
int dmt_light_tree_ref_select(const void* lights32, uint32_t count, int n, const float* p3, const float* n3, const float* u, float start_pmf,
                              int32_t* indices4, float* pmfs4, int32_t* counts, int* node_count, int* depth) {
  if ((count && !lights32) || n < 0 || (n && (!p3 || !n3 || !u || !indices4 || !pmfs4 || !counts))) return DMT_ERR_INVALID;
  std::vector<LightTreeRefNode> nodes;
  int d = 0;
  if (!buildLightTree<LightTreeRefKind>(lights32, count, nodes, &d) || nodes.empty()) return DMT_ERR_INVALID;
  if (node_count) *node_count = int(nodes.size());
  if (depth) *depth = d;
  for (int i = 0; i < n; ++i) {
    LightTreeRefSelection const sel = ltr_select(nodes.data(), p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], n3[3 * i], n3[3 * i + 1], n3[3 * i + 2], u[i], start_pmf);
    counts[i] = int32_t(sel.count);
    for (int k = 0; k < kLightTreeMaxSplitSize; ++k)
      indices4[4 * i + k] = k < int(sel.count) ? int32_t(sel.indices[k]) : -1, pmfs4[4 * i + k] = k < int(sel.count) ? sel.pmfs[k] : 0.f;
  }
  return DMT_OK;
}

// host only: the node array ensureLightTree uploads for `mode`: both go through buildLightTree<K>
int dmt_light_tree_nodes(const void* lights32, uint32_t count, int mode, void* nodes_out, uint32_t cap, int* node_count, int* depth) {
  if ((count && !lights32) || (cap && !nodes_out) || (mode != DMT_LIGHTS_TREE && mode != DMT_LIGHTS_TREE_REFERENCE)) return DMT_ERR_INVALID;
  return mode == DMT_LIGHTS_TREE ? lightTreeNodes<LightTreeKind>(lights32, count, nodes_out, cap, node_count, depth)
                                 : lightTreeNodes<LightTreeRefKind>(lights32, count, nodes_out, cap, node_count, depth);
}

// host only: any power-of-two pair >= 8
int dmt_envmap_tables(const float* rgb, int width, int height, float* func, float* cdf, float* row_integral,
                      float* marginal_func, float* marginal_cdf, float* marginal_integral) {
  if (!rgb || !envResolutionOk(width, height) || !func || !cdf || !row_integral || !marginal_func || !marginal_cdf || !marginal_integral)
    return DMT_ERR_INVALID;
  envmap::Tables const t = envmap::build(rgb, width, height);
  memcpy(func, t.func.data(), t.func.size() * 4), memcpy(cdf, t.cdf.data(), t.cdf.size() * 4);
  memcpy(row_integral, t.rowInt.data(), t.rowInt.size() * 4);
  memcpy(marginal_func, t.mFunc.data(), t.mFunc.size() * 4), memcpy(marginal_cdf, t.mCdf.data(), t.mCdf.size() * 4);
  *marginal_integral = t.mInt;
  return DMT_OK;
}

int dmt_clear_envmap(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->lights.env.buf.reset();
  ctx->lights.env.view = EnvView{};
  return DMT_OK;
}

int dmt_upload_envmap(dmt_ctx* ctx, const float* rgb, int width, int height, const float* quat_xyzw, float scale) {
  if (!ctx || !rgb || !quat_xyzw) return DMT_ERR_INVALID;
  // the reference asserts powers of two and width == 2 * height (core-light.cpp:116)
  if (!envResolutionOk(width, height) || width != 2 * height)
    return fail(ctx, DMT_ERR_INVALID, "dmt_upload_envmap: resolution must be powers of two >= 8 with width == 2 * height");
  float const len = std::sqrt(quat_xyzw[0] * quat_xyzw[0] + quat_xyzw[1] * quat_xyzw[1] + quat_xyzw[2] * quat_xyzw[2] +
                              quat_xyzw[3] * quat_xyzw[3]);
  if (!(len > 0.f)) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_envmap: zero quaternion");
  (void)scale;  // stored by the reference and never applied (core-light.cpp:115, :444-452)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  envmap::Tables const t = envmap::build(rgb, width, height);
  size_t const wh = size_t(width) * size_t(height), h = size_t(height);
  DevBuf<float> buf;
  HIP_TRY(ctx, buf.reserve(2 * wh + 3 * h + 3 * wh));
  float* p = buf.get();
  EnvView e{};
  hipError_t err = hipSuccess;
  auto put = [&](float const* src, size_t n) -> float const* {
    float* dst = p;
    p += n;
    if (err == hipSuccess) err = hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice);
    return dst;
  };
  e.func = put(t.func.data(), wh), e.cdf = put(t.cdf.data(), wh), e.rowInt = put(t.rowInt.data(), h);
  e.mFunc = put(t.mFunc.data(), h), e.mCdf = put(t.mCdf.data(), h), e.rgb = put(rgb, 3 * wh);
  if (err != hipSuccess) return fail(ctx, DMT_ERR_HIP, "dmt_upload_envmap: copy failed");
  e.mInt = t.mInt, e.w = width, e.h = height;
  e.qx = quat_xyzw[0] / len, e.qy = quat_xyzw[1] / len, e.qz = quat_xyzw[2] / len, e.qw = quat_xyzw[3] / len;
  ctx->lights.env.buf = std::move(buf);
  ctx->lights.env.view = e;
  return DMT_OK;
}

}  // extern "C"
