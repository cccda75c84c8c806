// light_state.hpp -- what a context keeps for the light layer: the light list, the light tree over it (light_tree.hpp,
// light_tree_ref.hpp) and the env map (envmap.hpp; 4.5).  The layer's device code is in pt_device.hpp,
// envmap.hpp and the two tree headers, its helpers and entry points in light_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, Rec32, EnvView, RenderParams, the
// node types of the trees and the kFeatEnv / kFeatLightTree / kFeatLightTreeRef / kFeatEmitterTree bits.
//
// Four records.  A new context holds the default values below.
//
//   record   setter                   cleared by                       survives
//   list     dmt_upload_lights        the next dmt_upload_lights       every other upload (dmt_upload_triangles, _bsdfs,
//            (a zero-count list or    (there is no clear call)         _textures, _area_lights, _envmap, dmt_update_vertices*),
//            one of infinite lights                                    dmt_set_camera, dmt_set_lens, dmt_set_accel,
//            only counts as uploaded)                                  dmt_set_light_sampling, a refused call
//   tree     mode:                    mode: the next                   the same, and dmt_upload_lights as far as the mode
//            dmt_set_light_sampling   dmt_set_light_sampling           goes; nodes, depth, valid and tooDeep are derived
//                                                                      (below) and go with an invalidation
//   env      dmt_upload_envmap        dmt_clear_envmap, the next       the same, and dmt_upload_lights and
//                                     dmt_upload_envmap                dmt_set_light_sampling
//
//   emitters mode:                    mode: the next                   the same as the tree's mode.  nodes, trails, counts,
//            dmt_set_emitter_sampling dmt_set_emitter_sampling         depth, valid and tooDeep are derived (below) and go
//                                                                      with an invalidation
//
//   uniformPath  DMT_UNIFORM_LIGHTS at    --                              everything: set once, when the context is created
//            context creation (0 clears it)
//
// Derived lazily: the tree's nodes, by the first launch or dmt_test_light_tree that wants them (resolveFeatures ->
// ensureLightTree), from the host copy of the list, for the mode the context has then.  Two things invalidate the tree
// (invalidateTree): dmt_upload_lights, and a dmt_set_light_sampling that CHANGES the mode -- through DMT_LIGHTS_UNIFORM too,
// so 1 -> 0 -> 1 builds again.  Nothing else does: the same mode set again keeps the tree, and emissive triangles, image
// textures and blend materials switch the tree rows off (features) without invalidating it.  It is used again, not rebuilt,
// when they go.  An invalidation frees nothing: both node buffers may hold an earlier tree, and only the one of the current
// mode, and only while valid, reaches a launch (fill).
//
// The emitter tree (emitter_tree.hpp) is derived lazily in the same place (resolveFeatures ->
// ensureEmitterTree), from the host copy of the list, the host copy of the emissive-triangle list (SurfaceState::Emissive) and
// the host mirrors of the soup's positions, which the vertex updates keep current.  invalidateEmitters is called by
// dmt_upload_lights, dmt_upload_area_lights, a new soup (dmt_upload_triangles), dmt_update_vertices and
// dmt_update_vertices_device, and a dmt_set_emitter_sampling that CHANGES the mode.  dmt_set_motion and dmt_clear_motion do
// not apply: they leave key 0 and its mirrors alone, and a launch with motion and emissive triangles is refused.  It
// survives everything else, dmt_set_light_sampling included.  Commit-last, the too-deep fall-back and draining are the
// tree's (below): its two DevBufs are assigned like the tree's, and every call that invalidates it with new positions or a
// new list has drained the stream or waited in hipFree before the next build.
//
// Feature bits (features), one list of conditions:
//   kFeatEnv            an env map is present (env.view.w > 0); nothing else matters to it
//   kFeatLightTree      all of: a list was uploaded; the mode is DMT_LIGHTS_TREE; the list has more than one record (infinite
//                       records do not count); the last build was not too deep; every record is a point or spot light
//                       (list.treeable: a directional record has no position); and the surfaces are plain -- no emissive
//                       triangles, no image textures, no blend materials, which featuresOf knows and passes in
//   kFeatLightTreeRef   the same with DMT_LIGHTS_TREE_REFERENCE
//   kFeatEmitterTree    all of: the emitter mode is DMT_EMITTERS_TREE; emissive triangles are present; every list record is a
//                       point or spot light, or the list is empty (a directional record keeps the uniform pick, as
//                       `treeable` does); the last build was not too deep.  whyEmitters() names the first that fails
// So a context with mode 1 set still runs the uniform rows when: no list was uploaded or it has fewer than two records, a
// record is directional, the tree came out too deep, or emissive triangles, image textures or blend materials are present.
// why() names the first of these that holds, in that order; dmt_test_light_tree refuses with it.
//
// The too-deep fall-back.  A tree deeper than its walk's guard (kLightTreeMaxDepth, kLightTreeRefMaxDepth) would cut paths
// short.  ensureLightTree sets tooDeep instead of uploading it and leaves a note in dmt_last_error; the call that found out
// goes on and runs the uniform rows, and so does every launch after it, without a note of its own.  Only an invalidation
// clears tooDeep: the next launch that wants a tree builds again and finds out again.
//
// Draining.  A launch in flight holds the env map's view and the pointers of the list and the tree by value in its kernel
// arguments and reads the arrays behind them.
//   dmt_upload_envmap        drains the stream once its arguments have passed: a refused upload does not touch the stream
//   dmt_clear_envmap         always drains it
//   dmt_upload_lights,       call no synchronise of their own.  dmt_upload_lights fills two new arrays and then moves them
//   the lazy tree upload     over the old ones, whose DevBuf frees them with hipFree, and hipFree waits for the whole device.
//                            The tree's DevBuf::assign copies in place when the old array has room.  That overwrites nodes a
//                            launch in flight may read only after a mode change (an upload has waited in hipFree, and no
//                            launch between it and the build reads a tree), and then with the bytes the array already
//                            holds: the builders are deterministic and the list is the same.  Both rest on the runtime and
//                            on that argument, not on a rule of devbuf.hpp.
//   dmt_set_light_sampling   touches no device memory
//
// Commit-last.  A call that fails -- an allocation, a copy, a refused argument -- leaves every record as it was:
// dmt_upload_lights and dmt_upload_envmap fill new arrays and commit them with the counts at the end; ensureLightTree sets
// valid after the copy, and the array of a failed copy reaches no launch because valid stays false.
#pragma once

namespace {

struct LightState {
  // what the kernels read as SceneView::lights / infLights
  struct List {
    bool have = false;              // dmt_upload_lights has run
    DevBuf<Rec32> recs, inf;        // point / spot / directional records; infinite records
    uint32_t count = 0, infCount = 0;
    std::vector<uint8_t> host;      // host copy of recs, packed: what the tree is built from
    bool treeable = false;          // count > 0 and every record is a point or spot light
  } list;
  // what the *_ltree / *_ltree2 rows read as RenderParams::lightTree / lightTreeRef
  struct Tree {
    int mode = DMT_LIGHTS_UNIFORM;
    DevBuf<LightTreeNode> nodes;        // DMT_LIGHTS_TREE
    DevBuf<LightTreeRefNode> refNodes;  // DMT_LIGHTS_TREE_REFERENCE
    int depth = 0;                      // of the last build
    bool valid = false;                 // the buffer of `mode` holds the tree of `list`
    bool tooDeep = false;               // the last build exceeded its walk's guard: the uniform pick is used instead
  } tree;
  // what the *_etree rows read as RenderParams::emitterTree / emitterTrails
  struct Emitters {
    int mode = DMT_EMITTERS_UNIFORM;
    DevBuf<EmitterNode> nodes;
    DevBuf<EmitterTrail> trails;        // [emitter]
    uint32_t emitters = 0, nodeCount = 0;  // of the last build
    int depth = 0;
    double buildMs = 0.0;               // host time of the last build
    bool valid = false;                 // the buffers hold the tree of the list, the emissive triangles and the positions
    bool tooDeep = false;               // the last build exceeded kEmitterTreeMaxDepth: the uniform pick is used instead
  } emitters;
  // what the *_env rows read as RenderParams::env
  struct Env {
    DevBuf<float> buf;  // A18: one allocation holding the five tables and the image
    EnvView view{};     // w == 0: no env map
  } env;

  // one-record lists through the scalar path (RenderParams::uniformLights).  DMT_UNIFORM_LIGHTS=0 at context creation clears
  // it: every pick then loads the lane's record, as lists of other sizes always do (A/B runs, tests)
  bool uniformPath = true;

  // which light pick a launch runs, and if the uniform one although a tree is asked for, the first reason why
  enum class Pick { Tree, NoList, UniformMode, OneLight, TooDeep, NotTreeable };
  Pick why(bool plainSurfaces) const {
    return !list.have ? Pick::NoList : tree.mode == DMT_LIGHTS_UNIFORM ? Pick::UniformMode : list.count <= 1 ? Pick::OneLight
           : tree.tooDeep ? Pick::TooDeep : !(list.treeable && plainSurfaces) ? Pick::NotTreeable : Pick::Tree;
  }

  // the emitter tree's turn: which pick the *_area rows' scenes run
  enum class EmitterPick { Tree, UniformMode, NoTriangles, NotTreeable, TooDeep };
  EmitterPick whyEmitters(uint32_t areaCount) const {
    return emitters.mode != DMT_EMITTERS_TREE ? EmitterPick::UniformMode : areaCount == 0 ? EmitterPick::NoTriangles
           : !(list.count == 0 || list.treeable) ? EmitterPick::NotTreeable : emitters.tooDeep ? EmitterPick::TooDeep : EmitterPick::Tree;
  }
  uint32_t emitterFeatures(uint32_t areaCount) const { return whyEmitters(areaCount) == EmitterPick::Tree ? kFeatEmitterTree : 0u; }
  void fillEmitters(RenderParams& P, uint32_t areaCount) const {
    if (emitters.valid && emitterFeatures(areaCount)) P.emitterTree = emitters.nodes.get(), P.emitterTrails = emitters.trails.get();
  }
  void invalidateEmitters() { emitters.valid = false, emitters.tooDeep = false; }

  // the layer's part of the feature mask (featuresOf).  A tree not built yet counts as applying: resolveFeatures builds it
  uint32_t features(bool plainSurfaces) const {
    uint32_t const treeBit = tree.mode == DMT_LIGHTS_TREE ? kFeatLightTree : kFeatLightTreeRef;
    return (env.view.w > 0 ? kFeatEnv : 0u) | (why(plainSurfaces) == Pick::Tree ? treeBit : 0u);
  }

  // the layer's part of the argument struct (baseParams): the tree's pointer only under its feature bit and while valid
  void fill(RenderParams& P, bool plainSurfaces) const {
    P.scene.lights = list.recs.get(), P.scene.infLights = list.inf.get(), P.scene.lightCount = list.count, P.scene.infLightCount = list.infCount;
    P.env = env.view;
    P.uniformLights = uniformPath ? 1u : 0u;
    uint32_t const F = tree.valid ? features(plainSurfaces) : 0u;
    if (F & kFeatLightTree) P.lightTree = tree.nodes.get();
    if (F & kFeatLightTreeRef) P.lightTreeRef = tree.refNodes.get();
  }

  // dmt_upload_lights, and a dmt_set_light_sampling that changes the mode: the next launch that wants a tree builds one
  void invalidateTree() { tree.valid = false, tree.tooDeep = false; }
};

}  // namespace
