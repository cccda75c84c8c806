// scene_state.hpp -- what a context keeps of the scene itself: the triangle soup with both device records of every triangle
// (tri_records.hpp) and the host copy the builders read, and the BSDF records.  The layer's helpers and entry points are in
// scene_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, TriIsect, TriPost, Rec32 and
// RenderParams.
//
// Two records.  A new context holds the default values below.
//
//   record   setter                  cleared by                      survives
//   soup     dmt_upload_triangles    the next dmt_upload_triangles   every other upload, dmt_set_camera, dmt_set_lens,
//            (a zero-count soup      (there is no clear call)        dmt_set_pixel_filter, dmt_set_accel*, a refused call.
//            counts as uploaded)                                     dmt_update_vertices[_device] overwrite the positions in
//                                                                    place -- tris, post and h_xs / h_ys / h_zs -- and keep
//                                                                    triCount, h_mat and maxMatId; dmt_set_motion reads the
//                                                                    soup as key 0 and leaves it alone
//   bsdfs    dmt_upload_bsdfs        the next dmt_upload_bsdfs       the same, and dmt_upload_triangles and the vertex updates
//
// Derived with the setter: maxMatId (the largest material index of the soup; 0 for an empty one) and hasBlend (some BSDF record
// is a BS_GGX_BLEND pair: the *_blend kernels carry that code, featuresOf and plainSurfaces read it).  The two records may
// arrive in either order, so a soup may name materials the BSDF array does not have: matIdOutside() says so, and every launch
// that would index the array asks it first -- render, probe, first-hit / denoise and dmt_upload_opacity, each with its own
// message.
//
// What a new soup invalidates (dmt_upload_triangles tells each layer, in this order, after its own commit): the static tree
// (AccelState::tree, dropped, rebuilt at the end under DMT_ACCEL_BVH), key 1 and the motion tree (dropMotion), the emitter
// tree (LightState::invalidateEmitters), vertex normals, opacity records and emissive triangles with the material kinds made
// anew (SurfaceState::soupReplaced), the denoiser's vertex mirror (DenoiseState::dropVertexMirror).  The cull tables
// (AccelState::cull) are planned from the new soup and committed with it.  The light list, the env map, the textures, the
// medium, the camera, the lens, the pixel filter and the film are left alone; texture tables that no longer match are refused
// at the launch (SurfaceState::texturesMatch).
// What new BSDFs invalidate: the cutout records, which name materials of the old array, and the material kinds
// (SurfaceState::bsdfsReplaced).  Nothing else.
//
// Draining.  A launch in flight holds the records' pointers by value in its kernel arguments.
//   dmt_upload_triangles  calls no synchronise of its own: it fills new arrays and moves them over the old ones, whose DevBuf
//                         frees them with hipFree, and hipFree waits for the whole device (as LightState's list)
//   dmt_upload_bsdfs      drains the stream once its arguments have passed, before SurfaceState::bsdfsReplaced drops the cutout
//                         records a launch in flight may read; a refused upload does not touch the stream
//
// Commit-last.  A call that fails -- a refused argument, a blend record without its conductor, an allocation, a copy, the
// cull tables' upload -- leaves both records as they were: the new arrays are filled first and committed with the counts at
// the end.  Past the commit, a failure of the material-kind table (kindRc) or of the BVH build is reported with the new
// records in place.
#pragma once

namespace {

struct SceneState {
  // what the kernels read as SceneView::tris / post / bsdfs
  DevBuf<TriIsect> tris;
  DevBuf<TriPost> post;
  DevBuf<Rec32> bsdfs;
  uint32_t triCount = 0, bsdfCount = 0;
  uint32_t maxMatId = 0;
  std::vector<float> h_xs, h_ys, h_zs;  // host copy of the soup (the builders' input); the vertex updates keep it current
  std::vector<uint32_t> h_mat;
  bool hasBlend = false;  // some uploaded BSDF record is a BS_GGX_BLEND pair: the *_blend kernels carry that code
  bool haveTris = false, haveBsdfs = false;  // dmt_upload_triangles / dmt_upload_bsdfs has run

  // some triangle's material index is outside the BSDF array
  bool matIdOutside() const { return triCount > 0 && maxMatId >= bsdfCount; }

  // the layer's part of the argument struct (baseParams)
  void fill(RenderParams& P) const {
    P.scene.tris = tris.get(), P.scene.post = post.get(), P.scene.bsdfs = bsdfs.get();
    P.scene.triCount = triCount, P.scene.bsdfCount = bsdfCount;
  }
};

}  // namespace
