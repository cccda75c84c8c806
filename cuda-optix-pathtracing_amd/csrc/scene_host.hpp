// scene_host.hpp -- the host side of the scene layer (scene_state.hpp): the records of a soup and the two uploads.
//
// Part of dmt_hip.hip's translation unit, included once: after dmt_ctx, HIP_TRY, fail and accel_host.hpp, whose soupArgsOk,
// cull tables, dropMotion and buildBvh an upload of triangles calls, and which names packSoup among its needs through a forward
// declaration.
#pragma once

namespace {

// ---- what dmt_upload_triangles, dmt_update_vertices and dmt_set_motion share ----
// both records of every triangle of a soup (tri_records.hpp; the record kernel of dmt_update_vertices_device runs the same function)
void packSoup(float const* xs, float const* ys, float const* zs, uint32_t const* mat, size_t count, std::vector<TriIsect>& a,
              std::vector<TriPost>& b) {
  a.resize(count), b.resize(count);
  for (size_t i = 0; i < count; ++i) {
    float const v[9] = {xs[4 * i], ys[4 * i], zs[4 * i], xs[4 * i + 1], ys[4 * i + 1], zs[4 * i + 1], xs[4 * i + 2], ys[4 * i + 2], zs[4 * i + 2]};
    packTriangle(v, mat[i], a[i], b[i]);
  }
}

}  // namespace

extern "C" {

int dmt_upload_triangles(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs,
                         const uint32_t* mat_id, size_t count) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!soupArgsOk(xs, ys, zs, mat_id, count)) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_triangles: null array or count out of range");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<TriIsect> a;
  std::vector<TriPost> b;
  packSoup(xs, ys, zs, mat_id, count, a, b);
  uint32_t maxMat = 0;
  for (size_t i = 0; i < count; ++i)
    if (mat_id[i] > maxMat) maxMat = mat_id[i];
  DevBuf<TriIsect> tris;
  DevBuf<TriPost> post;
  HIP_TRY(ctx, tris.assign(a.data(), count));
  HIP_TRY(ctx, post.assign(b.data(), count));
  CullTables cull;
  if (int const rcC = uploadCullTables(ctx, planCullClusters(ctx->ac.bruteCull, CullSoup{xs, ys, zs, mat_id, uint32_t(count)}), a.data(), count, cull)) return rcC;
  SceneState& S = ctx->scene;
  S.tris = std::move(tris), S.post = std::move(post);
  ctx->ac.cull = std::move(cull);
  S.triCount = uint32_t(count);
  S.maxMatId = maxMat;
  S.haveTris = true;
  S.h_xs.assign(xs, xs + 4 * count), S.h_ys.assign(ys, ys + 4 * count), S.h_zs.assign(zs, zs + 4 * count);
  S.h_mat.assign(mat_id, mat_id + count);
  ctx->ac.tree.drop();         // it is of the soup just replaced
  dropMotion(ctx);             // key 1 was a motion from the soup just replaced
  ctx->lights.invalidateEmitters();  // the emitter tree was over triangles of the soup just replaced
  hipError_t const kindRc = ctx->surf.soupReplaced(S.h_mat);  // vertex normals, opacity records and emissive triangles were of the soup just replaced; the material kinds are made anew
  ctx->dn.dropVertexMirror();  // temporal history: its triangle indices are of the soup just replaced
  HIP_TRY(ctx, kindRc);
  if (ctx->accel == DMT_ACCEL_BVH) return buildBvh(ctx);
  return DMT_OK;
}

int dmt_upload_bsdfs(dmt_ctx* ctx, const void* bsdf32, uint32_t count) {
  if (!ctx) return DMT_ERR_INVALID;
  if (count && !bsdf32) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_bsdfs: null array");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<Rec32> bsdfs;
  HIP_TRY(ctx, bsdfs.assign(bsdf32, count));
  // fractional-metallic materials (BS_GGX_BLEND: this record + the conductor record after it) run on the *_tex kernels
  bool blend = false;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t w1;
    memcpy(&w1, static_cast<unsigned char const*>(bsdf32) + 32 * size_t(i) + 4, 4);
    if ((w1 >> 16) == BS_GGX_BLEND) {
      uint32_t w1next = 0;
      if (i + 1 < count) memcpy(&w1next, static_cast<unsigned char const*>(bsdf32) + 32 * size_t(i + 1) + 4, 4);
      if (i + 1 >= count || (w1next >> 16) != BS_GGX_COND)
        return fail(ctx, DMT_ERR_INVALID, "dmt_upload_bsdfs: a blend record (type 4) must be followed by its GGX conductor record");
      blend = true;
    }
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (a launch in flight may read the cutout records dropped below)
  hipError_t const kindRc = ctx->surf.bsdfsReplaced(bsdf32, count, ctx->scene.h_mat);  // the cutout records name the materials just replaced; the material kinds are made anew
  ctx->scene.bsdfs = std::move(bsdfs);
  ctx->scene.hasBlend = blend;
  ctx->scene.bsdfCount = count;
  ctx->scene.haveBsdfs = true;
  HIP_TRY(ctx, kindRc);
  return DMT_OK;
}

}  // extern "C"
