// surface_host.hpp -- the host side of the surface-attribute layer (surface_state.hpp): the MIP chain and the camera
// footprint of the first-hit texture filter, the checks and record builders the uploads share, the chooser of the first-hit
// kernel variant, and the dmt_* entry points of textures, emissive triangles, vertex normals and opacity records.
//
// Part of dmt_hip.hip's translation unit, included once: after the host helpers it uses (dmt_ctx, HIP_TRY, fail;
// camera_host.hpp's cameraFromRaster and worldFromCamera; vnormals.hpp's packRecords and smoothNormals, opacity.hpp's
// opacity_alpha8_at; SceneState::matIdOutside) and before denoise_host.hpp and probes.hpp, which call into it
// (firstHitVariant); camera_host.hpp's dmt_set_camera reaches textureFootprint through a forward declaration.  The
// rule for what each upload invalidates is SurfaceState's table; every hipStreamSynchronize here sits in front of a drop or
// a replace of arrays that a launch in flight may read.
#pragma once

namespace {

// MIP chain of one RGBA8 texture (makeRGBMipmappedTexture, core-texture.cu:340-540): the reference's level count
// (`while (w > 0 || h > 0)`), level l of resolution (max(1, w >> l), max(1, h >> l)), each texel the 2x2 box average of the
// level above in float, stored as a byte by truncation (toByte).  Levels 1.. are appended to `out` row by row; returns the
// level count.  [fix 1] a level where one axis has reached 0 averages the parent texels that exist (1x2 or 2x1); the
// reference stores zeros there.  Textures of other than power-of-two sides (which the reference refuses) follow the same
// rule, so the last odd row or column of a level takes no part in the next, as the reference's indexing would have it.
int buildMipChain(uint8_t const* rgba, int w, int h, std::vector<uint32_t>& out) {
  int levels = 0;
  for (int a = w, b = h; a > 0 || b > 0; a >>= 1, b >>= 1) ++levels;
  out.clear();
  std::vector<uint8_t> prev(rgba, rgba + 4 * size_t(w) * size_t(h)), cur;
  int pw = w, ph = h;
  for (int l = 1; l < levels; ++l) {
    int const cw = std::max(1, w >> l), ch = std::max(1, h >> l);
    cur.assign(4 * size_t(cw) * size_t(ch), 0);
    for (int v = 0; v < ch; ++v)
      for (int u = 0; u < cw; ++u) {
        bool const x1 = 2 * u + 1 < pw, y1 = 2 * v + 1 < ph;
        float const scale = (x1 && y1) ? 0.25f : (x1 || y1) ? 0.5f : 1.f;
        uint32_t word = 0;
        for (int c = 0; c < 4; ++c) {
          auto at = [&](int x, int y) { return float(prev[4 * (size_t(y) * size_t(pw) + size_t(x)) + size_t(c)]) / 255.f; };
          float sum = at(2 * u, 2 * v);  // c00 + c10 + c01 + c11, left to right
          if (x1) sum += at(2 * u + 1, 2 * v);
          if (y1) sum += at(2 * u, 2 * v + 1);
          if (x1 && y1) sum += at(2 * u + 1, 2 * v + 1);
          float const t = scale * sum * 255.f;
          uint8_t const byte = uint8_t(std::min(std::max(t, 0.f), 255.f));
          cur[4 * (size_t(v) * size_t(cw) + size_t(u)) + size_t(c)] = byte;
          word |= uint32_t(byte) << (8 * c);
        }
        out.push_back(word);
      }
    prev.swap(cur);
    pw = cw, ph = ch;
  }
  return levels;
}

// The camera's footprint for the first-hit texture filter (minDifferentialsFromCamera, core-render.cpp:928-980), once per
// camera: 512 rays along the film diagonal, pFilm = i / 511 * resolution; for each, the x / y neighbour directions
// (camera-space direction + one raster step) in Frame::fromZ(ray.d) (gramSchmidt, cudautils-vecmath.cu:960-969); the
// smallest of each by squared length is kept (strict <, so the first of equals).  The origin differentials of a pinhole
// camera are 0.  The scale is max(1/8, 1/sqrt(spp)) of the frame's spp (dmt_camera.spp; < 1 counts as 1).  Evaluated in
// double from the float matrices of dmt_set_camera; out = camera-from-render as a row-major 3x4, min dx[3], min dy[3], scale.
void textureFootprint(dmt_camera const& cam, float out[19]) {
  float cf[16], rf[16];
  cameraFromRaster(cam.focal_length, cam.sensor_size, uint32_t(cam.width), uint32_t(cam.height), cf);
  worldFromCamera(cam.dir, cam.pos, rf);
  struct D3 { double x, y, z; };
  auto add = [](D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; };
  auto sub = [](D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; };
  auto dotd = [](D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
  auto crossd = [](D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
  auto norm = [&](D3 a) { double const l = std::sqrt(dotd(a, a)); return D3{a.x / l, a.y / l, a.z / l}; };
  auto point = [](float const* m, D3 p) {  // affine, column-major
    return D3{m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
              m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]};
  };
  auto dir = [](float const* m, D3 v) {
    return D3{m[0] * v.x + m[4] * v.y + m[8] * v.z, m[1] * v.x + m[5] * v.y + m[9] * v.z, m[2] * v.x + m[6] * v.y + m[10] * v.z};
  };
  auto dirT = [](float const* m, D3 v) {  // the inverse of the rotation: its transpose
    return D3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
  };
  D3 const pos{rf[12], rf[13], rf[14]};
  D3 const tr = dirT(rf, pos);
  for (int r = 0; r < 3; ++r) {
    out[4 * r + 0] = rf[4 * r + 0], out[4 * r + 1] = rf[4 * r + 1], out[4 * r + 2] = rf[4 * r + 2];
    out[4 * r + 3] = float(-(r == 0 ? tr.x : r == 1 ? tr.y : tr.z));
  }
  D3 const dxCam = sub(point(cf, D3{1, 0, 0}), point(cf, D3{0, 0, 0}));
  D3 const dyCam = sub(point(cf, D3{0, 1, 0}), point(cf, D3{0, 0, 0}));
  double const inf = std::numeric_limits<double>::infinity();
  D3 minX{inf, inf, inf}, minY{inf, inf, inf};
  for (int i = 0; i < 512; ++i) {
    double const f = double(i) / 511.0;
    D3 const pCam = point(cf, D3{f * cam.width, f * cam.height, 0});
    D3 const d = norm(dir(rf, norm(pCam)));
    D3 const rx = norm(dir(rf, add(dirT(rf, d), dxCam)));
    D3 const ry = norm(dir(rf, add(dirT(rf, d), dyCam)));
    D3 const gx = (d.x != d.y || d.x != d.z) ? D3{d.z - d.y, d.x - d.z, d.y - d.x} : D3{d.z - d.y, d.x + d.z, -d.y - d.x};
    D3 const fx = norm(gx), fy = crossd(d, fx);
    auto local = [&](D3 v) { return D3{dotd(v, fx), dotd(v, fy), dotd(v, d)}; };
    D3 const df = norm(local(d)), dxf = norm(local(rx)), dyf = norm(local(ry));
    D3 const ex = sub(dxf, df), ey = sub(dyf, df);
    if (dotd(ex, ex) < dotd(minX, minX)) minX = ex;
    if (dotd(ey, ey) < dotd(minY, minY)) minY = ey;
  }
  out[12] = float(minX.x), out[13] = float(minX.y), out[14] = float(minX.z);
  out[15] = float(minY.x), out[16] = float(minY.y), out[17] = float(minY.z);
  out[18] = float(std::max(0.125, 1.0 / std::sqrt(double(std::max(cam.spp, 1)))));
}

// every descriptor {first texel, width, height} lies inside a texel array of `texelCount` words and has no side above `maxSide`
bool descriptorsInside(int32_t const* desc3, uint32_t textureCount, uint64_t texelCount, int64_t maxSide) {
  for (uint32_t k = 0; k < textureCount; ++k) {
    int64_t const first = desc3[3 * k], w = desc3[3 * k + 1], h = desc3[3 * k + 2];
    if (first < 0 || w <= 0 || h <= 0 || w > maxSide || h > maxSide || uint64_t(first) + uint64_t(w) * uint64_t(h) > texelCount) return false;
  }
  return true;
}

// the cutout record of a triangle with the UVs uv6: of the texture with descriptor desc3, or opaque (null)
OpacityRec makeOpacityRec(float const* uv6, int32_t const* desc3) {
  return OpacityRec{uv6[0], uv6[1], uv6[2], uv6[3], uv6[4], uv6[5], desc3 ? uint32_t(desc3[0]) : 0u,
                    desc3 ? uint32_t(desc3[1]) | (uint32_t(desc3[2]) << 16) : 0u};
}

// The first-hit kernels (k_aov*, k_test_trace_log*) have one variant per feature that changes what a camera ray hits or the
// normal it is shaded with: 0 plain, 1 vertex normals, 2 motion, 3 cutout.  No kernel combines two of them.
int firstHitVariant(dmt_ctx* ctx, char const* who, int* variant) {
  bool const normals = ctx->surf.vn.have, motion = ctx->ac.haveMotion, cutout = ctx->surf.op.have;
  if (ctx->medium.active())  // the feature pass and the path log know surfaces only
    return fail(ctx, DMT_ERR_STATE, (std::string(who) + ": a participating medium (dmt_set_medium) is not supported here").c_str());
  if (normals && motion)
    return fail(ctx, DMT_ERR_STATE, (std::string(who) + ": vertex normals (dmt_upload_vertex_normals) together with motion blur are not supported").c_str());
  if (cutout && (motion || normals))
    return fail(ctx, DMT_ERR_STATE, (std::string(who) + ": opacity textures (dmt_upload_opacity) together with motion blur or vertex normals are not supported").c_str());
  *variant = cutout ? 3 : motion ? 2 : normals ? 1 : 0;
  return DMT_OK;
}

// dmt_clear_vertex_normals, dmt_clear_opacity: drops the record, if there is one
template <class Rec>
int clearRecord(dmt_ctx* ctx, Rec& rec) {
  if (!rec.have) return DMT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the records
  rec = Rec{};
  return DMT_OK;
}

}  // namespace

extern "C" {

// ---- emissive triangles ----------------------------------------------------------------------
// The list is of the uploaded soup: without one, or with count 0, the context has no emissive triangles, and a refused list
// leaves none either: the record is emptied first and gets its count last.
int dmt_upload_area_lights(dmt_ctx* ctx, const uint32_t* triangle_index, const float* radiance_rgb, uint32_t count) {
  if (!ctx || (count && (!triangle_index || !radiance_rgb))) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  SurfaceState::Emissive& area = ctx->surf.area = SurfaceState::Emissive{};
  ctx->lights.invalidateEmitters();  // the emitter tree was of the old list
  if (count == 0 || !ctx->scene.haveTris) return DMT_OK;
  std::vector<uint32_t> of(ctx->scene.triCount, 0xFFFFFFFFu);
  for (uint32_t k = 0; k < count; ++k) {
    if (triangle_index[k] >= ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "area light refers to a triangle outside the uploaded soup");
    of[triangle_index[k]] = k;
  }
  HIP_TRY(ctx, area.of.assign(of.data(), of.size()));
  HIP_TRY(ctx, area.tri.assign(triangle_index, count));
  HIP_TRY(ctx, area.le.assign(radiance_rgb, 3 * size_t(count)));
  area.hostTri.assign(triangle_index, triangle_index + count), area.hostLe.assign(radiance_rgb, radiance_rgb + 3 * size_t(count));
  area.count = count;
  return DMT_OK;
}

// ---- material kind per triangle (SurfaceState::Kind) --------------------------------------------------------
// What a launch reads: the device array where the table travels as one, the words that go into the kernel arguments otherwise.
int dmt_tri_kind_bits(dmt_ctx* ctx, uint32_t* out, uint64_t words) {
  if (!ctx) return DMT_ERR_INVALID;
  SurfaceState::Kind const& kind = ctx->surf.kind;
  size_t const n = kind.words.size();
  if (words < n || (n && !out)) return fail(ctx, DMT_ERR_INVALID, "dmt_tri_kind_bits: room for (triangles + 31) / 32 words is needed");
  if (n == 0) return DMT_OK;
  if (kind.bits.get()) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(out, kind.bits.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  } else {
    RenderParams P{};
    ctx->surf.fill(P);
    for (size_t w = 0; w < n; ++w) out[w] = w < 2 ? P.triKindInline[w] : 0u;  // (n > 2 here only after a failed upload of the table: all zeros)
  }
  return DMT_OK;
}

// ---- image textures and the first-hit texture filter -------------------------
int dmt_upload_textures(dmt_ctx* ctx, const uint8_t* rgba8, uint64_t texel_count, const int32_t* desc3, uint32_t texture_count,
                        const uint32_t* mat_tex4, uint32_t bsdf_count, const float* tri_uv6, uint64_t triangle_count) {
  if (!ctx) return DMT_ERR_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->surf.texturesReplaced();  // the old tables go before the new ones are looked at; the cutout records point into them
  SurfaceState::Textures& tex = ctx->surf.tex;  // filled in place, the counts last: without them the context has no textures
  if (texture_count == 0) return DMT_OK;  // cleared
  if (!rgba8 || !desc3 || !mat_tex4 || !tri_uv6 || texel_count == 0 || bsdf_count == 0 || triangle_count == 0)
    return fail(ctx, DMT_ERR_INVALID, "dmt_upload_textures: null array or zero count");
  if (!descriptorsInside(desc3, texture_count, texel_count, INT32_MAX))
    return fail(ctx, DMT_ERR_INVALID, "dmt_upload_textures: texture descriptor outside the texel array");
  for (uint32_t b = 0; b < bsdf_count; ++b)
    for (int j = 0; j < 3; ++j) {
      uint32_t const t = mat_tex4[4 * size_t(b) + size_t(j)];
      if (t != 0xFFFFFFFFu && t >= texture_count) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_textures: material refers to a texture that does not exist");
    }
  std::vector<uint32_t> mip;  // levels 1.. of every texture, back to back (upload-time host work)
  std::vector<int32_t> mipDesc(2 * size_t(texture_count));
  for (uint32_t k = 0; k < texture_count; ++k) {
    std::vector<uint32_t> chain;
    mipDesc[2 * k] = buildMipChain(rgba8 + 4 * size_t(desc3[3 * k]), desc3[3 * k + 1], desc3[3 * k + 2], chain);
    if (mip.size() + chain.size() > size_t(INT32_MAX)) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_textures: MIP chains too large");
    mipDesc[2 * k + 1] = int32_t(mip.size());
    mip.insert(mip.end(), chain.begin(), chain.end());
  }
  HIP_TRY(ctx, tex.mip.assign(mip.data(), mip.size()));
  HIP_TRY(ctx, tex.mipDesc.assign(mipDesc.data(), mipDesc.size()));
  HIP_TRY(ctx, tex.rgba.assign(rgba8, size_t(texel_count)));
  HIP_TRY(ctx, tex.desc.assign(desc3, 3 * size_t(texture_count)));
  HIP_TRY(ctx, tex.matTex.assign(mat_tex4, 4 * size_t(bsdf_count)));
  HIP_TRY(ctx, tex.triUv.assign(tri_uv6, 6 * size_t(triangle_count)));
  tex.count = texture_count, tex.matTexCount = bsdf_count, tex.triUvCount = size_t(triangle_count);
  return DMT_OK;
}

int dmt_set_texture_filter(dmt_ctx* ctx, int mode) {
  if (!ctx) return DMT_ERR_INVALID;
  if (mode != DMT_TEXFILTER_LEVEL0 && mode != DMT_TEXFILTER_REFERENCE) return fail(ctx, DMT_ERR_INVALID, "dmt_set_texture_filter: unknown mode");
  ctx->surf.texFilter = mode;
  return DMT_OK;
}

int dmt_texture_mip_chain(const uint8_t* rgba8, int width, int height, uint8_t* out, uint64_t out_texels, int* levels) {
  if (!rgba8 || width <= 0 || height <= 0 || width > 65536 || height > 65536 || !levels) return DMT_ERR_INVALID;
  std::vector<uint32_t> chain;
  *levels = buildMipChain(rgba8, width, height, chain);
  if (out_texels < chain.size() || (!out && !chain.empty())) return DMT_ERR_INVALID;
  if (!chain.empty()) memcpy(out, chain.data(), 4 * chain.size());
  return DMT_OK;
}

int dmt_texture_footprint(const dmt_camera* cam, float* out) {
  if (!cam || !out || cam->width <= 0 || cam->height <= 0) return DMT_ERR_INVALID;
  textureFootprint(*cam, out);
  return DMT_OK;
}

// ---- smooth shading -----------------------------------------------------------------------
int dmt_upload_vertex_normals(dmt_ctx* ctx, const float* n9, size_t count) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->scene.haveTris) return fail(ctx, DMT_ERR_STATE, "dmt_upload_vertex_normals: before any dmt_upload_triangles");
  if (count != ctx->scene.triCount) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_vertex_normals: count differs from the uploaded triangle count");
  if (count && !n9) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_vertex_normals: null array");
  std::vector<VtxNormalRec> recs;
  SurfaceState::VertexNormals vn;  // adopted at the end
  long long const bad = vnormals::packRecords(n9, count, recs, &vn.smooth);
  if (bad >= 0)
    return fail(ctx, DMT_ERR_INVALID, ("dmt_upload_vertex_normals: triangle " + std::to_string(bad) +
                                       " has a normal that is not finite or shorter than 1e-6 (all nine zeros mark a flat triangle)").c_str());
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the old records
  HIP_TRY(ctx, vn.recs.assign(recs.data(), count));
  vn.have = true;
  ctx->surf.vn = std::move(vn);
  return DMT_OK;
}

int dmt_clear_vertex_normals(dmt_ctx* ctx) { return ctx ? clearRecord(ctx, ctx->surf.vn) : DMT_ERR_INVALID; }

int dmt_vertex_normals_info(dmt_ctx* ctx, uint64_t* triangles, uint64_t* smooth_triangles) {
  if (!ctx) return DMT_ERR_INVALID;
  if (triangles) *triangles = ctx->surf.vn.have ? ctx->scene.triCount : 0u;
  if (smooth_triangles) *smooth_triangles = ctx->surf.vn.smooth;  // a dropped record holds zeros
  return DMT_OK;
}

int dmt_smooth_normals(const float* xs, const float* ys, const float* zs, size_t count, float crease_degrees, float* n9_out) {
  if (!std::isfinite(crease_degrees) || (count && (!xs || !ys || !zs || !n9_out))) return DMT_ERR_INVALID;
  vnormals::smoothNormals(xs, ys, zs, count, crease_degrees, n9_out);
  return DMT_OK;
}

// ---- alpha cutouts ------------------------------------------------------------------------
int dmt_upload_opacity(dmt_ctx* ctx, const uint32_t* mat_opacity_tex, uint32_t bsdf_count, float cutoff) {
  if (!ctx) return DMT_ERR_INVALID;
  SurfaceState::Textures const& tex = ctx->surf.tex;
  if (!ctx->scene.haveTris || !ctx->scene.haveBsdfs || tex.count == 0)
    return fail(ctx, DMT_ERR_STATE, "dmt_upload_opacity: upload triangles, BSDFs and textures first");
  if (tex.triUvCount != ctx->scene.triCount)
    return fail(ctx, DMT_ERR_STATE, "dmt_upload_opacity: the uploaded textures carry no UV triple per uploaded triangle (upload textures last)");
  if (!mat_opacity_tex || bsdf_count != ctx->scene.bsdfCount) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_opacity: null array, or count differs from the uploaded BSDF count");
  if (!std::isfinite(cutoff) || cutoff < 0.f || cutoff > 1.f) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_opacity: the cutoff must be finite and in [0, 1]");
  for (uint32_t b = 0; b < bsdf_count; ++b)
    if (mat_opacity_tex[b] != 0xFFFFFFFFu && mat_opacity_tex[b] >= tex.count)
      return fail(ctx, DMT_ERR_INVALID, "dmt_upload_opacity: a material refers to a texture that does not exist");
  if (ctx->scene.matIdOutside()) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_opacity: material index outside the BSDF array");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // launches in flight read the old records
  std::vector<int32_t> desc(3 * size_t(tex.count));
  std::vector<float> uv(6 * size_t(ctx->scene.triCount));
  HIP_TRY(ctx, hipMemcpy(desc.data(), tex.desc.get(), desc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (!uv.empty()) HIP_TRY(ctx, hipMemcpy(uv.data(), tex.triUv.get(), uv.size() * sizeof(float), hipMemcpyDeviceToHost));
  SurfaceState::Opacity op;  // counted into, adopted at the end
  for (uint32_t b = 0; b < bsdf_count; ++b) {
    uint32_t const t = mat_opacity_tex[b];
    if (t == 0xFFFFFFFFu) continue;
    ++op.cutoutMats;
    if (desc[3 * size_t(t) + 1] > 65535 || desc[3 * size_t(t) + 2] > 65535)
      return fail(ctx, DMT_ERR_INVALID, ("dmt_upload_opacity: opacity texture " + std::to_string(t) + " is wider or taller than 65535 texels").c_str());
  }
  std::vector<OpacityRec> recs(ctx->scene.triCount);
  for (size_t i = 0; i < ctx->scene.triCount; ++i) {
    float const* const q = &uv[6 * i];
    uint32_t const t = mat_opacity_tex[ctx->scene.h_mat[i]];
    bool const cutout = t != 0xFFFFFFFFu;
    for (int j = 0; cutout && j < 6; ++j)
      if (!std::isfinite(q[j]) || std::fabs(q[j]) > 1048576.f)
        return fail(ctx, DMT_ERR_INVALID, ("dmt_upload_opacity: triangle " + std::to_string(i) + " of a cutout material has a UV that is not finite or beyond 2^20").c_str());
    recs[i] = makeOpacityRec(q, cutout ? &desc[3 * size_t(t)] : nullptr);
    op.cutoutTris += cutout;
  }
  HIP_TRY(ctx, op.recs.assign(recs.data(), recs.size()));
  op.have = true, op.cutoff = cutoff;
  ctx->surf.op = std::move(op);
  return DMT_OK;
}

int dmt_clear_opacity(dmt_ctx* ctx) { return ctx ? clearRecord(ctx, ctx->surf.op) : DMT_ERR_INVALID; }

int dmt_opacity_info(dmt_ctx* ctx, uint64_t* cutout_triangles, uint32_t* cutout_materials, float* cutoff) {
  if (!ctx) return DMT_ERR_INVALID;
  if (cutout_triangles) *cutout_triangles = ctx->surf.op.cutoutTris;  // a dropped record holds zeros
  if (cutout_materials) *cutout_materials = ctx->surf.op.cutoutMats;
  if (cutoff) *cutoff = ctx->surf.op.cutoff;
  return DMT_OK;
}

int dmt_opacity_eval(const uint8_t* rgba8, uint64_t texel_count, const int32_t* desc3, uint32_t texture_count, int n, const int32_t* tex,
                     const float* uv6, const float* bu, const float* bv, float cutoff, float* alpha8_out, uint8_t* pass_out) {
  if (n < 0 || !rgba8 || !desc3 || texture_count == 0 || !std::isfinite(cutoff) || cutoff < 0.f || cutoff > 1.f) return DMT_ERR_INVALID;
  if (n && (!tex || !uv6 || !bu || !bv || !alpha8_out || !pass_out)) return DMT_ERR_INVALID;
  if (!descriptorsInside(desc3, texture_count, texel_count, 65535)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (tex[i] < 0 || uint32_t(tex[i]) >= texture_count) return DMT_ERR_INVALID;
  struct Texels {  // the RGBA8 store as the device's little-endian words
    uint8_t const* p;
    uint32_t operator[](size_t i) const { return uint32_t(p[4 * i]) | uint32_t(p[4 * i + 1]) << 8 | uint32_t(p[4 * i + 2]) << 16 | uint32_t(p[4 * i + 3]) << 24; }
  };
  for (int i = 0; i < n; ++i) {
    OpacityRec const R = makeOpacityRec(uv6 + 6 * size_t(i), desc3 + 3 * size_t(tex[i]));
    alpha8_out[i] = opacity_alpha8_at(Texels{rgba8}, R, bu[i], bv[i]);
    pass_out[i] = alpha8_out[i] >= cutoff * 255.f ? 1 : 0;
  }
  return DMT_OK;
}

}  // extern "C"
