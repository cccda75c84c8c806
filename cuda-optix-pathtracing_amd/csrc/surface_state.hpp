// surface_state.hpp -- what a context keeps for the surface-attribute layer: image textures with their MIP chains and UVs,
// the first-hit texture filter and its camera footprint, per-vertex normals, opacity records and emissive triangles.  The
// layer's device code is in surface_device.hpp (vnormals.hpp, opacity.hpp), its helpers and entry points in surface_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, RenderParams, VtxNormalRec and
// OpacityRec.
//
// What invalidates what.  "drop" frees a record's arrays and zeroes its counts, so its *_info call answers zeros and fill()
// leaves its RenderParams fields null.  The caller has drained the stream where a launch in flight may read the arrays.
//
//   event            member function     vertex normals   opacity   emissive triangles   textures and UVs                             material kinds
//   soup replaced    soupReplaced        drop             drop      drop                 kept (checked at launch: texturesMatch)      rebuilt
//   BSDFs replaced   bsdfsReplaced       kept             drop      kept                 kept (checked at launch: texturesMatch)      rebuilt
//   textures         texturesReplaced    kept             drop      kept                 the old tables are dropped first: a refused  kept
//   replaced or                                                                          upload leaves the context without textures
//   cleared
//   vertices updated (none)              kept             kept      kept                 kept                                         kept
//   (dmt_update_vertices*)
//
// Opacity records are made from the soup's materials, the texture descriptors and the UVs, so each of the three takes them
// along.  The texture filter mode and the camera footprint survive everything (dmt_set_texture_filter, dmt_set_camera).
// The material kinds (Kind: a bit per triangle, set where its material is a GGX one) are a function of the soup's material
// ids and the BSDF records, and are made anew from both by the two events that replace either; dmt_tri_kind_bits reads them.
//
//   setting                   setter                  environment variable
//   kind.allowInline          --                      DMT_TRI_KIND_INLINE (0: the kinds always travel as a device array; tests)
#pragma once

namespace {

struct SurfaceState {
  // SURVEY 8f-1 image textures (dmt_upload_textures)
  struct Textures {
    DevBuf<uint32_t> rgba;
    DevBuf<int32_t> desc;      // 3 words per texture
    DevBuf<uint32_t> matTex;   // 4 words per BSDF
    DevBuf<float> triUv;       // 6 floats per triangle
    DevBuf<uint32_t> mip;      // MIP levels 1.. of every texture (buildMipChain)
    DevBuf<int32_t> mipDesc;   // 2 words per texture: {levels, first texel of level 1}
    uint32_t count = 0, matTexCount = 0;
    size_t triUvCount = 0;
  } tex;
  int texFilter = DMT_TEXFILTER_LEVEL0;
  float texFoot[19] = {};      // dmt_texture_footprint of the current camera
  // smooth shading (dmt_upload_vertex_normals; vnormals.hpp): one record per triangle of the soup
  struct VertexNormals {
    DevBuf<VtxNormalRec> recs;
    bool have = false;
    uint64_t smooth = 0;       // triangles with a smooth record
  } vn;
  // alpha cutouts (dmt_upload_opacity; opacity.hpp): one record per triangle of the soup
  struct Opacity {
    DevBuf<OpacityRec> recs;
    bool have = false;
    float cutoff = 0.f;
    uint64_t cutoutTris = 0;
    uint32_t cutoutMats = 0;
  } op;
  // SURVEY 8f-3 emissive triangles (dmt_upload_area_lights)
  struct Emissive {
    DevBuf<uint32_t> of, tri;  // [triangle] index into the list, 0xFFFFFFFF: not emissive; [count] triangle index
    DevBuf<float> le;          // [count] rgb radiance
    uint32_t count = 0;
    std::vector<uint32_t> hostTri;  // host copies of tri and le: what the emitter tree is built from (light_host.hpp)
    std::vector<float> hostLe;
  } area;
  // material kind per triangle (k_megakernel's ggx_park; dmt_tri_kind_bits): bit i of word i >> 5 is set when the material
  // of ORIGINAL triangle i is a GGX one.  Host arithmetic over the soup's material ids and the BSDF records' type words,
  // redone whenever either is replaced; a material id beyond the BSDF array counts as not GGX (such a scene is refused at
  // launch).  A soup of at most kTriKindInlineTris triangles travels in the kernel arguments, a larger one -- or every one,
  // with DMT_TRI_KIND_INLINE=0 at context creation -- as a device array.
  struct Kind {
    std::vector<uint8_t> matGgx;   // [bsdf] 1: hi16(w[1]) is BS_GGX_DIEL or BS_GGX_COND
    std::vector<uint32_t> words;   // the table, (triangles + 31) / 32 words
    DevBuf<uint32_t> bits;         // its device copy; empty while the table travels in the arguments
    bool allowInline = true;
  } kind;
  static constexpr size_t kTriKindInlineTris = 64;

  // the events of the table above.  Each rebuilds `kind`, from the soup's material ids and, bsdfsReplaced, the new records;
  // a failed upload of the table leaves it empty and in the arguments (no hit is parked then: slower, the same film).
  hipError_t soupReplaced(std::vector<uint32_t> const& matId) {
    vn = VertexNormals{}, op = Opacity{}, area = Emissive{};
    return buildKind(matId);
  }
  hipError_t bsdfsReplaced(void const* bsdf32, uint32_t count, std::vector<uint32_t> const& matId) {
    op = Opacity{};
    kind.matGgx.assign(count, 0);
    for (uint32_t i = 0; i < count; ++i) {
      uint32_t w1;
      memcpy(&w1, static_cast<unsigned char const*>(bsdf32) + 32 * size_t(i) + 4, 4);
      kind.matGgx[i] = (w1 >> 16) == BS_GGX_DIEL || (w1 >> 16) == BS_GGX_COND;
    }
    return buildKind(matId);
  }
  void texturesReplaced() { tex = Textures{}, op = Opacity{}; }

  hipError_t buildKind(std::vector<uint32_t> const& matId) {
    kind.words.assign((matId.size() + 31) / 32, 0u);
    for (size_t i = 0; i < matId.size(); ++i)
      if (matId[i] < kind.matGgx.size() && kind.matGgx[matId[i]]) kind.words[i >> 5] |= 1u << (i & 31);
    DevBuf<uint32_t> fresh;  // (a new array: a launch in flight may read the old one, whose release waits for it)
    if (!kind.allowInline || matId.size() > kTriKindInlineTris) {
      hipError_t const e = fresh.assign(kind.words.data(), kind.words.size());
      if (e != hipSuccess) {
        kind.words.assign(kind.words.size(), 0u), kind.bits.reset();
        return e;
      }
    }
    kind.bits = std::move(fresh);
    return hipSuccess;
  }

  // the texture tables, if any, are of the uploaded BSDFs and triangles: what every launch that reads them asks first
  bool texturesMatch(uint32_t bsdfCount, size_t triCount) const { return tex.count == 0 || (tex.matTexCount == bsdfCount && tex.triUvCount == triCount); }

  // the layer's part of the argument struct (baseParams)
  void fill(RenderParams& P) const {
    P.areaOf = area.of.get(), P.areaTri = area.tri.get(), P.areaLe = area.le.get(), P.areaCount = area.count;
    P.triKindBits = kind.bits.get();
    for (size_t w = 0; !P.triKindBits && w < 2 && w < kind.words.size(); ++w) P.triKindInline[w] = kind.words[w];
    if (vn.have) P.vtxNormals = vn.recs.get();
    if (op.have) P.opacity = op.recs.get(), P.opacityCutoff8 = op.cutoff * 255.f;
    if (tex.count > 0) {
      P.texRgba = tex.rgba.get(), P.texDesc = tex.desc.get(), P.matTex = tex.matTex.get(), P.triUv = tex.triUv.get();
      P.texMip = tex.mip.get(), P.texMipDesc = tex.mipDesc.get();
      memcpy(P.texCfr, texFoot, 12 * sizeof(float));
      memcpy(P.texMinDx, texFoot + 12, 3 * sizeof(float));
      memcpy(P.texMinDy, texFoot + 15, 3 * sizeof(float));
      P.texSppScale = texFoot[18];
    }
  }
};

}  // namespace
