// dmt_host_c.cpp -- flat C view of the host-side scene library (for ctypes / other FFIs).
#include <cstdio>
#include <cstring>
#include <new>

#include "dmt_scene.hpp"

using namespace dmt_host;

extern "C" {

struct dmt_host_scene {
  Scene s;
};

dmt_host_scene* dmt_host_scene_cornell_box() {
  auto* h = new (std::nothrow) dmt_host_scene();
  if (h) h->s = cornellBox();
  return h;
}
dmt_host_scene* dmt_host_scene_random_triangles(uint64_t count, uint64_t seed) {
  auto* h = new (std::nothrow) dmt_host_scene();
  if (h) h->s = randomTriangleScene(size_t(count), seed);
  return h;
}
dmt_host_scene* dmt_host_scene_random_triangles_ex(uint64_t count, uint64_t seed, float extent) {
  if (!(extent > 0.f)) return nullptr;
  auto* h = new (std::nothrow) dmt_host_scene();
  if (h) h->s = randomTriangleScene(size_t(count), seed, extent);
  return h;
}
// JSON front-end; on failure returns null and copies the message (NUL-terminated, truncated) into err
dmt_host_scene* dmt_host_scene_load_json(const char* path, int* max_depth, int* samples_per_pixel, char* err, uint64_t err_cap) {
  auto* h = new (std::nothrow) dmt_host_scene();
  if (!h || !path) return delete h, nullptr;
  JsonScene js;
  std::string msg;
  if (!loadJsonScene(path, js, &msg)) {
    if (err && err_cap) {
      size_t const n = msg.size() < err_cap - 1 ? msg.size() : size_t(err_cap - 1);
      memcpy(err, msg.data(), n);
      err[n] = 0;
    }
    delete h;
    return nullptr;
  }
  h->s = std::move(js.scene);
  if (max_depth) *max_depth = js.maxDepth;
  if (samples_per_pixel) *samples_per_pixel = js.samplesPerPixel;
  return h;
}
// first mesh of a binary FBX file as a triangle list (9 floats per triangle); returns the triangle count, -1 on
// failure (message in err).  Call with out == null to get the count.
int64_t dmt_host_read_fbx(const char* path, float* out9, uint64_t cap_triangles, char* err, uint64_t err_cap) {
  std::vector<Triangle> tris;
  std::string msg;
  if (!path || !readFbxMesh(path, tris, &msg)) {
    if (err && err_cap) {
      size_t const n = msg.size() < err_cap - 1 ? msg.size() : size_t(err_cap - 1);
      memcpy(err, msg.data(), n);
      err[n] = 0;
    }
    return -1;
  }
  if (out9)
    for (size_t i = 0; i < tris.size() && i < cap_triangles; ++i) {
      Vec3 const v[3] = {tris[i].v0, tris[i].v1, tris[i].v2};
      for (int k = 0; k < 3; ++k) out9[9 * i + 3 * size_t(k)] = v[k].x, out9[9 * i + 3 * size_t(k) + 1] = v[k].y, out9[9 * i + 3 * size_t(k) + 2] = v[k].z;
    }
  return int64_t(tris.size());
}
// the vertex normals of the same mesh (9 floats per triangle, the triangles and corners of dmt_host_read_fbx); returns the
// number of triangles that carry normals -- 0 for a file without a normal layer -- or -1 on failure.  Same protocol.
int64_t dmt_host_read_fbx_normals(const char* path, float* out9, uint64_t cap_triangles, char* err, uint64_t err_cap) {
  std::vector<Triangle> tris;
  std::vector<float> n9;
  std::string msg;
  if (!path || !readFbxMesh(path, tris, &msg, nullptr, &n9)) {
    if (err && err_cap) {
      size_t const n = msg.size() < err_cap - 1 ? msg.size() : size_t(err_cap - 1);
      memcpy(err, msg.data(), n);
      err[n] = 0;
    }
    return -1;
  }
  size_t const count = n9.size() / 9;
  if (out9 && count) memcpy(out9, n9.data(), 9 * sizeof(float) * (count < cap_triangles ? count : size_t(cap_triangles)));
  return int64_t(count);
}
// PBRT-v4 subset front-end; same protocol as dmt_host_scene_load_json
dmt_host_scene* dmt_host_scene_load_pbrt(const char* path, int* max_depth, int* samples_per_pixel, char* err, uint64_t err_cap) {
  auto* h = new (std::nothrow) dmt_host_scene();
  if (!h || !path) return delete h, nullptr;
  PbrtScene ps;
  std::string msg;
  if (!loadPbrtScene(path, ps, &msg)) {
    if (err && err_cap) {
      size_t const n = msg.size() < err_cap - 1 ? msg.size() : size_t(err_cap - 1);
      memcpy(err, msg.data(), n);
      err[n] = 0;
    }
    delete h;
    return nullptr;
  }
  h->s = std::move(ps.scene);
  if (max_depth) *max_depth = ps.maxDepth;
  if (samples_per_pixel) *samples_per_pixel = ps.samplesPerPixel;
  return h;
}
uint32_t dmt_host_scene_area_light_count(const dmt_host_scene* h) { return uint32_t(h->s.areaTri.size()); }
const uint32_t* dmt_host_scene_area_tri(const dmt_host_scene* h) { return h->s.areaTri.data(); }
const float* dmt_host_scene_area_le(const dmt_host_scene* h) { return h->s.areaLe.data(); }
const float* dmt_host_scene_env_rgb(const dmt_host_scene* h, int* width, int* height) {
  if (width) *width = h->s.envWidth;
  if (height) *height = h->s.envHeight;
  return h->s.envRgb.empty() ? nullptr : h->s.envRgb.data();
}
// image textures: counts, then the four arrays in dmt_upload_textures' layout
uint32_t dmt_host_scene_texture_count(const dmt_host_scene* h) { return uint32_t(h->s.texDesc.size() / 3); }
uint64_t dmt_host_scene_texel_count(const dmt_host_scene* h) { return uint64_t(h->s.texRgba.size() / 4); }
const uint8_t* dmt_host_scene_tex_rgba(const dmt_host_scene* h) { return h->s.texRgba.data(); }
const int32_t* dmt_host_scene_tex_desc(const dmt_host_scene* h) { return h->s.texDesc.data(); }
const uint32_t* dmt_host_scene_mat_tex(const dmt_host_scene* h) { return h->s.matTex.data(); }
const float* dmt_host_scene_tri_uv(const dmt_host_scene* h) { return h->s.triUv.data(); }
// vertex normals (smooth shading): 9 floats per triangle, or null when no mesh of the scene carries any
const float* dmt_host_scene_tri_normals(const dmt_host_scene* h) { return h->s.triNormals.empty() ? nullptr : h->s.triNormals.data(); }
// alpha cutouts: per BSDF the opacity texture (0xFFFFFFFF = opaque), or null when no material of the scene names one; the cutoff
const uint32_t* dmt_host_scene_mat_opacity(const dmt_host_scene* h) { return h->s.matOpacity.empty() ? nullptr : h->s.matOpacity.data(); }
float dmt_host_scene_opacity_cutoff(const dmt_host_scene* h) { return h->s.opacityCutoff; }
void dmt_host_scene_destroy(dmt_host_scene* h) { delete h; }

uint64_t dmt_host_scene_triangle_count(const dmt_host_scene* h) { return h->s.triangleCount(); }
uint32_t dmt_host_scene_bsdf_count(const dmt_host_scene* h) { return uint32_t(h->s.bsdfs.size()); }
uint32_t dmt_host_scene_light_count(const dmt_host_scene* h) { return uint32_t(h->s.lights.size()); }
uint32_t dmt_host_scene_infinite_light_count(const dmt_host_scene* h) { return uint32_t(h->s.infiniteLights.size()); }
const float* dmt_host_scene_xs(const dmt_host_scene* h) { return h->s.xs.data(); }
const float* dmt_host_scene_ys(const dmt_host_scene* h) { return h->s.ys.data(); }
const float* dmt_host_scene_zs(const dmt_host_scene* h) { return h->s.zs.data(); }
const uint32_t* dmt_host_scene_mat_ids(const dmt_host_scene* h) { return h->s.matId.data(); }
const void* dmt_host_scene_bsdfs(const dmt_host_scene* h) { return h->s.bsdfs.data(); }
const void* dmt_host_scene_lights(const dmt_host_scene* h) { return h->s.lights.data(); }
const void* dmt_host_scene_infinite_lights(const dmt_host_scene* h) { return h->s.infiniteLights.data(); }
dmt_camera* dmt_host_scene_camera(dmt_host_scene* h) { return &h->s.camera; }
void dmt_host_scene_lens(const dmt_host_scene* h, float* lens_radius, float* focus_distance) {
  *lens_radius = h->s.lensRadius, *focus_distance = h->s.focusDistance;
}
void dmt_host_scene_projection(const dmt_host_scene* h, int* kind, float* param) {
  *kind = h->s.projection, *param = h->s.projectionParam;
}
// the pixel filter the scene file records (not applied by an upload unless asked): 0 without one, 1 for a kind the library
// offers (*kind = its DMT_FILTER_* value), 2 for an unsupported kind (mitchell, sinc); radius, sigma, and the file's name
// for the kind (up to name_cap - 1 characters)
int dmt_host_scene_pixel_filter(const dmt_host_scene* h, int* kind, float* radius, float* sigma, char* name, int name_cap) {
  dmt_host::Scene const& s = h->s;
  if (s.pixelFilterKind == dmt_host::Scene::kNoPixelFilter) return 0;
  *kind = s.pixelFilterKind, *radius = s.pixelFilterRadius, *sigma = s.pixelFilterSigma;
  if (name && name_cap > 0) std::snprintf(name, size_t(name_cap), "%s", s.pixelFilterName.c_str());
  return s.pixelFilterKind == dmt_host::Scene::kUnsupportedPixelFilter ? 2 : 1;
}
// the scene's participating medium: 1 and the record (sigma_t, albedo3, g, min3, max3 -> out11), or 0 without one
int dmt_host_scene_medium(const dmt_host_scene* h, float* out11) {
  if (!h->s.hasMedium) return 0;
  out11[0] = h->s.mediumSigmaT, out11[4] = h->s.mediumG;
  for (int i = 0; i < 3; ++i) out11[1 + i] = h->s.mediumAlbedo[i], out11[5 + i] = h->s.mediumMin[i], out11[8 + i] = h->s.mediumMax[i];
  return 1;
}
// its spectrum: the extinction colour and the emission (out6); the defaults (1, 1, 1, 0, 0, 0) for a grey, dark medium
void dmt_host_scene_medium_spectrum(const dmt_host_scene* h, float* out6) {
  for (int i = 0; i < 3; ++i) out6[i] = h->s.mediumExtinction[i], out6[3 + i] = h->s.mediumEmission[i];
}
// its density grid: the nx * ny * nz values and dims3 = (nx, ny, nz), or null without one
const float* dmt_host_scene_medium_grid(const dmt_host_scene* h, int* dims3) {
  if (h->s.mediumGrid.empty()) return nullptr;
  for (int i = 0; i < 3; ++i) dims3[i] = h->s.mediumGridDims[i];
  return h->s.mediumGrid.data();
}
// readNpyGrid: the number of values and dims3 = (nx, ny, nz), the values into out when it is not null and cap holds them;
// -1 and the message in err on failure (the protocol of dmt_host_read_fbx)
int64_t dmt_host_read_npy_grid(const char* path, float* out, uint64_t cap, int* dims3, char* err, uint64_t err_cap) {
  std::vector<float> grid;
  std::string msg;
  int dims[3] = {0, 0, 0};
  if (!path || !readNpyGrid(path, grid, dims, &msg)) {
    if (err && err_cap) {
      size_t const n = msg.size() < err_cap - 1 ? msg.size() : size_t(err_cap - 1);
      memcpy(err, msg.data(), n);
      err[n] = 0;
    }
    return -1;
  }
  if (dims3)
    for (int i = 0; i < 3; ++i) dims3[i] = dims[i];
  if (out && cap >= grid.size()) memcpy(out, grid.data(), grid.size() * sizeof(float));
  return int64_t(grid.size());
}
void dmt_host_scene_set_resolution(dmt_host_scene* h, int width, int height) {
  h->s.camera.width = width, h->s.camera.height = height;
}
int dmt_host_scene_upload(const dmt_host_scene* h, dmt_ctx* ctx) { return uploadScene(ctx, h->s); }

// packers, one 32-byte record out
static void put(Packed32 const& p, void* out32) { memcpy(out32, p.bytes, 32); }
static Vec3 v(const float* p) { return {p[0], p[1], p[2]}; }
void dmt_host_make_lambert(void* out32) { put(makeLambert(), out32); }
void dmt_host_make_oren_nayar(const float* color3, float roughness, void* out32) { put(makeOrenNayar(v(color3), roughness), out32); }
void dmt_host_make_ggx_dielectric(const float* r3, const float* t3, float phi0, float eta, float ax, float ay, void* out32) {
  put(makeGGXDielectric(v(r3), v(t3), phi0, eta, ax, ay), out32);
}
void dmt_host_make_ggx_conductor(const float* eta3, const float* k3, float phi0, float ax, float ay, void* out32) {
  put(makeGGXConductor(v(eta3), v(k3), phi0, ax, ay), out32);
}
void dmt_host_make_point_light(const float* c3, const float* p3, float radius, void* out32) { put(makePointLight(v(c3), v(p3), radius), out32); }
void dmt_host_make_spot_light(const float* c3, const float* p3, const float* d3, float cos0, float cosE, float radius, void* out32) {
  put(makeSpotLight(v(c3), v(p3), v(d3), cos0, cosE, radius), out32);
}
void dmt_host_make_directional_light(const float* c3, const float* d3, float omc, void* out32) {
  put(makeDirectionalLight(v(c3), v(d3), omc), out32);
}
void dmt_host_make_environmental_light(const float* c3, void* out32) { put(makeEnvironmentalLight(v(c3)), out32); }
uint16_t dmt_host_float_to_half_bits(float f) { return float_to_half_bits(f); }
float dmt_host_half_bits_to_float(uint16_t h) { return half_bits_to_float(h); }

void dmt_host_film_to_rgb8(const float* mean4, const float* m24, uint64_t pixels, uint8_t* meanRgb, uint8_t* stdErrRgb) {
  filmToRgb8(mean4, m24, size_t(pixels), meanRgb, stdErrRgb);
}
int dmt_host_write_mean_and_mse(const float* mean4, const float* m24, uint32_t width, uint32_t height, const char* baseName) {
  return writeMeanAndMSERowMajor(mean4, m24, width, height, baseName) ? 0 : 1;
}
int dmt_host_write_pfm(const float* mean4, uint32_t width, uint32_t height, const char* path) {
  return writePfmRgb(path, mean4, width, height) ? 0 : 1;
}

}  // extern "C"
