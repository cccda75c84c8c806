// camera_host.hpp -- the host side of the camera layer (camera_state.hpp): the one-off camera and sampler set-up math, the
// host's camera ray, the pixel filter's table, the projections' host rays and inverses, and the dmt_* entry points of the
// camera, the film, the thin lens, the pixel filter and the projection.
//
// Part of dmt_hip.hip's translation unit, included once: after dmt_ctx, HIP_TRY and fail, and before accel_host.hpp,
// surface_host.hpp, denoise_host.hpp and probes.hpp, which use its set-up math (computeSamplerParams, cameraFromRaster,
// worldFromCamera) and the argument checks it shares with them (resolutionOk, haltonIndices).  The calls the other way are
// the three forward declarations below and dmt_test_closest_hit (probes.hpp), which dmt_hip.h declares.
#pragma once

namespace {

void textureFootprint(dmt_camera const& cam, float out[19]);  // surface_host.hpp
int checkErrorFlag(dmt_ctx* ctx);                              // launch_host.hpp
ProjXf makeProjXf(dmt_camera const& cam);                      // denoise_host.hpp

// ---- host math for the one-off camera / sampler setup (IEEE fp32, same expressions as the
// reference host code: CC/private/extra_math.cu:43-90, CC/private/common_math.cu:16-78,
// CC/private/rng.cu:21-46,182-208)
struct H3 {
  float x, y, z;
};
H3 hcross(H3 a, H3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
H3 hnormalize(H3 a) {
  float const inv = 1.0f / sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x * inv, a.y * inv, a.z * inv};
}
void worldFromCamera(float const dir[3], float const pos[3], float m[16]) {
  H3 const fwd = hnormalize({dir[0], dir[1], dir[2]});
  H3 const right = hnormalize(hcross(fwd, {0, 0, 1}));
  H3 const up = hcross(right, fwd);
  m[0] = right.x, m[4] = up.x, m[8] = fwd.x, m[12] = pos[0];
  m[1] = right.y, m[5] = up.y, m[9] = fwd.y, m[13] = pos[1];
  m[2] = right.z, m[6] = up.z, m[10] = fwd.z, m[14] = pos[2];
  m[3] = 0.f, m[7] = 0.f, m[11] = 0.f, m[15] = 1.f;
}
void cameraFromRaster(float focal_mm, float sensorH_mm, uint32_t xRes, uint32_t yRes, float m[16]) {
  float const sensorW_mm = sensorH_mm * float(xRes) / float(yRes);
  float const MM = 0.001f;
  float const focal = focal_mm * MM, sh = sensorH_mm * MM, sw = sensorW_mm * MM;
  float const psx = sw / float(xRes), psy = sh / float(yRes);
  float const tx = -0.5f * sw + 0.5f * psx;
  float const ty = 0.5f * sh - 0.5f * psy;
  for (int i = 0; i < 16; ++i) m[i] = 0.f;
  m[0] = psx, m[5] = -psy, m[10] = 1.f, m[12] = tx, m[13] = ty, m[14] = focal, m[15] = 1.f;
}
int64_t multInverse(int64_t a, int64_t n) {
  int64_t t = 0, nt = 1, r = n, nr = a;
  while (nr != 0) {
    int64_t const q = r / nr;
    int64_t tmp = t - q * nt;
    t = nt, nt = tmp;
    tmp = r - q * nr;
    r = nr, nr = tmp;
  }
  return t < 0 ? t + n : t;
}
SamplerParams computeSamplerParams(int width, int height) {
  SamplerParams p{};
  int const res[2] = {width, height};
  int32_t scale[2], ex[2];
  int const base[2] = {2, 3};
  for (int i = 0; i < 2; ++i) {
    scale[i] = 1, ex[i] = 0;
    int const lim = res[i] < 128 ? res[i] : 128;
    while (scale[i] < lim) scale[i] *= base[i], ++ex[i];
  }
  p.scale0 = scale[0], p.scale1 = scale[1], p.exp0 = ex[0], p.exp1 = ex[1];
  p.inv0 = int32_t(multInverse(scale[1], scale[0]));
  p.inv1 = int32_t(multInverse(scale[0], scale[1]));
  return p;
}
// both matrices of a camera: what dmt_set_camera keeps and the host-only calls make for themselves
CameraXf hostCameraXf(dmt_camera const& cam) {
  CameraXf xf{};
  cameraFromRaster(cam.focal_length, cam.sensor_size, uint32_t(cam.width), uint32_t(cam.height), xf.cfr);
  worldFromCamera(cam.dir, cam.pos, xf.rfc);
  return xf;
}

// ---- the argument checks the entry points share ----
bool resolutionOk(int width, int height) { return !(width <= 0 || height <= 0 || width > 65536 || height > 65536); }
// what dmt_set_lens takes: null, or why it refuses (as mediumArgsError)
char const* lensArgsError(float lens_radius, float focus_distance) {
  if (!std::isfinite(lens_radius) || lens_radius < 0.f) return "dmt_set_lens: the radius must be finite and >= 0";
  if (lens_radius > 0.f && !(std::isfinite(focus_distance) && focus_distance > 0.f)) return "dmt_set_lens: the focus distance must be finite and > 0";
  return nullptr;
}
// The Halton index of every (pixel, sample) of a host-only call, or false: outside the frame, or the sample overflows the
// 32-bit Halton index.  All of them are checked before the caller writes anything.
bool haltonIndices(SamplerParams const& sp, int width, int height, int n, int32_t const* pxs, int32_t const* pys, int32_t const* ss, std::vector<int32_t>& h) {
  int64_t const stride = int64_t(sp.scale0) * sp.scale1;
  h.resize(size_t(n));
  for (int i = 0; i < n; ++i) {
    if (pxs[i] < 0 || pys[i] < 0 || pxs[i] >= width || pys[i] >= height || ss[i] < 0 || (int64_t(ss[i]) + 1) * stride > 0x7FFFFFFFll) return false;
    h[size_t(i)] = halton_pixel_base(sp, pxs[i], pys[i]) + ss[i] * int32_t(stride);
  }
  return true;
}

// The host's camera ray through the continuous film position (fx, fy): camera_ray_jittered and camera_ray_lens in plain
// fp32 without contraction, with the host's division, square root, sine and cosine where the device has its own.
void hostCameraRay(CameraXf const& xf, float fx, float fy, float lensR, float focusD, LensU u, float* o3, float* d3) {
#pragma clang fp contract(off)
  float d[3];
  if (lensR > 0.f) {
    // sample_uniform_disk (pt_device.hpp), the reference's branches
    float const a = 2.f * u.x - 1.f, b = 2.f * u.y - 1.f;
    float lx = 0.f, ly = 0.f;
    if (!(a == 0.f && b == 0.f)) {
      float rho, phi;
      if (std::fabs(a) > std::fabs(b))
        rho = a, phi = (kPi / 4) * (b / a);
      else
        rho = b, phi = (3 * kPi / 4) * (a / b);
      lx = rho * std::cos(phi), ly = rho * std::sin(phi);
    }
    lens_ray_parts(xf.cfr, xf.rfc, fx, fy, focusD, lensR * lx, lensR * ly, o3, d);
  } else {  // xf_point / xf_dir of camera_ray_jittered (both matrices affine: w == 1)
    float const* const c = xf.cfr;
    float const* const m = xf.rfc;
    float const cx = c[0] * fx + c[4] * fy + c[8] * 0.0f + c[12];
    float const cy = c[1] * fx + c[5] * fy + c[9] * 0.0f + c[13];
    float const cz = c[2] * fx + c[6] * fy + c[10] * 0.0f + c[14];
    for (int i = 0; i < 3; ++i) {
      o3[i] = m[i] * 0.f + m[4 + i] * 0.f + m[8 + i] * 0.f + m[12 + i];
      d[i] = m[i] * cx + m[4 + i] * cy + m[8 + i] * cz;
    }
  }
  float const inv = 1.0f / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d3[0] = d[0] * inv, d3[1] = d[1] * inv, d3[2] = d[2] * inv;
}

// ---- projections ------------------------------------------------------------------------
// what dmt_set_projection takes: null, or why it refuses
char const* projectionArgsError(int kind, float param) {
  if (kind < DMT_PROJECTION_PERSPECTIVE || kind > DMT_PROJECTION_FISHEYE)
    return "dmt_set_projection: a kind DMT_PROJECTION_PERSPECTIVE .. DMT_PROJECTION_FISHEYE";
  if (kind == DMT_PROJECTION_ORTHOGRAPHIC && !(std::isfinite(param) && param > 0.f))
    return "dmt_set_projection: the orthographic view height must be finite and > 0";
  if (kind == DMT_PROJECTION_FISHEYE && !(std::isfinite(param) && param > 0.f && param <= 360.f))
    return "dmt_set_projection: the fisheye field of view must be finite, > 0 and <= 360 degrees";
  return nullptr;
}
// The host's ray through the film position (fx, fy) under a projection: camera_ray_projection's bodies with the host's
// sine, cosine, division and square root; perspective is hostCameraRay's pinhole ray.
void hostProjectionRay(dmt_camera const& cam, CameraXf const& xf, int kind, float a, float fx, float fy, float* o3, float* d3) {
#pragma clang fp contract(off)
  if (kind == DMT_PROJECTION_PERSPECTIVE) return hostCameraRay(xf, fx, fy, 0.f, 1.f, LensU{0.f, 0.f}, o3, d3);
  float const W = float(cam.width), H = float(cam.height);
  float d[3];
  if (kind == DMT_PROJECTION_ORTHOGRAPHIC) {
    ortho_ray_parts(xf.cfr, xf.rfc, fx, fy, a, o3, d);
  } else {
    float c[3];
    if (kind == DMT_PROJECTION_EQUIRECT) {
      float lon, lat;
      equirect_angles(fx, fy, W, H, lon, lat);
      equirect_dir(std::sin(lon), std::cos(lon), std::sin(lat), std::cos(lat), c);
    } else {
      float ux, uy, theta;
      fisheye_angle(fx, fy, W, H, a, ux, uy, theta);
      fisheye_dir(ux, uy, std::sin(theta), std::cos(theta), c);
    }
    angular_ray_parts(xf.rfc, c, o3, d);
  }
  float const inv = 1.0f / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d3[0] = d[0] * inv, d3[1] = d[1] * inv, d3[2] = d[2] * inv;
}

// ---- pixel filter ---------------------------------------------------------------------
// The filter's 1-D profile over w = x / radius in [-1, 1], integrated in float64 (each kind has a closed-form integral) and
// normalised to F(-1) = 0, F(1) = 1.  False for arguments dmt_set_pixel_filter refuses.
bool pixelFilterArgsOk(int kind, float radius, float param) {
  if (kind < DMT_FILTER_BOX || kind > DMT_FILTER_BLACKMAN_HARRIS) return false;
  if (!std::isfinite(radius) || !(radius > 0.f) || radius > 8.f) return false;
  if (kind == DMT_FILTER_GAUSSIAN && !(std::isfinite(param) && param > 0.f)) return false;
  return true;
}
double pixelFilterIntegral(int kind, double sigmaW, double w) {  // unnormalised, from -1 to w
  double const pi = 3.14159265358979323846;
  switch (kind) {
    case DMT_FILTER_TENT: return w <= 0.0 ? 0.5 * (1.0 + w) * (1.0 + w) : 1.0 - 0.5 * (1.0 - w) * (1.0 - w);
    case DMT_FILTER_GAUSSIAN: {  // max(0, G(w) - G(1)), pbrt-v4's; sigmaW = sigma / radius
      double const a = 1.0 / (sigmaW * std::sqrt(2.0));
      return sigmaW * std::sqrt(pi / 2.0) * (std::erf(a * w) + std::erf(a)) - std::exp(-0.5 / (sigmaW * sigmaW)) * (w + 1.0);
    }
    case DMT_FILTER_BLACKMAN_HARRIS: {  // the four-term window over t = (w + 1) / 2
      double const t = 0.5 * (w + 1.0);
      return 2.0 * (0.35875 * t - 0.48829 * std::sin(2.0 * pi * t) / (2.0 * pi) + 0.14128 * std::sin(4.0 * pi * t) / (4.0 * pi) -
                    0.01168 * std::sin(6.0 * pi * t) / (6.0 * pi));
    }
    default: return w + 1.0;  // box
  }
}
// The kFilterKnots knots W(i / 256) of the inverse CDF: bisection on the float64 integral for the lower half, mirrored for
// the upper one (the profiles are even), rounded to float32 once.  False when the profile has no mass in float64 (a Gaussian
// whose sigma is so far above the radius that G(w) - G(1) cancels).
bool pixelFilterKnots(int kind, float radius, float param, float* knots) {
  double const sigmaW = kind == DMT_FILTER_GAUSSIAN ? double(param) / double(radius) : 1.0;
  double const total = pixelFilterIntegral(kind, sigmaW, 1.0);
  if (!(total > 1e-12) || !std::isfinite(total)) return false;
  knots[0] = -1.f, knots[128] = 0.f, knots[256] = 1.f;
  for (int i = 1; i < 128; ++i) {
    double const target = total * (double(i) / 256.0);
    double lo = -1.0, hi = 0.0;
    for (int it = 0; it < 64; ++it) {
      double const mid = 0.5 * (lo + hi);
      (pixelFilterIntegral(kind, sigmaW, mid) < target ? lo : hi) = mid;
    }
    float k = float(0.5 * (lo + hi));
    if (k < knots[i - 1]) k = knots[i - 1];  // monotone after the rounding to float32
    knots[i] = k, knots[256 - i] = -k;
  }
  return true;
}
bool pixelFilterIsDefault(int kind, float radius) { return kind == DMT_FILTER_BOX && radius == 0.5f; }
// what filter_warp reads: per bin the knot and the fp32 difference to the next one
void pixelFilterBins(float const* knots, FilterBin* bins) {
#pragma clang fp contract(off)
  for (int i = 0; i < kFilterBins; ++i) bins[i] = FilterBin{knots[i], knots[i + 1] - knots[i]};
}

}  // namespace

extern "C" {

int dmt_set_camera(dmt_ctx* ctx, const dmt_camera* cam) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!cam || !resolutionOk(cam->width, cam->height)) return fail(ctx, DMT_ERR_INVALID, "dmt_set_camera: bad camera / resolution");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (cam->width != ctx->film.w || cam->height != ctx->film.h) {  // a new film, zeroed
    size_t const pixels = size_t(cam->width) * size_t(cam->height);
    FilmState film;
    film.w = cam->width, film.h = cam->height;
    HIP_TRY(ctx, film.ownMean.reserve(pixels));
    HIP_TRY(ctx, film.ownM2.reserve(pixels));
    film.mean = film.ownMean.get(), film.m2 = film.ownM2.get();
    HIP_TRY(ctx, film.clear(ctx->stream));
    ctx->film = std::move(film);
    ctx->dn.dropHistory();  // temporal history: it is of the old resolution
  }
  ctx->camera.cam = *cam;
  ctx->camera.xf = hostCameraXf(*cam);
  ctx->camera.sp = computeSamplerParams(cam->width, cam->height);
  textureFootprint(*cam, ctx->surf.texFoot);
  ctx->camera.have = true;
  return DMT_OK;
}

int dmt_film_clear(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->film.mean) return fail(ctx, DMT_ERR_STATE, "dmt_film_clear: no film (call dmt_set_camera first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->film.clear(ctx->stream));
  return DMT_OK;
}

int dmt_film_bind(dmt_ctx* ctx, void* d_mean, void* d_m2) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, "dmt_film_bind: call dmt_set_camera first");
  if (!d_mean || !d_m2) return fail(ctx, DMT_ERR_INVALID, "dmt_film_bind: null buffer");
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->film.ownMean.reset(), ctx->film.ownM2.reset();
  ctx->film.mean = static_cast<float4*>(d_mean);
  ctx->film.m2 = static_cast<float4*>(d_m2);
  return DMT_OK;
}

int dmt_film_device_ptrs(dmt_ctx* ctx, void** d_mean, void** d_m2) {
  if (!ctx || !d_mean || !d_m2) return DMT_ERR_INVALID;
  *d_mean = ctx->film.mean, *d_m2 = ctx->film.m2;
  return DMT_OK;
}

int dmt_download_film(dmt_ctx* ctx, float* mean4, float* m24) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->film.mean) return fail(ctx, DMT_ERR_STATE, "dmt_download_film: no film");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t const bytes = ctx->film.bytes();
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int const rc = checkErrorFlag(ctx)) return rc;
  if (mean4) HIP_TRY(ctx, hipMemcpy(mean4, ctx->film.mean, bytes, hipMemcpyDeviceToHost));
  if (m24) HIP_TRY(ctx, hipMemcpy(m24, ctx->film.m2, bytes, hipMemcpyDeviceToHost));
  return DMT_OK;
}

// ---- thin lens ------------------------------------------------------------------------
int dmt_set_lens(dmt_ctx* ctx, float lens_radius, float focus_distance) {
  if (!ctx) return DMT_ERR_INVALID;
  if (char const* const why = lensArgsError(lens_radius, focus_distance)) return fail(ctx, DMT_ERR_INVALID, why);
  if (lens_radius > 0.f && ctx->camera.projKind != DMT_PROJECTION_PERSPECTIVE)
    return fail(ctx, DMT_ERR_STATE, "dmt_set_lens: only the perspective camera has a lens (dmt_set_projection set another projection)");
  ctx->camera.lensR = lens_radius;
  if (lens_radius > 0.f) ctx->camera.lensD = focus_distance;  // radius 0: the distance is ignored
  return DMT_OK;
}

int dmt_lens_info(dmt_ctx* ctx, float* lens_radius, float* focus_distance) {
  if (!ctx) return DMT_ERR_INVALID;
  if (lens_radius) *lens_radius = ctx->camera.lensR;
  if (focus_distance) *focus_distance = ctx->camera.lensD;
  return DMT_OK;
}

int dmt_lens_rays(const dmt_camera* cam, float lens_radius, float focus_distance, int n, const int32_t* pxs, const int32_t* pys,
                  const int32_t* ss, float* o3, float* d3, float* lens2) {
  if (!cam || n < 0 || !resolutionOk(cam->width, cam->height)) return DMT_ERR_INVALID;
  if (n && (!pxs || !pys || !ss || !o3 || !d3 || !lens2)) return DMT_ERR_INVALID;
  if (lensArgsError(lens_radius, focus_distance)) return DMT_ERR_INVALID;
  CameraXf const xf = hostCameraXf(*cam);
  SamplerParams const sp = computeSamplerParams(cam->width, cam->height);
  std::vector<int32_t> hs;
  if (!haltonIndices(sp, cam->width, cam->height, n, pxs, pys, ss, hs)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    int32_t const h = hs[size_t(i)];
    LensU const u = lens_values(uint32_t(h));
    lens2[2 * size_t(i)] = u.x, lens2[2 * size_t(i) + 1] = u.y;
    f2 const r = pixel2d(sp, h);
    float const fx = ((r.x - 0.5f) + 0.5f) + float(pxs[i]);  // as camera_ray_jittered
    float const fy = ((r.y - 0.5f) + 0.5f) + float(pys[i]);
    hostCameraRay(xf, fx, fy, lens_radius, focus_distance, u, o3 + 3 * size_t(i), d3 + 3 * size_t(i));
  }
  return DMT_OK;
}

int dmt_focus_distance_at(dmt_ctx* ctx, float fx, float fy, float* distance) {
#pragma clang fp contract(off)
  if (!ctx || !distance || !std::isfinite(fx) || !std::isfinite(fy)) return DMT_ERR_INVALID;
  if (!(ctx->scene.haveTris && ctx->camera.have)) return fail(ctx, DMT_ERR_STATE, "dmt_focus_distance_at: upload triangles and set the camera first");
  if (ctx->camera.projKind != DMT_PROJECTION_PERSPECTIVE)
    return fail(ctx, DMT_ERR_STATE, "dmt_focus_distance_at: the autofocus ray is the pinhole's (dmt_set_projection set another projection)");
  float o[3], d[3];
  hostCameraRay(ctx->camera.xf, fx, fy, 0.f, 1.f, LensU{0.f, 0.f}, o, d);
  int32_t tri = -1;
  float t = 0.f;
  if (int const rc = dmt_test_closest_hit(ctx, 1, o, d, &tri, &t)) return rc;  // the context's accel mode; synchronous
  if (tri < 0) return fail(ctx, DMT_ERR_STATE, "dmt_focus_distance_at: the ray leaves the scene");
  float const* const m = ctx->camera.xf.rfc;  // column 2 = the viewing direction
  *distance = t * ((d[0] * m[8] + d[1] * m[9]) + d[2] * m[10]);
  return DMT_OK;
}

// ---- projections ------------------------------------------------------------------------
int dmt_set_projection(dmt_ctx* ctx, int kind, float param) {
  if (!ctx) return DMT_ERR_INVALID;
  if (char const* const why = projectionArgsError(kind, param)) return fail(ctx, DMT_ERR_INVALID, why);
  if (kind != DMT_PROJECTION_PERSPECTIVE && ctx->camera.lensR > 0.f)
    return fail(ctx, DMT_ERR_STATE, "dmt_set_projection: a thin lens (dmt_set_lens, radius > 0) is set; only the perspective camera has one");
  ctx->camera.projKind = kind;
  ctx->camera.projParam = (kind == DMT_PROJECTION_ORTHOGRAPHIC || kind == DMT_PROJECTION_FISHEYE) ? param : 0.f;
  return DMT_OK;
}

int dmt_projection_info(dmt_ctx* ctx, int* kind, float* param) {
  if (!ctx) return DMT_ERR_INVALID;
  if (kind) *kind = ctx->camera.projKind;
  if (param) *param = ctx->camera.projParam;
  return DMT_OK;
}

int dmt_projection_rays(const dmt_camera* cam, int kind, float param, int n, const float* xy2, float* o3, float* d3) {
  if (!cam || n < 0 || !resolutionOk(cam->width, cam->height) || projectionArgsError(kind, param)) return DMT_ERR_INVALID;
  if (n && (!xy2 || !o3 || !d3)) return DMT_ERR_INVALID;
  CameraXf const xf = hostCameraXf(*cam);
  float const a = projectionFactor(*cam, kind, param);
  for (int i = 0; i < n; ++i)
    hostProjectionRay(*cam, xf, kind, a, xy2[2 * size_t(i)], xy2[2 * size_t(i) + 1], o3 + 3 * size_t(i), d3 + 3 * size_t(i));
  return DMT_OK;
}

int dmt_projection_project(const dmt_camera* cam, int kind, float param, int n, const float* p3, float* xy2, float* depth) {
#pragma clang fp contract(off)
  if (!cam || n < 0 || !resolutionOk(cam->width, cam->height) || projectionArgsError(kind, param)) return DMT_ERR_INVALID;
  if (n && (!p3 || !xy2 || !depth)) return DMT_ERR_INVALID;
  if (kind == DMT_PROJECTION_PERSPECTIVE) return dmt_camera_project(cam, n, p3, xy2, depth);
  ProjXf const c = makeProjXf(*cam);
  float const a = projectionFactor(*cam, kind, param);
  float const W = float(cam->width), H = float(cam->height);
  for (int i = 0; i < n; ++i) {
    float const dx = p3[3 * size_t(i)] - c.pos[0], dy = p3[3 * size_t(i) + 1] - c.pos[1], dz = p3[3 * size_t(i) + 2] - c.pos[2];
    float const cx = (c.right[0] * dx + c.right[1] * dy) + c.right[2] * dz;  // camera space, as project_point
    float const cy = (c.up[0] * dx + c.up[1] * dy) + c.up[2] * dz;
    float const cz = (c.fwd[0] * dx + c.fwd[1] * dy) + c.fwd[2] * dz;
    float fx, fy, dep;
    if (kind == DMT_PROJECTION_ORTHOGRAPHIC) {
      fx = (cx / a - c.tx) * c.ipx, fy = (cy / a - c.ty) * c.ipy, dep = cz;
    } else if (kind == DMT_PROJECTION_EQUIRECT) {
      float const lon = std::atan2(cx, cz), lat = std::atan2(cy, std::hypot(cx, cz));
      fx = (lon / (2.0f * kPi) + 0.5f) * W, fy = (0.5f - lat / kPi) * H;
      dep = std::sqrt((cx * cx + cy * cy) + cz * cz);
    } else {
      float const rho = std::hypot(cx, cy);
      float const r = std::atan2(rho, cz) / a;  // theta / s, in pixels
      float const ux = rho > 0.f ? cx / rho : 0.f, uy = rho > 0.f ? cy / rho : 0.f;
      fx = 0.5f * W + r * ux, fy = 0.5f * H - r * uy;
      dep = std::sqrt((cx * cx + cy * cy) + cz * cz);
    }
    xy2[2 * size_t(i)] = fx, xy2[2 * size_t(i) + 1] = fy, depth[i] = dep;
  }
  return DMT_OK;
}

// ---- pixel filter ---------------------------------------------------------------------
int dmt_pixel_filter_table(int kind, float radius, float param, float* knots257) {
  if (!knots257 || !pixelFilterArgsOk(kind, radius, param)) return DMT_ERR_INVALID;
  return pixelFilterKnots(kind, radius, param, knots257) ? DMT_OK : DMT_ERR_INVALID;
}

int dmt_set_pixel_filter(dmt_ctx* ctx, int kind, float radius, float param) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!pixelFilterArgsOk(kind, radius, param))
    return fail(ctx, DMT_ERR_INVALID,
                "dmt_set_pixel_filter: a kind DMT_FILTER_BOX .. DMT_FILTER_BLACKMAN_HARRIS, a finite radius in (0, 8], and for the Gaussian a finite sigma > 0");
  if (!pixelFilterIsDefault(kind, radius)) {
    float knots[kFilterKnots];
    if (!pixelFilterKnots(kind, radius, param, knots))
      return fail(ctx, DMT_ERR_INVALID, "dmt_set_pixel_filter: the Gaussian's sigma is too large for its radius (the profile has no mass)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a launch in flight may still read the old table
    FilterBin bins[kFilterBins];
    pixelFilterBins(knots, bins);
    HIP_TRY(ctx, ctx->camera.filt.knots.assign(bins, kFilterBins));
  }
  ctx->camera.filt.kind = kind, ctx->camera.filt.radius = radius, ctx->camera.filt.param = kind == DMT_FILTER_GAUSSIAN ? param : 0.f;
  ctx->camera.filt.active = !pixelFilterIsDefault(kind, radius);
  return DMT_OK;
}

int dmt_pixel_filter_info(dmt_ctx* ctx, int* kind, float* radius, float* param, int* active) {
  if (!ctx) return DMT_ERR_INVALID;
  if (kind) *kind = ctx->camera.filt.kind;
  if (radius) *radius = ctx->camera.filt.radius;
  if (param) *param = ctx->camera.filt.param;
  if (active) *active = ctx->camera.filt.active ? 1 : 0;
  return DMT_OK;
}

int dmt_pixel_filter_positions(int width, int height, int kind, float radius, float param, int n, const int32_t* pxs, const int32_t* pys,
                               const int32_t* ss, float* xy2) {
  if (n < 0 || !resolutionOk(width, height) || !pixelFilterArgsOk(kind, radius, param)) return DMT_ERR_INVALID;
  if (n && (!pxs || !pys || !ss || !xy2)) return DMT_ERR_INVALID;
  float knots[kFilterKnots];
  bool const active = !pixelFilterIsDefault(kind, radius);
  if (active && !pixelFilterKnots(kind, radius, param, knots)) return DMT_ERR_INVALID;
  FilterBin bins[kFilterBins];
  if (active) pixelFilterBins(knots, bins);
  SamplerParams const sp = computeSamplerParams(width, height);
  std::vector<int32_t> hs;
  if (!haltonIndices(sp, width, height, n, pxs, pys, ss, hs)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    f2 r = pixel2d(sp, hs[size_t(i)]);
    if (active) r = f2{filter_warp(bins, radius, r.x), filter_warp(bins, radius, r.y)};
    xy2[2 * size_t(i)] = film_coord(r.x, pxs[i]), xy2[2 * size_t(i) + 1] = film_coord(r.y, pys[i]);
  }
  return DMT_OK;
}

}  // extern "C"
