// denoise_host.hpp -- the host side of the image-space layer (denoise.hpp): the dmt_* entry points of the feature pass, the
// a-trous filter and temporal accumulation, and the rules that keep the temporal history and its raw-vertex mirror valid.
//
// Part of dmt_hip.hip's translation unit, included once after the host helpers it uses (dmt_ctx, HIP_TRY, fail, baseParams,
// checkErrorFlag; camera_host.hpp's cameraFromRaster and worldFromCamera; accel_host.hpp's requireTree, reserveOverflow,
// motionParams; surface_host.hpp's firstHitVariant; SceneState::matIdOutside) and before the first entry point that calls
// into it.  accel_host.hpp forward-declares the two mirror calls below for its vertex updates.
// The rest of the library reaches DenoiseState through dropHistory / dropVertexMirror and the two mirror calls below.
#pragma once

namespace {
// temporal accumulation: the raw vertices of the current soup, 9 floats per triangle, from the host copy.  The caller has
// drained the stream (a kernel in flight may read the array)
int uploadRawVertices(dmt_ctx* ctx) {
  size_t const n = ctx->scene.triCount;
  std::vector<float> v(9 * n);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < 3; ++k)
      v[9 * i + 3 * k] = ctx->scene.h_xs[4 * i + k], v[9 * i + 3 * k + 1] = ctx->scene.h_ys[4 * i + k], v[9 * i + 3 * k + 2] = ctx->scene.h_zs[4 * i + k];
  HIP_TRY(ctx, ctx->dn.tvCur.assign(v.data(), v.size()));
  ctx->dn.tvValid = true;
  return DMT_OK;
}
// before an update overwrites tvCur: the first update after the history's frame moves that frame's vertices to tvPrev
// (beginUpdate has drained the stream).  wait: the overwrite is a host copy, not a launch on the stream.  Without a history
// there is no such frame
int keepHistoryVertices(dmt_ctx* ctx, bool wait) {
  if (!ctx->dn.tvPrevIsCur || !ctx->dn.thValid) return DMT_OK;
  size_t const n = 9 * size_t(ctx->scene.triCount);
  HIP_TRY(ctx, ctx->dn.tvPrev.reserve(n ? n : 1));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->dn.tvPrev.get(), ctx->dn.tvCur.get(), n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  if (wait) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->dn.tvPrevIsCur = false;
  return DMT_OK;
}
// The mirror's half of the two vertex updates; both do nothing unless the mirror is live.  Host path: tvCur again from the
// host copy, which holds the new positions
bool mirrorLive(dmt_ctx const* ctx) { return ctx->dn.temporalOn && ctx->dn.tvValid; }
int mirrorHostUpdate(dmt_ctx* ctx) {
  if (!mirrorLive(ctx)) return DMT_OK;
  if (int const rc = keepHistoryVertices(ctx, true)) return rc;
  return uploadRawVertices(ctx);
}
// device path: the caller's array has the layout of tvCur; the copy is ordered behind the snapshot on the context's stream
int mirrorDeviceUpdate(dmt_ctx* ctx, void const* d_verts9, size_t count) {
  if (!mirrorLive(ctx)) return DMT_OK;
  if (int const rc = keepHistoryVertices(ctx, false)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->dn.tvCur.get(), d_verts9, count * 9 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return DMT_OK;
}

ProjXf makeProjXf(dmt_camera const& cam) {
  float cf[16], rf[16];
  cameraFromRaster(cam.focal_length, cam.sensor_size, uint32_t(cam.width), uint32_t(cam.height), cf);
  worldFromCamera(cam.dir, cam.pos, rf);
  ProjXf c{};
  for (int a = 0; a < 3; ++a) c.right[a] = rf[a], c.up[a] = rf[4 + a], c.fwd[a] = rf[8 + a], c.pos[a] = rf[12 + a];
  c.focal = cf[14], c.tx = cf[12], c.ty = cf[13];
  c.ipx = 1.0f / cf[0], c.ipy = 1.0f / cf[5];
  return c;
}
// the first temporal call, a new resolution, a new soup: the history's planes and the current raw vertices
int prepareHistory(dmt_ctx* ctx, size_t pixels) {
  if (ctx->dn.thW != ctx->film.w || ctx->dn.thH != ctx->film.h) ctx->dn.dropHistory();
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(ctx, ctx->dn.histCv[i].reserve(pixels));
    HIP_TRY(ctx, ctx->dn.histLen[i].reserve(pixels));
  }
  HIP_TRY(ctx, ctx->dn.histNormal.reserve(pixels));
  HIP_TRY(ctx, ctx->dn.histPos.reserve(pixels));
  HIP_TRY(ctx, ctx->dn.counts.reserve(2));
  ctx->dn.thW = ctx->film.w, ctx->dn.thH = ctx->film.h;
  if (!ctx->dn.tvValid) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int const rc = uploadRawVertices(ctx)) return rc;  // the soup is new: dropVertexMirror has dropped the history
  }
  ctx->dn.temporalOn = true;
  return DMT_OK;
}

// k_denoise_init (validation + pass-0 planes), then `iterations` k_atrous passes ping-ponging between two planes.  tp (the
// temporal form): k_temporal between the two blends the pass-0 plane with the reprojected history into the new history,
// which pass 0 then reads in place
int denoiseRun(dmt_ctx* ctx, char const* name, const dmt_denoise_params* params, const dmt_temporal_params* tp, const float* mean4,
               const float* m24, float* out4, float* kernel_ms) {
  if (!ctx) return DMT_ERR_INVALID;
  if (kernel_ms) *kernel_ms = 0.f;
  dmt_denoise_params const p = params ? *params : dmt_denoise_defaults();
  std::string const pre = std::string(name) + ": ";
  auto failn = [&](int code, char const* msg) { return fail(ctx, code, (pre + msg).c_str()); };
  if (!out4 || (mean4 == nullptr) != (m24 == nullptr)) return failn(DMT_ERR_INVALID, "out4 is required, and mean4 / m24 come both or not at all");
  if (p.iterations < 0 || p.iterations > 10) return failn(DMT_ERR_INVALID, "iterations must be 0 .. 10");
  auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  if (!positive(p.sigma_normal) || !positive(p.sigma_position) || !positive(p.sigma_albedo) || !positive(p.sigma_luminance))
    return failn(DMT_ERR_INVALID, "every sigma must be finite and > 0");
  if (tp && (!(tp->alpha >= 0.f && tp->alpha <= 1.f) || !std::isfinite(tp->normal_threshold) || !positive(tp->plane_threshold)))
    return failn(DMT_ERR_INVALID, "alpha must be 0 .. 1, normal_threshold finite, plane_threshold finite and > 0");
  if (!ctx->camera.have) return failn(DMT_ERR_STATE, "set the camera first");
  if (ctx->camera.projKind != DMT_PROJECTION_PERSPECTIVE)  // before anything is touched: the history stays as it was
    return failn(DMT_ERR_STATE, "the depth scale and the reprojection are the perspective camera's (dmt_set_projection set another projection)");
  if (ctx->dn.aovW == 0) return failn(DMT_ERR_STATE, "no AOVs (call dmt_render_aovs or dmt_upload_aovs first)");
  if (ctx->dn.aovW != ctx->film.w || ctx->dn.aovH != ctx->film.h) {
    char msg[160];
    snprintf(msg, sizeof(msg), "the AOVs are %d x %d, the film %d x %d", ctx->dn.aovW, ctx->dn.aovH, ctx->film.w, ctx->film.h);
    return failn(DMT_ERR_STATE, msg);
  }
  if (tp && !ctx->dn.aovSurface) return failn(DMT_ERR_STATE, "no surface plane (call dmt_render_aovs, or dmt_upload_aov_surface after dmt_upload_aovs)");
  if (tp && !ctx->scene.haveTris) return failn(DMT_ERR_STATE, "upload triangles first");
  if (tp && ctx->scene.triCount > (1u << 24)) return failn(DMT_ERR_STATE, "more than 2^24 triangles: the surface plane's float index is not exact");
  if (!mean4 && !ctx->film.mean) return failn(DMT_ERR_STATE, "no film");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t const pixels = size_t(ctx->film.w) * size_t(ctx->film.h);
  float4 const* mean = ctx->film.mean;
  float4 const* m2 = ctx->film.m2;
  if (mean4) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, ctx->dn.film.reserve(2 * pixels));
    HIP_TRY(ctx, hipMemcpy(ctx->dn.film.get(), mean4, pixels * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dn.film.get() + pixels, m24, pixels * sizeof(float4), hipMemcpyHostToDevice));
    mean = ctx->dn.film.get(), m2 = ctx->dn.film.get() + pixels;
  }
  HIP_TRY(ctx, ctx->dn.cv.reserve(2 * pixels));
  HIP_TRY(ctx, ctx->dn.bad.reserve(1));
  if (tp)
    if (int const rc = prepareHistory(ctx, pixels)) return rc;
  float4* const cv[2] = {ctx->dn.cv.get(), ctx->dn.cv.get() + pixels};
  DenoiseArgs A{};
  A.mean = mean, A.m2 = m2, A.albedo = ctx->dn.albedo.get(), A.normal = ctx->dn.normal.get(), A.position = ctx->dn.pos.get();
  A.bad = ctx->dn.bad.get(), A.width = ctx->film.w, A.height = ctx->film.h;
  A.theta = ctx->camera.cam.sensor_size / (ctx->camera.cam.focal_length * float(ctx->camera.cam.height));
  A.sigmaN = p.sigma_normal, A.sigmaX = p.sigma_position, A.sigmaA = p.sigma_albedo, A.sigmaL = p.sigma_luminance;
  EventPair ev, evT;
  HIP_TRY(ctx, hipEventCreate(&ev.a));
  HIP_TRY(ctx, hipEventCreate(&ev.b));
  HIP_TRY(ctx, hipMemsetAsync(A.bad, 0, sizeof(uint32_t), ctx->stream));
  if (tp) {
    HIP_TRY(ctx, hipEventCreate(&evT.a));
    HIP_TRY(ctx, hipEventCreate(&evT.b));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dn.counts.get(), 0, 2 * sizeof(uint32_t), ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ev.a, ctx->stream));
  A.dst = cv[0];
  hipLaunchKernelGGL(k_denoise_init, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  dim3 const grid(uint32_t((ctx->film.w + 63) / 64), uint32_t((ctx->film.h + 3) / 4));
  int const slotNew = ctx->dn.thSlot ^ 1;
  ProjXf const camCur = tp ? makeProjXf(ctx->camera.cam) : ProjXf{};
  if (tp) {
    TemporalArgs T{};
    T.cur = cv[0], T.albedo = A.albedo, T.normal = A.normal, T.surface = ctx->dn.surface.get();
    T.vertsCur = ctx->dn.tvCur.get(), T.vertsPrev = ctx->dn.tvPrevIsCur ? ctx->dn.tvCur.get() : ctx->dn.tvPrev.get();
    T.histCv = ctx->dn.histCv[ctx->dn.thSlot].get(), T.histLen = ctx->dn.histLen[ctx->dn.thSlot].get();
    T.histNormal = ctx->dn.histNormal.get(), T.histPos = ctx->dn.histPos.get();
    T.outCv = ctx->dn.histCv[slotNew].get(), T.outLen = ctx->dn.histLen[slotNew].get();
    T.counts = ctx->dn.counts.get();
    T.camCur = camCur, T.camPrev = ctx->dn.thValid ? ctx->dn.thCam : camCur;
    T.width = ctx->film.w, T.height = ctx->film.h, T.triCount = ctx->scene.triCount, T.haveHistory = ctx->dn.thValid ? 1 : 0;
    T.alpha = tp->alpha, T.normalThreshold = tp->normal_threshold, T.planeThreshold = tp->plane_threshold;
    T.thetaPrev = ctx->dn.thValid ? ctx->dn.thTheta : A.theta;
    HIP_TRY(ctx, hipEventRecord(evT.a, ctx->stream));
    hipLaunchKernelGGL(k_temporal, grid, dim3(256), 0, ctx->stream, T);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(evT.b, ctx->stream));
  }
  float4 const* result = tp ? ctx->dn.histCv[slotNew].get() : cv[0];
  for (int i = 0; i < p.iterations; ++i) {
    A.src = result, A.dst = cv[(i + 1) & 1], A.step = 1 << i;
    for (int dy = -2; dy <= 2; ++dy)
      for (int dx = -2; dx <= 2; ++dx) A.tapDist[5 * (dy + 2) + dx + 2] = float(A.step) * std::sqrt(float(dx * dx + dy * dy));
    hipLaunchKernelGGL(k_atrous, grid, dim3(256), 0, ctx->stream, A);
    HIP_TRY(ctx, hipGetLastError());
    result = A.dst;
  }
  HIP_TRY(ctx, hipEventRecord(ev.b, ctx->stream));
  uint32_t bad = 0, counts[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(&bad, A.bad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
  if (tp) HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->dn.counts.get(), sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!mean4)
    if (int const rc = checkErrorFlag(ctx)) return rc;
  if (bad) {
    char msg[400];
    snprintf(msg, sizeof(msg), "%u pixel(s) have fewer than 2 samples or a non-finite mean / M2%s", bad,
             !mean4 && ctx->launch.world > 1 ? " (this context renders only the tiles of its dmt_set_partition rank: combine the ranks' "
                                        "films and pass the combined film as mean4 / m24)" : "");
    return failn(DMT_ERR_STATE, msg);
  }
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
  if (kernel_ms) *kernel_ms = ms;
  HIP_TRY(ctx, hipMemcpy(out4, result, pixels * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < pixels; ++i) out4[4 * i + 3] = 1.f;
  if (tp) {  // the call succeeded: its plane, its AOVs, its camera and its vertices become the history
    float msT = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&msT, evT.a, evT.b));
    HIP_TRY(ctx, hipMemcpy(ctx->dn.histNormal.get(), ctx->dn.normal.get(), pixels * sizeof(float4), hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dn.histPos.get(), ctx->dn.pos.get(), pixels * sizeof(float4), hipMemcpyDeviceToDevice));
    ctx->dn.thSlot = slotNew, ctx->dn.thValid = true, ctx->dn.tvPrevIsCur = true;
    ctx->dn.thCam = camCur, ctx->dn.thTheta = A.theta;
    ctx->dn.thRecord.frames += 1, ctx->dn.thRecord.reprojected = counts[0], ctx->dn.thRecord.reset = counts[1], ctx->dn.thRecord.temporal_ms = msT;
  }
  return DMT_OK;
}
}  // namespace

extern "C" {

// ---- denoiser ------------------------------------------------------------------
dmt_denoise_params dmt_denoise_defaults(void) {
  dmt_denoise_params p;
  p.iterations = 4, p.sigma_normal = 128.f, p.sigma_position = 1.f, p.sigma_albedo = 0.1f, p.sigma_luminance = 32.f;
  return p;
}

int dmt_render_aovs(dmt_ctx* ctx, uint32_t aov_spp) {
  if (!ctx) return DMT_ERR_INVALID;
  if (aov_spp == 0 || aov_spp > 65536u) return fail(ctx, DMT_ERR_INVALID, "dmt_render_aovs: aov_spp must be 1 .. 65536");
  if (!(ctx->scene.haveTris && ctx->scene.haveBsdfs && ctx->camera.have))
    return fail(ctx, DMT_ERR_STATE, "dmt_render_aovs: upload triangles, bsdfs and set the camera first");
  if (ctx->scene.matIdOutside())
    return fail(ctx, DMT_ERR_INVALID, "dmt_render_aovs: material index outside the BSDF array");
  if (!ctx->surf.texturesMatch(ctx->scene.bsdfCount, ctx->scene.triCount))
    return fail(ctx, DMT_ERR_STATE, "dmt_render_aovs: texture tables do not match the uploaded BSDFs / triangles (upload textures last)");
  int variant = 0;
  if (int const rcV = firstHitVariant(ctx, "dmt_render_aovs", &variant)) return rcV;
  bool const useBvh = ctx->accel == DMT_ACCEL_BVH;
  if (int const rcT = useBvh ? requireTree(ctx, "dmt_render_aovs") : DMT_OK) return rcT;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t const pixels = size_t(ctx->film.w) * size_t(ctx->film.h);
  ctx->dn.aovW = ctx->dn.aovH = 0;  // no AOVs unless this call succeeds
  ctx->dn.aovSurface = false;
  HIP_TRY(ctx, ctx->dn.albedo.reserve(pixels));
  HIP_TRY(ctx, ctx->dn.normal.reserve(pixels));
  HIP_TRY(ctx, ctx->dn.pos.reserve(pixels));
  HIP_TRY(ctx, ctx->dn.surface.reserve(pixels));
  // a grid of a few 256-lane blocks per CU strides over the frame: the BVH overflow stack is sized by the launch's lanes
  size_t const blocks = std::min((pixels + 255) / 256, size_t(std::max(ctx->launch.cuCount, 1)) * 8);
  size_t const threads = blocks * 256;
  if (useBvh) HIP_TRY(ctx, reserveOverflow(ctx, threads));
  AovArgs A{};
  A.albedo = ctx->dn.albedo.get(), A.normal = ctx->dn.normal.get(), A.position = ctx->dn.pos.get();
  A.surface = ctx->dn.surface.get();
  A.width = ctx->film.w, A.pixels = uint32_t(pixels), A.aovSpp = aov_spp, A.useBvh = useBvh;
  RenderParams P = baseParams(ctx, threads);
  uint32_t const motionMask = ctx->ac.haveMotion ? kFeatMotion | (useBvh ? kFeatBvh : 0u) : 0u;  // the samples' times, as the film's rows
  if (int const rcM = motionParams(ctx, motionMask, P)) return rcM;
  decltype(&k_aov) const kernels[4] = {k_aov, k_aov_vn, k_aov_motion, k_aov_cut};  // by firstHitVariant
  hipLaunchKernelGGL(kernels[variant], dim3(uint32_t(blocks)), dim3(256), 0, ctx->stream, P, A);
  HIP_TRY(ctx, hipGetLastError());
  ctx->dn.aovW = ctx->film.w, ctx->dn.aovH = ctx->film.h;
  ctx->dn.aovSurface = true;
  return DMT_OK;
}

int dmt_upload_aovs(dmt_ctx* ctx, const float* albedo4, const float* normal4, const float* position4, int width, int height) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!albedo4 || !normal4 || !position4 || width <= 0 || height <= 0)
    return fail(ctx, DMT_ERR_INVALID, "dmt_upload_aovs: three planes of a positive size");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a feature pass in flight writes the same planes
  size_t const pixels = size_t(width) * size_t(height);
  ctx->dn.aovW = ctx->dn.aovH = 0;
  ctx->dn.aovSurface = false;  // the surface plane is uploaded after these (dmt_upload_aov_surface)
  HIP_TRY(ctx, ctx->dn.albedo.assign(albedo4, pixels));
  HIP_TRY(ctx, ctx->dn.normal.assign(normal4, pixels));
  HIP_TRY(ctx, ctx->dn.pos.assign(position4, pixels));
  ctx->dn.aovW = width, ctx->dn.aovH = height;
  return DMT_OK;
}

int dmt_download_aovs(dmt_ctx* ctx, float* albedo4, float* normal4, float* position4) {
  if (!ctx) return DMT_ERR_INVALID;
  if (ctx->dn.aovW == 0) return fail(ctx, DMT_ERR_STATE, "dmt_download_aovs: no AOVs (call dmt_render_aovs or dmt_upload_aovs first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  size_t const bytes = size_t(ctx->dn.aovW) * size_t(ctx->dn.aovH) * sizeof(float4);
  if (albedo4) HIP_TRY(ctx, hipMemcpy(albedo4, ctx->dn.albedo.get(), bytes, hipMemcpyDeviceToHost));
  if (normal4) HIP_TRY(ctx, hipMemcpy(normal4, ctx->dn.normal.get(), bytes, hipMemcpyDeviceToHost));
  if (position4) HIP_TRY(ctx, hipMemcpy(position4, ctx->dn.pos.get(), bytes, hipMemcpyDeviceToHost));
  return DMT_OK;
}

int dmt_denoise(dmt_ctx* ctx, const dmt_denoise_params* params, const float* mean4, const float* m24, float* out4, float* kernel_ms) {
  return denoiseRun(ctx, "dmt_denoise", params, nullptr, mean4, m24, out4, kernel_ms);
}

// ---- temporal accumulation ---------------------------------------------------------
dmt_temporal_params dmt_temporal_defaults(void) {
  dmt_temporal_params p;
  p.alpha = 0.2f, p.normal_threshold = 0.9f, p.plane_threshold = 2.f;
  return p;
}

int dmt_denoise_temporal(dmt_ctx* ctx, const dmt_denoise_params* params, const dmt_temporal_params* tparams, const float* mean4,
                         const float* m24, float* out4, float* kernel_ms) {
  dmt_temporal_params const tp = tparams ? *tparams : dmt_temporal_defaults();
  return denoiseRun(ctx, "dmt_denoise_temporal", params, &tp, mean4, m24, out4, kernel_ms);
}

int dmt_temporal_reset(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  ctx->dn.dropHistory();
  return DMT_OK;
}

int dmt_temporal_info(dmt_ctx* ctx, dmt_temporal_record* out) {
  if (!ctx || !out) return DMT_ERR_INVALID;
  *out = ctx->dn.thRecord;
  out->history_bytes = ctx->dn.historyBytes();
  return DMT_OK;
}

int dmt_temporal_download(dmt_ctx* ctx, float* color_var4, float* length1) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!ctx->dn.thValid) return fail(ctx, DMT_ERR_STATE, "dmt_temporal_download: no history (call dmt_denoise_temporal first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  size_t const pixels = size_t(ctx->dn.thW) * size_t(ctx->dn.thH);
  if (color_var4) HIP_TRY(ctx, hipMemcpy(color_var4, ctx->dn.histCv[ctx->dn.thSlot].get(), pixels * sizeof(float4), hipMemcpyDeviceToHost));
  if (length1) HIP_TRY(ctx, hipMemcpy(length1, ctx->dn.histLen[ctx->dn.thSlot].get(), pixels * sizeof(float), hipMemcpyDeviceToHost));
  return DMT_OK;
}

int dmt_download_aov_surface(dmt_ctx* ctx, float* surface4) {
  if (!ctx || !surface4) return DMT_ERR_INVALID;
  if (ctx->dn.aovW == 0 || !ctx->dn.aovSurface) return fail(ctx, DMT_ERR_STATE, "dmt_download_aov_surface: no surface plane (call dmt_render_aovs or dmt_upload_aov_surface first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(surface4, ctx->dn.surface.get(), size_t(ctx->dn.aovW) * size_t(ctx->dn.aovH) * sizeof(float4), hipMemcpyDeviceToHost));
  return DMT_OK;
}

int dmt_upload_aov_surface(dmt_ctx* ctx, const float* surface4, int width, int height) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!surface4 || width <= 0 || height <= 0) return fail(ctx, DMT_ERR_INVALID, "dmt_upload_aov_surface: a plane of a positive size");
  if (width != ctx->dn.aovW || height != ctx->dn.aovH)
    return fail(ctx, DMT_ERR_STATE, "dmt_upload_aov_surface: the plane must have the size of the context's AOVs (upload or render those first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->dn.aovSurface = false;
  HIP_TRY(ctx, ctx->dn.surface.assign(surface4, size_t(width) * size_t(height)));
  ctx->dn.aovSurface = true;
  return DMT_OK;
}

int dmt_camera_project(const dmt_camera* cam, int n, const float* p3, float* xy2, float* depth) {
  if (!cam || n < 0 || (n && (!p3 || !xy2 || !depth)) || cam->width <= 0 || cam->height <= 0) return DMT_ERR_INVALID;
  ProjXf const c = makeProjXf(*cam);
  for (int i = 0; i < n; ++i) {
    Proj const o = project_point(c, p3[3 * size_t(i)], p3[3 * size_t(i) + 1], p3[3 * size_t(i) + 2]);
    xy2[2 * size_t(i)] = o.fx, xy2[2 * size_t(i) + 1] = o.fy, depth[i] = o.depth;
  }
  return DMT_OK;
}

}  // extern "C"
