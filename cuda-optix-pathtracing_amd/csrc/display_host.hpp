// display_host.hpp -- the host side of the display transform (display.hpp): the parameter check, the metering
// of the histogram, the launch sequence, and the dmt_display* entry points with their host-only twins.
//
// Part of dmt_hip.hip's translation unit, included once after denoise_host.hpp.  It uses dmt_ctx, HIP_TRY and fail; of the
// rest of the context it reads the camera's size, the film's mean pointer, the stream, the CU count and the partition's
// world, and writes DisplayState only.
#pragma once

namespace {

// what dmt_display refuses of its parameters: the message, or null.  `white` 0 stands for the curve's default
char const* displayParamsError(dmt_display_params const& p) {
  if (!std::isfinite(p.exposure_ev) || !std::isfinite(p.key) || !std::isfinite(p.low_fraction) || !std::isfinite(p.high_fraction) ||
      !std::isfinite(p.bloom_strength) || !std::isfinite(p.white))
    return "a parameter is not finite";
  if (!(p.key > 0.f)) return "key must be > 0";
  if (p.low_fraction < 0.f || p.low_fraction >= 1.f || p.high_fraction < 0.f || p.high_fraction >= 1.f ||
      double(p.low_fraction) + double(p.high_fraction) >= 1.0)
    return "low_fraction and high_fraction must be in [0, 1) and sum to less than 1";
  if (p.bloom_levels < 0 || p.bloom_levels > 8) return "bloom_levels must be 0 .. 8";
  if (p.bloom_strength < 0.f || p.bloom_strength > 1.f) return "bloom_strength must be 0 .. 1";
  if (p.tone < DMT_TONE_LINEAR || p.tone > DMT_TONE_HABLE) return "unknown tone curve";
  if (p.oetf < DMT_OETF_LINEAR || p.oetf > DMT_OETF_GAMMA22) return "unknown transfer function";
  if (p.quantiser < DMT_QUANT_TRUNCATE || p.quantiser > DMT_QUANT_DITHER) return "unknown quantiser";
  if (p.white < 0.f) return "white must be >= 0 (0: the curve's default)";
  return nullptr;
}
float displayWhite(dmt_display_params const& p) {
  if (p.white > 0.f) return p.white;
  return p.tone == DMT_TONE_HABLE ? 11.2f : 4.f;
}
float displayManualScale(dmt_display_params const& p) { return float(std::exp2(double(p.exposure_ev))); }

// Metering, in double.  Bin k stands for L_k = floor(k/8) - 16 + log2(1 + ((k mod 8) + 0.5)/8).  The counted pixels, sorted
// by bin, occupy [0, T); the mass between low T and (1 - high) T is kept, a bin weighted by its overlap with that interval.
void displayMeter(dmt_display_params const& p, uint32_t const* hist, uint64_t* counted, double* avgLog2, float* scale) {
  uint64_t T = 0;
  for (uint32_t k = 0; k < kDisplayBins; ++k) T += hist[k];
  double const lo = double(p.low_fraction) * double(T), hi = (1.0 - double(p.high_fraction)) * double(T);
  double mass = 0.0, sum = 0.0, below = 0.0;
  for (uint32_t k = 0; k < kDisplayBins; ++k) {
    double const top = below + double(hist[k]);
    double const ov = std::min(top, hi) - std::max(below, lo);
    if (hist[k] && ov > 0.0) {
      double const Lk = double(int(k / 8u) - 16) + std::log2(1.0 + (double(k % 8u) + 0.5) / 8.0);
      mass += ov, sum += ov * Lk;
    }
    below = top;
  }
  *counted = T;
  if (T == 0 || !(mass > 0.0)) {
    *avgLog2 = 0.0, *scale = displayManualScale(p);
    return;
  }
  *avgLog2 = sum / mass;
  *scale = float(double(p.key) / std::exp2(*avgLog2) * std::exp2(double(p.exposure_ev)));
}

struct DisplayLevel {
  int w, h;
  size_t offset;  // into the pyramid, in float4
};

// scrub -> exposure -> bloom -> tone -> transfer -> quantise on device planes, on the context's stream.  Returns after the
// last launch; only auto exposure waits (for its histogram).  Leaves the record pending (finishDisplay)
int displayRun(dmt_ctx* ctx, dmt_display_params const& p, float4 const* d_src, float4* d_out4, uint32_t* d_out8) {
  DisplayState& S = ctx->disp;
  int const w = ctx->camera.cam.width, h = ctx->camera.cam.height;
  size_t const pixels = size_t(w) * size_t(h);
  HIP_TRY(ctx, S.counters.reserve(kDisplayCounters));
  for (EventPair* ev : {&S.evHist, &S.evBloom, &S.evResolve}) {
    if (!ev->a) HIP_TRY(ctx, hipEventCreate(&ev->a));
    if (!ev->b) HIP_TRY(ctx, hipEventCreate(&ev->b));
  }
  // bloom: the levels that fit, and where they live
  int levels = 0;
  DisplayLevel lv[9];
  lv[0] = {w, h, 0};
  if (p.bloom_levels > 0 && p.bloom_strength > 0.f) {
    int fit = 0;
    while ((std::min(w, h) >> (fit + 1)) > 0) ++fit;  // floor(log2(min(w, h)))
    levels = std::min(p.bloom_levels, fit);
  }
  size_t total = pixels;
  for (int l = 1; l <= levels; ++l) {
    lv[l] = {(lv[l - 1].w + 1) / 2, (lv[l - 1].h + 1) / 2, total};
    total += size_t(lv[l].w) * size_t(lv[l].h);
  }
  if (levels > 0) HIP_TRY(ctx, S.pyramid.reserve(total));

  dmt_display_record R{};
  R.width = w, R.height = h, R.levels = levels;
  S.pending = false, S.timedHist = S.timedBloom = S.timedResolve = false;
  HIP_TRY(ctx, hipMemsetAsync(S.counters.get(), 0, kDisplayCounters * sizeof(uint32_t), ctx->stream));
  if (p.auto_exposure) {
    // a few blocks per CU stride over the frame: blocks x 257 global atomics at most
    size_t const blocks = std::min((pixels + 255) / 256, size_t(std::max(ctx->launch.cuCount, 1)) * 8);
    HIP_TRY(ctx, hipEventRecord(S.evHist.a, ctx->stream));
    hipLaunchKernelGGL(k_display_histogram, dim3(uint32_t(blocks)), dim3(256), 0, ctx->stream, d_src, uint32_t(pixels), S.counters.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(S.evHist.b, ctx->stream));
    uint32_t host[kDisplayBins + 1];
    HIP_TRY(ctx, hipMemcpyAsync(host, S.counters.get(), sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    S.timedHist = true;
    std::memcpy(R.histogram, host, sizeof(R.histogram));
    R.skipped = host[kDisplaySkipped];
    uint64_t T = 0;
    displayMeter(p, R.histogram, &T, &R.avg_log2, &R.scale);
    R.counted = uint32_t(T);
  } else {
    R.scale = displayManualScale(p);
  }
  if (levels > 0) {
    float4* const pyr = S.pyramid.get();
    HIP_TRY(ctx, hipEventRecord(S.evBloom.a, ctx->stream));
    for (int l = 0; l < levels; ++l) {  // B_{l+1} from B_l; B_0 is the exposed source
      BloomArgs A{};
      A.src = l == 0 ? d_src : pyr + lv[l].offset, A.dst = pyr + lv[l + 1].offset;
      A.ws = lv[l].w, A.hs = lv[l].h, A.wd = lv[l + 1].w, A.hd = lv[l + 1].h, A.scale = R.scale, A.level0 = l == 0;
      size_t const n = size_t(A.wd) * size_t(A.hd);
      hipLaunchKernelGGL(k_bloom_down, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
      HIP_TRY(ctx, hipGetLastError());
    }
    for (int l = levels - 1; l >= 0; --l) {  // U_l = B_l + up2(U_{l+1}), over B_l; U_0 in the pyramid's first plane
      BloomArgs A{};
      A.src = pyr + lv[l + 1].offset, A.fine = l == 0 ? d_src : pyr + lv[l].offset, A.dst = pyr + lv[l].offset;
      A.ws = lv[l + 1].w, A.hs = lv[l + 1].h, A.wd = lv[l].w, A.hd = lv[l].h, A.scale = R.scale, A.level0 = l == 0;
      size_t const n = size_t(A.wd) * size_t(A.hd);
      hipLaunchKernelGGL(k_bloom_up, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
      HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(S.evBloom.b, ctx->stream));
    S.timedBloom = true;
  }
  ResolveArgs A{};
  A.src = d_src, A.bloom = levels > 0 ? S.pyramid.get() : nullptr, A.out4 = d_out4, A.out8 = d_out8, A.counters = S.counters.get();
  A.pixels = uint32_t(pixels), A.width = uint32_t(w);
  A.scale = R.scale, A.strength = p.bloom_strength, A.levels1 = float(levels + 1), A.white = displayWhite(p);
  A.tone = p.tone, A.oetf = p.oetf, A.quantiser = p.quantiser;
  HIP_TRY(ctx, hipEventRecord(S.evResolve.a, ctx->stream));
  hipLaunchKernelGGL(k_display_resolve, dim3(uint32_t((pixels + 255) / 256)), dim3(256), 0, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(S.evResolve.b, ctx->stream));
  S.timedResolve = true;
  S.record = R, S.pending = true;
  return DMT_OK;
}
// what the last call left on the device: waits for the stream, then the non-finite count and the stages' times
int finishDisplay(dmt_ctx* ctx) {
  DisplayState& S = ctx->disp;
  if (!S.pending) return DMT_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(&S.record.nonfinite, S.counters.get() + kDisplayNonfinite, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (S.timedHist) HIP_TRY(ctx, hipEventElapsedTime(&S.record.histogram_ms, S.evHist.a, S.evHist.b));
  if (S.timedBloom) HIP_TRY(ctx, hipEventElapsedTime(&S.record.bloom_ms, S.evBloom.a, S.evBloom.b));
  if (S.timedResolve) HIP_TRY(ctx, hipEventElapsedTime(&S.record.resolve_ms, S.evResolve.a, S.evResolve.b));
  S.pending = false;
  return DMT_OK;
}
// the checks both entry points share, before anything is touched
int displayCheck(dmt_ctx* ctx, char const* name, dmt_display_params const& p, bool haveSrc, bool haveOut) {
  std::string const pre = std::string(name) + ": ";
  if (char const* why = displayParamsError(p)) return fail(ctx, DMT_ERR_INVALID, (pre + why).c_str());
  if (!ctx->camera.have) return fail(ctx, DMT_ERR_STATE, (pre + "set the camera first (the plane has its size)").c_str());
  if (uint64_t(ctx->camera.cam.width) * uint64_t(ctx->camera.cam.height) > (1ull << 31))  // the kernels index pixels in 32 bits
    return fail(ctx, DMT_ERR_STATE, (pre + "frames of more than 2^31 pixels are not supported").c_str());
  if (!haveOut) return fail(ctx, DMT_ERR_INVALID, (pre + "out4 and out_rgba8 are both null").c_str());
  if (!haveSrc && !ctx->film.mean) return fail(ctx, DMT_ERR_STATE, (pre + "no film").c_str());
  if (!haveSrc && ctx->launch.world > 1)
    return fail(ctx, DMT_ERR_STATE, (pre + "this context renders only the tiles of its dmt_set_partition rank: combine the ranks' films and pass "
                                           "the combined mean as the source plane").c_str());
  return DMT_OK;
}

}  // namespace

extern "C" {

// ---- display transform -----------------------------------------------------------
dmt_display_params dmt_display_defaults(void) {
  dmt_display_params p;
  p.auto_exposure = 0, p.exposure_ev = 0.f, p.key = 0.18f, p.low_fraction = 0.10f, p.high_fraction = 0.05f;
  p.bloom_levels = 0, p.bloom_strength = 0.f;
  p.tone = DMT_TONE_ACES, p.white = 0.f, p.oetf = DMT_OETF_SRGB, p.quantiser = DMT_QUANT_ROUND;
  return p;
}

int dmt_display(dmt_ctx* ctx, const dmt_display_params* params, const float* src4, float* out4, uint8_t* out_rgba8, float* kernel_ms) {
  if (!ctx) return DMT_ERR_INVALID;
  if (kernel_ms) *kernel_ms = 0.f;
  dmt_display_params const p = params ? *params : dmt_display_defaults();
  if (int const rc = displayCheck(ctx, "dmt_display", p, src4 != nullptr, out4 || out_rgba8)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DisplayState& S = ctx->disp;
  size_t const pixels = size_t(ctx->camera.cam.width) * size_t(ctx->camera.cam.height);
  float4 const* src = ctx->film.mean;
  if (src4) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a call in flight may still read the copy
    HIP_TRY(ctx, S.src.reserve(pixels));
    HIP_TRY(ctx, hipMemcpy(S.src.get(), src4, pixels * sizeof(float4), hipMemcpyHostToDevice));
    src = S.src.get();
  }
  if (out4) HIP_TRY(ctx, S.out4.reserve(pixels));
  if (out_rgba8) HIP_TRY(ctx, S.out8.reserve(pixels));
  if (int const rc = displayRun(ctx, p, src, out4 ? S.out4.get() : nullptr, out_rgba8 ? S.out8.get() : nullptr)) return rc;
  if (int const rc = finishDisplay(ctx)) return rc;
  if (out4) HIP_TRY(ctx, hipMemcpy(out4, S.out4.get(), pixels * sizeof(float4), hipMemcpyDeviceToHost));
  if (out_rgba8) HIP_TRY(ctx, hipMemcpy(out_rgba8, S.out8.get(), pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (kernel_ms) *kernel_ms = S.record.histogram_ms + S.record.bloom_ms + S.record.resolve_ms;
  return DMT_OK;
}

int dmt_display_device(dmt_ctx* ctx, const dmt_display_params* params, const void* d_src4, void* d_out4, void* d_out_rgba8) {
  if (!ctx) return DMT_ERR_INVALID;
  dmt_display_params const p = params ? *params : dmt_display_defaults();
  if (int const rc = displayCheck(ctx, "dmt_display_device", p, d_src4 != nullptr, d_out4 || d_out_rgba8)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return displayRun(ctx, p, d_src4 ? static_cast<float4 const*>(d_src4) : ctx->film.mean, static_cast<float4*>(d_out4),
                    static_cast<uint32_t*>(d_out_rgba8));
}

int dmt_display_info(dmt_ctx* ctx, dmt_display_record* out) {
  if (!ctx || !out) return DMT_ERR_INVALID;
  if (ctx->disp.record.width == 0) return fail(ctx, DMT_ERR_STATE, "dmt_display_info: no display call yet");
  if (int const rc = finishDisplay(ctx)) return rc;
  *out = ctx->disp.record;
  return DMT_OK;
}

int dmt_display_curve(const dmt_display_params* params, int n, const float* rgb3_in, float* rgb3_out) {
  dmt_display_params const p = params ? *params : dmt_display_defaults();
  if (displayParamsError(p) || n < 0 || (n && (!rgb3_in || !rgb3_out))) return DMT_ERR_INVALID;
  float const white = displayWhite(p);
  for (size_t i = 0; i < size_t(n); ++i) {
    DRgb const o = display_oetf(display_tone(DRgb{rgb3_in[3 * i], rgb3_in[3 * i + 1], rgb3_in[3 * i + 2]}, p.tone, white), p.oetf);
    rgb3_out[3 * i] = o.x, rgb3_out[3 * i + 1] = o.y, rgb3_out[3 * i + 2] = o.z;
  }
  return DMT_OK;
}

int dmt_display_metering(const dmt_display_params* params, const uint32_t* histogram256, double* avg_log2, float* scale) {
  dmt_display_params const p = params ? *params : dmt_display_defaults();
  if (displayParamsError(p) || !histogram256 || !avg_log2 || !scale) return DMT_ERR_INVALID;
  uint64_t T = 0;
  displayMeter(p, histogram256, &T, avg_log2, scale);
  return DMT_OK;
}

int dmt_display_bin(int n, const float* y, int32_t* bin) {
  if (n < 0 || (n && (!y || !bin))) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) bin[i] = display_bin(y[i]);
  return DMT_OK;
}

}  // extern "C"
