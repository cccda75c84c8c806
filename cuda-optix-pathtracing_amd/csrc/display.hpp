// display.hpp -- the display transform's device code and state (dmt_display): a linear RGB plane to a
// display-referred one.  scrub -> exposure -> bloom -> tone curve -> transfer function -> quantise, in that order.
//
// Part of dmt_hip.hip's translation unit, included once inside its anonymous namespace after denoise.hpp.  It uses nothing of
// the path tracer: no RenderParams, no megakernel row, so no existing kernel gains a register.  The entry points are in
// display_host.hpp; tests/display_ref.py restates every stage in numpy.
//
// What is exact and what is not.  The scrub, the luminance, the histogram bin, the exposure product and the quantiser are
// written without contraction, one rounding per operation, and are compared bit for bit with the restatement.  The tone
// curves and the transfer functions divide and call powf: the device divides by a reciprocal and one residual step
// (display_div) and its powf is ocml's, so those are compared with float64 under a tolerance.  The library flushes fp32 denormals on the device (Makefile),
// so a luminance below 2^-126 meters as 0 there ("skipped"); the host twin dmt_display_bin counts it in bin 0.
#pragma once

struct DRgb {
  float x, y, z;
};

// stage 0: a component that is not finite, or whose sign bit is set, becomes +0; `bad` is set for a non-finite one.  On the
// bits, so that neither a NaN's comparison nor the denormal mode has a say
DMT_HD float display_scrub1(float v, bool& bad) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  bool const nonfinite = (b & 0x7F800000u) == 0x7F800000u;
  bad = bad || nonfinite;
  return (nonfinite || (b >> 31)) ? 0.f : v;
}
DMT_HD DRgb display_scrub(float r, float g, float b, bool& bad) {
  bad = false;
  DRgb o;
  o.x = display_scrub1(r, bad), o.y = display_scrub1(g, bad), o.z = display_scrub1(b, bad);
  return o;
}
// Rec. 709 luminance, (0.2126 r + 0.7152 g) + 0.0722 b, every operation rounded
DMT_HD float display_lum(DRgb c) {
#pragma clang fp contract(off)
  float const a = 0.2126f * c.x;
  float const b = 0.7152f * c.y;
  float const d = 0.0722f * c.z;
  float const ab = a + b;
  return ab + d;
}
// stage 1, metering: the histogram bin of a luminance from the float's own bits, exponent plus three mantissa bits: eight
// bins per stop over [2^-16, 2^16), clamped.  -1: not counted (y <= 0; a scrubbed pixel has no other kind)
DMT_HD int display_bin(float y) {
  uint32_t b;
  __builtin_memcpy(&b, &y, 4);
  if (b == 0u || (b >> 31) || b > 0x7F800000u) return -1;  // 0, negative, NaN
  int const k = int(b >> 20) - 888;
  return k < 0 ? 0 : (k > 255 ? 255 : k);
}
// stage 1: c = scale * rgb
DMT_HD DRgb display_expose(DRgb c, float scale) {
#pragma clang fp contract(off)
  DRgb o;
  o.x = scale * c.x, o.y = scale * c.y, o.z = scale * c.z;
  return o;
}

// a / b of the curves: the library's device `/` is the 2.5-ulp one (Makefile), which would cost the curves their accuracy;
// proj_div (denoise.hpp) rounds as the host does except in rare half-way cases
DMT_HD float display_div(float a, float b) { return proj_div(a, b); }
// stage 3: the tone curves.  `white` is the curve's white point (the caller has replaced 0 by the default)
DMT_HD float display_clamp01(float v) { return __builtin_fminf(__builtin_fmaxf(v, 0.f), 1.f); }
DMT_HD float display_aces1(float x) {  // Narkowicz's fit
#pragma clang fp contract(off)
  return display_div(x * (2.51f * x + 0.03f), x * (2.43f * x + 0.59f) + 0.14f);
}
DMT_HD float display_hable_f(float x) {
#pragma clang fp contract(off)
  float const A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
  return display_div(x * (A * x + C * B) + D * E, x * (A * x + B) + D * F) - display_div(E, F);
}
DMT_HD DRgb display_tone(DRgb c, int tone, float white) {
#pragma clang fp contract(off)
  DRgb o = c;
  if (tone == DMT_TONE_REINHARD) {
    float const L = display_lum(c);
    float k = 0.f;
    if (L > 0.f) {
      float const Ld = display_div(L * (1.f + display_div(L, white * white)), 1.f + L);
      k = display_div(Ld, L);
    }
    o.x = c.x * k, o.y = c.y * k, o.z = c.z * k;
  } else if (tone == DMT_TONE_ACES) {
    o.x = display_aces1(c.x), o.y = display_aces1(c.y), o.z = display_aces1(c.z);
  } else if (tone == DMT_TONE_HABLE) {
    float const fw = display_hable_f(white);
    o.x = display_div(display_hable_f(2.f * c.x), fw), o.y = display_div(display_hable_f(2.f * c.y), fw), o.z = display_div(display_hable_f(2.f * c.z), fw);
  }
  o.x = display_clamp01(o.x), o.y = display_clamp01(o.y), o.z = display_clamp01(o.z);
  return o;
}
// stage 4: the transfer functions, on [0, 1]
DMT_HD float display_oetf1(float x, int oetf) {
#pragma clang fp contract(off)
  float v = x;
  if (oetf == DMT_OETF_SRGB) v = x <= 0.0031308f ? 12.92f * x : 1.055f * powf(x, 1.f / 2.4f) - 0.055f;
  else if (oetf == DMT_OETF_GAMMA22) v = powf(x, 1.f / 2.2f);
  return display_clamp01(v);
}
DMT_HD DRgb display_oetf(DRgb c, int oetf) {
  DRgb o;
  o.x = display_oetf1(c.x, oetf), o.y = display_oetf1(c.y, oetf), o.z = display_oetf1(c.z, oetf);
  return o;
}
// stage 5: the standard 8 x 8 Bayer index matrix (0 .. 63) at (x & 7, y & 7), and the quantiser of one channel
DMT_HD uint32_t display_bayer(uint32_t x, uint32_t y) {
  uint32_t const xc = x ^ y;
  uint32_t m = 0;
  for (uint32_t i = 0; i < 3; ++i) m |= ((xc >> i) & 1u) << (5u - 2u * i) | ((y >> i) & 1u) << (4u - 2u * i);
  return m;
}
DMT_HD float display_quant_bias(int quantiser, uint32_t x, uint32_t y) {
  if (quantiser == DMT_QUANT_ROUND) return 0.5f;
  if (quantiser == DMT_QUANT_DITHER) return (float(display_bayer(x & 7u, y & 7u)) + 0.5f) / 64.f;  // exact: 7 significant bits
  return 0.f;
}
DMT_HD uint32_t display_quant1(float v, float bias) {  // v in [0, 1]
#pragma clang fp contract(off)
  float const t = v * 255.f;
  float const u = t + bias;
  return uint32_t(__builtin_floorf(__builtin_fminf(u, 255.f)));
}

// ---- kernels -----------------------------------------------------------------------------------------
// The counters of one call, in one device array: the 256 bins, then the pixels the meter skipped, then the pixels with a
// non-finite component
constexpr uint32_t kDisplayBins = 256;
constexpr uint32_t kDisplaySkipped = 256, kDisplayNonfinite = 257, kDisplayCounters = 258;

// Log-luminance histogram.  Each block counts into LDS with LDS integer atomics and flushes with one global integer atomic
// per non-zero counter; the grid is bounded (a few blocks per CU) and strides over the frame, so a large frame sends
// blocks x 256 global atomics at most, not one per pixel.  Integer counts: independent of the order, exactly reproducible.
__global__ void __launch_bounds__(256) k_display_histogram(float4 const* __restrict__ src, uint32_t pixels, uint32_t* __restrict__ counters) {
  __shared__ uint32_t s_bins[kDisplayBins + 1];  // [256]: skipped
  for (uint32_t i = threadIdx.x; i < kDisplayBins + 1; i += 256u) s_bins[i] = 0u;
  __syncthreads();
  uint32_t const stride = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < pixels; i += stride) {
    float4 const v = src[i];
    bool bad;
    int const k = display_bin(display_lum(display_scrub(v.x, v.y, v.z, bad)));
    atomicAdd(&s_bins[k < 0 ? kDisplaySkipped : uint32_t(k)], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kDisplayBins + 1; i += 256u) {
    uint32_t const n = s_bins[i];
    if (n) atomicAdd(&counters[i], n);
  }
}

// Bloom pyramid, one thread per output pixel, plain gathers: a level is a quarter of the one below, every tap of a wave lies
// in two short row segments, and the whole pyramid of a 4096^2 frame is 85 MB, so the taps come from L2; LDS tiles would
// save loads the cache already absorbs.  Level 0 is never stored: it is scale * scrub(src), formed where it is read.
struct BloomArgs {
  float4 const* src;     // down: level l.  up: the coarse plane U_{l+1}
  float4 const* fine;    // up only: B_l (level 0: the source plane)
  float4* dst;           // down: level l + 1.  up: U_l (may be `fine` itself: a thread reads and writes its own pixel only)
  int ws, hs, wd, hd;    // size of src and of dst
  float scale;           // level 0 only (level0 != 0): the exposure
  int level0;            // down: src is the source plane.  up: fine is the source plane
};
DMT_DEV DRgb bloom_load(float4 const* p, size_t i, bool level0, float scale) {
  float4 const v = p[i];
  if (!level0) return DRgb{v.x, v.y, v.z};
  bool bad;
  return display_expose(display_scrub(v.x, v.y, v.z, bad), scale);
}
// B_{l+1}(x, y) = ((a + b) + (c + d)) * 0.25 over B_l at (min(2x + i, w - 1), min(2y + j, h - 1))
__global__ void __launch_bounds__(256) k_bloom_down(BloomArgs A) {
#pragma clang fp contract(off)
  uint32_t const i = blockIdx.x * 256u + threadIdx.x;
  if (i >= uint32_t(A.wd) * uint32_t(A.hd)) return;
  int const x = int(i % uint32_t(A.wd)), y = int(i / uint32_t(A.wd));
  int const x0 = min(2 * x, A.ws - 1), x1 = min(2 * x + 1, A.ws - 1);
  int const y0 = min(2 * y, A.hs - 1), y1 = min(2 * y + 1, A.hs - 1);
  bool const l0 = A.level0 != 0;
  DRgb const a = bloom_load(A.src, size_t(y0) * size_t(A.ws) + size_t(x0), l0, A.scale);
  DRgb const b = bloom_load(A.src, size_t(y0) * size_t(A.ws) + size_t(x1), l0, A.scale);
  DRgb const c = bloom_load(A.src, size_t(y1) * size_t(A.ws) + size_t(x0), l0, A.scale);
  DRgb const d = bloom_load(A.src, size_t(y1) * size_t(A.ws) + size_t(x1), l0, A.scale);
  A.dst[i] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.f);
}
// U_l = B_l + up2(U_{l+1}); up2 is separable, rows then columns: fine index x takes 0.75 C[i] + 0.25 C[n], i = x >> 1,
// n = clamp(i + (x odd ? 1 : -1), 0, wc - 1)
__global__ void __launch_bounds__(256) k_bloom_up(BloomArgs A) {
#pragma clang fp contract(off)
  uint32_t const i = blockIdx.x * 256u + threadIdx.x;
  if (i >= uint32_t(A.wd) * uint32_t(A.hd)) return;
  int const x = int(i % uint32_t(A.wd)), y = int(i / uint32_t(A.wd));
  int const xi = min(x >> 1, A.ws - 1), yi = min(y >> 1, A.hs - 1);  // (x >> 1 < ws by the level sizes; the clamp keeps any size inside)
  int const xn = min(max(xi + ((x & 1) ? 1 : -1), 0), A.ws - 1), yn = min(max(yi + ((y & 1) ? 1 : -1), 0), A.hs - 1);
  float4 const cii = A.src[size_t(yi) * size_t(A.ws) + size_t(xi)], cni = A.src[size_t(yi) * size_t(A.ws) + size_t(xn)];
  float4 const cin = A.src[size_t(yn) * size_t(A.ws) + size_t(xi)], cnn = A.src[size_t(yn) * size_t(A.ws) + size_t(xn)];
  auto mix = [](float a, float b) {
    float const p = 0.75f * a;
    float const q = 0.25f * b;
    return p + q;
  };
  float const rx = mix(mix(cii.x, cni.x), mix(cin.x, cnn.x));  // the two rows at this column, then the column
  float const ry = mix(mix(cii.y, cni.y), mix(cin.y, cnn.y));
  float const rz = mix(mix(cii.z, cni.z), mix(cin.z, cnn.z));
  DRgb const f = bloom_load(A.fine, i, A.level0 != 0, A.scale);
  A.dst[i] = make_float4(f.x + rx, f.y + ry, f.z + rz, 0.f);
}

// Exposure, bloom mix, tone curve, transfer function and quantiser in one pass: one float4 load (and one of the bloom plane),
// one float4 store and / or one packed 4-byte store per pixel.  Counts the pixels with a non-finite component: one ballot per
// wave, one global atomic per wave that has any.
struct ResolveArgs {
  float4 const* src;
  float4 const* bloom;  // U_0, or null
  float4* out4;         // or null
  uint32_t* out8;       // RGBA8, R in the low byte; or null
  uint32_t* counters;
  uint32_t pixels, width;
  float scale, strength, levels1;  // levels1 = K' + 1
  float white;
  int tone, oetf, quantiser;
};
__global__ void __launch_bounds__(256) k_display_resolve(ResolveArgs A) {
#pragma clang fp contract(off)
  uint32_t const i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  if (i < A.pixels) {
    float4 const v = A.src[i];
    DRgb c = display_expose(display_scrub(v.x, v.y, v.z, bad), A.scale);
    if (A.bloom) {  // c + s (U_0 / (K' + 1) - c)
      float4 const u = A.bloom[i];
      float const bx = display_div(u.x, A.levels1), by = display_div(u.y, A.levels1), bz = display_div(u.z, A.levels1);
      float const dx = bx - c.x, dy = by - c.y, dz = bz - c.z;
      float const sx = A.strength * dx, sy = A.strength * dy, sz = A.strength * dz;
      c.x = c.x + sx, c.y = c.y + sy, c.z = c.z + sz;
    }
    DRgb const o = display_oetf(display_tone(c, A.tone, A.white), A.oetf);
    if (A.out4) A.out4[i] = make_float4(o.x, o.y, o.z, 1.f);
    if (A.out8) {
      float const bias = display_quant_bias(A.quantiser, i % A.width, i / A.width);
      A.out8[i] = display_quant1(o.x, bias) | display_quant1(o.y, bias) << 8 | display_quant1(o.z, bias) << 16 | 0xFF000000u;
    }
  }
  unsigned long long const m = __ballot(bad);
  if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(&A.counters[kDisplayNonfinite], uint32_t(__popcll(m)));
}

// What a context keeps for this layer: the scratch of a call, reused across calls, and the record of the last one.  A call
// never reads what an earlier one left, so nothing here has to be dropped when the camera or the film changes.
struct DisplayState {
  DevBuf<float4> src;        // a host plane's copy (dmt_display with a source)
  DevBuf<float4> out4;       // dmt_display's device-side outputs
  DevBuf<uint32_t> out8;
  DevBuf<float4> pyramid;    // U_0 (a full plane), then levels 1 .. K' back to back
  DevBuf<uint32_t> counters; // kDisplayCounters
  EventPair evHist, evBloom, evResolve;
  bool timedHist = false, timedBloom = false, timedResolve = false;  // the pairs recorded by the last call
  bool pending = false;      // the last call's non-finite count and times are still on the device (dmt_display_device)
  dmt_display_record record{};
};
