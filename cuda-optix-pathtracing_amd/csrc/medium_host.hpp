// medium_host.hpp -- the host side of the medium layer: the argument checks, the scan of a density grid and the one shell of
// its two uploads, the records of a medium given in a call (the host twins and the probes), and the dmt_* entry points of
// the medium, its grid and its spectrum.  The layer's state and its rules -- what each call keeps and drops, what is
// derived at launch, when a record is active, which calls drain the stream -- are in medium_state.hpp, its device code in
// medium_device.hpp, the arithmetic both sides share in medium.hpp and medium_grid.hpp.
//
// Part of dmt_hip.hip's translation unit, included once after the host helpers it uses (dmt_ctx, HIP_TRY, fail) and before
// probes.hpp, which calls mediumRefused, mediumArgsError, mediumGridCallRecord and mediumSpectrumCallRecord.
#pragma once

namespace {

// a refused call: "<who>: <why>" for dmt_last_error
int mediumRefused(dmt_ctx* ctx, char const* who, std::string const& why) { return fail(ctx, DMT_ERR_INVALID, (std::string(who) + ": " + why).c_str()); }

// ---- the participating medium (medium.hpp) ----------------------------------------
bool mediumBoxOk(const float* box_min3, const float* box_max3) {  // finite with min < max on every axis
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(box_min3[i]) || !std::isfinite(box_max3[i]) || !(box_min3[i] < box_max3[i])) return false;
  return true;
}
char const* mediumArgsError(float sigma_t, const float* albedo3, float g, const float* box_min3, const float* box_max3) {
  if (!albedo3 || !box_min3 || !box_max3) return "null argument";
  if (!std::isfinite(sigma_t) || sigma_t < 0.f) return "sigma_t must be finite and >= 0";
  for (int i = 0; i < 3; ++i)
    if (!(albedo3[i] >= 0.f && albedo3[i] <= 1.f)) return "the albedo must be in [0, 1] per channel";
  if (!(std::fabs(g) < 1.f)) return "g must be in (-1, 1)";
  if (!mediumBoxOk(box_min3, box_max3)) return "the box must be finite with min < max on every axis";
  return nullptr;
}

// ---- the medium's spectrum (medium.hpp) -------------------------------------------
char const* mediumSpectrumArgsError(const float* extinction3, const float* emission3) {
  if (!extinction3 || !emission3) return "null argument";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(extinction3[i]) || extinction3[i] < 0.f) return "the extinction colour must be finite and >= 0 per channel";
  if (extinction3[0] == 0.f && extinction3[1] == 0.f && extinction3[2] == 0.f) return "the extinction colour must not be all zero";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(emission3[i]) || emission3[i] < 0.f) return "the emission must be finite and >= 0 per channel";
  return nullptr;
}
// channel extinctions given in a call (dmt_medium_spectrum_event, dmt_test_medium_spectrum): finite, >= 0, not all zero;
// q3 = k / the largest
char const* mediumSpectrumCallRecord(const float* k3, float* q3) {
  if (!k3) return "null argument";
  int m = 0;
  for (int i = 0; i < 3; ++i) {
    if (!std::isfinite(k3[i]) || k3[i] < 0.f) return "the channel extinctions must be finite and >= 0";
    if (k3[i] > k3[m]) m = i;
  }
  if (!(k3[m] > 0.f)) return "the channel extinctions must not be all zero";
  for (int i = 0; i < 3; ++i) q3[i] = medium_spectrum_q(k3[i], k3[m]);
  return nullptr;
}

// ---- the medium's density grid (medium_grid.hpp) ----------------------------------
char const* mediumGridDimsError(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > kMediumGridMaxAxis || ny > kMediumGridMaxAxis || nz > kMediumGridMaxAxis) return "nx, ny and nz must be in 1 .. 512";
  if (uint64_t(nx) * uint64_t(ny) * uint64_t(nz) > kMediumGridMaxVoxels) return "at most 2^26 voxels";
  return nullptr;
}
// what a pass over the densities finds: the support index ranges, the voxels > 0, the largest density, the first voxel that
// is negative or not finite (~0: none).  k_medium_grid_scan reduces the same words on the device.
struct MediumGridScan {
  uint32_t lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u}, count = 0u, top = 0u, bad = ~0u;
  // the support as the records hold it: imin > imax without a density > 0
  void support(int32_t* imin, int32_t* imax) const {
    for (int a = 0; a < 3; ++a) imin[a] = count ? int32_t(lo[a]) : 0, imax[a] = count ? int32_t(hi[a]) : -1;
  }
  // what a grid with a bad voxel is refused with
  std::string badVoxel(int nx, int ny) const {
    return "every density must be finite and >= 0; voxel (" + std::to_string(bad % uint64_t(nx)) + ", " + std::to_string((bad / uint64_t(nx)) % uint64_t(ny)) +
           ", " + std::to_string(bad / (uint64_t(nx) * uint64_t(ny))) + ") is not";
  }
};
static_assert(sizeof(MediumGridScan) == 9 * sizeof(uint32_t), "the nine words of k_medium_grid_scan");
MediumGridScan mediumGridScanHost(float const* density, int nx, int ny, int nz) {
  MediumGridScan s;
  size_t v = 0;
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x, ++v) {
        float const d = density[v];
        if (!(d >= 0.f) || !std::isfinite(d)) {
          if (s.bad == ~0u) s.bad = uint32_t(v);
        } else if (d > 0.f) {
          uint32_t const i[3] = {uint32_t(x), uint32_t(y), uint32_t(z)};
          for (int a = 0; a < 3; ++a) s.lo[a] = std::min(s.lo[a], i[a]), s.hi[a] = std::max(s.hi[a], i[a]);
          uint32_t bits;
          std::memcpy(&bits, &d, 4);
          ++s.count, s.top = std::max(s.top, bits);
        }
      }
  return s;
}
// the device upload's way into `staged`: a copy on the stream, scanned there; s arrives with the reduction's initial values
int mediumGridStageDevice(dmt_ctx* ctx, void const* d_density, int nx, int ny, size_t total, DevBuf<float>& staged, MediumGridScan& s) {
  DevBuf<uint32_t> words;
  HIP_TRY(ctx, staged.reserve(total));
  HIP_TRY(ctx, words.reserve(9));
  HIP_TRY(ctx, hipMemcpyAsync(staged.get(), d_density, total * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(words.get(), &s, sizeof s, hipMemcpyHostToDevice, ctx->stream));
  unsigned const blocks = unsigned(std::min<size_t>((total + 255) / 256, 1024));
  hipLaunchKernelGGL(k_medium_grid_scan, dim3(blocks), dim3(256), 0, ctx->stream, staged.get(), nx, ny, uint32_t(total), words.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&s, words.get(), sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DMT_OK;
}
// dmt_set_medium_grid and dmt_set_medium_grid_device.  They differ in how the densities reach `staged` and in who scans
// them: host memory is scanned here before anything touches the stream, and copied only when the scan has passed.
int mediumGridUpload(dmt_ctx* ctx, char const* who, void const* density, bool onDevice, int nx, int ny, int nz) {
  if (!ctx) return DMT_ERR_INVALID;
  if (!density) return mediumRefused(ctx, who, "null argument");
  if (char const* const why = mediumGridDimsError(nx, ny, nz)) return mediumRefused(ctx, who, why);
  size_t const total = size_t(nx) * size_t(ny) * size_t(nz);
  MediumGridScan s;
  if (!onDevice) s = mediumGridScanHost(static_cast<float const*>(density), nx, ny, nz);
  DevBuf<float> staged;
  if (s.bad == ~0u) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (onDevice) {
      if (int const rc = mediumGridStageDevice(ctx, density, nx, ny, total, staged, s)) return rc;
    } else {
      HIP_TRY(ctx, staged.assign(static_cast<float const*>(density), total));
    }
  }
  if (s.bad != ~0u) return mediumRefused(ctx, who, s.badVoxel(nx, ny));
  MediumState::Grid& g = ctx->medium.grid;
  g.density = std::move(staged);
  g.have = true;
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  s.support(g.imin, g.imax);
  g.positive = s.count;
  std::memcpy(&g.maxDensity, &s.top, 4);
  return DMT_OK;
}
// a grid given in a call (dmt_medium_grid_march, dmt_test_medium_grid): checked as the uploads check theirs; the record
// with the support of `density`, whose pointer the caller sets
char const* mediumGridCallRecord(const float* box_min3, const float* box_max3, float sigma_t, int nx, int ny, int nz, const float* density,
                                 MediumGridParams& g, std::string& why) {
  float const white[3] = {1.f, 1.f, 1.f};
  if (!density) return "null argument";
  if (char const* const e = mediumArgsError(sigma_t, white, 0.f, box_min3, box_max3)) return e;
  if (char const* const e = mediumGridDimsError(nx, ny, nz)) return e;
  MediumGridScan const s = mediumGridScanHost(density, nx, ny, nz);
  if (s.bad != ~0u) return (why = s.badVoxel(nx, ny)).c_str();
  g = MediumGridParams{};
  g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
  s.support(g.imin, g.imax);
  medium_grid_derive(g, box_min3, box_max3);
  return nullptr;
}

}  // namespace

extern "C" {

int dmt_set_medium(dmt_ctx* ctx, float sigma_t, const float* albedo3, float g, const float* box_min3, const float* box_max3) {
  if (!ctx) return DMT_ERR_INVALID;
  if (char const* const why = mediumArgsError(sigma_t, albedo3, g, box_min3, box_max3)) return mediumRefused(ctx, "dmt_set_medium", why);
  MediumParams& m = ctx->medium.p;
  m.sigmaT = sigma_t, m.g = g;
  for (int i = 0; i < 3; ++i) m.albedo[i] = albedo3[i], m.lo[i] = box_min3[i], m.hi[i] = box_max3[i];
  return DMT_OK;
}

int dmt_clear_medium(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  if (int const rc = dmt_clear_medium_grid(ctx)) return rc;
  ctx->medium.p = MediumParams{};
  ctx->medium.spectrum = MediumState::Spectrum{};
  return DMT_OK;
}

int dmt_medium_info(dmt_ctx* ctx, int* active, float* sigma_t, float* albedo3, float* g, float* box_min3, float* box_max3) {
  if (!ctx) return DMT_ERR_INVALID;
  MediumParams const& m = ctx->medium.p;
  if (active) *active = ctx->medium.active() ? 1 : 0;
  if (sigma_t) *sigma_t = m.sigmaT;
  if (g) *g = m.g;
  for (int i = 0; i < 3; ++i) {
    if (albedo3) albedo3[i] = m.albedo[i];
    if (box_min3) box_min3[i] = m.lo[i];
    if (box_max3) box_max3[i] = m.hi[i];
  }
  return DMT_OK;
}

int dmt_set_medium_spectrum(dmt_ctx* ctx, const float* extinction3, const float* emission3) {
  if (!ctx) return DMT_ERR_INVALID;
  if (char const* const why = mediumSpectrumArgsError(extinction3, emission3)) return mediumRefused(ctx, "dmt_set_medium_spectrum", why);
  MediumState::Spectrum& s = ctx->medium.spectrum;
  s.have = true;
  for (int i = 0; i < 3; ++i) s.e[i] = extinction3[i], s.le[i] = emission3[i];
  return DMT_OK;
}

int dmt_clear_medium_spectrum(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  ctx->medium.spectrum = MediumState::Spectrum{};
  return DMT_OK;
}

int dmt_medium_spectrum_info(dmt_ctx* ctx, int* present, float* extinction3, float* emission3, float* k3, int* ref_channel, int* active) {
  if (!ctx) return DMT_ERR_INVALID;
  MediumState const& m = ctx->medium;
  float k[3];
  int const ref = m.channelK(k);
  if (present) *present = m.spectrum.have ? 1 : 0;
  for (int i = 0; i < 3; ++i) {
    if (extinction3) extinction3[i] = m.spectrum.e[i];
    if (emission3) emission3[i] = m.spectrum.le[i];
    if (k3) k3[i] = k[i];
  }
  if (ref_channel) *ref_channel = ref;
  if (active) *active = m.spectrumActive() ? 1 : 0;
  return DMT_OK;
}

int dmt_set_medium_grid(dmt_ctx* ctx, const float* density, int nx, int ny, int nz) {
  return mediumGridUpload(ctx, "dmt_set_medium_grid", density, false, nx, ny, nz);
}

int dmt_set_medium_grid_device(dmt_ctx* ctx, const void* d_density, int nx, int ny, int nz) {
  return mediumGridUpload(ctx, "dmt_set_medium_grid_device", d_density, true, nx, ny, nz);
}

int dmt_clear_medium_grid(dmt_ctx* ctx) {
  if (!ctx) return DMT_ERR_INVALID;
  MediumState::Grid& g = ctx->medium.grid;
  if (g.have) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  g = MediumState::Grid{};
  return DMT_OK;
}

int dmt_medium_grid_info(dmt_ctx* ctx, int* present, int* dims3, int* support_min3, int* support_max3, uint64_t* positive, float* max_density, int* active) {
  if (!ctx) return DMT_ERR_INVALID;
  MediumState::Grid const& g = ctx->medium.grid;
  if (present) *present = g.have ? 1 : 0;
  for (int a = 0; a < 3; ++a) {
    if (dims3) dims3[a] = g.n[a];
    if (support_min3) support_min3[a] = g.imin[a];
    if (support_max3) support_max3[a] = g.imax[a];
  }
  if (positive) *positive = g.positive;
  if (max_density) *max_density = g.maxDensity;
  if (active) *active = ctx->medium.gridActive() ? 1 : 0;
  return DMT_OK;
}

// ---- the host twins of the device arithmetic: no context, DMT_ERR_INVALID without a message ------
int dmt_medium_segment(const float* box_min3, const float* box_max3, int n, const float* o3, const float* d3, const float* t_hit, float* seg2,
                       int32_t* hit) {
  if (!box_min3 || !box_max3 || n < 0 || !o3 || !d3 || !t_hit || !seg2 || !hit) return DMT_ERR_INVALID;
  if (!mediumBoxOk(box_min3, box_max3)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) hit[i] = medium_segment(o3 + 3 * i, d3 + 3 * i, t_hit[i], box_min3, box_max3, seg2 + 2 * i, seg2 + 2 * i + 1) ? 1 : 0;
  return DMT_OK;
}

int dmt_medium_values(int n, const uint32_t* h, const uint32_t* depth, float* u) {
  if (n < 0 || !h || !depth || !u) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) u[i] = medium_u(h[i], depth[i]);
  return DMT_OK;
}

int dmt_phase_hg(float g, int n, const float* cosine, float* eval, const float* wo3, const float* u2, float* wi3, float* pdf) {
  if (n < 0 || !(std::fabs(g) < 1.f)) return DMT_ERR_INVALID;
  if ((cosine != nullptr) != (eval != nullptr)) return DMT_ERR_INVALID;
  bool const sample = wo3 || u2 || wi3 || pdf;
  if (sample && !(wo3 && u2 && wi3 && pdf)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    if (eval) eval[i] = hg_eval(g, cosine[i]);
    if (sample) hg_sample(g, wo3 + 3 * i, u2[2 * i], u2[2 * i + 1], wi3 + 3 * i, pdf + i);
  }
  return DMT_OK;
}

int dmt_medium_grid_march(const float* box_min3, const float* box_max3, float sigma_t, int nx, int ny, int nz, const float* density, int n,
                          const float* o3, const float* d3, const float* t_end, const float* tau_target, float* tau, float* ts, int32_t* collided,
                          int32_t* steps) {
  if (n < 0 || !o3 || !d3 || !t_end || !tau_target || !tau || !ts || !collided || !steps || !box_min3 || !box_max3) return DMT_ERR_INVALID;
  MediumGridParams g;
  std::string why;
  if (mediumGridCallRecord(box_min3, box_max3, sigma_t, nx, ny, nz, density, g, why)) return DMT_ERR_INVALID;
  g.density = density;
  bool const empty = g.imin[0] > g.imax[0];  // no density > 0: nothing to march
  for (int i = 0; i < n; ++i) {
    MediumGridMarch r{0.f, 0.f, 0, 0};
    if (!empty) r = medium_grid_march(o3 + 3 * i, d3 + 3 * i, t_end[i], tau_target[i], sigma_t, box_min3, box_max3, g);
    tau[i] = r.tau, ts[i] = r.ts, collided[i] = r.collided, steps[i] = r.steps;
  }
  return DMT_OK;
}

int dmt_medium_spectrum_event(const float* k3, int n, const float* beta3, const uint32_t* h, const uint32_t* depth, const float* tau_seg,
                              int32_t* channel, int32_t* collided, float* tau_at, float* weight3) {
  if (n < 0 || !beta3 || !h || !depth || !tau_seg || !channel || !collided || !tau_at || !weight3) return DMT_ERR_INVALID;
  float q[3];
  if (mediumSpectrumCallRecord(k3, q)) return DMT_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    MediumSpectrumEvent const ev = medium_spectrum_event(q, beta3 + 3 * i, h[i], depth[i], tau_seg[i]);
    channel[i] = ev.channel, collided[i] = ev.collided, tau_at[i] = ev.tauAt;
    for (int c = 0; c < 3; ++c) weight3[3 * i + c] = ev.w[c];
  }
  return DMT_OK;
}

}  // extern "C"
