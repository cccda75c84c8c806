// medium_state.hpp -- what a context keeps for the medium layer: the participating medium (medium.hpp), its
// density grid (medium_grid.hpp; 4.18) and its spectrum (4.19).  The layer's device code is in medium_device.hpp, its
// helpers and entry points in medium_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, RenderParams, the kFeatMedium* bits
// and the records and arithmetic of medium.hpp and medium_grid.hpp.
//
// Three records, per context and part of no upload.  A new context and a cleared record hold the default values below.
// Each may be set without the others, in any order: a grid or a spectrum set first waits for its medium.
//
//   record     setter                         cleared by                   survives
//   p          dmt_set_medium                 dmt_clear_medium             every upload (dmt_upload_*, dmt_update_vertices*),
//                                                                          dmt_set_camera, a refused call
//   grid       dmt_set_medium_grid,           dmt_clear_medium_grid,       the same, and dmt_set_medium
//              dmt_set_medium_grid_device     dmt_clear_medium
//   spectrum   dmt_set_medium_spectrum        dmt_clear_medium_spectrum,   the same, and dmt_set_medium
//                                             dmt_clear_medium
//
// Derived at launch (fill), not stored, so that both follow dmt_set_medium:
//   from the current box      the grid's cell, invCell, slo and shi (medium_grid_derive)
//   from the current sigmaT   the channel extinctions k_c = fl32(sigmaT * e_c) (a product beyond the floats' range counts as
//                             the largest float), the reference channel m (the first largest k_c) and q_c = k_c / k_m
//                             (medium_spectrum_q).  A launch marches with k_m: RenderParams::medium.sigmaT is k_m then.
//
// Feature bits (features):
//   kFeatMedium           the extinction a launch marches with -- p.sigmaT, with a spectrum k_m -- is > 0, and the grid, if
//                         there is one, has a density > 0
//   kFeatMediumGrid       kFeatMedium, and a grid is present
//   kFeatMediumSpectrum   kFeatMedium, a spectrum is present, and the k_c are not all equal or some emission is not 0
// So three degenerate states launch simpler rows.  sigmaT == 0 (dmt_set_medium with 0, dmt_clear_medium, a new context) and
// a grid with no density > 0 (an empty medium) select the rows of a context without a medium, whatever else is present.  A
// spectrum with three equal k_c and zero emission selects the grey rows, at sigmaT = that k.  The *_info calls then report
// the record as present and not active.
//
// Draining.  A launch in flight holds p, the spectrum and everything derived by value in its kernel arguments, and reads
// the grid's densities from the context's array.  The calls that replace or release that array drain the stream first:
//   dmt_set_medium_grid          once its host scan has passed, before the copy: a refused upload does not touch the stream
//   dmt_set_medium_grid_device   once its arguments have passed; its copy and scan run on the stream and it drains again
//                                before it reads the scan's words
//   dmt_clear_medium_grid,       when a grid is present
//   dmt_clear_medium
// dmt_set_medium, dmt_set_medium_spectrum, dmt_clear_medium_spectrum and the *_info calls never drain it.
#pragma once

namespace {

struct MediumState {
  MediumParams p{};  // what the *_medium rows read as RenderParams::medium
  // what the *_medium_grid rows read as RenderParams::mediumGrid
  struct Grid {
    bool have = false;
    DevBuf<float> density;
    int32_t n[3] = {0, 0, 0}, imin[3] = {0, 0, 0}, imax[3] = {0, 0, 0};  // imin > imax without a density > 0
    uint64_t positive = 0;                                                // voxels with density > 0
    float maxDensity = 0.f;
  } grid;
  // what the *_rgb rows read as RenderParams::mediumSpectrum
  struct Spectrum {
    bool have = false;
    float e[3] = {1.f, 1.f, 1.f}, le[3] = {0.f, 0.f, 0.f};
  } spectrum;

  // the channel extinctions k_c, and the reference channel
  int channelK(float* k) const {
    int m = 0;
    for (int c = 0; c < 3; ++c) {
      float const x = p.sigmaT * spectrum.e[c];
      k[c] = x < 3.402823466e+38f ? x : 3.402823466e+38f;
      if (k[c] > k[m]) m = c;
    }
    return m;
  }
  // the extinction the launch marches with
  float sigmaT() const {
    float k[3];
    int const m = channelK(k);
    return spectrum.have ? k[m] : p.sigmaT;
  }
  bool active() const { return sigmaT() > 0.f && !(grid.have && grid.positive == 0); }
  bool gridActive() const { return active() && grid.have; }
  bool spectrumActive() const {
    if (!active() || !spectrum.have) return false;
    float k[3];
    channelK(k);
    return k[0] != k[1] || k[1] != k[2] || spectrum.le[0] != 0.f || spectrum.le[1] != 0.f || spectrum.le[2] != 0.f;
  }

  // the layer's part of the feature mask (featuresOf)
  uint32_t features() const { return (active() ? kFeatMedium : 0u) | (gridActive() ? kFeatMediumGrid : 0u) | (spectrumActive() ? kFeatMediumSpectrum : 0u); }

  // the layer's part of the argument struct (baseParams): a record that is not active leaves its fields zero
  void fill(RenderParams& P) const {
    if (!active()) return;
    P.medium = p, P.medium.sigmaT = sigmaT();
    if (gridActive()) {
      MediumGridParams& g = P.mediumGrid;
      g.density = grid.density.get();
      for (int a = 0; a < 3; ++a) g.n[a] = grid.n[a], g.imin[a] = grid.imin[a], g.imax[a] = grid.imax[a];
      medium_grid_derive(g, p.lo, p.hi);
    }
    if (spectrumActive()) {
      float k[3];
      int const m = channelK(k);
      for (int c = 0; c < 3; ++c) P.mediumSpectrum.q[c] = medium_spectrum_q(k[c], k[m]), P.mediumSpectrum.le[c] = spectrum.le[c];
    }
  }
};

}  // namespace
