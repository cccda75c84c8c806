// camera_state.hpp -- what a context keeps for the camera side: the camera with its two matrices and the sampler set-up, the
// thin lens, the pixel filter with its table (4.21), the projection (4.22), and the film the launches accumulate into.  The layer's
// helpers and entry points are in camera_host.hpp.
//
// Part of dmt_hip.hip's translation unit, included once before dmt_ctx: it uses DevBuf, dmt_camera, CameraXf, SamplerParams,
// CameraExtra, FilterBin, float4 and RenderParams.
//
// Five records.  A new context holds the default values below.
//
//   record   setter                  cleared by                        survives
//   camera   dmt_set_camera          the next dmt_set_camera           every upload, dmt_update_vertices*, dmt_set_lens,
//            (cam, xf, sp, have)     (there is no clear call)          dmt_set_pixel_filter, dmt_film_*, a refused call
//   lens     dmt_set_lens            dmt_set_lens(0, any): radius 0    the same, and dmt_set_camera.  The distance given with
//            (lensR, lensD)          is the pinhole                    radius 0 is ignored: lensD keeps what the last radius
//                                                                      > 0 came with (1 in a new context)
//   filter   dmt_set_pixel_filter    dmt_set_pixel_filter(box, 0.5):   the same as the lens.  The table (knots) is written only
//            (kind, radius, param,   the default, inactive -- no       for another filter than the default and is KEPT, unread,
//            active, knots)          table is read, no warp            after a return to it: view() is null while inactive
//   project- dmt_set_projection      dmt_set_projection(PERSPECTIVE,   the same as the lens.  Refused (DMT_ERR_STATE) while the
//   ion      (projKind, projParam,   any): the default, no tail work   lens radius is > 0, as dmt_set_lens refuses a radius > 0
//            projA)                  of its own                        under another projection than the perspective one: the
//                                                                      two are never set together
//   film     dmt_set_camera at       the next dmt_set_camera at        every upload, dmt_set_lens, dmt_set_pixel_filter and a
//            another resolution      another resolution; zeroed by     dmt_set_camera of the SAME resolution, which keeps the
//            (own, zeroed);          dmt_film_clear                    buffers, own or bound, and every value in them
//            dmt_film_bind (the
//            caller's)
//
// The film.  `mean` / `m2` are the buffers in use: the context's own (ownMean / ownM2) or the caller's after dmt_film_bind.
// dmt_set_camera allocates and zeroes an own film only when the resolution CHANGES; that replaces a bound film too (the
// caller's buffers are of the old size) and drops the denoiser's temporal history (DenoiseState::dropHistory), which is of
// the old resolution.  dmt_film_bind needs a camera, drains the stream, frees the own film and takes the caller's pointers as
// they are, neither cleared nor checked for size.  dmt_film_device_ptrs reports the buffers in use: a bound pointer is the
// caller's own.
//
// What dmt_set_camera refreshes beside its own record: SurfaceState::texFoot, the camera footprint of the first-hit texture
// filter.  The launch layer's sampler table is planned per launch from film.w / film.h and the lens (launch_host.hpp).
//
// Draining.  A launch in flight holds the matrices, the sampler set-up and the lens by value in its kernel arguments, and the
// film's and the filter table's pointers.
//   dmt_set_pixel_filter  drains the stream before it replaces the table (DevBuf::assign copies in place when there is room);
//                         a return to the default and a refused call do not touch the stream
//   dmt_film_bind         drains the stream, then frees the own film
//   dmt_set_camera        calls no synchronise of its own.  At another resolution it moves the new buffers over the old own
//                         ones, whose DevBuf frees them with hipFree, and hipFree waits for the whole device; a BOUND film is
//                         given up without any wait (found, not fixed: DESIGN.md 8, item 11)
//   dmt_film_clear        enqueues its two memsets on the context's stream, in order with the launches
//   dmt_download_film     drains the stream and reads the fold's error flag before it copies
//   dmt_set_lens          touches no device memory
//   dmt_set_projection    touches no device memory: the kind and its factor travel by value in the kernel arguments
//
// Commit-last.  A refused call -- a null or 0 x 0 camera, a negative radius, a focus distance that is not > 0, a filter kind
// out of range, a radius outside (0, 8], a Gaussian whose sigma has no mass, dmt_film_bind of a null pointer or before a camera,
// a projection kind out of range, an orthographic height or a fisheye angle outside its range, a projection under a lens or a
// lens under a projection -- changes nothing but dmt_last_error.  dmt_set_camera makes and zeroes the new film before it commits anything, and
// dmt_set_pixel_filter sets kind / radius / param / active after the table's copy has succeeded.
#pragma once

namespace {

// The host-made factor of a projection (camera_ray_projection's `a`), in fp32 as include/dmt_hip.h states it; 0 where the
// model has none.
inline float projectionFactor(dmt_camera const& cam, int kind, float param) {
#pragma clang fp contract(off)
  if (kind == DMT_PROJECTION_ORTHOGRAPHIC) return param / (cam.sensor_size * 0.001f);
  if (kind == DMT_PROJECTION_FISHEYE) {
    float const W = float(cam.width), H = float(cam.height);
    return (param * 0.5f * (kPi / 180.0f)) / (0.5f * std::sqrt(W * W + H * H));
  }
  return 0.f;
}

struct CameraState {
  bool have = false;  // dmt_set_camera has run
  dmt_camera cam{};
  CameraXf xf{};       // what the kernels read as RenderParams::cam
  SamplerParams sp{};  // of the camera's resolution
  float lensR = 0.f, lensD = 1.f;  // thin lens (dmt_set_lens): radius 0 = pinhole
  // pixel filter (dmt_set_pixel_filter): box 0.5, the default, is inactive (no table, no warp)
  struct PixelFilter {
    int kind = DMT_FILTER_BOX;
    float radius = 0.5f, param = 0.f;
    bool active = false;
    DevBuf<FilterBin> knots;  // kFilterBins pairs while active (kept, unread, after a return to the default)
    FilterBin const* view() const { return active ? knots.get() : nullptr; }
  } filt;

  // projection (dmt_set_projection): perspective is the default.  projParam: the view height (orthographic) or the diagonal
  // field of view in degrees (fisheye), else 0
  int projKind = DMT_PROJECTION_PERSPECTIVE;
  float projParam = 0.f;
  // the factor camera_ray_projection reads, formed per use from the camera: k = height / sensor height (orthographic),
  // s = half the field of view in radians / half the film's diagonal in pixels (fisheye)
  float projA() const { return projectionFactor(cam, projKind, projParam); }

  // camera-side state read where a camera ray is made, as the probes pass it
  CameraExtra extra() const { return CameraExtra{lensR, lensD, filt.view(), filt.radius, projKind, projA(), float(cam.width), float(cam.height)}; }

  // the layer's part of the argument struct (baseParams).  camTail: non-zero when prepare_sample's cold tail has work
  void fill(RenderParams& P) const {
    P.cam = xf, P.sp = sp;
    P.lensRad = lensR, P.lensD = lensD;
    P.filtKnots = filt.view(), P.filtR = filt.radius;
    P.projKind = projKind, P.projA = projA(), P.projW = float(cam.width), P.projH = float(cam.height);
    // (a tabulated launch without a lens and under the perspective camera clears it: growLaunchBuffers)
    P.camTail = (lensR > 0.f || filt.active || projKind != DMT_PROJECTION_PERSPECTIVE) ? 1.f : 0.f;
  }
};

struct FilmState {
  DevBuf<float4> ownMean, ownM2;  // the context's own film; empty after dmt_film_bind
  float4* mean = nullptr;         // the buffers in use: the own ones, or the caller's
  float4* m2 = nullptr;
  int w = 0, h = 0;

  size_t bytes() const { return size_t(w) * size_t(h) * sizeof(float4); }
  // zero both buffers in use, in order with the stream's launches
  hipError_t clear(hipStream_t stream) const {
    hipError_t const e = hipMemsetAsync(mean, 0, bytes(), stream);
    return e != hipSuccess ? e : hipMemsetAsync(m2, 0, bytes(), stream);
  }
};

}  // namespace
