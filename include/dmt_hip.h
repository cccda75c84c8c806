/* dmt_hip.h -- C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * Drop-in boundary for the reference's kernel-launch boundary (paths relative to
 * /root/reference/examples/triangles/, T/ = that directory, CC/ = T/cuda-core/):
 *
 *   reference interface                                          replaced by
 *   ------------------------------------------------------------ ---------------------------
 *   cudaInitDevice/cudaSetDevice/cudaStreamCreate                dmt_ctx_create / _destroy
 *     (T/megakernel/main.cu:135-136,264-265)
 *   triSoupFromTriangles (CC/public/cuda-core/host_utils.cuh:163) dmt_upload_triangles
 *   deviceBSDF           (host_utils.cuh:166)                    dmt_upload_bsdfs
 *   deviceLights         (host_utils.cuh:167-169)                dmt_upload_lights
 *   deviceCamera + allocateDeviceConstantMemory                  dmt_set_camera
 *     (host_utils.cuh:170, T/megakernel/megakernel.cuh:18)
 *   DeviceOutputBuffer::allocate/free (CC/public/cuda-core/types.cuh:175-193)
 *                                                                dmt_set_camera / dmt_film_clear /
 *                                                                dmt_film_bind
 *   copyHaltonOwenToDeviceAlloc (host_utils.cuh:159)             (none: sampler state is per-lane
 *                                                                registers, nothing to upload)
 *   pathTraceMegakernel<<<...>>>(..., sampleOffset, ...)         dmt_render
 *     (T/megakernel/megakernel.cuh:99-112, launch main.cu:141-155)
 *   cudaStreamSynchronize (main.cu:169)                          dmt_sync
 *   cudaMemcpyAsync D2H of mean / M2 (main.cu:202-205)           dmt_download_film
 *   triangleIntersectKernel (T/tests/triangle_intersect.cu:146)  dmt_test_triangle_intersect
 *
 * Record layouts are byte-identical to the reference so its host packers interoperate:
 *   BSDF  32 B  CC/public/cuda-core/bsdf.cuh:18-73
 *   Light 32 B  CC/public/cuda-core/light.cuh:10-49
 *   DeviceCamera 44 B  CC/public/cuda-core/types.cuh:101-109  (= dmt_camera below)
 *   TriangleSoup: one float4 per axis per triangle {c0,c1,c2,pad} + uint32 matId
 *                 (types.cuh:119-129)
 *   film: two row-major float4 planes, mean.xyz (w = 0) and M2.xyz with the sample count N
 *         in .w  (T/megakernel/megakernel.cuh:81-85, megakernel.cu:92-93)
 *
 * Ownership: the context owns all device memory; host pointers are borrowed for the call.
 * Errors: every call returns DMT_OK (0) or a DMT_ERR_* code; the library never exits the
 * process (the reference's CUDA_CHECK does, types.cuh:20-29).  A context is bound to one device
 * and one stream and is not thread-safe; contexts are independent (one per GPU).
 */
#ifndef DMT_HIP_H
#define DMT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmt_ctx dmt_ctx;

typedef struct dmt_camera {
  float dir[3];
  float pos[3];
  int32_t width;
  int32_t height;
  int32_t spp; /* kept for layout parity; dmt_render's spp argument is what is rendered */
  float focal_length; /* mm */
  float sensor_size;  /* mm */
} dmt_camera;

enum {
  DMT_OK = 0,
  DMT_ERR_INVALID = 1,   /* bad argument */
  DMT_ERR_HIP = 2,       /* a HIP runtime call failed; see dmt_last_error */
  DMT_ERR_STATE = 3,     /* call sequence error (e.g. render before upload) */
  DMT_ERR_NO_DEVICE = 4, /* no usable GPU */
};

enum {
  DMT_ACCEL_BRUTE_FORCE = 0, /* the reference's loop over all triangles */
  DMT_ACCEL_BVH = 1,         /* same closest hit (lowest index on ties), BVH traversal */
};

/* ---- lifetime ---------------------------------------------------------------------------- */
int dmt_ctx_create(int device_ordinal, dmt_ctx** out);
int dmt_ctx_destroy(dmt_ctx* ctx);
/* last error text of the context; ctx == NULL returns the last dmt_ctx_create failure */
const char* dmt_last_error(const dmt_ctx* ctx);

/* ---- scene upload ------------------------------------------------------------------------ */
int dmt_upload_triangles(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs,
                         const uint32_t* mat_id, size_t count);
int dmt_upload_bsdfs(dmt_ctx* ctx, const void* bsdf32, uint32_t count);
/* A list of ONE record (either list) is read by the kernels through the scalar path: the uniform pick over one record is
 * record 0 for every draw, so the record is wave-uniform.  Films do not depend on it; DMT_UNIFORM_LIGHTS=0 in the environment
 * at context creation makes every list use the lane's pick and vector loads (A/B runs, tests). */
int dmt_upload_lights(dmt_ctx* ctx, const void* lights32, uint32_t count, const void* infinite32,
                      uint32_t infinite_count);
/* enabled = 1 when launches of this context pass the scalar path's switch to the kernels (RenderParams::uniformLights), 0 under
 * DMT_UNIFORM_LIGHTS=0.  Which lists take the path is the kernels' matter (one record; path_shade). */
int dmt_uniform_lights_info(dmt_ctx* ctx, int* enabled);
/* (re)computes camera transforms and sampler parameters; (re)allocates and zeroes the film when
 * the resolution changes */
int dmt_set_camera(dmt_ctx* ctx, const dmt_camera* cam);

/* ---- thin lens: depth of field (opt-in, beyond the reference) ------------------------ */
/* Context state, not part of dmt_camera: a lens of radius lens_radius >= 0 focused at focus_distance > 0, both in scene
 * units; the distance is measured along the viewing direction (the depth dmt_camera_project reports).  Radius 0, the
 * default, is the pinhole: every film is then bit-identical to one rendered without this call, and the distance is ignored.
 * The lens survives dmt_set_camera and scene uploads.  DMT_ERR_INVALID for a radius that is negative or not finite, and
 * with a radius > 0 for a distance that is not finite or not positive.
 *
 * Sample s of pixel (px, py), Halton index h, in fp32 without contraction:
 *   pCamera = cameraFromRaster (fx, fy, 0)               (fx, fy) the sample's film position, as for the pinhole
 *   ft = D / pCamera.z;  pf = (pCamera.x ft, pCamera.y ft, D)            the point in focus
 *   l  = R sample_uniform_disk(u10, u11)
 *   o  = renderFromCamera point(l.x, l.y, 0);  d = normalize(renderFromCamera vector(pf.x - l.x, pf.y - l.y, pf.z))
 * with (u10, u11) = Halton dimensions 10 and 11 of h: Owen-scrambled radical inverses in bases 31 and 37.  The path's own
 * dimensions 2..9 do not move: a lens changes which ray a sample traces and nothing else about the sample.  Every render
 * path traces these rays (dmt_render, its sampler table, the wavefront form, dmt_render_adaptive), and so does the
 * feature pass dmt_render_aovs, whose planes therefore blur where the image blurs.
 * Two things keep the pinhole: dmt_denoise_temporal's motion vectors, the projection of a surface point under both
 * frames' cameras, which is the projection through the lens centre and stays correct (a change of lens does not reset
 * the history); and the ray differentials of dmt_texture_footprint and of the first-hit texture filter. */
int dmt_set_lens(dmt_ctx* ctx, float lens_radius, float focus_distance);
int dmt_lens_info(dmt_ctx* ctx, float* lens_radius, float* focus_distance);
/* host only (no GPU): the serial twin of the device's camera rays.  Rays (o3, d3: n x 3) of samples ss of pixels
 * (pxs, pys) of the camera under the given lens (radius 0: the pinhole rays), and lens2 (n x 2) = (u10, u11).  The lens
 * values are the device's bit for bit; the rays use the host's division, square root, sine and cosine.
 * DMT_ERR_INVALID for a pixel outside the frame, a negative sample, or lens arguments dmt_set_lens would refuse. */
int dmt_lens_rays(const dmt_camera* cam, float lens_radius, float focus_distance, int n, const int32_t* pxs, const int32_t* pys,
                  const int32_t* ss, float* o3, float* d3, float* lens2);
/* autofocus: traces the pinhole ray through the continuous film coordinates (fx, fy) (dmt_camera_project's) under the
 * current accel mode; *distance = the hit's depth along the viewing direction, what dmt_set_lens takes as focus_distance.
 * DMT_ERR_STATE when the ray leaves the scene.  Synchronous. */
int dmt_focus_distance_at(dmt_ctx* ctx, float fx, float fy, float* distance);

/* ---- pixel reconstruction filter, importance-sampled per sample (opt-in, beyond the reference) ---- */
/* Context state beside the camera, like the lens: it survives dmt_set_camera and scene uploads.  The filter is separable,
 * f(x, y) = f1(x) f1(y), with a radius in pixels.  Kinds: box; tent (triangle); Gaussian, pbrt-v4's max(0, G(x) - G(radius))
 * with param = sigma; the four-term Blackman-Harris window.  param is ignored by the other kinds.
 * DMT_ERR_INVALID, and the state untouched, for an unknown kind, a radius that is not finite, not > 0 or above 8, and for a
 * Gaussian a sigma that is not finite or not > 0 (or so far above the radius that the profile has no mass in float64).
 * The default, box with radius 0.5, is inactive: the same kernels run, nothing is allocated, and every film is
 * byte-identical to one of a context that never saw this call.
 *
 * Filter importance sampling.  The filter moves where a sample's camera ray goes and nothing else: no splatting, every
 * sample's weight is exactly 1, every pixel is still owned by one tile.  The sample's film jitter r = pixel2d in [0,1)^2
 * becomes, per axis,   r' = 0.5 + radius * W(r),   and the film position is formed from r' as from r:
 * ((r' - 0.5) + 0.5) + pixel.  Positions outside the film are ordinary rays.  W: [0,1) -> [-1,1] is the inverse CDF of f1
 * over x / radius, tabulated on the host (f1 integrated in float64) as 257 float32 knots at u = i / 256 with W(0) = -1,
 * W(1) = 1, antisymmetric about u = 1/2, and evaluated in fp32 without contraction as
 *   i = floor(256 u);  t = 256 u - i;  W = fmaf(t, knot[i+1] - knot[i], knot[i])
 * by the device and by dmt_pixel_filter_positions alike, from the same bytes: they agree bit for bit.
 * THE RENDERED FILTER IS THE TABULATED ONE: 256 bins of equal mass with constant density inside each bin.  Its CDF equals
 * the analytic CDF at every knot and deviates from it between knots (DESIGN.md 4.21 records by how much, about 1e-3).
 * W is monotone, so the Halton stratification of a pixel's samples survives.  Sampler dimensions 2..9, the lens's 10 and 11
 * and the shutter's 12 do not move.  Every render path traces the filtered positions (dmt_render, its sampler table, whose
 * jitter plane then holds r', the wavefront form, dmt_render_adaptive, the motion rows), and so do the feature pass
 * dmt_render_aovs and the trace probes.  What keeps the pixel centre or the pinhole reading, as under the lens:
 * dmt_denoise_temporal's reprojection (a change of filter does not reset the history), dmt_camera_project,
 * dmt_texture_footprint and the first-hit texture filter, dmt_focus_distance_at.  Signed filters (Mitchell, sinc) are
 * not offered: they need a per-sample weight in the film's fold. */
enum {
  DMT_FILTER_BOX = 0,
  DMT_FILTER_TENT = 1,
  DMT_FILTER_GAUSSIAN = 2, /* param = sigma, in pixels */
  DMT_FILTER_BLACKMAN_HARRIS = 3,
};
int dmt_set_pixel_filter(dmt_ctx* ctx, int kind, float radius, float param);
/* any output may be null; *active = 0 for the default (box, radius 0.5) */
int dmt_pixel_filter_info(dmt_ctx* ctx, int* kind, float* radius, float* param, int* active);
/* host only (no GPU): the 257 knots W(i / 256) of a filter dmt_set_pixel_filter would accept (the box's are 2u - 1) */
int dmt_pixel_filter_table(int kind, float radius, float param, float* knots257);
/* host only (no GPU): the film positions (xy2: n x 2) of samples ss of pixels (pxs, pys) of a width x height frame under the
 * filter; box with radius 0.5 gives the unfiltered positions.  The device's bit for bit (dmt_test_film_positions).
 * DMT_ERR_INVALID for a pixel outside the frame, a negative sample, or filter arguments dmt_set_pixel_filter would refuse. */
int dmt_pixel_filter_positions(int width, int height, int kind, float radius, float param, int n, const int32_t* pxs, const int32_t* pys,
                               const int32_t* ss, float* xy2);

/* ---- camera projections: orthographic, equirectangular, fisheye (opt-in, beyond the reference) ---- */
/* Context state beside the camera, like the lens and the filter: dmt_camera does not change, and the projection survives
 * dmt_set_camera and scene uploads.  A projection changes which ray a sample traces and nothing else about the sample, so
 * every kernel row runs under it (media, motion, cutouts, textures, the emitter tree, both accel modes), and every render
 * path traces its rays: dmt_render, its sampler table, the wavefront form, dmt_render_adaptive, the feature pass
 * dmt_render_aovs and the trace probes.  Perspective, the default, launches what it always launched: every film is
 * byte-identical to one of a context that never saw this call.
 *
 * param: the view height in scene units for orthographic (finite, > 0); the field of view across the film's DIAGONAL in
 * degrees for fisheye (finite, 0 < fov <= 360); ignored for perspective and equirect.  DMT_ERR_INVALID, and the state
 * untouched, for an unknown kind or a bad param.
 *
 * The models, in camera space (x right, y up, z forward; the world is z-up), for the continuous film position (fx, fy) of
 * a W x H film, fp32 without contraction; (cx, cy, focal) = cameraFromRaster (fx, fy, 0); every direction is normalised once.
 *   orthographic   k = param / (sensor_size 0.001f), formed once on the host
 *                  o = renderFromCamera point(cx k, cy k, 0);  d = the forward column of renderFromCamera
 *                  The film's height spans param scene units; with param = sensor D / focal it frames depth D as the
 *                  perspective camera does.  inverse: fx = (c.x / k - tx) ipx, fy = (c.y / k - ty) ipy, depth = c.z
 *   equirect       u = fx / W, v = fy / H, lon = (u - 0.5) 2 pi, lat = (0.5 - v) pi          (the full sphere)
 *                  d_cam = (cos lat sin lon, sin lat, cos lat cos lon);  o = the camera position
 *                  The film's centre looks along dir, the top row up, the left and right edges meet behind the camera.
 *                  inverse: lon = atan2(c.x, c.z), lat = atan2(c.y, hypot(c.x, c.z)), depth = |c|
 *   fisheye        x = fx - W / 2, y = H / 2 - fy, r = sqrt(x x + y y), theta = r s          (equidistant, full frame)
 *                  s = (fov / 2 in radians) / (sqrt(W W + H H) / 2), formed once on the host: the fov is reached at the
 *                  film's corners, so every pixel has a ray
 *                  d_cam = (sin theta x / r, sin theta y / r, cos theta), (0, 0, 1) at r = 0;  o = the camera position
 *                  inverse: theta = atan2(hypot(c.x, c.y), c.z), r = theta / s, depth = |c|
 * A wide pixel filter can push (fx, fy) slightly outside the film; the angles then leave their nominal range by a fraction
 * of a pixel's worth.  Nothing is clamped.
 *
 * What another projection than the perspective one refuses, each with DMT_ERR_STATE and a message that names
 * dmt_set_projection, and nothing else changed: a lens (dmt_set_projection while the lens radius is > 0, and dmt_set_lens
 * with a radius > 0 under the projection); a render whose kernels use the first-hit texture filter, whose footprints are
 * the pinhole's differentials; a render, or a trace probe, of one of the two kernel rows that are compiled without the
 * projection's ray because they spill a register more with it: a scene under an env map with no other
 * surface feature in brute-force mode (set DMT_ACCEL_BVH), and an env map with the BVH and the light tree (use the uniform
 * pick); dmt_denoise and dmt_denoise_temporal, whose depth scale and reprojection are the pinhole's
 * (the temporal history is left as it was); dmt_focus_distance_at.  Not offered: partial panoramas, circular fisheyes with
 * dead pixels, camera motion, the PBRT front end's other cameras. */
enum {
  DMT_PROJECTION_PERSPECTIVE = 0,
  DMT_PROJECTION_ORTHOGRAPHIC = 1, /* param = the view height, in scene units */
  DMT_PROJECTION_EQUIRECT = 2,
  DMT_PROJECTION_FISHEYE = 3,      /* param = the field of view across the film's diagonal, in degrees */
};
int dmt_set_projection(dmt_ctx* ctx, int kind, float param);
/* either output may be null; *param = 0 for the kinds that ignore it */
int dmt_projection_info(dmt_ctx* ctx, int* kind, float* param);
/* host only (no GPU): the serial twin of the device's rays.  Rays (o3, d3: n x 3) through the continuous film positions
 * xy2 (n x 2; (fx, fy) as dmt_camera_project defines them) of the camera under the projection; perspective gives the
 * pinhole rays.  The device's arithmetic with the host's division, square root, sine and cosine.
 * DMT_ERR_INVALID for arguments dmt_set_projection would refuse. */
int dmt_projection_rays(const dmt_camera* cam, int kind, float param, int n, const float* xy2, float* o3, float* d3);
/* host only (no GPU): the inverse, render-space points p3 (n x 3) -> film positions xy2 (n x 2) and depth (n): the
 * camera-space z for perspective (dmt_camera_project) and orthographic, the distance from the camera for the angular models. */
int dmt_projection_project(const dmt_camera* cam, int kind, float param, int n, const float* p3, float* xy2, float* depth);

/* ---- motion blur: linear vertex motion over a shutter interval (opt-in, beyond the reference) ---- */
/* Keys.  Key 0 is the positions the context holds (dmt_upload_triangles, dmt_update_vertices*).  Key 1 is a second position
 * set for the same triangles (dmt_set_motion).  Motion is active exactly when key 1 is present; without it every film is
 * byte for byte what it was before these calls existed, whatever the shutter.
 *
 * Time of a sample.  Sample s of pixel (px, py) has Halton index h.  It draws u12 = the Owen-scrambled radical inverse of h
 * in base 41 (Halton dimension 12; the lens holds 10 and 11, the path 2..9, none of which moves) and its time is
 *   t = fmaf(close - open, u12, open)                          [open, close] the shutter, default [0, 1]
 * Every ray of that sample's path sees the scene at t: the camera ray, the bounce rays and the shadow rays.  open == close
 * pins every sample to one time.
 *
 * The triangle at time t, once for every path.  A = the key-0 intersection record (p0, e0 = p1 - p0, e1 = p2 - p0 in fp32),
 * B = the same record of key 1, D = B - A component by component in fp32 (made at dmt_set_motion).  The nine floats of the
 * tested triangle are fmaf(t, D, A).  Brute force and the BVH rebuild it from the same two records with the same fmaf, so
 * they return bit-identical hits (tri, t, u, v), as they do for static triangles.  For the post-hit record the vertices are
 *   p_i(t) = fmaf(t, P1_i - P0_i, P0_i)
 * and the geometric normal is normalize(cross(e1, e0)) of those vertices, in the order of operations of the static record,
 * with the device's arithmetic (no contraction, v_rsq_f32).  Material ids and everything else come from key 0.
 *
 * The BVH.  Launches with key 1 traverse a second tree, built by the host SAH builder over each triangle's UNION box of both
 * keys -- whatever dmt_set_accel_build says; the device builder and the refit know one key -- when key 1 arrives under
 * DMT_ACCEL_BVH or a BVH launch first needs it.  The static tree stays as it is.
 *
 * Scope.  Motion has the plain and the env-map megakernel rows, under both accel modes: dmt_render (partitions, chunks),
 * dmt_render_adaptive, dmt_test_trace_samples / dmt_test_trace_log, and the feature pass dmt_render_aovs, which traces at the
 * samples' times so its planes blur where the film does.  Motion launches compute their samples (no sampler table), so
 * films do not depend on dmt_set_sampler_table.  The brute-force pass of a motion launch is the plain loop over every
 * triangle (the culled clusters' bounds are of key 0).  Refused with DMT_ERR_STATE and a message that names the
 * combination: motion with emissive triangles, with image textures or blend materials, with either light tree, with the
 * first-hit texture filter, with dmt_render_stats / dmt_render_profile, with the wavefront BVH strategy.
 * Left on key 0: dmt_focus_distance_at, dmt_test_closest_hit, and the temporal denoiser's motion vectors. */
/* Key 1.  Layout as dmt_upload_triangles (4 floats per triangle and axis).  DMT_ERR_STATE before any upload, DMT_ERR_INVALID
 * when count differs from the uploaded triangle count or a position is not finite.  Synchronises the stream first.
 * Dropped by dmt_upload_triangles, dmt_update_vertices and dmt_update_vertices_device: the positions it was a motion from
 * are gone. */
int dmt_set_motion(dmt_ctx* ctx, const float* xs1, const float* ys1, const float* zs1, size_t count);
/* drops key 1; every film is then byte for byte what it was before dmt_set_motion */
int dmt_clear_motion(dmt_ctx* ctx);
/* the shutter: finite 0 <= open <= close <= 1, DMT_ERR_INVALID otherwise.  Survives scene uploads and dmt_set_camera, like
 * the lens.  No effect without key 1. */
int dmt_set_shutter(dmt_ctx* ctx, float open, float close);
/* *keys = 0 before an upload, 1, or 2 with key 1; the shutter; the motion tree's node and pair count and the host time of
 * its build in ms (zeros while no BVH launch has needed it).  Any pointer may be null. */
int dmt_motion_info(dmt_ctx* ctx, int* keys, float* open, float* close, uint32_t* tree_nodes, uint32_t* tree_pairs, double* tree_build_ms);
/* host only (no GPU): the times of samples ss of pixels (pxs, pys) of a width x height frame under the shutter, the device's
 * bit for bit (integer arithmetic and explicit fmaf).  DMT_ERR_INVALID for a pixel outside the frame, a negative sample or
 * a shutter dmt_set_shutter would refuse. */
int dmt_shutter_times(int width, int height, float open, float close, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss,
                      float* t);
/* host only (no GPU): the vertices at time t (finite), p_i(t) above, the device's bit for bit; layout as the inputs */
int dmt_motion_positions(const float* xs0, const float* ys0, const float* zs0, const float* xs1, const float* ys1, const float* zs1,
                         size_t count, float t, float* xs, float* ys, float* zs);
/* host only (no GPU): builds the motion tree of the two keys and checks dmt_bvh_validate's invariants against BOTH: every
 * decoded child box contains the vertices below it at key 0 and at key 1.  DMT_ERR_STATE when one fails. */
int dmt_motion_bvh_validate(const float* xs0, const float* ys0, const float* zs0, const float* xs1, const float* ys1, const float* zs1,
                            size_t count, int* node_count, int* pair_count, int* depth);
/* ---- smooth shading: per-vertex normals interpolated at every hit (opt-in, beyond the reference) ---- */
/* Without vertex normals every surface is faceted: the shading normal ns is the triangle's geometric normal unless a normal
 * map moves it.  With them ns is interpolated at the hit; the geometric normal ng keeps every role it has (ray offsets, the
 * ng argument of the BSDF routines, light sampling, texture footprints).  Without an upload every film is byte for byte
 * what it was before these calls existed.
 *
 * The record.  16 bytes per triangle, read by one 16-byte load per hit: the three normals in the 2 x 16 bit octahedral
 * mapping of the light records (what the device's decoder inverts; the reference's encoder clamps a component to [0, 1]
 * before rounding and so cannot carry a normal: the record is written with the clamp at 65535) and a flags word, bit 0 =
 * smooth.  The round trip moves a normal by less than 1e-4 rad.
 *
 * The shading normal at a hit with barycentrics (bu, bv) of vertices 1 and 2, for the geometric normal ngFacing already
 * flipped against the ray:  n = (1 - bu - bv) n0 + bu n1 + bv n2, normalised, and negated if dot(n, ngFacing) < 0 -- it
 * lives in the hemisphere of the ray-facing geometric normal whichever way the file's normals and winding point.  A flat
 * triangle, and a sum whose squared length is not finite or below 1e-12, give ngFacing bit for bit.  A normal map perturbs
 * the smooth normal: its tangent frame is taken around it.  No terminator softening.
 *
 * Scope.  Vertex normals have the plain, env-map and texture megakernel rows with and without the env map (_vn, _env_vn,
 * _tex_vn, _env_tex_vn and their _bvh twins): dmt_render with the sampler table as before, dmt_render_adaptive,
 * dmt_test_trace_samples / dmt_test_trace_log, and dmt_render_aovs, whose normal plane then holds the smooth normal.
 * Refused with DMT_ERR_STATE and a message that names the combination: vertex normals with emissive triangles, with blend
 * materials, with either light tree, with the first-hit texture filter, with motion blur, with the wavefront BVH strategy,
 * with dmt_render_stats / dmt_render_profile. */
/* n9: 9 floats per triangle, the normals at vertices 0, 1, 2 in the vertex order of dmt_upload_triangles; any length, they
 * are normalised here.  A triangle whose nine floats are all exactly zero is flat and keeps its geometric normal, so one
 * scene can mix flat walls and smooth meshes.  DMT_ERR_STATE before any upload of triangles; DMT_ERR_INVALID when count
 * differs from the uploaded triangle count, or when any other normal is not finite or shorter than 1e-6 (the message names
 * the triangle).  Synchronises the stream first.
 * Dropped by dmt_upload_triangles.  KEPT by dmt_update_vertices and dmt_update_vertices_device, like UVs, materials and
 * emissive triangles: a caller who deforms the mesh uploads the normals of the new shape. */
int dmt_upload_vertex_normals(dmt_ctx* ctx, const float* n9, size_t count);
/* drops the normals; every film is then byte for byte what it was before dmt_upload_vertex_normals */
int dmt_clear_vertex_normals(dmt_ctx* ctx);
/* *triangles = the number of records (0 without normals), *smooth_triangles = those not flat.  Either pointer may be null. */
int dmt_vertex_normals_info(dmt_ctx* ctx, uint64_t* triangles, uint64_t* smooth_triangles);
/* host only (no GPU): vertex normals for a soup that comes without any (layout of dmt_upload_triangles in, of
 * dmt_upload_vertex_normals out).  Corners with bit-equal positions are welded.  A corner's normal is the normalised sum of
 * the stored face normals, normalize(cross(e1, e0)) in fp32, of the triangles around that position, each weighted by its
 * interior angle at that corner; only faces whose normal lies within crease_degrees (finite; clamped to [0, 180]) of the
 * corner's own face contribute.  Zero-area triangles contribute nothing and come out flat (nine zeros). */
int dmt_smooth_normals(const float* xs, const float* ys, const float* zs, size_t count, float crease_degrees, float* n9_out);

/* ---- alpha cutouts: opacity textures tested at every ray-triangle hit (opt-in, beyond the reference) ---- */
/* Binary cutout.  A material may name one of the uploaded textures as its opacity texture.  A hit on a triangle of such a
 * material counts only if the texture's A channel at the hit passes a cutoff; otherwise the ray goes on as if the triangle
 * were not there.  Fractional or stochastic transparency and coloured transmission are out of scope.  Without the upload
 * every film, tree and probe result is byte for byte what it was before these calls existed.
 *
 * The lookup.  With (bu, bv) the hit's barycentrics and (u_i, v_i) the triangle's UVs of dmt_upload_textures, in fp32 with
 * every operation rounded (nothing contracted):
 *   w0 = (1 - bu) - bv;   s = (w0*u0 + bu*u1) + bv*u2;   t = (w0*v0 + bu*v1) + bv*v2
 *   x = s*w - 0.5, y = t*h - 0.5 (each clamped to +-2^30), x0 = floorf(x), tx = x - x0 (y alike), texels mirror-wrapped
 *   ax0 = a00*(1 - tx) + a10*tx;  ax1 = a01*(1 - tx) + a11*tx;  alpha8 = ax0*(1 - ty) + ax1*ty
 * -- the arithmetic of the level-0 bilinear colour lookup, on the raw A bytes a_xy as floats in [0, 255], with no division.
 * The test: the hit passes iff alpha8 >= cutoff8, cutoff8 = cutoff * 255.f computed once on the host.  No reciprocal and no
 * contraction: dmt_opacity_eval (host) and a plain float32 restatement equal the device bit for bit.
 *
 * Rays.  Closest hit = the minimum t over valid AND passing hits, the lowest original index on equal t, as for solid
 * triangles.  A shadow ray is occluded iff some valid and passing hit has t < its length.  Every ray of a path sees
 * cutouts: camera, bounce and shadow rays.  The pass decision is a function of (triangle, bu, bv) alone, which brute force
 * and the BVH produce bit for bit, so their hits and films stay bit-identical.  The trees do not change (boxes only
 * cull): dmt_accel_download, the refit and the device builder are byte-identical with and without opacity.
 *
 * Scope.  Cutouts run on the four texture megakernel rows (plain / env map, brute force / BVH): dmt_render (partitions,
 * chunks), dmt_render_adaptive, dmt_test_trace_samples / dmt_test_trace_log and dmt_render_aovs, whose planes see through
 * holes.  The brute-force pass of a cutout launch is the plain loop over every triangle.  Refused with DMT_ERR_STATE and a
 * message that names opacity and the other side: blend materials, the first-hit texture filter, vertex normals.  Refused as
 * for any textured scene, with those messages: emissive triangles, motion blur, dmt_render_stats / dmt_render_profile.  The
 * wavefront strategy and the light trees behave as for a textured scene (the megakernel runs; the uniform light pick).
 * Left on solid geometry: dmt_focus_distance_at, dmt_test_closest_hit, and the temporal denoiser's motion vectors. */
/* Per BSDF the index of an uploaded texture whose A channel is the material's opacity, 0xFFFFFFFF = opaque.
 * DMT_ERR_STATE before triangles, BSDFs and textures (with one UV triple per triangle) are uploaded.  DMT_ERR_INVALID for a
 * count that differs from the uploaded BSDF count, a texture index out of range, an opacity texture wider or taller than
 * 65535 texels, a cutoff that is not finite or outside [0, 1], or a triangle of a cutout material with a UV that is not
 * finite or has |uv| > 2^20 (texel coordinates then stay inside int on host and device alike; the message names the
 * triangle).  A refused upload leaves the context as it was.  Synchronises the stream first.  Dropped by
 * dmt_upload_triangles, dmt_upload_bsdfs and dmt_upload_textures; kept by dmt_update_vertices[_device], like the UVs. */
int dmt_upload_opacity(dmt_ctx* ctx, const uint32_t* mat_opacity_tex, uint32_t bsdf_count, float cutoff);
/* drops the opacity; every film is then byte for byte what it was before dmt_upload_opacity */
int dmt_clear_opacity(dmt_ctx* ctx);
/* triangles and materials that carry an opacity texture, and the cutoff; all zero without opacity.  Any pointer may be null. */
int dmt_opacity_info(dmt_ctx* ctx, uint64_t* cutout_triangles, uint32_t* cutout_materials, float* cutoff);
/* host only (no GPU): the serial twin of the device lookup, bit for bit.  Textures as dmt_upload_textures takes them (rgba8,
 * desc3 = {first texel, width, height} per texture); case i looks texture tex[i] up for a triangle with UVs uv6[6i..] at
 * barycentrics (bu[i], bv[i]): alpha8_out[i], and pass_out[i] = alpha8 >= cutoff * 255.f ? 1 : 0.  DMT_ERR_INVALID for a
 * descriptor outside the texel array or beyond 65535 texels a side, a texture index out of range, or a cutoff
 * dmt_upload_opacity would refuse. */
int dmt_opacity_eval(const uint8_t* rgba8, uint64_t texel_count, const int32_t* desc3, uint32_t texture_count, int n, const int32_t* tex,
                     const float* uv6, const float* bu, const float* bv, float cutoff, float* alpha8_out, uint8_t* pass_out);
/* ---- participating medium: homogeneous fog in a box, sampled in-path (opt-in, beyond the reference) ---- */
/* The medium.  One per context: an extinction coefficient sigma_t >= 0 per scene unit (grey unless dmt_set_medium_spectrum colours it), a single-scattering albedo in
 * [0, 1] per channel, the Henyey-Greenstein asymmetry g with |g| < 1, and a finite axis-aligned box min < max.  It is active
 * exactly when it has been set with sigma_t > 0: dmt_set_medium with sigma_t == 0 and dmt_clear_medium both leave the
 * context on the kernels it launches without these calls, and every film is then byte for byte what it was.  The medium
 * belongs to no upload: scene uploads, vertex updates and dmt_set_camera leave it as it is.
 *
 * Per path segment, origin o, unit direction d, ending at t_hit = dot(hit.pos - o, d), +inf on a miss:
 *   [t0, t1] = the clip of the ray against the box, intersected with [0, t_hit] (dmt_medium_segment states the arithmetic);
 *   empty (not t0 < t1): nothing changes for the segment.  Otherwise
 *   s = -log1p(-u) / sigma_t with u = medium_u(h, depth), a hash of the sample's Halton index h and the path's depth:
 *       x = mix_bits32(h ^ mix_bits32(0x9E3779B9 * (depth + 1))), u = (x >> 8) * 2^-24 in [0, 1)  (the sampler's mix_bits32);
 *   t0 + s < t1: the path scatters at p = o + (t0 + s) d instead of reaching the surface or the miss; otherwise it goes on
 *   with beta untouched and the sampler's dimensions unmoved -- the chance of getting through is the transmittance, which
 *   is why emission seen through the fog needs no factor and the MIS weights stand as they are.
 * A scatter vertex ends the path at depth >= max_depth or with an all-zero albedo.  Otherwise it draws what a surface
 * bounce draws, in its order (1 + 2 numbers for the light, 2 + 1 for the bounce, the roulette number under the surface's
 * condition).  NEE: the light is chosen as at a surface (uniform pick; half env map in the env rows), sampled as from a point
 * without a normal, f = albedo p_HG(dot(wo, wi)) with material pdf p_HG and no cosine, combined with the light's pdf by the
 * surface code's expressions; the shadow ray starts at p itself.  Bounce: wi by pbrt's HG inversion (isotropic below
 * |g| = 1e-3), beta *= albedo, then roulette and depth + 1 as at a surface.  wo = -d, and
 *   p_HG(c) = (1 - g^2) / (4 pi (1 + g^2 + 2 g c)^1.5),   c = dot(wo, wi) = -1 straight on.
 * Every NEE contribution of a medium launch, made at a surface or at a scatter vertex, is multiplied by
 * exp(-sigma_t len), len = the length of its shadow segment inside the box (the same clip with t_hit = the ray's length).
 *
 * Scope.  The medium has the plain and the env-map megakernel rows under both accel modes, whose films agree bit for bit:
 * dmt_render (partitions, chunks, the sampler table, a lens), dmt_render_adaptive, dmt_test_trace_samples.  Refused with
 * DMT_ERR_STATE and a message that names the combination: the medium with emissive triangles, with image textures or blend
 * materials, with either light tree, with the first-hit texture filter, with motion blur, with vertex normals, with
 * opacity textures, with the wavefront BVH strategy, with dmt_render_stats / dmt_render_profile, and dmt_render_aovs /
 * dmt_test_trace_log (the feature pass and the path log know surfaces only). */
/* DMT_ERR_INVALID for sigma_t negative or not finite, an albedo outside [0, 1], |g| >= 1, or a box that is not finite or
 * has min >= max on an axis; a refused call leaves the medium as it was.  Takes effect with the next launch. */
int dmt_set_medium(dmt_ctx* ctx, float sigma_t, const float* albedo3, float g, const float* box_min3, const float* box_max3);
int dmt_clear_medium(dmt_ctx* ctx);
/* the record as it was set (zeros after dmt_clear_medium) and *active = 1 iff sigma_t > 0.  Any pointer may be null. */
int dmt_medium_info(dmt_ctx* ctx, int* active, float* sigma_t, float* albedo3, float* g, float* box_min3, float* box_max3);
/* host only (no GPU): the clip, the device's bit for bit while no intermediate is subnormal (the device flushes those).
 * fp32 without contraction.  t0 = 0, t1 = t_hit; per axis a in x, y, z order: |d[a]| < 2^-100 (parallel): the interval is
 * emptied when o[a] < min[a] or o[a] > max[a] and left alone otherwise; else inv = fl32(1 / d[a]) correctly rounded,
 * ta = (min[a] - o[a]) * inv, tb = (max[a] - o[a]) * inv, t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb)).
 * seg2[i] = (t0, t1) and hit[i] = t0 < t1 for ray i (o3, d3: n x 3; t_hit[i] >= 0, may be +inf). */
int dmt_medium_segment(const float* box_min3, const float* box_max3, int n, const float* o3, const float* d3, const float* t_hit, float* seg2,
                       int32_t* hit);
/* host only: u[i] = medium_u(h[i], depth[i]), the device's bit for bit */
int dmt_medium_values(int n, const uint32_t* h, const uint32_t* depth, float* u);
/* host only: Henyey-Greenstein in fp32.  Evaluation (cosine and eval both given, or both null): eval[i] = p_HG(cosine[i]).
 * Sampling (wo3, u2, wi3, pdf all given, or all null): wi3[i] around the unit vector wo3[i] for the numbers u2[i], and
 * pdf[i] = p_HG at the sampled cosine.  The device's operations with the host's sine, cosine, division and square root. */
int dmt_phase_hg(float g, int n, const float* cosine, float* eval, const float* wo3, const float* u2, float* wi3, float* pdf);
/* ---- heterogeneous medium: a density grid in the medium's box, marched exactly (opt-in) ---- */
/* The grid.  nx * ny * nz float32 densities, x fastest, then y, then z, attached to the context's medium and filling its box
 * [min, max].  The extinction in voxel v is sigma_t * density[v], looked up nearest-neighbour (piecewise constant); albedo, g
 * and the box stay those of dmt_set_medium.  Limits: every density finite and >= 0, 1 <= n <= 512 per axis, at most 2^26
 * voxels.
 *
 * Active.  The grid rows (*_medium_grid) run exactly when the medium is active (sigma_t > 0) and a grid is present with at
 * least one density > 0.  Medium active, no grid: the *_medium rows, byte for byte.  A grid without a density > 0 is an empty
 * medium: the plain rows, as for sigma_t = 0, and dmt_medium_info reports the medium as not active.  The grid belongs to no
 * scene upload: uploads, vertex updates and dmt_set_camera keep it, dmt_set_medium keeps it (the same grid under a new box
 * or sigma_t), dmt_clear_medium and dmt_clear_medium_grid drop it.  It may be set before dmt_set_medium.
 *
 * Derived (host, fp32, no contraction; made again from the box of every launch): cell[a] = (max[a] - min[a]) / n[a],
 * invCell[a] = fl32(1 / cell[a]) correctly rounded, plane(a, i) = i == n[a] ? max[a] : min[a] + float(i) * cell[a] (multiply,
 * then add), and the support box: per axis the inclusive index range [imin, imax] of the voxels with density > 0 and its
 * planes plane(a, imin), plane(a, imax + 1).
 *
 * The march of the ray o + t d over [0, t_end] up to the optical depth tau_target (dmt_medium_grid_march is the host twin;
 * fp32, no contraction, one order of operations):
 *   1. [t0, t1] = the clip of dmt_medium_segment against the SUPPORT box, intersected with [0, t_end].  Empty: tau = 0, no
 *      collision, steps = 0.
 *   2. Per axis i = clamp(floorf((o + t0 * d - min) * invCell), imin, imax).  |d| < 2^-100: the axis never steps; otherwise
 *      inv = fl32(1 / d) correctly rounded and step = d > 0 ? +1 : -1.
 *   3. tc = t0, tau = 0; per iteration: tn[a] = (plane(a, i[a] + (step > 0)) - o[a]) * inv[a], +inf on a parallel axis (from the
 *      plane index every time, never accumulated); ax = the axis of the smallest tn, the lowest axis on a tie;
 *      te = tn[ax] < t1 ? tn[ax] : t1; seg = te - tc, 0 unless seg > 0; s = sigma_t * density[voxel]; dtau = s * seg.
 *      s > 0 and tau + dtau >= tau_target: collision at ts = min(tc + float(double(tau_target - tau) / double(s)), te), done.
 *      Otherwise tau += dtau, tc = max(tc, te); stop unless tn[ax] < t1; i[ax] += step, stop when that leaves [imin, imax].
 *   tau = the segment's optical depth when no collision happened; steps = iterations, at most nx + ny + nz.
 * In the grid rows a path segment ending at t_hit collides where the march with tau_target = -log1p(-medium_u(h, depth))
 * does, at p = o + ts d; everything after that point is dmt_set_medium's scatter vertex.  No collision: the path goes on
 * untouched.  Every NEE contribution is multiplied by exp(-tau) of its shadow segment (tau_target = +inf), unless tau == 0.
 * u == 0 gives target 0: the first voxel with s > 0 collides at its entry.
 *
 * Scope: as the medium's, and refused with the medium's messages. */
/* DMT_ERR_INVALID for sizes outside the limits or a density that is negative or not finite (the message names the voxel); a
 * refused call leaves the context as it was.  Synchronises the context's stream, then copies. */
int dmt_set_medium_grid(dmt_ctx* ctx, const float* density, int nx, int ny, int nz);
/* the same from device memory on the context's device (a torch tensor's data_ptr()): a device-to-device copy on the context's
 * stream, one kernel that reduces the support ranges and the invalid-value flag, one synchronous read-back.  Same errors,
 * same resulting state and films as dmt_set_medium_grid. */
int dmt_set_medium_grid_device(dmt_ctx* ctx, const void* d_density, int nx, int ny, int nz);
int dmt_clear_medium_grid(dmt_ctx* ctx);
/* *present = 1 with a grid; dims3 = (nx, ny, nz); the support index ranges (min > max without a density > 0); the number of
 * voxels > 0; the largest density; *active = 1 iff the grid rows would run.  Any pointer may be null. */
int dmt_medium_grid_info(dmt_ctx* ctx, int* present, int* dims3, int* support_min3, int* support_max3, uint64_t* positive, float* max_density,
                         int* active);
/* host only (no GPU): the march above for n rays through a grid given here, the device's bit for bit while no intermediate
 * is subnormal.  sigma_t, the box and the grid are checked as dmt_set_medium / dmt_set_medium_grid check them.  t_end[i] >= 0
 * and tau_target[i] >= 0, both may be +inf.  ts[i] is 0 without a collision. */
int dmt_medium_grid_march(const float* box_min3, const float* box_max3, float sigma_t, int nx, int ny, int nz, const float* density, int n,
                          const float* o3, const float* d3, const float* t_end, const float* tau_target, float* tau, float* ts, int32_t* collided,
                          int32_t* steps);
/* ---- chromatic and emissive media: RGB extinction by one-sample MIS (opt-in) ---- */
/* The spectrum.  Attached to the context's medium, the way the grid is: an extinction colour e[3] >= 0 (finite, not all zero)
 * and an emission radiance Le[3] >= 0 (finite).  The channel extinctions are k_c = fl32(sigma_t * e_c); with a grid the
 * extinction in voxel v is k_c * density[v].  Defaults: e = (1, 1, 1), Le = (0, 0, 0).  The spectrum belongs to no upload: it
 * survives dmt_set_medium, scene uploads and dmt_set_camera; dmt_clear_medium and dmt_clear_medium_spectrum drop it.  It may
 * be set before dmt_set_medium.
 *
 * Active.  The spectrum rows (*_medium_rgb, *_medium_grid_rgb) run exactly when the medium is active and either the three k_c
 * are not all equal or Le != 0.  With three equal k_c and Le == 0 the context launches the grey rows with sigma_t = k_0, and
 * films are byte for byte those of dmt_set_medium(k_0, ..); without a spectrum every film of every row is what it was.  With
 * a spectrum the medium is active iff its largest k_c is > 0 (and its grid, if any, has a density > 0).
 *
 * Reference channel.  m = the channel with the largest k (the lowest index on a tie); q_c = fl32(k_c / k_m), correctly
 * rounded on the host.  All clipping and marching is done once, in channel m: tau_m = k_m * len in the homogeneous rows,
 * the march of dmt_medium_grid_march with sigma_t = k_m in the grid rows.  Every other optical depth is tau_c = q_c tau_m.
 *
 * Per path segment whose channel-m optical depth is tau_seg > 0 (tau_seg == 0 or a miss of the box: nothing changes):
 *   1. j = the channel chosen with probability p_j = beta_j / (beta_0 + beta_1 + beta_2) by v = medium_u(h, depth + 2^31), the
 *      free-flight hash's second stream (2^31 and not a smaller offset: dmt_set_limits admits every depth below 2^31):
 *      x = v * ((beta_0 + beta_1) + beta_2); j = 0 if x < beta_0, else 1 if x < beta_0 + beta_1, else 2; a channel with
 *      beta_j == 0 is never chosen (a j that rounding let through falls back to the last channel before it with beta > 0).
 *      An all-zero (or non-finite) beta has no event: the segment is a pass with weights 1.
 *   2. T = fl32(-log(1 - medium_u(h, depth)) / q_j), the logarithm and the quotient in double by the same IEEE operations on
 *      both sides (so T is the device's bit for bit); +inf when q_j == 0.
 *   3. Collision (T < tau_seg; in the grid rows: the march with tau_target = T collides): at the point where the channel-m
 *      optical depth reaches T, i.e. t0 + T / k_m, or the march's ts.  tau_c = q_c T,
 *        w_c = q_c e^(-tau_c) / sum_i p_i q_i e^(-tau_i).
 *      First L += beta_c w_c (1 - albedo_c) Le_c (before the depth cap, as a surface adds its emission before it), then
 *      beta_c *= w_c, then dmt_set_medium's scatter vertex unchanged.
 *   4. Pass (otherwise): tau_c = q_c tau_seg, beta_c *= e^(-tau_c) / sum_i p_i e^(-tau_i); the sampler's dimensions stay
 *      unmoved and the path goes on to the surface or the miss.
 *   5. Every pending NEE contribution, made at a surface or at a scatter vertex, is multiplied per channel by
 *      e^(-q_c tau_m(shadow segment)).
 * A channel with q_c == 0 has optical depth 0 (e^0 = 1) whatever tau_m is.  This is the one-sample balance heuristic over
 * the three free-flight densities: unbiased for any positive p, and with throughput-proportional p the sum
 * beta_0 + beta_1 + beta_2 is conserved exactly by both weights (sum_c p_c w_c = 1).  fp32 range: the chosen channel's term
 * p_j q_j e^(-tau_j) must stay a normal float (p_j q_j above about 2^-100).
 *
 * Scope: as the medium's, and refused with the medium's messages. */
/* DMT_ERR_INVALID for a negative or non-finite value or an all-zero extinction; a refused call changes nothing. */
int dmt_set_medium_spectrum(dmt_ctx* ctx, const float* extinction3, const float* emission3);
int dmt_clear_medium_spectrum(dmt_ctx* ctx);
/* *present = 1 with a spectrum; the colour and the emission as set (the defaults without one); k3 = fl32(sigma_t * e_c) from
 * the medium's current sigma_t; the reference channel; *active = 1 iff the spectrum rows would run.  Any pointer may be null. */
int dmt_medium_spectrum_info(dmt_ctx* ctx, int* present, float* extinction3, float* emission3, float* k3, int* ref_channel, int* active);
/* host only (no GPU): steps 1 to 4 for n cases in a medium of channel extinctions k3 (finite, >= 0, not all zero): beta3
 * [n x 3] >= 0, the Halton index h, the depth, tau_seg > 0 (may be +inf).  channel = j (-1 without an event), collided,
 * tau_at = T on a collision and tau_seg on a pass, weight3 = the factors of beta.  The decisions are the device's bit for
 * bit; the weights differ by the two sides' expf and division. */
int dmt_medium_spectrum_event(const float* k3, int n, const float* beta3, const uint32_t* h, const uint32_t* depth, const float* tau_seg,
                              int32_t* channel, int32_t* collided, float* tau_at, float* weight3);
/* depth cap of the bounce loop; the reference hard-codes 32 (megakernel.cu:154) */
int dmt_set_limits(dmt_ctx* ctx, int max_depth);
int dmt_set_accel(dmt_ctx* ctx, int mode);
/* SURVEY 8f-4 -- how next-event estimation picks its light from the uploaded light list.  DMT_LIGHTS_UNIFORM (default) is
 * the reference megakernel's uniform pick (T/megakernel/megakernel.cu:170-173): the parity mode.  DMT_LIGHTS_TREE builds a
 * light BVH over the point / spot lights (after src/core/public/core-light-tree-builder.h:17-110; differences and why in
 * csrc/light_tree.hpp) and picks in proportion to flux x cosine / distance^2: same expected image, less noise with many
 * lights.  Applies to light lists of point / spot lights (scenes with emissive triangles, image textures, or a
 * directional light in the list keep the uniform pick). */
#define DMT_LIGHTS_UNIFORM 0
#define DMT_LIGHTS_TREE 1
/* the reference's light tree with its OWN semantics (src/core/public/core-light-tree-builder.h:17-104, .cpp:5-539): LightBounds with
 * normal cone and emission falloff, lbImportance's orientation term, 32-bin summed-area-orientation splits, an adaptive cut of
 * up to LightTreeMaxSplitSize = 4 nodes per shading point = up to four lights and four shadow rays per bounce
 * (csrc/light_tree_ref.hpp lists what is kept as written and the four places that had to be corrected).  Same applicability
 * rule as DMT_LIGHTS_TREE.  Unpinned by the reference (experimental, disabled code without outputs). */
#define DMT_LIGHTS_TREE_REFERENCE 2
int dmt_set_light_sampling(dmt_ctx* ctx, int mode);
/* host only (no GPU): the cut + selection of DMT_LIGHTS_TREE_REFERENCE at n shading points p3 / n3 with one random number u each:
 * up to four (light index, pmf) pairs per point (indices4 = -1 beyond counts[i]); start_pmf = probability that the light list
 * (not the env map) was asked */
int dmt_light_tree_ref_select(const void* lights32, uint32_t count, int n, const float* p3, const float* n3, const float* u, float start_pmf,
                              int32_t* indices4, float* pmfs4, int32_t* counts, int* node_count, int* depth);
/* host only (no GPU): probability of each of the `count` packed lights at point p3 with normal n3 under the tree */
int dmt_light_tree_pmfs(const void* lights32, uint32_t count, const float* p3, const float* n3, float* pmf_out, int* node_count,
                        int* depth);
/* host only (no GPU): the node array a context uploads for the `count` packed lights under `mode`, root first -- 32-byte
 * records for DMT_LIGHTS_TREE (csrc/light_tree.hpp LightTreeNode), 64-byte records for DMT_LIGHTS_TREE_REFERENCE
 * (csrc/light_tree_ref.hpp LightTreeRefNode).  nodes_out has room for `cap` records; node_count and depth are always
 * reported, and a cap below node_count is refused (DMT_ERR_INVALID) with nothing written to nodes_out. */
int dmt_light_tree_nodes(const void* lights32, uint32_t count, int mode, void* nodes_out, uint32_t cap, int* node_count, int* depth);
/* How next-event estimation picks among [uploaded lights..., emissive triangles...] when emissive triangles
 * (dmt_upload_area_lights) are present.  DMT_EMITTERS_UNIFORM (default): the uniform pick.  DMT_EMITTERS_TREE: a light BVH
 * with normal cones over the point / spot lights and the emissive triangles together (csrc/emitter_tree.hpp, after the light
 * BVH of pbrt-v4), walked once per bounce; a path ray that hits an emissive triangle weighs it with the
 * tree's probability of that triangle at the vertex the ray left.  Same expected image, less noise with many emitters.
 * Without emissive triangles, with a directional light in the list, or where the tree comes out deeper than its walk's
 * guard (a note in dmt_last_error), the uniform rows run as if the mode were not set.  Independent of
 * dmt_set_light_sampling.  An unknown mode is refused. */
#define DMT_EMITTERS_UNIFORM 0
#define DMT_EMITTERS_TREE 1
int dmt_set_emitter_sampling(dmt_ctx* ctx, int mode);
/* mode; active = a launch now runs the *_etree rows (builds the tree if it has to); emitters, nodes, depth (levels, a lone
 * leaf = 1) and the host build time of the last build (zeros while not active).  Any pointer may be null. */
int dmt_emitter_tree_info(dmt_ctx* ctx, int* mode, int* active, uint32_t* emitters, uint32_t* nodes, int* depth, double* build_ms);
/* host only (no GPU): the emitter tree a context builds for `count` packed lights (point / spot only), a soup xs / ys / zs
 * (4 floats per triangle and axis, as dmt_upload_triangles) of tri_count triangles and the emissive list area_tri / area_le
 * (3 floats each) of area_count entries.  Emitter i < count is light i, otherwise triangle area_tri[i - count].  nodes_out:
 * room for `cap` 48-byte records (csrc/emitter_tree.hpp EmitterNode), root first; trails_out / lengths_out: one bit trail
 * (bit k = the choice at level k below the root, 1 = right) and its length per emitter; any of the three may be null.
 * node_count and depth are always reported; a cap below node_count is refused with nothing written. */
int dmt_emitter_tree_nodes(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                           const uint32_t* area_tri, const float* area_le, uint32_t area_count, void* nodes_out, uint32_t cap,
                           uint64_t* trails_out, int32_t* lengths_out, int* node_count, int* depth);
/* host only: et_select at n cases (p3, n3, u) on that tree: index_out (-1: none), pmf_out = start_pmf x the walk's
 * probability, pmf_by_trail_out = start_pmf x et_pmf along the selected emitter's trail (0 where none was selected) */
int dmt_emitter_tree_select(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                            const uint32_t* area_tri, const float* area_le, uint32_t area_count, int n, const float* p3, const float* n3,
                            const float* u, float start_pmf, int32_t* index_out, float* pmf_out, float* pmf_by_trail_out);
/* host only: et_pmf of every emitter (count + area_count values) at point p3 with normal n3 */
int dmt_emitter_tree_pmfs(const void* lights32, uint32_t count, const float* xs, const float* ys, const float* zs, uint64_t tri_count,
                          const uint32_t* area_tri, const float* area_le, uint32_t area_count, const float* p3, const float* n3,
                          float* pmf_out);
/* How DMT_ACCEL_BVH launches are executed (results are bit-identical either way): 0 = automatic = 1 = the megakernel
 * (fastest on every measured scene); 2 = the device-side wavefront -- generate / trace / shade / fold kernels over
 * path-state arrays in HBM, csrc/wavefront.hpp -- kept as a measured alternative.  paths_per_pass: path
 * slots of one wavefront pass (0 = keep; default 2^22, 144 bytes of state each; more is faster, up to ~2^27). */
int dmt_set_bvh_strategy(dmt_ctx* ctx, int strategy, uint64_t paths_per_pass);
/* tile partition for multi-GPU rendering: this context renders only the 8x8-pixel tiles whose
 * index (row-major over the tile grid) is congruent to `rank` modulo `world`.  Default 0 of 1. */
int dmt_set_partition(dmt_ctx* ctx, int rank, int world);
/* SURVEY 8f-3 -- emissive triangles (diffuse area lights; what scenes/cornell-box.pbrt's AreaLightSource needs).  The
 * reference has no implementation; semantics are pbrt-v4's: one-sided emission on the side of
 * normalize(cross(p1 - p0, p2 - p0)), uniform point sampling, uniform choice among [uploaded lights..., emissive
 * triangles...], power-heuristic MIS.  triangle_index refers to the triangles of the last dmt_upload_triangles (which
 * clears this list); count == 0 removes the lights.  With an env map set, the map still takes half of the NEE samples. */
int dmt_upload_area_lights(dmt_ctx* ctx, const uint32_t* triangle_index, const float* radiance_rgb, uint32_t count);
/* A18 -- environment-map light of the reference's CPU renderer (src/core/private/core-light.cpp:84-117,394-491;
 * PiecewiseConstant2D src/core/private/core-math.cu:385-675; MIS rules src/core/private/core-render.cpp:154-163,
 * 290-299,357-369), added to the megakernel path: rgb = height x width x 3 floats (equirectangular, powers of two,
 * width == 2 * height), quat_xyzw = lightFromRender.  While an env map is set, rays that leave the scene see the map
 * (MIS against NEE) instead of the constant environment records, and NEE samples the map with probability 1/2.
 * `scale` is accepted for signature parity; the reference stores it and never applies it. */
int dmt_upload_envmap(dmt_ctx* ctx, const float* rgb, int width, int height, const float* quat_xyzw, float scale);
int dmt_clear_envmap(dmt_ctx* ctx);
/* SURVEY 8f-1 -- image textures of JSON materials ("textures" + string-valued "diffuse" / "roughness" / "normal" of
 * src/core/private/core-parser.cpp:306-560; the reference's megakernel has none, semantics are its CPU renderer's,
 * src/core/private/core-material.cpp:20-56,180-240): bilinear at MIP level 0, mirror wrap, byte / 255; the sampled albedo
 * and roughness patch the material's packed record as the host packers would build it, a normal map turns the geometric
 * normal into the shading normal.  rgba8: texel_count RGBA8 texels, all textures back to back, row major;
 * desc3[texture] = {first texel, width, height}; mat_tex4[bsdf] = {diffuse, roughness, normal texture index or
 * 0xFFFFFFFF, anisotropy as float bits}; tri_uv6[triangle] = {u0, v0, u1, v1, u2, v2}.  Upload AFTER triangles and
 * BSDFs (the counts must match at render time); texture_count == 0 clears.  Not combinable with emissive triangles. */
int dmt_upload_textures(dmt_ctx* ctx, const uint8_t* rgba8, uint64_t texel_count, const int32_t* desc3, uint32_t texture_count,
                        const uint32_t* mat_tex4, uint32_t bsdf_count, const float* tri_uv6, uint64_t triangle_count);
/* First-hit texture filtering (the reference's CPU renderer, src/core/private/core-material.cpp:83-175): at the camera
 * ray's hit every texture lookup is filtered by the pixel's footprint -- isotropic trilinear, or two EWA lookups -- over a
 * 2x2-box MIP chain that dmt_upload_textures builds; every later hit keeps the level-0 bilinear lookup.  Mode
 * DMT_TEXFILTER_LEVEL0 (the default) is the level-0 lookup everywhere; DMT_TEXFILTER_REFERENCE selects the filtering
 * kernels when textures are uploaded.  The footprint uses the camera's spp field (the frame's samples per pixel). */
enum {
  DMT_TEXFILTER_LEVEL0 = 0,
  DMT_TEXFILTER_REFERENCE = 1,
};
int dmt_set_texture_filter(dmt_ctx* ctx, int mode);
/* host only: MIP levels 1.. of one RGBA8 texture (width x height texels, 4 bytes each), back to back and row major, into
 * `out` (capacity out_texels texels); *levels = the level count including level 0 */
int dmt_texture_mip_chain(const uint8_t* rgba8, int width, int height, uint8_t* out, uint64_t out_texels, int* levels);
/* host only: the camera's footprint, 19 floats: camera-from-render as a row-major 3x4, the smallest x and y direction
 * differentials (3 + 3), the spp scale max(1/8, 1/sqrt(spp)) */
int dmt_texture_footprint(const dmt_camera* cam, float* out);
/* device probes of the filtered lookup of texture tex[i] at triangle tri[i], barycentrics (bu[i], bv[i]) of the uploaded
 * scene, as at a hit of depth depth[i] (0 = the camera ray's hit): rgb3, branch (0 level 0, 1 trilinear, 2 EWA, 3 EWA at a
 * level raised to bound its work) and the level used (integer part) with its interpolation weight (fraction) */
int dmt_test_texture_filter(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const int32_t* tex,
                            const int32_t* depth, float* rgb3, int32_t* branch, float* lod);
/* host only (no GPU needed): the sampling tables dmt_upload_envmap builds; func/cdf: height*width floats each,
 * row_integral / marginal_func / marginal_cdf: height floats each */
int dmt_envmap_tables(const float* rgb, int width, int height, float* func, float* cdf, float* row_integral,
                      float* marginal_func, float* marginal_cdf, float* marginal_integral);
/* device probes of the env-map functions: per case u2 -> sampled wi3, pdf, uv2, Le3 (by uv), ok; and
 * wi_in3 -> Le_dir3, pdf_dir (evaluation by direction) */
int dmt_test_envmap(dmt_ctx* ctx, int n, const float* u2, const float* wi_in3, float* wi3, float* pdf, float* uv2,
                    float* Le3, int32_t* ok, float* Le_dir3, float* pdf_dir);
/* samples per work item inside one dmt_render pass (0 = automatic, the default: 1 024 path samples per item; at most 512).  Purely a
 * scheduling knob: a pixel's samples are folded in index order for any value, the film is bit-identical. */
int dmt_set_chunk(dmt_ctx* ctx, uint32_t samples_per_item);
/* Sampler table.  The sampler's 8 values and the film jitter of sample s depend on (px % 128, py % 128, s) only, so a
 * dmt_render call may tabulate them once over the frame's period min(width,128) x min(height,128) (a fill kernel inside
 * the call's timed span, refilled by every call) and have every pixel load them instead of computing them.  The film
 * is bit-identical either way.  Modes: OFF; AUTO (the default) uses the table when the call's owned pixels cover at
 * least 4 periods; FORCE uses it whenever the launch kind allows.  dmt_render_stats / _profile, dmt_render_adaptive and
 * the wavefront form always compute.  budget_bytes bounds the table's device memory (0 = the default, 512 MiB): a call
 * whose table is larger runs as consecutive sample slices of whole chunks, each a fill and a launch, still one entry of
 * dmt_kernel_time; if not even one chunk fits, the call computes.  DMT_SAMPLER_TABLE=0|1|2 in the environment sets
 * the mode at context creation. */
#define DMT_SAMPLER_TABLE_OFF 0
#define DMT_SAMPLER_TABLE_AUTO 1
#define DMT_SAMPLER_TABLE_FORCE 2
int dmt_set_sampler_table(dmt_ctx* ctx, int mode, uint64_t budget_bytes);
typedef struct dmt_sampler_table_plan_record {
  uint32_t use;                          /* 1: the call fills and reads a table */
  uint32_t period_width, period_height;  /* min(width,128), min(height,128) */
  uint32_t entry_bytes;                  /* per (sample, period pixel): 32 bytes of values + 8 of jitter */
  uint32_t slices;                       /* fill + launch pairs of the call (0 without a table) */
  uint32_t reserved;
  uint64_t slice_bytes;                  /* table bytes of the largest slice */
} dmt_sampler_table_plan_record;
/* host only (no GPU needed): what a dmt_render call of spp samples in chunks of chunk_spp does with owned_pixels owned
 * pixels (whole tiles x 64) of a width x height frame.  slice_spp[0 .. min(slices, slice_cap)) receives the slices'
 * sample counts: consecutive, every one but the last a multiple of chunk_spp, together spp. */
int dmt_sampler_table_plan(int width, int height, uint64_t owned_pixels, uint32_t spp, uint32_t chunk_spp, uint64_t budget_bytes,
                           int mode, dmt_sampler_table_plan_record* out, uint32_t* slice_spp, uint32_t slice_cap);
/* borrow an external hipStream_t (e.g. the caller's); NULL restores the context's own stream */
int dmt_set_stream(dmt_ctx* ctx, void* hip_stream);

/* ---- film ---------------------------------------------------------------------------------- */
int dmt_film_clear(dmt_ctx* ctx);
/* use caller-owned device buffers (width*height float4 each) instead of the context's own */
int dmt_film_bind(dmt_ctx* ctx, void* d_mean, void* d_m2);
int dmt_film_device_ptrs(dmt_ctx* ctx, void** d_mean, void** d_m2);
/* synchronises the stream; DMT_ERR_HIP (and no copy) if a past launch did not fold every sample chunk exactly once (see dmt_sync) */
int dmt_download_film(dmt_ctx* ctx, float* mean4, float* m24);

/* ---- render -------------------------------------------------------------------------------- */
/* Enqueue one pass: samples [sample_offset, sample_offset + spp) of every owned pixel in
 * [x0,x1) x [y0,y1) are traced and folded into the film (Welford, in sample order).
 * Asynchronous on the context's stream. */
int dmt_render(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1);
/* Adaptive sampling: rounds of step_spp samples from sample 0; before each round the film decides which pixels of
 * [x0,x1) x [y0,y1) owned by this partition go on.  Rule (fp32 on the device): with N = M2.w,
 *   err = sqrt((M2.x + M2.y + M2.z) / (N (N - 1))) / max(mean.x + mean.y + mean.z, 1e-3)   (+inf for N < 2)
 * and a pixel takes part in the round starting at sample `offset` iff
 *   N == offset && N < max_spp && (N < min_spp || err > threshold).
 * A pixel that stopped at N samples is bit-identical to the same pixel of a uniform N-spp film.  Every round runs the
 * megakernel (also under dmt_set_bvh_strategy 2) and counts in dmt_kernel_time.  Synchronous (one 8-byte read-back per
 * round).  *rounds = rounds launched, *samples = path samples traced (either may be NULL).  DMT_ERR_INVALID for
 * step_spp == 0, max_spp == 0, max_spp > 2^24 or a negative or non-finite threshold.  Call dmt_film_clear first for a
 * fresh image. */
int dmt_render_adaptive(dmt_ctx* ctx, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, float threshold,
                        int x0, int y0, int x1, int y1, uint32_t* rounds, uint64_t* samples);
/* Same pass through the counting build of the BVH kernel (synchronous, not for timing): stats6 =
 * {samples, closest-hit rays, shadow rays, BVH node visits, triangle tests, bounces}.  The film is
 * updated exactly as by dmt_render. */
int dmt_render_stats(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1,
                     uint64_t* stats6);
/* Diagnostic: dmt_render_stats plus the loop profile of the BVH kernel.  stats16 = the six counters above, then
 * wave-loop iterations x 64 (node steps, leaf steps, shading steps, outer iterations, sample preparations) and the
 * lanes that did work in leaf / shading / preparation steps; node visits that entered no child; traversal-stack pushes that
 * went to the global overflow area (entries beyond the LDS part of the stack). */
int dmt_render_profile(dmt_ctx* ctx, uint32_t sample_offset, uint32_t spp, int x0, int y0, int x1, int y1,
                       uint64_t* stats16);
/* waits for the stream; DMT_ERR_HIP if the launches so far did not fold every (tile, sample chunk) into the film exactly
 * once (the in-launch hand-over that makes the film schedule-independent counts its folds): the film is then invalid.
 * dmt_download_film and dmt_kernel_time report the same condition. */
int dmt_sync(dmt_ctx* ctx);
/* Diagnostics of the in-launch fold hand-over, accumulated over the launches since the last reset (synchronises):
 * out8 = {sample chunks folded, chunks handed over to the folder of their predecessor, chunks folded on behalf of another
 * wave, times a wave found all its staging slabs handed over, waves that left the launch early because of that,
 * longest such stall in 10 ns ticks, sample chunks launched (must equal [0]), staging slabs per wave}. */
int dmt_sched_diag(dmt_ctx* ctx, uint64_t* out8, int reset);
/* GGX batching (brute-force launches without an env map, textures, area lights, motion, cutouts, vertex normals or a light
 * tree, i.e. k_megakernel; every other launch ignores the setting).  A hit on a GGX material below the bounce cap is not shaded in the pass that found it:
 * the lane writes the path into its wave's queue in device memory and starts its next sample; when `batch` hits wait
 * (or their work item has no other work left), lanes that fall free take them back and shade them together.  The film is
 * bit-identical for every batch, 0 (off) included.  batch <= 64; DMT_GGX_BATCH=0|T in the environment sets it at context
 * creation.  Off is not free: the kernel carries the code either way, and with batch 0 the 1024^2 Cornell frame runs
 * about 1 % slower than it did before the kernel had it; so does a scene without a GGX material.
 * dmt_sync (and what reports like it) fails if a launch took back fewer hits than it parked. */
int dmt_set_ggx_batch(dmt_ctx* ctx, uint32_t batch);
/* Its counters since the last dmt_sched_diag reset (synchronises): out5 = {hits parked, hits taken back, shading passes that
 * ran the GGX code, GGX hits shaded at once because the queue was full, the context's batch size}.  The first four are
 * counted while batching is on only.  dmt_sched_diag itself reports none of them (its eight words are taken), and its
 * reset clears them: read these first. */
int dmt_ggx_batch_diag(dmt_ctx* ctx, uint64_t* out5);
/* The table that tells GGX batching which hits to park, as a launch reads it: bit i of word i / 32 is set when the
 * material of triangle i is a GGX dielectric or conductor.  It is made on the host from the material ids of
 * dmt_upload_triangles and the records of dmt_upload_bsdfs, anew by either call (in any order; a material id beyond the
 * BSDF array counts as not GGX).  Soups of at most 64 triangles carry it in the kernel arguments, larger ones as a
 * device array; DMT_TRI_KIND_INLINE=0 in the environment at context creation makes every soup use the array (tests).
 * out: (triangles + 31) / 32 words; `words` is the room at out.  Synchronises where the table is a device array. */
int dmt_tri_kind_bits(dmt_ctx* ctx, uint32_t* out, uint64_t words);
/* HIP-event time of the megakernel launches since the last reset (synchronises the stream):
 * total milliseconds and launch count. */
int dmt_kernel_time(dmt_ctx* ctx, double* total_ms, uint64_t* launches, int reset);
/* compile-time facts of the loaded code object: vgprs, sgprs, LDS bytes, max resident waves/CU
 * as reported by the runtime for the megakernel; CU count of the device */
int dmt_kernel_info(dmt_ctx* ctx, int* vgprs, int* sgprs, int* lds_bytes, int* blocks_per_cu,
                    int* cu_count);

/* host-only check of the BVH builder behind DMT_ACCEL_BVH (no GPU needed): builds the tree of a soup
 * and verifies that every triangle sits in exactly one leaf, child boxes nest and enclose their
 * vertices, leaves hold <= 4 triangles and the depth respects the traversal-stack bound */
int dmt_bvh_validate(const float* xs, const float* ys, const float* zs, size_t count, int* node_count,
                     int* depth, int* max_leaf);

/* ---- who builds the tree of DMT_ACCEL_BVH (beyond the reference) ---------------------------- */
/* DMT_BVH_BUILD_HOST (default): binned SAH on one host core (csrc/bvh.hpp), pairs packed on the host, both arrays
 * copied over.  DMT_BVH_BUILD_DEVICE: an LBVH built on the context's stream from the vertices the context already holds
 * on the device (csrc/bvh_gpu_build.hip: Morton keys, radix sort, binary radix tree, bottom-up boxes, level-by-level
 * collapse into the same 4-wide nodes and triangle pairs).  Boxes only cull and the triangle test alone decides hits,
 * so closest hits and films are bit-identical under either tree; what differs is the build time and the tree's quality.
 * The trade, measured on one MI355X: 1 M random triangles build in 4.5 ms instead of 760 ms, 16 M in
 * 67 ms instead of 19.9 s (end to end either way); the device tree's SAH cost is 1.05x the host tree's on those soups
 * and it renders at 0.97x the host tree's rate (1 M triangles, 1024^2 x 64 spp: 501 against 516 Msamples/s); on the
 * 26-triangle Cornell box it renders at 1.045x.  The build holds 260 bytes of temporary device memory per triangle,
 * which the context keeps for the next build.  Unknown mode -> DMT_ERR_INVALID.  A change of mode drops the current tree; it is rebuilt
 * at once when the accel mode is DMT_ACCEL_BVH and triangles are present (as dmt_set_accel does), and
 * dmt_upload_triangles builds with the mode in force.  A soup whose Morton-order tree would be deeper than the
 * traversal stack allows (only possible with > 2^18 triangles in one Morton cell) is built by the host builder
 * instead; the build record says so.  A failed device allocation is an error (DMT_ERR_HIP), never a silent host build. */
enum {
  DMT_BVH_BUILD_HOST = 0,
  DMT_BVH_BUILD_DEVICE = 1,
};
enum { /* dmt_accel_build_record.builder */
  DMT_BVH_BUILT_BY_HOST = 0,
  DMT_BVH_BUILT_BY_DEVICE = 1,
  DMT_BVH_BUILT_BY_HOST_AFTER_DEVICE = 2, /* the device build was abandoned by its depth guard */
};
int dmt_set_accel_build(dmt_ctx* ctx, int mode);
typedef struct dmt_accel_build_record {
  int32_t builder;     /* DMT_BVH_BUILT_BY_* */
  int32_t depth;       /* 4-wide levels */
  uint32_t triangles;
  uint32_t nodes;
  uint32_t pairs;      /* triangle pairs, without the three guard pairs */
  uint32_t reserved;
  double build_ms;     /* device: HIP events around the build on the stream; host: wall clock around build, pair
                        * packing and the copies to the device -- end to end either way */
  uint64_t temp_bytes; /* temporary device memory the build held (kept by the context for the next build) */
} dmt_accel_build_record;
/* the record of the current tree; without a tree: zero counts and the builder the next build will use */
int dmt_accel_build_info(dmt_ctx* ctx, dmt_accel_build_record* out);
/* the current tree for checks (synchronises the stream): its 64-byte nodes and the two ORIGINAL triangle indices of
 * each pair.  DMT_ERR_STATE without a tree, DMT_ERR_INVALID when a capacity (in nodes / pairs) is below the record's count. */
int dmt_accel_download(dmt_ctx* ctx, void* nodes64, size_t node_cap, uint32_t* pair_orig2, size_t pair_cap);
/* host only (no GPU): the serial restatement of the device builder (csrc/bvh.hpp lbvh::reference), bit for bit the
 * tree DMT_BVH_BUILD_DEVICE builds for the same soup.  max_depth: the depth guard's bound (the device uses 48);
 * *abandoned = 1 and zero counts when the level loop would pass it.  Capacities as for dmt_accel_download:
 * max(count, 1) nodes and pairs always suffice; DMT_ERR_INVALID when one is too small. */
int dmt_lbvh_reference(const float* xs, const float* ys, const float* zs, size_t count, int max_depth, void* nodes64,
                       size_t node_cap, uint32_t* pair_orig2, size_t pair_cap, uint32_t* node_count, uint32_t* pair_count,
                       int* depth, int* abandoned);
/* host only (no GPU): the walk of dmt_bvh_validate on ANY tree in this layout over the soup: every triangle in exactly
 * one leaf, every node reached once, decoded boxes contain their vertices and nest within a quantisation step, counts in
 * range, leaves <= 2 triangles, depth <= 48.  DMT_OK or DMT_ERR_STATE.  *depth = 4-wide levels, *max_leaf = triangles in
 * the largest leaf, *sah_cost = sum over all child slots of the decoded child box's area, a leaf slot weighted by its
 * triangle count, divided by the area of the union of the root's child boxes (any of the three may be NULL). */
int dmt_bvh_check(const void* nodes64, size_t node_count, const uint32_t* pair_orig2, size_t pair_count, const float* xs,
                  const float* ys, const float* zs, size_t count, int* depth, int* max_leaf, double* sah_cost);

/* ---- moving geometry: same triangles, new positions (beyond the reference) ------------------- */
/* Same triangles, new positions.  count must equal the current triangle count (DMT_ERR_INVALID otherwise; DMT_ERR_STATE
 * before any dmt_upload_triangles).  Layout of xs / ys / zs as in dmt_upload_triangles.  Material ids, the emissive-triangle
 * list, texture tables and UVs, lights, camera and film are kept.  Synchronises the stream first (launches in flight read
 * the old records), then leaves the context as dmt_upload_triangles + the same dmt_upload_area_lights +
 * dmt_upload_textures would -- except for the tree, which follows dmt_set_accel_update.  The film is not cleared and
 * AOVs are not recomputed.  An empty soup (count 0 on a 0-triangle context) is a no-op. */
int dmt_update_vertices(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs, size_t count);
/* The same from device memory of the context's device: count x 9 floats (p0 xyz, p1 xyz, p2 xyz), read on the context's
 * stream; the caller orders its own writes before that (same stream via dmt_set_stream, or a synchronise).  A kernel makes
 * the records (byte for byte the host packer's for triangles of non-zero area); the context's host copy of the soup is
 * refreshed by device-to-host copies. */
int dmt_update_vertices_device(dmt_ctx* ctx, const void* d_verts9, size_t count);
/* What an update does to the tree of DMT_ACCEL_BVH (under brute force an update drops any tree, as an upload does).  A refit
 * (csrc/bvh.hpp namespace refit, kernels in csrc/bvh_gpu_build.hip) is a pure function of the topology and the new
 * positions: pairs rewritten, every box recomputed bottom-up from exact fp32 boxes, one launch per 4-wide level; refitting
 * back to the positions a tree was built from gives the builder's bytes again.  It keeps the topology of either builder;
 * closest hits and films stay bit-identical to brute force, what degrades with the deformation is the tree's quality
 * (sah_cost against sah_cost_at_build).  The library ships no default ratio. */
enum {
  DMT_BVH_UPDATE_REBUILD = 0, /* default: rebuild with the builder in force -- what a re-upload does */
  DMT_BVH_UPDATE_REFIT = 1,   /* keep topology and pair order, recompute every box on the device */
  DMT_BVH_UPDATE_AUTO = 2,    /* refit, then rebuild if cost > max_cost_ratio x the cost the builder left */
};
/* AUTO: max_cost_ratio finite and > 1, else DMT_ERR_INVALID; ignored otherwise.  Unknown mode -> DMT_ERR_INVALID. */
int dmt_set_accel_update(dmt_ctx* ctx, int mode, double max_cost_ratio);
enum { /* dmt_accel_update_record.action */
  DMT_BVH_UPDATED_NONE = 0, /* no update yet, or no tree to update (brute force) */
  DMT_BVH_UPDATED_REFIT = 1,
  DMT_BVH_UPDATED_REBUILD = 2,
  DMT_BVH_UPDATED_REBUILD_AFTER_REFIT = 3, /* AUTO: the refitted tree's cost passed the ratio */
};
typedef struct dmt_accel_update_record {
  int32_t action;               /* DMT_BVH_UPDATED_*, of the last update */
  uint32_t updates_since_build; /* refits since a builder made the topology; every build (upload, dmt_set_accel_build, rebuild) resets it */
  double update_ms;             /* HIP events on the stream around record making + refit (+ cost); a rebuild adds its build_ms */
  double sah_cost;              /* dmt_bvh_check's definition, of the current tree; 0 when not computed (REBUILD mode) */
  double sah_cost_at_build;     /* the same of the tree as its builder left it; 0 when not computed */
  uint64_t temp_bytes;          /* refit scratch the context keeps (boxes per node and per pair, cost terms) */
} dmt_accel_update_record;
/* the record of the last update; dmt_accel_build_info keeps describing the build that made the topology */
int dmt_accel_update_info(dmt_ctx* ctx, dmt_accel_update_record* out);
/* host only (no GPU): the serial restatement of the refit.  In: any tree in this layout (as from dmt_accel_download,
 * dmt_lbvh_reference) and the NEW soup.  Out: the refitted nodes (node_count x 64 bytes), bit for bit what the device
 * refit leaves.  DMT_ERR_STATE if a child index is not above its parent's or a reference leaves the arrays. */
int dmt_bvh_refit_reference(const void* nodes64, size_t node_count, const uint32_t* pair_orig2, size_t pair_count,
                            const float* xs, const float* ys, const float* zs, size_t count, void* nodes64_out);

/* host-only (no GPU needed): how the brute-force pass splits a soup.  Up to 4 culled clusters, runs of
 * >= 4 consecutive triangles of one material whose bounding sphere is small next to the scene; every other triangle is
 * tested for every ray.  Cluster k: cluster_first_count[2k], [2k + 1] = first original index, triangle count;
 * cluster_sphere[4k .. 4k + 3] = centre and inflated radius.  enable = 0 gives no cluster (what DMT_BRUTE_CULL=0 does). */
int dmt_brute_cull_plan(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count,
                        int enable, uint32_t* cluster_count, uint32_t* cluster_first_count, float* cluster_sphere);

/* host-only: the box clusters the brute-force pass adds after those of dmt_brute_cull_plan (flat meshes such as walls).  Up
 * to 12 minus the sphere clusters: runs of >= 2 consecutive triangles of one material that the sphere rule rejects and
 * whose box has at most 0.35 of the scene box's surface area.  Cluster k: cluster_first_count[2k], [2k + 1] as above;
 * cluster_box[6k .. 6k + 5] = inflated box lo xyz, hi xyz.  enable = 0 gives none (DMT_BRUTE_CULL=0 or 1). */
int dmt_brute_cull_box_plan(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count,
                            int enable, uint32_t* cluster_count, uint32_t* cluster_first_count, float* cluster_box);

/* host-only: the same box clusters in both forms, cluster_box[6k .. 6k + 5] as above and cluster_record[6k .. 6k + 5] =
 * centre xyz, half-width xyz: what the device's bound test reads.  [centre - half-width, centre + half-width] holds the
 * inflated box in exact arithmetic.  Either array may be null. */
int dmt_brute_cull_box_records(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count,
                               int enable, uint32_t* cluster_count, float* cluster_box, float* cluster_record);

/* host-only: the whole cluster table of a soup as the device reads it, sphere clusters first, then box clusters, for
 * level = what DMT_BRUTE_CULL selects (0 none, 1 spheres, 2 spheres and boxes).  records (may be null) takes cluster_count
 * <= 12 records of *record_bytes = 64 bytes each, little-endian 32-bit words: [0..5] the bound as float (sphere: centre xyz,
 * squared inflated radius, 0, 0; box: centre xyz, half-width xyz), [6] 1 for a box bound, [7] triangle count, [8] first
 * original index, [9] first slot in the block's LDS copy, [10] ceil(2^32 / count), [11..15] zero.  Words 0..7 are what a
 * bound test loads, in one 32-byte scalar load; *record_align = 64 is the alignment of a record in the device table. */
int dmt_cull_records(const float* xs, const float* ys, const float* zs, const uint32_t* mat_id, size_t count, int level,
                     uint32_t* cluster_count, uint32_t* record_bytes, uint32_t* record_align, void* records);

/* host-only: the device's box bound test, the same inline functions compiled for the host (a division stands for the
 * device's reciprocal instruction).  record6 = one cluster_record; ray i: origins[3i .. 3i + 2], dirs[3i .. 3i + 2] and the
 * segment end tmax[i] (inf allowed); accept[i] = 1 when the brute-force pass would test the cluster's triangles for it. */
int dmt_cull_box_test(const float* record6, const float* origins, const float* dirs, const float* tmax, size_t count,
                      uint8_t* accept);

/* ---- denoiser (an explicit post-process; beyond the reference) ----------------------------- */
/* Feature pass: camera samples 0 .. aov_spp-1 of EVERY pixel of the frame (the film's own camera rays; dmt_set_partition
 * and regions do not apply), closest hit under the current accel mode (brute force and BVH give bit-identical planes).
 * Three row-major float4 planes that the context owns, summed in sample order in fp32 over the samples whose ray hit a
 * triangle ("hits"):
 *   albedo   = (sum W / aov_spp, hits / aov_spp): W = the material record's fp16 weight after the level-0 texture patch;
 *              BS_GGX_BLEND pairs: (1 - metallic) W_dielectric + metallic W_conductor
 *   normal   = (normalize(sum of shading normals), 0): face-forwarded or normal-mapped; 0 without hits or if |sum| < 1e-6
 *   position = (sum hit point / hits, sum t / hits); 0 without hits
 * Asynchronous on the context's stream.  DMT_ERR_INVALID for aov_spp outside 1 .. 65536. */
int dmt_render_aovs(dmt_ctx* ctx, uint32_t aov_spp);
/* host -> device: three width x height planes in the layout above (e.g. synthetic input for dmt_denoise) */
int dmt_upload_aovs(dmt_ctx* ctx, const float* albedo4, const float* normal4, const float* position4, int width, int height);
/* device -> host copy of the planes (any pointer may be NULL); synchronises the stream */
int dmt_download_aovs(dmt_ctx* ctx, float* albedo4, float* normal4, float* position4);
/* Spatial SVGF: edge-avoiding a-trous passes (Dammertz et al. 2010) with the variance-guided luminance term of Schied et al.
 * 2017.  Pass i = 0 .. iterations-1 has step s = 2^i and taps q = p + s (dx, dy), dx, dy in -2 .. 2, kernel h(dx) h(dy) with
 * h = [1/16, 1/4, 3/8, 1/4, 1/16]; taps outside the image are skipped.  A tap q != p counts only if both p and q have
 * coverage (albedo.w > 0), with edge weight
 *   max(0, n_p . n_q)^sigma_normal
 *   x exp(-|n_p . (x_q - x_p)| / (sigma_position t_p theta s sqrt(dx^2 + dy^2)))     theta = sensor_size / (focal_length height)
 *   x exp(-|a_p - a_q|^2 / sigma_albedo^2)
 *   x exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-10))      l = Rec. 709 luminance, g_p = 3x3 [1/4 1/2 1/4] blur of v
 * c' = sum w c / sum w, v' = sum w^2 v / (sum w)^2; c0 = mean.xyz, v0 = (M2.x + M2.y + M2.z) / (3 N (N - 1)). */
typedef struct dmt_denoise_params {
  int32_t iterations;    /* 0 .. 10; 0 returns mean.xyz bit for bit */
  float sigma_normal;    /* every sigma: finite and > 0 */
  float sigma_position;
  float sigma_albedo;
  float sigma_luminance;
} dmt_denoise_params;
dmt_denoise_params dmt_denoise_defaults(void);
/* Denoises a film with the AOVs of the context into out4 (width x height float4, w = 1).  mean4 / m24 NULL: the context's
 * film (own or bound); otherwise host planes of the camera's size (e.g. the combined film of several partitions).  params
 * NULL: dmt_denoise_defaults().  Synchronous; *kernel_ms (may be NULL) = HIP-event time of its kernels.  Never modifies the
 * film or the AOVs.  DMT_ERR_STATE without AOVs, for AOVs of another size than the film, or when a pixel has N < 2 or a
 * non-finite mean / M2 (e.g. a partitioned film that was not combined); DMT_ERR_INVALID for bad parameters. */
int dmt_denoise(dmt_ctx* ctx, const dmt_denoise_params* params, const float* mean4, const float* m24, float* out4, float* kernel_ms);

/* ---- temporal accumulation (opt-in; the "T" of SVGF with motion vectors from geometry) ------ */
/* dmt_render_aovs also writes a fourth plane, surface = (tri, bu, bv, 1) of the first camera sample, in sample order, whose
 * ray hit a triangle: tri = the original triangle index as a float, (bu, bv) the barycentrics of p1 and p2; (-1, 0, 0, 0)
 * without a hit.  dmt_upload_aovs drops it: upload it after the three planes, in their size (DMT_ERR_STATE otherwise). */
int dmt_download_aov_surface(dmt_ctx* ctx, float* surface4);
int dmt_upload_aov_surface(dmt_ctx* ctx, const float* surface4, int width, int height);
/* host only (no GPU): render-space points p3 (n x 3) -> xy2 (n x 2) = the continuous film coordinates (fx, fy) at which the
 * camera's ray passes through the point (sample s of pixel (px, py) has fx = px + its pixel offset in [0, 1)), and depth (n)
 * = the distance along the viewing direction (<= 0: behind the camera, xy2 is then meaningless).  fp32 without contraction:
 *   d = p - pos; c = (right . d, up . d, fwd . d), each (a + b) + c; s = focal / c.z; fx = (c.x s - tx) ipx; fy = (c.y s - ty) ipy
 * with right / up / fwd / pos of dmt_set_camera's render-from-camera matrix and focal, tx, ty, ipx = 1 / psx, ipy = -1 / psy
 * of its camera-from-raster matrix.  dmt_test_camera_project is the device twin under the context's camera. */
int dmt_camera_project(const dmt_camera* cam, int n, const float* p3, float* xy2, float* depth);
typedef struct dmt_temporal_params {
  float alpha;            /* 0 .. 1: the current frame's least share; 0 = the plain mean of the frames, 1 = no history */
  float normal_threshold; /* finite: a history tap counts if n_p . n_prev(q) >= normal_threshold */
  float plane_threshold;  /* finite and > 0: and if |n_prev(q) . (X_prev - x_prev(q))| <= plane_threshold t_prev(q) theta_prev */
} dmt_temporal_params;
dmt_temporal_params dmt_temporal_defaults(void);
/* dmt_denoise with a history.  The current (rgb, v0) plane is blended with the previous call's accumulated plane,
 * reprojected: for a pixel p with coverage and surface (tri, bu, bv), X = w0 p0 + bu p1 + bv p2 (w0 = (1 - bu) - bv) under
 * the current and under the history frame's raw vertices, (u, v) = p + project_prev(X_prev) - project_cur(X_cur), the 2 x 2
 * bilinear taps at floor(u, v).  A tap q counts if it lies in the image, h_prev(q) >= 1 and it passes the two tests above.
 * With W = sum w > 0: c_prev = sum w c / W, v_prev = sum w^2 v / W^2, h = min(sum w h / W + 1, 65536), a = max(alpha, 1 / h),
 * c = c_prev + a (c_cur - c_prev), v = (1 - a)^2 v_prev + a^2 v_cur (a = 1: c_cur, v_cur themselves).  Otherwise (no counted
 * tap, no surface, depth <= 0 under the history's camera; there is no wider search): c_cur, v_cur, h = 1; without
 * coverage h = 0.  This plane is the new history; `iterations` a-trous passes of dmt_denoise then filter it into out4.
 * The history (allocated by the first call) also keeps the normal / position planes, the camera and the raw vertices of
 * its frame; dmt_update_vertices[_device] keep the current vertices.  It is reset (every pixel h = 1) by
 * dmt_upload_triangles, a change of resolution and dmt_temporal_reset.  params / tparams NULL: the defaults.  Refusals as
 * dmt_denoise (the history is then left as it was), and DMT_ERR_STATE without a surface plane or for more than 2^24
 * triangles, DMT_ERR_INVALID for alpha outside [0, 1], a non-finite threshold or plane_threshold <= 0.  Never modifies the
 * film or the AOVs.  Synchronous. */
int dmt_denoise_temporal(dmt_ctx* ctx, const dmt_denoise_params* params, const dmt_temporal_params* tparams, const float* mean4,
                         const float* m24, float* out4, float* kernel_ms);
/* forgets the history (its memory is kept): the next temporal call starts at h = 1 */
int dmt_temporal_reset(dmt_ctx* ctx);
typedef struct dmt_temporal_record {
  uint32_t frames;        /* temporal calls accumulated since the last reset */
  uint32_t reprojected;   /* last call: pixels that took history (at least one counted tap) */
  uint32_t reset;         /* last call: covered pixels that took none (h = 1) */
  float temporal_ms;      /* last call: HIP-event time of the reprojection kernel alone */
  uint64_t history_bytes; /* device memory of the history and the vertex snapshots; 0 before the first temporal call */
} dmt_temporal_record;
int dmt_temporal_info(dmt_ctx* ctx, dmt_temporal_record* out);
/* the history: color_var4 (width x height float4: accumulated rgb, variance of the mean) and length1 (width x height
 * float), either may be NULL; DMT_ERR_STATE without a history */
int dmt_temporal_download(dmt_ctx* ctx, float* color_var4, float* length1);

/* ---- display transform (an explicit post-process; beyond the reference) ----- */
/* A linear RGB plane (the film's mean, or any plane of the camera's size) to a display-referred one, in this order:
 *   0 scrub     a component that is not finite or is negative becomes 0 (pixels with a non-finite component are counted);
 *   1 exposure  c = scale * rgb.  Manual: scale = 2^exposure_ev.  Auto: metered from a histogram of the log luminance
 *               y = (0.2126 r + 0.7152 g) + 0.0722 b, eight bins per stop over [2^-16, 2^16) taken from the float's bits
 *               (dmt_display_bin); pixels with y <= 0 are skipped.  Of the T counted pixels the mass between
 *               low_fraction T and (1 - high_fraction) T is kept, avg is its mean log2 luminance (bin k stands for
 *               floor(k/8) - 16 + log2(1 + (k mod 8 + 0.5) / 8)) and scale = key / 2^avg * 2^exposure_ev, in double, rounded
 *               once (dmt_display_metering).  Nothing counted: scale = 2^exposure_ev;
 *   2 bloom     a mean-preserving pyramid without a threshold: K' = min(bloom_levels, floor(log2(min(w, h)))) levels, each a
 *               2x2 box average of the one below (edges clamped), summed back up through a separable (0.75, 0.25) upsample,
 *               divided by K' + 1 and mixed in: c + bloom_strength (bloom - c).  Off at 0 levels or strength 0;
 *   3 tone      LINEAR; REINHARD (extended, on luminance, white point `white`, default 4); ACES (Narkowicz's fit, per
 *               channel); HABLE (Uncharted 2's curve at 2x over its value at `white`, default 11.2).  Clamped to [0, 1];
 *   4 transfer  LINEAR; SRGB (the piecewise sRGB OETF); GAMMA22 (x^(1/2.2)).  Clamped to [0, 1]: the float output, w = 1;
 *   5 quantise  to RGBA8, A = 255: TRUNCATE floor(min(255 v, 255)); ROUND floor(min(255 v + 0.5, 255)); DITHER
 *               floor(min(255 v + (M[y & 7][x & 7] + 0.5) / 64, 255)), M the 8 x 8 Bayer index matrix.
 * LINEAR / LINEAR / TRUNCATE at 0 EV without bloom is the rule of the PNG writer.  The same plane always gives the same bytes:
 * the histogram is integer, the metering is the host's, and stages 0, 1 and 5 round once per operation.  The device flushes
 * fp32 denormals, so a luminance below 2^-126 is skipped there where dmt_display_bin counts it. */
enum { DMT_TONE_LINEAR = 0, DMT_TONE_REINHARD = 1, DMT_TONE_ACES = 2, DMT_TONE_HABLE = 3 };
enum { DMT_OETF_LINEAR = 0, DMT_OETF_SRGB = 1, DMT_OETF_GAMMA22 = 2 };
enum { DMT_QUANT_TRUNCATE = 0, DMT_QUANT_ROUND = 1, DMT_QUANT_DITHER = 2 };
typedef struct dmt_display_params {
  int32_t auto_exposure;  /* 0: manual, scale = 2^exposure_ev; otherwise metered, exposure_ev is a compensation on top */
  float exposure_ev;
  float key;              /* auto: the luminance the metered average is mapped to; > 0 */
  float low_fraction;     /* auto: the share of the counted pixels trimmed at the dark end, and */
  float high_fraction;    /*       at the bright end; each in [0, 1), their sum < 1 */
  int32_t bloom_levels;   /* 0 .. 8 */
  float bloom_strength;   /* 0 .. 1 */
  int32_t tone;           /* DMT_TONE_* */
  float white;            /* the curve's white point; 0: its default; >= 0 */
  int32_t oetf;           /* DMT_OETF_* */
  int32_t quantiser;      /* DMT_QUANT_* */
} dmt_display_params;
/* manual 0 EV, key 0.18, fractions 0.10 / 0.05, no bloom (0 levels, strength 0), ACES, sRGB, ROUND, white 0 */
dmt_display_params dmt_display_defaults(void);
/* src4: a host plane of the camera's size (width x height float4, w ignored), or NULL for the context's film mean.  out4
 * (float4, w = 1) and out_rgba8 (4 bytes per pixel) may each be NULL, not both.  params NULL: the defaults.  Synchronous;
 * *kernel_ms (may be NULL) = HIP-event time of its kernels.  Never modifies the film, the AOVs or the temporal history.
 * DMT_ERR_INVALID, with a message and nothing changed, for a non-finite parameter, key <= 0, a fraction outside [0, 1) or a
 * sum >= 1, bloom_levels outside 0 .. 8, bloom_strength outside [0, 1], an unknown enum, white < 0, or both outputs NULL;
 * DMT_ERR_STATE before dmt_set_camera, for a frame of more than 2^31 pixels, and for a NULL source on a context whose dmt_set_partition world is above 1 (its
 * film holds its own tiles only: combine the ranks' films and pass the plane). */
int dmt_display(dmt_ctx* ctx, const dmt_display_params* params, const float* src4, float* out4, uint8_t* out_rgba8, float* kernel_ms);
/* The same with device pointers (e.g. torch data_ptr()): d_src4 NULL for the film mean; d_out4 / d_out_rgba8 as above.
 * Asynchronous on the context's stream, with one exception: auto exposure reads the histogram back, so such a call has waited
 * for the stream up to and including its histogram kernel when it returns. */
int dmt_display_device(dmt_ctx* ctx, const dmt_display_params* params, const void* d_src4, void* d_out4, void* d_out_rgba8);
typedef struct dmt_display_record {
  uint32_t histogram[256]; /* last call, auto exposure: the counts; all 0 after a manual call */
  uint32_t counted;        /* their sum T */
  uint32_t skipped;        /* auto: pixels with y <= 0 */
  uint32_t nonfinite;      /* pixels with a non-finite component */
  int32_t levels;          /* bloom levels used, K' (0: no bloom ran) */
  double avg_log2;         /* auto: the metered average; 0 when nothing was kept */
  float scale;             /* the exposure applied */
  float histogram_ms, bloom_ms, resolve_ms; /* HIP-event times of the stages' kernels; 0 for a stage that did not run */
  int32_t width, height;   /* of the plane */
} dmt_display_record;
/* the record of the last dmt_display / dmt_display_device call; waits for the stream when that call was asynchronous.
 * DMT_ERR_STATE before any call */
int dmt_display_info(dmt_ctx* ctx, dmt_display_record* out);
/* Host only (no GPU): the twins that tests and callers can use.
 * dmt_display_curve: stages 3 and 4 on n already exposed rgb triples.  dmt_display_metering: avg_log2 and scale of a
 * histogram under the parameters' key, fractions and exposure_ev.  dmt_display_bin: the bin of each luminance, -1 where the
 * meter skips it.  DMT_ERR_INVALID for parameters dmt_display would refuse or a null array. */
int dmt_display_curve(const dmt_display_params* params, int n, const float* rgb3_in, float* rgb3_out);
int dmt_display_metering(const dmt_display_params* params, const uint32_t* histogram256, double* avg_log2, float* scale);
int dmt_display_bin(int n, const float* y, int32_t* bin);

/* ---- device unit-test entry points (GPU twins of the reference's T/tests kernels) ---------- */
int dmt_test_triangle_intersect(dmt_ctx* ctx, const float* xs, const float* ys, const float* zs,
                                size_t count, const float* o3, const float* d3, int32_t* hit,
                                float* t, float* pos3, float* nrm3, float* err3);
int dmt_test_sampler(dmt_ctx* ctx, int width, int height, int n, const int32_t* pxs,
                     const int32_t* pys, const int32_t* ss, int ndims, int32_t* halton_index,
                     float* pixel2d, float* dims);
/* fills the sampler table of samples [s0, s0 + n) of a width x height frame as a dmt_render call would and downloads
 * it: out_vals [n][ph][pw][8], out_jitter [n][ph][pw][2] with pw = min(width,128), ph = min(height,128).  Under a pixel
 * filter (dmt_set_pixel_filter) out_jitter is the warped jitter r', which is what the table then holds */
int dmt_test_sampler_table(dmt_ctx* ctx, int width, int height, uint32_t s0, uint32_t n, float* out_vals, float* out_jitter);
/* the film positions (xy2: n x 2) of the samples as the device forms them under the context's pixel filter: the device twin
 * of dmt_pixel_filter_positions */
int dmt_test_film_positions(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* xy2);
/* the camera rays the render kernels trace: lens rays when a lens is set (dmt_set_lens), through the filtered film
 * positions when a pixel filter is set (dmt_set_pixel_filter) */
int dmt_test_camera_rays(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys,
                         const int32_t* ss, float* o3, float* d3);
/* the lens values (u10, u11) of the samples, lens2 (n x 2), as the device computes them */
int dmt_test_lens_values(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* lens2);
/* the times of the samples under the context's shutter, as the motion rows compute them: the device twin of dmt_shutter_times */
int dmt_test_shutter_times(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys, const int32_t* ss, float* t);
/* what the *_medium rows compute between two ray casts, by the device, for a medium given here and not the context's own:
 * medium8 = {sigma_t > 0, g, box min x y z, box max x y z}, checked as dmt_set_medium checks them.  Case i: seg2 / hit = the clip of ray (o3, d3, t_hit) as dmt_medium_segment; values3 = (medium_u(h,
 * depth), the free-flight distance -log1p(-u) / sigma_t for that u, the transmittance exp(-sigma_t (t1 - t0)) of the clipped
 * segment, 1 when it is empty); eval = p_HG(cosine); wi3 / pdf = the direction sampled around wo = -d3 for the numbers u2. */
int dmt_test_medium(dmt_ctx* ctx, const float* medium8, int n, const float* o3, const float* d3, const float* t_hit, const uint32_t* h,
                    const uint32_t* depth, const float* cosine, const float* u2, float* seg2, int32_t* hit, float* values3, float* eval,
                    float* wi3, float* pdf);
/* dmt_medium_spectrum_event by the device, the body the *_rgb rows run: the same arguments and results */
int dmt_test_medium_spectrum(dmt_ctx* ctx, const float* k3, int n, const float* beta3, const uint32_t* h, const uint32_t* depth, const float* tau_seg,
                             int32_t* channel, int32_t* collided, float* tau_at, float* weight3);
/* dmt_medium_grid_march by the device, the body the *_medium_grid rows run, for a grid given here and not the context's own:
 * medium7 = {sigma_t, box min x y z, box max x y z}, the rest as dmt_medium_grid_march */
int dmt_test_medium_grid(dmt_ctx* ctx, const float* medium7, int nx, int ny, int nz, const float* density, int n, const float* o3,
                         const float* d3, const float* t_end, const float* tau_target, float* tau, float* ts, int32_t* collided,
                         int32_t* steps);
/* one trace call of the render kernels for the ray pairs (closest ray o3 / d3, shadow ray so3 / sd3 up to smax) under the
 * current accel mode, a wave of 64 pairs at a time as the megakernel traces them (brute force: the always list, then the
 * culled clusters): tri_index (-1: none) and barycentrics uv2 (n x 2) of the closest ray's hit, occluded[i] = the shadow
 * ray meets a triangle before smax[i].  Key 0, solid geometry. */
int dmt_test_trace_pair(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* so3, const float* sd3, const float* smax,
                        int32_t* tri_index, float* uv2, uint8_t* occluded);
/* closest hit of ray i against the scene at time[i], under the current accel mode (the motion tree for DMT_ACCEL_BVH):
 * tri_index (-1: none), t (+inf: none) and, when uv2 is not null, the barycentrics (n x 2).  DMT_ERR_STATE without key 1.
 * dmt_test_closest_hit keeps answering for key 0. */
int dmt_test_closest_hit_at(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* time, int32_t* tri_index, float* t,
                            float* uv2);
/* shading_normal_at of the uploaded vertex normals: the shading normal ns3 (n x 3) of triangle tri[i] at barycentrics
 * (bu, bv) for a ray of direction rd3[i]; ngFacing is the stored geometric normal flipped against rd as at a hit.
 * DMT_ERR_STATE without vertex normals. */
int dmt_test_shading_normal(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* rd3, float* ns3);
/* the same, then the material's normal map (level 0) applied around it as the *_tex_vn rows apply it; needs BSDFs and
 * textures uploaded */
int dmt_test_shading_normal_mapped(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* rd3,
                                   float* ns3);
/* the cutout lookup on the uploaded scene, by the device function the cutout rows run: alpha8[i] and pass[i] of triangle tri[i]
 * at barycentrics (bu, bv); a triangle of an opaque material answers 255 and passes.  DMT_ERR_STATE without opacity. */
int dmt_test_opacity(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, float* alpha8, uint8_t* pass);
/* ray i under the cutout rule and the current accel mode, through the trace the cutout rows run: the closest PASSING hit --
 * tri_index (-1: none), t (+inf: none), uv2 (n x 2, may be null) -- and occluded[i] (may be null) = some valid and passing
 * hit has t < tmax[i].  DMT_ERR_STATE without opacity.  dmt_test_closest_hit keeps answering for solid geometry. */
int dmt_test_closest_hit_opacity(dmt_ctx* ctx, int nrays, const float* o3, const float* d3, const float* tmax, int32_t* tri_index, float* t,
                                 float* uv2, uint8_t* occluded);
/* dmt_camera_project on the device, under the camera of dmt_set_camera */
int dmt_test_camera_project(dmt_ctx* ctx, int n, const float* p3, float* xy2, float* depth);
int dmt_test_bsdf(dmt_ctx* ctx, const void* bsdf32, int n, const float* ns3, const float* wo3,
                  const float* u2, const float* uc, const float* wi_eval3, float* prepared12,
                  float* sample10, float* eval4);
/* dmt_test_bsdf with a geometric normal of its own (ng3) handed to the sampling and evaluation routines, as the render
 * kernels do under a normal map; same output layouts */
int dmt_test_bsdf_ng(dmt_ctx* ctx, const void* bsdf32, int n, const float* ns3, const float* ng3, const float* wo3,
                     const float* u2, const float* uc, const float* wi_eval3, float* prepared12, float* sample10,
                     float* eval4);
/* the material of triangle tri[i] of the uploaded scene at barycentrics (bu, bv), as the shading code patches it from the
 * level-0 texture lookups: the 32-byte record (rec32) and the shading normal (ns3) for the geometric normal ng3[i].  A
 * fractional-metallic pair also returns its second record (rec2_32) and the metallic fraction (mix); zero otherwise. */
int dmt_test_material(dmt_ctx* ctx, int n, const int32_t* tri, const float* bu, const float* bv, const float* ng3, void* rec32,
                      float* ns3, void* rec2_32, float* mix);
int dmt_test_light(dmt_ctx* ctx, const void* light32, int n, const float* pos3, const float* nrm3,
                   const float* u2, const int32_t* had_transmission, float* out14);
/* the light choice of a bounce at n shading points (pos3, nrm3) with one random number u each, on the device: the selection
 * function of the context's light sampling mode on the tree it built from the uploaded lights.  DMT_LIGHTS_TREE: counts[i] is
 * 0 or 1, indices4[4 i] the light and pmfs4[4 i] = start_pmf x the tree's probability; DMT_LIGHTS_TREE_REFERENCE: the cut's
 * up to four (light, pmf) pairs as dmt_light_tree_ref_select returns them.  Slots past counts[i] hold -1 / 0.  DMT_ERR_STATE
 * where the context would not use a tree: uniform mode, fewer than two lights, a list that cannot be put in a tree, a tree
 * deeper than the walk's guard. */
int dmt_test_light_tree(dmt_ctx* ctx, int n, const float* pos3, const float* nrm3, const float* u, float start_pmf, int32_t* indices4,
                        float* pmfs4, int32_t* counts);
/* the emitter choice of a bounce at n shading points (pos3, nrm3) with one random number u each, on the device: et_select and
 * et_pmf themselves, one lane per case, on the tree the context uploaded.  index_out: the emitter or -1; pmf_out = start_pmf x
 * the walk's probability; pmf_by_trail_out = start_pmf x et_pmf along the selected emitter's trail (0 where none).
 * DMT_ERR_STATE, with the reason, where the emitter tree is not active (dmt_emitter_tree_info). */
/* scratch (private segment) bytes per lane of the kernel dmt_render would launch now; 0: no spills, no stack */
int dmt_kernel_scratch(dmt_ctx* ctx, int* scratch_bytes);
int dmt_test_emitter_tree(dmt_ctx* ctx, int n, const float* pos3, const float* nrm3, const float* u, float start_pmf, int32_t* index_out,
                          float* pmf_out, float* pmf_by_trail_out);
int dmt_test_half(dmt_ctx* ctx, int n, const float* f_in, uint16_t* h_out, const uint16_t* h_in,
                  float* f_out);
/* radiance of individual (pixel, sample) paths of the uploaded scene */
int dmt_test_trace_samples(dmt_ctx* ctx, int n, const int32_t* pxs, const int32_t* pys,
                           const int32_t* ss, float* L3);
/* per-bounce log of one path: records of 12 floats {tri, pos3, beta3, L3 before shading, depth,
 * sampler dimension}; *n_out = records written (<= cap) */
int dmt_test_trace_log(dmt_ctx* ctx, int px, int py, int s, float* rec12, int cap, int* n_out,
                       float* L3);
/* closest hit (triangle index or -1, t) of rays against the uploaded scene, current accel mode */
int dmt_test_closest_hit(dmt_ctx* ctx, int nrays, const float* o3, const float* d3,
                         int32_t* tri_index, float* t);

#ifdef __cplusplus
}
#endif
#endif /* DMT_HIP_H */
