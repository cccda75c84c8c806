"""ctypes binding of include/dmt_hip.h.  Plumbing only -- every call goes to libdmt_hip.so."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE / "csrc"
_LIB = None

DMT_ACCEL_BRUTE_FORCE = 0
DMT_ACCEL_BVH = 1
# dmt_set_accel_build modes and dmt_accel_build_record.builder values (include/dmt_hip.h)
BVH_BUILD_HOST = 0
BVH_BUILD_DEVICE = 1
BVH_BUILT_BY_HOST = 0
BVH_BUILT_BY_DEVICE = 1
BVH_BUILT_BY_HOST_AFTER_DEVICE = 2
# dmt_set_accel_update modes and dmt_accel_update_record.action values
BVH_UPDATE_REBUILD = 0
BVH_UPDATE_REFIT = 1
BVH_UPDATE_AUTO = 2
BVH_UPDATED_NONE = 0
BVH_UPDATED_REFIT = 1
BVH_UPDATED_REBUILD = 2
BVH_UPDATED_REBUILD_AFTER_REFIT = 3


class DmtError(RuntimeError):
    pass


def library_path():
    # DMT_HIP_LIB: developer knob to A/B an experimental build of the same C ABI
    import os
    alt = os.environ.get("DMT_HIP_LIB")
    return Path(alt) if alt else _CSRC / "libdmt_hip.so"


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of the HIP library, in-tree."""
    args = ["make", "-C", str(_CSRC)]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return library_path()


def load_library():
    """Load libdmt_hip.so.  Raises if it has not been built -- there is no CPU fallback."""
    global _LIB
    if _LIB is None:
        so = library_path()
        if not so.exists():
            raise DmtError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP path has no fallback)")
        lib = C.CDLL(str(so))
        lib.dmt_last_error.restype = C.c_char_p
        lib.dmt_last_error.argtypes = [C.c_void_p]
        _LIB = lib
    return _LIB


# every symbol include/dmt_hip.h declares (checked by tests/test_abi.py against the header text)
EXPORTED_SYMBOLS = [
    "dmt_ctx_create", "dmt_ctx_destroy", "dmt_last_error", "dmt_upload_triangles", "dmt_upload_bsdfs",
    "dmt_upload_lights", "dmt_uniform_lights_info", "dmt_set_camera", "dmt_set_limits", "dmt_set_accel", "dmt_set_light_sampling", "dmt_light_tree_pmfs", "dmt_light_tree_ref_select", "dmt_light_tree_nodes", "dmt_test_light_tree", "dmt_set_emitter_sampling", "dmt_emitter_tree_info", "dmt_emitter_tree_nodes", "dmt_emitter_tree_select", "dmt_emitter_tree_pmfs", "dmt_test_emitter_tree", "dmt_kernel_scratch", "dmt_set_bvh_strategy", "dmt_set_partition", "dmt_set_chunk", "dmt_render_profile",
    "dmt_upload_area_lights", "dmt_upload_textures", "dmt_upload_envmap", "dmt_clear_envmap", "dmt_envmap_tables", "dmt_test_envmap",
    "dmt_set_stream", "dmt_film_clear", "dmt_film_bind", "dmt_film_device_ptrs", "dmt_download_film",
    "dmt_render", "dmt_render_adaptive", "dmt_render_stats", "dmt_sync", "dmt_sched_diag", "dmt_kernel_time", "dmt_kernel_info", "dmt_bvh_validate", "dmt_brute_cull_plan", "dmt_brute_cull_box_plan", "dmt_brute_cull_box_records", "dmt_cull_records", "dmt_cull_box_test", "dmt_test_triangle_intersect",
    "dmt_test_sampler", "dmt_test_camera_rays", "dmt_test_bsdf", "dmt_test_bsdf_ng", "dmt_test_material", "dmt_test_light", "dmt_test_half",
    "dmt_test_trace_samples", "dmt_test_trace_log", "dmt_test_closest_hit", "dmt_test_trace_pair",
    "dmt_set_texture_filter", "dmt_texture_mip_chain", "dmt_texture_footprint", "dmt_test_texture_filter",
    "dmt_render_aovs", "dmt_upload_aovs", "dmt_download_aovs", "dmt_denoise_defaults", "dmt_denoise",
    "dmt_set_accel_build", "dmt_accel_build_info", "dmt_accel_download", "dmt_lbvh_reference", "dmt_bvh_check",
    "dmt_update_vertices", "dmt_update_vertices_device", "dmt_set_accel_update", "dmt_accel_update_info", "dmt_bvh_refit_reference",
    "dmt_download_aov_surface", "dmt_upload_aov_surface", "dmt_camera_project", "dmt_test_camera_project", "dmt_temporal_defaults",
    "dmt_denoise_temporal", "dmt_temporal_reset", "dmt_temporal_info", "dmt_temporal_download",
    "dmt_display_defaults", "dmt_display", "dmt_display_device", "dmt_display_info", "dmt_display_curve", "dmt_display_metering",
    "dmt_display_bin",
    "dmt_set_sampler_table", "dmt_sampler_table_plan", "dmt_test_sampler_table",
    "dmt_set_lens", "dmt_lens_info", "dmt_lens_rays", "dmt_focus_distance_at", "dmt_test_lens_values",
    "dmt_set_pixel_filter", "dmt_pixel_filter_info", "dmt_pixel_filter_table", "dmt_pixel_filter_positions", "dmt_test_film_positions",
    "dmt_set_projection", "dmt_projection_info", "dmt_projection_rays", "dmt_projection_project",
    "dmt_set_motion", "dmt_clear_motion", "dmt_set_shutter", "dmt_motion_info", "dmt_shutter_times", "dmt_motion_positions",
    "dmt_motion_bvh_validate", "dmt_test_shutter_times", "dmt_test_closest_hit_at",
    "dmt_upload_vertex_normals", "dmt_clear_vertex_normals", "dmt_vertex_normals_info", "dmt_smooth_normals",
    "dmt_test_shading_normal", "dmt_test_shading_normal_mapped",
    "dmt_set_ggx_batch", "dmt_ggx_batch_diag", "dmt_tri_kind_bits",
    "dmt_upload_opacity", "dmt_clear_opacity", "dmt_opacity_info", "dmt_opacity_eval", "dmt_test_opacity", "dmt_test_closest_hit_opacity",
    "dmt_set_medium", "dmt_clear_medium", "dmt_medium_info", "dmt_medium_segment", "dmt_medium_values", "dmt_phase_hg", "dmt_test_medium",
    "dmt_set_medium_grid", "dmt_set_medium_grid_device", "dmt_clear_medium_grid", "dmt_medium_grid_info", "dmt_medium_grid_march", "dmt_test_medium_grid",
    "dmt_set_medium_spectrum", "dmt_clear_medium_spectrum", "dmt_medium_spectrum_info", "dmt_medium_spectrum_event", "dmt_test_medium_spectrum",
]

# dmt_set_sampler_table modes (include/dmt_hip.h)
SAMPLER_TABLE_OFF = 0
SAMPLER_TABLE_AUTO = 1
SAMPLER_TABLE_FORCE = 2


class SamplerTablePlanRecord(C.Structure):
    """dmt_sampler_table_plan_record (include/dmt_hip.h)"""
    _fields_ = [("use", C.c_uint32), ("period_width", C.c_uint32), ("period_height", C.c_uint32), ("entry_bytes", C.c_uint32),
                ("slices", C.c_uint32), ("reserved", C.c_uint32), ("slice_bytes", C.c_uint64)]


def sampler_table_plan(width, height, owned_pixels, spp, chunk_spp, budget_bytes=0, mode=SAMPLER_TABLE_AUTO):
    """Host only (dmt_sampler_table_plan): what a render call does with its sampler table.  Returns a dict: use,
    period_width, period_height, entry_bytes, slices, slice_bytes, slice_spp (list of the slices' sample counts)."""
    lib = load_library()
    rec = SamplerTablePlanRecord()
    args = [int(width), int(height), C.c_uint64(int(owned_pixels)), C.c_uint32(int(spp)), C.c_uint32(int(chunk_spp)),
            C.c_uint64(int(budget_bytes)), int(mode)]
    rc = lib.dmt_sampler_table_plan(*args, C.byref(rec), None, C.c_uint32(0))
    if rc != 0:
        raise DmtError(f"dmt_sampler_table_plan failed ({rc})")
    lens = (C.c_uint32 * max(int(rec.slices), 1))()
    rc = lib.dmt_sampler_table_plan(*args, C.byref(rec), lens, C.c_uint32(int(rec.slices)))
    if rc != 0:
        raise DmtError(f"dmt_sampler_table_plan failed ({rc})")
    out = {name: int(getattr(rec, name)) for name, _ in SamplerTablePlanRecord._fields_ if name != "reserved"}
    out["use"] = bool(rec.use)
    out["slice_spp"] = [int(x) for x in lens[:int(rec.slices)]]
    return out


class DenoiseParams(C.Structure):
    """dmt_denoise_params (include/dmt_hip.h)"""
    _fields_ = [("iterations", C.c_int32), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_luminance", C.c_float)]


def denoise_defaults():
    """dmt_denoise_defaults() as a dict: iterations, sigma_normal, sigma_position, sigma_albedo, sigma_luminance."""
    lib = load_library()
    lib.dmt_denoise_defaults.restype = DenoiseParams
    p = lib.dmt_denoise_defaults()
    return {name: getattr(p, name) for name, _ in DenoiseParams._fields_}



class TemporalParams(C.Structure):
    """dmt_temporal_params (include/dmt_hip.h)"""
    _fields_ = [("alpha", C.c_float), ("normal_threshold", C.c_float), ("plane_threshold", C.c_float)]


class TemporalRecord(C.Structure):
    """dmt_temporal_record (include/dmt_hip.h)"""
    _fields_ = [("frames", C.c_uint32), ("reprojected", C.c_uint32), ("reset", C.c_uint32), ("temporal_ms", C.c_float),
                ("history_bytes", C.c_uint64)]


def temporal_defaults():
    """dmt_temporal_defaults() as a dict: alpha, normal_threshold, plane_threshold."""
    lib = load_library()
    lib.dmt_temporal_defaults.restype = TemporalParams
    p = lib.dmt_temporal_defaults()
    return {name: getattr(p, name) for name, _ in TemporalParams._fields_}


# dmt_display_params enums (include/dmt_hip.h)
TONE_LINEAR, TONE_REINHARD, TONE_ACES, TONE_HABLE = 0, 1, 2, 3
OETF_LINEAR, OETF_SRGB, OETF_GAMMA22 = 0, 1, 2
QUANT_TRUNCATE, QUANT_ROUND, QUANT_DITHER = 0, 1, 2


class DisplayParams(C.Structure):
    """dmt_display_params (include/dmt_hip.h)"""
    _fields_ = [("auto_exposure", C.c_int32), ("exposure_ev", C.c_float), ("key", C.c_float), ("low_fraction", C.c_float),
                ("high_fraction", C.c_float), ("bloom_levels", C.c_int32), ("bloom_strength", C.c_float), ("tone", C.c_int32),
                ("white", C.c_float), ("oetf", C.c_int32), ("quantiser", C.c_int32)]


class DisplayRecord(C.Structure):
    """dmt_display_record (include/dmt_hip.h)"""
    _fields_ = [("histogram", C.c_uint32 * 256), ("counted", C.c_uint32), ("skipped", C.c_uint32), ("nonfinite", C.c_uint32),
                ("levels", C.c_int32), ("avg_log2", C.c_double), ("scale", C.c_float), ("histogram_ms", C.c_float),
                ("bloom_ms", C.c_float), ("resolve_ms", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


def display_defaults():
    """dmt_display_defaults() as a dict: auto_exposure, exposure_ev, key, low_fraction, high_fraction, bloom_levels,
    bloom_strength, tone, white, oetf, quantiser."""
    lib = load_library()
    lib.dmt_display_defaults.restype = DisplayParams
    p = lib.dmt_display_defaults()
    return {name: getattr(p, name) for name, _ in DisplayParams._fields_}


def _display_params(params):
    p = display_defaults()
    unknown = set(params or {}) - set(p)
    if unknown:
        raise ValueError(f"unknown display parameters {sorted(unknown)}")
    p.update(params or {})
    return DisplayParams(*[(int if t is C.c_int32 else float)(p[name]) for name, t in DisplayParams._fields_])


def display_curve(rgb, params=None):
    """Host only (dmt_display_curve): the tone curve and the transfer function of `params` on already exposed rgb triples."""
    a = np.ascontiguousarray(rgb, np.float32)
    assert a.shape[-1] == 3
    out = np.zeros_like(a)
    cp = _display_params(params)
    rc = load_library().dmt_display_curve(C.byref(cp), int(a.size // 3), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DmtError(f"dmt_display_curve failed ({rc})")
    return out


def display_metering(histogram, params=None):
    """Host only (dmt_display_metering): (avg_log2, scale) of a 256-bin histogram under the parameters' key, fractions and
    exposure_ev; scale is a numpy float32."""
    h = np.ascontiguousarray(histogram, np.uint32)
    assert h.shape == (256,)
    cp = _display_params(params)
    avg, scale = C.c_double(), C.c_float()
    rc = load_library().dmt_display_metering(C.byref(cp), h.ctypes.data_as(C.c_void_p), C.byref(avg), C.byref(scale))
    if rc != 0:
        raise DmtError(f"dmt_display_metering failed ({rc})")
    return avg.value, np.float32(scale.value)


def display_bin(y):
    """Host only (dmt_display_bin): the histogram bin of each luminance, int32; -1 where the meter skips it."""
    a = np.ascontiguousarray(y, np.float32)
    out = np.zeros(a.shape, np.int32)
    rc = load_library().dmt_display_bin(int(a.size), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DmtError(f"dmt_display_bin failed ({rc})")
    return out


def camera_project(camera44, points):
    """Host only (dmt_camera_project): render-space points [n, 3] -> (film coordinates [n, 2], camera-space depth [n])."""
    lib = load_library()
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    xy, depth = np.zeros((p.shape[0], 2), np.float32), np.zeros(p.shape[0], np.float32)
    rc = lib.dmt_camera_project(cam.ctypes.data_as(C.c_void_p), int(p.shape[0]), p.ctypes.data_as(C.c_void_p),
                                xy.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DmtError(f"dmt_camera_project failed ({rc})")
    return xy, depth


def lens_rays(camera44, lens_radius, focus_distance, pxs, pys, ss):
    """Host only (dmt_lens_rays): the camera rays of samples ss of pixels (pxs, pys) under a thin lens (radius 0: the pinhole
    rays) -> (origins [n, 3], directions [n, 3], lens values (u10, u11) [n, 2]).  The serial twin of the device code."""
    lib = load_library()
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    pxs, pys, ss = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (pxs, pys, ss))
    n = pxs.shape[0]
    assert pys.shape[0] == n and ss.shape[0] == n
    o, d, u = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dmt_lens_rays(as_p(cam), C.c_float(lens_radius), C.c_float(focus_distance), int(n), as_p(pxs), as_p(pys), as_p(ss),
                           as_p(o), as_p(d), as_p(u))
    if rc != 0:
        raise DmtError(f"dmt_lens_rays failed ({rc})")
    return o, d, u


# dmt_set_projection kinds (include/dmt_hip.h)
PROJECTION_PERSPECTIVE = 0
PROJECTION_ORTHOGRAPHIC = 1
PROJECTION_EQUIRECT = 2
PROJECTION_FISHEYE = 3
PROJECTION_KINDS = {"perspective": PROJECTION_PERSPECTIVE, "orthographic": PROJECTION_ORTHOGRAPHIC, "equirect": PROJECTION_EQUIRECT,
                    "fisheye": PROJECTION_FISHEYE}


def _projection_kind(kind, who):
    if isinstance(kind, str):
        if kind not in PROJECTION_KINDS:
            raise DmtError(f"{who}: unsupported projection '{kind}'")
        return PROJECTION_KINDS[kind]
    return int(kind)


def projection_rays(camera44, kind, param, xy):
    """Host only (dmt_projection_rays): the rays through the continuous film positions xy [n, 2] of the camera under a
    projection (kind or its name; param: the orthographic view height or the fisheye's diagonal field of view in degrees)
    -> (origins [n, 3], directions [n, 3]).  The serial twin of the device code."""
    lib = load_library()
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = xy.shape[0]
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dmt_projection_rays(as_p(cam), _projection_kind(kind, "projection_rays"), C.c_float(param), int(n), as_p(xy), as_p(o), as_p(d))
    if rc != 0:
        raise DmtError(f"dmt_projection_rays failed ({rc})")
    return o, d


def projection_project(camera44, kind, param, points):
    """Host only (dmt_projection_project): render-space points [n, 3] -> (film coordinates [n, 2], depth [n]) under a
    projection; the depth is the camera-space z for perspective and orthographic, the distance for equirect and fisheye."""
    lib = load_library()
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    xy, depth = np.zeros((p.shape[0], 2), np.float32), np.zeros(p.shape[0], np.float32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dmt_projection_project(as_p(cam), _projection_kind(kind, "projection_project"), C.c_float(param), int(p.shape[0]), as_p(p),
                                    as_p(xy), as_p(depth))
    if rc != 0:
        raise DmtError(f"dmt_projection_project failed ({rc})")
    return xy, depth


# dmt_set_pixel_filter kinds (include/dmt_hip.h)
FILTER_BOX = 0
FILTER_TENT = 1
FILTER_GAUSSIAN = 2
FILTER_BLACKMAN_HARRIS = 3
PIXEL_FILTER_KINDS = {"box": FILTER_BOX, "tent": FILTER_TENT, "triangle": FILTER_TENT, "gaussian": FILTER_GAUSSIAN,
                      "blackman-harris": FILTER_BLACKMAN_HARRIS}


def pixel_filter_table(kind, radius, param=0.0):
    """Host only (dmt_pixel_filter_table): the 257 float32 knots W(i / 256) of the filter's inverse CDF over [-1, 1]."""
    lib = load_library()
    knots = np.zeros(257, np.float32)
    rc = lib.dmt_pixel_filter_table(int(kind), C.c_float(radius), C.c_float(param), knots.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DmtError(f"dmt_pixel_filter_table failed ({rc})")
    return knots


def pixel_filter_positions(width, height, kind, radius, param, pxs, pys, ss):
    """Host only (dmt_pixel_filter_positions): the film positions [n, 2] of samples ss of pixels (pxs, pys) of a
    width x height frame under the filter (box with radius 0.5: the unfiltered positions), the device's bit for bit."""
    lib = load_library()
    pxs, pys, ss = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (pxs, pys, ss))
    n = pxs.shape[0]
    assert pys.shape[0] == n and ss.shape[0] == n
    xy = np.zeros((n, 2), np.float32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dmt_pixel_filter_positions(int(width), int(height), int(kind), C.c_float(radius), C.c_float(param), int(n), as_p(pxs),
                                        as_p(pys), as_p(ss), as_p(xy))
    if rc != 0:
        raise DmtError(f"dmt_pixel_filter_positions failed ({rc})")
    return xy


def shutter_times(width, height, open, close, pxs, pys, ss):
    """Host only (dmt_shutter_times): the times [n] of samples ss of pixels (pxs, pys) of a width x height frame under the
    shutter [open, close], the device's bit for bit."""
    lib = load_library()
    pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
    n = pxs.shape[0]
    assert pys.shape[0] == n and ss.shape[0] == n
    t = np.zeros(n, np.float32)
    rc = lib.dmt_shutter_times(int(width), int(height), C.c_float(open), C.c_float(close), int(n), _p(pxs), _p(pys), _p(ss), _p(t))
    if rc != 0:
        raise DmtError(f"dmt_shutter_times failed ({rc})")
    return t


def motion_positions(xs0, ys0, zs0, xs1, ys1, zs1, t):
    """Host only (dmt_motion_positions): the vertices at time t between key 0 and key 1, fmaf(t, p1 - p0, p0) in fp32, the
    device's bit for bit.  Layout as upload_triangles; returns (xs, ys, zs)."""
    lib = load_library()
    a = [_f32(v).reshape(-1) for v in (xs0, ys0, zs0, xs1, ys1, zs1)]
    n = a[0].size // 4
    assert all(v.size == 4 * n for v in a)
    out = [np.zeros(4 * n, np.float32) for _ in range(3)]
    rc = lib.dmt_motion_positions(*[_p(v) for v in a], C.c_size_t(n), C.c_float(t), *[_p(v) for v in out])
    if rc != 0:
        raise DmtError(f"dmt_motion_positions failed ({rc})")
    return tuple(out)


def motion_bvh_validate(xs0, ys0, zs0, xs1, ys1, zs1):
    """Host only (dmt_motion_bvh_validate): builds the motion tree of the two keys and checks it against both; returns
    dict(ok, node_count, pair_count, depth)."""
    lib = load_library()
    a = [_f32(v).reshape(-1) for v in (xs0, ys0, zs0, xs1, ys1, zs1)]
    n = a[0].size // 4
    assert all(v.size == 4 * n for v in a)
    nc, pc, d = C.c_int(), C.c_int(), C.c_int()
    rc = lib.dmt_motion_bvh_validate(*[_p(v) for v in a], C.c_size_t(n), C.byref(nc), C.byref(pc), C.byref(d))
    return {"ok": rc == 0, "node_count": nc.value, "pair_count": pc.value, "depth": d.value}


def smooth_normals(xs, ys, zs, crease_degrees=180.0):
    """Host only (dmt_smooth_normals): angle-weighted vertex normals [n, 9] for a soup laid out as upload_triangles; corners
    with bit-equal positions are welded, faces beyond crease_degrees of a corner's own face do not contribute, zero-area
    triangles come out flat (zeros)."""
    lib = load_library()
    xs, ys, zs = _f32(xs).reshape(-1), _f32(ys).reshape(-1), _f32(zs).reshape(-1)
    n = xs.size // 4
    assert xs.size == 4 * n and ys.size == 4 * n and zs.size == 4 * n
    out = np.zeros((n, 9), np.float32)
    rc = lib.dmt_smooth_normals(_p(xs), _p(ys), _p(zs), C.c_size_t(n), C.c_float(crease_degrees), _p(out))
    if rc != 0:
        raise DmtError(f"dmt_smooth_normals failed ({rc})")
    return out


def _u32(a):
    return np.ascontiguousarray(a, np.uint32).reshape(-1)


def medium_segment(box_min, box_max, o, d, t_hit):
    """Host only (dmt_medium_segment): the clip of rays (o, d: [n, 3]) ending at t_hit [n] (may be +inf) against the box, the
    device's bit for bit -> (seg [n, 2] = (t0, t1), hit [n] bool = t0 < t1)."""
    lib = load_library()
    o, d = _f32(o).reshape(-1, 3), _f32(d).reshape(-1, 3)
    t = _f32(t_hit).reshape(-1)
    n = o.shape[0]
    assert d.shape[0] == n and t.shape[0] == n
    seg, hit = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
    rc = lib.dmt_medium_segment(_p(_f32(box_min, (3,))), _p(_f32(box_max, (3,))), int(n), _p(o), _p(d), _p(t), _p(seg), _p(hit))
    if rc != 0:
        raise DmtError(f"dmt_medium_segment failed ({rc})")
    return seg, hit.astype(bool)


def medium_values(h, depth):
    """Host only (dmt_medium_values): the free-flight numbers medium_u(h, depth) [n] in [0, 1), the device's bit for bit."""
    lib = load_library()
    h, depth = _u32(h), _u32(depth)
    assert h.shape[0] == depth.shape[0]
    u = np.zeros(h.shape[0], np.float32)
    rc = lib.dmt_medium_values(int(h.shape[0]), _p(h), _p(depth), _p(u))
    if rc != 0:
        raise DmtError(f"dmt_medium_values failed ({rc})")
    return u


def phase_hg(g, cosine=None, wo=None, u=None):
    """Host only (dmt_phase_hg): Henyey-Greenstein of asymmetry g in fp32.  With cosine [n] = dot(wo, wi): eval [n].  With wo
    [n, 3] (unit) and u [n, 2]: (wi [n, 3], pdf [n]).  With both: (eval, wi, pdf)."""
    lib = load_library()
    ev = wi = pdf = None
    n = 0
    if cosine is not None:
        cosine = _f32(cosine).reshape(-1)
        n, ev = cosine.shape[0], np.zeros(cosine.shape[0], np.float32)
    if wo is not None or u is not None:
        wo, u = _f32(wo).reshape(-1, 3), _f32(u).reshape(-1, 2)
        assert wo.shape[0] == u.shape[0] and (cosine is None or wo.shape[0] == n)
        n, wi, pdf = wo.shape[0], np.zeros(wo.shape, np.float32), np.zeros(wo.shape[0], np.float32)
    rc = lib.dmt_phase_hg(C.c_float(g), int(n), _p(cosine), _p(ev), _p(wo), _p(u), _p(wi), _p(pdf))
    if rc != 0:
        raise DmtError(f"dmt_phase_hg failed ({rc})")
    if wi is None:
        return ev
    return (wi, pdf) if ev is None else (ev, wi, pdf)


def _grid_call(density, o, d, t_end, tau_target):
    """the arrays of dmt_medium_grid_march / dmt_test_medium_grid: density [nz, ny, nx], n rays, four outputs"""
    density = _f32(density)
    assert density.ndim == 3, "the density grid has shape (nz, ny, nx)"
    o, d = _f32(o).reshape(-1, 3), _f32(d).reshape(-1, 3)
    t, target = _f32(t_end).reshape(-1), _f32(tau_target).reshape(-1)
    n = o.shape[0]
    assert d.shape[0] == n and t.shape[0] == n and target.shape[0] == n
    out = dict(tau=np.zeros(n, np.float32), ts=np.zeros(n, np.float32), collided=np.zeros(n, np.int32), steps=np.zeros(n, np.int32))
    return density, o, d, t, target, n, out


def medium_grid_march(box_min, box_max, sigma_t, density, o, d, t_end, tau_target):
    """Host only (dmt_medium_grid_march): the voxel march of rays (o, d: [n, 3]) over [0, t_end] up to the optical depth
    tau_target (both [n], may be +inf) through the grid density [nz, ny, nx] in the box, the device's bit for bit ->
    dict(tau [n], ts [n], collided [n] bool, steps [n])."""
    lib = load_library()
    density, o, d, t, target, n, out = _grid_call(density, o, d, t_end, tau_target)
    nz, ny, nx = density.shape
    rc = lib.dmt_medium_grid_march(_p(_f32(box_min, (3,))), _p(_f32(box_max, (3,))), C.c_float(sigma_t), int(nx), int(ny), int(nz), _p(density),
                                   int(n), _p(o), _p(d), _p(t), _p(target), _p(out["tau"]), _p(out["ts"]), _p(out["collided"]), _p(out["steps"]))
    if rc != 0:
        raise DmtError(f"dmt_medium_grid_march failed ({rc})")
    out["collided"] = out["collided"].astype(bool)
    return out


def _spectrum_call(beta, h, depth, tau_seg):
    """the arrays of dmt_medium_spectrum_event / dmt_test_medium_spectrum: n cases, four outputs"""
    beta, tau = _f32(beta).reshape(-1, 3), _f32(tau_seg).reshape(-1)
    h, depth = _u32(h), _u32(depth)
    n = beta.shape[0]
    assert h.shape[0] == n and depth.shape[0] == n and tau.shape[0] == n
    out = dict(channel=np.zeros(n, np.int32), collided=np.zeros(n, np.int32), tau_at=np.zeros(n, np.float32), weight=np.zeros((n, 3), np.float32))
    return beta, h, depth, tau, n, out


def medium_spectrum_event(k, beta, h, depth, tau_seg):
    """Host only (dmt_medium_spectrum_event): the event of n path segments in a medium of channel extinctions k (3): the
    throughputs beta [n, 3], Halton indices h [n], depths [n] and channel-m optical depths tau_seg [n] (may be +inf) ->
    dict(channel [n] (-1 without an event), collided [n] bool, tau_at [n], weight [n, 3]); the decisions are the device's
    bit for bit."""
    lib = load_library()
    beta, h, depth, tau, n, out = _spectrum_call(beta, h, depth, tau_seg)
    rc = lib.dmt_medium_spectrum_event(_p(_f32(k, (3,))), int(n), _p(beta), _p(h), _p(depth), _p(tau), _p(out["channel"]), _p(out["collided"]),
                                       _p(out["tau_at"]), _p(out["weight"]))
    if rc != 0:
        raise DmtError(f"dmt_medium_spectrum_event failed ({rc})")
    out["collided"] = out["collided"].astype(bool)
    return out


OPACITY_NONE = 0xFFFFFFFF  # dmt_upload_opacity: the material is opaque


def opacity_eval(tex_rgba, tex_desc, tex, uv6, bu, bv, cutoff=0.5):
    """Host only (dmt_opacity_eval): the cutout lookup of texture tex[i] (textures as upload_textures takes them) for a
    triangle with UVs uv6[i] at barycentrics (bu[i], bv[i]), the device's bit for bit.  Returns (alpha8 [n] float32,
    passes [n] bool), passes = alpha8 >= cutoff * 255."""
    lib = load_library()
    rgba = np.ascontiguousarray(tex_rgba, np.uint8).reshape(-1, 4)
    desc = np.ascontiguousarray(tex_desc, np.int32).reshape(-1, 3)
    tex, uv6 = _i32(tex).reshape(-1), _f32(uv6).reshape(-1, 6)
    bu, bv = _f32(bu).reshape(-1), _f32(bv).reshape(-1)
    n = tex.shape[0]
    assert uv6.shape[0] == n and bu.shape[0] == n and bv.shape[0] == n
    a, ok = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    rc = lib.dmt_opacity_eval(_p(rgba), C.c_uint64(rgba.shape[0]), _p(desc), C.c_uint32(desc.shape[0]), int(n), _p(tex), _p(uv6), _p(bu),
                              _p(bv), C.c_float(cutoff), _p(a), _p(ok))
    if rc != 0:
        raise DmtError(f"dmt_opacity_eval failed ({rc})")
    return a, ok.astype(bool)


# dmt_set_texture_filter modes (include/dmt_hip.h)
TEXFILTER_LEVEL0 = 0
TEXFILTER_REFERENCE = 1


def mip_level_count(width, height):
    """The reference's MIP level count: halve both sides until both reach 0 (core-texture.cu:360-366)."""
    n, w, h = 0, int(width), int(height)
    while w > 0 or h > 0:
        n, w, h = n + 1, w >> 1, h >> 1
    return n


def texture_mip_chain(rgba8):
    """Host only: MIP levels 1.. of one texture (h x w x 4 uint8) as dmt_upload_textures builds them.  Returns
    (levels, [level 1 array, level 2 array, ...]), each level (max(1, h >> l), max(1, w >> l), 4) uint8."""
    lib = load_library()
    img = np.ascontiguousarray(rgba8, np.uint8)
    h, w = img.shape[:2]
    levels = mip_level_count(w, h)
    sizes = [(max(1, h >> l), max(1, w >> l)) for l in range(1, levels)]
    total = sum(a * b for a, b in sizes)
    out = np.zeros(max(total, 1) * 4, np.uint8)
    n = C.c_int()
    rc = lib.dmt_texture_mip_chain(_p(img), int(w), int(h), _p(out), C.c_uint64(total), C.byref(n))
    if rc != 0:
        raise DmtError(f"dmt_texture_mip_chain failed ({rc})")
    chain, off = [], 0
    for a, b in sizes:
        chain.append(out[4 * off:4 * (off + a * b)].reshape(a, b, 4))
        off += a * b
    return n.value, chain


def texture_footprint(camera44):
    """Host only: the camera's footprint for the first-hit texture filter -- dict(cfr = camera-from-render 3x4, min_dx,
    min_dy, spp_scale)."""
    lib = load_library()
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    out = np.zeros(19, np.float32)
    rc = lib.dmt_texture_footprint(_p(cam), _p(out))
    if rc != 0:
        raise DmtError(f"dmt_texture_footprint failed ({rc})")
    return dict(cfr=out[:12].reshape(3, 4).copy(), min_dx=out[12:15].copy(), min_dy=out[15:18].copy(), spp_scale=np.float32(out[18]))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(shape) if shape is not None else a


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def light_tree_pmfs(lights32, p, n):
    """Host-only: selection probability of every packed light at point p with normal n; returns (pmfs, node_count, depth)."""
    lib = load_library()
    L = np.ascontiguousarray(lights32, np.uint8).reshape(-1, 32)
    out = np.zeros(L.shape[0], np.float32)
    nc, d = C.c_int(), C.c_int()
    rc = lib.dmt_light_tree_pmfs(_p(L), C.c_uint32(L.shape[0]), _p(_f32(p, (3,))), _p(_f32(n, (3,))), _p(out), C.byref(nc), C.byref(d))
    if rc != 0:
        raise DmtError(f"dmt_light_tree_pmfs failed ({rc})")
    return out, nc.value, d.value


def light_tree_ref_select(lights32, p, n, u, start_pmf=1.0):
    """Host-only: DMT_LIGHTS_TREE_REFERENCE's cut + selection (csrc/light_tree_ref.hpp ltr_select) at shading points p [k,3]
    with normals n [k,3] and one random number each -> (indices [k,4] (-1 = none), pmfs [k,4], counts [k], node_count, depth)."""
    lib = load_library()
    L = np.ascontiguousarray(lights32, np.uint8).reshape(-1, 32)
    p, n = _f32(p).reshape(-1, 3), _f32(n).reshape(-1, 3)
    u = _f32(u).reshape(-1)
    k = p.shape[0]
    idx, pmf, cnt = np.zeros((k, 4), np.int32), np.zeros((k, 4), np.float32), np.zeros(k, np.int32)
    nc, d = C.c_int(), C.c_int()
    rc = lib.dmt_light_tree_ref_select(_p(L), C.c_uint32(L.shape[0]), C.c_int(k), _p(p), _p(n), _p(u), C.c_float(start_pmf), _p(idx), _p(pmf),
                                       _p(cnt), C.byref(nc), C.byref(d))
    if rc != 0:
        raise DmtError(f"dmt_light_tree_ref_select failed ({rc})")
    return idx, pmf, cnt, nc.value, d.value


# one node of the trees dmt_light_tree_nodes returns (csrc/light_tree.hpp LightTreeNode, csrc/light_tree_ref.hpp LightTreeRefNode)
LIGHT_TREE_NODE = np.dtype([("lo", "<f4", 3), ("phi", "<f4"), ("hi", "<f4", 3), ("ref", "<u4")])
LIGHT_TREE_REF_NODE = np.dtype([("lo", "<f4", 3), ("phi", "<f4"), ("hi", "<f4", 3), ("varPhi", "<f4"), ("w", "<f4", 3), ("cosTheta_o", "<f4"),
                                ("cosTheta_e", "<f4"), ("numEmitters", "<u4"), ("left", "<u4"), ("light", "<u4")])
LIGHT_TREE_LEAF = 0x80000000


def light_tree_nodes(lights32, mode, cap=None):
    """Host-only (dmt_light_tree_nodes): the node array a context uploads for the packed lights under light sampling `mode`
    (1: LIGHT_TREE_NODE records, 2: LIGHT_TREE_REF_NODE records), root first -> (nodes, depth).  cap: room offered, in nodes
    (default: what the tree needs); too little is refused."""
    lib = load_library()
    L = np.ascontiguousarray(lights32, np.uint8).reshape(-1, 32)
    nc, d = C.c_int(), C.c_int()
    if cap is None:
        lib.dmt_light_tree_nodes(_p(L), C.c_uint32(L.shape[0]), int(mode), None, C.c_uint32(0), C.byref(nc), C.byref(d))
        cap = nc.value
    out = np.zeros(max(int(cap), 1), LIGHT_TREE_NODE if int(mode) == 1 else LIGHT_TREE_REF_NODE)
    rc = lib.dmt_light_tree_nodes(_p(L), C.c_uint32(L.shape[0]), int(mode), _p(out), C.c_uint32(int(cap)), C.byref(nc), C.byref(d))
    if rc != 0:
        raise DmtError(f"dmt_light_tree_nodes failed ({rc}): {nc.value} nodes, room for {int(cap)}")
    return out[:nc.value], d.value


# one node of the tree dmt_emitter_tree_nodes returns (csrc/emitter_tree.hpp EmitterNode, 48 bytes)
EMITTER_TREE_NODE = np.dtype([("lo", "<f4", 3), ("phi", "<f4"), ("hi", "<f4", 3), ("ref", "<u4"), ("axis", "<f4", 3), ("cosO", "<f4")])
EMITTER_TREE_LEAF = 0x80000000
EMITTERS_UNIFORM, EMITTERS_TREE = 0, 1


def _emitter_scene(lights32, xs, ys, zs, area_tri, area_le):
    """The arguments the host-only emitter-tree calls share: packed lights [k,32] (may be empty), the soup as
    dmt_upload_triangles takes it (4 floats per triangle and axis), the emissive list (triangle indices, rgb radiance)."""
    L = np.ascontiguousarray(lights32, np.uint8).reshape(-1, 32)
    xs, ys, zs = _f32(xs).reshape(-1), _f32(ys).reshape(-1), _f32(zs).reshape(-1)
    tri = np.ascontiguousarray(area_tri, np.uint32).reshape(-1)
    le = _f32(area_le).reshape(-1, 3)
    assert xs.size % 4 == 0 and ys.size == xs.size and zs.size == xs.size and le.shape[0] == tri.size
    keep = (L, xs, ys, zs, tri, le)
    args = (_p(L) if L.size else None, C.c_uint32(L.shape[0]), _p(xs), _p(ys), _p(zs), C.c_uint64(xs.size // 4), _p(tri) if tri.size else None,
            _p(le) if tri.size else None, C.c_uint32(tri.size))
    return keep, args, L.shape[0] + tri.size


def emitter_tree_nodes(lights32, xs, ys, zs, area_tri, area_le, cap=None):
    """Host-only (dmt_emitter_tree_nodes): the emitter tree a context uploads for this scene -> (nodes [EMITTER_TREE_NODE],
    trails [emitters] uint64, lengths [emitters] int32, depth).  cap: room offered, in nodes; too little is refused."""
    lib = load_library()
    keep, args, count = _emitter_scene(lights32, xs, ys, zs, area_tri, area_le)
    nc, d = C.c_int(), C.c_int()
    if cap is None:
        rc = lib.dmt_emitter_tree_nodes(*args, None, C.c_uint32(0), None, None, C.byref(nc), C.byref(d))
        if rc != 0:
            raise DmtError(f"dmt_emitter_tree_nodes failed ({rc})")
        cap = nc.value
    out = np.zeros(max(int(cap), 1), EMITTER_TREE_NODE)
    trails, lengths = np.zeros(max(count, 1), np.uint64), np.zeros(max(count, 1), np.int32)
    rc = lib.dmt_emitter_tree_nodes(*args, _p(out), C.c_uint32(int(cap)), _p(trails), _p(lengths), C.byref(nc), C.byref(d))
    if rc != 0:
        raise DmtError(f"dmt_emitter_tree_nodes failed ({rc}): {nc.value} nodes, room for {int(cap)}")
    return out[:nc.value], trails[:count], lengths[:count], d.value


def emitter_tree_select(lights32, xs, ys, zs, area_tri, area_le, p, n, u, start_pmf=1.0):
    """Host-only (dmt_emitter_tree_select): et_select at cases (p [k,3], n [k,3], u [k]) -> (index [k] (-1 = none), pmf [k],
    pmf_by_trail [k]), both probabilities times start_pmf."""
    lib = load_library()
    keep, args, _ = _emitter_scene(lights32, xs, ys, zs, area_tri, area_le)
    p, n, u = _f32(p).reshape(-1, 3), _f32(n).reshape(-1, 3), _f32(u).reshape(-1)
    k = p.shape[0]
    assert n.shape[0] == k and u.shape[0] == k
    idx, pmf, trail = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float32)
    rc = lib.dmt_emitter_tree_select(*args, C.c_int(k), _p(p), _p(n), _p(u), C.c_float(start_pmf), _p(idx), _p(pmf), _p(trail))
    if rc != 0:
        raise DmtError(f"dmt_emitter_tree_select failed ({rc})")
    return idx, pmf, trail


def emitter_tree_pmfs(lights32, xs, ys, zs, area_tri, area_le, p, n):
    """Host-only (dmt_emitter_tree_pmfs): et_pmf of every emitter at point p with normal n."""
    lib = load_library()
    keep, args, count = _emitter_scene(lights32, xs, ys, zs, area_tri, area_le)
    out = np.zeros(max(count, 1), np.float32)
    rc = lib.dmt_emitter_tree_pmfs(*args, _p(_f32(p, (3,))), _p(_f32(n, (3,))), _p(out))
    if rc != 0:
        raise DmtError(f"dmt_emitter_tree_pmfs failed ({rc})")
    return out[:count]


def bvh_validate(xs, ys, zs):
    """Host-only BVH build + invariant check; returns dict(node_count, depth, max_leaf, ok)."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    n = xs.size // 4
    nc, d, ml = C.c_int(), C.c_int(), C.c_int()
    rc = lib.dmt_bvh_validate(_p(xs), _p(ys), _p(zs), C.c_size_t(n), C.byref(nc), C.byref(d), C.byref(ml))
    return {"ok": rc == 0, "node_count": nc.value, "depth": d.value, "max_leaf": ml.value}


class AccelBuildRecord(C.Structure):
    """dmt_accel_build_record (include/dmt_hip.h)"""
    _fields_ = [("builder", C.c_int32), ("depth", C.c_int32), ("triangles", C.c_uint32), ("nodes", C.c_uint32),
                ("pairs", C.c_uint32), ("reserved", C.c_uint32), ("build_ms", C.c_double), ("temp_bytes", C.c_uint64)]


def lbvh_reference(xs, ys, zs, max_depth=48):
    """Host-only: the serial restatement of the device BVH builder.  Returns dict(abandoned, nodes = [node_count, 64] uint8,
    pairs = [pair_count, 2] uint32 original indices, depth); abandoned (the depth guard fired) comes with empty arrays."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    n = xs.size // 4
    cap = max(n, 1)
    nodes, pairs = np.zeros((cap, 64), np.uint8), np.zeros((cap, 2), np.uint32)
    nn, npairs, d, ab = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
    rc = lib.dmt_lbvh_reference(_p(xs), _p(ys), _p(zs), C.c_size_t(n), C.c_int(max_depth), _p(nodes), C.c_size_t(cap), _p(pairs),
                                C.c_size_t(cap), C.byref(nn), C.byref(npairs), C.byref(d), C.byref(ab))
    if rc != 0:
        raise DmtError(f"dmt_lbvh_reference failed ({rc})")
    return {"abandoned": bool(ab.value), "nodes": nodes[:nn.value].copy(), "pairs": pairs[:npairs.value].copy(), "depth": d.value}


class AccelUpdateRecord(C.Structure):
    """dmt_accel_update_record (include/dmt_hip.h)"""
    _fields_ = [("action", C.c_int32), ("updates_since_build", C.c_uint32), ("update_ms", C.c_double), ("sah_cost", C.c_double),
                ("sah_cost_at_build", C.c_double), ("temp_bytes", C.c_uint64)]


def bvh_refit_reference(nodes, pairs, xs, ys, zs):
    """Host-only: the serial restatement of the device refit.  A tree (nodes [k, 64] uint8, pairs [m, 2] uint32 original
    indices) and the NEW soup -> the refitted nodes [k, 64] uint8.  Raises DmtError on an inconsistent tree (DMT_ERR_STATE)."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 64)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    out = np.zeros_like(nodes)
    rc = lib.dmt_bvh_refit_reference(_p(nodes), C.c_size_t(nodes.shape[0]), _p(pairs), C.c_size_t(pairs.shape[0]), _p(xs), _p(ys), _p(zs),
                                     C.c_size_t(xs.size // 4), _p(out))
    if rc != 0:
        raise DmtError(f"dmt_bvh_refit_reference failed ({rc})")
    return out


def bvh_check(nodes, pairs, xs, ys, zs):
    """Host-only: dmt_bvh_validate's walk on any tree (nodes [k, 64] uint8, pairs [m, 2] uint32) over a soup; returns
    dict(ok, depth, max_leaf, sah_cost, node_count, pair_count)."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 64)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    d, ml, sah = C.c_int(), C.c_int(), C.c_double()
    rc = lib.dmt_bvh_check(_p(nodes), C.c_size_t(nodes.shape[0]), _p(pairs), C.c_size_t(pairs.shape[0]), _p(xs), _p(ys), _p(zs),
                           C.c_size_t(xs.size // 4), C.byref(d), C.byref(ml), C.byref(sah))
    return {"ok": rc == 0, "depth": d.value, "max_leaf": ml.value, "sah_cost": sah.value, "node_count": nodes.shape[0],
            "pair_count": pairs.shape[0]}


def brute_cull_plan(xs, ys, zs, mat_id, enable=True):
    """Host-only: the culled clusters of the brute-force pass, a list of (first, count, (cx, cy, cz), radius)."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    mat = np.ascontiguousarray(mat_id, np.uint32)
    n = xs.size // 4
    nc, fc, sph = C.c_uint32(), np.zeros(8, np.uint32), np.zeros(16, np.float32)
    rc = lib.dmt_brute_cull_plan(_p(xs), _p(ys), _p(zs), _p(mat), C.c_size_t(n), int(bool(enable)), C.byref(nc), _p(fc), _p(sph))
    if rc != 0:
        raise DmtError(f"dmt_brute_cull_plan failed ({rc})")
    return [(int(fc[2 * k]), int(fc[2 * k + 1]), tuple(float(x) for x in sph[4 * k:4 * k + 3]), float(sph[4 * k + 3]))
            for k in range(nc.value)]


def brute_cull_box_plan(xs, ys, zs, mat_id, enable=True):
    """Host-only: the box clusters of the brute-force pass, a list of (first, count, (lox, loy, loz), (hix, hiy, hiz))."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    mat = np.ascontiguousarray(mat_id, np.uint32)
    n = xs.size // 4
    nc, fc, box = C.c_uint32(), np.zeros(24, np.uint32), np.zeros(72, np.float32)
    rc = lib.dmt_brute_cull_box_plan(_p(xs), _p(ys), _p(zs), _p(mat), C.c_size_t(n), int(bool(enable)), C.byref(nc), _p(fc), _p(box))
    if rc != 0:
        raise DmtError(f"dmt_brute_cull_box_plan failed ({rc})")
    return [(int(fc[2 * k]), int(fc[2 * k + 1]), tuple(float(x) for x in box[6 * k:6 * k + 3]),
             tuple(float(x) for x in box[6 * k + 3:6 * k + 6])) for k in range(nc.value)]


def brute_cull_box_records(xs, ys, zs, mat_id, enable=True):
    """Host-only: the box clusters as planned and as the device reads them, a list of (box [6] = lo xyz, hi xyz as
    brute_cull_box_plan gives them, record [6] = centre xyz, half-width xyz), float32 arrays."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    mat = np.ascontiguousarray(mat_id, np.uint32)
    n = xs.size // 4
    nc, box, rec = C.c_uint32(), np.zeros(72, np.float32), np.zeros(72, np.float32)
    rc = lib.dmt_brute_cull_box_records(_p(xs), _p(ys), _p(zs), _p(mat), C.c_size_t(n), int(bool(enable)), C.byref(nc), _p(box), _p(rec))
    if rc != 0:
        raise DmtError(f"dmt_brute_cull_box_records failed ({rc})")
    return [(box[6 * k:6 * k + 6].copy(), rec[6 * k:6 * k + 6].copy()) for k in range(nc.value)]


CULL_RECORD_DTYPE = np.dtype([("b", "<f4", 6), ("box", "<u4"), ("count", "<u4"), ("first", "<u4"), ("slot", "<u4"),
                              ("magic", "<u4"), ("pad", "<u4", 5)])


def cull_records(xs, ys, zs, mat_id, level=2):
    """Host-only: the cluster table the brute-force pass uploads for a soup at DMT_BRUTE_CULL = level, as
    (records, record_bytes, record_align): a CULL_RECORD_DTYPE array of the clusters, sphere clusters first."""
    lib = load_library()
    xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
    mat = np.ascontiguousarray(mat_id, np.uint32)
    n = xs.size // 4
    nc, nb, na = C.c_uint32(), C.c_uint32(), C.c_uint32()
    raw = np.zeros(12 * 64, np.uint8)
    rc = lib.dmt_cull_records(_p(xs), _p(ys), _p(zs), _p(mat), C.c_size_t(n), int(level), C.byref(nc), C.byref(nb), C.byref(na), _p(raw))
    if rc != 0:
        raise DmtError(f"dmt_cull_records failed ({rc})")
    if nb.value != CULL_RECORD_DTYPE.itemsize:
        raise DmtError(f"dmt_cull_records: record of {nb.value} bytes, expected {CULL_RECORD_DTYPE.itemsize}")
    return raw[:nc.value * nb.value].view(CULL_RECORD_DTYPE).copy(), nb.value, na.value


def cull_box_test(record, origins, dirs, tmax):
    """Host-only: the device's box bound test (brute_clusters) for rays [n, 3] / [n, 3] / tmax [n] against one box record
    (centre xyz, half-width xyz); returns a bool array, True = the cluster's triangles would be tested for the ray."""
    lib = load_library()
    rec = np.ascontiguousarray(record, np.float32).reshape(6)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tmax, np.float32).reshape(-1)
    if not (o.shape[0] == d.shape[0] == t.shape[0]):
        raise ValueError("cull_box_test: origins, dirs and tmax differ in length")
    out = np.zeros(o.shape[0], np.uint8)
    rc = lib.dmt_cull_box_test(_p(rec), _p(o), _p(d), _p(t), C.c_size_t(o.shape[0]), _p(out))
    if rc != 0:
        raise DmtError(f"dmt_cull_box_test failed ({rc})")
    return out.astype(bool)


def envmap_tables(rgb):
    """Host-only: the PiecewiseConstant2D tables dmt_upload_envmap builds for an env map [h, w, 3]."""
    lib = load_library()
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    func, cdf = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    row_int, m_func, m_cdf = np.zeros(h, np.float32), np.zeros(h, np.float32), np.zeros(h, np.float32)
    m_int = C.c_float()
    rc = lib.dmt_envmap_tables(_p(rgb), int(w), int(h), _p(func), _p(cdf), _p(row_int), _p(m_func), _p(m_cdf),
                               C.byref(m_int))
    if rc != 0:
        raise DmtError(f"dmt_envmap_tables failed ({rc})")
    return dict(func=func, cdf=cdf, row_int=row_int, m_func=m_func, m_cdf=m_cdf, m_int=np.float32(m_int.value))


class Renderer:
    """One dmt_ctx: one device, one stream.  Mirrors the reference's launch boundary
    (upload helpers + pathTraceMegakernel launches + film download)."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.dmt_ctx_create(int(device), C.byref(self._ctx))
        if rc != 0:
            msg = self._lib.dmt_last_error(None)
            raise DmtError(f"dmt_ctx_create failed ({rc}): {msg.decode() if msg else ''}")
        self.width = self.height = 0
        self._aov_shape = None      # (height, width) of the AOVs on the device
        self.denoise_ms = 0.0       # HIP-event time of the last denoise()
        self.display_ms = 0.0       # HIP-event time of the last display()

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dmt_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.dmt_last_error(self._ctx)
            raise DmtError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def last_error(self):
        """dmt_last_error: the context's latest message -- a refused call's reason, or a note such as the light tree's
        fall-back to the uniform pick."""
        msg = self._lib.dmt_last_error(self._ctx)
        return msg.decode() if msg else ""

    # ---- uploads ---------------------------------------------------------------------------
    def upload_triangles(self, xs, ys, zs, mat_id):
        xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
        mat_id = np.ascontiguousarray(mat_id, np.uint32)
        n = mat_id.shape[0]
        assert xs.size == 4 * n and ys.size == 4 * n and zs.size == 4 * n
        self._check(self._lib.dmt_upload_triangles(self._ctx, _p(xs), _p(ys), _p(zs), _p(mat_id), C.c_size_t(n)),
                    "dmt_upload_triangles")

    def update_vertices(self, xs, ys, zs):
        """Same triangles, new positions (dmt_update_vertices): layout as upload_triangles; materials, emissive triangles,
        textures, lights, camera and film are kept; the tree follows set_accel_update."""
        xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
        n = xs.size // 4
        assert xs.size == 4 * n and ys.size == 4 * n and zs.size == 4 * n
        self._check(self._lib.dmt_update_vertices(self._ctx, _p(xs), _p(ys), _p(zs), C.c_size_t(n)), "dmt_update_vertices")

    def update_vertices_device(self, ptr, count):
        """dmt_update_vertices_device: `ptr` = device address of count x 9 floats (p0, p1, p2 of every triangle) on this
        context's device, e.g. a contiguous float32 torch tensor's data_ptr(); read on the context's stream."""
        self._check(self._lib.dmt_update_vertices_device(self._ctx, C.c_void_p(int(ptr)), C.c_size_t(int(count))),
                    "dmt_update_vertices_device")

    def set_accel_update(self, mode, max_cost_ratio=0.0):
        """What an update does to the tree: BVH_UPDATE_REBUILD (0, default), BVH_UPDATE_REFIT (1) or BVH_UPDATE_AUTO (2: refit,
        then rebuild when the cost passes max_cost_ratio x the cost the builder left)."""
        self._check(self._lib.dmt_set_accel_update(self._ctx, int(mode), C.c_double(max_cost_ratio)), "dmt_set_accel_update")

    def accel_update_info(self):
        """The record of the last update: dict(action, updates_since_build, update_ms, sah_cost, sah_cost_at_build, temp_bytes)."""
        rec = AccelUpdateRecord()
        self._check(self._lib.dmt_accel_update_info(self._ctx, C.byref(rec)), "dmt_accel_update_info")
        return {name: getattr(rec, name) for name, _ in AccelUpdateRecord._fields_}

    def upload_bsdfs(self, bsdfs):
        b = np.ascontiguousarray(bsdfs, np.uint8).reshape(-1, 32)
        self._check(self._lib.dmt_upload_bsdfs(self._ctx, _p(b), C.c_uint32(b.shape[0])), "dmt_upload_bsdfs")

    def upload_lights(self, lights, inf_lights):
        l = np.ascontiguousarray(lights, np.uint8).reshape(-1, 32)
        i = np.ascontiguousarray(inf_lights, np.uint8).reshape(-1, 32)
        self._check(self._lib.dmt_upload_lights(self._ctx, _p(l) if l.shape[0] else None, C.c_uint32(l.shape[0]),
                                                _p(i) if i.shape[0] else None, C.c_uint32(i.shape[0])),
                    "dmt_upload_lights")

    def uniform_lights_info(self):
        """True when launches pass the scalar path's switch for one-record light lists (dmt_uniform_lights_info)."""
        v = C.c_int()
        self._check(self._lib.dmt_uniform_lights_info(self._ctx, C.byref(v)), "dmt_uniform_lights_info")
        return bool(v.value)

    def set_camera(self, camera44):
        cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
        self._check(self._lib.dmt_set_camera(self._ctx, _p(cam)), "dmt_set_camera")
        self.width = int(cam[24:28].view(np.int32)[0])
        self.height = int(cam[28:32].view(np.int32)[0])

    def set_lens(self, lens_radius, focus_distance=1.0):
        """Thin lens (dmt_set_lens): radius >= 0 (0 = pinhole, the default) and focus distance > 0 along the viewing
        direction, in scene units.  The lens survives set_camera and scene uploads."""
        self._check(self._lib.dmt_set_lens(self._ctx, C.c_float(lens_radius), C.c_float(focus_distance)), "dmt_set_lens")

    def set_medium(self, sigma_t, albedo=(1.0, 1.0, 1.0), g=0.0, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
        """Participating medium (dmt_set_medium): homogeneous fog of grey extinction sigma_t >= 0 per scene unit, albedo in
        [0, 1] per channel and Henyey-Greenstein asymmetry |g| < 1 inside the box [box_min, box_max].  Active exactly when
        sigma_t > 0; survives scene uploads and set_camera."""
        self._check(self._lib.dmt_set_medium(self._ctx, C.c_float(sigma_t), _p(_f32(albedo, (3,))), C.c_float(g), _p(_f32(box_min, (3,))),
                                             _p(_f32(box_max, (3,)))), "dmt_set_medium")

    def clear_medium(self):
        """dmt_clear_medium: every film is then byte for byte what it was without a medium."""
        self._check(self._lib.dmt_clear_medium(self._ctx), "dmt_clear_medium")

    def medium_info(self):
        """dmt_medium_info -> dict(active, sigma_t, albedo, g, box_min, box_max): the record as it was set."""
        act, st, g = C.c_int(), C.c_float(), C.c_float()
        a, lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self._lib.dmt_medium_info(self._ctx, C.byref(act), C.byref(st), _p(a), C.byref(g), _p(lo), _p(hi)), "dmt_medium_info")
        return dict(active=bool(act.value), sigma_t=st.value, albedo=a, g=g.value, box_min=lo, box_max=hi)

    def test_medium(self, sigma_t, g, box_min, box_max, o, d, t_hit, h, depth, cosine, u):
        """dmt_test_medium: the device versions of the medium's arithmetic over n cases -> dict(seg [n, 2], hit [n] bool,
        u [n], flight [n], transmittance [n], eval [n], wi [n, 3], pdf [n]); wi is sampled around wo = -d."""
        o, d, u = _f32(o).reshape(-1, 3), _f32(d).reshape(-1, 3), _f32(u).reshape(-1, 2)
        t, cosine, h, depth = _f32(t_hit).reshape(-1), _f32(cosine).reshape(-1), _u32(h), _u32(depth)
        n = o.shape[0]
        assert all(a.shape[0] == n for a in (d, u, t, cosine, h, depth))
        seg, hit, val = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        ev, wi, pdf = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        medium8 = np.concatenate([[sigma_t, g], _f32(box_min, (3,)), _f32(box_max, (3,))]).astype(np.float32)
        self._check(self._lib.dmt_test_medium(self._ctx, _p(medium8), int(n),
                                              _p(o), _p(d), _p(t), _p(h), _p(depth), _p(cosine), _p(u), _p(seg), _p(hit), _p(val), _p(ev),
                                              _p(wi), _p(pdf)), "dmt_test_medium")
        return dict(seg=seg, hit=hit.astype(bool), u=val[:, 0].copy(), flight=val[:, 1].copy(), transmittance=val[:, 2].copy(), eval=ev,
                    wi=wi, pdf=pdf)

    def set_medium_grid(self, density):
        """The medium's density grid (dmt_set_medium_grid), shape (nz, ny, nx), every value finite and >= 0:
        the extinction in a voxel is sigma_t * density, the grid fills the medium's box.  A numpy array (anything
        np.asarray takes) goes through the host call; a contiguous float32 torch tensor on the context's device goes through
        dmt_set_medium_grid_device, after the tensor's stream has been synchronised.  Kept by set_medium, scene uploads and
        set_camera; dropped by clear_medium and clear_medium_grid."""
        if hasattr(density, "data_ptr"):  # a torch tensor
            import torch
            if density.dim() != 3 or density.dtype != torch.float32 or not density.is_contiguous() or not density.is_cuda:
                raise DmtError("set_medium_grid: a tensor must be contiguous float32 of shape (nz, ny, nx) on the context's device")
            nz, ny, nx = (int(v) for v in density.shape)
            torch.cuda.current_stream(density.device).synchronize()
            self._check(self._lib.dmt_set_medium_grid_device(self._ctx, C.c_void_p(int(density.data_ptr())), nx, ny, nz), "dmt_set_medium_grid_device")
            return
        density = _f32(density)
        if density.ndim != 3:
            raise DmtError("set_medium_grid: the density grid has shape (nz, ny, nx)")
        nz, ny, nx = density.shape
        self._check(self._lib.dmt_set_medium_grid(self._ctx, _p(density), int(nx), int(ny), int(nz)), "dmt_set_medium_grid")

    def clear_medium_grid(self):
        """dmt_clear_medium_grid: the medium is homogeneous again."""
        self._check(self._lib.dmt_clear_medium_grid(self._ctx), "dmt_clear_medium_grid")

    def medium_grid_info(self):
        """dmt_medium_grid_info -> dict(present, dims (nx, ny, nz), support_min, support_max (inclusive voxel indices per axis;
        min > max without a density > 0), positive (voxels > 0), max_density, active (the grid rows would run))."""
        present, active, positive, top = C.c_int(), C.c_int(), C.c_uint64(), C.c_float()
        dims, lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        self._check(self._lib.dmt_medium_grid_info(self._ctx, C.byref(present), _p(dims), _p(lo), _p(hi), C.byref(positive), C.byref(top),
                                                   C.byref(active)), "dmt_medium_grid_info")
        return dict(present=bool(present.value), dims=tuple(int(v) for v in dims), support_min=tuple(int(v) for v in lo),
                    support_max=tuple(int(v) for v in hi), positive=int(positive.value), max_density=top.value, active=bool(active.value))

    def test_medium_grid(self, box_min, box_max, sigma_t, density, o, d, t_end, tau_target):
        """dmt_test_medium_grid: medium_grid_march by the device, for a grid given here -> as the module's medium_grid_march."""
        density, o, d, t, target, n, out = _grid_call(density, o, d, t_end, tau_target)
        nz, ny, nx = density.shape
        medium7 = np.concatenate([[sigma_t], _f32(box_min, (3,)), _f32(box_max, (3,))]).astype(np.float32)
        self._check(self._lib.dmt_test_medium_grid(self._ctx, _p(medium7), int(nx), int(ny), int(nz), _p(density), int(n), _p(o), _p(d), _p(t),
                                                   _p(target), _p(out["tau"]), _p(out["ts"]), _p(out["collided"]), _p(out["steps"])),
                    "dmt_test_medium_grid")
        out["collided"] = out["collided"].astype(bool)
        return out

    def set_medium_spectrum(self, extinction=(1.0, 1.0, 1.0), emission=(0.0, 0.0, 0.0)):
        """The medium's spectrum (dmt_set_medium_spectrum): an extinction colour (the channel extinctions are
        sigma_t * extinction; finite, >= 0, not all zero) and an emitted radiance (finite, >= 0) per channel.  Kept by
        set_medium, scene uploads and set_camera; dropped by clear_medium and clear_medium_spectrum."""
        self._check(self._lib.dmt_set_medium_spectrum(self._ctx, _p(_f32(extinction, (3,))), _p(_f32(emission, (3,)))), "dmt_set_medium_spectrum")

    def clear_medium_spectrum(self):
        """dmt_clear_medium_spectrum: the medium is grey and dark again."""
        self._check(self._lib.dmt_clear_medium_spectrum(self._ctx), "dmt_clear_medium_spectrum")

    def medium_spectrum_info(self):
        """dmt_medium_spectrum_info -> dict(present, extinction, emission, k (the channel extinctions from the medium's
        sigma_t), ref_channel, active (the spectrum rows would run))."""
        present, ref, active = C.c_int(), C.c_int(), C.c_int()
        e, le, k = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self._lib.dmt_medium_spectrum_info(self._ctx, C.byref(present), _p(e), _p(le), _p(k), C.byref(ref), C.byref(active)),
                    "dmt_medium_spectrum_info")
        return dict(present=bool(present.value), extinction=e, emission=le, k=k, ref_channel=int(ref.value), active=bool(active.value))

    def test_medium_spectrum(self, k, beta, h, depth, tau_seg):
        """dmt_test_medium_spectrum: medium_spectrum_event by the device -> as the module's medium_spectrum_event."""
        beta, h, depth, tau, n, out = _spectrum_call(beta, h, depth, tau_seg)
        self._check(self._lib.dmt_test_medium_spectrum(self._ctx, _p(_f32(k, (3,))), int(n), _p(beta), _p(h), _p(depth), _p(tau), _p(out["channel"]),
                                                       _p(out["collided"]), _p(out["tau_at"]), _p(out["weight"])), "dmt_test_medium_spectrum")
        out["collided"] = out["collided"].astype(bool)
        return out

    def lens_info(self):
        """(lens_radius, focus_distance) of the context."""
        r, d = C.c_float(), C.c_float()
        self._check(self._lib.dmt_lens_info(self._ctx, C.byref(r), C.byref(d)), "dmt_lens_info")
        return r.value, d.value

    def set_motion(self, xs1, ys1, zs1):
        """Key 1 (dmt_set_motion): a second position set for the uploaded triangles, layout as upload_triangles.  Samples
        then see the scene at their own time within the shutter.  Dropped by upload_triangles and update_vertices*."""
        xs1, ys1, zs1 = _f32(xs1), _f32(ys1), _f32(zs1)
        n = xs1.size // 4
        assert xs1.size == 4 * n and ys1.size == 4 * n and zs1.size == 4 * n
        self._check(self._lib.dmt_set_motion(self._ctx, _p(xs1), _p(ys1), _p(zs1), C.c_size_t(n)), "dmt_set_motion")

    def clear_motion(self):
        """Drops key 1 (dmt_clear_motion): every film is again what it was before set_motion."""
        self._check(self._lib.dmt_clear_motion(self._ctx), "dmt_clear_motion")

    def set_shutter(self, open=0.0, close=1.0):
        """The shutter interval (dmt_set_shutter), 0 <= open <= close <= 1; survives set_camera and scene uploads."""
        self._check(self._lib.dmt_set_shutter(self._ctx, C.c_float(open), C.c_float(close)), "dmt_set_shutter")

    def motion_info(self):
        """dmt_motion_info as a dict: keys (0, 1 or 2), open, close, tree_nodes, tree_pairs, tree_build_ms."""
        k, o, c = C.c_int(), C.c_float(), C.c_float()
        nn, npairs, ms = C.c_uint32(), C.c_uint32(), C.c_double()
        self._check(self._lib.dmt_motion_info(self._ctx, C.byref(k), C.byref(o), C.byref(c), C.byref(nn), C.byref(npairs), C.byref(ms)),
                    "dmt_motion_info")
        return {"keys": k.value, "open": o.value, "close": c.value, "tree_nodes": nn.value, "tree_pairs": npairs.value,
                "tree_build_ms": ms.value}

    def upload_vertex_normals(self, n9):
        """Smooth shading (dmt_upload_vertex_normals): [n, 9] the normals at vertices 0, 1, 2 of every uploaded triangle; a
        row of zeros keeps that triangle flat.  Dropped by upload_triangles, kept by update_vertices*."""
        n9 = _f32(n9).reshape(-1, 9)
        self._check(self._lib.dmt_upload_vertex_normals(self._ctx, _p(n9), C.c_size_t(n9.shape[0])), "dmt_upload_vertex_normals")

    def clear_vertex_normals(self):
        """Drops the vertex normals (dmt_clear_vertex_normals): every film is again what it was before the upload."""
        self._check(self._lib.dmt_clear_vertex_normals(self._ctx), "dmt_clear_vertex_normals")

    def vertex_normals_info(self):
        """dmt_vertex_normals_info as a dict: triangles (0 without normals), smooth_triangles."""
        t, sm = C.c_uint64(), C.c_uint64()
        self._check(self._lib.dmt_vertex_normals_info(self._ctx, C.byref(t), C.byref(sm)), "dmt_vertex_normals_info")
        return {"triangles": t.value, "smooth_triangles": sm.value}

    def upload_opacity(self, mat_opacity_tex, cutoff=0.5):
        """Alpha cutouts (dmt_upload_opacity): per BSDF the index of the uploaded texture whose A channel is its opacity,
        OPACITY_NONE = opaque.  A hit counts iff the A channel there is at least cutoff * 255.  After upload_textures;
        dropped by upload_triangles, upload_bsdfs and upload_textures, kept by update_vertices*."""
        m = np.ascontiguousarray(mat_opacity_tex, np.uint32).reshape(-1)
        self._check(self._lib.dmt_upload_opacity(self._ctx, _p(m), C.c_uint32(m.shape[0]), C.c_float(cutoff)), "dmt_upload_opacity")

    def clear_opacity(self):
        """Drops the opacity (dmt_clear_opacity): every film is again what it was before the upload."""
        self._check(self._lib.dmt_clear_opacity(self._ctx), "dmt_clear_opacity")

    def opacity_info(self):
        """dmt_opacity_info as a dict: cutout_triangles, cutout_materials, cutoff (zeros without opacity)."""
        t, m, c = C.c_uint64(), C.c_uint32(), C.c_float()
        self._check(self._lib.dmt_opacity_info(self._ctx, C.byref(t), C.byref(m), C.byref(c)), "dmt_opacity_info")
        return {"cutout_triangles": t.value, "cutout_materials": m.value, "cutoff": c.value}

    def test_opacity(self, tri, bu, bv):
        """dmt_test_opacity: (alpha8 [n], passes [n] bool) of triangle tri[i] at (bu, bv), as the cutout rows compute them."""
        tri, bu, bv = _i32(tri).reshape(-1), _f32(bu).reshape(-1), _f32(bv).reshape(-1)
        n = tri.shape[0]
        assert bu.shape[0] == n and bv.shape[0] == n
        a, ok = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self._check(self._lib.dmt_test_opacity(self._ctx, int(n), _p(tri), _p(bu), _p(bv), _p(a), _p(ok)), "dmt_test_opacity")
        return a, ok.astype(bool)

    def test_closest_hit_opacity(self, o, d, tmax):
        """dmt_test_closest_hit_opacity: ray i under the cutout rule and the current accel mode -> (tri [n], t [n], uv [n, 2],
        occluded [n] bool); occluded = some passing hit has t < tmax[i]."""
        o, d = _f32(o, (-1, 3)), _f32(d, (-1, 3))
        n = o.shape[0]
        tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        idx, t, uv, occ = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        self._check(self._lib.dmt_test_closest_hit_opacity(self._ctx, n, _p(o), _p(d), _p(tmax), _p(idx), _p(t), _p(uv), _p(occ)),
                    "dmt_test_closest_hit_opacity")
        return idx, t, uv, occ.astype(bool)

    def test_shading_normal(self, tri, bu, bv, rd, mapped=False):
        """The shading normal [n, 3] the vertex-normal rows compute for triangle tri[i] at (bu, bv) under a ray of direction
        rd[i] (dmt_test_shading_normal); mapped: with the material's normal map applied around it."""
        tri, bu, bv = _i32(tri).reshape(-1), _f32(bu).reshape(-1), _f32(bv).reshape(-1)
        rd = _f32(rd).reshape(-1, 3)
        n = tri.shape[0]
        assert bu.shape[0] == n and bv.shape[0] == n and rd.shape[0] == n
        ns = np.zeros((n, 3), np.float32)
        fn = self._lib.dmt_test_shading_normal_mapped if mapped else self._lib.dmt_test_shading_normal
        self._check(fn(self._ctx, int(n), _p(tri), _p(bu), _p(bv), _p(rd), _p(ns)), "dmt_test_shading_normal")
        return ns

    def set_pixel_filter(self, kind, radius, param=0.0):
        """Pixel reconstruction filter, importance-sampled per sample (dmt_set_pixel_filter).  kind: FILTER_BOX, FILTER_TENT,
        FILTER_GAUSSIAN (param = sigma) or FILTER_BLACKMAN_HARRIS, or its name ("box", "tent", "gaussian",
        "blackman-harris"); radius in pixels, in (0, 8].  Box with radius 0.5, the default, is inactive.  The filter
        survives set_camera and scene uploads."""
        if isinstance(kind, str):
            if kind not in PIXEL_FILTER_KINDS:
                raise DmtError(f"set_pixel_filter: unsupported kind '{kind}'")
            kind = PIXEL_FILTER_KINDS[kind]
        self._check(self._lib.dmt_set_pixel_filter(self._ctx, int(kind), C.c_float(radius), C.c_float(param)), "dmt_set_pixel_filter")

    def pixel_filter_info(self):
        """The context's pixel filter as a dict: kind, radius, param, active."""
        k, a, r, p = C.c_int(), C.c_int(), C.c_float(), C.c_float()
        self._check(self._lib.dmt_pixel_filter_info(self._ctx, C.byref(k), C.byref(r), C.byref(p), C.byref(a)), "dmt_pixel_filter_info")
        return {"kind": k.value, "radius": r.value, "param": p.value, "active": bool(a.value)}

    def set_projection(self, kind, param=0.0):
        """Camera projection (dmt_set_projection).  kind: PROJECTION_PERSPECTIVE (the default), PROJECTION_ORTHOGRAPHIC
        (param = the view height in scene units), PROJECTION_EQUIRECT or PROJECTION_FISHEYE (param = the field of view across
        the film's diagonal, in degrees), or its name ("perspective", "orthographic", "equirect", "fisheye").  The projection
        survives set_camera and scene uploads; it is refused while a lens is set."""
        self._check(self._lib.dmt_set_projection(self._ctx, _projection_kind(kind, "set_projection"), C.c_float(param)), "dmt_set_projection")

    def projection_info(self):
        """The context's projection as a dict: kind, param."""
        k, p = C.c_int(), C.c_float()
        self._check(self._lib.dmt_projection_info(self._ctx, C.byref(k), C.byref(p)), "dmt_projection_info")
        return {"kind": k.value, "param": p.value}

    def focus_distance_at(self, fx, fy):
        """Autofocus (dmt_focus_distance_at): the depth along the viewing direction of what the pinhole ray through the
        continuous film coordinates (fx, fy) hits; DmtError when it leaves the scene."""
        d = C.c_float()
        self._check(self._lib.dmt_focus_distance_at(self._ctx, C.c_float(fx), C.c_float(fy), C.byref(d)), "dmt_focus_distance_at")
        return d.value

    @staticmethod
    def scene_pixel_filter(scene):
        """(kind, radius, sigma) of the pixel filter a scene records, for set_pixel_filter; None for a scene without one;
        DmtError for a kind the library does not offer."""
        pf = getattr(scene, "pixel_filter", None)
        if pf is None:
            return None
        if pf.get("kind") is None:
            raise DmtError(f"the scene's pixel filter '{pf.get('type')}' is an unsupported kind (signed filters need a per-sample weight)")
        return int(pf["kind"]), float(pf["radius"]), float(pf["sigma"])

    def upload_scene(self, scene, vertex_normals=False, opacity=True, pixel_filter=False):
        """`scene`: any object with xs, ys, zs, mat_id, bsdfs, lights, inf_lights, camera arrays; a scene with a `lens`
        (lens_radius, focus_distance), as the loaders report one, sets the context's lens too, one with a `projection`
        (kind, param) the context's projection, and one with a `medium`
        (the keyword arguments of set_medium, and the "extinction" and "emission" of set_medium_spectrum) the context's medium.  vertex_normals: also
        upload the scene's `tri_normals` (smooth shading); off by default, the files' normals are not used unasked.
        opacity: upload the scene's `mat_opacity` / `opacity_cutoff` (alpha cutouts) when it carries them.
        pixel_filter: also set the pixel filter the scene records (`pixel_filter`: PBRT PixelFilter, JSON film.filter); off by
        default, so that every load renders as before.  DmtError, before anything is uploaded, for a recorded kind the library
        does not offer (mitchell, sinc)."""
        wanted_filter = self.scene_pixel_filter(scene) if pixel_filter else None
        if wanted_filter is not None:
            self.set_pixel_filter(*wanted_filter)
        self.upload_triangles(scene.xs, scene.ys, scene.zs, scene.mat_id)
        if vertex_normals:
            tn = getattr(scene, "tri_normals", None)
            if tn is None or len(tn) != len(scene.mat_id):
                raise DmtError("upload_scene(vertex_normals=True): the scene carries no tri_normals")
            self.upload_vertex_normals(tn)
        self.upload_bsdfs(scene.bsdfs)
        self.upload_lights(scene.lights, scene.inf_lights)
        self.set_camera(scene.camera)
        # lens and projection exclude each other: a scene that carries both records has the one it leaves at its default set
        # first, so that a context still holding the last scene's projection takes this scene's lens (and the other way round)
        lens, proj = getattr(scene, "lens", None), getattr(scene, "projection", None)
        lens_first = not (lens is not None and float(lens[0]) > 0.0)
        for which in (("lens", "projection") if lens_first else ("projection", "lens")):
            if which == "lens" and lens is not None:
                self.set_lens(float(lens[0]), float(lens[1]))
            if which == "projection" and proj is not None:
                self.set_projection(proj[0], float(proj[1]))
        if getattr(scene, "medium", None) is not None:  # a scene file's "medium"; a scene without one leaves the context's
            m = dict(scene.medium)
            e, le = m.pop("extinction", (1.0, 1.0, 1.0)), m.pop("emission", (0.0, 0.0, 0.0))  # its "extinction" and "emission"
            self.set_medium(**m)
            if tuple(float(v) for v in e) == (1.0, 1.0, 1.0) and not any(float(v) for v in le):
                self.clear_medium_spectrum()  # the file's medium is grey and dark
            else:
                self.set_medium_spectrum(e, le)
        if getattr(scene, "medium_grid", None) is not None:  # its "grid"
            self.set_medium_grid(scene.medium_grid)
        if getattr(scene, "area_tri", None) is not None and len(scene.area_tri):
            self.upload_area_lights(scene.area_tri, scene.area_le)
        if getattr(scene, "env_rgb", None) is not None:
            self.upload_envmap(scene.env_rgb, scene.env_quat, scene.env_scale)
        else:
            self.clear_envmap()
        if getattr(scene, "tex_desc", None) is not None and len(scene.tex_desc):
            self.upload_textures(scene.tex_rgba, scene.tex_desc, scene.mat_tex, scene.tri_uv)
        else:
            self.upload_textures(None, None, None, None)
        mo = getattr(scene, "mat_opacity", None)
        if opacity and mo is not None and len(mo):
            self.upload_opacity(mo, float(getattr(scene, "opacity_cutoff", 0.5)))

    def upload_textures(self, tex_rgba, tex_desc, mat_tex, tri_uv):
        """SURVEY 8f-1 image textures (layout: include/dmt_hip.h dmt_upload_textures); all None clears."""
        if tex_desc is None or len(tex_desc) == 0:
            self._check(self._lib.dmt_upload_textures(self._ctx, None, C.c_uint64(0), None, C.c_uint32(0), None, C.c_uint32(0), None,
                                                      C.c_uint64(0)), "dmt_upload_textures")
            return
        rgba = np.ascontiguousarray(tex_rgba, np.uint8).reshape(-1, 4)
        desc = np.ascontiguousarray(tex_desc, np.int32).reshape(-1, 3)
        mt = np.ascontiguousarray(mat_tex, np.uint32).reshape(-1, 4)
        uv = np.ascontiguousarray(tri_uv, np.float32).reshape(-1, 6)
        self._check(self._lib.dmt_upload_textures(self._ctx, _p(rgba), C.c_uint64(rgba.shape[0]), _p(desc), C.c_uint32(desc.shape[0]), _p(mt),
                                                  C.c_uint32(mt.shape[0]), _p(uv), C.c_uint64(uv.shape[0])), "dmt_upload_textures")

    def upload_area_lights(self, tri, le):
        tri = np.ascontiguousarray(tri, np.uint32).reshape(-1)
        le = np.ascontiguousarray(le, np.float32).reshape(-1, 3)
        assert tri.shape[0] == le.shape[0]
        self._check(self._lib.dmt_upload_area_lights(self._ctx, _p(tri), _p(le), C.c_uint32(tri.shape[0])),
                    "dmt_upload_area_lights")

    def upload_envmap(self, rgb, quat=(0, 0, 0, 1), scale=1.0):
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w = rgb.shape[:2]
        q = np.ascontiguousarray(quat, np.float32)
        self._check(self._lib.dmt_upload_envmap(self._ctx, _p(rgb), int(w), int(h), _p(q), C.c_float(scale)),
                    "dmt_upload_envmap")

    def clear_envmap(self):
        self._check(self._lib.dmt_clear_envmap(self._ctx), "dmt_clear_envmap")

    def test_envmap(self, u2, wi):
        u2, wi = _f32(u2).reshape(-1, 2), _f32(wi).reshape(-1, 3)
        n = u2.shape[0]
        assert wi.shape[0] == n
        out = dict(wi=np.zeros((n, 3), np.float32), pdf=np.zeros(n, np.float32), uv=np.zeros((n, 2), np.float32),
                   Le=np.zeros((n, 3), np.float32), ok=np.zeros(n, np.int32), Le_dir=np.zeros((n, 3), np.float32),
                   pdf_dir=np.zeros(n, np.float32))
        self._check(self._lib.dmt_test_envmap(self._ctx, n, _p(u2), _p(wi), _p(out["wi"]), _p(out["pdf"]), _p(out["uv"]),
                                              _p(out["Le"]), _p(out["ok"]), _p(out["Le_dir"]), _p(out["pdf_dir"])),
                    "dmt_test_envmap")
        return out

    def set_limits(self, max_depth):
        self._check(self._lib.dmt_set_limits(self._ctx, int(max_depth)), "dmt_set_limits")

    def set_accel(self, mode):
        self._check(self._lib.dmt_set_accel(self._ctx, int(mode)), "dmt_set_accel")

    def set_accel_build(self, mode):
        """Who builds the tree of DMT_ACCEL_BVH: BVH_BUILD_HOST (0, default) or BVH_BUILD_DEVICE (1)."""
        self._check(self._lib.dmt_set_accel_build(self._ctx, int(mode)), "dmt_set_accel_build")

    def accel_build_info(self):
        """The build record of the current tree: dict(builder, depth, triangles, nodes, pairs, build_ms, temp_bytes)."""
        rec = AccelBuildRecord()
        self._check(self._lib.dmt_accel_build_info(self._ctx, C.byref(rec)), "dmt_accel_build_info")
        return {name: getattr(rec, name) for name, _ in AccelBuildRecord._fields_ if name != "reserved"}

    def download_accel(self):
        """The current tree: (nodes [node_count, 64] uint8, pairs [pair_count, 2] uint32 original indices)."""
        info = self.accel_build_info()
        nodes = np.zeros((max(info["nodes"], 1), 64), np.uint8)
        pairs = np.zeros((max(info["pairs"], 1), 2), np.uint32)
        self._check(self._lib.dmt_accel_download(self._ctx, _p(nodes), C.c_size_t(nodes.shape[0]), _p(pairs), C.c_size_t(pairs.shape[0])),
                    "dmt_accel_download")
        return nodes[:info["nodes"]].copy(), pairs[:info["pairs"]].copy()

    def set_light_sampling(self, mode):
        """0 = uniform pick (reference, parity mode), 1 = light tree (csrc/light_tree.hpp)."""
        self._check(self._lib.dmt_set_light_sampling(self._ctx, int(mode)), "dmt_set_light_sampling")

    def set_texture_filter(self, mode):
        """TEXFILTER_LEVEL0 (default: level-0 bilinear lookups) or TEXFILTER_REFERENCE (first-hit MIP / EWA filtering)."""
        self._check(self._lib.dmt_set_texture_filter(self._ctx, int(mode)), "dmt_set_texture_filter")

    def set_bvh_strategy(self, strategy, paths_per_pass=0):
        """0 = automatic, 1 = megakernel, 2 = device-side wavefront (films are bit-identical)."""
        self._check(self._lib.dmt_set_bvh_strategy(self._ctx, int(strategy), C.c_uint64(int(paths_per_pass))), "dmt_set_bvh_strategy")

    def set_partition(self, rank, world):
        self._check(self._lib.dmt_set_partition(self._ctx, int(rank), int(world)), "dmt_set_partition")

    def set_chunk(self, samples_per_item):
        self._check(self._lib.dmt_set_chunk(self._ctx, C.c_uint32(samples_per_item)), "dmt_set_chunk")

    def set_sampler_table(self, mode, budget_bytes=0):
        """SAMPLER_TABLE_OFF / _AUTO (default) / _FORCE; budget_bytes bounds the table's device memory (0 = 512 MiB).
        Films are bit-identical in every mode."""
        self._check(self._lib.dmt_set_sampler_table(self._ctx, int(mode), C.c_uint64(int(budget_bytes))), "dmt_set_sampler_table")

    def set_ggx_batch(self, batch):
        """GGX hits of the plain brute-force launches (k_megakernel) are shaded `batch` at a time (0: in the pass that
        finds them).  Films are bit-identical for every value."""
        self._check(self._lib.dmt_set_ggx_batch(self._ctx, C.c_uint32(int(batch))), "dmt_set_ggx_batch")

    def ggx_batch(self):
        """The context's batch size (dmt_ggx_batch_diag; synchronises)."""
        out = (C.c_uint64 * 5)()
        self._check(self._lib.dmt_ggx_batch_diag(self._ctx, out), "dmt_ggx_batch_diag")
        return int(out[4])

    def tri_kind_bits(self, triangles):
        """The per-triangle material kinds as a launch reads them (dmt_tri_kind_bits): uint32 [(triangles + 31) // 32], bit i
        of word i // 32 set when triangle i has a GGX material."""
        out = np.zeros((int(triangles) + 31) // 32, np.uint32)
        self._check(self._lib.dmt_tri_kind_bits(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size)), "dmt_tri_kind_bits")
        return out

    def set_stream(self, stream_ptr):
        self._check(self._lib.dmt_set_stream(self._ctx, C.c_void_p(stream_ptr)), "dmt_set_stream")

    # ---- film ------------------------------------------------------------------------------
    def film_clear(self):
        self._check(self._lib.dmt_film_clear(self._ctx), "dmt_film_clear")

    def film_bind(self, mean_ptr, m2_ptr):
        self._check(self._lib.dmt_film_bind(self._ctx, C.c_void_p(mean_ptr), C.c_void_p(m2_ptr)), "dmt_film_bind")

    def film_device_ptrs(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self._lib.dmt_film_device_ptrs(self._ctx, C.byref(a), C.byref(b)), "dmt_film_device_ptrs")
        return a.value, b.value

    def download_film(self):
        mean = np.zeros((self.height, self.width, 4), np.float32)
        m2 = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._lib.dmt_download_film(self._ctx, _p(mean), _p(m2)), "dmt_download_film")
        return mean, m2

    # ---- render ----------------------------------------------------------------------------
    def render(self, spp, sample_offset=0, region=None):
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        self._check(self._lib.dmt_render(self._ctx, C.c_uint32(sample_offset), C.c_uint32(spp), int(x0), int(y0),
                                         int(x1), int(y1)), "dmt_render")

    def render_adaptive(self, threshold, max_spp, step_spp, min_spp=0, region=None):
        """Adaptive sampling (dmt_render_adaptive): rounds of step_spp samples from sample 0 until each pixel of the region
        has max_spp samples, or at least min_spp and a relative standard error of its mean <= threshold.  Synchronous.
        Returns (rounds launched, path samples traced).  Call film_clear() first for a fresh image."""
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        rounds, samples = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.dmt_render_adaptive(self._ctx, C.c_uint32(min_spp), C.c_uint32(max_spp), C.c_uint32(step_spp),
                                                  C.c_float(threshold), int(x0), int(y0), int(x1), int(y1), C.byref(rounds),
                                                  C.byref(samples)), "dmt_render_adaptive")
        return int(rounds.value), int(samples.value)

    def render_stats(self, spp, sample_offset=0, region=None):
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        out = np.zeros(6, np.uint64)
        self._check(self._lib.dmt_render_stats(self._ctx, C.c_uint32(sample_offset), C.c_uint32(spp), int(x0), int(y0),
                                               int(x1), int(y1), _p(out)), "dmt_render_stats")
        keys = ["samples", "closest_rays", "shadow_rays", "node_visits", "tri_tests", "bounces"]
        return dict(zip(keys, (int(v) for v in out)))

    def render_profile(self, spp, sample_offset=0, region=None):
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        out = np.zeros(16, np.uint64)
        self._check(self._lib.dmt_render_profile(self._ctx, C.c_uint32(sample_offset), C.c_uint32(spp), int(x0), int(y0),
                                                 int(x1), int(y1), _p(out)), "dmt_render_profile")
        keys = ["samples", "closest_rays", "shadow_rays", "node_visits", "tri_tests", "bounces", "it_node", "it_leaf",
                "it_shade", "it_outer", "it_prep", "lanes_leaf", "lanes_shade", "lanes_prep", "dead_nodes", "overflow_pushes"]
        return dict(zip(keys, (int(v) for v in out)))

    # ---- denoiser -----------------------------------------------------------
    def render_aovs(self, aov_spp=4):
        """Feature pass (dmt_render_aovs): albedo / normal / position planes from camera samples 0 .. aov_spp-1 of every
        pixel, kept on the device for denoise().  Asynchronous."""
        self._check(self._lib.dmt_render_aovs(self._ctx, C.c_uint32(aov_spp)), "dmt_render_aovs")
        self._aov_shape = (self.height, self.width)

    def upload_aovs(self, albedo, normal, position):
        """Host planes (H x W x 4 each, layout of dmt_render_aovs) as the context's AOVs."""
        a, n, p = _f32(albedo), _f32(normal), _f32(position)
        assert a.ndim == 3 and a.shape[2] == 4 and a.shape == n.shape == p.shape
        h, w = a.shape[:2]
        self._check(self._lib.dmt_upload_aovs(self._ctx, _p(a), _p(n), _p(p), int(w), int(h)), "dmt_upload_aovs")
        self._aov_shape = (h, w)

    def download_aovs(self):
        """(albedo, normal, position), each H x W x 4 float32."""
        h, w = self._aov_shape or (self.height, self.width)
        out = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
        self._check(self._lib.dmt_download_aovs(self._ctx, *[_p(x) for x in out]), "dmt_download_aovs")
        return tuple(out)

    def denoise(self, params=None, film=None):
        """dmt_denoise: the film (the context's own, or `film` = (mean, m2) host arrays of the camera's size) denoised with
        the context's AOVs -> H x W x 4 float32 (w = 1).  `params`: a dict overriding denoise_defaults().  Synchronous;
        the kernels' HIP-event time lands in self.denoise_ms."""
        p = denoise_defaults()
        unknown = set(params or {}) - set(p)
        if unknown:
            raise ValueError(f"unknown denoise parameters {sorted(unknown)}")
        p.update(params or {})
        cp = DenoiseParams(int(p["iterations"]), float(p["sigma_normal"]), float(p["sigma_position"]), float(p["sigma_albedo"]),
                           float(p["sigma_luminance"]))
        mean = m2 = None
        if film is not None:
            mean, m2 = _f32(film[0]), _f32(film[1])
            assert mean.shape == m2.shape == (self.height, self.width, 4)
        out = np.zeros((self.height, self.width, 4), np.float32)
        ms = C.c_float()
        self._check(self._lib.dmt_denoise(self._ctx, C.byref(cp), _p(mean), _p(m2), _p(out), C.byref(ms)), "dmt_denoise")
        self.denoise_ms = ms.value
        return out

    # ---- temporal accumulation ------------------------------------------------
    def download_aov_surface(self):
        """The surface plane of the AOVs, H x W x 4 float32: (triangle, bu, bv, 1) of the first camera sample that hit."""
        h, w = self._aov_shape or (self.height, self.width)
        out = np.zeros((h, w, 4), np.float32)
        self._check(self._lib.dmt_download_aov_surface(self._ctx, _p(out)), "dmt_download_aov_surface")
        return out

    def upload_aov_surface(self, surface):
        """A host surface plane (H x W x 4) of the size of the context's AOVs; upload_aovs() drops it, so it comes after."""
        s = _f32(surface)
        assert s.ndim == 3 and s.shape[2] == 4
        self._check(self._lib.dmt_upload_aov_surface(self._ctx, _p(s), int(s.shape[1]), int(s.shape[0])), "dmt_upload_aov_surface")

    def denoise_temporal(self, params=None, temporal=None, film=None):
        """dmt_denoise_temporal: denoise() with the previous call's accumulated plane reprojected into this frame.
        `temporal`: a dict overriding temporal_defaults().  The a-trous passes' and the reprojection's HIP-event time lands in
        self.denoise_ms; temporal_info() has the reprojection's own."""
        p = denoise_defaults()
        t = temporal_defaults()
        unknown = (set(params or {}) - set(p)) | (set(temporal or {}) - set(t))
        if unknown:
            raise ValueError(f"unknown denoise parameters {sorted(unknown)}")
        p.update(params or {})
        t.update(temporal or {})
        cp = DenoiseParams(int(p["iterations"]), float(p["sigma_normal"]), float(p["sigma_position"]), float(p["sigma_albedo"]),
                           float(p["sigma_luminance"]))
        ct = TemporalParams(float(t["alpha"]), float(t["normal_threshold"]), float(t["plane_threshold"]))
        mean = m2 = None
        if film is not None:
            mean, m2 = _f32(film[0]), _f32(film[1])
            assert mean.shape == m2.shape == (self.height, self.width, 4)
        out = np.zeros((self.height, self.width, 4), np.float32)
        ms = C.c_float()
        self._check(self._lib.dmt_denoise_temporal(self._ctx, C.byref(cp), C.byref(ct), _p(mean), _p(m2), _p(out), C.byref(ms)),
                    "dmt_denoise_temporal")
        self.denoise_ms = ms.value
        return out

    def temporal_reset(self):
        """Forget the history: the next denoise_temporal() starts at h = 1."""
        self._check(self._lib.dmt_temporal_reset(self._ctx), "dmt_temporal_reset")

    def temporal_info(self):
        """dict(frames, reprojected, reset, temporal_ms, history_bytes) of the history and the last temporal call."""
        rec = TemporalRecord()
        self._check(self._lib.dmt_temporal_info(self._ctx, C.byref(rec)), "dmt_temporal_info")
        return {name: getattr(rec, name) for name, _ in TemporalRecord._fields_}

    def download_history(self):
        """The history: (accumulated (rgb, variance of the mean) H x W x 4, length H x W), float32."""
        cv = np.zeros((self.height, self.width, 4), np.float32)
        ln = np.zeros((self.height, self.width), np.float32)
        self._check(self._lib.dmt_temporal_download(self._ctx, _p(cv), _p(ln)), "dmt_temporal_download")
        return cv, ln

    # ---- display transform ------------------------------------------------------
    def display(self, params=None, image=None, want=("float", "u8")):
        """dmt_display: a linear plane (the context's film mean, or `image`, an H x W x 4 host array of the camera's size)
        through exposure, bloom, tone curve, transfer function and quantiser.  `params`: a dict overriding
        display_defaults().  `want` names the outputs: "float" (H x W x 4 float32, w = 1) and / or "u8" (H x W x 4 uint8,
        A = 255).  Returns them in that order, or the one array when one is asked for.  Synchronous; the kernels' HIP-event
        time lands in self.display_ms, display_info() has the rest."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or set(want) - {"float", "u8"}:
            raise ValueError(f"want must name 'float' and / or 'u8', got {want!r}")
        cp = _display_params(params)
        src = None
        if image is not None:
            src = _f32(image)
            assert src.shape == (self.height, self.width, 4)
        out4 = np.zeros((self.height, self.width, 4), np.float32) if "float" in want else None
        out8 = np.zeros((self.height, self.width, 4), np.uint8) if "u8" in want else None
        ms = C.c_float()
        self._check(self._lib.dmt_display(self._ctx, C.byref(cp), _p(src), _p(out4), _p(out8), C.byref(ms)), "dmt_display")
        self.display_ms = ms.value
        outs = tuple(out4 if w == "float" else out8 for w in want)
        return outs[0] if len(outs) == 1 else outs

    def display_device(self, params=None, src_ptr=None, out4_ptr=None, out8_ptr=None):
        """dmt_display_device: display() on device pointers (e.g. torch data_ptr()): the source plane (None: the film mean),
        the float4 output and the RGBA8 output (either None, not both).  Asynchronous on the context's stream, except that
        auto exposure waits for its histogram."""
        cp = _display_params(params)
        self._check(self._lib.dmt_display_device(self._ctx, C.byref(cp), C.c_void_p(src_ptr), C.c_void_p(out4_ptr),
                                                 C.c_void_p(out8_ptr)), "dmt_display_device")

    def display_info(self):
        """dict of the last display call: histogram (uint32[256]), counted, skipped, nonfinite, levels, avg_log2, scale,
        histogram_ms, bloom_ms, resolve_ms, width, height.  Waits for the stream after display_device()."""
        rec = DisplayRecord()
        self._check(self._lib.dmt_display_info(self._ctx, C.byref(rec)), "dmt_display_info")
        out = {name: getattr(rec, name) for name, _ in DisplayRecord._fields_ if name != "histogram"}
        out["histogram"] = np.array(rec.histogram, np.uint32)
        out["scale"] = np.float32(rec.scale)
        return out

    def test_camera_project(self, points):
        """dmt_test_camera_project: camera_project() on the device under the context's camera."""
        p = _f32(points).reshape(-1, 3)
        xy, depth = np.zeros((p.shape[0], 2), np.float32), np.zeros(p.shape[0], np.float32)
        self._check(self._lib.dmt_test_camera_project(self._ctx, int(p.shape[0]), _p(p), _p(xy), _p(depth)), "dmt_test_camera_project")
        return xy, depth

    def sync(self):
        self._check(self._lib.dmt_sync(self._ctx), "dmt_sync")

    def sched_diag(self, reset=False):
        """Counters of the in-launch fold hand-over (dmt_sched_diag) and, under ggx_*, of the GGX batching
        (dmt_ggx_batch_diag, read first: the reset clears both); synchronises the stream."""
        out = (C.c_uint64 * 8)()
        if not hasattr(self._lib, "dmt_sched_diag"):   # an older build loaded through DMT_HIP_LIB for an A/B run
            return dict.fromkeys(["folds", "handed_over", "folded_for_others", "slab_stalls", "early_exits",
                                  "max_stall_ticks_10ns", "launched", "slabs_per_wave"], 0)
        ggx = (C.c_uint64 * 5)()
        if hasattr(self._lib, "dmt_ggx_batch_diag"):   # (read before dmt_sched_diag resets the counters)
            self._check(self._lib.dmt_ggx_batch_diag(self._ctx, ggx), "dmt_ggx_batch_diag")
        self._check(self._lib.dmt_sched_diag(self._ctx, out, int(bool(reset))), "dmt_sched_diag")
        keys = ["folds", "handed_over", "folded_for_others", "slab_stalls", "early_exits", "max_stall_ticks_10ns", "launched", "slabs_per_wave"]
        d = dict(zip(keys, [int(x) for x in out]))
        d.update(ggx_parked=int(ggx[0]), ggx_resumed=int(ggx[1]), ggx_shade_passes=int(ggx[2]), ggx_shaded_full=int(ggx[3]))
        return d

    def kernel_time(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._lib.dmt_kernel_time(self._ctx, C.byref(ms), C.byref(n), int(bool(reset))), "dmt_kernel_time")
        return ms.value, n.value

    def set_emitter_sampling(self, mode):
        """0 = uniform pick among lights and emissive triangles (default), 1 = the emitter tree (csrc/emitter_tree.hpp)."""
        self._check(self._lib.dmt_set_emitter_sampling(self._ctx, int(mode)), "dmt_set_emitter_sampling")

    def emitter_tree_info(self):
        """dict(mode, active, emitters, nodes, depth, build_ms) of dmt_emitter_tree_info."""
        mode, active, depth = C.c_int(), C.c_int(), C.c_int()
        emitters, nodes, ms = C.c_uint32(), C.c_uint32(), C.c_double()
        self._check(self._lib.dmt_emitter_tree_info(self._ctx, C.byref(mode), C.byref(active), C.byref(emitters), C.byref(nodes), C.byref(depth),
                                                    C.byref(ms)), "dmt_emitter_tree_info")
        return dict(mode=mode.value, active=bool(active.value), emitters=emitters.value, nodes=nodes.value, depth=depth.value, build_ms=ms.value)

    def kernel_scratch(self):
        """Scratch bytes per lane of the kernel a render would launch now (dmt_kernel_scratch)."""
        v = C.c_int()
        self._check(self._lib.dmt_kernel_scratch(self._ctx, C.byref(v)), "dmt_kernel_scratch")
        return v.value

    def kernel_info(self):
        v = [C.c_int() for _ in range(5)]
        self._check(self._lib.dmt_kernel_info(self._ctx, *[C.byref(x) for x in v]), "dmt_kernel_info")
        keys = ["vgprs", "sgprs", "lds_bytes", "blocks_per_cu", "cu_count"]
        return dict(zip(keys, (x.value for x in v)))

    # ---- device unit-test entry points -----------------------------------------------------
    def test_triangle_intersect(self, xs, ys, zs, o, d):
        xs, ys, zs = _f32(xs), _f32(ys), _f32(zs)
        n = xs.size // 4
        o, d = _f32(o), _f32(d)
        hit = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        pos, nrm, err = (np.zeros((n, 3), np.float32) for _ in range(3))
        self._check(self._lib.dmt_test_triangle_intersect(self._ctx, _p(xs), _p(ys), _p(zs), C.c_size_t(n), _p(o),
                                                          _p(d), _p(hit), _p(t), _p(pos), _p(nrm), _p(err)),
                    "dmt_test_triangle_intersect")
        return hit, t, pos, nrm, err

    def test_sampler(self, w, h, pxs, pys, ss, ndims):
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        hi = np.zeros(n, np.int32)
        p2 = np.zeros((n, 2), np.float32)
        d = np.zeros((n, ndims), np.float32)
        self._check(self._lib.dmt_test_sampler(self._ctx, int(w), int(h), n, _p(pxs), _p(pys), _p(ss), int(ndims),
                                               _p(hi), _p(p2), _p(d)), "dmt_test_sampler")
        return hi, p2, d

    def test_sampler_table(self, w, h, s0, n):
        """The sampler table of samples [s0, s0 + n) of a w x h frame: (values [n, ph, pw, 8], jitter [n, ph, pw, 2])."""
        pw, ph = min(int(w), 128), min(int(h), 128)
        vals = np.zeros((n, ph, pw, 8), np.float32)
        jit = np.zeros((n, ph, pw, 2), np.float32)
        self._check(self._lib.dmt_test_sampler_table(self._ctx, int(w), int(h), C.c_uint32(int(s0)), C.c_uint32(int(n)), _p(vals), _p(jit)),
                    "dmt_test_sampler_table")
        return vals, jit

    def test_camera_rays(self, pxs, pys, ss):
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        o = np.zeros((n, 3), np.float32)
        d = np.zeros((n, 3), np.float32)
        self._check(self._lib.dmt_test_camera_rays(self._ctx, n, _p(pxs), _p(pys), _p(ss), _p(o), _p(d)),
                    "dmt_test_camera_rays")
        return o, d

    def test_film_positions(self, pxs, pys, ss):
        """dmt_test_film_positions: the film positions [n, 2] of the samples as the device forms them under the context's
        pixel filter (the device twin of pixel_filter_positions)."""
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        xy = np.zeros((n, 2), np.float32)
        self._check(self._lib.dmt_test_film_positions(self._ctx, n, _p(pxs), _p(pys), _p(ss), _p(xy)), "dmt_test_film_positions")
        return xy

    def test_lens_values(self, pxs, pys, ss):
        """dmt_test_lens_values: (u10, u11) [n, 2] of the samples, as the device computes them."""
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        u = np.zeros((n, 2), np.float32)
        self._check(self._lib.dmt_test_lens_values(self._ctx, n, _p(pxs), _p(pys), _p(ss), _p(u)), "dmt_test_lens_values")
        return u

    def test_bsdf(self, bsdf32, ns, wo, u2, uc, wi_eval):
        b = np.ascontiguousarray(bsdf32, np.uint8).reshape(32)
        ns, wo, wi_eval = _f32(ns, (-1, 3)), _f32(wo, (-1, 3)), _f32(wi_eval, (-1, 3))
        u2, uc = _f32(u2, (-1, 2)), _f32(uc, (-1,))
        n = ns.shape[0]
        prep = np.zeros((n, 12), np.float32)
        samp = np.zeros((n, 10), np.float32)
        ev = np.zeros((n, 4), np.float32)
        self._check(self._lib.dmt_test_bsdf(self._ctx, _p(b), n, _p(ns), _p(wo), _p(u2), _p(uc), _p(wi_eval),
                                            _p(prep), _p(samp), _p(ev)), "dmt_test_bsdf")
        return prep, samp, ev

    def test_bsdf_ng(self, bsdf32, ns, ng, wo, u2, uc, wi_eval):
        """test_bsdf with a geometric normal `ng` of its own for the sampling and evaluation routines."""
        b = np.ascontiguousarray(bsdf32, np.uint8).reshape(32)
        ns, ng, wo, wi_eval = _f32(ns, (-1, 3)), _f32(ng, (-1, 3)), _f32(wo, (-1, 3)), _f32(wi_eval, (-1, 3))
        u2, uc = _f32(u2, (-1, 2)), _f32(uc, (-1,))
        n = ns.shape[0]
        assert ng.shape[0] == n and wo.shape[0] == n and wi_eval.shape[0] == n and u2.shape[0] == n and uc.shape[0] == n
        prep = np.zeros((n, 12), np.float32)
        samp = np.zeros((n, 10), np.float32)
        ev = np.zeros((n, 4), np.float32)
        self._check(self._lib.dmt_test_bsdf_ng(self._ctx, _p(b), n, _p(ns), _p(ng), _p(wo), _p(u2), _p(uc), _p(wi_eval),
                                               _p(prep), _p(samp), _p(ev)), "dmt_test_bsdf_ng")
        return prep, samp, ev

    def test_material(self, tri, bu, bv, ng):
        """The uploaded scene's material at hits (tri, bu, bv) with geometric normals `ng` after the texture patch:
        (records (n, 32) uint8, ns (n, 3), second records of fractional-metallic pairs (n, 32), metallic fraction (n,))."""
        tri, bu, bv, ng = _i32(tri), _f32(bu, (-1,)), _f32(bv, (-1,)), _f32(ng, (-1, 3))
        n = tri.shape[0]
        assert bu.shape[0] == n and bv.shape[0] == n and ng.shape[0] == n
        rec, rec2 = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
        ns = np.zeros((n, 3), np.float32)
        mix = np.zeros(n, np.float32)
        self._check(self._lib.dmt_test_material(self._ctx, n, _p(tri), _p(bu), _p(bv), _p(ng), _p(rec), _p(ns), _p(rec2),
                                                _p(mix)), "dmt_test_material")
        return rec, ns, rec2, mix

    def test_light(self, light32, pos, nrm, u2, had_t):
        l = np.ascontiguousarray(light32, np.uint8).reshape(32)
        pos, nrm, u2 = _f32(pos, (-1, 3)), _f32(nrm, (-1, 3)), _f32(u2, (-1, 2))
        ht = _i32(had_t)
        n = pos.shape[0]
        out = np.zeros((n, 14), np.float32)
        self._check(self._lib.dmt_test_light(self._ctx, _p(l), n, _p(pos), _p(nrm), _p(u2), _p(ht), _p(out)),
                    "dmt_test_light")
        return out

    def test_light_tree(self, pos, nrm, u, start_pmf=1.0):
        """dmt_test_light_tree: the device's light choice at shading points pos [k,3] with normals nrm [k,3] and one random
        number each, under the context's light sampling mode -> (indices [k,4] (-1 = none), pmfs [k,4], counts [k])."""
        pos, nrm, u = _f32(pos, (-1, 3)), _f32(nrm, (-1, 3)), _f32(u, (-1,))
        k = pos.shape[0]
        assert nrm.shape[0] == k and u.shape[0] == k
        idx, pmf, cnt = np.zeros((k, 4), np.int32), np.zeros((k, 4), np.float32), np.zeros(k, np.int32)
        self._check(self._lib.dmt_test_light_tree(self._ctx, k, _p(pos), _p(nrm), _p(u), C.c_float(start_pmf), _p(idx), _p(pmf), _p(cnt)),
                    "dmt_test_light_tree")
        return idx, pmf, cnt

    def test_emitter_tree(self, pos, nrm, u, start_pmf=1.0):
        """dmt_test_emitter_tree: the device's emitter choice at shading points pos [k,3] with normals nrm [k,3] and one random
        number each -> (index [k] (-1 = none), pmf [k], pmf_by_trail [k])."""
        pos, nrm, u = _f32(pos, (-1, 3)), _f32(nrm, (-1, 3)), _f32(u, (-1,))
        k = pos.shape[0]
        assert nrm.shape[0] == k and u.shape[0] == k
        idx, pmf, trail = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float32)
        self._check(self._lib.dmt_test_emitter_tree(self._ctx, k, _p(pos), _p(nrm), _p(u), C.c_float(start_pmf), _p(idx), _p(pmf), _p(trail)),
                    "dmt_test_emitter_tree")
        return idx, pmf, trail

    def test_half(self, floats=None, halves=None):
        h_out = f_out = None
        n = 0
        if floats is not None:
            floats = _f32(floats, (-1,))
            n = floats.shape[0]
            h_out = np.zeros(n, np.uint16)
        if halves is not None:
            halves = np.ascontiguousarray(halves, np.uint16).reshape(-1)
            n = halves.shape[0]
            f_out = np.zeros(n, np.float32)
        if floats is not None and halves is not None:
            assert floats.shape[0] == halves.shape[0]
        self._check(self._lib.dmt_test_half(self._ctx, n, _p(floats), _p(h_out), _p(halves), _p(f_out)),
                    "dmt_test_half")
        return h_out, f_out

    def test_trace_samples(self, pxs, pys, ss):
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        out = np.zeros((n, 3), np.float32)
        self._check(self._lib.dmt_test_trace_samples(self._ctx, n, _p(pxs), _p(pys), _p(ss), _p(out)),
                    "dmt_test_trace_samples")
        return out

    def test_texture_filter(self, tri, bu, bv, tex, depth=0):
        """Filtered lookups of texture `tex` at (tri, bu, bv) by the filtering kernels' device code, as at a hit of depth
        `depth` (0 = the camera ray's).  Returns (rgb (n, 3), branch (n,), lod (n,))."""
        tri, tex = _i32(tri), _i32(tex)
        bu, bv = _f32(bu), _f32(bv)
        n = tri.shape[0]
        tex = np.ascontiguousarray(np.broadcast_to(tex, (n,)), np.int32)
        depth = np.ascontiguousarray(np.broadcast_to(_i32(depth), (n,)), np.int32)
        assert bu.shape[0] == n and bv.shape[0] == n
        rgb = np.zeros((n, 3), np.float32)
        branch = np.zeros(n, np.int32)
        lod = np.zeros(n, np.float32)
        self._check(self._lib.dmt_test_texture_filter(self._ctx, n, _p(tri), _p(bu), _p(bv), _p(tex), _p(depth), _p(rgb),
                                                      _p(branch), _p(lod)), "dmt_test_texture_filter")
        return rgb, branch, lod

    def test_trace_log(self, px, py, s, cap=64):
        rec = np.zeros((cap, 12), np.float32)
        n = C.c_int()
        L = np.zeros(3, np.float32)
        self._check(self._lib.dmt_test_trace_log(self._ctx, int(px), int(py), int(s), _p(rec), int(cap), C.byref(n),
                                                 _p(L)), "dmt_test_trace_log")
        return rec[:n.value], L

    def test_shutter_times(self, pxs, pys, ss):
        """dmt_test_shutter_times: the times [n] of the samples under the context's shutter, as the device computes them."""
        pxs, pys, ss = _i32(pxs), _i32(pys), _i32(ss)
        n = pxs.shape[0]
        t = np.zeros(n, np.float32)
        self._check(self._lib.dmt_test_shutter_times(self._ctx, n, _p(pxs), _p(pys), _p(ss), _p(t)), "dmt_test_shutter_times")
        return t

    def test_closest_hit_at(self, o, d, time):
        """dmt_test_closest_hit_at: closest hit of ray i against the scene at time[i] under the current accel mode ->
        (tri [n], t [n], uv [n, 2])."""
        o, d = _f32(o, (-1, 3)), _f32(d, (-1, 3))
        n = o.shape[0]
        time = np.ascontiguousarray(np.broadcast_to(np.asarray(time, np.float32), (n,)))
        idx, t, uv = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
        self._check(self._lib.dmt_test_closest_hit_at(self._ctx, n, _p(o), _p(d), _p(time), _p(idx), _p(t), _p(uv)),
                    "dmt_test_closest_hit_at")
        return idx, t, uv

    def test_trace_pair(self, o, d, so, sd, smax):
        """dmt_test_trace_pair: pair i = (closest ray o, d; shadow ray so, sd up to smax) through one trace call of the
        render kernels under the current accel mode -> (tri [n], uv [n, 2], occluded [n] bool)."""
        o, d, so, sd = _f32(o, (-1, 3)), _f32(d, (-1, 3)), _f32(so, (-1, 3)), _f32(sd, (-1, 3))
        n = o.shape[0]
        assert d.shape[0] == n and so.shape[0] == n and sd.shape[0] == n
        smax = np.ascontiguousarray(np.broadcast_to(np.asarray(smax, np.float32), (n,)))
        idx, uv, occ = np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        self._check(self._lib.dmt_test_trace_pair(self._ctx, n, _p(o), _p(d), _p(so), _p(sd), _p(smax), _p(idx), _p(uv), _p(occ)),
                    "dmt_test_trace_pair")
        return idx, uv, occ.astype(bool)

    def test_closest_hit(self, o, d):
        o, d = _f32(o, (-1, 3)), _f32(d, (-1, 3))
        n = o.shape[0]
        idx = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        self._check(self._lib.dmt_test_closest_hit(self._ctx, n, _p(o), _p(d), _p(idx), _p(t)),
                    "dmt_test_closest_hit")
        return idx, t
