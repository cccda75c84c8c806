"""Temporal accumulation without a GPU (dmt_denoise_temporal): the C ABI declares the entry points and the
parameter layouts, the binding wraps them, the library refuses bad calls, the host projection (dmt_camera_project) inverts
the oracle's camera rays, and the numpy restatement (tests/temporal_ref.py) has the accumulation's properties."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as T
from test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
NEW = ("dmt_download_aov_surface", "dmt_upload_aov_surface", "dmt_camera_project", "dmt_test_camera_project",
       "dmt_temporal_defaults", "dmt_denoise_temporal", "dmt_temporal_reset", "dmt_temporal_info", "dmt_temporal_download")

# The worst distance, in pixels, between dmt_camera_project(o + t d) and the film position of the sample that made the ray
# (o, d), over every pixel of the two 1024 x 1024 cameras below at t = 0.5, 2 and 7.  Measured (this test prints it):
# 7.32e-4 pixels; the bound is 4 x that.  It is the fp32 rounding of the ray's unit direction and of o + t d, which the
# projection magnifies by focal / pixel size, not an error of the projection (whose own rounding is a few ulps of 1024).
PROJECT_ERR_MEASURED = 7.32e-4
PROJECT_ERR_BOUND = 4 * PROJECT_ERR_MEASURED


def _header():
    return (ROOT / "include" / "dmt_hip.h").read_text()


def _decl(name):
    text = _header()
    m = re.search(r"\b(int|dmt_temporal_params) " + name + r"\(", text)
    decl = text[m.start():]
    return " ".join(decl[:decl.index(";")].split())


def _struct_fields(name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [f.strip() for f in body.split(";") if f.strip()]


def test_header_declares_the_temporal_entry_points():
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert _decl("dmt_denoise_temporal") == ("int dmt_denoise_temporal(dmt_ctx* ctx, const dmt_denoise_params* params, "
                                             "const dmt_temporal_params* tparams, const float* mean4, const float* m24, "
                                             "float* out4, float* kernel_ms)")
    assert _decl("dmt_temporal_defaults") == "dmt_temporal_params dmt_temporal_defaults(void)"
    assert _decl("dmt_camera_project") == "int dmt_camera_project(const dmt_camera* cam, int n, const float* p3, float* xy2, float* depth)"
    assert _decl("dmt_test_camera_project") == "int dmt_test_camera_project(dmt_ctx* ctx, int n, const float* p3, float* xy2, float* depth)"
    assert _decl("dmt_download_aov_surface") == "int dmt_download_aov_surface(dmt_ctx* ctx, float* surface4)"
    assert _decl("dmt_upload_aov_surface") == "int dmt_upload_aov_surface(dmt_ctx* ctx, const float* surface4, int width, int height)"
    assert _decl("dmt_temporal_download") == "int dmt_temporal_download(dmt_ctx* ctx, float* color_var4, float* length1)"
    # the existing signatures did not change
    assert _decl("dmt_download_aovs") == "int dmt_download_aovs(dmt_ctx* ctx, float* albedo4, float* normal4, float* position4)"
    assert _decl("dmt_upload_aovs") == ("int dmt_upload_aovs(dmt_ctx* ctx, const float* albedo4, const float* normal4, "
                                        "const float* position4, int width, int height)")


def test_struct_layouts(pkg):
    from cuda_optix_pathtracing_amd import binding
    assert _struct_fields("dmt_temporal_params") == ["float alpha", "float normal_threshold", "float plane_threshold"]
    assert _struct_fields("dmt_temporal_record") == ["uint32_t frames", "uint32_t reprojected", "uint32_t reset", "float temporal_ms",
                                                     "uint64_t history_bytes"]
    assert [n for n, _ in binding.TemporalParams._fields_] == ["alpha", "normal_threshold", "plane_threshold"]
    assert C.sizeof(binding.TemporalParams) == 12
    assert [n for n, _ in binding.TemporalRecord._fields_] == ["frames", "reprojected", "reset", "temporal_ms", "history_bytes"]
    assert C.sizeof(binding.TemporalRecord) == 24 and binding.TemporalRecord.history_bytes.offset == 16


def test_library_and_binding(pkg):
    lib = pkg.load_library()
    from cuda_optix_pathtracing_amd import binding
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTED_SYMBOLS, s
    for m in ("denoise_temporal", "temporal_reset", "temporal_info", "download_history", "download_aov_surface", "upload_aov_surface"):
        assert callable(getattr(binding.Renderer, m, None)), m
    d = pkg.temporal_defaults()
    assert sorted(d) == sorted(T.DEFAULTS)
    for k in d:
        assert F(d[k]) == F(T.DEFAULTS[k]), k
    assert callable(pkg.camera_project)


def test_null_context_and_bad_arguments_are_invalid(pkg):
    lib = pkg.load_library()
    out = np.zeros(4, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.dmt_denoise_temporal(None, None, None, None, None, p, None) == 1
    assert lib.dmt_temporal_reset(None) == 1
    assert lib.dmt_temporal_info(None, p) == 1
    assert lib.dmt_temporal_download(None, p, None) == 1
    assert lib.dmt_download_aov_surface(None, p) == 1
    assert lib.dmt_upload_aov_surface(None, p, 1, 1) == 1
    assert lib.dmt_test_camera_project(None, 1, p, p, p) == 1
    cam = T.make_camera((0, 1, 0), (0, 0, 0), 8, 8)
    pc = cam.ctypes.data_as(C.c_void_p)
    assert lib.dmt_camera_project(None, 1, p, p, p) == 1
    assert lib.dmt_camera_project(pc, -1, p, p, p) == 1
    assert lib.dmt_camera_project(pc, 1, None, p, p) == 1
    assert lib.dmt_camera_project(pc, 1, p, None, p) == 1
    assert lib.dmt_camera_project(pc, 1, p, p, None) == 1
    assert lib.dmt_camera_project(pc, 0, None, None, None) == 0
    bad = T.make_camera((0, 1, 0), (0, 0, 0), 0, 8)
    assert lib.dmt_camera_project(bad.ctypes.data_as(C.c_void_p), 1, p, p, p) == 1


# ---- the projection ------------------------------------------------------------------------------------------------
def _cameras(O):
    cornell = np.ascontiguousarray(O.cornell_box(1024, 1024).camera, np.uint8).reshape(44).copy()
    tilted = T.make_camera((0.35, 0.8, -0.45), (0.7, -2.5, 1.3), 1024, 1024, focal=35.0, sensor=24.0)
    return {"cornell": cornell, "tilted": tilted}


def test_camera_project_inverts_the_oracles_camera_rays(O, pkg):
    yy, xx = np.mgrid[0:1024, 0:1024]
    px, py = xx.ravel().astype(np.int32), yy.ravel().astype(np.int32)
    worst = 0.0
    for name, cam in _cameras(O).items():
        sc = O.cornell_box(1024, 1024)
        sc.camera[:] = cam
        for s in (0, 5):
            ss = np.full_like(px, s)
            o, d = O.camera_rays(sc, px, py, ss)
            _, p2, _ = O.sampler_stream(1024, 1024, px, py, ss, 2)
            want = np.stack([((p2[:, 0] - F(0.5)) + F(0.5)) + px.astype(F), ((p2[:, 1] - F(0.5)) + F(0.5)) + py.astype(F)], -1)
            for t in (0.5, 2.0, 7.0):
                P = (o + F(t) * d).astype(F)
                xy, depth = pkg.camera_project(cam, P)
                err = float(np.abs(xy.astype(np.float64) - want).max())
                worst = max(worst, err)
                print(f"{name} sample {s} t {t}: worst |projected - film position| = {err:.3e} pixels")
                np.testing.assert_allclose(depth, F(t) * (d @ T.proj_xf(cam)["fwd"]), rtol=2e-5, atol=0)
                # the restatement is the same arithmetic, bit for bit
                fx, fy, dz = T.project(T.proj_xf(cam), P)
                assert np.array_equal(fx, xy[:, 0]) and np.array_equal(fy, xy[:, 1]) and np.array_equal(dz, depth)
    print(f"worst over all: {worst:.3e} pixels (bound {PROJECT_ERR_BOUND:.3e})")
    assert worst <= PROJECT_ERR_BOUND
    assert worst >= PROJECT_ERR_MEASURED / 4, "the recorded measurement no longer describes this test"


def test_points_behind_the_camera_have_nonpositive_depth(pkg):
    cam = T.make_camera((0, 1, 0), (0, 0, 0), 64, 64)
    _, depth = pkg.camera_project(cam, np.array([[0, 2, 0], [0, -2, 0], [1, 0, 0]], F))
    assert depth[0] == 2 and depth[1] == -2 and depth[2] == 0


# ---- the restatement -----------------------------------------------------------------------------------------------
def synthetic(h, w, seed, cam=None):
    """Two frames' worth of inputs over real geometry: a floor quad and a tilted quad in front of a camera, a background
    strip; surface / normal / position planes by ray casting in float64, film noise with N from 2 to 1000.  Returns a dict
    with verts [4, 9], camera, albedo, normal, position, surface and a function film(seed) -> (mean, m2)."""
    cam = T.make_camera((0, 1, -0.25), (0.1, -3.0, 1.2), w, h, focal=24.0) if cam is None else cam
    tris = np.array([[[-8, -4, 0], [8, -4, 0], [8, 12, 0]], [[-8, -4, 0], [8, 12, 0], [-8, 12, 0]],          # floor
                     [[-1.5, 2.0, 0], [1.2, 2.9, 0], [1.2, 2.9, 2.2]], [[-1.5, 2.0, 0], [1.2, 2.9, 2.2], [-1.5, 2.0, 2.2]]], np.float64)
    return cast(tris, cam, h, w, seed)


def cast(tris, cam, h, w, seed):
    xf = T.proj_xf(cam)
    yy, xx = np.mgrid[0:h, 0:w]
    # the ray through film position (px + 0.5, py + 0.5), from the projection's own constants
    cx = (xx + 0.5) / float(xf["ipx"]) + float(xf["tx"])
    cy = (yy + 0.5) / float(xf["ipy"]) + float(xf["ty"])
    d = (cx[..., None] * xf["right"].astype(np.float64) + cy[..., None] * xf["up"].astype(np.float64)
         + float(xf["focal"]) * xf["fwd"].astype(np.float64))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = xf["pos"].astype(np.float64)
    best_t = np.full((h, w), np.inf)
    surface = np.zeros((h, w, 4), F)
    surface[..., 0] = -1
    normal, position, albedo = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for i, tr in enumerate(tris):
        e0, e1 = tr[1] - tr[0], tr[2] - tr[0]
        pv = np.cross(d, e1)
        det = pv @ e0
        with np.errstate(all="ignore"):
            tv = o - tr[0]
            u = (pv @ tv) / det
            v = (np.cross(tv, e0) @ d.reshape(-1, 3).T).reshape(h, w) / det
            t = (np.cross(tv, e0) @ e1) / det
        hit = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6) & (t < best_t)
        n = np.cross(e0, e1)
        n /= np.linalg.norm(n)
        nf = np.where((d @ n > 0)[..., None], -n, n)
        best_t = np.where(hit, t, best_t)
        surface[hit] = np.stack([np.full((h, w), i), u, v, np.ones((h, w))], -1)[hit].astype(F)
        normal[hit, :3] = nf[hit].astype(F)
        position[hit, :3] = (o + t[..., None] * d)[hit].astype(F)
        position[hit, 3] = t[hit].astype(F)
        albedo[hit] = np.array([0.3 + 0.2 * (i // 2), 0.6, 0.5 - 0.1 * (i // 2), 1], F)

    def film(fseed):
        rng = np.random.default_rng(fseed)
        N = np.exp(rng.uniform(np.log(2), np.log(1e3), (h, w))).round().astype(F)
        mean = np.zeros((h, w, 4), F)
        mean[..., :3] = albedo[..., :3] * F(0.6) + F(0.05) + rng.normal(0, 0.2, (h, w, 3)).astype(F) / np.sqrt(N)[..., None]
        m2 = np.zeros((h, w, 4), F)
        m2[..., :3] = rng.uniform(0.005, 0.2, (h, w, 3)).astype(F) * (N[..., None] - 1)
        m2[..., 3] = N
        return mean, m2

    verts = tris.reshape(-1, 9).astype(F)
    return dict(verts=verts, camera=cam, albedo=albedo, normal=normal, position=position, surface=surface, film=film)


def _step(hist, s, film_seed, verts_prev=None, **kw):
    mean, m2 = s["film"](film_seed)
    return T.step(hist, mean, m2, s["albedo"], s["normal"], s["position"], s["surface"], s["verts"],
                  s["verts"] if verts_prev is None else verts_prev, s["camera"], **kw)


def test_synthetic_scene_has_coverage_background_and_both_surfaces():
    s = synthetic(50, 80, 1)
    cov = s["albedo"][..., 3] > 0
    assert 0.5 < cov.mean() < 0.98
    assert set(np.unique(s["surface"][..., 0]).astype(int)) == {-1, 0, 1, 2, 3}


def test_a_reset_gives_length_one_and_the_current_frame():
    s = synthetic(50, 80, 1)
    mean, m2 = s["film"](3)
    out, hist, info = _step(None, s, 3, denoise={"iterations": 0})
    cov = s["albedo"][..., 3] > 0
    assert np.array_equal(hist["h"], cov.astype(F))
    assert np.array_equal(hist["c"].view(np.uint32), mean[..., :3].view(np.uint32))
    assert info["reprojected"] == 0 and info["reset"] == int(cov.sum()) and not info["mask"].any()


def test_zero_motion_gives_weights_exactly_1_0_0_0():
    s = synthetic(50, 80, 1)
    _, hist, _ = _step(None, s, 3)
    _, hist2, info = _step(hist, s, 4)
    cov = s["albedo"][..., 3] > 0
    took = info["weights"].sum(-1) > 0
    assert took.sum() > 0.9 * cov.sum()
    assert np.array_equal(info["weights"][took], np.tile(np.array([1, 0, 0, 0], F), (int(took.sum()), 1)))
    assert np.array_equal(info["u"], np.mgrid[0:50, 0:80][1].astype(F)) and np.array_equal(info["v"], np.mgrid[0:50, 0:80][0].astype(F))
    assert (hist2["h"][took] == 2).all()
    assert info["mask"].mean() <= T.MASK_CAP


def test_alpha_zero_is_the_arithmetic_mean_of_the_frames():
    s = synthetic(50, 80, 1)
    k = 8
    hist = None
    cs, vs = [], []
    for j in range(k):
        mean, m2 = s["film"](10 + j)
        c0, v0, _ = DR.initial(mean, m2)
        cs.append(c0.astype(np.float64)), vs.append(v0.astype(np.float64))
        _, hist, info = _step(hist, s, 10 + j, temporal={"alpha": 0.0}, denoise={"iterations": 0})
    took = hist["h"] == k
    assert took.sum() > 0.9 * (s["albedo"][..., 3] > 0).sum()
    want_c, want_v = sum(cs) / k, sum(vs) / k ** 2
    # k fp32 updates c += (c_j - c) / j: a few ulps of the values each
    np.testing.assert_allclose(hist["c"][took], want_c[took], rtol=0, atol=k * 4 * 2.0 ** -24 * float(np.abs(want_c).max()))
    np.testing.assert_allclose(hist["v"][took], want_v[took], rtol=k * 4 * 2.0 ** -24, atol=0)


def test_alpha_one_returns_the_current_frame_bit_for_bit():
    s = synthetic(50, 80, 1)
    _, hist, _ = _step(None, s, 3, temporal={"alpha": 1.0})
    mean, m2 = s["film"](4)
    out, hist2, info = _step(hist, s, 4, temporal={"alpha": 1.0})
    c0, v0, _ = DR.initial(mean, m2)
    assert info["reprojected"] > 0
    assert np.array_equal(hist2["c"].view(np.uint32), c0.view(np.uint32)) and np.array_equal(hist2["v"].view(np.uint32), v0.view(np.uint32))
    ref = DR.denoise(mean, m2, s["albedo"], s["normal"], s["position"], DR.theta(s["camera"]))
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert (hist2["h"][info["weights"].sum(-1) > 0] == 2).all()


def test_a_tap_across_the_normal_threshold_never_contributes():
    s = synthetic(50, 80, 1)
    _, hist, _ = _step(None, s, 3)
    turned = hist["normal"].copy()
    wall = s["surface"][..., 0] >= 2
    turned[wall, :3] = np.array([0.6, 0.8, 0], F)  # n . n_prev = 0.6 n.x + 0.8 n.y < 0.9 for the wall's own normal
    assert ((s["normal"][wall, :3] @ np.array([0.6, 0.8, 0], F)) < 0.9).all()
    h2 = dict(hist, normal=turned)
    other = dict(h2, c=np.where(wall[..., None], F(1000), hist["c"]))
    a = _step(h2, s, 4)
    b = _step(other, s, 4)
    assert np.array_equal(a[1]["c"].view(np.uint32), b[1]["c"].view(np.uint32))
    assert (a[1]["h"][wall] == 1).all() and (a[2]["weights"][wall] == 0).all()


def test_an_integer_pixel_shift_moves_the_history_by_that_shift():
    """The history planes rolled by (3, -2) pixels and a motion of exactly (3, -2): every pixel whose tap stays inside the
    image takes the value it takes from the unrolled history under zero motion, bit for bit, with weights (1, 0, 0, 0)."""
    h, w, dx, dy = 40, 64, 3, -2
    s = synthetic(h, w, 2)
    _, hist, _ = _step(None, s, 3)
    roll = lambda a: np.roll(a, (dy, dx), (0, 1))  # noqa: E731
    moved = dict(hist, c=roll(hist["c"]), v=roll(hist["v"]), h=roll(hist["h"]), normal=roll(hist["normal"]), position=roll(hist["position"]))
    mean, m2 = s["film"](4)
    c0, v0, _ = DR.initial(mean, m2)
    args = (c0, v0, s["albedo"], s["normal"], s["surface"], s["verts"], s["verts"], s["camera"])
    c, v, hh, info = T.accumulate(*args, moved, motion=(dx, dy))
    cs, vs, hs, _ = T.accumulate(*args, hist, motion=(0, 0))
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
    assert (hs[inside] == 2).sum() > 0.5 * inside.sum()
    assert np.array_equal(c[inside].view(np.uint32), cs[inside].view(np.uint32))
    assert np.array_equal(v[inside].view(np.uint32), vs[inside].view(np.uint32))
    assert np.array_equal(hh[inside], hs[inside])
    took = inside & (hs == 2)
    assert np.array_equal(info["weights"][took], np.tile(np.array([1, 0, 0, 0], F), (int(took.sum()), 1)))
    assert np.array_equal(info["u"][took], (xx + dx).astype(F)[took]) and np.array_equal(info["v"][took], (yy + dy).astype(F)[took])
    outside = ~inside & (s["albedo"][..., 3] > 0)
    assert (hh[outside] == 1).all()  # the tap left the image: reset


def test_moving_geometry_keeps_the_mask_under_its_cap():
    """the inputs of the GPU comparison (tests/test_temporal_gpu.py (a)): the wall slides, the camera pans; the restatement's
    own near-threshold mask stays under the cap, most pixels reproject and some are disoccluded"""
    for seed in (1, 2):
        a, b = moving_pair(50, 80, seed)
        _, hist, _ = _step(None, a, 3)
        mean, m2 = b["film"](4)
        out, hist2, info = T.step(hist, mean, m2, b["albedo"], b["normal"], b["position"], b["surface"], b["verts"], a["verts"], b["camera"])
        cov = (b["albedo"][..., 3] > 0).sum()
        assert info["mask"].mean() <= T.MASK_CAP, info["mask"].mean()
        assert info["reprojected"] > 0.6 * cov and info["reset"] > 0.02 * cov, (info["reprojected"], info["reset"], cov)
        frac = info["weights"][info["weights"].sum(-1) > 0]
        assert ((frac > 0.05) & (frac < 0.95)).any()  # genuinely bilinear taps


def moving_pair(h, w, seed):
    """frame A and frame B of one scene: in B the wall has slid 0.45 along x and the camera has moved and turned a little"""
    a = synthetic(h, w, seed)
    cam_b = T.make_camera((0.03, 1, -0.27), (0.16, -2.95, 1.22), w, h, focal=24.0)
    tris = a["verts"].reshape(-1, 3, 3).astype(np.float64).copy()
    tris[2:, :, 0] += 0.45
    b = cast(tris, cam_b, h, w, seed)
    return a, b
