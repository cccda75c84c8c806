"""First-hit texture filtering (DMT_TEXFILTER_REFERENCE), the parts that need no GPU: the MIP chain and
the camera footprint of the library against the numpy restatement (texfilter_ref.py), the EWA weight table, the mode
switch, and one restatement row per [fix]."""
import re

import numpy as np
import pytest

import texfilter_ref as R
from conftest import GOLDEN, ROOT


def _img(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


@pytest.mark.parametrize("w, h", [(16, 16), (64, 64), (64, 4), (1, 32), (24, 10)])
def test_mip_chain_equals_restatement(pkg, w, h):
    img = _img(w, h, w * 1000 + h)
    levels, chain = pkg.texture_mip_chain(img)
    ref = R.mip_chain(img)
    assert levels == len(ref) == R.mip_level_count(w, h)
    n, a, b = 0, w, h  # the reference's loop (core-texture.cu:360-366)
    while a > 0 or b > 0:
        n, a, b = n + 1, a >> 1, b >> 1
    assert levels == n
    assert len(chain) == levels - 1
    for l, (got, want) in enumerate(zip(chain, ref[1:]), start=1):
        assert got.shape == (max(1, h >> l), max(1, w >> l), 4)
        assert np.array_equal(got, want), f"level {l}"


def test_mip_chain_box_average_by_hand(pkg):
    """2x2 -> 1x1: 0.25 (c00 + c10 + c01 + c11) in float, truncated; 1x2 -> 1x1 ([fix 1]): 0.5 (c0 + c1)."""
    img = np.array([[[10, 0, 255, 1], [11, 0, 255, 2]], [[12, 1, 255, 3], [14, 2, 0, 4]]], np.uint8)
    _, chain = pkg.texture_mip_chain(img)
    assert chain[0][0, 0].tolist() == [11, 0, 191, 2]
    _, chain = pkg.texture_mip_chain(np.array([[[3, 200, 0, 0]], [[4, 101, 0, 0]]], np.uint8))
    assert chain[0][0, 0].tolist() == [3, 150, 0, 0]


def _cameras(O, pkg):
    cams = []
    for w, h, spp in [(64, 64, 16), (200, 120, 256)]:
        sc = O.cornell_box(w, h)
        sc.camera[32:36] = np.array([spp], np.int32).view(np.uint8)
        cams.append(("cornell", sc.camera.copy()))
    st = pkg.host_scene.load_json(GOLDEN / "scene_test" / "scene_test.json")
    for w, h, spp in [(256, 256, 32), (96, 160, 100)]:
        cam = np.array(st.camera, np.uint8).reshape(44).copy()
        cam[24:36] = np.array([w, h, spp], np.int32).view(np.uint8)
        cams.append(("scene_test", cam))
    return cams


def test_footprint_equals_restatement(O, pkg):
    for name, cam44 in _cameras(O, pkg):
        got = pkg.texture_footprint(cam44)
        want = R.footprint(R.parse_camera(cam44))
        spp = R.parse_camera(cam44)["spp"]
        assert got["spp_scale"] == np.float32(max(0.125, 1 / np.sqrt(spp)))
        for k in ("cfr", "min_dx", "min_dy", "spp_scale"):
            a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), (name, k, a, b)
        # the smallest differentials are about one pixel's angle, and not zero
        assert 0 < np.linalg.norm(got["min_dx"]) < 0.1 and 0 < np.linalg.norm(got["min_dy"]) < 0.1


def test_restated_camera_rays_agree_with_oracle(O, pkg):
    for name, cam44 in _cameras(O, pkg):
        cam = R.parse_camera(cam44)
        sc = O.cornell_box(cam["width"], cam["height"])
        sc.camera[:] = cam44
        rng = np.random.default_rng(2)
        px, py = rng.integers(0, cam["width"], 64), rng.integers(0, cam["height"], 64)
        ss = rng.integers(0, 64, 64)
        o, d = O.camera_rays(sc, px, py, ss)
        for i in range(64):
            x, y = R.raster_of_direction(cam, d[i])
            assert px[i] - 1e-3 <= x <= px[i] + 1 + 1e-3 and py[i] - 1e-3 <= y <= py[i] + 1 + 1e-3, (name, i, x, y)
            ro, rd = R.generate_ray(cam, x, y)
            assert np.abs(rd - d[i]).max() < 1e-5 and np.abs(ro - o[i]).max() < 1e-5


def test_ewa_lut_formula_and_include():
    lut = R.ewa_lut()
    i = np.arange(128)
    assert np.allclose(lut, np.exp(-2.0 * i / 127) - np.exp(-2.0), rtol=0, atol=1e-7)
    assert lut[127] == 0 and np.all(np.diff(lut) < 0)
    text = (ROOT / "include" / "dmt_ewa_lut.inc").read_text()
    vals = np.array([float(v) for v in re.findall(r"([-+0-9.e]+)f", text.split("DMT_EWA_LUT_VALUES", 1)[1])], np.float32)
    assert np.array_equal(vals, lut)


def test_set_texture_filter_rejects_unknown_mode(pkg):
    try:
        r = pkg.Renderer(0)
    except pkg.DmtError as e:
        pytest.skip(f"no context without a GPU: {e}")
    with r:
        r.set_texture_filter(pkg.TEXFILTER_REFERENCE)
        r.set_texture_filter(pkg.TEXFILTER_LEVEL0)
        for bad in (2, -1, 7):
            with pytest.raises(pkg.DmtError):
                r.set_texture_filter(bad)


def test_mip_chain_rejects_bad_arguments(pkg):
    lib = pkg.load_library()
    import ctypes as C
    n = C.c_int()
    img = _img(8, 8, 1)
    assert lib.dmt_texture_mip_chain(img.ctypes.data_as(C.c_void_p), 8, 8, None, C.c_uint64(0), C.byref(n)) != 0  # no room
    assert lib.dmt_texture_mip_chain(None, 8, 8, None, C.c_uint64(0), C.byref(n)) != 0
    assert lib.dmt_texture_mip_chain(img.ctypes.data_as(C.c_void_p), 0, 8, None, C.c_uint64(0), C.byref(n)) != 0
    one = _img(1, 1, 2)
    assert lib.dmt_texture_mip_chain(one.ctypes.data_as(C.c_void_p), 1, 1, None, C.c_uint64(0), C.byref(n)) == 0 and n.value == 1


# ---- one restatement row per [fix] -------------------------------------------------------------------------------------
def _checker(n=64):
    yy, xx = np.mgrid[0:n, 0:n]
    c = (((xx + yy) % 2) * 255).astype(np.uint8)
    return R.mip_chain(np.stack([c, c, c, np.full_like(c, 255)], -1))


def test_fix1_non_square_levels_average_what_exists():
    levels = R.mip_chain(_img(8, 2, 3))
    assert [l.shape[:2] for l in levels] == [(2, 8), (1, 4), (1, 2), (1, 1)]
    parent = levels[1].astype(np.float32) / np.float32(255)
    want = ((np.float32(0.5) * (parent[0, 0] + parent[0, 1])) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(levels[2][0, 0], want)


def test_fix2_second_level_past_the_end_reads_the_last():
    levels = _checker()
    r = R.lookup(levels, 0.3, 0.7, (50.0, 20.0, -40.0, 60.0))   # rho far beyond the chain
    assert r["branch"] == 1 and r["lod"] > len(levels) and np.isfinite(r["rgb"]).all()
    assert np.allclose(r["rgb"], levels[-1][0, 0, :3] / 255.0, atol=1e-6)


def test_fix3_zero_length_shorter_axis_is_isotropic():
    levels = _checker()
    r = R.lookup(levels, 0.3, 0.7, (0.05, 0.0, 0.0, 0.0))   # dst1 = 0, dst0 != 0: 0 * inf in the clamp
    assert r["branch"] == 1 and np.isfinite(r["rgb"]).all()


def test_fix4_grazing_ellipse_is_bounded():
    levels = _checker(256)
    d = (0.9, 1e-9, 1e-4, 0.0)   # 230 texels along u per pixel, the minor axis almost 0: level 0, a box of thousands
    w = levels[0].shape[1]
    lam = R.lod_minor(d, w, w)
    assert lam == 0
    b0 = R.ewa_box(w, w, 0.4, 0.6, np.array([0.9, 1e-4], np.float32), np.array([1e-9 * 8 * 1e4, 0], np.float32))
    r = R.lookup(levels, 0.4, 0.6, d)
    assert r["branch"] == 3 and np.isfinite(r["rgb"]).all()
    il = int(r["lod"])
    lh, lw = levels[il].shape[:2]
    dx, dy = np.array([0.9, 1e-4], np.float32), np.array([1e-9, 0.0], np.float32)
    d1 = dy * (np.sqrt(np.float32(dx @ dx)) / (np.sqrt(np.float32(dy @ dy)) * np.float32(8)))
    assert R.ewa_box(lw, lh, 0.4, 0.6, dx, d1)["count"] <= R.EWA_MAX_TEXELS
    assert R.ewa_box(w, w, 0.4, 0.6, dx, d1)["count"] > R.EWA_MAX_TEXELS
    assert b0["count"] > 0


def test_fix5_zero_uv_determinant_gives_level_zero():
    fp = dict(cfr=np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0]], np.float32), min_dx=np.array([1e-3, 0, 0], np.float32),
              min_dy=np.array([0, 1e-3, 0], np.float32), spp_scale=np.float32(1), rfc_rot=np.array([1, 0, 0, 0, 0, 1, 0, 1, 0], np.float32))
    p0, p1, p2 = np.array([[-1, 5, -1]], np.float32), np.array([[1, 5, -1]], np.float32), np.array([[0, 5, 1]], np.float32)
    p = (p0 + p1 + p2) / 3
    ng = np.array([[0, -1, 0]], np.float32)
    good = np.array([[0, 0, 1, 0, 0.5, 1]], np.float32)
    flat = np.array([[0, 0, 1, 1, 2, 2]], np.float32)   # collinear UVs: det == 0
    d, margin = R.hit_differentials(fp, p, ng, p0, p1, p2, good)
    assert np.any(d != 0) and margin[0] > 1
    d, _ = R.hit_differentials(fp, p, ng, p0, p1, p2, flat)
    assert np.all(d == 0)
    levels = _checker()
    assert R.lookup(levels, 0.3, 0.3, d[0])["branch"] == 0
