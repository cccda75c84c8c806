"""The box bound in its centre / half-width form where its arithmetic is thin: a scene 1000 units from the
origin and rays that start 64 scene extents away.  There o * (1 / d) is large next to the t of a hit, and its rounding is what
the bound's E term has to cover.  Closest hits and films must stay what the plain loop over every triangle gives, bit for
bit (DMT_BRUTE_CULL=0 turns every cluster off, =1 keeps the sphere clusters, =2 both kinds)."""
import ctypes as C

import numpy as np
import pytest

from test_brute_cull_box_gpu import _ctx, _wall_rays

pytestmark = pytest.mark.gpu

SHIFT = np.array([1000.0, -1000.0, 1000.0], np.float32)


def _translated_cornell(pkg, res):
    """Cornell with soup and camera moved by SHIFT, lit by one point light at the middle of the moved room."""
    s = pkg.host_scene.cornell_box(res, res)
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4).copy() for a in (s.xs, s.ys, s.zs))
    for a, t in zip((xs, ys, zs), SHIFT):
        a[:, :3] += t
    cam = s.camera.copy()
    cam[12:24] = (cam[12:24].view(np.float32) + SHIFT).view(np.uint8)
    mid = np.array([0.5 * (a[:, :3].min() + a[:, :3].max()) for a in (xs, ys, zs)], np.float32)
    H = pkg.host_scene.load_host_library()
    f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
    light = np.zeros(32, np.uint8)
    H.dmt_host_make_point_light(f3([4, 4, 4]), f3(mid), C.c_float(0.01), light.ctypes.data_as(C.c_void_p))
    return pkg.host_scene.ArrayScene(xs, ys, zs, s.mat_id, s.bsdfs, light[None], s.inf_lights[:0], cam)


def _closest(pkg, monkeypatch, s, o, d):
    out = {}
    for mode in (0, 2):
        r = _ctx(pkg, monkeypatch, mode)
        try:
            r.upload_scene(s)
            out[mode] = r.test_closest_hit(o, d)
        finally:
            r.close()
    return out


@pytest.mark.parametrize("case", ["translated", "far_camera"])
def test_closest_hit_bit_equal_far_from_the_origin(pkg, monkeypatch, case):
    """About 64 K rays at the walls: edges and corners, origins on and beside the surfaces, grazing, axis-parallel and on
    the inflated boxes' faces (the ray families of tests/test_brute_cull_box_gpu.py)."""
    s = _translated_cornell(pkg, 64) if case == "translated" else pkg.host_scene.cornell_box(64, 64)
    boxes = pkg.binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id)
    assert [(f, c) for f, c, _, _ in boxes] == [(16, 2), (18, 2), (20, 2), (22, 2), (24, 2)]
    o, d = _wall_rays(s, boxes, 66_000, 31 if case == "translated" else 32)
    if case == "far_camera":
        # the same lines, started up to 64 scene extents back: an axis-parallel ray keeps its exact coordinates on the
        # other axes, so the on-face rays stay on their faces
        v = np.stack([np.asarray(a, np.float64).reshape(-1, 4)[:, :3].ravel() for a in (s.xs, s.ys, s.zs)], axis=-1)
        ext = float((v.max(0) - v.min(0)).max())
        back = np.random.default_rng(33).choice([64.0, 64.0, 16.0, 1.0], (o.shape[0], 1)) * ext
        o = (o.astype(np.float64) - back * d.astype(np.float64)).astype(np.float32)
    assert 60_000 <= o.shape[0] <= 70_000
    out = _closest(pkg, monkeypatch, s, o, d)
    i0, t0 = out[0]
    i2, t2 = out[2]
    assert ((i0 >= 16) & (i0 < 26)).mean() > 0.3          # the rays do reach the walls
    assert np.array_equal(i0, i2)
    assert np.array_equal(t0.view(np.uint32), t2.view(np.uint32))


def _film(pkg, monkeypatch, mode, scene, spp, env, table):
    r = _ctx(pkg, monkeypatch, mode)
    try:
        r.upload_scene(scene)
        if env:
            r.upload_envmap(pkg.host_scene.synthetic_sky(64))
        r.set_sampler_table(table)
        r.set_limits(8)
        r.film_clear()
        r.render(spp)
        return r.download_film()
    finally:
        r.close()


@pytest.mark.parametrize("table", ["table_off", "table_forced"])
@pytest.mark.parametrize("env", ["plain", "env"])
@pytest.mark.parametrize("case", ["cornell_64", "translated_32"])
def test_films_byte_equal_across_cull_modes(pkg, monkeypatch, case, env, table):
    s = pkg.host_scene.cornell_box(64, 64) if case == "cornell_64" else _translated_cornell(pkg, 32)
    tmode = pkg.binding.SAMPLER_TABLE_OFF if table == "table_off" else pkg.binding.SAMPLER_TABLE_FORCE
    films = [_film(pkg, monkeypatch, mode, s, 16, env == "env", tmode) for mode in (0, 1, 2)]
    ref = films[0]
    assert np.isfinite(ref[0]).all() and (ref[0][..., :3] > 0).mean() > 0.5
    for f in films[1:]:
        assert ref[0].tobytes() == f[0].tobytes()
        assert ref[1].tobytes() == f[1].tobytes()
