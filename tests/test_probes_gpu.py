"""GPU tests of the probes' staging (csrc/probe_stage.hpp, csrc/probes.hpp): every array-taking dmt_test_* entry point runs
the first n of one fixed set of cases, n = one lane, one full block, and one lane into a second block; case i of every output
must be byte-equal for every n that includes it.  The code is compared with itself at another size, so there is no tolerance:
a wrong element count, stride, byte count or grid in the staging shows as a difference or as stale bytes.

dmt_test_trace_log has no other test; it is compared with the oracle's log here."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 65)                 # probes launched in blocks of 64
SIZES_256 = SIZES + (256, 257)      # probes launched in blocks of 256
N, N_256 = max(SIZES), max(SIZES_256)


def same_at_every_size(run, sizes):
    """run(n) -> the outputs (arrays of n rows) of the probe over the first n cases"""
    full = run(max(sizes))
    for n in sizes[:-1]:
        part = run(n)
        assert len(part) == len(full)
        for k, (a, b) in enumerate(zip(part, full)):
            assert a.shape[0] == n and b.shape[0] == max(sizes), (n, k, a.shape, b.shape)
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b[:n]).tobytes(), f"output {k} differs at n = {n}"
    return full


@pytest.fixture(scope="module")
def cornell():
    g = golden("cornell_scene.npz")
    sc = SimpleNamespace(**{k: g[k] for k in g.files})
    sc.width, sc.height = (int(v) for v in sc.camera[24:32].view(np.int32))
    return sc


@pytest.fixture(scope="module")
def cases(cornell):
    rng = np.random.default_rng(65)
    c = SimpleNamespace()
    c.px, c.py = rng.integers(0, cornell.width, N).astype(np.int32), rng.integers(0, cornell.height, N).astype(np.int32)
    c.s = rng.integers(0, 64, N).astype(np.int32)
    c.u2 = rng.random((N, 2), dtype=np.float32)
    d = rng.normal(size=(N, 3))
    c.dir = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    c.points = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    c.bu = rng.uniform(0.02, 0.6, N).astype(np.float32)
    c.bv = (rng.uniform(0.02, 0.9, N) * (1 - c.bu)).astype(np.float32)
    return c


@pytest.fixture()
def scene(renderer, cornell):
    """the golden Cornell box uploaded, brute force, no textures, no env map; the same after the test"""
    def plain():
        renderer.set_accel(0)
        renderer.set_partition(0, 1)
        renderer.set_limits(32)
        renderer.upload_scene(cornell)
    plain()
    yield cornell
    plain()


# ---- probes without a scene --------------------------------------------------------------------------------------------
def test_half_staging(renderer):
    rng = np.random.default_rng(1)
    f = (rng.standard_normal(N_256) * 100).astype(np.float32)
    h = rng.integers(0, 65536, N_256).astype(np.uint16)
    same_at_every_size(lambda n: renderer.test_half(floats=f[:n], halves=h[:n]), SIZES_256)
    # one direction only: the absent output stays untouched (None in, None out)
    ho, fo = renderer.test_half(floats=f)
    both = renderer.test_half(floats=f, halves=h)
    assert fo is None and np.array_equal(ho, both[0])
    ho, fo = renderer.test_half(halves=h)
    assert ho is None and fo.tobytes() == both[1].tobytes()


def test_triangle_intersect_staging(renderer):
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, (N_256, 1, 3)) * 0.3 + rng.uniform(-0.5, 0.5, (N_256, 3, 3))
    xs, ys, zs = (np.zeros((N_256, 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    o, d = np.array([0.05, -3.0, 0.1], np.float32), np.array([0.0, 1.0, 0.0], np.float32)
    full = same_at_every_size(lambda n: renderer.test_triangle_intersect(xs[:n], ys[:n], zs[:n], o, d), SIZES_256)
    assert 0 < full[0].sum() < N_256                       # hits and misses
    # the optional outputs left out (null): only the hit flags come back
    hit = np.full(N_256, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = renderer._lib.dmt_test_triangle_intersect(renderer._ctx, p(xs), p(ys), p(zs), C.c_size_t(N_256), p(o), p(d), p(hit), None, None,
                                                   None, None)
    assert rc == 0 and np.array_equal(hit, full[0])


def test_sampler_staging(renderer, cases):
    c = cases
    same_at_every_size(lambda n: renderer.test_sampler(100, 300, c.px[:n] % 100, c.py[:n], c.s[:n], 9), SIZES)
    hi, p2, dims = renderer.test_sampler(100, 300, c.px % 100, c.py, c.s, 0)     # no dimensions asked for: nothing copied
    assert dims.shape == (N, 0) and hi.shape == (N,)


def test_sampler_table_staging(renderer):
    """a 1 x 1 frame: one table entry per sample, so n samples are n lanes of the fill kernel's 256-lane blocks"""
    same_at_every_size(lambda n: renderer.test_sampler_table(1, 1, 3, n), SIZES_256)
    same_at_every_size(lambda n: renderer.test_sampler_table(5, 13, 3, n), (1, 2))       # 65 entries per sample


def test_bsdf_staging(renderer, O):
    import shading_sweep as S
    rec = S.plain_bsdf_records(O)["diel_a03"]
    x = S.bsdf_inputs(1)
    pick = np.arange(N) * (x["ns"].shape[0] // N)             # across the generator's cells
    a = {k: x[k][pick] for k in ("ns", "ng", "wo", "u2", "uc", "wi")}
    ng = same_at_every_size(lambda n: renderer.test_bsdf_ng(rec, a["ns"][:n], a["ng"][:n], a["wo"][:n], a["u2"][:n], a["uc"][:n], a["wi"][:n]), SIZES)
    plain = same_at_every_size(lambda n: renderer.test_bsdf(rec, a["ns"][:n], a["wo"][:n], a["u2"][:n], a["uc"][:n], a["wi"][:n]), SIZES)
    assert any(p.tobytes() != g.tobytes() for p, g in zip(plain, ng))       # the geometric normal is used when it is given


def test_light_staging(renderer, O, cases):
    import shading_sweep as S
    rec = S.light_specs(O)["spot_wide"][0]
    rng = np.random.default_rng(3)
    pos = S._shell(rng, N, 1.0, 3.0).astype(np.float32)
    hadt = (rng.random(N) < 0.25).astype(np.int32)
    same_at_every_size(lambda n: (renderer.test_light(rec, pos[:n], cases.dir[:n], cases.u2[:n], hadt[:n]),), SIZES)


# ---- probes of the uploaded scene --------------------------------------------------------------------------------------
def test_envmap_staging(renderer, scene, cases):
    from test_parity_gpu import _envmap
    renderer.upload_envmap(_envmap(16), np.array([0.2, -0.1, 0.3, 0.9], np.float32))
    try:
        keys = ("wi", "pdf", "uv", "Le", "ok", "Le_dir", "pdf_dir")

        def run(n):
            g = renderer.test_envmap(cases.u2[:n], cases.dir[:n])
            return tuple(g[k] for k in keys)
        same_at_every_size(run, SIZES)
    finally:
        renderer.clear_envmap()


@pytest.mark.parametrize("mode", [1, 2])
def test_light_tree_staging(renderer, pkg, scene, cases, mode):
    from test_light_tree_select import light_set
    renderer.upload_lights(light_set(pkg, "n17"), [])
    renderer.set_light_sampling(mode)
    try:
        pos = cases.points * 3.0 + np.array([0.0, 6.0, 0.0], np.float32)
        full = same_at_every_size(lambda n: renderer.test_light_tree(pos[:n], cases.dir[:n], cases.u2[:n, 0]), SIZES)
        assert full[2].max() >= 1
    finally:
        renderer.set_light_sampling(0)


def test_camera_staging(renderer, scene, cases):
    c = cases
    same_at_every_size(lambda n: renderer.test_camera_rays(c.px[:n], c.py[:n], c.s[:n]), SIZES)
    same_at_every_size(lambda n: renderer.test_camera_project(c.points[:n]), SIZES)


@pytest.mark.parametrize("accel", [0, 1], ids=["brute", "bvh"])
def test_trace_staging(renderer, scene, cases, accel):
    c = cases
    o, d = renderer.test_camera_rays(c.px, c.py, c.s)
    renderer.set_accel(accel)
    tri, t = same_at_every_size(lambda n: renderer.test_closest_hit(o[:n], d[:n]), SIZES)
    assert (tri >= 0).all() and (tri < scene.xs.shape[0]).all()          # the box is closed around the camera's view
    renderer.set_limits(6)
    (L,) = same_at_every_size(lambda n: (renderer.test_trace_samples(c.px[:n], c.py[:n], c.s[:n]),), SIZES)
    assert np.isfinite(L).all() and (L > 0).any()


def test_material_and_texture_filter_staging(renderer, O, scene, cases):
    import shading_sweep as S
    sc = S.textured_cornell(O)
    rng = np.random.default_rng(4)
    tri = rng.integers(0, sc.tri_count, N).astype(np.int32)
    tex = rng.integers(0, 3, N).astype(np.int32)
    depth = (np.arange(N) % 2).astype(np.int32)
    ng = S.triangle_normals(sc)[tri]
    c = cases
    renderer.upload_scene(sc)
    rec = same_at_every_size(lambda n: renderer.test_material(tri[:n], c.bu[:n], c.bv[:n], ng[:n]), SIZES)[0]
    assert len({r.tobytes() for r in rec}) > 4                          # the patch differs from hit to hit
    same_at_every_size(lambda n: renderer.test_texture_filter(tri[:n], c.bu[:n], c.bv[:n], tex[:n], depth[:n]), SIZES)


# ---- dmt_test_trace_log against the oracle -----------------------------------------------------------------------------
def test_trace_log_vs_oracle(renderer, O, scene):
    """The per-bounce log of single paths of the Cornell box, depth cap 4 (up to the depth cap of 8 device and oracle differ
    at float-rounding level, test_parity_gpu's module docstring).  Everything discrete -- record count, triangle, depth,
    sampler dimension -- is exact; positions within test_triangle_intersect_random_soup's tolerance for hit positions of
    general rays (rel 1e-4, abs 1e-5); throughput and radiance within test_path_radiance_samples' (rel 1e-3, abs 1e-5).
    A shorter capacity returns the first records of the same log."""
    g = golden("path_samples.npz")
    osc = O.Scene(scene.xs, scene.ys, scene.zs, scene.mat_id, scene.bsdfs, scene.lights, scene.inf_lights, scene.camera)
    renderer.set_limits(4)
    bounces = 0
    for px, py, s in zip(g["px"][:8] % scene.width, g["py"][:8] % scene.height, g["s"][:8]):
        rec, L = renderer.test_trace_log(px, py, s)
        orec, oL = O.trace_log(osc, px, py, s, max_depth=4)
        assert rec.shape == orec.shape and 1 <= rec.shape[0] <= 5, (px, py, s, rec.shape, orec.shape)
        assert np.array_equal(rec[:, [0, 10, 11]], orec[:, [0, 10, 11]]), (px, py, s)
        assert np.allclose(rec[:, 1:4], orec[:, 1:4], rtol=1e-4, atol=1e-5), (px, py, s)
        assert np.allclose(rec[:, 4:10], orec[:, 4:10], rtol=1e-3, atol=1e-5), (px, py, s)
        assert np.allclose(L, oL, rtol=1e-3, atol=1e-5), (px, py, s)
        for cap in (1, 2):
            short, Ls = renderer.test_trace_log(px, py, s, cap=cap)
            assert short.tobytes() == rec[:cap].tobytes() and Ls.tobytes() == L.tobytes()
        bounces += rec.shape[0]
    assert bounces > 8                                                   # paths that bounce, not only first hits
