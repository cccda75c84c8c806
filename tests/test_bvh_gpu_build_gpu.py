"""GPU tests of the device BVH builder (dmt_set_accel_build(DMT_BVH_BUILD_DEVICE), csrc/bvh_gpu_build.hip).

The pin of its kernels is exact: the downloaded tree equals the serial host restatement (dmt_lbvh_reference) in all 64
bytes of every node and in every pair's indices.  Above that, the traversal contract: boxes only cull, so closest hits
and films under the device-built tree are bit-identical to brute force and to the host-built tree."""
import numpy as np
import pytest

from test_parity_gpu import _random_soup, _rays

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1


@pytest.fixture
def dev(renderer):
    """The session's renderer with the device builder selected; everything is put back afterwards."""
    renderer.set_accel_build(DEVICE)
    yield renderer
    renderer.set_accel(0)
    renderer.set_accel_build(HOST)
    renderer.set_bvh_strategy(0, 1 << 22)
    renderer.clear_envmap()


def _soup_for(pkg, n):
    if n == 1_000_000:                                   # BASELINE config 4's scene
        s = pkg.host_scene.random_triangle_scene(n, width=1024, height=1024)
        return s.xs, s.ys, s.zs
    xs, ys, zs = _random_soup(n, n)
    if n == 777:                                         # 377 duplicates: equal Morton codes, ordered by index
        xs[400:] = xs[:377]; ys[400:] = ys[:377]; zs[400:] = zs[:377]
    return xs, ys, zs


def _assert_tree_is_the_restatement(pkg, r, xs, ys, zs):
    nodes, pairs = r.download_accel()
    ref = pkg.lbvh_reference(xs, ys, zs)
    assert not ref["abandoned"]
    info = r.accel_build_info()
    assert info["builder"] == pkg.BVH_BUILT_BY_DEVICE
    assert (info["nodes"], info["pairs"], info["depth"]) == (ref["nodes"].shape[0], ref["pairs"].shape[0], ref["depth"])
    assert np.array_equal(pairs, ref["pairs"])
    if not np.array_equal(nodes, ref["nodes"]):
        bad = np.flatnonzero((nodes != ref["nodes"]).any(axis=1))
        raise AssertionError(f"{bad.size} of {nodes.shape[0]} nodes differ, first {bad[:8]}: device {nodes[bad[0]].tolist()} "
                             f"restatement {ref['nodes'][bad[0]].tolist()}")
    c = pkg.bvh_check(nodes, pairs, xs, ys, zs)
    assert c["ok"] and c["max_leaf"] <= 2 and c["depth"] == info["depth"], c
    return info, c


@pytest.mark.parametrize("n", [1, 2, 3, 5, 26, 777, 20000, 1_000_000])
def test_device_tree_equals_host_restatement(dev, pkg, n):
    xs, ys, zs = _soup_for(pkg, n)
    dev.upload_triangles(xs, ys, zs, np.zeros(n, np.uint32))
    dev.set_accel(1)
    info, _ = _assert_tree_is_the_restatement(pkg, dev, xs, ys, zs)
    assert info["triangles"] == n and info["build_ms"] > 0 and info["temp_bytes"] > 0


def test_empty_soup(dev, pkg):
    z = np.zeros((0, 4), np.float32)
    dev.upload_triangles(z, z, z, np.zeros(0, np.uint32))
    dev.set_accel(1)
    nodes, pairs = dev.download_accel()
    ref = pkg.lbvh_reference(z, z, z)
    assert nodes.shape == (1, 64) and pairs.shape[0] == 0 and np.array_equal(nodes, ref["nodes"])


def test_rebuilds_reuse_their_temporaries(dev, pkg):
    """Built twice in one context with a different soup of the SAME size in between: every temporary (keys, links, boxes,
    arrival counters) is reused with warm caches, so a box or a counter left over from the build before, or a sibling's
    box read stale in the bottom-up pass, shows as a difference from the restatement."""
    n = 300_000
    a, b = _random_soup(n, 41), _random_soup(n, 42, spread=5.0, size=0.2)
    dev.set_accel(1)
    for xs, ys, zs in (a, b, a, b):
        dev.upload_triangles(xs, ys, zs, np.zeros(n, np.uint32))
        _assert_tree_is_the_restatement(pkg, dev, xs, ys, zs)


@pytest.mark.parametrize("ntri", [1, 5, 26, 777, 20000])
def test_closest_hit_equals_brute_force(dev, O, pkg, ntri):
    xs, ys, zs = _soup_for(pkg, ntri)
    dev.upload_triangles(xs, ys, zs, np.zeros(ntri, np.uint32))
    o, d = _rays(8192, ntri + 1)
    dev.set_accel(0)
    bi, bt = dev.test_closest_hit(o, d)
    dev.set_accel(1)
    assert dev.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
    ai, at = dev.test_closest_hit(o, d)
    assert np.array_equal(ai, bi)
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32))
    oi, ot = O.closest_hit(xs, ys, zs, o[:2048], d[:2048])
    assert (ai[:2048] != oi).sum() <= 1
    if ntri >= 777:
        assert (ai >= 0).mean() > 0.02
    if ntri == 777:
        assert ai.max() < 400 or (ai[ai >= 377] < 400).all()          # duplicates resolve to the lowest original index


def test_empty_slots_axis_parallel_rays(dev, pkg):
    """test_bvh_empty_slots_axis_parallel_rays under the device-built tree: the guard pairs behind the array."""
    def tri(p0, p1, p2):
        return [p0[0], p1[0], p2[0], 0.0], [p0[1], p1[1], p2[1], 0.0], [p0[2], p1[2], p2[2], 0.0]
    for nfloor in (1, 2, 3):
        t = [tri((-1, 0, -1), (1, 0, -1), (1, 0, 1)), tri((-1, 0, -1), (1, 0, 1), (-1, 0, 1)), tri((2, 0, 2), (3, 0, 2), (3, 0, 3))][:nfloor]
        xs = np.array([a[0] for a in t], np.float32).reshape(-1); ys = np.array([a[1] for a in t], np.float32).reshape(-1)
        zs = np.array([a[2] for a in t], np.float32).reshape(-1)
        dev.upload_triangles(xs, ys, zs, np.zeros(nfloor, np.uint32))
        g = np.linspace(-1.5, 3.5, 41, dtype=np.float32)
        gx, gz = np.meshgrid(g, g)
        n = gx.size
        o = np.stack([gx.ravel(), np.full(n, 5.0, np.float32), gz.ravel()], axis=1).astype(np.float32)
        d = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (n, 1))
        o = np.concatenate([o, o * np.array([1, -1, 1], np.float32), np.stack([np.full(n, -9.0, np.float32), gz.ravel() * 0, gx.ravel()], axis=1)])
        d = np.concatenate([d, -d, np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))])
        dev.set_accel(0)
        bi, bt = dev.test_closest_hit(o, d)
        dev.set_accel(1)
        assert dev.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
        ai, at = dev.test_closest_hit(o, d)
        assert np.array_equal(ai, bi) and np.array_equal(at.view(np.uint32), bt.view(np.uint32))
        assert (ai >= 0).sum() > 100


def _films(r, spp, modes=(0, 1), region=None):
    out = []
    for mode in modes:
        r.set_accel(mode)
        r.film_clear()
        r.render(spp, region=region)
        r.sync()
        out.append(r.download_film())
    return out


def _assert_same_film(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0][..., :3].max() > 0


def test_films_bit_identical_to_brute_force(dev, pkg):
    for scene, spp in ((pkg.host_scene.cornell_box(64, 64), 16), (pkg.host_scene.random_triangle_scene(4000, width=48, height=48), 4)):
        dev.upload_scene(scene)
        dev.set_limits(8)
        brute, bvh = _films(dev, spp)
        assert dev.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
        _assert_same_film(brute, bvh)


def test_env_map_and_area_light_rows(dev, pkg, O):
    """One env-map scene and one emissive-triangle scene: the BVH rows of those kernels under the device-built tree."""
    dev.upload_scene(pkg.host_scene.sphere_envmap_scene(96, 96, lat=8, lon=16, env_height=16))
    dev.set_limits(8)
    _assert_same_film(*_films(dev, 8))
    dev.clear_envmap()
    sc = O.cornell_box(72, 72)
    for a in (sc.xs, sc.ys, sc.zs):
        a[[0, 1, 16, 17]] = a[[0, 1, 16, 17]][:, [0, 2, 1, 3]]
    sc.set_area_lights([0, 1, 16, 17, 20, 21], [[6, 6, 5], [6, 6, 5], [12, 14, 20], [12, 14, 20], [20, 15, 10], [20, 15, 10]])
    try:
        dev.upload_scene(sc)
        dev.set_limits(6)
        _assert_same_film(*_films(dev, 8))
        assert dev.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
    finally:
        dev.upload_area_lights([], np.zeros((0, 3), np.float32))


def test_wavefront_strategy(dev, pkg):
    dev.upload_scene(pkg.host_scene.random_triangle_scene(6000, width=200, height=136))
    dev.set_limits(8)
    dev.set_accel(1)
    dev.set_bvh_strategy(2, 20000)
    brute, wavefront = _films(dev, 12, region=(3, 5, 197, 131))
    _assert_same_film(brute, wavefront)


def test_million_triangles_records_and_build_time(dev, pkg, O):
    """The 1 M-triangle scene: films under the device-built tree equal the films under the HOST-built tree on the two
    windows of test_bvh_million_triangles (bit-identical by the contract; brute force would cost 2e11 triangle tests),
    the 32 rays of that test agree with the CPU closest hit, the build records name their builders, and -- the reason
    the feature exists -- the second device build is faster than the second host build, both measured here."""
    scene = pkg.host_scene.random_triangle_scene(1_000_000, width=1024, height=1024)
    dev.set_accel_build(HOST)
    dev.upload_scene(scene)
    dev.set_limits(8)
    dev.set_accel(1)
    regions = ((480, 480, 544, 544), (3, 950, 67, 1014))
    host_films = [_films(dev, 4, modes=(1,), region=reg)[0] for reg in regions]
    v = pkg.bvh_validate(scene.xs, scene.ys, scene.zs)
    rec = dev.accel_build_info()
    assert rec["builder"] == pkg.BVH_BUILT_BY_HOST
    assert (rec["nodes"], rec["depth"], rec["triangles"]) == (v["node_count"], v["depth"], 1_000_000)
    nodes, pairs = dev.download_accel()                   # the factored-out walk on the host builder's tree agrees with dmt_bvh_validate
    c = pkg.bvh_check(nodes, pairs, scene.xs, scene.ys, scene.zs)
    assert (c["ok"], c["node_count"], c["depth"], c["max_leaf"]) == (v["ok"], v["node_count"], v["depth"], v["max_leaf"])
    assert rec["pairs"] == pairs.shape[0]
    host_cost = c["sah_cost"]

    dev.set_accel_build(DEVICE)                           # rebuilt at once
    rec = dev.accel_build_info()
    assert rec["builder"] == pkg.BVH_BUILT_BY_DEVICE
    nodes, pairs = dev.download_accel()
    assert (rec["nodes"], rec["pairs"]) == (nodes.shape[0], pairs.shape[0])
    c = pkg.bvh_check(nodes, pairs, scene.xs, scene.ys, scene.zs)
    assert c["ok"] and c["depth"] == rec["depth"]
    print(f"SAH cost: host {host_cost:.1f}, device {c['sah_cost']:.1f}, ratio {c['sah_cost'] / host_cost:.3f}")
    for reg, hf in zip(regions, host_films):
        df = _films(dev, 4, modes=(1,), region=reg)[0]
        _assert_same_film(hf, df)
        x0, y0, x1, y1 = reg
        assert np.all(df[1][y0:y1, x0:x1, 3] == 4) and df[1][..., 3].sum() == 4 * 64 * 64
    o, d = _rays(32, 99)
    o[:] = 0
    ai, at = dev.test_closest_hit(o, d)
    oi, ot = O.closest_hit(scene.xs, scene.ys, scene.zs, o, d)
    assert np.array_equal(ai, oi)

    # second build of each kind
    dev.set_accel_build(HOST)
    host_ms = dev.accel_build_info()["build_ms"]
    assert dev.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_HOST
    dev.set_accel_build(DEVICE)
    rec = dev.accel_build_info()
    assert rec["builder"] == pkg.BVH_BUILT_BY_DEVICE
    print(f"1 M triangles: host build {host_ms:.1f} ms, device build {rec['build_ms']:.2f} ms, {rec['temp_bytes'] / 1e6:.0f} MB of temporaries")
    assert rec["build_ms"] < host_ms


def test_a_fresh_context_reports_the_host_builder(pkg):
    xs, ys, zs = _random_soup(500, 500)
    with pkg.Renderer(0) as r:
        assert r.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_HOST and r.accel_build_info()["nodes"] == 0
        r.upload_triangles(xs, ys, zs, np.zeros(500, np.uint32))
        r.set_accel(1)
        rec = r.accel_build_info()
        v = pkg.bvh_validate(xs, ys, zs)
        assert rec["builder"] == pkg.BVH_BUILT_BY_HOST and (rec["nodes"], rec["depth"]) == (v["node_count"], v["depth"])
        assert rec["temp_bytes"] == 0
        with pytest.raises(pkg.DmtError):
            r.set_accel_build(2)
        r.set_accel_build(DEVICE)                          # rebuilt at once, as dmt_set_accel does
        assert r.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
        r.upload_triangles(xs[:100], ys[:100], zs[:100], np.zeros(100, np.uint32))   # uploads honour the mode
        rec = r.accel_build_info()
        assert rec["builder"] == pkg.BVH_BUILT_BY_DEVICE and rec["triangles"] == 100
