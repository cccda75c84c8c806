"""GPU tests of the acceleration layer's state (csrc/accel_state.hpp, csrc/accel_host.hpp): call orders that reach the same
geometric state give the same bytes -- the static tree's nodes and pair indices, the build, update and motion records
without their measured times, and the film.  Every comparison is of bytes or integers.

Sizes: 1 triangle (one pair with an unused half, three guard copies of the only pair), 3 (an odd count across two pairs),
26 (one level), 777 (several levels: the refit path is live).  Film 32 x 32, 4 spp, bounce cap 4.

The five `<caller>: BVH not built` returns (dmt_render twice, dmt_render_aovs, dmt_test_trace_samples,
dmt_test_closest_hit) cannot be reached through the binding: the only calls that drop the static tree and leave it dropped
are an update or an upload under brute force, where no caller asks for a tree, and dmt_set_accel(BVH) builds eagerly.  So
test_no_route_leaves_bvh_without_a_tree checks that route instead: the tree is gone after a brute-force update, is back
after set_accel(BVH), and the five callers then agree with brute force in every bit."""
import numpy as np
import pytest

from test_bvh_gpu_build_gpu import _soup_for
from test_bvh_refit import deform
from test_bvh_refit_gpu import BUILDERS, DEVICE, HOST, REBUILD, upd  # noqa: F401  (upd: the fixture)
from test_parity_gpu import _rays

pytestmark = pytest.mark.gpu

BRUTE, BVH = 0, 1
RES, SPP, CAP = 32, 4, 4
SIZES = [1, 3, 26, 777]


@pytest.fixture
def acc(upd):  # noqa: F811
    """test_bvh_refit_gpu's fixture (the session's renderer, put back afterwards), and key 1 dropped as well"""
    yield upd
    upd.clear_motion()
    upd.set_shutter(0.0, 1.0)


@pytest.fixture(scope="module")
def look(pkg):
    """materials, lights and a camera at the origin looking at the soups of _soup_for (+y)"""
    s = pkg.host_scene.random_triangle_scene(26, width=RES, height=RES)
    return s.bsdfs, s.lights, s.inf_lights, s.camera


def _dress(r, look):
    r.upload_bsdfs(look[0])
    r.upload_lights(look[1], look[2])
    r.set_camera(look[3])
    r.set_limits(CAP)
    r.set_lens(0.0)
    r.set_shutter(0.0, 1.0)
    r.set_light_sampling(0)
    r.set_bvh_strategy(0, 1 << 22)


def _upload(r, soup):
    r.upload_triangles(*soup, np.zeros(soup[0].size // 4, np.uint32))


def _film(r, accel=None):
    if accel is not None:
        r.set_accel(accel)
    r.film_clear()
    r.render(SPP)
    r.sync()
    mean, m2 = r.download_film()
    assert np.all(m2[..., 3] == SPP)
    return mean.tobytes() + m2.tobytes()


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def _state(r):
    """what the tests compare: the tree, the three records without their measured figures, the film"""
    nodes, pairs = r.download_accel()
    return dict(nodes=nodes.tobytes(), pairs=pairs.tobytes(), build=_without(r.accel_build_info(), "build_ms", "temp_bytes"),
                update=_without(r.accel_update_info(), "update_ms"), motion=_without(r.motion_info(), "tree_build_ms"), film=_film(r))


def _assert_same(got, want, what, keys=("nodes", "pairs", "build", "update", "motion", "film")):
    for k in keys:
        assert got[k] == want[k], f"{what}: {k} differs" + (f": {got[k]} != {want[k]}" if isinstance(got[k], dict) else "")


# ---- (a) the static tree ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_static_tree_does_not_depend_on_the_route(acc, pkg, look, builder, n):
    v1 = _soup_for(pkg, n)
    v0 = deform(v1, 0.3, phase=0.4)
    other = DEVICE if builder == HOST else HOST
    keys = ("nodes", "pairs", "build", "motion", "film")  # the update record tells the routes apart, by design
    with pkg.Renderer(0) as fresh:  # configured first, then one upload
        fresh.set_accel_build(builder)
        fresh.set_accel(BVH)
        _dress(fresh, look)
        _upload(fresh, v1)
        want = _state(fresh)
    assert want["build"] == dict(builder=builder, depth=want["build"]["depth"], triangles=n, nodes=len(want["nodes"]) // 64,
                                 pairs=len(want["pairs"]) // 8)
    assert want["motion"]["keys"] == 1 and want["motion"]["tree_nodes"] == 0
    r = acc
    _dress(r, look)
    # brute force first, both builders visited, then the upload
    r.set_accel(BRUTE), r.set_accel_build(builder)
    _upload(r, v0)
    r.set_accel(BVH), r.set_accel_build(other), r.set_accel_build(builder)
    _upload(r, v1)
    _assert_same(_state(r), want, "upload after switching builders", keys)
    # uploaded and rendered under brute force, the tree built by set_accel
    r.set_accel(BRUTE)
    _upload(r, v1)
    brute = _film(r)
    assert brute == want["film"], "the BVH film is not the brute-force film"
    r.set_accel(BVH)
    _assert_same(_state(r), want, "set_accel after a brute-force render", keys)
    # another soup's tree, replaced by an update in REBUILD mode
    _upload(r, v0)
    r.set_accel_update(REBUILD)
    r.update_vertices(*v1)
    got = _state(r)
    _assert_same(got, want, "update_vertices in REBUILD mode", keys)
    assert got["update"] == dict(action=pkg.BVH_UPDATED_REBUILD, updates_since_build=0, sah_cost=0.0, sah_cost_at_build=0.0,
                                 temp_bytes=got["update"]["temp_bytes"])


# ---- (b) the motion tree ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_motion_tree_does_not_depend_on_the_route(acc, pkg, look, n):
    v1 = _soup_for(pkg, n)
    k, k_other = deform(v1, 0.2, phase=0.9), deform(v1, 0.45, phase=2.2)
    ref = pkg.motion_bvh_validate(*v1, *k)
    assert ref["ok"]
    r = acc
    _dress(r, look)
    r.set_accel_build(HOST)

    def check(what, want):
        got = dict(motion=_without(r.motion_info(), "tree_build_ms"), film=_film(r))
        assert got["motion"]["keys"] == 2
        assert (got["motion"]["tree_nodes"], got["motion"]["tree_pairs"]) == (ref["node_count"], ref["pair_count"]), what
        if want is not None:
            _assert_same(got, want, what, ("motion", "film"))
        return got

    r.set_accel(BRUTE)
    _upload(r, v1)
    r.set_motion(*k)
    assert r.motion_info()["tree_nodes"] == 0  # brute force: no tree yet
    brute = _film(r)
    r.set_accel(BVH)
    want = check("set_motion before set_accel(BVH)", None)
    assert want["film"] == brute, "the BVH motion film is not the brute-force motion film"
    r.set_accel(BRUTE)
    _upload(r, v1)
    r.set_accel(BVH)
    r.set_motion(*k)
    check("set_motion after set_accel(BVH)", want)
    _upload(r, v1)
    r.set_motion(*k_other)
    r.set_motion(*k)
    check("set_motion(K') then set_motion(K)", want)
    r.clear_motion()
    assert _without(r.motion_info(), "open", "close") == dict(keys=1, tree_nodes=0, tree_pairs=0, tree_build_ms=0.0)
    r.set_motion(*k)
    check("set_motion, clear_motion, set_motion", want)
    static_host = r.download_accel()
    r.set_accel_build(DEVICE)  # the static tree is rebuilt by the device builder; the motion tree stays the host builder's
    assert r.accel_build_info()["builder"] == pkg.BVH_BUILT_BY_DEVICE
    dev = pkg.lbvh_reference(*v1)
    nodes, pairs = r.download_accel()
    assert np.array_equal(nodes, dev["nodes"]) and np.array_equal(pairs, dev["pairs"])
    check("set_motion then set_accel_build(device)", want)
    r.set_accel_build(HOST)
    nodes, pairs = r.download_accel()
    assert np.array_equal(nodes, static_host[0]) and np.array_equal(pairs, static_host[1])
    check("and back to the host builder", want)


# ---- (c) clear_motion ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_clear_motion_restores_the_static_state(acc, pkg, look, builder, n):
    v1 = _soup_for(pkg, n)
    r = acc
    _dress(r, look)
    r.set_accel_build(builder)
    r.set_accel(BVH)
    _upload(r, v1)
    before = _state(r)
    r.set_motion(*deform(v1, 0.2, phase=0.9))
    during = _state(r)
    _assert_same(during, before, "the static tree under set_motion", ("nodes", "pairs", "build", "update"))
    assert during["motion"]["keys"] == 2 and during["motion"]["tree_nodes"] > 0
    r.clear_motion()
    _assert_same(_state(r), before, "after clear_motion")


# ---- (d) a refused update --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_refused_update_changes_nothing(acc, pkg, look, builder, n):
    v1 = _soup_for(pkg, n)
    longer = _soup_for(pkg, n + 1)
    r = acc
    _dress(r, look)
    r.set_accel_build(builder)
    r.set_accel(BVH)
    _upload(r, deform(v1, 0.1))
    r.set_accel_update(REBUILD)
    r.update_vertices(*v1)  # an update record that is not the initial one
    r.set_motion(*deform(v1, 0.2, phase=0.9))
    before = _state(r)
    for call in (r.update_vertices, r.set_motion):
        with pytest.raises(pkg.DmtError) as e:
            call(*longer)
        assert "(1)" in str(e.value) and "count differs from the uploaded triangle count" in str(e.value)  # DMT_ERR_INVALID
        _assert_same(_state(r), before, f"after a refused {call.__name__}")


# ---- (e) the callers that ask for the tree ---------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_no_route_leaves_bvh_without_a_tree(acc, pkg, look, n):
    v1 = _soup_for(pkg, n)
    r = acc
    _dress(r, look)
    r.set_accel_build(HOST)
    r.set_accel(BVH)
    _upload(r, deform(v1, 0.1))
    assert r.accel_build_info()["nodes"] > 0
    r.set_accel(BRUTE)
    r.update_vertices(*v1)  # a brute-force update drops the tree, as an upload does
    assert _without(r.accel_build_info(), "builder") == dict(depth=0, triangles=0, nodes=0, pairs=0, build_ms=0.0, temp_bytes=0)
    with pytest.raises(pkg.DmtError) as e:
        r.download_accel()
    assert "(3)" in str(e.value) and "no tree" in str(e.value)  # DMT_ERR_STATE
    px, py = np.meshgrid(np.arange(RES, dtype=np.int32), np.arange(RES, dtype=np.int32))
    px, py, ss = px.ravel(), py.ravel(), (np.arange(RES * RES, dtype=np.int32) % SPP)
    o, d = _rays(2048, n + 1)

    def five(accel):
        out = [_film(r, accel)]
        r.set_bvh_strategy(2, 4096)  # the wavefront launch (brute force ignores the strategy)
        out.append(_film(r))
        r.set_bvh_strategy(0, 1 << 22)
        r.render_aovs(2)
        out.append(b"".join(np.ascontiguousarray(a).tobytes() for a in r.download_aovs()))
        out.append(r.test_trace_samples(px, py, ss).tobytes())
        out.append(b"".join(a.tobytes() for a in r.test_closest_hit(o, d)))
        return out

    brute = five(BRUTE)
    bvh = five(BVH)  # set_accel(BVH) built the tree again
    assert r.accel_build_info()["nodes"] > 0 and r.accel_build_info()["triangles"] == n
    for name, a, b in zip(("dmt_render", "dmt_render (wavefront)", "dmt_render_aovs", "dmt_test_trace_samples", "dmt_test_closest_hit"), bvh, brute):
        assert a == b, f"{name}: BVH differs from brute force"
