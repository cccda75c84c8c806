"""Light-tree selection on the DEVICE (dmt_test_light_tree: lt_select / ltr_select as the *_ltree / *_ltree2 kernels compile
them, on the tree the context uploaded) against the float64 twins of tests/light_tree_f64.py.

Inputs, exclusion rule and caps are those of tests/test_light_tree_select.py, which runs the host fp32 compile over them: 64
shading points x 256 values of u per light set.  A case is compared unless its decision is closer than EPS = 1e-6 to a tie
(mode 1: u within EPS of a boundary between two float64 intervals; mode 2: the twin's decision margin below EPS); compared
cases must select exactly the twin's lights.  The pmf bounds are DEVICE_FACTOR = 4 x the worst host-fp32-against-float64
errors measured there (the device's divide and sqrt are 2.5-ulp operations instead of 0.5-ulp, and its products contract):

                               measured, host fp32       bound, device
                               absolute    relative      absolute    relative
  DMT_LIGHTS_TREE              4.18e-6     3.48e-4       1.68e-5     1.4e-3
    the 60-level chain         2.43e-6     7.43e-3       1.0e-5      3.0e-2
  DMT_LIGHTS_TREE_REFERENCE    4.82e-7     1.01e-5       1.96e-6     4.08e-5

(the relative error is taken over probabilities above 2 EPS, the only ones a compared case can have; the absolute and the
relative bound both hold).  Share of cases excluded, measured: mode 1 at most 0.043 % per set (0.12 % on the chain; cap 0.2 %);
mode 2 at most 0.45 % per set up to 64 lights (cap 1 %) and 18.7 % at 301 lights (cap 20 %).
"""
import ctypes as C

import numpy as np
import pytest

import light_tree_f64 as F64
import test_light_tree_select as T

pytestmark = pytest.mark.gpu


@pytest.fixture
def lit(renderer, O):
    """The session's context with a plain scene under it (no textures, emissive triangles or blend materials, which would keep the
    uniform pick); uniform light sampling again afterwards."""
    renderer.upload_scene(O.cornell_box(16, 16))
    renderer.upload_textures(None, None, None, None)
    renderer.upload_area_lights([], np.zeros((0, 3), np.float32))
    renderer.clear_envmap()
    yield renderer
    renderer.set_light_sampling(0)


def probe(r, p, nrm, u, start=1.0):
    return r.test_light_tree(*T.flat(p, nrm, u), start)


def check_mode1(name, nodes, p, nrm, u, got, abs_bound, rel_bound, start=1.0):
    """A device selection of the flat cases of a set against the float64 partition of its tree."""
    gi, gp, gc = got
    part = F64.intervals(nodes, p, nrm)
    light, prob, dist = F64.locate(part, np.tile(u, (len(p), 1)))
    light, prob, dist = light.reshape(-1), prob.reshape(-1), dist.reshape(-1)
    assert ((gc == 0) | (gc == 1)).all() and (gi[:, 1:] == -1).all() and (gp[:, 1:] == 0).all(), name
    chosen = np.where(gc == 1, gi[:, 0], -1)
    assert ((gc == 1) == (gi[:, 0] >= 0)).all() and (chosen < (len(nodes) + 1) // 2).all(), name
    assert (gp[gc == 1, 0] > 0).all() and (gp[gc == 1, 0] <= start).all() and (gp[gc == 0, 0] == 0).all(), name
    sure = dist > T.EPS
    share = float((~sure).mean())
    wrong = sure & (chosen != light)
    print(f"mode 1 {name}: excluded {100 * share:.4f} %, compared cases with another light than float64's: {int(wrong.sum())}")
    assert share <= T.EXCLUDED_CAP_MODE1, (name, share)
    assert not wrong.any(), (name, int(wrong.sum()), np.nonzero(wrong)[0][:8], chosen[wrong][:8], light[wrong][:8], dist[wrong][:8])
    both = sure & (light >= 0)
    a, _ = T.errors(gp[both, 0], start * prob[both])
    _, r = T.errors(gp[both, 0], start * prob[both], start * 2 * T.EPS)
    print(f"mode 1 {name}: device vs float64 pmf abs {a:.3e} (bound {abs_bound:.3e}) rel {r:.3e} (bound {rel_bound:.3e})")
    assert a <= abs_bound and r <= rel_bound, (name, a, r)


def check_strata(name, got):
    """On the device's output alone (start pmf 1): over the 256 strata of a point, a light of probability q is chosen by
    256 q +- 2 values of u, and every case that chose it reports the same q."""
    gi, gp, gc = got
    chosen = np.where(gc == 1, gi[:, 0], -1).reshape(T.POINTS, T.STRATA)
    pmf = gp[:, 0].reshape(T.POINTS, T.STRATA)
    for j in range(T.POINTS):
        for light in np.unique(chosen[j][chosen[j] >= 0]):
            m = chosen[j] == light
            q = pmf[j][m]
            assert (q == q[0]).all(), (name, j, light)
            assert abs(int(m.sum()) - T.STRATA * float(q[0])) <= 2.0, (name, j, int(light), int(m.sum()), float(q[0]))


@pytest.mark.parametrize("name", T.SETS + ["chain60"])
def test_mode1_device_selection_against_float64(lit, pkg, name):
    L, p, nrm, u = T.cases(pkg, name)
    nodes, depth = pkg.light_tree_nodes(L, 1)
    assert depth <= 60
    lit.upload_lights(L, [])
    lit.set_light_sampling(1)
    got = probe(lit, p, nrm, u)
    chain = name == "chain60"
    bounds = [T.DEVICE_FACTOR * x for x in ((T.CHAIN_ABS, T.CHAIN_REL) if chain else (T.MODE1_ABS, T.MODE1_REL))]
    check_mode1(name, nodes, p, nrm, u, got, *bounds)
    check_strata(name, got)
    half = probe(lit, p, nrm, u, 0.5)
    assert np.array_equal(half[0], got[0]) and np.array_equal(half[2], got[2])
    assert np.array_equal(half[1], 0.5 * got[1])                        # exactly: a power of two


@pytest.mark.parametrize("name", T.SETS)
def test_mode2_device_selection_against_float64(lit, pkg, name):
    L, p, nrm, u = T.cases(pkg, name)
    nodes, depth = pkg.light_tree_nodes(L, 2)
    lit.upload_lights(L, [])
    lit.set_light_sampling(2)
    for start in (1.0, 0.5):
        got = probe(lit, p, nrm, u, start)
        share, a, r = T.mode2_compare(name, nodes, p, nrm, u, start, got)
        print(f"mode 2 {name} start {start}: excluded {100 * share:.3f} %, device vs float64 pmf abs {a:.3e} "
              f"(bound {T.DEVICE_FACTOR * T.MODE2_ABS:.3e}) rel {r:.3e} (bound {T.DEVICE_FACTOR * T.MODE2_REL:.3e})")
        assert share <= T.EXCLUDED_CAP_MODE2.get(len(L), 0.01), (name, share)
        assert a <= T.DEVICE_FACTOR * T.MODE2_ABS and r <= T.DEVICE_FACTOR * T.MODE2_REL, (name, start, a, r)


def test_probe_follows_the_uploaded_lights_and_the_mode(lit, pkg):
    """The tree the probe walks is rebuilt after dmt_upload_lights and after dmt_set_light_sampling switches between the modes."""
    A, pa, na, u = T.cases(pkg, "n17")
    B, pb, nb, _ = T.cases(pkg, "n64")
    lit.upload_lights(A, [])
    lit.set_light_sampling(1)
    check_mode1("n17", pkg.light_tree_nodes(A, 1)[0], pa, na, u, probe(lit, pa, na, u), T.DEVICE_FACTOR * T.MODE1_ABS, T.DEVICE_FACTOR * T.MODE1_REL)
    lit.upload_lights(B, [])
    got = probe(lit, pb, nb, u)
    assert got[0].max() >= 17                                           # lights the first list does not have
    check_mode1("n64", pkg.light_tree_nodes(B, 1)[0], pb, nb, u, got, T.DEVICE_FACTOR * T.MODE1_ABS, T.DEVICE_FACTOR * T.MODE1_REL)
    lit.set_light_sampling(2)
    got2 = probe(lit, pb, nb, u)
    assert got2[2].max() > 1                                            # cuts of several lights: the other tree
    T.mode2_compare("n64", pkg.light_tree_nodes(B, 2)[0], pb, nb, u, 1.0, got2)
    lit.set_light_sampling(1)
    again = probe(lit, pb, nb, u)
    assert all(np.array_equal(x, y) for x, y in zip(again, got))


def test_probe_is_refused_where_no_tree_applies(lit, pkg):
    L, p, nrm, u = T.cases(pkg, "n17")
    lit.upload_lights(L, [])
    lit.set_light_sampling(0)
    with pytest.raises(pkg.DmtError, match="uniformly"):
        probe(lit, p, nrm, u)
    for mode in (1, 2):
        lit.set_light_sampling(mode)
        lit.upload_lights(L[:1], [])
        with pytest.raises(pkg.DmtError, match="more than one light"):
            probe(lit, p, nrm, u)
        H = pkg.host_scene.load_host_library()
        f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
        distant = np.zeros(32, np.uint8)
        H.dmt_host_make_directional_light(f3([0.4, 0.4, 0.3]), f3([0.2, 0.6, -0.7]), C.c_float(0.0), distant.ctypes.data_as(C.c_void_p))
        lit.upload_lights(np.concatenate([L, distant[None]]), [])
        with pytest.raises(pkg.DmtError, match="keeps the uniform pick"):
            probe(lit, p, nrm, u)
        lit.upload_lights(L, [])
        assert probe(lit, p, nrm, u)[2].max() >= 1                      # and answers again once a tree applies


# ---- the fall-back for trees deeper than the walk's guard --------------------------------------------------------------------
def _chain_film(r, O, pkg, count, mode):
    sc = O.cornell_box(32, 32)
    sc.lights = T.light_set(pkg, f"chain{count}", chain_yz=(2.0, 0.5))   # the near end of the chain is inside the box
    r.upload_scene(sc)
    r.set_limits(4)
    r.set_accel(0)
    r.set_partition(0, 1)
    r.set_light_sampling(mode)
    r.film_clear()
    r.render(8)
    r.sync()
    return r.download_film()


def test_a_tree_deeper_than_the_guard_falls_back_to_the_uniform_pick(lit, pkg, O):
    """61 zero-radius lights at x = 2^(i-20) make a tree of 61 levels, one more than lt_select's walk admits: the context
    renders with the uniform pick (bit-identical films), says so through dmt_last_error, and the probe has no tree to walk.
    With 60 lights the tree is used."""
    L = T.light_set(pkg, "chain61", chain_yz=(2.0, 0.5))
    assert pkg.light_tree_nodes(L, 1)[1] == 61
    uniform = _chain_film(lit, O, pkg, 61, 0)
    deep = _chain_film(lit, O, pkg, 61, 1)
    assert "uniform pick" in lit.last_error() and "61" in lit.last_error()
    assert np.array_equal(uniform[0], deep[0]) and np.array_equal(uniform[1], deep[1])
    assert float(deep[0][..., :3].mean()) > 1e-3                        # not black
    _, p, nrm, u = T.cases(pkg, "chain60")
    with pytest.raises(pkg.DmtError, match="too deep"):
        probe(lit, p, nrm, u)
    uniform = _chain_film(lit, O, pkg, 60, 0)
    tree = _chain_film(lit, O, pkg, 60, 1)
    assert probe(lit, p, nrm, u)[2].max() == 1
    assert np.isfinite(tree[0]).all() and not np.array_equal(uniform[0], tree[0])
