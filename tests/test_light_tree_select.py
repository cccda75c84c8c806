"""Light-tree selection against float64 (tests/light_tree_f64.py), host side.  No GPU.

The selection functions are shared by host and device (csrc/light_tree.hpp lt_select / lt_importance, csrc/light_tree_ref.hpp
ltr_select); tests/test_light_tree_select_gpu.py holds the DEVICE compile of them to the float64 twins.  This module runs the
host fp32 compile over the same inputs, which does three jobs: it keeps the twins honest, it measures the
fp32-against-float64 error the device tolerances are derived from, and it checks the exclusion caps without a GPU.

Inputs (shared with the GPU tests): light sets of 2, 3, 17, 64 and 301 mixed point / spot lights (test_light_tree._lights, one
point light made zero-radius), 17-light variants (one light of 100x flux, one of zero intensity, all at one point, all
collinear) and, for DMT_LIGHTS_TREE, a chain of 60 zero-radius lights at x = 2^(i-20) whose tree is 60 levels deep, the
deepest the walk's guard admits.  64 shading points per set (around the lights, within 0.01 of one, exactly at the zero-radius
light, 30x farther out than the lights' spread, normals along and across the direction to the root's centre) x 256 values of u
(one per stratum, the first exactly 0, the last exactly 0.99999994).

Measured on these inputs, host fp32 against float64 (printed by the tests below, which also assert that MODE*_ / CHAIN_*
still hold them; the device is allowed DEVICE_FACTOR = 4 x each because its divide and sqrt are 2.5-ulp operations instead of
0.5-ulp and its products contract):
                                                   worst absolute   worst relative error of a probability
  DMT_LIGHTS_TREE, all sets but the chain          4.18e-6          3.48e-4
  DMT_LIGHTS_TREE, the 60-level chain              2.43e-6          7.43e-3
  DMT_LIGHTS_TREE_REFERENCE                        4.82e-7          1.01e-5
The relative error is taken over probabilities above 2 EPS: a compared case lies more than EPS from both ends of its interval.
The absolute figure of mode 1 is the 2-light set's, whose lights are 0.02 apart (p - centre cancels); the other sets stay below
5.1e-7.  The relative ones come from 1 - p0 with p0 near 1.
Share of cases excluded as too close to a decision (EPS = 1e-6), worst set: mode 1 0.043 % (the chain 0.12 %; cap 0.2 %, expected
2 n EPS); mode 2 0.45 % up to 64 lights (cap 1 %) and 18.7 % at 301 lights (cap 20 %: after several walks with small
probabilities fp32 u has few bits left).  The host compile selects the twin's lights in every compared case.
"""
import ctypes as C

import numpy as np
import pytest

import light_tree_f64 as F64
from test_light_tree import _lights

EPS = 1e-6                    # decisions closer than this (in u, or in the margin's own units) are not compared
DEVICE_FACTOR = 4.0
EXCLUDED_CAP_MODE1 = 0.002
EXCLUDED_CAP_MODE2 = {2: 0.01, 3: 0.01, 17: 0.01, 64: 0.01, 301: 0.20}
# worst host-fp32-against-float64 pmf errors measured by the tests below (they assert that these still hold)
MODE1_ABS, MODE1_REL = 4.2e-6, 3.5e-4
CHAIN_ABS, CHAIN_REL = 2.5e-6, 7.5e-3
MODE2_ABS, MODE2_REL = 4.9e-7, 1.02e-5

POINTS, STRATA = 64, 256
SIZES = [2, 3, 17, 64, 301]
VARIANTS = ["bright", "dark", "same", "line"]
SETS = [f"n{n}" for n in SIZES] + VARIANTS


def _half(x):
    return np.atleast_1d(np.asarray(x, np.float16)).view(np.uint8)


def light_set(pkg, name, chain_yz=(0.0, 0.0)):
    """The packed lights of a set; light 1 (a point light) has radius 0 in all of them but the chain, where every light has
    (chain_yz: the line the chain lies on)."""
    if name == "chain60" or name == "chain61":
        H = pkg.host_scene.load_host_library()
        f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
        out = []
        for i in range(int(name[5:])):
            rec = np.zeros(32, np.uint8)
            H.dmt_host_make_point_light(f3([2.0, 2.0, 2.0]), f3([2.0 ** (i - 20), chain_yz[0], chain_yz[1]]), C.c_float(0.0), rec.ctypes.data_as(C.c_void_p))
            out.append(rec)
        return np.stack(out)
    n = int(name[1:]) if name[0] == "n" and name[1:].isdigit() else 17
    L = _lights(pkg, n, 4000 + n + 10 * SETS.index(name))
    L[1, 20:22] = _half(0.0)                                             # zero radius: a shading point can sit exactly on it
    # ... and a neighbour whose box straddles it in y.  Alone, a zero-radius light is a corner of the box of every node above
    # it, and a point on that corner has len2 == radius2 in exact arithmetic: a tie that rounding decides, outside any margin.
    pos = L[:, 8:20].copy().view(np.float32).reshape(-1, 3)
    pos[2 if n >= 3 else 0] = pos[1] + np.array([0.015, 0.005, 0.012], np.float32)
    L[:, 8:20] = pos.view(np.uint8).reshape(-1, 12)
    if name == "bright":
        L[4, 0:6] = _half(L[4, 0:6].copy().view(np.float16).astype(np.float32) * 100.0)
    if name == "dark":
        L[9, 0:6] = _half([0.0, 0.0, 0.0])
    if name == "same":
        # (light 1 keeps its radius here: a zero-radius light at the root's centre would get importance phi |cos_i| / d^2 from the
        # normals ACROSS the direction to that centre, where cos_i is rounding noise around 0 in any precision)
        L = _lights(pkg, n, 4000 + n + 10 * SETS.index(name))
        L[:, 8:20] = L[1, 8:20]
    if name == "line":
        L[:, 12:20] = L[1, 12:20]
    return L


def positions(L):
    return L[:, 8:20].copy().view(np.float32).reshape(-1, 3).astype(np.float64)


def shading_points(L, seed, exact_lights):
    """64 (point, normal) pairs as float32, see the module's header; six of them exactly at the lights `exact_lights`."""
    rng = np.random.default_rng(seed)
    pos = positions(L)
    lo, hi = pos.min(0), pos.max(0)
    centre, spread = 0.5 * (lo + hi), max(float((hi - lo).max()), 1e-3)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    around = lambda k: centre + rng.uniform(-1.3, 1.3, (k, 3)) * spread
    ring = lambda k: centre + unit(rng.normal(size=(k, 3))) * rng.uniform(2.0, 8.0, (k, 1)) * spread
    near = pos[rng.integers(0, len(pos), 12)] + unit(rng.normal(size=(12, 3))) * rng.uniform(1e-4, 0.01, (12, 1))
    far = centre + unit(rng.normal(size=(12, 3))) * 30.0 * spread
    # [0, 10) around the lights, [10, 22) a few spreads away, [22, 34) near a light, [34, 40) on a light, [40, 52) far,
    # [52, 58) normal along the direction to the root's centre, [58, 64) across it (three around, three a few spreads away each)
    p = np.concatenate([around(10), ring(12), near, pos[exact_lights], far, around(3), ring(3), around(3), ring(3)]).astype(np.float32)
    nrm = unit(rng.normal(size=(POINTS, 3)))
    to_centre = unit(centre - p[52:64].astype(np.float64) + 1e-30)
    nrm[52:58] = to_centre[:6]
    nrm[58:64] = unit(np.cross(to_centre[6:], unit(rng.normal(size=(6, 3)))))
    nrm[34:40] = unit(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [1, 1, 1], [-1, 2, -3]], np.float64))
    assert p.shape == (POINTS, 3)
    return p, nrm.astype(np.float32)


def u_values(seed):
    """One value per stratum of 256, the first exactly 0 and the last exactly 0.99999994, as float32."""
    rng = np.random.default_rng(seed)
    u = ((np.arange(STRATA) + rng.uniform(0.05, 0.95, STRATA)) / STRATA).astype(np.float32)
    u[0], u[-1] = 0.0, np.float32(0.99999994)
    return u


def cases(pkg, name):
    """(lights, p [64,3], n [64,3], u [256]) of a set."""
    L = light_set(pkg, name)
    seed = 77 + sum(map(ord, name))
    p, nrm = shading_points(L, seed, [1, 7, 20, 33, 46, 59] if name.startswith("chain") else [1] * 6)
    return L, p, nrm, u_values(seed + 1)


def flat(p, nrm, u):
    """Every point with every u: (p [k,3], n [k,3], u [k]) with k = 64 x 256, the u of one point adjacent."""
    return np.repeat(p, len(u), 0), np.repeat(nrm, len(u), 0), np.tile(u, len(p))


def errors(got, want, floor=0.0):
    """Worst absolute and relative difference of got against want (float64), over want > floor."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m = want > floor
    if not m.any():
        return 0.0, 0.0
    d = np.abs(got[m] - want[m])
    return float(d.max()), float((d / want[m]).max())


def per_light(part, count):
    """The probability of every light index under a partition [k, count]."""
    light, lo, hi = part
    out = np.zeros((light.shape[0], count))
    for j in range(light.shape[1]):
        ok = light[:, j] >= 0
        out[ok, light[ok, j]] += (hi - lo)[ok, j]
    return out


def mode1_excluded_share(part, u):
    _, _, dist = F64.locate(part, np.tile(u, (part[0].shape[0], 1)))
    return float((dist <= EPS).mean())


# ---- DMT_LIGHTS_TREE ---------------------------------------------------------------------------------------------------------
def _mode1_host_errors(pkg, name):
    L, p, nrm, u = cases(pkg, name)
    nodes, depth = pkg.light_tree_nodes(L, 1)
    part = F64.intervals(nodes, p, nrm)
    want = per_light(part, len(L))
    got = np.stack([pkg.light_tree_pmfs(L, p[i], nrm[i])[0] for i in range(len(p))])
    # the same lights reachable, as far as either side can tell: the twin's interval ends are absolute positions in [0, 1) and
    # lose a length below 2^-53; fp32 forms 1 - p0 and loses a light below half an ulp of 1, and one whose cosine at the shading
    # point is rounding noise; neither matters to a compared case (below)
    assert (got[want == 0] < 2.0 ** -50).all() and (got[want > 2 * EPS] > 0).all(), name
    assert np.abs(want.sum(1) - 1.0).max() < 1e-12                      # the twin's intervals tile [0, 1)
    # a compared case lies more than EPS from both ends of its interval: only lights with more than 2 EPS can be its answer
    return errors(got, want, 2 * EPS), mode1_excluded_share(part, u), depth


def test_mode1_host_pmfs_against_float64(pkg):
    worst_abs = worst_rel = 0.0
    for name in SETS:
        (a, r), share, depth = _mode1_host_errors(pkg, name)
        print(f"mode 1 {name}: depth {depth}, host fp32 vs float64 pmf abs {a:.3e} rel {r:.3e}, excluded {100 * share:.4f} %")
        assert share <= EXCLUDED_CAP_MODE1, (name, share)
        worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
    print(f"mode 1 worst: abs {worst_abs:.3e} rel {worst_rel:.3e}")
    assert worst_abs <= MODE1_ABS and worst_rel <= MODE1_REL, (worst_abs, worst_rel)


def test_mode1_chain_is_60_levels_deep_and_host_pmfs_against_float64(pkg):
    (a, r), share, depth = _mode1_host_errors(pkg, "chain60")
    print(f"mode 1 chain60: depth {depth}, host fp32 vs float64 pmf abs {a:.3e} rel {r:.3e}, excluded {100 * share:.4f} %")
    assert depth == 60 and pkg.light_tree_nodes(light_set(pkg, "chain61"), 1)[1] == 61
    assert share <= EXCLUDED_CAP_MODE1, share
    assert a <= CHAIN_ABS and r <= CHAIN_REL, (a, r)


# ---- DMT_LIGHTS_TREE_REFERENCE -----------------------------------------------------------------------------------------------
def mode2_compare(name, nodes, p, nrm, u, start, got):
    """A selection (indices, pmfs, counts) of the flat cases against the twin: the structural checks on every case, equal
    counts and indices where the decision margin is at least EPS -> (share excluded, worst abs error, worst rel error)."""
    gi, gp, gc = got
    fp, fn, fu = flat(p, nrm, u)
    wi, wp, wc, margin = F64.select(nodes, fp, fn, fu, start)
    slot = np.arange(4)[None, :]
    used = slot < gc[:, None]
    assert gc.min() >= 0 and gc.max() <= 4, name
    assert (gi[~used] == -1).all() and (gp[~used] == 0).all(), name
    assert (gi[used] >= 0).all() and (gi[used] < (len(nodes) + 1) // 2).all(), name
    assert (gp[used] > 0).all() and (gp[used] <= start * (1 + 1e-6)).all(), name
    srt = np.sort(np.where(used, gi, -1 - slot), 1)                     # unused slots made distinct
    assert (srt[:, 1:] != srt[:, :-1]).all(), name                      # the lights of one case are distinct
    sure = margin >= EPS
    same = (gc == wc) & (gi == wi).all(1)
    assert same[sure].all(), (name, int((~same & sure).sum()), np.nonzero(~same & sure)[0][:8], margin[~same & sure][:8])
    both = sure & same
    a, r = errors(gp[both], wp[both])
    return float((~sure).mean()), a, r


def test_mode2_host_selection_against_float64(pkg):
    worst_abs = worst_rel = 0.0
    for name in SETS:
        L, p, nrm, u = cases(pkg, name)
        nodes, depth = pkg.light_tree_nodes(L, 2)
        fp, fn, fu = flat(p, nrm, u)
        for start in (1.0, 0.5):
            gi, gp, gc, count, d = pkg.light_tree_ref_select(L, fp, fn, fu, start)
            assert count == len(nodes) and d == depth
            share, a, r = mode2_compare(name, nodes, p, nrm, u, start, (gi, gp, gc))
            print(f"mode 2 {name} start {start}: depth {depth}, excluded {100 * share:.3f} %, host fp32 vs float64 pmf abs {a:.3e} rel {r:.3e}, "
                  f"lights per case {gc.mean():.2f}")
            assert share <= EXCLUDED_CAP_MODE2.get(len(L), 0.01), (name, share)
            worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
    print(f"mode 2 worst: abs {worst_abs:.3e} rel {worst_rel:.3e}")
    assert worst_abs <= MODE2_ABS and worst_rel <= MODE2_REL, (worst_abs, worst_rel)


# ---- dmt_light_tree_nodes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 17, 64])
def test_light_tree_nodes_round_trip(pkg, n):
    L = light_set(pkg, f"n{n}")
    p, nrm = [0.3, 5.0, 0.1], [0.0, 1.0, 0.0]
    nodes, depth = pkg.light_tree_nodes(L, 1)
    _, count, d = pkg.light_tree_pmfs(L, p, nrm)
    assert len(nodes) == count == 2 * n - 1 and depth == d and nodes.dtype.itemsize == 32
    leaves = nodes["ref"][(nodes["ref"] & F64.LEAF) != 0] & ~np.uint32(F64.LEAF)
    assert sorted(leaves.tolist()) == list(range(n))
    ref, rdepth = pkg.light_tree_nodes(L, 2)
    _, _, _, count, d = pkg.light_tree_ref_select(L, [p], [nrm], [0.5])
    assert len(ref) == count == 2 * n - 1 and rdepth == d and ref.dtype.itemsize == 64
    assert int(ref["numEmitters"][0]) == n
    for mode in (1, 2):
        with pytest.raises(pkg.DmtError, match=f"{2 * n - 1} nodes"):
            pkg.light_tree_nodes(L, mode, cap=2 * n - 2)
        assert len(pkg.light_tree_nodes(L, mode, cap=2 * n + 5)[0]) == 2 * n - 1
