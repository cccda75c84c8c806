"""The emitter tree (csrc/emitter_tree.hpp; dmt_set_emitter_sampling) on the host: structure of the built tree, probabilities,
selection against float64 (tests/emitter_tree_f64.py), and the too-deep report.  No GPU; tests/test_emitter_tree_gpu.py holds
the DEVICE compile of et_select / et_pmf to the same twin over the same inputs.

Inputs (shared with the GPU tests): sets of 1, 2, 3, 17, 64 and 301 mixed emitters -- about a quarter point / spot lights of
radius 2e-4, the rest one-sided emissive triangles of mixed size, orientation and radiance, in a soup whose first two triangles
are not emissive -- and variants of the 17-emitter set: one triangle 100x brighter, one zero-radiance and one zero-area
triangle, all triangles in one plane with one normal, all triangles identical (the builder's median fall-back), all centroids
on one line.  64 shading points per set, placed as tests/test_light_tree_select.py places them around the emitters' centroids
(six of them exactly at emitter 1, a light), x 256 values of u (one per stratum, the first exactly 0, the last exactly
0.99999994).  The coplanar set has eight more points BEHIND its plane, for the probabilities only.

Measured on these inputs, host fp32 against float64 (printed below; HOST_ABS / HOST_REL are asserted to still hold them; the
device is allowed DEVICE_FACTOR = 4 x each, the project's rule, see tests/test_light_tree_select_gpu.py):
  worst absolute error of a probability                  1.853e-6   (the set with one triangle 100x brighter; the others stay below 5e-7)
  worst relative error, over probabilities above 2 EPS   4.254e-5   (the same set)
Share of cases excluded as within EPS = 1e-6 of a decision (an interval end in u, or the bounding-sphere test of a node on
the walk): worst set 0.37 % (the 17-emitter set with the dark triangles; 0.36 % at 64 emitters), cap 1 % per set.  The host
compile selects the twin's emitter in every compared case, and
pmf_by_trail equals pmf bit for bit in every case that selected one.

Probabilities.  An emitter "provably out of reach" is one the BOUND excludes: a triangle whose plane through its box centre has
the point behind it by more than the box's bounding radius (theta_w - theta_b >= pi / 2); a point just behind a triangle's plane
is inside that bound and may get a probability, as with pbrt's bounds.  The probabilities sum to 1 except for the share of u for
which the walk ends at a node whose children both have no importance although the node's wider bound has: there et_select
returns no emitter, as pbrt's walk does, and the test asserts sum + that share = 1 (the twin measures the share).
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import emitter_tree_f64 as F64
import test_light_tree_select as TLS

EPS = F64.EPS
DEVICE_FACTOR = 4.0
EXCLUDED_CAP = 0.01
HOST_ABS, HOST_REL = 1.9e-6, 4.3e-5           # worst host-fp32-against-float64 pmf errors measured below (asserted to still hold)
POINTS, STRATA = TLS.POINTS, TLS.STRATA
SIZES = [1, 2, 3, 17, 64, 301]
VARIANTS = ["bright", "dark", "coplanar", "same", "line"]
SETS = [f"n{n}" for n in SIZES] + VARIANTS
GUARD = F64.MAX_DEPTH


class Scene:
    """lights [k,32] packed, the soup xs / ys / zs (4 floats per triangle and axis, as dmt_upload_triangles), the emissive list."""

    def __init__(self, lights, verts, area_tri, area_le):
        self.lights = np.ascontiguousarray(lights, np.uint8).reshape(-1, 32)
        v = np.asarray(verts, np.float32).reshape(-1, 3, 3)               # [triangle, corner, xyz]
        soa = np.zeros((3, len(v), 4), np.float32)
        soa[:, :, :3] = v.transpose(2, 0, 1)
        self.verts, self.xs, self.ys, self.zs = v, soa[0].reshape(-1).copy(), soa[1].reshape(-1).copy(), soa[2].reshape(-1).copy()
        self.area_tri = np.ascontiguousarray(area_tri, np.uint32)
        self.area_le = np.ascontiguousarray(area_le, np.float32).reshape(-1, 3)
        self.count = len(self.lights) + len(self.area_tri)

    def args(self):
        return self.lights, self.xs, self.ys, self.zs, self.area_tri, self.area_le

    def light_positions(self):
        return self.lights[:, 8:20].copy().view(np.float32).reshape(-1, 3).astype(np.float64)

    def centroids(self):
        """Box centre of every emitter, in emitter order (lights, then the emissive triangles)."""
        t = self.verts[self.area_tri].astype(np.float64)
        return np.concatenate([self.light_positions(), 0.5 * (t.min(1) + t.max(1))])

    def planes(self):
        """(unit normal, box centre, half diagonal) of every emissive triangle; normal 0 for a zero-area one."""
        t = self.verts[self.area_tri].astype(np.float64)
        c = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        length = np.linalg.norm(c, axis=1, keepdims=True)
        return c / np.where(length > 0, length, 1.0), 0.5 * (t.min(1) + t.max(1)), 0.5 * np.linalg.norm(t.max(1) - t.min(1), axis=1)


def make_lights(pkg, n, rng, radius=2e-4, positions=None):
    H = pkg.host_scene.load_host_library()
    f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        pos = rng.uniform(-3.0, 3.0, 3) + [0, 6, 0] if positions is None else positions[i]
        col = rng.uniform(0.05, 6.0, 3)
        rec = out[i]
        if i % 3 == 2:
            H.dmt_host_make_spot_light(f3(col), f3(pos), f3([0, 0, -1]), C.c_float(0.9), C.c_float(0.7), C.c_float(radius), rec.ctypes.data_as(C.c_void_p))
        else:
            H.dmt_host_make_point_light(f3(col), f3(pos), C.c_float(radius), rec.ctypes.data_as(C.c_void_p))
    return out


def emitter_set(pkg, name):
    n = int(name[1:]) if name[0] == "n" and name[1:].isdigit() else 17
    rng = np.random.default_rng(9000 + n + 10 * SETS.index(name))
    k = 0 if n == 1 else max(1, n // 4)                                  # lights; emitter 1 is a light from n = 8 on, emitter 0 from n = 2 on
    m = n - k
    lights = make_lights(pkg, k, rng)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    centre = rng.uniform(-3.0, 3.0, (m, 3)) + [0, 6, 0]
    e0, e1 = unit(rng.normal(size=(m, 3))), unit(rng.normal(size=(m, 3)))
    size = rng.uniform(0.05, 0.4, (m, 1))
    le = rng.uniform(0.5, 20.0, (m, 3))
    if name == "coplanar":                                               # in the plane y = 6, all facing down
        centre[:, 1] = 6.0
        e0, e1 = unit(e0 * [1, 0, 1]), unit(e1 * [1, 0, 1])
    if name == "line":
        centre[:, 1:] = centre[0, 1:]
    tris = np.stack([centre - size * (e0 + e1) / 3, centre + size * (2 * e0 - e1) / 3, centre + size * (2 * e1 - e0) / 3], 1)
    if name == "coplanar":
        up = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])[:, 1] > 0
        tris[up] = tris[up][:, [0, 2, 1]]
    if name == "same":
        tris[:] = tris[0]
    if name == "bright":
        le[3] *= 100.0
    if name == "dark":
        le[2] = 0.0
        tris[5, 2] = tris[5, 1]                                          # zero area
    floor = np.array([[[-5, 0, -5], [5, 0, -5], [5, 0, 5]], [[-5, 0, -5], [5, 0, 5], [-5, 0, 5]]], np.float64)   # not emissive
    return Scene(lights, np.concatenate([floor, tris]), 2 + np.arange(m), le)


def cases(pkg, name):
    """(scene, p [64,3], n [64,3], u [256]) of a set."""
    S = emitter_set(pkg, name)
    fake = np.zeros((S.count, 32), np.uint8)                             # shading_points reads the positions of a light list
    fake[:, 8:20] = S.centroids().astype(np.float32).view(np.uint8).reshape(-1, 12)
    seed = 177 + sum(map(ord, name))
    p, nrm = TLS.shading_points(fake, seed, [min(1, S.count - 1)] * 6)
    return S, p, nrm, TLS.u_values(seed + 1)


def behind_points(S):
    """Eight points above the coplanar set's plane (its triangles face down), at least 1 away, normals facing the plane."""
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(-3, 3, (8, 1)), rng.uniform(7.0, 12.0, (8, 1)), rng.uniform(-3, 3, (8, 1))], 1).astype(np.float32)
    return p, np.tile(np.array([[0, -1, 0]], np.float32), (8, 1))


def compare(name, part, u, got, start=1.0):
    """A selection (index, pmf, pmf_by_trail) of the flat cases (every point with every u) against the twin's partition: the
    twin's emitter in every case further than EPS from a decision, pmf_by_trail == pmf bit for bit -> (share excluded, worst
    abs error, worst rel error of the compared probabilities above 2 EPS)."""
    gi, gp, gt = (np.asarray(x).reshape(part[0].shape[0], len(u)) for x in got)
    wi, wp, dist, margin = F64.locate(part, np.tile(u, (part[0].shape[0], 1)))
    picked = gi >= 0
    assert np.array_equal(gp[picked].view(np.uint32), gt[picked].view(np.uint32)), name
    assert (gp[~picked] == 0).all() and (gt[~picked] == 0).all() and (gp[picked] > 0).all() and (gp <= start * (1 + 1e-6)).all(), name
    sure = (dist > EPS) & (margin >= EPS)
    same = gi == wi
    assert same[sure].all(), (name, int((~same & sure).sum()), np.argwhere(~same & sure)[:8], dist[~same & sure][:8], margin[~same & sure][:8])
    both = sure & same & (wi >= 0)
    a, r = TLS.errors(gp[both] / start, wp[both], 2 * EPS)
    a = max(a, TLS.errors(gp[both] / start, wp[both])[0])
    return float((~sure).mean()), a, r


def check_strata(name, got):
    """On the selection's output alone (start pmf 1), as test_light_tree_select_gpu.check_strata: over the 256 strata of a
    point, an emitter of probability q is chosen by 256 q +- 2 values of u, and every case that chose it reports the same q."""
    chosen, pmf = (np.asarray(x).reshape(POINTS, STRATA) for x in got[:2])
    for j in range(POINTS):
        for e in np.unique(chosen[j][chosen[j] >= 0]):
            m = chosen[j] == e
            q = pmf[j][m]
            assert (q == q[0]).all(), (name, j, e)
            assert abs(int(m.sum()) - STRATA * float(q[0])) <= 2.0, (name, j, int(e), int(m.sum()), float(q[0]))


# ---- 1. structure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_structure(pkg, name):
    S = emitter_set(pkg, name)
    nodes, trails, lengths, depth = pkg.emitter_tree_nodes(*S.args())
    assert nodes.dtype.itemsize == 48 and len(trails) == len(lengths) == S.count
    assert F64.check_structure(nodes, trails, lengths, S.count, GUARD) == depth
    assert depth <= 2 * int(np.ceil(np.log2(max(S.count, 2)))) + 6, depth
    if S.count > 1:
        with pytest.raises(pkg.DmtError, match=f"{2 * S.count - 1} nodes"):
            pkg.emitter_tree_nodes(*S.args(), cap=2 * S.count - 2)
    # leaves: a triangle's axis is its unit normal with cos theta_o = 1, a light's cone is the sphere; flux as the header says
    ref = nodes["ref"]
    leaf = (ref & F64.LEAF) != 0
    normal, _, _ = S.planes()
    for at in np.nonzero(leaf)[0]:
        e = int(ref[at] & (F64.LEAF - 1))
        if e < len(S.lights):
            assert nodes["cosO"][at] == -1.0 and nodes["phi"][at] > 0
        else:
            t = e - len(S.lights)
            tri = S.verts[S.area_tri[t]].astype(np.float64)
            area = 0.5 * np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
            want = np.pi * float(S.area_le[t] @ [0.2126, 0.7152, 0.0722]) * area
            assert nodes["cosO"][at] == 1.0 and abs(nodes["phi"][at] - want) <= 1e-5 * want + 1e-30
            if area > 0:
                assert np.abs(nodes["axis"][at] - normal[t]).max() < 1e-5
    if name == "dark":
        assert (nodes["phi"][leaf] == 0).sum() == 2


def test_a_20000_triangle_grid_builds(pkg):
    g = 100
    x, z = np.meshgrid(np.arange(g, dtype=np.float64), np.arange(g, dtype=np.float64), indexing="ij")
    o = np.stack([x.ravel(), np.full(g * g, 3.0), z.ravel()], 1) * 0.1
    a, b, c = o, o + [0.1, 0, 0], o + [0, 0, 0.1]
    d = o + [0.1, 0, 0.1]
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    S = Scene(np.zeros((0, 32), np.uint8), tris, np.arange(len(tris)), np.full((len(tris), 3), 2.0))
    nodes, trails, lengths, depth = pkg.emitter_tree_nodes(*S.args())
    assert len(nodes) == 2 * 20000 - 1 and depth <= 40
    ref = nodes["ref"]
    assert sorted((ref[(ref & F64.LEAF) != 0] & (F64.LEAF - 1)).tolist()) == list(range(20000))
    assert pkg.emitter_tree_pmfs(*S.args(), [5.0, 1.0, 5.0], [0.0, 1.0, 0.0]).sum() == 0      # above the grid, which faces down
    pm = pkg.emitter_tree_pmfs(*S.args(), [5.0, -1.0, 5.0], [0.0, 1.0, 0.0])
    assert abs(float(pm.astype(np.float64).sum()) - 1.0) < 1e-4 and (pm >= 0).all()


# ---- 2. probabilities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_probabilities(pkg, name):
    S, p, nrm, _ = cases(pkg, name)
    if name == "coplanar":
        bp, bn = behind_points(S)
        p, nrm = np.concatenate([p, bp]), np.concatenate([nrm, bn])
    nodes = pkg.emitter_tree_nodes(*S.args())[0]
    part = F64.intervals(nodes, p, nrm)
    want = F64.per_emitter(part, S.count)
    # the share of [0, 1) for which the walk ends at a node whose two children both have no importance at p although the node
    # itself has: its bound is the union's, wider than either child's.  et_select returns -1 there (no NEE sample at this
    # vertex, as pbrt's walk does) and no emitter owns that share, so the probabilities sum to 1 - none, not to 1
    none = np.where(part[0] < 0, part[2] - part[1], 0.0).sum(1)
    normal, centre, radius = S.planes()
    k = len(S.lights)
    for i in range(len(p)):
        pm = pkg.emitter_tree_pmfs(*S.args(), p[i], nrm[i]).astype(np.float64)
        assert (pm >= 0).all() and np.isfinite(pm).all()
        # provably out of reach: behind the triangle's plane through its box centre by more than the box's bounding radius, which
        # is where the bound itself (theta_w - theta_b >= pi / 2) says so
        out = ((p[i].astype(np.float64) - centre) * normal).sum(1) < -radius * (1 + 1e-4) - 1e-6
        assert (pm[k:][out] == 0).all(), (name, i)
        assert (pm[k:][(S.area_le.max(1) == 0) | (np.abs(normal).max(1) == 0)] == 0).all()
        assert abs(pm.sum() + none[i] - 1.0) < 1e-5, (name, i, pm.sum(), none[i])   # 1 wherever no walk can end short of a leaf
        assert np.abs(pm - want[i]).max() < 1e-5
    if name == "coplanar":
        assert (want[64:, k:] == 0).all() and np.abs(want[64:, :k].sum(1) + none[64:] - 1.0).max() < 1e-12   # behind the plane: the lights only


# ---- 3. selection against float64 --------------------------------------------------------------------------------------------
def test_host_selection_against_float64(pkg):
    worst_abs = worst_rel = 0.0
    for name in SETS:
        S, p, nrm, u = cases(pkg, name)
        nodes, _, _, depth = pkg.emitter_tree_nodes(*S.args())
        part = F64.intervals(nodes, p, nrm)
        assert np.abs((part[2] - part[1]).sum(1) - 1.0).max() < 1e-12      # the twin's intervals tile [0, 1)
        fp, fn, fu = TLS.flat(p, nrm, u)
        one = pkg.emitter_tree_select(*S.args(), fp, fn, fu, 1.0)
        share, a, r = compare(name, part, u, one)
        print(f"emitter tree {name}: depth {depth}, excluded {100 * share:.4f} %, host fp32 vs float64 pmf abs {a:.3e} rel {r:.3e}")
        assert share <= EXCLUDED_CAP, (name, share)
        worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
        check_strata(name, one)
        half = pkg.emitter_tree_select(*S.args(), fp, fn, fu, 0.5)
        assert np.array_equal(one[0], half[0]) and all(np.array_equal(x * np.float32(0.5), y) for x, y in zip(one[1:], half[1:]))   # exactly: a power of two
    print(f"emitter tree worst: abs {worst_abs:.3e} rel {worst_rel:.3e}")
    assert worst_abs <= HOST_ABS and worst_rel <= HOST_REL, (worst_abs, worst_rel)


# ---- 4. the too-deep report --------------------------------------------------------------------------------------------------
def chain(pkg, n, k=30, ratio=2.0):
    """n emissive triangles of equal radiance at x = 2^(i - k) (ratio^i 2^-k), each a tenth of its x in size, all facing +y:
    self-similar, so the builder takes the same decision at every scale and peels one triangle per level."""
    x = ratio ** np.arange(n) * 2.0 ** -float(k)
    o = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    s = 0.1 * x[:, None]
    tris = np.stack([o, o + s * [0, 0, 1], o + s * [1, 0, 0]], 1)
    return Scene(np.zeros((0, 32), np.uint8), tris, np.arange(n), np.full((n, 3), 4.0))


def chain_lengths(pkg):
    """(n whose tree has GUARD levels, n whose tree has one more): a chain of n is n levels deep."""
    return GUARD, GUARD + 1


def test_a_chain_deeper_than_the_guard_is_reported(pkg):
    fits, deep = chain_lengths(pkg)
    S = chain(pkg, fits)
    nodes, trails, lengths, depth = pkg.emitter_tree_nodes(*S.args())
    assert depth == GUARD and F64.check_structure(nodes, trails, lengths, S.count, GUARD) == GUARD
    pm = pkg.emitter_tree_pmfs(*S.args(), [0.3, 1.0, 0.2], [0.0, -1.0, 0.0])
    assert abs(float(pm.astype(np.float64).sum()) - 1.0) < 1e-5
    D = chain(pkg, deep)
    assert pkg.emitter_tree_nodes(*D.args())[3] == GUARD + 1             # built and reported ...
    with pytest.raises(pkg.DmtError):                                    # ... and not walked: its trails would not fit the guard
        pkg.emitter_tree_pmfs(*D.args(), [0.3, 1.0, 0.2], [0.0, -1.0, 0.0])
    with pytest.raises(pkg.DmtError):
        pkg.emitter_tree_select(*D.args(), [[0.3, 1.0, 0.2]], [[0.0, -1.0, 0.0]], [0.5])


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_has_the_emitter_tree_flag():
    exe = Path(__file__).resolve().parent.parent / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    h = subprocess.run([str(exe), "-h"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--emitter-tree" in h.stdout
