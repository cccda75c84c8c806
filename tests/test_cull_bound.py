"""CPU tests of the brute-force pass's box bound in its centre / half-width form.  dmt_cull_box_test runs
the inline functions that brute_clusters calls, compiled for the host, so the arithmetic under test is the shipped one.

The reference is the float64 overlap of the segment [1e-4, tmax] with the cluster's UNINFLATED vertex box: a ray it accepts
can hit a triangle of the cluster, so the bound must never reject it.  The same rays go through a float32 restatement of
the former lo / hi slab test; both accept counts are printed, and written to profiles/cull_bound/accept_counts.txt when
DMT_WRITE_PROFILES=1 (the committed copy comes from such a run)."""
import os
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from test_brute_cull_box_gpu import _dense_scene

ROOT = Path(__file__).resolve().parent.parent
T_LO = np.float32(1e-4) * (np.float32(1) - np.float32(1) / np.float32(256))   # kCullTLo
T_SLACK = np.float32(1) + np.float32(1) / np.float32(256)                      # kCullTSlack
N_PER_KIND = 2_100_000


@pytest.fixture(scope="module")
def binding(pkg):
    return pkg.binding


def _soup(v):
    v = np.asarray(v, np.float32)
    xs, ys, zs = (np.zeros((v.shape[0], 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    return xs, ys, zs


BIG = np.array([[[-1, -1, -1], [1, -1, 1], [1, 1, 1]], [[-1, -1, -1], [1, 1, 1], [-1, 1, -1]]], np.float64)  # the scene box
KINDS = {
    # a flat wall: zero thickness across z
    "flat wall": (np.array([[[0, 0, 0.5], [0.4, 0, 0.5], [0.4, 0.4, 0.5]], [[0, 0, 0.5], [0.4, 0.4, 0.5], [0, 0.4, 0.5]]], np.float64), 0.0),
    # two triangles that are not coplanar: a box with three extents
    "thick box": (np.array([[[0.1, -0.3, 0.2], [0.5, -0.3, 0.3], [0.3, 0.2, 0.45]], [[0.1, 0.1, 0.25], [0.45, -0.1, 0.2], [0.5, 0.2, 0.4]]], np.float64), 0.0),
    # the flat wall's scene 1000 units from the origin on every axis
    "box 1000 units out": (np.array([[[0, 0, 0.5], [0.4, 0, 0.5], [0.4, 0.4, 0.5]], [[0, 0, 0.5], [0.4, 0.4, 0.5], [0, 0.4, 0.5]]], np.float64),
                           np.array([1000.0, -1000.0, 1000.0])),
}


def _cluster(binding, kind):
    tris, shift = KINDS[kind]
    xs, ys, zs = _soup(np.concatenate([BIG, tris]) + shift)
    recs = binding.brute_cull_box_records(xs, ys, zs, np.array([0, 0, 1, 1], np.uint32))
    assert len(recs) == 1
    v = np.stack([xs[2:, :3], ys[2:, :3], zs[2:, :3]], axis=-1).reshape(-1, 3).astype(np.float64)   # the float32 vertices
    s = np.stack([xs[:, :3], ys[:, :3], zs[:, :3]], axis=-1).reshape(-1, 3).astype(np.float64)
    box, rec = recs[0]
    return dict(vlo=v.min(0), vhi=v.max(0), slo=s.min(0), shi=s.max(0), box=box, rec=rec)


def _rays(cl, n, seed):
    """About n rays (float32 origins, float32 unit directions, float32 tmax) around one cluster; see the module docstring of
    the issue's list: every family below is one of its items."""
    rng = np.random.default_rng(seed)
    vlo, vhi, slo, shi = cl["vlo"], cl["vhi"], cl["slo"], cl["shi"]
    blo, bhi = cl["box"][:3].astype(np.float64), cl["box"][3:].astype(np.float64)
    ext = float((shi - slo).max())
    ctr = 0.5 * (vlo + vhi)
    k = n // 9 + 1
    O, D, T = [], [], []

    def inbox(m, lo=vlo, hi=vhi, grow=0.0):
        g = grow * (hi - lo + 1e-3 * ext)
        return rng.uniform(lo - g, hi + g, (m, 3))

    def add(o, d, t=None):
        o = np.asarray(o, np.float64).astype(np.float32)
        d = np.asarray(d, np.float64)
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        if t is None:
            t = rng.uniform(0, 3 * ext, o.shape[0])
        t = np.asarray(t, np.float64).astype(np.float32)
        t[rng.uniform(0, 1, t.shape[0]) < 0.25] = np.inf
        O.append(o), D.append(d), T.append(t)

    # uniform random segments through the scene, half of them aimed at the cluster
    o = rng.uniform(slo - 0.25 * ext, shi + 0.25 * ext, (2 * k, 3))
    p = np.where(rng.uniform(0, 1, (2 * k, 1)) < 0.5, inbox(2 * k, grow=0.5), rng.uniform(slo, shi, (2 * k, 3)))
    add(o, p - o, np.linalg.norm(p - o, axis=1) * rng.uniform(0, 2, 2 * k))
    # origins exactly on a face of the vertex box or of the planner's inflated box, or one float step outside it
    for lo, hi in ((vlo, vhi), (blo, bhi)):
        o = inbox(k // 2, lo, hi, grow=0.05).astype(np.float32)
        ax, side = rng.integers(0, 3, k // 2), rng.integers(0, 2, k // 2)
        f = np.where(side == 1, hi[ax], lo[ax]).astype(np.float32)
        step = rng.uniform(0, 1, k // 2) < 0.5
        f = np.where(step, np.nextafter(f, np.where(side == 1, np.float32(np.inf), np.float32(-np.inf)), dtype=np.float32), f)
        o[np.arange(k // 2), ax] = f
        d = rng.normal(size=(k // 2, 3))
        zero = rng.uniform(0, 1, k // 2) < 0.3   # ... some of them parallel to that face
        d[zero, ax[zero]] = 0.0
        add(o, d)
    # axis-parallel rays and rays with one or two zero components, from inside and around the cluster's slabs
    o = np.where(rng.uniform(0, 1, (2 * k, 1)) < 0.5, inbox(2 * k, grow=0.02), rng.uniform(slo, shi, (2 * k, 3)))
    sel = rng.uniform(0, 1, (2 * k, 3)) < 0.5
    sel[sel.all(1) | ~sel.any(1)] = [True, False, False]
    o = np.where(sel, o, inbox(2 * k))   # the other coordinates start inside the box: most of these rays meet it
    d = rng.normal(size=(2 * k, 3)) * sel
    add(o, d)
    # grazing a face's plane at 1e-1 ... 1e-7 rad, from on it, just off it and from far along it
    ax = rng.integers(0, 3, 2 * k)
    nrm = np.eye(3)[ax]
    p = inbox(2 * k)
    p[np.arange(2 * k), ax] = np.where(rng.uniform(0, 1, 2 * k) < 0.5, vlo[ax], vhi[ax])
    tang = rng.normal(size=(2 * k, 3))
    tang -= nrm * (tang * nrm).sum(1, keepdims=True)
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    ang = 10.0 ** rng.uniform(-7, -1, (2 * k, 1)) * rng.choice([-1.0, 1.0], (2 * k, 1))
    d = tang + np.tan(ang) * nrm
    back = rng.choice([0.0, 1e-3, 1.0, 8.0], (2 * k, 1)) * ext
    add(p - back * d, d, np.where(rng.uniform(0, 1, 2 * k) < 0.5, back[:, 0] * np.linalg.norm(d, axis=1) * rng.uniform(0.5, 2, 2 * k), 20 * ext))
    # origins out to 64 scene extents, aimed at the cluster
    u = rng.normal(size=(k, 3))
    o = ctr + u / np.linalg.norm(u, axis=1, keepdims=True) * (2.0 ** rng.uniform(0, 6, (k, 1))) * ext
    p = inbox(k, grow=0.3)
    add(o, p - o, np.linalg.norm(p - o, axis=1) * rng.choice([0.999, 1.0, 1.5, 4.0], k))
    # segments that end exactly on a face of the vertex box
    o = rng.uniform(slo, shi, (k, 3))
    p = inbox(k)
    ax = rng.integers(0, 3, k)
    p[np.arange(k), ax] = np.where(rng.uniform(0, 1, k) < 0.5, vlo[ax], vhi[ax])
    o32 = o.astype(np.float32).astype(np.float64)
    d32 = ((p - o32) / np.linalg.norm(p - o32, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tface = (p[np.arange(k), ax] - o32[np.arange(k), ax]) / d32[np.arange(k), ax]   # of the float32 ray
    tface = np.where(np.isfinite(tface) & (tface > 0), tface, 1.0)
    n0 = len(T)
    add(o32, d32, tface)
    T[n0][:] = tface.astype(np.float32)   # (no inf here: the end on the face is the point)
    return np.concatenate(O), np.concatenate(D), np.concatenate(T)


def _reference(cl, o, d, tmax):
    """float64: does the segment [1e-4, tmax] of the float32 ray meet the vertex box?"""
    o, d, tmax = o.astype(np.float64), d.astype(np.float64), tmax.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (cl["vlo"] - o) / d
        t1 = (cl["vhi"] - o) / d
    inside = (o >= cl["vlo"]) & (o <= cl["vhi"])
    par = d == 0
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return np.maximum(near.max(1), 1e-4) <= np.minimum(far.min(1), tmax)


def _former_test(cl, o, d, tmax):
    """float32 restatement of the lo / hi slab test this form replaced (planner box, FLT_MIN floor, min / max network)."""
    f = np.float32
    lo, hi = cl["box"][:3], cl["box"][3:]
    with np.errstate(over="ignore", invalid="ignore"):
        inv = f(1) / np.copysign(np.maximum(np.abs(d), f(2.0 ** -126)), d)
        a, b = (lo - o) * inv, (hi - o) * inv
        near = np.maximum(np.minimum(a, b).max(1), T_LO)
        far = np.minimum(np.maximum(a, b).min(1), tmax * T_SLACK)
        return near <= far * T_SLACK


@pytest.fixture(scope="module")
def verdicts(binding):
    """Per cluster kind: the ray count and the accept masks of the reference, the shipped bound and the former bound,
    computed once for the tests below."""
    out = {}
    for i, kind in enumerate(KINDS):
        cl = _cluster(binding, kind)
        o, d, tmax = _rays(cl, N_PER_KIND, 1 + i)
        assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).sum(1) > 0).all()
        out[kind] = (o.shape[0], _reference(cl, o, d, tmax), binding.cull_box_test(cl["rec"], o, d, tmax), _former_test(cl, o, d, tmax))
    return out


def _table(verdicts):
    lines = ["box bound, accepted rays of tests/test_cull_bound.py's ray sets (float64 reference: segment [1e-4, tmax] against the",
             "uninflated vertex box; former bound: float32 restatement of the lo / hi slab test; misses: rejected though the",
             "reference accepts)",
             f"{'cluster':<20} {'rays':>9} {'reference':>10} {'new bound':>10} {'former':>10} {'new misses':>11} {'former misses':>14}"]
    for kind, (n, ref, new, old) in verdicts.items():
        lines.append(f"{kind:<20} {n:>9} {ref.sum():>10} {new.sum():>10} {old.sum():>10} {(ref & ~new).sum():>11} {(ref & ~old).sum():>14}")
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("kind", list(KINDS))
def test_bound_rejects_no_ray_that_meets_the_vertex_box(verdicts, kind):
    n, ref, new, old = verdicts[kind]
    print(_table({kind: verdicts[kind]}))
    assert n >= 2_000_000
    assert 0.1 < ref.mean() < 0.9                  # the set exercises both answers
    assert not new.all()                           # ... and so does the bound
    assert int((ref & ~new).sum()) == 0


def test_accept_counts_table(verdicts):
    """Prints both bounds' accept counts; DMT_WRITE_PROFILES=1 also writes them to profiles/cull_bound/accept_counts.txt."""
    text = _table(verdicts)
    print(text)
    assert len(text.splitlines()) == 4 + len(KINDS)
    if os.environ.get("DMT_WRITE_PROFILES") == "1":
        (ROOT / "profiles" / "cull_bound").mkdir(parents=True, exist_ok=True)
        (ROOT / "profiles" / "cull_bound" / "accept_counts.txt").write_text(text)


def _dense_soup(pkg):
    """Cornell plus two more small meshes: four sphere clusters and five box clusters (the GPU test's own builder)."""
    s = _dense_scene(pkg)
    return s.xs, s.ys, s.zs, s.mat_id


def _caps_soup():
    """The twelve-cluster scene of tests/test_brute_cull_box.py::test_box_clusters_respect_the_caps (built inside that test,
    so restated here: same seed, same recipe)."""
    rng = np.random.default_rng(7)
    tris, mats = [], []
    sizes = [1] + [2] * 14 + [6, 2]
    for k, n in enumerate(sizes):
        c = rng.uniform(-4, 4, 3)
        quad = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
        quad[..., 2] = c[2]
        tris.append(quad)
        mats += [k] * n
    tris.append(np.array([[[-5, -5, -5], [5, -5, -5], [5, 5, 5]]], np.float64))
    mats.append(len(sizes))
    return (*_soup(np.concatenate(tris)), np.asarray(mats, np.uint32))


@pytest.mark.parametrize("scene", ["cornell", "dense", "caps", "cornell+1000", "caps+1000"])
def test_record_holds_the_planner_box(pkg, binding, scene):
    """[c - h, c + h] in exact arithmetic holds the planner's inflated box, which dmt_brute_cull_box_plan still reports."""
    name, _, far = scene.partition("+")
    if name == "cornell":
        s = pkg.host_scene.cornell_box(64, 64)
        xs, ys, zs, mat = s.xs, s.ys, s.zs, s.mat_id
    else:
        xs, ys, zs, mat = _dense_soup(pkg) if name == "dense" else _caps_soup()
    if far:
        xs, ys, zs = (np.asarray(a, np.float32) + np.float32(t) for a, t in zip((xs, ys, zs), (1000, -1000, 1000)))
    plan = binding.brute_cull_box_plan(xs, ys, zs, mat)
    recs = binding.brute_cull_box_records(xs, ys, zs, mat)
    assert len(recs) == len(plan) >= 5
    for (first, count, lo, hi), (box, rec) in zip(plan, recs):
        assert np.array_equal(np.asarray(lo + hi, np.float32), box)
        ext = max(float(box[3 + a]) - float(box[a]) for a in range(3))
        for a in range(3):
            c, h = Fraction(float(rec[a])), Fraction(float(rec[3 + a]))
            assert h > 0 and c - h <= Fraction(float(box[a])) and c + h >= Fraction(float(box[3 + a]))
            # ... and no more than the rounding of c and h beyond it: 2^-22 of the coordinates and the extent
            slop = Fraction(2.0 ** -22) * (abs(c) + Fraction(ext))
            assert c - h >= Fraction(float(box[a])) - slop and c + h <= Fraction(float(box[3 + a])) + slop
