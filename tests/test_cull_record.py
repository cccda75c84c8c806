"""CPU tests of the cluster records of the brute-force pass (dmt_cull_records): 64 bytes, 64-byte aligned,
everything the device reads of a cluster in one record, the bound words and the count in its first 32 bytes.  The records
equal a numpy restatement of the two planners' rules (planBruteCull, planBruteCullBox), and Cornell's equal what the build
before the 64-byte record reported (tests/golden/cull_record/cornell.json: bounds as float bits, first, count from
dmt_brute_cull_plan / dmt_brute_cull_box_plan / dmt_brute_cull_box_records of that build; it had no entry point for slot and
magic, which the restatement covers)."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "cull_record", "cornell.json")

MAX_CLUSTERS, MAX_TRIS = 12, 44
MAX_SPHERES, MAX_SPHERE_TRIS, MIN_SPHERE_TRIS, MAX_RADIUS_FRAC = 4, 32, 4, 0.125
MIN_BOX_TRIS, MAX_AREA_FRAC = 2, 0.35


@pytest.fixture
def binding(pkg):
    return pkg.binding


def _soup(v):
    v = np.asarray(v, np.float32)
    xs, ys, zs = (np.zeros((v.shape[0], 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    return xs, ys, zs


def _verts64(xs, ys, zs):
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4)[:, :3].astype(np.float64) for a in (xs, ys, zs))
    return np.stack([xs, ys, zs], axis=-1)  # [tri][vertex][axis]


def _runs(mat):
    mat = np.asarray(mat)
    first = 0
    while first < len(mat):
        end = first + 1
        while end < len(mat) and mat[end] == mat[first]:
            end += 1
        yield first, end
        first = end


def _f32_down(x):
    """the nearest float, moved down when it lies above the double x"""
    f = np.float32(x)
    return np.nextafter(f, np.float32(-np.inf)) if float(f) > x else f


def _f32_up(x):
    f = np.float32(x)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < x else f


def _magic(count):
    return ((1 << 32) + count - 1) // count


def _plan_spheres(v, mat):
    """planBruteCull in numpy: (b[6], box, count, first, slot, magic) per cluster"""
    out = []
    if len(v) == 0:
        return out
    p = v.reshape(-1, 3)
    diag = float(np.sqrt(((p.max(0) - p.min(0)) ** 2).sum()))
    culled = 0
    for first, end in _runs(mat):
        if len(out) >= MAX_SPHERES:
            break
        count = end - first
        if count < MIN_SPHERE_TRIS or culled + count > MAX_SPHERE_TRIS:
            continue
        q = v[first:end].reshape(-1, 3)
        c = (0.5 * (q.min(0) + q.max(0))).astype(np.float32)
        dx, dy, dz = (q - c.astype(np.float64)).T
        r2 = float((dx * dx + dy * dy + dz * dz).max())
        cmax = float(np.abs(c.astype(np.float64)).max())
        r = np.sqrt(r2) * (1.0 + 1.0 / 1024) + 1e-6 * (cmax + np.sqrt(r2))
        if not r <= MAX_RADIUS_FRAC * diag:
            continue
        b = np.zeros(6, np.float32)
        b[:3] = c
        b[3] = np.nextafter(np.float32(r * r), np.float32(np.inf))
        out.append((b, 0, count, first, culled, _magic(count)))
        culled += count
    return out


def _area(lo, hi):
    x, y, z = hi - lo
    return 2.0 * (x * y + y * z + z * x)


def _plan_boxes(v, mat, spheres):
    """planBruteCullBox in numpy, after the sphere clusters"""
    out = []
    if len(v) == 0:
        return out
    p = v.reshape(-1, 3)
    scene_area = _area(p.min(0), p.max(0))
    if not (np.isfinite(scene_area) and scene_area > 0.0):
        return out
    culled = sum(s[2] for s in spheres)
    for first, end in _runs(mat):
        if len(spheres) + len(out) >= MAX_CLUSTERS:
            break
        count = end - first
        if count < MIN_BOX_TRIS or culled + count > MAX_TRIS:
            continue
        if any(s[3] == first for s in spheres):
            continue
        q = v[first:end].reshape(-1, 3)
        blo, bhi = q.min(0), q.max(0)
        if not _area(blo, bhi) <= MAX_AREA_FRAC * scene_area:
            continue
        ext = float((bhi - blo).max())
        cmax = float(max(np.abs(blo).max(), np.abs(bhi).max()))
        m = 2.0 ** -19 * (ext + cmax)
        b = np.zeros(6, np.float32)
        for a in range(3):
            lo, hi = _f32_down(blo[a] - m), _f32_up(bhi[a] + m)
            c = np.float32(0.5 * (float(lo) + float(hi)))
            hd = max(float(c) - float(lo), float(hi) - float(c))
            hw = np.nextafter(_f32_up(hd), np.float32(np.inf))
            b[a], b[3 + a] = c, hw
        out.append((b, 1, count, first, culled, _magic(count)))
        culled += count
    return out


def _expected(xs, ys, zs, mat, level):
    v = _verts64(xs, ys, zs)
    spheres = _plan_spheres(v, mat) if level >= 1 else []
    return spheres + (_plan_boxes(v, mat, spheres) if level >= 2 else [])


def _check(binding, xs, ys, zs, mat, level=2):
    rec, nbytes, align = binding.cull_records(xs, ys, zs, mat, level)
    assert nbytes == 64 and align == 64 and rec.dtype.itemsize == 64
    exp = _expected(xs, ys, zs, mat, level)
    assert len(rec) == len(exp)
    for r, (b, box, count, first, slot, magic) in zip(rec, exp):
        assert np.array_equal(r["b"].view(np.uint32), b.view(np.uint32))
        assert (int(r["box"]), int(r["count"]), int(r["first"]), int(r["slot"]), int(r["magic"])) == (box, count, first, slot, magic)
        assert not r["pad"].any()
    return rec


def _dense_scene(pkg):
    """the four-sphere-cluster scene of tests/test_brute_cull_gpu.py"""
    import importlib
    return importlib.import_module("test_brute_cull_gpu")._dense_scene(pkg)


def test_record_is_64_bytes_with_the_bound_words_first(binding):
    dt = binding.CULL_RECORD_DTYPE
    assert dt.itemsize == 64
    assert [dt.fields[n][1] for n in ("b", "box", "count", "first", "slot", "magic")] == [0, 24, 28, 32, 36, 40]
    rec, nbytes, align = binding.cull_records(*_soup(np.zeros((0, 3, 3))), np.zeros(0, np.uint32))
    assert len(rec) == 0 and nbytes == 64 and align == 64


@pytest.mark.parametrize("level", [0, 1, 2])
def test_cornell_records_equal_the_restated_planners_and_the_recorded_plan(pkg, binding, level):
    s = pkg.host_scene.cornell_box(64, 64)
    rec = _check(binding, s.xs, s.ys, s.zs, s.mat_id, level)
    gold = json.load(open(GOLDEN))
    want = [g for g in gold["clusters"] if level >= (2 if g["box"] else 1)]
    assert len(rec) == len(want) == (0, 2, 7)[level]
    for r, g in zip(rec, want):
        words = g["sphere_bits"] if not g["box"] else g["record_bits"]
        assert [int(x) for x in r["b"].view(np.uint32)[:len(words)]] == words
        assert (int(r["box"]), int(r["first"]), int(r["count"])) == (g["box"], g["first"], g["count"])
    # the whole table is one run of slots over the LDS copy, in cluster order
    assert [int(x) for x in rec["slot"]] == [int(x) for x in np.cumsum(np.r_[0, rec["count"][:-1]])][:len(rec)]


def test_cornell_records_agree_with_the_other_entry_points(pkg, binding):
    s = pkg.host_scene.cornell_box(64, 64)
    rec, _, _ = binding.cull_records(s.xs, s.ys, s.zs, s.mat_id)
    spheres = binding.brute_cull_plan(s.xs, s.ys, s.zs, s.mat_id)
    boxes = binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id)
    recs = binding.brute_cull_box_records(s.xs, s.ys, s.zs, s.mat_id)
    assert [(int(r["first"]), int(r["count"])) for r in rec] == [(f, c) for f, c, _, _ in spheres] + [(f, c) for f, c, _, _ in boxes]
    for r, (_, _, c, _) in zip(rec, spheres):
        assert np.array_equal(r["b"][:3], np.asarray(c, np.float32))
    for r, (_, b) in zip(rec[len(spheres):], recs):
        assert np.array_equal(r["b"].view(np.uint32), b.view(np.uint32))


def test_four_cluster_scene(pkg, binding):
    s = _dense_scene(pkg)
    for level in (1, 2):
        rec = _check(binding, s.xs, s.ys, s.zs, s.mat_id, level)
        assert [int(b) for b in rec["box"]] == [0] * 4 + [1] * (5 if level == 2 else 0)
    assert int(rec["count"][:4].sum()) == 32                 # the sphere clusters' triangle cap


def _tetra(c, r):
    p = np.asarray(c, np.float64) + r * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    return [[p[0], p[1], p[2]], [p[0], p[3], p[1]], [p[0], p[2], p[3]], [p[1], p[3], p[2]]]


def _quad(c, h, axis):
    c = np.asarray(c, np.float64)
    u, w = np.eye(3)[(axis + 1) % 3] * h, np.eye(3)[(axis + 2) % 3] * h
    return [[c - u - w, c + u - w, c + u + w], [c - u - w, c + u + w, c - u + w]]


def limit_soup(extra=True):
    """Four small tetrahedra (sphere clusters), twelve small flat quads (box candidates: the cluster cap takes eight) and one
    mesh more, each run a material of its own, spread over a 12 x 12 x 4 region."""
    tris, mats = [], []
    k = 0
    for i in range(4):
        tris += _tetra((-4.5 + 3.0 * i, -4.0, 0.5 * i), 0.25)
        mats += [k] * 4
        k += 1
    for i in range(12):
        tris += _quad((-5.0 + 0.9 * i, 1.0 + 0.3 * (i % 4), -1.5 + 0.25 * i), 0.3, i % 3)
        mats += [k] * 2
        k += 1
    if extra:
        tris += _quad((0.0, 5.0, 1.0), 0.4, 1)
        mats += [k] * 2
    xs, ys, zs = _soup(np.asarray(tris))
    return xs, ys, zs, np.asarray(mats, np.uint32)


def test_soup_at_the_planners_limits(binding):
    """4 sphere clusters and 12 box candidates: the table's 12 records are the spheres and the first 8 quads; the other
    four quads and the mesh after them stay on the always list, with or without that mesh in the soup."""
    for extra in (False, True):
        xs, ys, zs, mat = limit_soup(extra)
        rec = _check(binding, xs, ys, zs, mat)
        assert len(rec) == MAX_CLUSTERS
        assert [int(b) for b in rec["box"]] == [0] * 4 + [1] * 8
        assert [int(f) for f in rec["first"]] == [0, 4, 8, 12] + [16 + 2 * i for i in range(8)]
        assert int(rec["first"][-1] + rec["count"][-1]) == 32 < len(mat)      # triangles 32 .. stay on the always list
        assert int(rec["slot"][-1] + rec["count"][-1]) == 32 <= MAX_TRIS
    _check(binding, xs, ys, zs, mat, 1)
    _check(binding, xs, ys, zs, mat, 0)
