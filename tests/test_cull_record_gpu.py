"""The brute-force pass reads each culled cluster from one 64-byte record, its bound words and count in one scalar load
(DESIGN.md 4.1).  Soups of 1, 3, 4, 5, 7, 8 and 16 candidate meshes put the last, partial group of four at every length and
cross a group boundary; sphere and box clusters come in both index orders, with an empty and a non-empty always list.  For each
soup the trace of ray pairs (tri, u, v, occluded) and a small film are bit-equal between DMT_BRUTE_CULL=2 and =0.  The
lens radius, read earlier in prepare_sample, changes no film with or without a sampler table."""
import numpy as np
import pytest

import test_brute_cull_box_gpu as BOXES
import test_brute_cull_gpu as SPHERES
from test_cull_record import _quad, _tetra

pytestmark = pytest.mark.gpu

# soup name -> (meshes in index order: T = a small tetrahedron (sphere cluster), Q = a small flat quad (box cluster),
#               two lone triangles behind everything that stay on the always list?, clusters expected)
SOUPS = {
    "1": ("T", True, 1),
    "3": ("QTQ", False, 3),
    "4": ("TTQQ", True, 4),
    "5": ("QQQTT", False, 5),
    "7": ("TQTQTQQ", True, 7),
    "8": ("QQQQQTTT", False, 8),
    "16": ("TTTT" + "Q" * 12, True, 12),    # the table's cap: four quads join the always list
}


def _soup(pkg, kinds, anchor):
    """The meshes on a 4 x 4 grid in the Cornell box's volume (x, z in [-1.5, 1.5], y in [1.2, 3.4]), seen by its camera and lit
    by its light, materials cycling so that every mesh is a run of its own."""
    s = pkg.host_scene.cornell_box(64, 64)
    tris, mats = [], []
    for i, kind in enumerate(kinds):
        c = (-1.5 + 1.0 * (i % 4), 1.2 + 0.55 * (i // 4) + 0.13 * (i % 4), -1.5 + 1.0 * (i // 4) + 0.21 * (i % 3))
        mesh = _tetra(c, 0.16) if kind == "T" else _quad(c, 0.22, i % 3)
        tris += mesh
        mats += [i % 7] * len(mesh)
    if anchor:
        n = len(kinds)
        tris += [[[-2, 3.9, -2], [2, 3.9, -2], [2, 3.9, 2]]]
        tris += [[[-2, 0.1, -1.9], [2, 3.9, -1.9], [-2, 3.9, -1.9]]]
        mats += [n % 7, (n + 1) % 7]
    v = np.asarray(tris, np.float32)
    xs, ys, zs = (np.zeros((v.shape[0], 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    return pkg.host_scene.ArrayScene(xs, ys, zs, np.asarray(mats, np.uint32), s.bsdfs, s.lights, s.inf_lights, s.camera)


def _pairs(pkg, s, rec, seed):
    """About 20 000 ray pairs: the two existing generators' rays at the clusters (vertices, edges, grazing the bounds, from
    the meshes' own surfaces, on and through the inflated boxes' faces, axis-parallel) as closest rays, the same rays in
    another order as shadow rays with segment ends from 0.05 to past the scene and infinity."""
    plan = []
    for r in rec:
        b = r["b"].astype(np.float64)
        radius = float(np.sqrt(b[3])) if not r["box"] else float(np.linalg.norm(b[3:6]))
        plan.append((int(r["first"]), int(r["count"]), tuple(b[:3]), radius))
    boxes = pkg.binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id)
    o, d = SPHERES._rays(s, plan, 10_000 if boxes else 20_000, seed)
    if boxes:
        ob, db = BOXES._wall_rays(s, boxes, 10_000, seed + 100)
        o, d = np.concatenate([o, ob]), np.concatenate([d, db])
    rng = np.random.default_rng(seed + 200)
    perm = rng.permutation(o.shape[0])
    smax = rng.choice([0.05, 0.5, 1.5, 3.0, 8.0, np.inf], o.shape[0]).astype(np.float32) * rng.uniform(0.5, 1.0, o.shape[0]).astype(np.float32)
    return o, d, o[perm], d[perm], smax


def _run(pkg, monkeypatch, mode, s, pairs):
    monkeypatch.setenv("DMT_BRUTE_CULL", str(mode))
    r = pkg.Renderer(0)
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    try:
        r.upload_scene(s)
        trace = r.test_trace_pair(*pairs)
        r.set_limits(4)
        r.film_clear()
        r.render(16)
        return trace, r.download_film()
    finally:
        r.close()


@pytest.mark.parametrize("name", list(SOUPS))
def test_pairs_and_film_bit_equal_with_and_without_clusters(pkg, monkeypatch, name):
    kinds, anchor, want = SOUPS[name]
    s = _soup(pkg, kinds, anchor)
    rec, nbytes, align = pkg.binding.cull_records(s.xs, s.ys, s.zs, s.mat_id)
    assert (nbytes, align) == (64, 64)
    assert len(rec) == want
    ntri = np.asarray(s.mat_id).size
    assert (int(rec["count"].sum()) == ntri) == (not anchor)             # an empty always list without the lone triangles
    nT = min(kinds.count("T"), 4)
    assert [int(b) for b in rec["box"]] == [0] * nT + [1] * (want - nT)
    pairs = _pairs(pkg, s, rec, 300 + len(kinds))
    assert 15_000 <= pairs[0].shape[0] <= 25_000
    (i0, uv0, occ0), film0 = _run(pkg, monkeypatch, 0, s, pairs)
    (i2, uv2, occ2), film2 = _run(pkg, monkeypatch, 2, s, pairs)
    culled = np.zeros(i0.shape, bool)
    for r in rec:
        culled |= (i0 >= r["first"]) & (i0 < r["first"] + r["count"])
    assert culled.mean() > 0.05 and occ0.mean() > 0.02 and (~occ0).mean() > 0.02   # the rays do reach the culled meshes
    assert np.array_equal(i0, i2)
    assert np.array_equal(uv0.view(np.uint32), uv2.view(np.uint32))
    assert np.array_equal(occ0, occ2)
    assert np.isfinite(film0[0]).all() and film0[0][..., :3].max() > 0
    assert film0[0].tobytes() == film2[0].tobytes() and film0[1].tobytes() == film2[1].tobytes()


@pytest.mark.parametrize("lens", [False, True])
def test_film_does_not_depend_on_the_sampler_table(pkg, lens):
    s = pkg.host_scene.cornell_box(128, 128)
    films = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(s)
        r.set_limits(8)
        if lens:
            r.set_lens(0.05, 3.0)
        for mode in (pkg.binding.SAMPLER_TABLE_OFF, pkg.binding.SAMPLER_TABLE_AUTO, pkg.binding.SAMPLER_TABLE_FORCE):
            r.set_sampler_table(mode)
            r.film_clear()
            r.render(16)
            films[mode] = r.download_film()
        r.set_sampler_table(pkg.binding.SAMPLER_TABLE_FORCE)
        r.set_lens(0.0, 3.0) if lens else r.set_lens(0.05, 3.0)
        r.film_clear()
        r.render(16)
        other = r.download_film()
    off = films[pkg.binding.SAMPLER_TABLE_OFF]
    assert np.isfinite(off[0]).all()
    for mode, f in films.items():
        assert f[0].tobytes() == off[0].tobytes() and f[1].tobytes() == off[1].tobytes(), mode
    assert other[0].tobytes() != off[0].tobytes()                   # the lens radius is read: the other setting differs
