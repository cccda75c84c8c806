"""CPU tests of the brute-force pass's box clusters (dmt_brute_cull_box_plan): flat one-material runs, such
as walls, that are tested only for the rays that cross their inflated box."""
import numpy as np
import pytest


@pytest.fixture
def binding(pkg):
    return pkg.binding


def _soup(v):
    v = np.asarray(v, np.float32)
    xs, ys, zs = (np.zeros((v.shape[0], 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    return xs, ys, zs


def _verts(s, first, count):
    xs, ys, zs = (np.asarray(a, np.float64).reshape(-1, 4)[first:first + count, :3] for a in (s.xs, s.ys, s.zs))
    return np.stack([xs, ys, zs], axis=-1).reshape(-1, 3)


def test_cornell_walls_are_five_box_clusters(pkg, binding):
    s = pkg.host_scene.cornell_box(64, 64)
    assert [(f, c) for f, c, _, _ in binding.brute_cull_plan(s.xs, s.ys, s.zs, s.mat_id)] == [(0, 8), (8, 8)]
    boxes = binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id)
    assert [(f, c) for f, c, _, _ in boxes] == [(16, 2), (18, 2), (20, 2), (22, 2), (24, 2)]
    for first, count, lo, hi in boxes:
        v = _verts(s, first, count)
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        assert (v > lo).all() and (v < hi).all()      # strictly inside, also across a wall's zero thickness
        assert (hi - lo).min() < 1e-4                   # ... which stays thin: a ray leaving the wall is not handed it again
    assert binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id, enable=False) == []


def test_large_random_triangles_give_no_box_cluster(binding):
    rng = np.random.default_rng(3)
    n = 40
    xs, ys, zs = _soup(rng.uniform(-5, 5, (n, 3, 3)))
    assert binding.brute_cull_box_plan(xs, ys, zs, np.zeros(n, np.uint32)) == []          # one run: the whole scene
    assert binding.brute_cull_box_plan(xs, ys, zs, np.arange(n, dtype=np.uint32)) == []   # single triangles


def test_run_spanning_most_of_the_scene_is_not_culled(binding):
    """A diagonal quad whose box is the whole scene stays in the always list; a small flat quad beside it is culled."""
    big = [[[-1, -1, -1], [1, -1, 1], [1, 1, 1]], [[-1, -1, -1], [1, 1, 1], [-1, 1, -1]]]
    small = [[[0, 0, 0.5], [0.4, 0, 0.5], [0.4, 0.4, 0.5]], [[0, 0, 0.5], [0.4, 0.4, 0.5], [0, 0.4, 0.5]]]
    xs, ys, zs = _soup(big + small)
    plan = binding.brute_cull_box_plan(xs, ys, zs, np.array([0, 0, 1, 1], np.uint32))
    assert [(f, c) for f, c, _, _ in plan] == [(2, 2)]


def test_box_clusters_respect_the_caps(binding):
    """At most 12 clusters in all and 44 culled triangles, taken in index order after the sphere clusters; single
    triangles are never culled."""
    rng = np.random.default_rng(7)
    tris, mats = [], []
    sizes = [1] + [2] * 14 + [6, 2]
    for k, n in enumerate(sizes):
        c = rng.uniform(-4, 4, 3)
        quad = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
        quad[..., 2] = c[2]                                       # flat: the sphere rule is not what takes them
        tris.append(quad)
        mats += [k] * n
    tris.append(np.array([[[-5, -5, -5], [5, -5, -5], [5, 5, 5]]], np.float64))
    mats.append(len(sizes))
    xs, ys, zs = _soup(np.concatenate(tris))
    mat = np.asarray(mats, np.uint32)
    spheres = binding.brute_cull_plan(xs, ys, zs, mat)
    boxes = binding.brute_cull_box_plan(xs, ys, zs, mat)
    assert len(spheres) + len(boxes) <= 12
    assert sum(c for _, c, _, _ in spheres) + sum(c for _, c, _, _ in boxes) <= 44
    taken = {f for f, _, _, _ in spheres}
    firsts = [f for f, _, _, _ in boxes]
    assert firsts == sorted(firsts) and not taken & set(firsts)
    assert all(c >= 2 for _, c, _, _ in boxes) and 0 not in firsts
    assert len(spheres) + len(boxes) == 12                  # 15 candidate runs: the cluster cap binds
