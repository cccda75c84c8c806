"""CPU tests of the brute-force pass's culled clusters (dmt_brute_cull_plan): which runs of triangles are
tested only for the rays that touch their bounding sphere."""
import numpy as np
import pytest


@pytest.fixture
def binding(pkg):
    return pkg.binding


def _verts(s, first, count):
    xs, ys, zs = (np.asarray(a, np.float64).reshape(-1, 4)[first:first + count, :3] for a in (s.xs, s.ys, s.zs))
    return np.stack([xs, ys, zs], axis=-1).reshape(-1, 3)


def test_cornell_box_splits_into_walls_and_two_octahedra(pkg, binding):
    s = pkg.host_scene.cornell_box(64, 64)
    plan = binding.brute_cull_plan(s.xs, s.ys, s.zs, s.mat_id)
    assert [(f, c) for f, c, _, _ in plan] == [(0, 8), (8, 8)]   # 26 - 16 = 10 wall triangles stay in the always list
    for first, count, centre, radius in plan:
        d = np.linalg.norm(_verts(s, first, count) - np.asarray(centre, np.float64), axis=1)
        assert d.max() < radius and radius < 0.5 * 1.01        # every vertex inside the inflated bound; octahedra of radius 0.5
    assert binding.brute_cull_plan(s.xs, s.ys, s.zs, s.mat_id, enable=False) == []


def test_large_triangles_give_no_cluster(binding):
    rng = np.random.default_rng(3)
    n = 40
    xs, ys, zs = (np.zeros((n, 4), np.float32) for _ in range(3))
    v = rng.uniform(-5, 5, (n, 3, 3)).astype(np.float32)
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    assert binding.brute_cull_plan(xs, ys, zs, np.zeros(n, np.uint32)) == []


def test_small_meshes_are_culled_within_the_caps(binding):
    """Runs of one material: small ones are culled in index order, short runs and runs over the LDS cap are not."""
    rng = np.random.default_rng(5)
    sizes = [3, 8, 12, 10, 6, 8, 4]  # run 0 is too short; 8 + 12 + 10 = 30 culled triangles, every later run would exceed 32
    tris, mats = [], []
    for k, n in enumerate(sizes):
        c = rng.uniform(-4, 4, 3)
        tris.append(c + rng.uniform(-0.2, 0.2, (n, 3, 3)))
        mats += [k] * n
    tris.append(np.array([[[-5, -5, -5], [5, -5, -5], [5, 5, 5]]], np.float64))  # one large triangle sets the scene's size
    mats.append(len(sizes))
    v = np.concatenate(tris).astype(np.float32)
    xs, ys, zs = (np.zeros((v.shape[0], 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = v[..., 0], v[..., 1], v[..., 2]
    plan = binding.brute_cull_plan(xs, ys, zs, np.asarray(mats, np.uint32))
    assert [(f, c) for f, c, _, _ in plan] == [(3, 8), (11, 12), (23, 10)]
    for first, count, centre, radius in plan:
        d = np.linalg.norm(v[first:first + count].reshape(-1, 3).astype(np.float64) - np.asarray(centre, np.float64), axis=1)
        assert d.max() < radius
