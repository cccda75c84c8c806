"""The brute-force pass with box clusters gives the results of the plain loop over every triangle, bit for
bit: closest hits of rays aimed at the walls' edges and corners, leaving the walls, grazing them and lying on their inflated
boxes' faces, and films of the brute-force kernel rows.  DMT_BRUTE_CULL=0 turns every cluster off, =1 keeps the sphere
clusters only, unset gives both kinds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ctx(pkg, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    else:
        monkeypatch.setenv("DMT_BRUTE_CULL", str(mode))
    r = pkg.Renderer(0)
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    return r


def _verts(s):
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4)[:, :3] for a in (s.xs, s.ys, s.zs))
    return np.stack([xs, ys, zs], axis=-1)  # [tri][vertex][axis]


def _dense_scene(pkg):
    """Cornell box plus two more small meshes after the walls: four sphere clusters and five box clusters."""
    s = pkg.host_scene.cornell_box(128, 128)
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4) for a in (s.xs, s.ys, s.zs))
    mat = np.asarray(s.mat_id, np.uint32)
    add = []
    for src, shift, scale in ((slice(0, 8), (0.9, -0.6, 0.9), 0.6), (slice(8, 16), (-1.0, -0.9, 1.2), 0.4)):
        c = np.array([xs[src, :3].mean(), ys[src, :3].mean(), zs[src, :3].mean()], np.float32)
        p = [(a[src].copy() - ci) * scale + ci + di for a, ci, di in zip((xs, ys, zs), c, shift)]
        for q in p:
            q[:, 3] = 0
        add.append((p, mat[src]))
    xs = np.concatenate([xs] + [p[0] for p, _ in add]); ys = np.concatenate([ys] + [p[1] for p, _ in add])
    zs = np.concatenate([zs] + [p[2] for p, _ in add]); mat = np.concatenate([mat] + [m for _, m in add])
    return pkg.host_scene.ArrayScene(xs, ys, zs, mat, s.bsdfs, s.lights, s.inf_lights, s.camera)


def _wall_rays(s, boxes, n, seed):
    rng = np.random.default_rng(seed)
    v = _verts(s).astype(np.float64)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    k = n // (6 * len(boxes))
    o, d = [], []
    for first, count, blo, bhi in boxes:
        cv = v[first:first + count]
        n_ = np.cross(cv[0, 1] - cv[0, 0], cv[0, 2] - cv[0, 0])
        n_ /= np.linalg.norm(n_)
        # edges and corners, from anywhere in the scene box
        org = rng.uniform(lo, hi, (k, 3))
        t, a = rng.integers(0, count, k), rng.integers(0, 3, k)
        b = rng.uniform(0, 1, (k, 1)) * (rng.uniform(0, 1, (k, 1)) < 0.7)   # 30 % exactly at a vertex
        e0, e1 = cv[t, a], cv[t, (a + 1) % 3]
        o.append(org), d.append(e0 + b * (e1 - e0) - org)
        # from the surface, the origin pushed off by a few ulps to either side (offset_ray_origin), any direction
        bary = rng.dirichlet([1, 1, 1], k)
        t = rng.integers(0, count, k)
        p = np.einsum("mk,mka->ma", bary, cv[t]).astype(np.float32)
        side = rng.choice([-1.0, 1.0], (k, 1))
        p = np.nextafter(p, (p + side * n_ * rng.integers(1, 4, (k, 1))).astype(np.float32))
        o.append(p), d.append(rng.normal(size=(k, 3)))
        # leaving the surface at small angles (the box's own thickness against kCullTLo)
        p = np.einsum("mk,mka->ma", rng.dirichlet([1, 1, 1], k), cv[rng.integers(0, count, k)])
        tang = np.cross(n_, rng.normal(size=(k, 3)))
        tang /= np.linalg.norm(tang, axis=1, keepdims=True)
        ang = 10.0 ** rng.uniform(-6, -0.5, (k, 1)) * rng.choice([-1.0, 1.0], (k, 1))
        o.append(p), d.append(tang + ang * n_)
        # grazing, in the wall's plane or just off it
        p = np.einsum("mk,mka->ma", rng.dirichlet([1, 1, 1], k), cv[rng.integers(0, count, k)])
        p = p + n_ * rng.choice([0.0, 1e-6, -1e-6, 1e-4], (k, 1))
        o.append(p), d.append(np.cross(n_, rng.normal(size=(k, 3))))
        # axis-parallel, origins exactly on the inflated box's faces
        blo, bhi = np.asarray(blo, np.float32), np.asarray(bhi, np.float32)
        org = rng.uniform(blo, bhi, (k, 3)).astype(np.float32)
        ax = rng.integers(0, 3, k)
        org[np.arange(k), ax] = np.where(rng.uniform(0, 1, k) < 0.5, blo[ax], bhi[ax])
        dirs = np.zeros((k, 3))
        dirs[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
        o.append(org), d.append(dirs)
        # axis-parallel from anywhere, through the wall
        org = rng.uniform(lo, hi, (k, 3))
        dirs = np.zeros((k, 3))
        dirs[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
        o.append(org), d.append(dirs)
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ok = np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0)
    return o[ok], d[ok]


@pytest.mark.parametrize("scene", ["cornell", "dense"])
def test_closest_hit_bit_equal_with_box_clusters(pkg, monkeypatch, scene):
    s = pkg.host_scene.cornell_box(64, 64) if scene == "cornell" else _dense_scene(pkg)
    boxes = pkg.binding.brute_cull_box_plan(s.xs, s.ys, s.zs, s.mat_id)
    assert [(f, c) for f, c, _, _ in boxes] == [(16, 2), (18, 2), (20, 2), (22, 2), (24, 2)]
    o, d = _wall_rays(s, boxes, 1_250_000, 21 if scene == "cornell" else 22)
    assert o.shape[0] >= 1_000_000
    out = {}
    for mode in (0, 1, None):
        r = _ctx(pkg, monkeypatch, mode)
        try:
            r.upload_scene(s)
            out[mode] = r.test_closest_hit(o, d)
        finally:
            r.close()
    i0, t0 = out[0]
    assert ((i0 >= 16) & (i0 < 26)).mean() > 0.3          # the rays do reach the walls
    for mode in (1, None):
        i1, t1 = out[mode]
        assert np.array_equal(i0, i1)
        assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32))


def _film(pkg, monkeypatch, mode, scene, spp, env=False):
    r = _ctx(pkg, monkeypatch, mode)
    try:
        r.upload_scene(scene)
        if env:
            r.upload_envmap(pkg.host_scene.synthetic_sky(64))
        r.set_limits(8)
        r.film_clear()
        r.render(spp)
        return r.download_film()
    finally:
        r.close()


@pytest.mark.parametrize("case", ["cornell", "cornell_env", "dense"])
def test_films_bit_equal_across_cull_modes(pkg, monkeypatch, case):
    if case == "dense":
        s, spp = _dense_scene(pkg), 16
    else:
        s, spp = pkg.host_scene.cornell_box(256, 256), 64
    env = case == "cornell_env"
    ref = _film(pkg, monkeypatch, 0, s, spp, env)
    assert np.isfinite(ref[0]).all()
    for mode in (1, None):
        f = _film(pkg, monkeypatch, mode, s, spp, env)
        assert np.array_equal(ref[0].view(np.uint32), f[0].view(np.uint32))
        assert np.array_equal(ref[1].view(np.uint32), f[1].view(np.uint32))
