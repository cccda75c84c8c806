"""The brute-force pass with culled clusters gives the results of the plain loop over every triangle,
bit for bit: closest hits of single rays, and films of the brute-force kernel rows.  DMT_BRUTE_CULL=0, read when a
context is created, turns the clusters off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ctx(pkg, monkeypatch, cull):
    if cull:
        monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    else:
        monkeypatch.setenv("DMT_BRUTE_CULL", "0")
    r = pkg.Renderer(0)
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    return r


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _verts(s):
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4)[:, :3] for a in (s.xs, s.ys, s.zs))
    return np.stack([xs, ys, zs], axis=-1)  # [tri][vertex][axis]


def _rays(s, plan, n, seed):
    """Random rays in the scene's box, plus rays aimed at the culled meshes' vertices, edges and silhouettes, rays that graze
    their inflated bounds, rays that start on their surfaces, and axis-parallel rays."""
    rng = np.random.default_rng(seed)
    v = _verts(s)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    k = n // 8
    o, d = [], []
    o.append(rng.uniform(lo, hi, (2 * k, 3)))                                     # random
    d.append(rng.normal(size=(2 * k, 3)))
    for first, count, centre, radius in plan:
        cv = v[first:first + count]
        m = k // len(plan)
        org = rng.uniform(lo, hi, (m, 3))
        tgt = cv[rng.integers(0, count, m), rng.integers(0, 3, m)]                # vertices
        o.append(org), d.append(tgt - org)
        a, b = rng.integers(0, 3, m), rng.uniform(0, 1, (m, 1))                    # edges
        t = rng.integers(0, count, m)
        e0, e1 = cv[t, a], cv[t, (a + 1) % 3]
        org = rng.uniform(lo, hi, (m, 3))
        o.append(org), d.append(e0 + b * (e1 - e0) - org)
        org = rng.uniform(lo, hi, (m, 3))                                          # grazing the inflated sphere / silhouettes
        c = np.asarray(centre)
        to = c - org
        perp = np.cross(to, rng.normal(size=(m, 3)))
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        off = radius * rng.uniform(0.97, 1.03, (m, 1))
        o.append(org), d.append(c + perp * off - org)
        bary = rng.dirichlet([1, 1, 1], m)                                         # from the surface, any direction
        t = rng.integers(0, count, m)
        o.append(np.einsum("mk,mka->ma", bary, cv[t])), d.append(rng.normal(size=(m, 3)))
    m = k
    org = rng.uniform(lo, hi, (m, 3))                                              # axis-parallel
    ax = np.zeros((m, 3))
    ax[np.arange(m), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0], m)
    o.append(org), d.append(ax)
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d)
    d = _unit(d)
    ok = np.isfinite(d).all(1)
    return o[ok], d[ok]


def _dense_scene(pkg):
    """Cornell box plus two more small meshes after the walls: four clusters, 32 culled triangles (the cap)."""
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


@pytest.mark.parametrize("scene", ["cornell", "dense"])
def test_closest_hit_bit_equal_with_and_without_culling(pkg, monkeypatch, scene):
    s = pkg.host_scene.cornell_box(64, 64) if scene == "cornell" else _dense_scene(pkg)
    plan = pkg.binding.brute_cull_plan(s.xs, s.ys, s.zs, s.mat_id)
    assert len(plan) == (2 if scene == "cornell" else 4)
    o, d = _rays(s, plan, 1_200_000, 11 if scene == "cornell" else 12)
    assert o.shape[0] >= 1_000_000
    out = []
    for cull in (False, True):
        r = _ctx(pkg, monkeypatch, cull)
        try:
            r.upload_scene(s)
            out.append(r.test_closest_hit(o, d))
        finally:
            r.close()
    (i0, t0), (i1, t1) = out
    culled = np.zeros(i0.shape, bool)
    for first, count, _, _ in plan:
        culled |= (i0 >= first) & (i0 < first + count)
    assert culled.mean() > 0.05                      # the rays do reach the culled meshes
    assert np.array_equal(i0, i1)
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32))


def _film(pkg, monkeypatch, cull, scene, spp, env=False):
    r = _ctx(pkg, monkeypatch, cull)
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
def test_films_bit_equal_with_and_without_culling(pkg, monkeypatch, case):
    if case == "dense":
        s, spp = _dense_scene(pkg), 16
    else:
        s, spp = pkg.host_scene.cornell_box(256, 256), 64
    env = case == "cornell_env"
    a = _film(pkg, monkeypatch, False, s, spp, env)
    b = _film(pkg, monkeypatch, True, s, spp, env)
    assert np.isfinite(a[0]).all()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
