"""Motion blur on the GPU (dmt_set_motion): the sample times against the host twin, films untouched without
key 1, BVH == brute force under motion (hits and films), a hit at time t is the hit of the scene at t, the four kernel
rows against the single-sample probe, the width of the blur, schedule independence, and the refused combinations."""
import numpy as np
import pytest

import motion_ref as MR
from conftest import film_rmse
from test_lens_gpu import THETA, _quad_scene
from test_parity_gpu import _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu

F = np.float32
RMSE_TOL = 1e-3  # the project's parity bound between two arithmetics of one picture
OFF, FORCE = 0, 2
ERR_STATE = "(3)"


@pytest.fixture()
def ctx(pkg):
    """a context of the test's own: key 1 and the shutter are context state, and no other module's tests may inherit them"""
    r = pkg.Renderer(0)
    yield r
    r.close()


def _film(r, spp, offset=0):
    r.film_clear()
    r.render(spp, sample_offset=offset)
    r.sync()
    return r.download_film()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _cornell(O, res=32, deform=False):
    """the Cornell box and a key 1: the octahedra moved by about their own size (inside the box); deform adds a general,
    non-dyadic per-vertex deformation"""
    sc = O.cornell_box(res, res)
    k0, k1 = MR.cornell_keys(sc, offsets=((0.9, 0.3, 0.8), (-0.8, -0.4, 0.9)))
    if deform:
        T1 = MR.tris_of(*k1)
        moving = np.asarray(sc.mat_id) <= 1
        T1[moving] += np.random.default_rng(5).uniform(-0.11, 0.11, T1[moving].shape).astype(F)
        k1 = MR.soup(T1)
    return sc, k0, k1


class _Static:
    """a scene object with other positions"""
    def __init__(self, sc, k):
        self.__dict__.update({a: getattr(sc, a) for a in ("mat_id", "bsdfs", "lights", "inf_lights", "camera")})
        self.xs, self.ys, self.zs = k


# ---- 1. times ------------------------------------------------------------------------------------------
def test_shutter_times_equal_the_host_twin(ctx, pkg, O):
    ctx.set_camera(O.cornell_box(64, 64).camera)
    rng = np.random.default_rng(1)
    px, py = rng.integers(0, 64, 4096).astype(np.int32), rng.integers(0, 64, 4096).astype(np.int32)
    s = rng.integers(0, 4000, 4096).astype(np.int32)
    for open_, close in ((0.0, 1.0), (0.2, 0.7), (0.4, 0.4)):
        ctx.set_shutter(open_, close)
        assert ctx.test_shutter_times(px, py, s).tobytes() == pkg.shutter_times(64, 64, open_, close, px, py, s).tobytes()
    info = ctx.motion_info()
    assert (info["keys"], info["open"], info["close"]) == (0, F(0.4), F(0.4))


# ---- 2. nothing changes without key 1 ------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_films_without_key1_are_untouched(ctx, pkg, O, accel):
    sc, k0, k1 = _cornell(O)
    with pkg.Renderer(0) as plain:  # never sees a motion call
        plain.upload_scene(sc)
        plain.set_limits(6)
        plain.set_accel(accel)
        ref = _film(plain, 8)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_shutter(0.2, 0.7)
    assert _same(_film(ctx, 8), ref)
    ctx.set_motion(*k1)
    assert ctx.motion_info()["keys"] == 2
    moved = _film(ctx, 8)
    assert not _same(moved, ref)
    ctx.clear_motion()
    assert ctx.motion_info()["keys"] == 1
    assert _same(_film(ctx, 8), ref)
    ctx.set_camera(sc.camera)  # the shutter survives the camera and an upload
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
    assert (ctx.motion_info()["open"], ctx.motion_info()["close"]) == (F(0.2), F(0.7))


# ---- 3. BVH == brute force under motion: hits ----------------------------------------------------------
def _both(r, o, d, t):
    r.set_accel(0)
    a = r.test_closest_hit_at(o, d, t)
    r.set_accel(1)
    b = r.test_closest_hit_at(o, d, t)
    r.set_accel(0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    return a


def _aimed(pkg, k0, k1, t, origin, rng, n):
    """rays from `origin` at vertices and edge midpoints of n random triangles as they are at time t"""
    T = MR.tris_of(*pkg.motion_positions(*k0, *k1, float(t))).astype(np.float64)
    pick = T[rng.integers(0, T.shape[0], n)]
    targets = np.concatenate([pick.reshape(-1, 3), (pick + np.roll(pick, 1, axis=1)).reshape(-1, 3) / 2])
    d = targets - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.asarray(origin, F), (d.shape[0], 1)), d.astype(F)


@pytest.mark.parametrize("scene", ["cornell", "random300"])
def test_bvh_equals_brute_force_hits(ctx, pkg, O, scene):
    if scene == "cornell":
        sc, k0, k1 = _cornell(O, deform=True)
        origin = np.array([0.1, 0.2, 0.6])
    else:
        sc = O.cornell_box(32, 32)
        k0, k1 = MR.random_keys(300)
        origin = np.array([0.0, -1.5, 0.0])
    n = k0[0].size // 4
    ctx.upload_triangles(*k0, np.zeros(n, np.uint32) if scene != "cornell" else sc.mat_id)
    ctx.set_motion(*k1)
    rng = np.random.default_rng(17)
    os_, ds, ts = [], [], []
    for t in (0.0, 1.0, 0.375, float(F(rng.uniform())), float(F(rng.uniform()))):
        o, d = _aimed(pkg, k0, k1, t, origin, rng, 100)
        os_.append(o), ds.append(d), ts.append(np.full(o.shape[0], t, F))
    d = rng.normal(size=(2048, 3))  # and random directions at random times, from inside the scene
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    os_.append(np.tile(np.array([0.0, 2.0, 0.5], F), (2048, 1))), ds.append(d.astype(F)), ts.append(rng.uniform(0, 1, 2048).astype(F))
    o, d, t = np.concatenate(os_), np.concatenate(ds), np.concatenate(ts)
    assert o.shape[0] >= 4096
    tri, tt, uv = _both(ctx, o, d, t)
    assert (tri >= 0).mean() > 0.5 and np.isinf(tt[tri < 0]).all()
    assert len(np.unique(tri[tri >= 0])) > 8
    info = ctx.motion_info()
    assert info["tree_nodes"] >= 1 and (n + 1) // 2 <= info["tree_pairs"] <= n and info["tree_build_ms"] > 0
    # dmt_test_closest_hit keeps answering for key 0
    i0, t0 = ctx.test_closest_hit(o, d)
    ia, ta, _ = ctx.test_closest_hit_at(o, d, 0.0)
    assert np.array_equal(i0, ia) and np.array_equal(t0.view(np.uint32), ta.view(np.uint32))


@pytest.mark.parametrize("nfloor", [1, 2, 3])
def test_axis_parallel_rays_on_a_moving_floor(ctx, nfloor):
    """test_bvh_empty_slots_axis_parallel_rays' flat floor with a displaced key 1: the empty slots of its node 'hit' under
    axis-parallel rays, and their implicit references must stay inside the pair AND the delta array (guard records)."""
    k0, k1 = MR.floor_keys(nfloor)
    ctx.upload_triangles(*k0, np.zeros(nfloor, np.uint32))
    ctx.set_motion(*k0)  # zero displacement first: the node is flat, as in the static test
    g = np.linspace(-1.5, 3.5, 41, dtype=F)
    gx, gz = np.meshgrid(g, g)
    n = gx.size
    o = np.stack([gx.ravel(), np.full(n, 5.0, F), gz.ravel()], axis=1).astype(F)
    d = np.tile(np.array([0.0, -1.0, 0.0], F), (n, 1))
    o = np.concatenate([o, o * np.array([1, -1, 1], F), np.stack([np.full(n, -9.0, F), gz.ravel() * 0, gx.ravel()], axis=1)])
    d = np.concatenate([d, -d, np.tile(np.array([1.0, 0.0, 0.0], F), (n, 1))])
    t = np.random.default_rng(2).choice(np.array([0.0, 0.5, 1.0, 0.3], F), o.shape[0])
    tri, _, _ = _both(ctx, o, d, t)
    assert (tri >= 0).sum() > 100
    ctx.set_motion(*k1)
    tri, _, _ = _both(ctx, o, d, t)
    assert (tri >= 0).sum() > 100
    tri, _, _ = _both(ctx, o, d, np.zeros(o.shape[0], F))  # a flat node again, inside a tree of thick boxes
    assert (tri >= 0).sum() > 100


# ---- 4. BVH == brute force under motion: films ---------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 16])
@pytest.mark.parametrize("env", [False, True])
def test_bvh_equals_brute_force_films(ctx, pkg, O, env, chunk):
    sc, k0, k1 = _cornell(O, deform=True)
    if env:
        sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_motion(*k1)
    ctx.set_chunk(chunk)
    films = []
    for accel in (0, 1):
        ctx.set_accel(accel)
        films.append(_film(ctx, 16))
    assert _same(*films)
    assert np.isfinite(films[0][0]).all() and films[0][0][..., :3].max() > 0
    assert np.array_equal(films[0][1][..., 3], np.full((32, 32), 16, F))


# ---- 5. a hit is the hit of the scene at that time: the exact case -------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_hit_at_time_is_the_static_hit_exact_case(ctx, pkg, accel):
    """Vertices and per-triangle translations on a 2^-6 grid, times 0.25 and 0.5: fmaf(t, D, A) and the record packed from
    motion_positions(t) are the same numbers, so the hits agree bit for bit."""
    k0, k1 = MR.random_keys(300, seed=21, grid=2.0 ** -6)
    mat = np.zeros(300, np.uint32)
    rng = np.random.default_rng(4)
    d = np.array([0.0, 4.5, 0.0]) + rng.uniform(-2.5, 2.5, (4096, 3))  # from outside, into the cloud of triangles around (0, 3, 0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([0.0, -1.5, 0.0], F), (4096, 1))
    for tau in (0.25, 0.5):
        ctx.upload_triangles(*k0, mat)
        ctx.set_motion(*k1)
        ctx.set_accel(accel)
        tri, tt, _ = ctx.test_closest_hit_at(o, d.astype(F), tau)
        ctx.upload_triangles(*pkg.motion_positions(*k0, *k1, tau), mat)  # (drops key 1)
        assert ctx.motion_info()["keys"] == 1
        i1, t1 = ctx.test_closest_hit(o, d.astype(F))
        assert np.array_equal(tri, i1) and np.array_equal(tt.view(np.uint32), t1.view(np.uint32))
        assert (tri >= 0).sum() > 1000


# ---- 6. a film is the film of the scene at that time ---------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_film_at_one_time_is_the_static_film(ctx, pkg, O, accel):
    """Shutter [tau, tau] under a general deformation against the static film of motion_positions(tau): only the normal's
    last bits and the edge rounding differ.  Observed on MI355X (32 x 32 x 64 spp, depth 6): see DESIGN.md 4.14."""
    tau = 0.6
    sc, k0, k1 = _cornell(O, deform=True)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    key0 = _film(ctx, 64)
    ctx.set_motion(*k1)
    ctx.set_shutter(tau, tau)
    moving = _film(ctx, 64)
    ctx.upload_scene(_Static(sc, pkg.motion_positions(*k0, *k1, tau)))
    static = _film(ctx, 64)
    near, far = film_rmse(moving[0], static[0]), film_rmse(moving[0], key0[0])
    print(f"accel {accel}: film at tau against the static film of motion_positions(tau): {near:.3e}; against key 0: {far:.3e}")
    assert near < RMSE_TOL
    assert far > 1e-2


# ---- 7. the kernel table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("env", [False, True])
def test_trace_samples_run_the_motion_rows(ctx, pkg, O, env, accel):
    sc, k0, k1 = _cornell(O, deform=True)
    if env:
        sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_motion(*k1)
    s = 5
    ctx.film_clear()
    ctx.render(1, sample_offset=s)
    ctx.sync()
    mean, m2 = ctx.download_film()
    idx = np.random.default_rng(3).choice(32 * 32, 64, replace=False)
    px, py = (idx % 32).astype(np.int32), (idx // 32).astype(np.int32)
    L = ctx.test_trace_samples(px, py, np.full(64, s, np.int32))
    assert np.array_equal(m2[py, px, 3], np.ones(64, F))
    assert np.isfinite(L).all() and L.max() > 0
    assert np.array_equal(L, mean[py, px, :3]), np.abs(L - mean[py, px, :3]).max()
    if not env and accel == 0:  # the logged path is the same sample
        for i in range(8):
            rec, Llog = ctx.test_trace_log(int(px[i]), int(py[i]), s)
            assert rec.shape[0] >= 1 and np.array_equal(Llog, L[i]), (i, Llog, L[i])


# ---- 8. the blur has the predicted width ---------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_blur_has_the_predicted_width(ctx, pkg, O, accel):
    depth = 4.0
    q = _quad_scene(pkg, depth, 4.5, 0.37 * THETA * depth)
    sc = pkg.host_scene.ArrayScene(q.xs, q.ys, q.zs, q.mat_id, q.bsdfs, q.lights, O.cornell_box(64, 64).inf_lights, q.camera)
    k0 = (np.asarray(sc.xs, F).reshape(-1), np.asarray(sc.ys, F).reshape(-1), np.asarray(sc.zs, F).reshape(-1))
    T1 = MR.tris_of(*k0)
    T1[..., 0] += F(12 * THETA * depth)
    ctx.upload_scene(sc)
    ctx.set_limits(0)  # a pixel's mean = its miss fraction times the environment's value
    ctx.set_accel(accel)
    ctx.set_motion(*MR.soup(T1))

    def coverage():
        mean = _film(ctx, 64)[0][..., :3]
        env = mean[:, 0].mean(0)  # the leftmost column never sees the quad
        assert (env > 0).all() and np.array_equal(mean[:, 0], np.tile(env, (64, 1)))
        return 1.0 - (mean / env).mean(2).mean(0)  # per column: 64 rows x 64 samples

    col = coverage()
    partial = np.nonzero((col > 1e-6) & (col < 1 - 1e-6))[0]
    print(f"accel {accel}: partially covered columns {partial.min()}..{partial.max()} ({partial.size})")
    # Raster coordinate fx sees x = depth * THETA * (fx - 31.5) (pixel centres at half-integers, 64 columns), and the samples of
    # column c have fx in [c, c + 1).  The edge sweeps from fx = 31.87 to 43.87: column c is covered where t < (fx - 31.87) / 12.
    assert abs(partial.size - 13) <= 1 and partial.min() >= 30 and partial.max() <= 44
    assert (np.abs(col[:30]) < 1e-6).all() and (np.abs(col[45:] - 1) < 1e-6).all()  # 0 and 1 beyond the swept band
    interior = np.arange(32, 43)
    ramp = (interior + 0.5 - 31.87) / 12
    dev = np.abs(col[interior] - ramp).max()
    print(f"largest deviation from the linear ramp on the eleven interior columns: {dev:.4f} (bound 0.047)")
    assert dev <= 6 * np.sqrt(0.25 / 4096)
    ctx.render_aovs(64)
    ctx.sync()
    cov = ctx.download_aovs()[0][..., 3].mean(0)
    aov_partial = int(((cov > 0) & (cov < 1)).sum())
    assert abs(aov_partial - 13) <= 1 and np.abs(cov[interior] - ramp).max() <= 6 * np.sqrt(0.25 / 4096)
    ctx.set_shutter(0.0, 0.0)
    col0 = coverage()
    assert int(((col0 > 1e-6) & (col0 < 1 - 1e-6)).sum()) == 1


# ---- 9. films do not depend on the schedule ------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_films_do_not_depend_on_the_schedule(ctx, pkg, O, accel):
    sc, k0, k1 = _cornell(O, deform=True)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_motion(*k1)
    ctx.set_shutter(0.1, 0.9)
    ctx.set_sampler_table(OFF)
    ref = _film(ctx, 16)
    ctx.set_sampler_table(FORCE)
    assert _same(_film(ctx, 16), ref)
    ctx.set_sampler_table(OFF)
    ctx.film_clear()  # two halves of the sample range
    ctx.render(8)
    ctx.render(8, sample_offset=8)
    ctx.sync()
    assert _same(ctx.download_film(), ref)
    # Sample by sample: a 1-spp call gives no lane a second sample, while in the calls above a lane that parks a finished
    # sample's last shadow ray starts the next sample beside it -- two rays of two times in one pass.
    ctx.film_clear()
    for k in range(16):
        ctx.render(1, sample_offset=k)
    ctx.sync()
    assert _same(ctx.download_film(), ref)
    ctx.film_clear()  # two partitions
    for rank in (0, 1):
        ctx.set_partition(rank, 2)
        ctx.render(16)
    ctx.set_partition(0, 1)
    ctx.sync()
    assert _same(ctx.download_film(), ref)
    ctx.film_clear()  # adaptive rounds that stop no pixel: every pixel is below min_spp until the last round
    rounds, _ = ctx.render_adaptive(0.0, 16, 4, min_spp=16)
    assert rounds == 4
    assert _same(ctx.download_film(), ref)


# ---- 10. refusals, and what drops key 1 ----------------------------------------------------------------
def _refused(pkg, call, *words):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_STATE in msg and "motion" in msg and all(w in msg for w in words), msg


def test_refused_combinations(ctx, pkg, O):
    sc, k0, k1 = _cornell(O)
    render = lambda: ctx.render(1)
    # emissive triangles
    ctx.upload_scene(sc)
    ctx.set_motion(*k1)
    ctx.upload_area_lights([20], [[5, 5, 5]])
    _refused(pkg, render, "emissive")
    ctx.upload_area_lights([], np.zeros((0, 3), F))
    render()
    # counting kernels
    ctx.set_accel(1)
    _refused(pkg, lambda: ctx.render_stats(1), "dmt_render_stats")
    _refused(pkg, lambda: ctx.render_profile(1), "dmt_render_profile")
    # wavefront form
    ctx.set_bvh_strategy(2)
    _refused(pkg, render, "wavefront")
    ctx.set_bvh_strategy(0)
    render()
    ctx.set_accel(0)
    # light trees
    many = _many_lights_cornell(O, pkg, 32)
    ctx.upload_scene(many)
    ctx.set_motion(many.xs, many.ys, many.zs)
    for mode in (1, 2):
        ctx.set_light_sampling(mode)
        _refused(pkg, render, "light tree")
    ctx.set_light_sampling(0)
    render()
    # textures, and the texture filter on top of them
    tex = _textured_cornell(O, pkg, 32)
    ctx.upload_scene(tex)
    ctx.set_motion(tex.xs, tex.ys, tex.zs)
    _refused(pkg, render, "textures")
    ctx.set_texture_filter(pkg.TEXFILTER_REFERENCE)
    _refused(pkg, render, "texture filter")
    ctx.set_texture_filter(pkg.TEXFILTER_LEVEL0)
    ctx.clear_motion()
    render()
    ctx.sync()


def test_argument_and_state_errors(ctx, pkg, O):
    sc, k0, k1 = _cornell(O)
    with pytest.raises(pkg.DmtError, match=r"\(3\)"):  # before any upload
        ctx.set_motion(*k1)
    ctx.upload_scene(sc)
    with pytest.raises(pkg.DmtError, match=r"\(1\)"):  # another triangle count
        ctx.set_motion(*(a[:-4] for a in k1))
    bad = [a.copy() for a in k1]
    bad[1][5] = np.nan
    with pytest.raises(pkg.DmtError, match=r"\(1\)"):
        ctx.set_motion(*bad)
    for open_, close in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.1), (float("nan"), 1.0)):
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):
            ctx.set_shutter(open_, close)
    with pytest.raises(pkg.DmtError, match=r"\(3\)"):  # no key 1
        ctx.test_closest_hit_at(np.zeros((1, 3), F), np.ones((1, 3), F), 0.5)
    assert ctx.motion_info()["keys"] == 1


@pytest.mark.parametrize("accel", [0, 1])
def test_update_vertices_drops_key1(ctx, pkg, O, accel):
    sc, k0, k1 = _cornell(O)
    new = pkg.motion_positions(*k0, *k1, 0.5)
    with pkg.Renderer(0) as plain:
        plain.upload_scene(_Static(sc, new))
        plain.set_limits(6)
        plain.set_accel(accel)
        ref = _film(plain, 8)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_motion(*k1)
    assert ctx.motion_info()["keys"] == 2
    ctx.update_vertices(*new)
    info = ctx.motion_info()
    assert (info["keys"], info["tree_nodes"], info["tree_pairs"]) == (1, 0, 0)
    assert _same(_film(ctx, 8), ref)
