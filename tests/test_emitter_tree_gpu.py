"""The emitter tree on the DEVICE (dmt_set_emitter_sampling; csrc/emitter_tree.hpp, the *_etree rows of DMT_MEGAKERNELS).

Selection: dmt_test_emitter_tree runs et_select / et_pmf as the kernels compile them, on the tree the context uploaded, over
the inputs of tests/test_emitter_tree.py (64 shading points x 256 values of u per set), against the float64 twin of
tests/emitter_tree_f64.py: the same exclusion rule (EPS = 1e-6) and cap (1 % per set); compared cases select the twin's
emitter; probabilities within DEVICE_FACTOR = 4 x the host-fp32-against-float64 errors measured there (the project's rule: the
device's divide and sqrt are 2.5-ulp operations instead of 0.5-ulp and its products contract, see
tests/test_light_tree_select_gpu.py); pmf_by_trail == pmf bit for bit.

Films: nothing moves while the mode is not set or does not apply (byte-identical films); with the tree the image converges
to the uniform rows' (the z rule of test_light_tree_converges_to_the_uniform_image) with less variance; brute force and BVH
give bit-identical films; the fall-backs and refusals; the rows' resources.

Measured on an MI355X: device against float64 at most 1.59e-6 absolute and 3.98e-5 relative (bounds 7.6e-6 and 1.72e-4), at most
0.37 % of a set excluded; z rule 99th percentile 1.60 and mean 0.47 at 2 048 spp, 2.15 and 0.57 with an env map at 256 spp; mean
M2 of the tree film 0.82 of the uniform film's.  The whole module runs in about a second of GPU time.
"""
import ctypes as C

import numpy as np
import pytest

import emitter_tree_f64 as F64
import test_emitter_tree as T
import test_light_tree_select as TLS

pytestmark = pytest.mark.gpu

ABS_BOUND, REL_BOUND = T.DEVICE_FACTOR * T.HOST_ABS, T.DEVICE_FACTOR * T.HOST_REL


@pytest.fixture
def ctx(renderer, O):
    """The session's context with a Cornell box under it; defaults again afterwards, and no emissive triangles."""
    renderer.upload_scene(O.cornell_box(16, 16))
    renderer.set_limits(4)
    renderer.set_accel(0)
    renderer.set_partition(0, 1)
    renderer.set_light_sampling(0)
    renderer.set_emitter_sampling(0)
    yield renderer
    renderer.set_emitter_sampling(0)
    renderer.set_light_sampling(0)
    renderer.set_bvh_strategy(0)
    renderer.set_accel(0)
    renderer.upload_scene(O.cornell_box(16, 16))


def upload_set(r, S):
    """The emitters of a set of tests/test_emitter_tree.py under the context's materials and camera."""
    r.upload_triangles(S.xs, S.ys, S.zs, np.zeros(len(S.verts), np.uint32))
    r.upload_lights(S.lights, [])
    r.upload_area_lights(S.area_tri, S.area_le)


def probe(r, p, nrm, u, start=1.0):
    return r.test_emitter_tree(*TLS.flat(p, nrm, u), start)


def check_set(pkg, name, S, p, nrm, u, got, start=1.0):
    nodes = pkg.emitter_tree_nodes(*S.args())[0]
    part = F64.intervals(nodes, p, nrm)
    share, a, r = T.compare(name, part, u, got, start)
    print(f"emitter tree {name}: excluded {100 * share:.4f} %, device vs float64 pmf abs {a:.3e} (bound {ABS_BOUND:.3e}) rel {r:.3e} (bound {REL_BOUND:.3e})")
    assert share <= T.EXCLUDED_CAP, (name, share)
    assert a <= ABS_BOUND and r <= REL_BOUND, (name, a, r)


# ---- 5. device selection -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.SETS)
def test_device_selection_against_float64(ctx, pkg, name):
    S, p, nrm, u = T.cases(pkg, name)
    upload_set(ctx, S)
    ctx.set_emitter_sampling(1)
    got = probe(ctx, p, nrm, u)
    check_set(pkg, name, S, p, nrm, u, got)
    T.check_strata(name, got)
    half = probe(ctx, p, nrm, u, 0.5)
    assert np.array_equal(half[0], got[0])
    assert np.array_equal(half[1], np.float32(0.5) * got[1]) and np.array_equal(half[2], np.float32(0.5) * got[2])   # exactly: a power of two
    info = ctx.emitter_tree_info()
    assert info["mode"] == 1 and info["active"] and info["emitters"] == S.count and info["nodes"] == 2 * S.count - 1
    assert info["depth"] == pkg.emitter_tree_nodes(*S.args())[3]


def test_probe_is_refused_where_the_tree_is_not_active(ctx, pkg):
    S, p, nrm, u = T.cases(pkg, "n17")
    upload_set(ctx, S)
    with pytest.raises(pkg.DmtError, match="uniformly"):
        probe(ctx, p, nrm, u)
    assert not ctx.emitter_tree_info()["active"]
    ctx.set_emitter_sampling(1)
    ctx.upload_area_lights([], np.zeros((0, 3), np.float32))
    with pytest.raises(pkg.DmtError, match="no emissive triangles"):
        probe(ctx, p, nrm, u)
    info = ctx.emitter_tree_info()
    assert info["mode"] == 1 and not info["active"] and info["emitters"] == 0
    ctx.upload_area_lights(S.area_tri, S.area_le)
    H = pkg.host_scene.load_host_library()
    f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
    distant = np.zeros(32, np.uint8)
    H.dmt_host_make_directional_light(f3([0.4, 0.4, 0.3]), f3([0.2, 0.6, -0.7]), C.c_float(0.0), distant.ctypes.data_as(C.c_void_p))
    ctx.upload_lights(np.concatenate([S.lights, distant[None]]), [])
    with pytest.raises(pkg.DmtError, match="directional"):
        probe(ctx, p, nrm, u)
    assert not ctx.emitter_tree_info()["active"]
    ctx.upload_lights(S.lights, [])
    assert probe(ctx, p, nrm, u)[0].max() >= 0                          # and answers again once the tree applies
    with pytest.raises(pkg.DmtError, match="unknown mode"):
        ctx.set_emitter_sampling(2)
    assert ctx.emitter_tree_info()["mode"] == 1                          # a refused mode changes nothing


def test_probe_follows_uploads_vertex_updates_and_the_mode(ctx, pkg):
    """The tree the probe walks is rebuilt after dmt_upload_area_lights, dmt_upload_lights, dmt_update_vertices and a mode
    round trip; rebuilt answers equal a fresh context's."""
    A, pa, na, u = T.cases(pkg, "n17")
    B, pb, nb, _ = T.cases(pkg, "n64")

    def fresh(S, p, nrm):
        with pkg.Renderer(0) as r:
            upload_set(r, S)
            r.set_emitter_sampling(1)
            return probe(r, p, nrm, u)

    same = lambda x, y: all(np.array_equal(a, b) for a, b in zip(x, y))
    upload_set(ctx, A)
    ctx.set_emitter_sampling(1)
    first = probe(ctx, pa, na, u)
    assert same(first, fresh(A, pa, na))
    # fewer emissive triangles
    A2 = T.Scene(A.lights, A.verts, A.area_tri[:5], A.area_le[:5])
    ctx.upload_area_lights(A2.area_tri, A2.area_le)
    got = probe(ctx, pa, na, u)
    assert got[0].max() < A2.count and same(got, fresh(A2, pa, na))
    # fewer lights
    A3 = T.Scene(A.lights[:2], A.verts, A2.area_tri, A2.area_le)
    ctx.upload_lights(A3.lights, [])
    assert same(probe(ctx, pa, na, u), fresh(A3, pa, na))
    # moved vertices
    moved = A.verts + np.array([0.25, -0.5, 0.125], np.float32)
    A4 = T.Scene(A3.lights, moved, A3.area_tri, A3.area_le)
    ctx.update_vertices(A4.xs, A4.ys, A4.zs)
    got = probe(ctx, pa, na, u)
    assert not same(got, fresh(A3, pa, na)) and same(got, fresh(A4, pa, na))
    # a mode round trip, and a new soup
    ctx.set_emitter_sampling(0)
    with pytest.raises(pkg.DmtError, match="uniformly"):
        probe(ctx, pa, na, u)
    ctx.set_emitter_sampling(1)
    assert same(probe(ctx, pa, na, u), got)
    upload_set(ctx, B)
    got = probe(ctx, pb, nb, u)
    assert got[0].max() >= 17 and same(got, fresh(B, pb, nb))
    check_set(pkg, "n64", B, pb, nb, u, got)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def add_triangles(sc, tris, mat=0):
    """Triangles [k,3,3] appended to a scene's soup -> their indices."""
    t = np.asarray(tris, np.float32)
    first = sc.tri_count
    pad = lambda a: np.concatenate([a, np.zeros((len(a), 1), np.float32)], 1)
    sc.xs, sc.ys, sc.zs = (np.concatenate([old, pad(t[:, :, k])]) for k, old in enumerate((sc.xs, sc.ys, sc.zs)))
    sc.mat_id = np.concatenate([sc.mat_id, np.full(len(t), mat, np.uint32)])
    return first + np.arange(len(t))


def cornell_with_emitters(O, pkg, res, n_tri=128, n_lights=8, seed=11):
    """The Cornell box (x, z in [-2, 2], y in [0, 4], seen from y = 0; z up) with about 128 small emissive triangles near the
    ceiling and on the wall x = -2, radiances over three decades, a third of them facing away from the room, and 8 point lights
    of radius 2e-4."""
    sc = O.cornell_box(res, res)
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    m = n_tri // 2
    ceil_c = np.stack([rng.uniform(-1.8, 1.8, m), rng.uniform(0.6, 3.8, m), rng.uniform(1.55, 1.9, m)], 1)
    wall_c = np.stack([rng.uniform(-1.9, -1.6, n_tri - m), rng.uniform(0.6, 3.8, n_tri - m), rng.uniform(-1.5, 1.5, n_tri - m)], 1)
    centre = np.concatenate([ceil_c, wall_c])
    into_room = np.concatenate([np.tile([0.0, 0.0, -1.0], (m, 1)), np.tile([1.0, 0.0, 0.0], (n_tri - m, 1))])
    away = rng.uniform(size=n_tri) < 1 / 3
    normal = unit(np.where(away[:, None], -into_room, into_room) + rng.normal(scale=0.35, size=(n_tri, 3)))
    e0 = unit(np.cross(normal, unit(rng.normal(size=(n_tri, 3)))))
    e1 = np.cross(normal, e0)                                            # cross(e0, e1) = normal
    size = rng.uniform(0.04, 0.14, (n_tri, 1))
    tris = np.stack([centre, centre + size * e0, centre + size * e1], 1)
    le = (10.0 ** rng.uniform(0.0, 3.0, (n_tri, 1))) * rng.uniform(0.4, 1.0, (n_tri, 3))
    idx = add_triangles(sc, tris, int(sc.mat_id[0]))
    sc.set_area_lights(idx, le)
    pos = np.stack([rng.uniform(-1.7, 1.7, n_lights), rng.uniform(0.8, 3.6, n_lights), rng.uniform(-1.0, 1.8, n_lights)], 1)
    sc.lights = T.make_lights(pkg, n_lights, rng, positions=pos)
    for i in range(n_lights):                                            # intensities over three decades too
        rgb = sc.lights[i, 0:6].copy().view(np.float16).astype(np.float32) * np.float32(10.0 ** rng.uniform(-2.0, 1.0))
        sc.lights[i, 0:6] = rgb.astype(np.float16).view(np.uint8)
    return sc


def env_image():
    v, h = np.meshgrid(np.linspace(0.0, 1.0, 8), np.linspace(0.0, 1.0, 16), indexing="ij")
    return np.stack([0.3 + 0.6 * v, 0.25 + 0.5 * h, 0.5 + 0.3 * v * h], 2).astype(np.float32)


def film(r, spp):
    r.film_clear()
    r.render(spp)
    r.sync()
    return r.download_film()


def identical(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 6. nothing moves by default ---------------------------------------------------------------------------------------------
def test_films_do_not_move_unless_the_tree_is_on(ctx, pkg, O):
    sc = cornell_with_emitters(O, pkg, 32, n_tri=24)
    with pkg.Renderer(0) as r:                                           # the mode never set
        r.upload_scene(sc)
        r.set_limits(4)
        never = film(r, 8)
    ctx.upload_scene(sc)
    base = film(ctx, 8)
    assert identical(never, base) and float(base[0][..., :3].mean()) > 1e-3
    ctx.set_emitter_sampling(1)
    assert ctx.emitter_tree_info()["active"]
    tree = film(ctx, 8)
    assert not identical(tree, base) and np.isfinite(tree[0]).all()
    ctx.set_emitter_sampling(0)
    assert identical(film(ctx, 8), base)                                 # and back
    # without emissive triangles the mode changes nothing, whatever dmt_set_light_sampling says
    ctx.upload_area_lights([], np.zeros((0, 3), np.float32))
    for mode in (0, 1, 2):
        ctx.set_light_sampling(mode)
        ctx.set_emitter_sampling(0)
        uniform = film(ctx, 8)
        ctx.set_emitter_sampling(1)
        assert not ctx.emitter_tree_info()["active"]
        assert identical(film(ctx, 8), uniform), mode


# ---- 7. unbiased, and worth it -----------------------------------------------------------------------------------------------
def z_rule(uniform, tree, spp):
    (um, um2), (tm, tm2) = uniform, tree
    se = np.sqrt(np.maximum(um2[..., :3], 0)) / spp + np.sqrt(np.maximum(tm2[..., :3], 0)) / spp   # standard errors of both means
    z = np.abs(um[..., :3] - tm[..., :3]) / np.maximum(se, 1e-9)
    return float(np.percentile(z, 99)), float(z.mean())


def test_the_tree_converges_to_the_uniform_image_with_less_variance(ctx, pkg, O):
    """2 048 spp with the tree against 2 048 spp with the uniform rows, 48 x 48 pixels, brute force, depth 4: per-pixel
    z = |difference of the means| / (sum of their standard errors), 99th percentile < 5 and mean < 1.5; the tree film's mean M2
    is below the uniform film's (measured ratio: DESIGN.md 4.20).  The same with an env map at 256 spp."""
    sc = cornell_with_emitters(O, pkg, 48)
    ctx.upload_scene(sc)
    uniform = film(ctx, 2048)
    ctx.set_emitter_sampling(1)
    assert ctx.emitter_tree_info()["active"] and ctx.emitter_tree_info()["emitters"] == 136
    tree = film(ctx, 2048)
    p99, mean = z_rule(uniform, tree, 2048)
    ratio = float(tree[1][..., :3].mean()) / float(uniform[1][..., :3].mean())
    print(f"emitter tree vs uniform, 2048 spp: z p99 {p99:.3f} mean {mean:.3f}; mean M2 tree / uniform = {ratio:.4f}")
    assert p99 < 5.0 and mean < 1.5, (p99, mean)
    assert ratio < 1.0, ratio
    sc.set_envmap(env_image())
    ctx.upload_scene(sc)
    tree = film(ctx, 256)
    ctx.set_emitter_sampling(0)
    uniform = film(ctx, 256)
    p99, mean = z_rule(uniform, tree, 256)
    print(f"emitter tree vs uniform with an env map, 256 spp: z p99 {p99:.3f} mean {mean:.3f}")
    assert p99 < 5.0 and mean < 1.5, (p99, mean)


# ---- 8. brute force = BVH ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True])
def test_brute_force_and_bvh_films_are_bit_identical_under_the_tree(ctx, pkg, O, env):
    sc = cornell_with_emitters(O, pkg, 32)
    if env:
        sc.set_envmap(env_image())
    ctx.upload_scene(sc)
    ctx.set_emitter_sampling(1)
    brute = film(ctx, 8)
    ctx.set_accel(1)
    assert ctx.emitter_tree_info()["active"]
    assert identical(film(ctx, 8), brute)
    assert np.isfinite(brute[0]).all() and float(brute[0][..., :3].mean()) > 1e-3


# ---- 9. fall-backs and refusals ----------------------------------------------------------------------------------------------
def test_a_tree_deeper_than_the_guard_renders_with_the_uniform_rows(ctx, pkg, O):
    fits, deep = T.chain_lengths(pkg)
    films = {}
    for n in (deep, fits):
        sc = O.cornell_box(32, 32)
        # in the plane of the camera, facing into the box, its near end inside.  x = 1.5^i 2^-14, from 6e-5 to 2e6: over the
        # 60 octaves of the host test's chain the smallest triangles' pdfs, squared by the power heuristic, overflow fp32 and
        # the largest triangles' normals do, in the uniform rows as well
        C_ = T.chain(pkg, n, k=14, ratio=1.5)
        assert pkg.emitter_tree_nodes(*C_.args())[3] == n
        sc.lights = np.zeros((0, 32), np.uint8)                         # the chain alone: one more emitter would change its tree
        idx = add_triangles(sc, C_.verts, int(sc.mat_id[0]))
        sc.set_area_lights(idx, C_.area_le)
        ctx.upload_scene(sc)
        ctx.set_emitter_sampling(0)
        uniform = film(ctx, 8)
        ctx.set_emitter_sampling(1)
        films[n] = (uniform, film(ctx, 8))
        info = ctx.emitter_tree_info()
        if n == deep:
            assert "uniform pick" in ctx.last_error() and str(deep) in ctx.last_error() and "emitter tree" in ctx.last_error()
            assert info["mode"] == 1 and not info["active"] and info["depth"] == deep and info["emitters"] == deep
            with pytest.raises(pkg.DmtError, match="too deep"):
                ctx.test_emitter_tree([[0.0, 2.0, 0.0]], [[0.0, 0.0, 1.0]], [0.5])
        else:
            assert info["active"] and info["depth"] == fits
    assert np.isfinite(films[deep][0][0]).all() and identical(*films[deep]) and float(films[deep][0][0][..., :3].mean()) > 1e-3
    assert not identical(*films[fits]) and np.isfinite(films[fits][1][0]).all()


def test_a_directional_light_in_the_list_keeps_the_uniform_rows(ctx, pkg, O):
    sc = cornell_with_emitters(O, pkg, 32, n_tri=24)
    H = pkg.host_scene.load_host_library()
    f3 = lambda v: np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)
    distant = np.zeros(32, np.uint8)
    H.dmt_host_make_directional_light(f3([0.4, 0.4, 0.3]), f3([0.2, 0.6, -0.7]), C.c_float(0.0), distant.ctypes.data_as(C.c_void_p))
    sc.lights = np.concatenate([sc.lights, distant[None]])
    ctx.upload_scene(sc)
    uniform = film(ctx, 8)
    ctx.set_emitter_sampling(1)
    info = ctx.emitter_tree_info()
    assert info["mode"] == 1 and not info["active"]
    assert identical(film(ctx, 8), uniform)


def test_the_wavefront_form_and_the_counting_kernels_are_refused(ctx, pkg, O):
    sc = cornell_with_emitters(O, pkg, 32, n_tri=24)
    ctx.upload_scene(sc)
    ctx.set_emitter_sampling(1)
    ctx.set_accel(1)
    ctx.set_bvh_strategy(2)
    with pytest.raises(pkg.DmtError, match="emitter tree.*wavefront"):
        ctx.render(8)
    ctx.set_bvh_strategy(0)
    with pytest.raises(pkg.DmtError, match="emitter tree.*no counting kernels"):
        ctx.render_stats(8)
    ctx.set_emitter_sampling(0)
    ctx.set_bvh_strategy(2)
    ctx.film_clear()
    ctx.render(8)                                                        # the *_area rows have a wavefront form
    ctx.sync()


# ---- 10. rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel,env,waves", [(0, False, 3), (1, False, 2), (0, True, 3), (1, True, 2)])
def test_the_new_rows_use_no_scratch_at_their_launch_bounds(ctx, pkg, O, accel, env, waves):
    """k_megakernel_area_etree / _bvh_area_etree / _env_area_etree / _bvh_env_area_etree: no scratch, and the waves per SIMD
    DMT_MEGAKERNELS states for them (3 / 2 / 3 / 2; a block of 256 threads is one wave per SIMD)."""
    sc = cornell_with_emitters(O, pkg, 16, n_tri=24)
    if env:
        sc.set_envmap(env_image())
    ctx.upload_scene(sc)
    ctx.set_accel(accel)
    twin = ctx.kernel_info()
    ctx.set_emitter_sampling(1)
    info = ctx.kernel_info()
    print(f"accel {accel} env {env}: twin {twin}, etree {info}, scratch {ctx.kernel_scratch()}")
    assert ctx.kernel_scratch() == 0
    assert info["blocks_per_cu"] >= waves and info["vgprs"] <= 512 // waves
    assert info["lds_bytes"] == twin["lds_bytes"] + 6 * 256 * 4          # the previous vertex: six floats per lane
