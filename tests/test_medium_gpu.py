"""The participating medium on the GPU (dmt_set_medium): the device arithmetic against the host twins and
float64, films untouched without a medium, BVH == brute force under every schedule, and four closed forms -- the exact
attenuation of a delta light through a slab, the free-flight pass probability, single scattering against quadrature, and
the white furnace -- then the lens, adaptive rounds and the refused combinations.  Every group runs on a context of its own."""
import numpy as np
import pytest

import medium_ref as MR
from test_parity_gpu import _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu

F = np.float32
OFF, FORCE = 0, 2
ERR_STATE = "(3)"
# inside the Cornell box (x, z in [-2, 2], y in [0, 4], the camera at the origin looking along +y): rays enter and leave it
FOG = dict(sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))


@pytest.fixture()
def ctx(pkg):
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


# ---- 1. the probe --------------------------------------------------------------------------------------------
def test_device_arithmetic(ctx, pkg):
    rng = np.random.default_rng(5)
    n = 65536
    lo, hi, sigma, g = (-1.0, 0.5, -0.25), (2.0, 1.5, 0.75), 1.5, 0.6
    o = rng.uniform(-4, 4, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d[: n // 2] = rng.uniform(lo, hi, (n // 2, 3)) - o[: n // 2]  # half of them aimed at the box
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o[:64], d[:64] = (-5, 1.5, 0.25), (1, 0, 0)                   # axis-parallel, in a face plane
    t_hit = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0, 8, n)).astype(F)
    h, depth = rng.integers(0, 2 ** 31, n).astype(np.uint32), rng.integers(0, 9, n).astype(np.uint32)
    cosine, u = rng.uniform(-1, 1, n).astype(F), rng.uniform(0, 1, (n, 2)).astype(F)
    cosine[:2] = (-1, 1)
    out = ctx.test_medium(sigma, g, lo, hi, o, d, t_hit, h, depth, cosine, u)
    # the clip and medium_u: the host twins bit for bit
    seg, hit = pkg.medium_segment(lo, hi, o, d, t_hit)
    assert out["seg"].tobytes() == seg.tobytes() and (out["hit"] == hit).all() and 0.2 < hit.mean() < 0.8
    assert out["u"].tobytes() == pkg.medium_values(h, depth).tobytes()
    # transmittance and free flight against float64, for sigma_t * len <= 8: the argument's rounding is <= 8 * 2^-23 and
    # expf / log1pf are good to an ulp or two
    length = np.where(hit, seg[:, 1].astype(np.float64) - seg[:, 0].astype(np.float64), 0.0)
    keep = float(F(sigma)) * length <= 8
    tr = np.exp(-float(F(sigma)) * length)
    e_tr = float((np.abs(out["transmittance"] - tr) / tr)[keep].max())
    um = out["u"].astype(np.float64)
    fl = -np.log1p(-um) / float(F(sigma))
    pos = um > 0
    e_fl = float((np.abs(out["flight"] - fl)[pos] / fl[pos]).max())
    assert (out["flight"][~pos] == 0).all()
    ev = MR.hg64(g, cosine)
    e_hg = float((np.abs(out["eval"] - ev) / ev).max())
    print(f"max relative error: transmittance {e_tr:.3e}, free flight {e_fl:.3e}, HG eval {e_hg:.3e}")
    assert keep.mean() > 0.9 and e_tr <= 4e-6 and e_fl <= 4e-6 and e_hg <= 4e-6
    # the samples: unit length, pdf = eval at the sampled cosine, and their mean cosine along the direction of travel is g
    wi = out["wi"].astype(np.float64)
    assert np.abs(np.linalg.norm(wi, axis=1) - 1).max() < 4e-6
    c = (wi * d.astype(np.float64)).sum(1)
    assert abs(float(c.mean()) - g) <= 6 / np.sqrt(n)
    pdf64 = MR.hg64(g, (-c).astype(F))
    assert (np.abs(out["pdf"] - pdf64) / pdf64).max() <= 4e-6 + 8 * 2.0 ** -24 * 3 * g / (1 - g) ** 2


def test_argument_errors(ctx, pkg):
    ok = dict(sigma_t=1.0, albedo=(1, 1, 1), g=0.0, box_min=(0, 0, 0), box_max=(1, 1, 1))
    for bad in (dict(sigma_t=-1.0), dict(sigma_t=float("nan")), dict(sigma_t=float("inf")), dict(albedo=(0.5, 1.5, 0.5)), dict(albedo=(-0.1, 1, 1)),
                dict(g=1.0), dict(g=-1.0), dict(g=float("nan")), dict(box_max=(1, 0, 1)), dict(box_min=(0, -np.inf, 0)), dict(box_max=(1, np.nan, 1))):
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):
            ctx.set_medium(**{**ok, **bad})
    assert not ctx.medium_info()["active"]  # a refused call leaves the medium as it was
    ctx.set_medium(**FOG)
    m = ctx.medium_info()
    assert m["active"] and m["sigma_t"] == F(0.6) and m["g"] == F(0.4) and m["albedo"].tolist() == [F(0.9), F(0.8), F(0.7)]
    assert m["box_min"].tolist() == [-1.5, 0.5, -1.5] and m["box_max"].tolist() == [1.5, 3.5, 1.5]
    ctx.set_medium(**{**FOG, "sigma_t": 0.0})
    assert not ctx.medium_info()["active"] and ctx.medium_info()["g"] == F(0.4)
    ctx.clear_medium()
    assert not ctx.medium_info()["active"] and ctx.medium_info()["g"] == 0
    with pytest.raises(pkg.DmtError, match=r"\(1\)"):
        ctx.test_medium(0.0, 0.0, (0, 0, 0), (1, 1, 1), np.zeros((1, 3), F), np.ones((1, 3), F), [1.0], [0], [0], [0.0], np.zeros((1, 2), F))


# ---- 2. off is off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_films_without_a_medium_are_untouched(ctx, pkg, O, accel):
    sc = O.cornell_box(32, 32)
    with pkg.Renderer(0) as plain:  # never sees a medium call
        plain.upload_scene(sc)
        plain.set_limits(6)
        plain.set_accel(accel)
        ref = _film(plain, 16)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_medium(**{**FOG, "sigma_t": 0.0})
    assert _same(_film(ctx, 16), ref)
    ctx.set_medium(**FOG)
    fog = _film(ctx, 16)
    assert not _same(fog, ref) and np.isfinite(fog[0]).all()
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)  # the medium survives a geometry upload and the camera
    ctx.set_camera(sc.camera)
    assert ctx.medium_info()["active"] and _same(_film(ctx, 16), fog)
    ctx.clear_medium()
    assert _same(_film(ctx, 16), ref)


# ---- 3. one contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True])
def test_bvh_equals_brute_force_under_every_schedule(ctx, O, env):
    sc = O.cornell_box(32, 32)
    if env:
        sc.set_envmap(np.random.default_rng(2).uniform(0.0, 2.0, (8, 16, 3)).astype(F))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    films = {}
    for accel in (0, 1):
        ctx.set_accel(accel)
        for chunk in (1, 16):
            ctx.set_chunk(chunk)
            for tab in (OFF, FORCE):
                ctx.set_sampler_table(tab)
                films[(accel, chunk, tab)] = _film(ctx, 16)
    ref = films[(0, 16, OFF)]
    assert np.isfinite(ref[0]).all() and ref[0][..., :3].max() > 0
    for key, f in films.items():
        assert _same(f, ref), key
    # and the single-sample probe runs the same rows: its samples fold to the film's mean
    px, py, s = MR.pixel_samples(32, 32, 16)
    ctx.set_accel(0)
    L = ctx.test_trace_samples(px, py, s).reshape(32, 32, 16, 3).astype(np.float64)
    assert np.abs(L.mean(2) - ref[0][..., :3]).max() <= 1e-5 * max(1.0, float(L.max()))


# ---- 4. exact attenuation ------------------------------------------------------------------------------------
RES4, SPP4, SIGMA4 = 16, 8, 0.8


def test_exact_attenuation_of_a_delta_light_through_a_slab(ctx, O):
    """Floor, one delta light, bounce cap 1, a fog slab between them that no camera ray enters: every sample is its
    no-medium value times exp(-sigma_t * the slab's length along its shadow ray), and draws what it drew without the fog."""
    sc = MR.floor_scene(O, RES4)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES4, RES4, SPP4)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)  # the plain row
    assert (plain[:, 0] > 0).all()
    for accel in (0, 1):
        ctx.set_accel(accel)
        ctx.set_medium(SIGMA4, (0.8, 0.8, 0.8), 0.3, *MR.SLAB)
        mean = _film(ctx, SPP4)[0][..., :3].astype(np.float64)
        ctx.clear_medium()
        o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
        assert (MR.length64(*MR.SLAB, o, d, np.inf) == 0).all()  # no camera ray enters the slab
        _, P, wl, dist = MR.floor_shadow(o, d)
        length = MR.length64(*MR.SLAB, P, wl, dist)
        assert np.abs(length * np.abs(wl[:, 2]) - 1.0).max() < 1e-12  # the slab is one unit thick
        want = (plain * np.exp(-float(F(SIGMA4)) * length)[:, None]).reshape(RES4, RES4, SPP4, 3).mean(2)
        rel = np.abs(mean - want) / want
        print(f"accel {accel}: max relative deviation {rel.max():.3e}, attenuation {np.exp(-SIGMA4 * length).min():.3f} .. {np.exp(-SIGMA4 * length).max():.3f}")
        assert rel.max() <= 1e-5


# ---- 5. free flight ------------------------------------------------------------------------------------------
RES5, SPP5, SIGMA5 = 8, 4096, 0.35


def test_free_flight_pass_probability(ctx, O):
    """The same floor and light in a black fog (albedo 0) that holds the camera too: a sample survives its camera segment
    with probability exp(-sigma_t t_hit) and then carries its no-medium value times the shadow ray's transmittance."""
    sc = MR.floor_scene(O, RES5)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES5, RES5, SPP5)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)[:, 0]
    ctx.set_medium(SIGMA5, (0.0, 0.0, 0.0), 0.0, *MR.ROOM)
    mean = _film(ctx, SPP5)[0][..., 0].astype(np.float64)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t_hit, P, wl, dist = MR.floor_shadow(o, d)
    sig = float(F(SIGMA5))
    assert np.abs(MR.length64(*MR.ROOM, o, d, t_hit) - t_hit).max() < 1e-12 and np.abs(MR.length64(*MR.ROOM, P, wl, dist) - dist).max() < 1e-12
    p = np.exp(-sig * t_hit)                       # the analytic pass probability
    v = plain * np.exp(-sig * dist)                # what a surviving sample contributes
    want = (v * p).reshape(RES5, RES5, SPP5).mean(2)
    se = np.sqrt((v * v * p * (1 - p)).reshape(RES5, RES5, SPP5).sum(2)) / SPP5  # binomial, from p and not from the film's M2
    z = (mean - want) / se
    print(f"pass probability {p.min():.3f} .. {p.max():.3f}; z scores {z.min():.2f} .. {z.max():.2f}")
    assert (se > 0).all() and (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


# ---- 6. single scattering ------------------------------------------------------------------------------------
RES6, SPP6, SIGMA6, ALBEDO6 = 8, 4096, 0.5, 0.8


def test_single_scattering_against_quadrature(ctx, O):
    """Nothing visible, a delta light inside the fog, isotropic phase function, bounce cap 1: a sample's value is
    a / (4 pi) * I / d^2 * exp(-sigma_t d) at its collision point, if it collides inside the box."""
    sc = MR.void_scene(O, RES6)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    ctx.set_medium(SIGMA6, (ALBEDO6,) * 3, 0.0, *MR.VOID_BOX)
    mean = _film(ctx, SPP6)[0][..., 0].astype(np.float64)
    px, py, s = MR.pixel_samples(RES6, RES6, SPP6)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t0, t1 = MR.clip64(*MR.VOID_BOX, o, d, np.inf)
    assert (t1 - t0 > 2.9).all()
    sig, a, inten = float(F(SIGMA6)), float(F(ALBEDO6)), MR.light_intensity(sc.lights[0])[0]
    # Gauss-Legendre over [t0, t1] of the collision density sigma exp(-sigma (t - t0)) times the value, and times its square
    x, w = np.polynomial.legendre.leggauss(48)
    e1, e2, dmin = np.zeros(o.shape[0]), np.zeros(o.shape[0]), np.inf
    for xk, wk in zip(x, w):
        t = t0 + (t1 - t0) * (xk + 1) / 2
        dist = np.linalg.norm(o + t[:, None] * d - MR.VOID_LIGHT, axis=1)
        dmin = min(dmin, float(dist.min()))
        val = a / (4 * np.pi) * inten / dist ** 2 * np.exp(-sig * dist)
        dens = sig * np.exp(-sig * (t - t0)) * wk * (t1 - t0) / 2
        e1 += dens * val
        e2 += dens * val * val
    assert dmin >= 0.5  # the integrand stays bounded
    want = e1.reshape(RES6, RES6, SPP6).mean(2)
    se = np.sqrt((e2 - e1 * e1).reshape(RES6, RES6, SPP6).sum(2)) / SPP6
    z = (mean - want) / se
    print(f"single scattering: mean radiance {want.min():.4f} .. {want.max():.4f}; z scores {z.min():.2f} .. {z.max():.2f}")
    assert (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


# ---- 7. white furnace ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_white_furnace(ctx, O, accel):
    """White fog (albedo 1) under a constant environment of radiance 1: every path carries beta = 1 to the environment,
    no roulette fires, so every pixel is exactly 1 with no variance."""
    sc = MR.void_scene(O, 16, light=False, env=True)
    ctx.upload_scene(sc)
    ctx.set_limits(64)
    ctx.set_accel(accel)
    ctx.set_medium(1.0, (1.0, 1.0, 1.0), 0.5, *MR.FURNACE_BOX)
    mean, m2 = _film(ctx, 64)
    assert (mean[..., :3] == 1.0).all() and (m2[..., :3] == 0.0).all() and (m2[..., 3] == 64).all()


# ---- 8. lens + medium ----------------------------------------------------------------------------------------
def test_lens_combines_with_the_medium(ctx, O):
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    pinhole = _film(ctx, 16)
    ctx.set_lens(0.1, 2.5)
    for tab in (OFF, FORCE):
        ctx.set_sampler_table(tab)
        lens = _film(ctx, 16)
        assert np.isfinite(lens[0]).all() and (lens[1][..., 3] == 16).all() and not _same(lens, pinhole)
    ctx.set_accel(1)
    assert _same(_film(ctx, 16), lens)


# ---- 9. adaptive rounds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_adaptive_rounds_run_the_medium_rows(ctx, O, accel):
    """dmt_render_adaptive goes through the same launch plan: a pixel that stopped at N samples equals the uniform medium
    film of N samples bit for bit (as test_adaptive_gpu.py pins the other rows)."""
    step, max_spp = 8, 32
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(5)
    ctx.set_accel(accel)
    ctx.set_medium(**FOG)
    ctx.film_clear()
    copies = [(np.zeros((32, 32, 4), F), np.zeros((32, 32, 4), F))]
    for k in range(max_spp // step):
        ctx.render(step, sample_offset=k * step)
        copies.append(ctx.download_film())
    n16 = copies[2][1][..., 3]
    assert (n16 == 16).all()
    m, v = copies[2]
    err = np.sqrt(v[..., :3].astype(np.float64).sum(-1) / (16 * 15)) / np.maximum(m[..., :3].astype(np.float64).sum(-1), 1e-3)
    ctx.film_clear()
    rounds, samples = ctx.render_adaptive(float(np.median(err)), max_spp, step, min_spp=step)
    ctx.sync()
    mean, m2 = ctx.download_film()
    n = m2[..., 3]
    assert rounds == max_spp // step and (np.mod(n, step) == 0).all() and n.min() >= step and n.min() < max_spp and n.max() == max_spp
    assert samples == int(n.sum())
    k = (n / step).astype(np.int64)
    yy, xx = np.mgrid[0:32, 0:32]
    assert np.stack([c[0] for c in copies])[k, yy, xx].tobytes() == mean.tobytes()
    assert np.stack([c[1] for c in copies])[k, yy, xx].tobytes() == m2.tobytes()


# ---- 10. refusals --------------------------------------------------------------------------------------------
def _refused(pkg, call, *words):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_STATE in msg and "medium" in msg and all(w in msg for w in words), msg


def test_refused_combinations(ctx, pkg, O):
    sc = O.cornell_box(32, 32)
    render = lambda: ctx.render(1)
    ctx.upload_scene(sc)
    ctx.set_medium(**FOG)
    render()
    # emissive triangles
    ctx.upload_area_lights([20], [[5, 5, 5]])
    _refused(pkg, render, "emissive")
    ctx.upload_area_lights([], np.zeros((0, 3), F))
    render()
    # motion blur
    ctx.set_motion(sc.xs, sc.ys, sc.zs)
    _refused(pkg, render, "motion")
    ctx.clear_motion()
    render()
    # vertex normals
    ctx.upload_vertex_normals(pkg.smooth_normals(sc.xs, sc.ys, sc.zs))
    _refused(pkg, render, "vertex normals")
    ctx.clear_vertex_normals()
    render()
    # the feature pass and the path log
    _refused(pkg, lambda: ctx.render_aovs(1), "dmt_render_aovs")
    _refused(pkg, lambda: ctx.test_trace_log(3, 3, 0), "dmt_test_trace_log")
    # counting kernels, the wavefront form
    ctx.set_accel(1)
    _refused(pkg, lambda: ctx.render_stats(1), "dmt_render_stats")
    _refused(pkg, lambda: ctx.render_profile(1), "dmt_render_profile")
    ctx.set_bvh_strategy(2)
    _refused(pkg, render, "wavefront")
    ctx.set_bvh_strategy(0)
    render()
    ctx.set_accel(0)
    # light trees
    ctx.upload_scene(_many_lights_cornell(O, pkg, 32))
    for mode in (1, 2):
        ctx.set_light_sampling(mode)
        _refused(pkg, render, "light tree")
    ctx.set_light_sampling(0)
    render()
    # textures, the texture filter and cutouts on top of them
    tex = _textured_cornell(O, pkg, 32)
    ctx.upload_scene(tex)
    _refused(pkg, render, "textures")
    ctx.set_texture_filter(pkg.TEXFILTER_REFERENCE)
    _refused(pkg, render, "texture filter")
    ctx.set_texture_filter(pkg.TEXFILTER_LEVEL0)
    opacity = np.full(tex.bsdfs.shape[0], pkg.OPACITY_NONE, np.uint32)
    opacity[0] = 0
    ctx.upload_opacity(opacity, 0.5)
    _refused(pkg, render, "opacity")
    ctx.clear_opacity()
    _refused(pkg, render, "textures")
    assert ctx.medium_info()["active"]  # refused calls and uploads left the medium alone
    ctx.clear_medium()
    render()
    ctx.sync()
