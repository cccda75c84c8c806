"""The heterogeneous medium on the GPU (dmt_set_medium_grid): the device march against the host twin bit for
bit, films untouched without a grid, BVH == brute force under every schedule, host upload == device-pointer upload, and the
closed forms of the homogeneous medium restated for a grid -- exact attenuation through a slab of random densities, the
free-flight pass probability through the plume, single scattering in a two-density grid against quadrature, the white
furnace -- then the lens, adaptive rounds and the refused combinations.  Every group runs on a context of its own."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import medium_grid_ref as GR
import medium_ref as MR
from test_parity_gpu import _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu

F = np.float32
OFF, FORCE = 0, 2
ERR_STATE = "(3)"
PLUME = np.load(Path(__file__).resolve().parent / "golden" / "medium_grid_plume_8.npy")
# inside the Cornell box (x, z in [-2, 2], y in [0, 4], the camera at the origin looking along +y): rays enter and leave it
FOG = dict(sigma_t=1.2, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))


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
def test_device_march_equals_the_host_twin(ctx, pkg):
    most = 0
    for k, (name, dens) in enumerate(GR.make_grids(np.random.default_rng(41))):
        o, d, t_end, target = GR.make_rays(np.random.default_rng(300 + k), 65536)
        dev = ctx.test_medium_grid(*GR.BOX, 1.5, dens, o, d, t_end, target)
        host = pkg.medium_grid_march(*GR.BOX, 1.5, dens, o, d, t_end, target)
        for key in ("tau", "ts", "collided", "steps"):
            assert dev[key].tobytes() == host[key].tobytes(), (name, key, int((dev[key] != host[key]).sum()))
        nz, ny, nx = dens.shape
        assert dev["steps"].max() <= nx + ny + nz and 0.2 < (dev["steps"] > 0).mean() < 0.8 and dev["collided"].any()
        most = max(most, int(dev["steps"].max()))
    print(f"device march == host twin on 3 x 65536 rays; the longest walk took {most} steps")


def test_argument_errors(ctx, pkg):
    assert ctx.medium_grid_info() == dict(present=False, dims=(0, 0, 0), support_min=(0, 0, 0), support_max=(0, 0, 0), positive=0, max_density=0.0,
                                          active=False)
    bad = np.ones((2, 3, 4), F)
    bad[1, 2, 3] = np.nan
    with pytest.raises(pkg.DmtError, match=r"\(1\).*voxel \(3, 2, 1\)"):
        ctx.set_medium_grid(bad)
    bad[1, 2, 3], bad[0, 1, 2] = 1, -0.5
    with pytest.raises(pkg.DmtError, match=r"\(1\).*voxel \(2, 1, 0\)"):
        ctx.set_medium_grid(bad)
    bad[0, 1, 2] = np.inf
    with pytest.raises(pkg.DmtError, match=r"\(1\).*voxel \(2, 1, 0\)"):
        ctx.set_medium_grid(bad)
    for shape in ((1, 1, 513), (513, 1, 1), (1, 513, 1)):
        with pytest.raises(pkg.DmtError, match=r"\(1\).*1 \.\. 512"):
            ctx.set_medium_grid(np.ones(shape, F))
    with pytest.raises(pkg.DmtError):
        ctx.set_medium_grid(np.ones((2, 2), F))
    assert not ctx.medium_grid_info()["present"]  # a refused call leaves the context as it was
    # the grid may come before the medium; the fixture's support
    ctx.set_medium_grid(PLUME)
    info = ctx.medium_grid_info()
    assert info == dict(present=True, dims=(8, 8, 8), support_min=(1, 1, 1), support_max=(6, 6, 7), positive=168, max_density=float(PLUME.max()),
                        active=False)
    with pytest.raises(pkg.DmtError, match=r"\(1\)"):
        ctx.set_medium_grid(bad)
    assert ctx.medium_grid_info() == info
    ctx.set_medium(**FOG)
    assert ctx.medium_grid_info()["active"] and ctx.medium_info()["active"]
    ctx.set_medium(**{**FOG, "sigma_t": 0.0})
    assert not ctx.medium_grid_info()["active"] and ctx.medium_grid_info()["present"]
    ctx.set_medium(**FOG)
    ctx.set_medium_grid(np.zeros((2, 2, 2), F))  # an empty medium
    info = ctx.medium_grid_info()
    assert info["present"] and not info["active"] and info["positive"] == 0 and info["support_min"] > info["support_max"]
    assert not ctx.medium_info()["active"]
    ctx.clear_medium_grid()
    assert not ctx.medium_grid_info()["present"] and ctx.medium_info()["active"]
    ctx.set_medium_grid(PLUME)
    ctx.clear_medium()  # drops the grid with the medium
    assert not ctx.medium_grid_info()["present"]
    with pytest.raises(pkg.DmtError, match=r"\(1\).*voxel \(0, 0, 0\)"):
        ctx.test_medium_grid(*GR.BOX, 1.0, np.full((1, 1, 1), -1, F), np.zeros((1, 3), F), np.ones((1, 3), F), [1.0], [1.0])


# ---- 2. off is off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_films_without_a_grid_are_untouched(ctx, pkg, O, accel):
    sc = O.cornell_box(32, 32)
    with pkg.Renderer(0) as other:  # never sees a grid call
        other.upload_scene(sc)
        other.set_limits(6)
        other.set_accel(accel)
        plain = _film(other, 16)
        other.set_medium(**FOG)
        homogeneous = _film(other, 16)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_medium_grid(PLUME)  # a grid without a medium
    assert _same(_film(ctx, 16), plain)
    ctx.set_medium(**FOG)
    grid = _film(ctx, 16)
    assert not _same(grid, plain) and not _same(grid, homogeneous) and np.isfinite(grid[0]).all()
    # the grid survives a geometry upload, the camera and set_medium
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
    ctx.set_camera(sc.camera)
    ctx.set_medium(**{**FOG, "sigma_t": 0.3})
    assert ctx.medium_grid_info()["active"] and not _same(_film(ctx, 16), grid)
    ctx.set_medium(**FOG)
    assert _same(_film(ctx, 16), grid)
    ctx.set_medium_grid(np.zeros((3, 2, 1), F))  # an all-zero grid: the plain rows
    assert _same(_film(ctx, 16), plain)
    ctx.set_medium_grid(PLUME)
    assert _same(_film(ctx, 16), grid)
    ctx.clear_medium_grid()  # set, then cleared: the homogeneous rows
    assert _same(_film(ctx, 16), homogeneous)
    ctx.clear_medium()
    assert _same(_film(ctx, 16), plain)


# ---- 3. one contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True])
def test_bvh_equals_brute_force_under_every_schedule(ctx, O, env):
    sc = O.cornell_box(32, 32)
    if env:
        sc.set_envmap(np.random.default_rng(2).uniform(0.0, 2.0, (8, 16, 3)).astype(F))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    ctx.set_medium_grid(PLUME)
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


def test_host_upload_equals_device_pointer_upload(tmp_path):
    """Run in a child process (tests/_medium_grid_device_worker.py): torch must open the GPU before the HIP library does,
    which this session's renderer has long done."""
    out = tmp_path / "out.npz"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve().parent / "_medium_grid_device_worker.py"), str(out)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = dict(np.load(out))
    info = json.loads(str(r["host_info"]))
    assert info["active"] and info["dims"] == [8, 8, 8] and info["support_min"] == [1, 1, 1] and info["support_max"] == [6, 6, 7] and info["positive"] == 168
    assert json.loads(str(r["device_info"])) == info and json.loads(str(r["after_info"])) == info
    for tag in ("device", "after"):  # byte-identical films, also after the refused calls
        assert r[tag + "_mean"].tobytes() == r["host_mean"].tobytes() and r[tag + "_m2"].tobytes() == r["host_m2"].tobytes(), tag
    assert np.isfinite(r["host_mean"]).all() and r["host_mean"][..., :3].max() > 0
    # the same errors, from the device's own scan: the first offending voxel
    assert "(1)" in str(r["refused_values"]) and "voxel (0, 0, 1)" in str(r["refused_values"])
    assert "1 .. 512" in str(r["refused_size"]) and str(r["refused_dtype"]) and str(r["refused_strides"])
    zeros = json.loads(str(r["zeros_info"]))
    assert zeros["present"] and not zeros["active"] and zeros["positive"] == 0 and zeros["support_min"] > zeros["support_max"]


# ---- 4. exact attenuation ------------------------------------------------------------------------------------
RES4, SPP4, SIGMA4 = 16, 8, 0.8


def test_exact_attenuation_of_a_delta_light_through_a_grid_slab(ctx, pkg, O):
    """Floor, one delta light, bounce cap 1, a 4 x 4 x 2 grid of random densities with zeros in the slab between them, which
    no camera ray enters: every sample is its no-medium value times exp(-tau) of its shadow ray, and draws what it drew
    without the fog.

    Per sample the relative tolerance is the march's bound for its shadow ray,
    sigma_t * max_density * (steps + 2) * 2^-22 * max(|t0|, |t1|, 1), plus 4e-6 for expf."""
    sc = MR.floor_scene(O, RES4)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES4, RES4, SPP4)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)  # the plain row
    assert (plain[:, 0] > 0).all()
    dens = np.random.default_rng(8).uniform(0.2, 2.0, (2, 4, 4)).astype(F)
    dens[np.random.default_rng(9).uniform(size=dens.shape) < 0.3] = 0
    dens[1, 2, 1], dens[0, 2, 1], dens[1, 2, 2] = 0, 1.7, 0.9  # under the light: an empty voxel beside and above dense ones
    assert (dens == 0).any() and (dens > 0).sum() > 16
    G = GR.Grid(*MR.SLAB, dens)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    assert (MR.length64(*MR.SLAB, o, d, np.inf) == 0).all()  # no camera ray enters the slab
    _, P, wl, dist = MR.floor_shadow(o, d)
    tau = GR.tau64_many(G, SIGMA4, P, wl, dist)
    assert tau.min() >= 0 and tau.max() > 0.5 and np.unique(np.round(tau, 6)).size > 100
    twin = pkg.medium_grid_march(*MR.SLAB, SIGMA4, dens, P, wl, dist, np.full(dist.shape, np.inf))
    t = GR.pieces64_many(G, SIGMA4, P, wl, dist)[0]
    tol = float(F(SIGMA4)) * float(dens.max()) * (twin["steps"] + 2) * 2.0 ** -22 * np.maximum(np.abs(t).max(1), 1.0) + 4e-6
    sample = plain * np.exp(-tau)[:, None]
    want = sample.reshape(RES4, RES4, SPP4, 3).mean(2)
    allowed = (sample * tol[:, None]).reshape(RES4, RES4, SPP4, 3).mean(2)
    for accel in (0, 1):
        ctx.set_accel(accel)
        ctx.set_medium(SIGMA4, (0.8, 0.8, 0.8), 0.3, *MR.SLAB)
        ctx.set_medium_grid(dens)
        mean = _film(ctx, SPP4)[0][..., :3].astype(np.float64)
        ctx.clear_medium()
        dev = np.abs(mean - want)
        print(f"accel {accel}: max relative deviation {(dev / want).max():.3e} ({(dev / allowed).max():.3f} of the tolerance), "
              f"attenuation {np.exp(-tau).min():.3f} .. {np.exp(-tau).max():.3f}")
        assert (dev <= allowed).all()


# ---- 5. free flight ------------------------------------------------------------------------------------------
RES5, SPP5, SIGMA5 = 8, 4096, 0.35
ROOM5 = ((-6.0, -2.0, -1.0), (6.0, 12.0, 6.0))  # holds the camera, the floor's visible part and the light; the plume's voxels are 1.5 x 1.75 x 0.875


def test_free_flight_pass_probability(ctx, O):
    """The same floor and light in a black fog (albedo 0) on the plume fixture, around camera, floor and light: a sample
    survives its camera segment with probability exp(-tau) and then carries its no-medium value times the shadow ray's
    transmittance."""
    sc = MR.floor_scene(O, RES5)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES5, RES5, SPP5)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)[:, 0]
    ctx.set_medium(SIGMA5, (0.0, 0.0, 0.0), 0.0, *ROOM5)
    ctx.set_medium_grid(PLUME)
    mean = _film(ctx, SPP5)[0][..., 0].astype(np.float64)
    G = GR.Grid(*ROOM5, PLUME)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t_hit, P, wl, dist = MR.floor_shadow(o, d)
    p = np.exp(-GR.tau64_many(G, SIGMA5, o, d, t_hit))    # the pass probability of the camera segment
    v = plain * np.exp(-GR.tau64_many(G, SIGMA5, P, wl, dist))  # what a surviving sample contributes
    want = (v * p).reshape(RES5, RES5, SPP5).mean(2)
    se = np.sqrt((v * v * p * (1 - p)).reshape(RES5, RES5, SPP5).sum(2)) / SPP5  # binomial, from p and not from the film's M2
    z = (mean - want) / se
    print(f"pass probability {p.min():.3f} .. {p.max():.3f}; z scores {z.min():.2f} .. {z.max():.2f}")
    assert p.max() - p.min() > 0.2  # the plume is seen: the probability varies over the film
    assert (se > 0).all() and (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


# ---- 6. single scattering ------------------------------------------------------------------------------------
RES6, SPP6, SIGMA6, ALBEDO6 = 8, 1024, 0.5, 0.8
DENS6 = np.array([[[0.5, 2.0]]], F)  # 2 x 1 x 1: x < 0 and x > 0 of VOID_BOX


def test_single_scattering_against_quadrature(ctx, O):
    """Nothing visible, a delta light inside a two-density grid, isotropic phase function, bounce cap 1: a sample's value
    is a / (4 pi) * I / d^2 * exp(-tau(point, light)) at its collision point, if it collides inside the box.  Expectation and
    variance by Gauss-Legendre quadrature per voxel piece of each camera ray."""
    sc = MR.void_scene(O, RES6)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    ctx.set_medium(SIGMA6, (ALBEDO6,) * 3, 0.0, *MR.VOID_BOX)
    ctx.set_medium_grid(DENS6)
    mean = _film(ctx, SPP6)[0][..., 0].astype(np.float64)
    G = GR.Grid(*MR.VOID_BOX, DENS6)
    px, py, s = MR.pixel_samples(RES6, RES6, SPP6)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t, sig = GR.pieces64_many(G, SIGMA6, o, d, np.inf)  # break points [n, K + 1], extinction per piece [n, K]
    assert (t[:, -1] - t[:, 0] > 2.9).all() and sig.min() > 0 and np.unique(sig).size == 2  # (camera rays stay on their side of x = 0; shadow rays cross it)
    a, inten = float(F(ALBEDO6)), MR.light_intensity(sc.lights[0])[0]
    x, w = np.polynomial.legendre.leggauss(24)
    e1, e2, dmin = np.zeros(o.shape[0]), np.zeros(o.shape[0]), np.inf
    before = np.zeros(o.shape[0])  # the optical depth of the pieces already passed
    for k in range(sig.shape[1]):
        ta, tb = t[:, k], t[:, k + 1]
        for xk, wk in zip(x, w):
            tt = ta + (tb - ta) * (xk + 1) / 2
            p = o + tt[:, None] * d
            v = MR.VOID_LIGHT - p
            dist = np.linalg.norm(v, axis=1)
            dmin = min(dmin, float(dist.min()))
            val = a / (4 * np.pi) * inten / dist ** 2 * np.exp(-GR.tau64_many(G, SIGMA6, p, v / dist[:, None], dist))
            dens = sig[:, k] * np.exp(-(before + sig[:, k] * (tt - ta))) * wk * (tb - ta) / 2
            e1 += dens * val
            e2 += dens * val * val
        before += sig[:, k] * (tb - ta)
    assert dmin >= 0.5  # the integrand stays bounded
    want = e1.reshape(RES6, RES6, SPP6).mean(2)
    se = np.sqrt((e2 - e1 * e1).reshape(RES6, RES6, SPP6).sum(2)) / SPP6
    z = (mean - want) / se
    print(f"single scattering: mean radiance {want.min():.4f} .. {want.max():.4f}; z scores {z.min():.2f} .. {z.max():.2f}")
    assert (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


# ---- 7. white furnace ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_white_furnace(ctx, O, accel):
    """White fog (albedo 1) on the plume under a constant environment of radiance 1: every path carries beta = 1 to the
    environment, no roulette fires, so every pixel is exactly 1 with no variance."""
    sc = MR.void_scene(O, 16, light=False, env=True)
    ctx.upload_scene(sc)
    ctx.set_limits(64)
    ctx.set_accel(accel)
    ctx.set_medium(1.0, (1.0, 1.0, 1.0), 0.5, *MR.FURNACE_BOX)
    ctx.set_medium_grid(PLUME)
    assert ctx.medium_grid_info()["active"]
    mean, m2 = _film(ctx, 64)
    assert (mean[..., :3] == 1.0).all() and (m2[..., :3] == 0.0).all() and (m2[..., 3] == 64).all()


# ---- 8. lens + grid, adaptive rounds -------------------------------------------------------------------------
def test_lens_combines_with_the_grid(ctx, O):
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    ctx.set_medium_grid(PLUME)
    pinhole = _film(ctx, 16)
    ctx.set_lens(0.1, 2.5)
    for tab in (OFF, FORCE):
        ctx.set_sampler_table(tab)
        lens = _film(ctx, 16)
        assert np.isfinite(lens[0]).all() and (lens[1][..., 3] == 16).all() and not _same(lens, pinhole)
    ctx.set_accel(1)
    assert _same(_film(ctx, 16), lens)


@pytest.mark.parametrize("accel", [0, 1])
def test_adaptive_rounds_run_the_grid_rows(ctx, O, accel):
    """dmt_render_adaptive goes through the same launch plan: a pixel that stopped at N samples equals the uniform grid
    film of N samples bit for bit"""
    step, max_spp = 8, 32
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(5)
    ctx.set_accel(accel)
    ctx.set_medium(**FOG)
    ctx.set_medium_grid(PLUME)
    ctx.film_clear()
    copies = [(np.zeros((32, 32, 4), F), np.zeros((32, 32, 4), F))]
    for k in range(max_spp // step):
        ctx.render(step, sample_offset=k * step)
        copies.append(ctx.download_film())
    assert (copies[2][1][..., 3] == 16).all()
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


# ---- 9. refusals ---------------------------------------------------------------------------------------------
def _refused(pkg, call, *words):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_STATE in msg and "medium" in msg and all(w in msg for w in words), msg


def test_refused_combinations(ctx, pkg, O):
    """everything the medium refuses is refused for the grid rows, with the medium's messages"""
    sc = O.cornell_box(32, 32)
    render = lambda: ctx.render(1)
    ctx.upload_scene(sc)
    ctx.set_medium(**FOG)
    ctx.set_medium_grid(PLUME)
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
    assert ctx.medium_grid_info()["active"]  # refused calls and uploads left the grid alone
    # with an all-zero grid the medium is empty, and nothing is refused
    ctx.set_medium_grid(np.zeros((1, 1, 1), F))
    render()
    ctx.set_medium_grid(PLUME)
    _refused(pkg, render, "textures")
    ctx.clear_medium()
    render()
    ctx.sync()
