"""The medium's spectrum on the GPU (dmt_set_medium_spectrum): the device event against the host twin and
float64, films untouched by a grey spectrum, BVH == brute force under every schedule, and the closed forms per channel --
exact attenuation, the pass probability, single scattering and emission against quadrature, the white furnace's conserved
sum -- then degenerate channels, the lens, adaptive rounds, a device-pointer grid and the refused combinations.  Every group
runs on a context of its own; sizes are those of test_medium_gpu.py and test_medium_grid_gpu.py."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import medium_grid_ref as GR
import medium_ref as MR
import medium_spectrum_ref as SR
from test_parity_gpu import _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu

F = np.float32
OFF, FORCE = 0, 2
ERR_STATE = "(3)"
PLUME = np.load(Path(__file__).resolve().parent / "golden" / "medium_grid_plume_8.npy")
# inside the Cornell box (x, z in [-2, 2], y in [0, 4], the camera at the origin looking along +y): rays enter and leave it
FOG = dict(sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))
RGB = dict(extinction=(0.25, 1.0, 2.5), emission=(0.0, 0.0, 0.0))


def channel_k(sigma_t, extinction):
    """k_c = fl32(sigma_t * e_c), as float64"""
    return (F(sigma_t) * np.asarray(extinction, F)).astype(F).astype(np.float64)


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
def test_device_event_equals_the_host_twin(ctx, pkg):
    worst = 0.0
    for i, k in enumerate(SR.K_SETS):
        c = SR.make_cases(np.random.default_rng(100 + i), k, 16384)
        dev, host = ctx.test_medium_spectrum(k, *c), pkg.medium_spectrum_event(k, *c)
        for key in ("channel", "collided", "tau_at"):  # the decisions and the target: bit for bit
            assert dev[key].tobytes() == host[key].tobytes(), (k, key, int((dev[key] != host[key]).sum()))
        same, keep, err, _ = SR.compare(dev, k, *c)
        assert same and keep > 0.9, (k, keep)
        assert np.isfinite(dev["weight"]).all()
        worst = max(worst, err)
    print(f"device event == host twin on 4 x 16384 cases; worst relative weight error against float64 {worst:.3e}")
    assert worst <= 4e-6


def test_argument_errors_and_state(ctx, pkg):
    info = ctx.medium_spectrum_info()
    assert not info["present"] and not info["active"] and info["extinction"].tolist() == [1, 1, 1] and info["emission"].tolist() == [0, 0, 0]
    ctx.set_medium_spectrum((0.25, 1.0, 2.5), (1.0, 2.0, 4.0))  # before the medium
    for bad in (dict(extinction=(-1, 1, 1)), dict(extinction=(0, 0, 0)), dict(extinction=(1, np.nan, 1)), dict(extinction=(1, 1, np.inf)),
                dict(emission=(0, -1, 0)), dict(emission=(np.inf, 0, 0)), dict(emission=(0, 0, np.nan))):
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):
            ctx.set_medium_spectrum(**bad)
    info = ctx.medium_spectrum_info()  # a refused call leaves the state as it was
    assert info["present"] and not info["active"] and info["extinction"].tolist() == [0.25, 1, 2.5] and info["emission"].tolist() == [1, 2, 4]
    assert info["k"].tolist() == [0, 0, 0] and not ctx.medium_info()["active"]
    ctx.set_medium(**FOG)  # the spectrum survives dmt_set_medium
    info = ctx.medium_spectrum_info()
    assert info["present"] and info["active"] and info["ref_channel"] == 2 and ctx.medium_info()["active"]
    assert info["k"].tobytes() == (F(0.6) * np.array([0.25, 1.0, 2.5], F)).astype(F).tobytes()
    assert ctx.medium_info()["sigma_t"] == F(0.6)  # dmt_medium_info keeps its meaning
    ctx.set_medium_spectrum((2, 2, 2), (0, 0, 0))  # three equal k, no emission: the grey rows
    info = ctx.medium_spectrum_info()
    assert info["present"] and not info["active"] and info["ref_channel"] == 0 and info["k"].tolist() == [F(1.2)] * 3
    ctx.set_medium_spectrum((2, 2, 2), (0, 0.5, 0))  # equal k with emission: the spectrum rows
    assert ctx.medium_spectrum_info()["active"]
    ctx.set_medium_spectrum((3, 3, 1))  # a tie: the lowest index
    assert ctx.medium_spectrum_info()["ref_channel"] == 0 and ctx.medium_spectrum_info()["emission"].tolist() == [0, 0, 0]
    ctx.set_medium(**{**FOG, "sigma_t": 0.0})
    assert not ctx.medium_spectrum_info()["active"] and ctx.medium_spectrum_info()["present"]
    ctx.set_medium(**FOG)
    ctx.clear_medium_spectrum()
    assert not ctx.medium_spectrum_info()["present"] and ctx.medium_info()["active"]
    ctx.set_medium_spectrum(**RGB)
    ctx.clear_medium()  # the spectrum goes with its medium
    assert not ctx.medium_spectrum_info()["present"] and not ctx.medium_info()["active"]
    with pytest.raises(pkg.DmtError, match=r"\(1\)"):
        ctx.test_medium_spectrum((0, 0, 0), np.ones((1, 3), F), [1], [0], [1.0])


# ---- 2. off is off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("accel", [0, 1])
def test_a_grey_spectrum_changes_no_film(ctx, pkg, O, accel, grid):
    sc = O.cornell_box(32, 32)
    with pkg.Renderer(0) as other:  # never sees a spectrum call
        other.upload_scene(sc)
        other.set_limits(6)
        other.set_accel(accel)
        other.set_medium(**FOG)
        if grid:
            other.set_medium_grid(PLUME)
        grey1 = _film(other, 16)
        other.set_medium(**{**FOG, "sigma_t": float(F(2) * F(FOG["sigma_t"]))})
        grey2 = _film(other, 16)
    assert not _same(grey1, grey2)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_medium(**FOG)
    if grid:
        ctx.set_medium_grid(PLUME)
    ctx.set_medium_spectrum((1, 1, 1), (0, 0, 0))
    assert not ctx.medium_spectrum_info()["active"] and _same(_film(ctx, 16), grey1)
    ctx.set_medium_spectrum((2, 2, 2), (0, 0, 0))
    assert not ctx.medium_spectrum_info()["active"] and _same(_film(ctx, 16), grey2)
    ctx.set_medium_spectrum(**RGB)
    rgb = _film(ctx, 16)
    assert ctx.medium_spectrum_info()["active"] and np.isfinite(rgb[0]).all() and not _same(rgb, grey1) and not _same(rgb, grey2)
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)  # the spectrum survives a geometry upload and the camera
    ctx.set_camera(sc.camera)
    assert ctx.medium_spectrum_info()["active"] and _same(_film(ctx, 16), rgb)
    ctx.clear_medium_spectrum()  # clearing the spectrum restores the grey film
    assert _same(_film(ctx, 16), grey1)


# ---- 3. one contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("grid", [False, True])
def test_bvh_equals_brute_force_under_every_schedule(ctx, O, grid, env):
    sc = O.cornell_box(32, 32)
    if env:
        sc.set_envmap(np.random.default_rng(2).uniform(0.0, 2.0, (8, 16, 3)).astype(F))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    ctx.set_medium_spectrum((0.25, 1.0, 2.5), (0.0, 0.05, 0.1))
    if grid:
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


# ---- 4. exact attenuation per channel ------------------------------------------------------------------------
RES4, SPP4, SIGMA4, EXT4 = 16, 8, 0.8, (0.25, 1.0, 2.5)
DENS4 = np.where(np.random.default_rng(8).uniform(size=(4, 4, 4)) < 0.5, 0.5, 1.5).astype(F)  # 4 x 4 x 4, two levels


@pytest.mark.parametrize("grid", [False, True])
def test_exact_attenuation_per_channel(ctx, O, grid):
    """Floor, one delta light, bounce cap 1, a fog slab between them that no camera ray enters: every sample is its
    no-medium value times exp(-k_c * the slab's (density-weighted) length along its shadow ray) per channel -- step 5 alone,
    and deterministic."""
    sc = MR.floor_scene(O, RES4)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES4, RES4, SPP4)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)  # the plain row
    assert (plain > 0).all()
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    assert (MR.length64(*MR.SLAB, o, d, np.inf) == 0).all()  # no camera ray enters the slab
    _, P, wl, dist = MR.floor_shadow(o, d)
    if grid:
        assert set(np.unique(DENS4)) == {F(0.5), F(1.5)}
        length = GR.tau64_many(GR.Grid(*MR.SLAB, DENS4), 1.0, P, wl, dist)  # the density-length, by float64 integration
    else:
        length = MR.length64(*MR.SLAB, P, wl, dist)
    k = channel_k(SIGMA4, EXT4)
    want = (plain * np.exp(-k[None, :] * length[:, None])).reshape(RES4, RES4, SPP4, 3).mean(2)
    for accel in (0, 1):
        ctx.set_accel(accel)
        ctx.set_medium(SIGMA4, (0.8, 0.8, 0.8), 0.3, *MR.SLAB)
        ctx.set_medium_spectrum(EXT4)
        if grid:
            ctx.set_medium_grid(DENS4)
        assert ctx.medium_spectrum_info()["active"]
        mean = _film(ctx, SPP4)[0][..., :3].astype(np.float64)
        ctx.clear_medium()
        rel = np.abs(mean - want) / want
        att = np.exp(-k[None, :] * length[:, None])
        print(f"grid {grid}, accel {accel}: max relative deviation per channel {rel.max((0, 1))}, attenuation {att.min(0)} .. {att.max(0)}")
        assert rel.max() <= 1e-5


# ---- 5. pass probability per channel -------------------------------------------------------------------------
RES5, SPP5, SIGMA5, EXT5 = 8, 4096, 0.35, (0.4, 1.0, 2.0)


def test_pass_probability_per_channel(ctx, O):
    """The floor and its light in a black fog (albedo 0) that holds the camera too.  The throughputs are equal on the camera
    segment, so the choice is uniform: a sample passes with probability P = 1/3 sum_j exp(-k_j t) and then carries
    v_c exp(-k_c t) / P, v_c = its no-medium value times the shadow ray's transmittance: mean v_c exp(-k_c t), variance
    v_c^2 exp(-2 k_c t) (1 / P - 1)."""
    sc = MR.floor_scene(O, RES5)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    px, py, s = MR.pixel_samples(RES5, RES5, SPP5)
    plain = ctx.test_trace_samples(px, py, s).astype(np.float64)
    ctx.set_medium(SIGMA5, (0.0, 0.0, 0.0), 0.0, *MR.ROOM)
    ctx.set_medium_spectrum(EXT5)
    mean = _film(ctx, SPP5)[0][..., :3].astype(np.float64)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t_hit, P, wl, dist = MR.floor_shadow(o, d)
    assert np.abs(MR.length64(*MR.ROOM, o, d, t_hit) - t_hit).max() < 1e-12 and np.abs(MR.length64(*MR.ROOM, P, wl, dist) - dist).max() < 1e-12
    k = channel_k(SIGMA5, EXT5)
    tr = np.exp(-k[None, :] * t_hit[:, None])
    pbar = tr.mean(1)
    v = plain * np.exp(-k[None, :] * dist[:, None])
    want = (v * tr).reshape(RES5, RES5, SPP5, 3).mean(2)
    se = np.sqrt((v * v * tr * tr * (1 / pbar - 1)[:, None]).reshape(RES5, RES5, SPP5, 3).sum(2)) / SPP5
    z = (mean - want) / se
    print(f"pass probability {pbar.min():.3f} .. {pbar.max():.3f}; z scores per channel {z.min((0, 1))} .. {z.max((0, 1))}")
    assert (se > 0).all() and (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


# ---- 6. single scattering per channel, 8. emission -----------------------------------------------------------
RES6, SPP6, SIGMA6, EXT6, ALBEDO6 = 8, 4096, 0.5, (0.4, 1.0, 2.0), 0.8


def _void_quadrature(sc, res, spp, k, value):
    """per sample and channel, by 48-point Gauss-Legendre over the camera ray's stretch [t0, t1] inside VOID_BOX: e1 = the
    integral of k_c exp(-k_c s) val_c and e2 = that of (k_c exp(-k_c s) val_c)^2 / pbar(s), pbar = 1/3 sum_j k_j exp(-k_j s)
    the density the collisions are drawn from (equal throughputs: a uniform choice); val = value(points [n, 3]) -> [n, 3]"""
    px, py, s = MR.pixel_samples(res, res, spp)
    o, d, _ = MR.camera_rays64(sc.camera, px, py, s)
    t0, t1 = MR.clip64(*MR.VOID_BOX, o, d, np.inf)
    assert (t1 - t0 > 2.9).all()
    x, w = np.polynomial.legendre.leggauss(48)
    e1, e2 = np.zeros((o.shape[0], 3)), np.zeros((o.shape[0], 3))
    for xk, wk in zip(x, w):
        sdist = (t1 - t0) * (xk + 1) / 2
        f = k[None, :] * np.exp(-k[None, :] * sdist[:, None]) * value(o + (t0 + sdist)[:, None] * d)
        pbar = (k[None, :] * np.exp(-k[None, :] * sdist[:, None])).mean(1)
        e1 += f * (wk * (t1 - t0) / 2)[:, None]
        e2 += f * f / pbar[:, None] * (wk * (t1 - t0) / 2)[:, None]
    want = e1.reshape(res, res, spp, 3).mean(2)
    se = np.sqrt((e2 - e1 * e1).reshape(res, res, spp, 3).sum(2)) / spp
    return want, se, t1 - t0


def test_single_scattering_per_channel_against_quadrature(ctx, O):
    """Nothing visible, a delta light inside the fog, isotropic phase function, bounce cap 1: a sample that collides at s
    carries k_c exp(-k_c s) / pbar(s) * a / (4 pi) * I / d^2 * exp(-k_c d)."""
    sc = MR.void_scene(O, RES6)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    ctx.set_medium(SIGMA6, (ALBEDO6,) * 3, 0.0, *MR.VOID_BOX)
    ctx.set_medium_spectrum(EXT6)
    mean = _film(ctx, SPP6)[0][..., :3].astype(np.float64)
    k, a, inten = channel_k(SIGMA6, EXT6), float(F(ALBEDO6)), MR.light_intensity(sc.lights[0])
    dmin = [np.inf]

    def value(p):
        dist = np.linalg.norm(p - MR.VOID_LIGHT, axis=1)
        dmin[0] = min(dmin[0], float(dist.min()))
        return a / (4 * np.pi) * inten[None, :] / dist[:, None] ** 2 * np.exp(-k[None, :] * dist[:, None])

    want, se, _ = _void_quadrature(sc, RES6, SPP6, k, value)
    assert dmin[0] >= 0.5  # the integrand stays bounded
    z = (mean - want) / se
    print(f"single scattering: mean radiance per channel {want.min((0, 1))} .. {want.max((0, 1))}; z scores {z.min((0, 1))} .. {z.max((0, 1))}")
    assert (np.abs(mean - want) <= 6 * se + 1e-5 * want).all()


RES8, SPP8, LE8 = 8, 1024, (1.0, 2.0, 4.0)


def test_emission_against_its_closed_form(ctx, O):
    """No light, albedo 0, bounce cap 1: a sample that collides at s carries k_c exp(-k_c s) / pbar(s) * Le_c, so the mean is
    Le_c (1 - exp(-k_c len)).  Then albedo 0.5: a vertex at the depth cap still emits."""
    sc = MR.void_scene(O, RES8, light=False)
    ctx.upload_scene(sc)
    ctx.set_limits(1)
    ctx.set_medium(SIGMA6, (0.0, 0.0, 0.0), 0.0, *MR.VOID_BOX)
    ctx.set_medium_spectrum(EXT6, LE8)
    black = _film(ctx, SPP8)
    mean = black[0][..., :3].astype(np.float64)
    assert (black[1][..., 3] == SPP8).all()
    k, le = channel_k(SIGMA6, EXT6), np.asarray(LE8, np.float64)
    want, se, length = _void_quadrature(sc, RES8, SPP8, k, lambda p: np.broadcast_to(le, p.shape))
    closed = (le[None, :] * (1 - np.exp(-k[None, :] * length[:, None]))).reshape(RES8, RES8, SPP8, 3).mean(2)
    assert np.abs(want / closed - 1).max() < 1e-9  # the quadrature's mean is the closed form
    z = (mean - closed) / se
    print(f"emission: mean per channel {closed.min((0, 1))} .. {closed.max((0, 1))}; z scores {z.min((0, 1))} .. {z.max((0, 1))}")
    assert (np.abs(mean - closed) <= 6 * se + 1e-5 * closed).all()
    # albedo 0.5 at cap 1, with and without the emission, the same samples
    ctx.set_medium(SIGMA6, (0.5, 0.5, 0.5), 0.0, *MR.VOID_BOX)
    glow = _film(ctx, SPP8)[0][..., :3]
    ctx.set_medium_spectrum(EXT6)
    dark = _film(ctx, SPP8)[0][..., :3]
    assert np.isfinite(glow).all() and (glow > dark).all()
    # at cap 0 the first vertex sits at the cap: it emits (1 - albedo) Le = half the black fog's sample, exactly, and ends;
    # at cap 1 the second vertex sits there and adds its own
    ctx.set_medium_spectrum(EXT6, LE8)
    ctx.set_limits(0)
    first = _film(ctx, SPP8)[0][..., :3]
    assert first.tobytes() == (F(0.5) * black[0][..., :3]).tobytes() and (glow > first).all()


# ---- 7. white furnace ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_white_furnace_conserves_the_channel_sum(ctx, O, accel):
    """White fog (albedo 1) of k = (0.25, 0.5, 1.0) under a constant environment of radiance 1: with throughput-proportional
    choice every event keeps beta_0 + beta_1 + beta_2 = 3, so max(beta) >= 1 and no roulette fires: every sample's channels
    sum to 3 (ten roundings per vertex, at most 64 vertices), and each channel alone has mean 1 and variance <= 2."""
    spp = 64
    sc = MR.void_scene(O, 16, light=False, env=True)
    ctx.upload_scene(sc)
    ctx.set_limits(64)
    ctx.set_accel(accel)
    ctx.set_medium(1.0, (1.0, 1.0, 1.0), 0.5, *MR.FURNACE_BOX)
    ctx.set_medium_spectrum((0.25, 0.5, 1.0))
    assert ctx.medium_spectrum_info()["active"]
    mean, m2 = _film(ctx, spp)
    total = mean[..., :3].astype(np.float64).sum(-1)
    print(f"accel {accel}: max |sum of the channel means - 3| = {np.abs(total - 3).max():.3e}; channel means {mean[..., :3].min((0, 1))} .. {mean[..., :3].max((0, 1))}")
    assert (m2[..., 3] == spp).all()
    assert np.abs(total - 3).max() <= 3 * 64 * 10 * 2.0 ** -24
    assert np.abs(mean[..., :3].astype(np.float64) - 1).max() <= 6 * np.sqrt(2 / spp)
    assert mean[..., :3].std() > 0  # (the spectrum rows ran: the grey furnace is exactly 1)


# ---- 9. degenerate channels ----------------------------------------------------------------------------------
def test_degenerate_channels(ctx, O):
    """a channel without extinction and without albedo: it never collides by its own choice and never divides by zero"""
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(8)
    ctx.set_medium(**{**FOG, "albedo": (0.9, 0.0, 0.5)})
    ctx.set_medium_spectrum((1.0, 0.0, 2.0))
    info = ctx.medium_spectrum_info()
    assert info["active"] and info["k"][1] == 0 and info["ref_channel"] == 2
    brute = _film(ctx, 16)
    assert np.isfinite(brute[0]).all() and np.isfinite(brute[1]).all() and (brute[1][..., 3] == 16).all() and brute[0][..., :3].max() > 0
    ctx.set_accel(1)
    assert _same(_film(ctx, 16), brute)


# ---- 10. combinations ----------------------------------------------------------------------------------------
def test_lens_combines_with_the_spectrum(ctx, O):
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(6)
    ctx.set_medium(**FOG)
    ctx.set_medium_spectrum(**RGB)
    pinhole = _film(ctx, 16)
    ctx.set_lens(0.1, 2.5)
    for tab in (OFF, FORCE):
        ctx.set_sampler_table(tab)
        lens = _film(ctx, 16)
        assert np.isfinite(lens[0]).all() and (lens[1][..., 3] == 16).all() and not _same(lens, pinhole)
    ctx.set_accel(1)
    assert _same(_film(ctx, 16), lens)


@pytest.mark.parametrize("accel", [0, 1])
def test_adaptive_rounds_run_the_spectrum_rows(ctx, O, accel):
    """dmt_render_adaptive goes through the same launch plan: a pixel that stopped at N samples equals the uniform spectrum
    film of N samples bit for bit (as test_adaptive_rounds_run_the_medium_rows)"""
    step, max_spp = 8, 32
    ctx.upload_scene(O.cornell_box(32, 32))
    ctx.set_limits(5)
    ctx.set_accel(accel)
    ctx.set_medium(**FOG)
    ctx.set_medium_spectrum(**RGB)
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


def test_device_pointer_grid_combines_with_the_spectrum(tmp_path):
    """Run in a child process (tests/_medium_spectrum_device_worker.py): torch must open the GPU before the HIP library
    does, which this session's renderer has long done."""
    out = tmp_path / "out.npz"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve().parent / "_medium_spectrum_device_worker.py"), str(out)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = dict(np.load(out))
    info = json.loads(str(r["host_info"]))
    assert info["present"] and info["active"] and info["ref_channel"] == 2 and info["extinction"] == [0.25, 1.0, 2.5]
    assert json.loads(str(r["device_info"])) == info and bool(r["device_grid_active"])
    assert r["device_mean"].tobytes() == r["host_mean"].tobytes() and r["device_m2"].tobytes() == r["host_m2"].tobytes()
    assert np.isfinite(r["host_mean"]).all() and r["host_mean"][..., :3].max() > 0 and r["host_mean"].tobytes() != r["grey_mean"].tobytes()


# ---- 11. refusals --------------------------------------------------------------------------------------------
def _refused(pkg, call, *words):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_STATE in msg and "medium" in msg and all(w in msg for w in words), msg


def test_refused_combinations(ctx, pkg, O):
    """everything the medium refuses is refused for the spectrum rows, with the medium's messages"""
    sc = O.cornell_box(32, 32)
    render = lambda: ctx.render(1)
    ctx.upload_scene(sc)
    ctx.set_medium(**FOG)
    ctx.set_medium_spectrum((0.25, 1.0, 2.5), (0.0, 0.1, 0.0))
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
    info = ctx.medium_spectrum_info()  # refused calls and uploads left the spectrum alone
    assert info["active"] and info["extinction"].tolist() == [0.25, 1, 2.5] and info["emission"].tolist() == [0, F(0.1), 0] and ctx.medium_info()["active"]
    ctx.clear_medium()
    render()
    ctx.sync()
