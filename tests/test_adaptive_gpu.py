"""Adaptive sampling on the GPU (dmt_render_adaptive).  A pixel that stopped at N samples must be bit-identical
to the same pixel of a uniform N-spp film: films fold each pixel's samples in index order whatever the schedule, so every
check here is exact, and the stopping decisions are compared against a numpy restatement of the rule outside a 1e-4
band around the threshold (the device evaluates it with approximate division and square root)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES, DEPTH = 64, 5
STEP, MAX_SPP, MIN_SPP = 8, 64, 8
BAND = 1e-4


def _err(mean, m2):
    """the rule's relative standard error, float64; +inf below two samples"""
    n = m2[..., 3].astype(np.float64)
    s = m2[..., :3].astype(np.float64).sum(-1)
    mu = mean[..., :3].astype(np.float64).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.sqrt(s / (n * (n - 1.0))) / np.maximum(mu, 1e-3)
    return np.where(n < 2, np.inf, e)


def _active(mean, m2, offset, thr, min_spp, max_spp):
    n = m2[..., 3]
    return (n == offset) & (n < max_spp) & ((n < min_spp) | (_err(mean, m2) > thr))


def _near(mean, m2, thr):
    e = _err(mean, m2)
    with np.errstate(invalid="ignore"):
        return np.isfinite(e) & (np.abs(e - thr) < BAND * thr)


def _region_mask(region):
    x0, y0, x1, y1 = region
    m = np.zeros((RES, RES), bool)
    m[y0:y1, x0:x1] = True
    return m


def _uniform(r, steps, region=None):
    """film copies after 0, 1, ..., steps uniform rounds of STEP samples"""
    r.film_clear()
    copies = [(np.zeros((RES, RES, 4), np.float32), np.zeros((RES, RES, 4), np.float32))]
    for k in range(steps):
        r.render(STEP, sample_offset=k * STEP, region=region)
        copies.append(r.download_film())
    return copies


def _adaptive(r, thr, max_spp=MAX_SPP, min_spp=MIN_SPP, region=None):
    r.film_clear()
    rounds, samples = r.render_adaptive(thr, max_spp, STEP, min_spp=min_spp, region=region)
    r.sync()  # raises if a round lost or duplicated a fold
    mean, m2 = r.download_film()
    return mean, m2, rounds, samples


def _assert_identical(mean, m2, copies, region):
    """every pixel of the region equals the uniform copy at its own sample count; every other pixel is untouched"""
    inside = _region_mask(region)
    n = m2[..., 3]
    assert (n[~inside] == 0).all() and (mean[~inside] == 0).all() and (m2[~inside] == 0).all()
    assert (n[inside] > 0).all() and (np.mod(n, STEP) == 0).all()
    k = (n / STEP).astype(np.int64)
    ref_mean = np.stack([c[0] for c in copies])
    ref_m2 = np.stack([c[1] for c in copies])
    yy, xx = np.nonzero(inside)
    got_m, want_m = mean[yy, xx].view(np.uint32), ref_mean[k[yy, xx], yy, xx].view(np.uint32)
    got_v, want_v = m2[yy, xx].view(np.uint32), ref_m2[k[yy, xx], yy, xx].view(np.uint32)
    bad = ~((got_m == want_m).all(-1) & (got_v == want_v).all(-1))
    assert not bad.any(), f"{int(bad.sum())} pixels differ from the uniform film at their N, first at {(yy[bad][0], xx[bad][0])}"


def _assert_decisions(m2, copies, thr, min_spp, max_spp, region):
    """round k traced exactly the pixels the restated rule marks active on uniform copy k"""
    inside = _region_mask(region)
    n = m2[..., 3]
    for k in range(len(copies)):
        offset = k * STEP
        if offset >= max_spp:
            break
        cm, cv = copies[k]
        reached = inside & (n >= offset)
        keep = reached & ~_near(cm, cv, thr)
        predicted = _active(cm, cv, offset, thr, min_spp, max_spp)
        traced = n > offset
        assert (predicted[keep] == traced[keep]).all(), f"round {k}: {int((predicted[keep] != traced[keep]).sum())} decisions differ"


@pytest.fixture(scope="module")
def ctx(O, pkg):
    r = pkg.Renderer(0)
    r.upload_scene(O.cornell_box(RES, RES))
    r.set_limits(DEPTH)
    yield r
    r.close()


def _reset(r):
    r.set_accel(0)
    r.set_bvh_strategy(0)
    r.set_partition(0, 1)
    r.clear_envmap()


@pytest.fixture(scope="module")
def films(ctx, pkg):
    """uniform copies per configuration and the threshold: the median error of the 16-spp brute-force copy, so that
    roughly half the pixels stop early"""
    out = {}
    steps = MAX_SPP // STEP
    try:
        out["bf"] = _uniform(ctx, steps)
        ctx.set_accel(1)
        out["bvh"] = _uniform(ctx, steps)
        ctx.set_accel(0)
        ctx.upload_envmap(pkg.host_scene.synthetic_sky(16))
        out["env"] = _uniform(ctx, steps)
    finally:
        _reset(ctx)
    e = _err(*out["bf"][2])
    out["thr"] = float(np.median(e[np.isfinite(e)]))
    return out


def _setup(r, pkg, config):
    if config == "bvh":
        r.set_accel(1)
    elif config == "env":
        r.upload_envmap(pkg.host_scene.synthetic_sky(16))


@pytest.mark.parametrize("config", ["bf", "bvh", "env"])
def test_adaptive_film_is_bit_identical_to_uniform_films(ctx, pkg, films, config):
    full = (0, 0, RES, RES)
    try:
        _setup(ctx, pkg, config)
        mean, m2, rounds, samples = _adaptive(ctx, films["thr"])
    finally:
        _reset(ctx)
    n = m2[..., 3]
    stopped = n < MAX_SPP
    assert 0.2 < stopped.mean() < 0.9, f"threshold stops {stopped.mean():.2f} of the pixels early"
    assert n.min() >= MIN_SPP
    _assert_identical(mean, m2, films[config], full)
    _assert_decisions(m2, films[config], films["thr"], MIN_SPP, MAX_SPP, full)
    assert 1 <= rounds <= -(-MAX_SPP // STEP)
    assert samples == int(n.sum(dtype=np.float64))


def test_bookkeeping_on_a_region(ctx, films):
    region = (5, 11, 45, 50)  # not tile-aligned
    ctx.kernel_time(reset=True)
    ctx.sched_diag(reset=True)
    mean, m2, rounds, samples = _adaptive(ctx, films["thr"], region=region)
    _, launches = ctx.kernel_time(reset=True)
    d = ctx.sched_diag(reset=True)
    _assert_identical(mean, m2, films["bf"], region)
    _assert_decisions(m2, films["bf"], films["thr"], MIN_SPP, MAX_SPP, region)
    assert 1 <= rounds <= -(-MAX_SPP // STEP)
    assert samples == int(m2[..., 3].sum(dtype=np.float64))
    assert launches == rounds  # every round is one megakernel launch in dmt_kernel_time
    assert d["folds"] == d["launched"]


def test_row_bands_with_empty_bands(ctx, films):
    """a 2x2-tile region is scheduled as row bands (subShift 2).  The threshold is chosen so that, at the 16-spp round, one
    band of a listed tile has no active pixel (a work item with zero units) while another band of that tile has some."""
    region = (24, 24, 40, 40)
    x0, y0, x1, y1 = region
    min_spp, max_spp = 16, 32
    cm, cv = films["bf"][2]
    e = _err(cm, cv)
    best = None
    for ty in range(y0, y1, 8):
        for tx in range(x0, x1, 8):
            band_max = [float(e[ty + 2 * b:ty + 2 * b + 2, tx:tx + 8].max()) for b in range(4)]
            lo, hi = min(band_max), max(band_max)
            if best is None or hi / lo > best[1] / best[0]:
                best = (lo, hi)
    lo, hi = best
    assert hi > lo * 1.01, "no tile with bands of different error"
    thr = 0.5 * (lo + hi)
    mean, m2, rounds, samples = _adaptive(ctx, thr, max_spp=max_spp, min_spp=min_spp, region=region)
    n = m2[..., 3]
    empty_band_in_listed_tile = False
    for ty in range(y0, y1, 8):
        for tx in range(x0, x1, 8):
            tile = n[ty:ty + 8, tx:tx + 8]
            bands = [tile[2 * b:2 * b + 2] for b in range(4)]
            if (tile > min_spp).any() and any((b == min_spp).all() for b in bands):
                empty_band_in_listed_tile = True
    assert empty_band_in_listed_tile
    _assert_identical(mean, m2, films["bf"], region)
    _assert_decisions(m2, films["bf"], thr, min_spp, max_spp, region)
    assert samples == int(n.sum(dtype=np.float64))
    assert rounds <= (max_spp // STEP)


def test_partitions_are_disjoint_and_sum_to_the_whole(ctx, films):
    thr = films["thr"]
    parts = []
    try:
        for rank in (0, 1):
            ctx.set_partition(rank, 2)
            parts.append(_adaptive(ctx, thr))
    finally:
        _reset(ctx)
    whole = _adaptive(ctx, thr)
    n0, n1 = parts[0][1][..., 3], parts[1][1][..., 3]
    assert not ((n0 > 0) & (n1 > 0)).any()
    assert ((n0 > 0) | (n1 > 0)).all()
    for i in (0, 1):
        s = parts[0][i] + parts[1][i]
        assert np.array_equal(s.view(np.uint32), whole[i].view(np.uint32))
    assert parts[0][3] + parts[1][3] == whole[3]


def test_wavefront_strategy_runs_the_megakernel(ctx, films):
    try:
        ctx.set_accel(1)
        mega = _adaptive(ctx, films["thr"])
        ctx.set_bvh_strategy(2)
        wave = _adaptive(ctx, films["thr"])
    finally:
        _reset(ctx)
    for i in (0, 1):
        assert np.array_equal(mega[i].view(np.uint32), wave[i].view(np.uint32))
    assert mega[2:] == wave[2:]
    _assert_identical(wave[0], wave[1], films["bvh"], (0, 0, RES, RES))


def test_film_that_was_not_cleared_is_not_traced_again(ctx, films):
    """N == offset: a second call on the same film traces nothing"""
    mean, m2, _, _ = _adaptive(ctx, films["thr"])
    rounds, samples = ctx.render_adaptive(films["thr"], MAX_SPP, STEP, min_spp=MIN_SPP)
    mean2, m22 = ctx.download_film()
    assert (rounds, samples) == (0, 0)
    assert np.array_equal(mean.view(np.uint32), mean2.view(np.uint32)) and np.array_equal(m2.view(np.uint32), m22.view(np.uint32))


def test_bad_arguments_are_rejected(ctx, pkg):
    lib = pkg.load_library()
    rounds, samples = C.c_uint32(), C.c_uint64()

    def call(min_spp, max_spp, step, thr):
        return lib.dmt_render_adaptive(ctx._ctx, C.c_uint32(min_spp), C.c_uint32(max_spp), C.c_uint32(step), C.c_float(thr),
                                       0, 0, RES, RES, C.byref(rounds), C.byref(samples))
    for args in [(0, 16, 0, 0.1), (0, 0, 4, 0.1), (0, (1 << 24) + 1, 4, 0.1), (0, 16, 4, -1.0), (0, 16, 4, float("nan")),
                 (0, 16, 4, float("inf"))]:
        assert call(*args) == 1, args  # DMT_ERR_INVALID


def test_cli_adaptive_writes_sample_map(tmp_path):
    import subprocess
    from pathlib import Path
    exe = Path(__file__).resolve().parent.parent / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    r = subprocess.run([str(exe), "--width", "64", "--height", "64", "--spp", "32", "--kspp", "8", "--max-depth", "5",
                        "--adaptive", "0.05", "--min-spp", "8", "--time", "-o", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "output-32.png").exists() and (tmp_path / "output-32_sqrt_mse.png").exists()
    assert (tmp_path / "output-32_spp.png").exists()
    line = next(l for l in r.stdout.splitlines() if "adaptive sampling:" in l)
    assert "round(s)" in line and "samples traced" in line
