"""The sampler table (dmt_set_sampler_table): its contents equal the per-sample sampler bit for bit, and a film rendered
through it equals the film rendered without it byte for byte, for every way a call can be cut up."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFF, AUTO, FORCE = 0, 1, 2
W, H, SPP, DEPTH = 264, 136, 40, 8
ENTRY = 40
TILES = ((W + 7) // 8) * ((H + 7) // 8)


# ---- table contents -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(136, 130), (200, 72), (64, 64)])
def test_table_equals_sampler_and_oracle(renderer, O, w, h):
    """Every entry [k][y][x] of the table of samples 1000..1023 holds what the device sampler (dmt_test_sampler) and the
    CPU oracle give for sample 1000 + k of a pixel congruent to (x, y) modulo 128 -- the pixel one period further on
    where the frame has one (136 x 130: 8 and 2 of them; 200 x 72: 72 columns, scale1 = 81; 64 x 64: no wrap)."""
    s0, n = 1000, 24
    pw, ph = min(w, 128), min(h, 128)
    vals, jit = renderer.test_sampler_table(w, h, s0, n)
    assert vals.shape == (n, ph, pw, 8) and jit.shape == (n, ph, pw, 2)
    k, y, x = np.meshgrid(np.arange(n), np.arange(ph), np.arange(pw), indexing="ij")
    px = np.where(x + 128 < w, x + 128, x).ravel().astype(np.int32)
    py = np.where(y + 128 < h, y + 128, y).ravel().astype(np.int32)
    ss = (s0 + k).ravel().astype(np.int32)
    if w > 128:
        assert (px >= 128).any()
    for name, (hi, p2, d) in (("device", renderer.test_sampler(w, h, px, py, ss, 8)), ("oracle", O.sampler_stream(w, h, px, py, ss, 8))):
        assert np.array_equal(vals.reshape(-1, 8).view(np.uint32), d.view(np.uint32)), name
        assert np.array_equal(jit.reshape(-1, 2).view(np.uint32), p2.view(np.uint32)), name
    assert vals.min() >= 0.0 and vals.max() < 1.0 and len(np.unique(vals[..., 0])) > 1000


# ---- films --------------------------------------------------------------------------------------------------------
def _restore(r):
    r.set_sampler_table(AUTO)
    r.set_chunk(0)
    r.set_partition(0, 1)
    r.set_bvh_strategy(0, 1 << 22)
    r.set_accel(0)
    r.clear_envmap()


def _film(r, mode, calls=((0, SPP),), region=None, budget=0, chunk=0, part=(0, 1)):
    r.set_sampler_table(mode, budget)
    r.set_chunk(chunk)
    r.set_partition(*part)
    r.film_clear()
    for s0, n in calls:
        r.render(n, sample_offset=s0, region=region)
    r.sync()
    return r.download_film()


@pytest.fixture(scope="module")
def cornell(renderer, O):
    """Cornell 264 x 136 (2 x 1 periods and an 8-pixel remainder each way) and its 40-spp film without a table."""
    sc = O.cornell_box(W, H)
    renderer.upload_scene(sc)
    renderer.set_limits(DEPTH)
    renderer.set_accel(0)
    try:
        ref = _film(renderer, OFF)
    finally:
        _restore(renderer)
    assert ref[0][..., :3].max() > 0 and np.array_equal(ref[1][..., 3], np.full((H, W), SPP, np.float32))
    return sc, ref


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


CHUNK6_BYTES = 6 * 128 * 128 * ENTRY
CASES = {
    "default_budget": dict(),
    "three_slices_short_last": dict(chunk=6, budget=3 * CHUNK6_BYTES),       # 7 chunks -> slices of 18, 18 and 4 samples
    "chunk_1": dict(chunk=1, budget=16 * 128 * 128 * ENTRY),                 # 40 chunks -> slices of 14, 14, 12
    "chunk_7": dict(chunk=7, budget=2 * 7 * 128 * 128 * ENTRY),              # 6 chunks (the last of 5 samples) -> 3 slices
    "two_calls": dict(calls=((0, 24), (24, 16))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_film_with_table_equals_film_without(renderer, pkg, cornell, case):
    """The film does not depend on the chunk size or on how the samples are split over calls, so one film without a table
    is the reference for every case of the whole frame."""
    sc, ref = cornell
    kw = CASES[case]
    if "chunk" in kw:   # the slicing the case is about
        p = pkg.binding.sampler_table_plan(W, H, TILES * 64, SPP, kw["chunk"], kw["budget"], FORCE)
        assert p["slices"] >= 3 and p["slice_spp"][-1] < p["slice_spp"][0]
    renderer.upload_scene(sc)
    renderer.set_limits(DEPTH)
    try:
        film = _film(renderer, FORCE, **kw)
    finally:
        _restore(renderer)
    assert _same(film, ref)


@pytest.mark.parametrize("case", ["region", "partition"])
def test_film_with_table_region_and_partition(renderer, cornell, case):
    """A region aligned neither to the 8-pixel tiles nor to the period, and rank 1 of a 3-way tile partition."""
    sc, _ = cornell
    kw = dict(region=(5, 3, 261, 133)) if case == "region" else dict(part=(1, 3))
    renderer.upload_scene(sc)
    renderer.set_limits(DEPTH)
    try:
        a = _film(renderer, OFF, **kw)
        b = _film(renderer, FORCE, **kw)
        c = _film(renderer, FORCE, chunk=6, budget=3 * CHUNK6_BYTES, **kw)
    finally:
        _restore(renderer)
    n = a[1][..., 3]
    assert 0 < np.count_nonzero(n) < W * H and set(np.unique(n)) == {0.0, float(SPP)}
    assert _same(a, b) and _same(a, c)


@pytest.mark.parametrize("row", ["bvh", "env"])
def test_film_with_table_other_kernel_rows(renderer, pkg, O, row):
    sc = O.cornell_box(32, 32)
    if row == "env":
        sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    try:
        renderer.set_accel(1 if row == "bvh" else 0)
        a = _film(renderer, OFF, calls=((0, 32),))
        b = _film(renderer, FORCE, calls=((0, 32),))
    finally:
        _restore(renderer)
    assert a[0][..., :3].max() > 0 and a[1][..., 3].min() == 32
    assert _same(a, b)


# ---- bookkeeping --------------------------------------------------------------------------------------------------
def test_one_timed_launch_per_call_and_unsliced_fold_counts(renderer, cornell):
    sc, ref = cornell
    renderer.upload_scene(sc)
    renderer.set_limits(DEPTH)
    out = {}
    try:
        for mode in (OFF, FORCE):
            renderer.sync()
            renderer.kernel_time(reset=True)
            renderer.sched_diag(reset=True)
            film = _film(renderer, mode, calls=((0, 24), (24, 16)), chunk=6, budget=2 * CHUNK6_BYTES)   # 4 and 3 chunks: 2 + 2 slices
            ms, launches = renderer.kernel_time(reset=True)
            out[mode] = (renderer.sched_diag(reset=True), launches, film)
    finally:
        _restore(renderer)
    for mode in (OFF, FORCE):
        diag, launches, film = out[mode]
        assert launches == 2                                       # one per dmt_render call, sliced or not
        assert diag["folds"] == diag["launched"]
        assert diag["folds"] in [TILES * bands * 7 for bands in (1, 2, 4)]   # tiles (or their row bands) x chunks of the unsliced plan
        assert _same(film, ref)
    assert out[OFF][0]["folds"] == out[FORCE][0]["folds"]


# ---- launch kinds that keep the compute path -----------------------------------------------------------------------
def test_adaptive_stats_and_wavefront_ignore_the_table(renderer, cornell):
    sc, _ = cornell
    renderer.upload_scene(sc)
    renderer.set_limits(DEPTH)
    res = {}
    try:
        for mode in (OFF, FORCE):
            renderer.set_sampler_table(mode)
            renderer.set_accel(0)
            renderer.film_clear()
            rounds = renderer.render_adaptive(0.05, 24, 8, min_spp=8)
            adaptive = renderer.download_film()
            renderer.set_accel(1)
            renderer.film_clear()
            stats = renderer.render_stats(8)
            counted = renderer.download_film()
            renderer.set_bvh_strategy(2, 1 << 22)
            renderer.film_clear()
            renderer.render(8)
            renderer.sync()
            wave = renderer.download_film()
            renderer.set_bvh_strategy(0, 1 << 22)
            res[mode] = (rounds, adaptive, stats, counted, wave)
    finally:
        _restore(renderer)
    a, b = res[OFF], res[FORCE]
    assert a[0] == b[0] and a[0][0] >= 2 and _same(a[1], b[1])
    assert a[2] == b[2] and a[2]["samples"] == W * H * 8 and _same(a[3], b[3])
    assert _same(a[4], b[4]) and a[4][1][..., 3].min() == 8
