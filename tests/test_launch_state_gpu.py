"""The launch layer's state (csrc/launch_state.hpp): a long-lived context that reached a launch configuration by a route --
through other launch kinds, other settings and larger launches -- renders the same film, byte for byte, as a fresh context
that was given that configuration directly.  This guards the buffers that are grown once and reused, the words that are
zeroed per launch or per table slice, and the settings that must stay as they were set.  After every comparison dmt_sync
passes and the scheduler's counters show every launched work item folded exactly once, no wave leaving early, and every
parked GGX hit taken back.  Every comparison is of bytes or integers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = "(1)", "(3)"
DEPTH, SPP = 4, 8
OFF, AUTO, FORCE = 0, 1, 2
WF_PATHS = 1 << 22          # the wavefront form's path slots per pass of a fresh context
LENS = (0.05, 4.0)
BS_GGX_DIEL, BS_GGX_COND = 1, 2
WHOLE = None                # region: the whole film


def _cfg(**kw):
    """A launch configuration: every setting of the layer, and the lens, which decides the sampler table's planes."""
    c = dict(size=64, accel=0, chunk=0, table=(AUTO, 0), lens=0.0, ggx=None, strategy=1, paths=WF_PATHS, part=(0, 1))
    c.update(kw)
    return c


class _Scenes:
    def __init__(self, pkg):
        self.of = {n: pkg.host_scene.cornell_box(n, n) for n in (32, 64)}
        t = np.ascontiguousarray(self.of[64].bsdfs, np.uint8).reshape(-1, 32)[:, 4:8].copy().view(np.uint32)[:, 0] >> 16
        assert (t == BS_GGX_DIEL).any() or (t == BS_GGX_COND).any()   # GGX hits: the queues of parked hits are in use
        r = pkg.Renderer(0)
        try:
            self.ggx_default = r.ggx_batch()
        finally:
            r.close()


@pytest.fixture(scope="module")
def S(pkg):
    return _Scenes(pkg)


def _apply(r, S, c):
    """Every setting of `c`, given directly."""
    if r.width != c["size"]:
        if r.width == 0:
            r.upload_scene(S.of[c["size"]])
        else:
            r.set_camera(S.of[c["size"]].camera)   # the same box at another resolution: a new film
    r.set_limits(DEPTH)
    r.set_accel(c["accel"])
    r.set_chunk(c["chunk"])
    r.set_sampler_table(*c["table"])
    r.set_lens(c["lens"], LENS[1])
    r.set_ggx_batch(S.ggx_default if c["ggx"] is None else c["ggx"])
    r.set_bvh_strategy(c["strategy"], c["paths"])
    r.set_partition(*c["part"])


def _run(r, call):
    kind, a = call[0], call[1:]
    if kind == "render":
        return r.render(a[0], sample_offset=a[1], region=a[2])
    if kind == "adaptive":
        return r.render_adaptive(0.0, a[0], a[1])
    return {"stats": r.render_stats, "profile": r.render_profile}[kind](a[0])


def _snap(r, calls, items=True):
    """The film the calls leave on a cleared film, what they returned and how many work items they launched."""
    r.film_clear()
    r.sched_diag(reset=True)
    out = [_run(r, c) for c in calls]
    r.sync()
    mean, m2 = r.download_film()
    d = r.sched_diag()
    assert d["folds"] == d["launched"] and d["early_exits"] == 0 and d["ggx_parked"] == d["ggx_resumed"], d
    assert (d["launched"] > 0) == items, d   # (the wavefront form has no work items)
    return mean.tobytes(), m2.tobytes(), out, d["launched"]


PLAIN = (("render", SPP, 0, WHOLE),)


@pytest.fixture(scope="module")
def fresh(pkg, S):
    """_snap of a fresh context that was given a configuration directly; each (configuration, calls) is rendered once"""
    memo = {}

    def get(c, calls=PLAIN, items=True):
        key = (tuple(sorted(c.items())), calls)
        if key not in memo:
            r = pkg.Renderer(0)
            try:
                _apply(r, S, c)
                memo[key] = _snap(r, calls, items)
            finally:
                r.close()
        return memo[key]
    return get


@pytest.fixture(scope="module")
def old(pkg):
    """the long-lived context: every test below goes on from where the one before left it"""
    r = pkg.Renderer(0)
    yield r
    r.close()


def _refused(pkg, call, code, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert code in msg and all(n in msg for n in needles), msg


ACCELS = pytest.mark.parametrize("accel", [0, 1])


# ---- (a) the most hand-over words, then row bands -------------------------------------------------------------------
@ACCELS
def test_one_sample_chunks_then_a_region_off_the_tile_grid(old, S, fresh, accel):
    c = _cfg(accel=accel, chunk=1)
    _apply(old, S, c)
    assert _snap(old, PLAIN) == fresh(c)
    old.set_chunk(0)
    region = (("render", SPP, 0, (3, 5, 12, 14)),)   # 9 x 9 pixels over 2 x 2 tiles
    assert _snap(old, region) == fresh(_cfg(accel=accel), region)
    assert _snap(old, PLAIN) == fresh(_cfg(accel=accel))


# ---- (b), (c) the sampler table in slices, without and with the lens plane -------------------------------------------
def _slice_budget(pkg, chunk):
    """a budget of one chunk's table: 8 spp in chunks of 2 are then 4 slices"""
    plan = pkg.binding.sampler_table_plan(64, 64, 64 * 64, SPP, chunk, mode=FORCE)
    assert plan["use"] and plan["slices"] == 1
    budget = plan["entry_bytes"] * plan["period_width"] * plan["period_height"] * chunk
    plan = pkg.binding.sampler_table_plan(64, 64, 64 * 64, SPP, chunk, budget_bytes=budget, mode=FORCE)
    assert plan["use"] and plan["slices"] >= 3 and sum(plan["slice_spp"]) == SPP, plan
    return budget, plan["entry_bytes"]


@ACCELS
@pytest.mark.parametrize("lens", [0.0, LENS[0]])
def test_sampler_table_slices_then_off_then_automatic(old, pkg, S, fresh, accel, lens):
    budget, entry = _slice_budget(pkg, 2)
    if lens > 0.0:
        budget = budget * (entry + 8) // entry   # an entry of a launch with a lens has one float2 more
    for table in ((FORCE, budget), (OFF, 0), (AUTO, 0)):
        c = _cfg(accel=accel, chunk=2, table=table, lens=lens)
        _apply(old, S, c)
        assert _snap(old, PLAIN) == fresh(c)
    old.set_lens(0.0)
    old.set_chunk(0)
    assert _snap(old, PLAIN) == fresh(_cfg(accel=accel))


# ---- (d) GGX batching ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [64, 32])
def test_ggx_batch_sizes(old, S, fresh, size):
    for batch in (8, 0, None):
        c = _cfg(size=size, ggx=batch)
        _apply(old, S, c)
        assert _snap(old, PLAIN) == fresh(c)
        assert old.ggx_batch() == (S.ggx_default if batch is None else batch)
        parked = old.sched_diag()["ggx_parked"]
        assert (parked > 0) == (old.ggx_batch() > 0), parked


# ---- (e) adaptive rounds, then a plain launch that goes on from them -------------------------------------------------
@ACCELS
def test_adaptive_rounds_then_a_plain_launch(old, S, fresh, accel):
    c = _cfg(accel=accel)
    _apply(old, S, c)
    calls = (("adaptive", SPP, 4), ("render", 4, SPP, WHOLE))
    snap = _snap(old, calls)
    assert snap == fresh(c, calls)
    assert snap[2][0] == (2, 2 * 4 * 64 * 64)   # threshold 0: every pixel runs to max_spp, in two rounds
    assert _snap(old, PLAIN) == fresh(c)


# ---- (f) the counting launches ---------------------------------------------------------------------------------------
def test_counting_launches_then_a_plain_launch(old, S, fresh):
    """The six and the sixteen counters, and the film the two counting launches leave, equal a fresh context's.  A counting
    launch is the megakernel with counters: it folds its samples into the film like dmt_render does (the film is not left
    untouched), so after a plain launch and the two that count every pixel holds three times the samples."""
    c = _cfg(accel=1)
    _apply(old, S, c)
    calls = PLAIN + (("stats", SPP), ("profile", SPP))
    snap = _snap(old, calls)
    assert snap == fresh(c, calls)
    _, stats, profile = snap[2]
    assert len(stats) == 6 and len(profile) == 16 and stats["samples"] == profile["samples"] == 64 * 64 * SPP
    assert all(profile[k] == v for k, v in stats.items())
    assert (np.frombuffer(snap[1], np.float32).reshape(64, 64, 4)[..., 3] == 3 * SPP).all()
    assert _snap(old, PLAIN) == fresh(c)


# ---- (g) the wavefront form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [64, 32])
def test_wavefront_passes_then_the_megakernel(old, S, fresh, size):
    c = _cfg(size=size, accel=1, strategy=2, paths=4096)   # 64 x 64 x 8 spp: eight passes
    _apply(old, S, c)
    wave = _snap(old, PLAIN, items=False)
    assert wave == fresh(c, PLAIN, items=False)
    c = _cfg(size=size, accel=1)
    _apply(old, S, c)
    mega = _snap(old, PLAIN)
    assert mega == fresh(c) and mega[:2] == wave[:2]


# ---- (h) partitions --------------------------------------------------------------------------------------------------
@ACCELS
def test_partitions_sum_to_the_whole_film(old, S, fresh, accel):
    parts = {}
    for rank in (1, 0, 2):
        c = _cfg(accel=accel, part=(rank, 3))
        if rank == 1:
            _apply(old, S, c)
            assert _snap(old, PLAIN) == fresh(c)
        parts[rank] = fresh(c)
    c = _cfg(accel=accel)
    _apply(old, S, c)
    whole = _snap(old, PLAIN)
    assert whole == fresh(c)
    films = [[np.frombuffer(parts[k][i], np.float32).reshape(64, 64, 4) for k in range(3)] for i in (0, 1)]
    owners = sum((m2[..., 3] > 0).astype(int) for m2 in films[1])
    assert (owners == 1).all()   # each pixel is one rank's, so the sums below add zeros
    for i in (0, 1):
        assert (films[i][0] + films[i][1] + films[i][2]).tobytes() == whole[i]


# ---- (i) a refused launch leaves the layer as it was -----------------------------------------------------------------
@ACCELS
def test_refused_calls_change_nothing(old, pkg, S, fresh, accel):
    c = _cfg(accel=accel)
    _apply(old, S, c)
    old.kernel_time(reset=True)
    _refused(pkg, lambda: old.render(SPP, sample_offset=2**31 - 100), ERR_INVALID, "dmt_render: sample index overflows the 32-bit Halton index")
    if accel == 0:
        _refused(pkg, lambda: old.render_stats(SPP), ERR_STATE, "dmt_render_stats: only the BVH path has device counters")
    _refused(pkg, lambda: old.set_sampler_table(3), ERR_INVALID, "dmt_set_sampler_table: unknown mode")
    _refused(pkg, lambda: old.set_ggx_batch(65), ERR_INVALID, "dmt_set_ggx_batch: a batch is at most 64 hits (the queue's capacity)")
    assert old.kernel_time(reset=True)[1] == 0
    assert old.ggx_batch() == S.ggx_default
    assert _snap(old, PLAIN) == fresh(c)
    assert old.kernel_time(reset=True)[1] == 1


# ---- (j) timing and the kernel's facts -------------------------------------------------------------------------------
@ACCELS
def test_kernel_time_counts_launches(old, pkg, S, accel):
    c = _cfg(accel=accel)
    _apply(old, S, c)
    old.kernel_time(reset=True)
    for k in range(3):
        old.render(1, sample_offset=k)
    ms, n = old.kernel_time(reset=True)
    assert n == 3 and ms > 0.0
    assert old.kernel_time(reset=True) == (0.0, 0)
    r = pkg.Renderer(0)
    try:
        _apply(r, S, c)
        assert old.kernel_info() == r.kernel_info()
    finally:
        r.close()
