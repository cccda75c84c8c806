"""dmt_sampler_table_plan (host only): when a render call tabulates its sampler values over the frame's 128-pixel Halton
period, and how a table larger than the memory budget is cut into sample slices."""
import pytest

MIB = 1 << 20
ENTRY = 40  # bytes per (sample, period pixel): 8 values + 2 jitter floats


@pytest.fixture(scope="module")
def plan(pkg):
    return pkg.binding.sampler_table_plan


def check_slices(p, spp, chunk):
    """The slices cover [0, spp) exactly once, none is empty, all but the last are whole chunks."""
    lens = p["slice_spp"]
    assert len(lens) == p["slices"] >= 1
    assert all(n > 0 for n in lens)
    assert sum(lens) == spp
    assert all(n % chunk == 0 for n in lens[:-1])
    assert len(set(lens[:-1])) <= 1                     # equal chunk counts
    assert lens[-1] <= lens[0]


def test_flagship_plan(plan):
    p = plan(1024, 1024, 1024 * 1024, 1024, 16, 512 * MIB)
    assert p["use"] and (p["period_width"], p["period_height"]) == (128, 128) and p["entry_bytes"] == ENTRY
    check_slices(p, 1024, 16)
    assert p["slice_bytes"] <= 512 * MIB
    assert p["slice_bytes"] == p["slice_spp"][0] * 128 * 128 * ENTRY
    # 640 MiB of table against 512 MiB: two slices of 32 chunks
    assert p["slice_spp"] == [512, 512]
    assert plan(1024, 1024, 1024 * 1024, 1024, 16, 1024 * MIB)["slice_spp"] == [1024]


@pytest.mark.parametrize("w,h,owned", [(128, 128, 128 * 128), (64, 64, 64 * 64), (100, 300, 3 * 64)])
def test_no_table_below_the_ratio_in_auto_mode(plan, pkg, w, h, owned):
    p = plan(w, h, owned, 64, 16)
    assert not p["use"] and p["slices"] == 0 and p["slice_spp"] == []
    assert (p["period_width"], p["period_height"]) == (min(w, 128), min(h, 128))
    forced = plan(w, h, owned, 64, 16, mode=pkg.binding.SAMPLER_TABLE_FORCE)
    assert forced["use"] and forced["slice_spp"] == [64]
    assert not plan(w, h, owned, 64, 16, mode=pkg.binding.SAMPLER_TABLE_OFF)["use"]


def test_ratio_threshold_is_four_periods(plan):
    assert plan(256, 256, 256 * 256, 64, 16)["use"]
    assert not plan(256, 256, 256 * 256 - 64, 64, 16)["use"]
    assert plan(1024, 1024, 1024 * 1024 // 8, 64, 16)["use"]          # one GPU's share of eight


def test_ragged_frame_period(plan):
    p = plan(200, 72, 25 * 9 * 64, 40, 16)
    assert (p["period_width"], p["period_height"]) == (128, 72)
    assert not p["use"]                                                # 14 400 owned pixels < 4 x 128 x 72
    p = plan(200, 72, 25 * 9 * 64, 40, 16, mode=2)
    assert p["use"] and p["slice_spp"] == [40] and p["slice_bytes"] == 40 * 128 * 72 * ENTRY


def test_budget_below_one_chunk_means_no_table(plan):
    one_chunk = 16 * 128 * 128 * ENTRY
    for mode in (1, 2):
        p = plan(1024, 1024, 1024 * 1024, 64, 16, one_chunk - 1, mode)
        assert not p["use"] and p["slices"] == 0 and p["slice_spp"] == []
        p = plan(1024, 1024, 1024 * 1024, 64, 16, one_chunk, mode)
        assert p["use"] and p["slice_spp"] == [16, 16, 16, 16]


@pytest.mark.parametrize("spp,chunk", [(40, 6), (40, 1), (40, 7), (1024, 16), (100, 512), (513, 512), (7, 16)])
def test_slices_cover_the_samples_over_a_budget_sweep(plan, spp, chunk):
    eff = min(chunk, spp)                                              # a launch never uses a chunk longer than the call
    chunk_bytes = eff * 128 * 128 * ENTRY
    chunks = -(-spp // eff)
    for k in range(1, chunks + 2):
        for extra in (0, 1, chunk_bytes - 1):
            budget = k * chunk_bytes + extra
            p = plan(264, 136, 33 * 17 * 64, spp, chunk, budget, 2)
            assert p["use"]
            check_slices(p, spp, eff)
            assert p["slice_bytes"] <= budget
            assert p["slices"] == -(-chunks // -(-chunks // -(-chunks // k)))   # ceil(chunks / k) slices, evened out


def test_short_last_slice(plan):
    p = plan(264, 136, 33 * 17 * 64, 40, 6, 3 * 6 * 128 * 128 * ENTRY, 2)
    assert p["slice_spp"] == [18, 18, 4]


def test_bad_arguments(pkg):
    with pytest.raises(pkg.DmtError):
        pkg.binding.sampler_table_plan(0, 64, 64, 8, 8)
    with pytest.raises(pkg.DmtError):
        pkg.binding.sampler_table_plan(64, 64, 64, 8, 8, mode=3)
