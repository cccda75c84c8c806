"""GGX batching (dmt_set_ggx_batch): a film rendered with GGX hits parked and shaded in batches equals the film rendered
with batching off byte for byte, in one process, for every way the queue of parked hits can fill and drain.  Every case
checks that the launches took back exactly the hits they parked and that dmt_sync passes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BS_OREN, BS_GGX_DIEL, BS_GGX_COND = 0, 1, 2


def _types(bsdfs):
    """Material type of every packed BSDF record: the high half of its second word."""
    return np.ascontiguousarray(bsdfs, np.uint8).reshape(-1, 32)[:, 4:8].copy().view(np.uint32)[:, 0] >> 16


def _with_materials(pkg, sc, keep):
    """`sc` with every record replaced by its first record of type `keep`."""
    t = _types(sc.bsdfs)
    row = sc.bsdfs[np.flatnonzero(t == keep)[0]]
    return pkg.host_scene.ArrayScene(sc.xs, sc.ys, sc.zs, sc.mat_id, np.tile(row, (sc.bsdfs.shape[0], 1)), sc.lights, sc.inf_lights,
                                     sc.camera)


def _film(r, batch, calls, chunk=0, part=(0, 1)):
    r.set_ggx_batch(batch)
    r.set_chunk(chunk)
    r.set_partition(*part)
    r.film_clear()
    r.sched_diag(reset=True)
    for s0, n in calls:
        r.render(n, sample_offset=s0)
    r.sync()   # fails if a launch took back fewer hits than it parked, or did not fold every chunk
    film = r.download_film()
    d = r.sched_diag(reset=True)
    assert d["ggx_parked"] == d["ggx_resumed"], d
    assert d["folds"] == d["launched"] > 0 and d["early_exits"] == 0, d
    return film, d


def _compare(r, sc, batch, spp, depth=8, calls=None, **kw):
    """Films at batch 0 and at `batch`, byte for byte; returns the two counter records."""
    default = r.ggx_batch()
    calls = calls or ((0, spp),)
    r.upload_scene(sc)
    r.set_limits(depth)
    r.set_accel(0)
    try:
        ref, d0 = _film(r, 0, calls, **kw)
        got, d = _film(r, batch, calls, **kw)
    finally:
        r.set_ggx_batch(default)
        r.set_chunk(0)
        r.set_partition(0, 1)
        r.clear_envmap()
    assert d0["ggx_parked"] == 0 and d0["ggx_shade_passes"] == 0 and d0["ggx_shaded_full"] == 0, d0   # off: nothing parks, nothing is counted
    assert np.isfinite(ref[0]).all() and (depth == 0 or ref[0][..., :3].max() > 0)   # (cap 0 shades nothing: a black film)
    assert np.array_equal(ref[0].view(np.uint32), got[0].view(np.uint32))
    assert np.array_equal(ref[1].view(np.uint32), got[1].view(np.uint32))
    return d0, d


@pytest.mark.parametrize("batch", [8, 64])
def test_cornell_film_is_bit_equal(renderer, pkg, batch):
    """Cornell 64 x 64 x 64 spp, cap 8.  Batch 8: the queue fills and empties all through the launch.  Batch 64 is the
    queue's capacity: hits come back when an item drains (or, rarely, when the queue is full)."""
    sc = pkg.host_scene.cornell_box(64, 64)
    assert (_types(sc.bsdfs) == BS_GGX_DIEL).any() or (_types(sc.bsdfs) == BS_GGX_COND).any()
    _, d = _compare(renderer, sc, batch, 64)
    assert d["ggx_parked"] > 1000, d
    if batch == 8:
        assert d["ggx_shade_passes"] < d["ggx_parked"], d   # hits were shaded together


def test_one_sample_chunks_hand_over(renderer, pkg):
    """64 x 64 x 32 spp in 1-sample chunks: items of 64 units, chunks finish out of order and are folded in chains."""
    sc = pkg.host_scene.cornell_box(64, 64)
    _, d = _compare(renderer, sc, 8, 32, chunk=1)
    assert d["ggx_parked"] > 0 and d["handed_over"] > 0, d


def test_every_hit_parks_and_the_queue_fills(renderer, pkg):
    """Every material is the GGX dielectric: every hit below the cap parks, free lanes start samples that park again, and
    hits that find the queue full are shaded at once -- more GGX passes than the drains alone would run."""
    sc = _with_materials(pkg, pkg.host_scene.cornell_box(32, 32), BS_GGX_DIEL)
    _, d = _compare(renderer, sc, 64, 16)
    # (an item here is 256 units: its wave's first 64 camera hits fill the queue, the next 64 find it full)
    assert d["ggx_parked"] >= 64 and d["ggx_shade_passes"] > 0, d
    assert d["ggx_shaded_full"] > 0, d   # the queue-full fallback fired


def test_no_ggx_material_parks_nothing(renderer, pkg):
    sc = _with_materials(pkg, pkg.host_scene.cornell_box(32, 32), BS_OREN)
    _, d = _compare(renderer, sc, 8, 16)
    assert d["ggx_parked"] == d["ggx_resumed"] == d["ggx_shade_passes"] == d["ggx_shaded_full"] == 0, d


@pytest.mark.parametrize("cap", [0, 1])
def test_low_bounce_caps(renderer, pkg, cap):
    """Cap 0: no hit is below the cap (st.depth < max_depth never holds) and nothing parks.  Cap 1: only the camera ray's hit
    is, so a parked hit is always a path's first and last shading."""
    sc = pkg.host_scene.cornell_box(64, 64)
    _, d = _compare(renderer, sc, 8, 16, depth=cap)
    if cap == 0:
        assert d["ggx_parked"] == d["ggx_resumed"] == d["ggx_shade_passes"] == d["ggx_shaded_full"] == 0, d
    else:
        assert d["ggx_parked"] > 0, d


def test_single_tile_frame(renderer, pkg):
    """8 x 8 x 64 spp: one tile, a handful of waves, each with one item at a time and nothing to draw from while it drains."""
    _compare(renderer, pkg.host_scene.cornell_box(8, 8), 8, 64)


def test_second_of_two_partitions(renderer, pkg):
    _, d = _compare(renderer, pkg.host_scene.cornell_box(64, 64), 8, 32, part=(1, 2))
    assert d["ggx_parked"] > 0, d


def test_two_calls_with_sample_offsets(renderer, pkg):
    _, d = _compare(renderer, pkg.host_scene.cornell_box(64, 64), 8, 32, calls=((0, 16), (16, 16)))
    assert d["ggx_parked"] > 0, d


def test_env_row_is_not_batched(renderer, pkg):
    """k_megakernel_env (a GGX conductor sphere on an Oren-Nayar plane under an importance-sampled sky, 32 x 32) is compiled
    without the batching code: the setting changes nothing there, and nothing is parked or counted."""
    sc = pkg.host_scene.sphere_envmap_scene(32, 32, lat=8, lon=16, env_height=16)
    assert (_types(sc.bsdfs) == BS_GGX_COND).any()
    _, d = _compare(renderer, sc, 8, 32)
    assert d["ggx_parked"] == d["ggx_resumed"] == d["ggx_shade_passes"] == d["ggx_shaded_full"] == 0, d
