"""GPU tests of in-place vertex updates (dmt_update_vertices, dmt_update_vertices_device) and the device-side BVH refit
(dmt_set_accel_update, csrc/bvh_gpu_build.hip).

The pin of the refit kernels is exact: the downloaded tree equals the serial host restatement (dmt_bvh_refit_reference) in
all 64 bytes of every node.  Above that, the traversal contract (closest hits and films bit-identical to brute force and to
a fresh upload) and the state an update keeps: materials, emissive triangles, textures."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from test_bvh_gpu_build_gpu import _soup_for
from test_bvh_refit import deform, permuted
from test_parity_gpu import _random_soup, _rays

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
REBUILD, REFIT, AUTO = 0, 1, 2
BUILDERS = [pytest.param(HOST, id="host-sah"), pytest.param(DEVICE, id="device-lbvh")]


@pytest.fixture
def upd(renderer):
    """The session's renderer; accel, builder, update mode, env map and area lights are put back afterwards."""
    yield renderer
    renderer.set_accel(0)
    renderer.set_accel_build(HOST)
    renderer.set_accel_update(REBUILD)
    renderer.set_bvh_strategy(0, 1 << 22)
    renderer.clear_envmap()
    renderer.upload_area_lights([], np.zeros((0, 3), np.float32))
    renderer.upload_textures(None, None, None, None)


def _assert_same_nodes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} nodes differ, first {bad[:8]}: device {got[bad[0]].tolist()} "
                             f"expected {want[bad[0]].tolist()}")


def _assert_cost_agrees(pkg, r, nodes, pairs, soup):
    """The record's cost against dmt_bvh_check's of the downloaded tree: the same fp64 terms, only the order of <= 2^20
    positive additions differs (a worst case of about 1e-10 relative)."""
    rec = r.accel_update_info()
    c = pkg.bvh_check(nodes, pairs, *soup)
    assert c["ok"], c
    print(f"sah_cost: device {rec['sah_cost']!r}, check {c['sah_cost']!r}, at build {rec['sah_cost_at_build']!r}")
    assert abs(rec["sah_cost"] - c["sah_cost"]) <= 1e-9 * abs(c["sah_cost"])
    return rec, c


def _start(r, soup, builder, mode, ratio=0.0):
    n = soup[0].size // 4
    r.set_accel(0)
    r.set_accel_build(builder)
    r.upload_triangles(*soup, np.zeros(n, np.uint32))
    r.set_accel(1)
    r.set_accel_update(mode, ratio)
    assert r.accel_build_info()["builder"] == (0 if builder == HOST else 1)


@pytest.mark.parametrize("n", [1, 3, 26, 777, 20000, 1_000_000])
@pytest.mark.parametrize("builder", BUILDERS)
def test_refitted_tree_equals_the_restatement(upd, pkg, builder, n):
    soup = _soup_for(pkg, n)
    _start(upd, soup, builder, REFIT)
    built_nodes, built_pairs = upd.download_accel()
    build_rec = upd.accel_build_info()
    prev = built_nodes
    frames = (deform(soup, 0.1), deform(soup, 0.1, phase=1.7), soup)
    for k, frame in enumerate(frames):
        upd.update_vertices(*frame)
        nodes, pairs = upd.download_accel()
        assert np.array_equal(pairs, built_pairs)
        _assert_same_nodes(nodes, pkg.bvh_refit_reference(prev, built_pairs, *frame), f"frame {k}")
        rec, _ = _assert_cost_agrees(pkg, upd, nodes, pairs, frame)
        assert rec["action"] == pkg.BVH_UPDATED_REFIT and rec["updates_since_build"] == k + 1
        assert rec["update_ms"] > 0 and rec["temp_bytes"] >= 24 * (nodes.shape[0] + pairs.shape[0]) + 8 * nodes.shape[0]
        assert upd.accel_build_info() == build_rec            # still the build that made the topology
        prev = nodes
    _assert_same_nodes(nodes, built_nodes, "back at the build's positions")
    rec = upd.accel_update_info()
    assert abs(rec["sah_cost"] - rec["sah_cost_at_build"]) <= 1e-9 * rec["sah_cost_at_build"]


def test_refits_reuse_their_scratch(upd, pkg):
    """Two soups of one size alternate through updates in one context: the boxes per node and per pair, the padding word and
    the cost terms are reused with warm caches, so anything left over from the refit before shows as a difference from the
    restatement."""
    n = 300_000
    a, b = _random_soup(n, 41), _random_soup(n, 42, spread=5.0, size=0.2)
    _start(upd, a, DEVICE, REFIT)
    prev, pairs0 = upd.download_accel()
    for k, soup in enumerate((b, a, b, a)):
        upd.update_vertices(*soup)
        nodes, pairs = upd.download_accel()
        assert np.array_equal(pairs, pairs0)
        _assert_same_nodes(nodes, pkg.bvh_refit_reference(prev, pairs0, *soup), f"update {k}")
        _assert_cost_agrees(pkg, upd, nodes, pairs, soup)
        prev = nodes


@pytest.mark.parametrize("ntri", [26, 777, 20000])
@pytest.mark.parametrize("builder", BUILDERS)
def test_closest_hit_after_a_refit_equals_brute_force(upd, pkg, builder, ntri):
    soup = _soup_for(pkg, ntri)
    _start(upd, soup, builder, REFIT)
    moved = deform(soup, 1.0)
    upd.update_vertices(*moved)
    assert upd.accel_update_info()["action"] == pkg.BVH_UPDATED_REFIT
    o, d = _rays(8192, ntri + 1)
    ai, at = upd.test_closest_hit(o, d)
    upd.set_accel(0)
    bi, bt = upd.test_closest_hit(o, d)
    assert np.array_equal(ai, bi)
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32))
    if ntri >= 777:
        assert (ai >= 0).mean() > 0.02


@pytest.mark.parametrize("builder", BUILDERS)
def test_guard_pairs_after_a_refit(upd, pkg, builder):
    """test_empty_slots_axis_parallel_rays after an update: the refit rewrites the three guard pairs behind the array."""
    def tri(p0, p1, p2):
        return [p0[0], p1[0], p2[0], 0.0], [p0[1], p1[1], p2[1], 0.0], [p0[2], p1[2], p2[2], 0.0]
    for nfloor in (1, 2, 3):
        t = [tri((-1, 0, -1), (1, 0, -1), (1, 0, 1)), tri((-1, 0, -1), (1, 0, 1), (-1, 0, 1)), tri((2, 0, 2), (3, 0, 2), (3, 0, 3))][:nfloor]
        xs = np.array([a[0] for a in t], np.float32).reshape(-1, 4); ys = np.array([a[1] for a in t], np.float32).reshape(-1, 4)
        zs = np.array([a[2] for a in t], np.float32).reshape(-1, 4)
        _start(upd, (xs + np.float32(7.0), ys, zs * np.float32(0.5)), builder, REFIT)   # built somewhere else
        upd.update_vertices(xs, ys, zs)
        assert upd.accel_update_info()["action"] == pkg.BVH_UPDATED_REFIT
        g = np.linspace(-1.5, 3.5, 41, dtype=np.float32)
        gx, gz = np.meshgrid(g, g)
        n = gx.size
        o = np.stack([gx.ravel(), np.full(n, 5.0, np.float32), gz.ravel()], axis=1).astype(np.float32)
        d = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (n, 1))
        o = np.concatenate([o, o * np.array([1, -1, 1], np.float32), np.stack([np.full(n, -9.0, np.float32), gz.ravel() * 0, gx.ravel()], axis=1)])
        d = np.concatenate([d, -d, np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))])
        ai, at = upd.test_closest_hit(o, d)
        upd.set_accel(0)
        bi, bt = upd.test_closest_hit(o, d)
        assert np.array_equal(ai, bi) and np.array_equal(at.view(np.uint32), bt.view(np.uint32))
        assert (ai >= 0).sum() > 100


def _film(r, spp, accel):
    r.set_accel(accel)
    r.film_clear()
    r.render(spp)
    r.sync()
    return r.download_film()


def _moved_cornell(pkg):
    """The Cornell parity scene and the same with its first sphere's eight triangles translated."""
    a, b = pkg.host_scene.cornell_box(64, 64), pkg.host_scene.cornell_box(64, 64)
    b.xs[:8, :3] += np.float32(0.4); b.ys[:8, :3] -= np.float32(0.3); b.zs[:8, :3] += np.float32(0.5)
    return a, b


@pytest.fixture(scope="module")
def from_device_memory(tmp_path_factory):
    """The update_vertices_device cases, run once in a child process (tests/_refit_device_worker.py): torch must open the
    GPU before the HIP library does, which this session's renderer has long done."""
    out = tmp_path_factory.mktemp("refit_device") / "out.npz"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve().parent / "_refit_device_worker.py"), str(out)], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("accel", [pytest.param(1, id="bvh"), pytest.param(0, id="brute-force")])
def test_films_after_an_update_equal_a_fresh_upload(pkg, from_device_memory, accel):
    """(a) fresh upload of the moved scene, (b) update with REFIT, (c) update with REBUILD, (d) update from a torch tensor's
    device memory: the four films agree in every bit.  Under brute force this proves the cull clusters were replanned."""
    original, moved = _moved_cornell(pkg)
    spp = 16
    films = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(moved)
        r.set_limits(8)
        films["fresh"] = _film(r, spp, accel)
    for tag, mode in (("refit", REFIT), ("rebuild", REBUILD)):
        with pkg.Renderer(0) as r:
            r.upload_scene(original)
            r.set_limits(8)
            r.set_accel(accel)
            r.set_accel_update(mode)
            before = _film(r, spp, accel)
            r.update_vertices(moved.xs, moved.ys, moved.zs)
            want = (pkg.BVH_UPDATED_REFIT if mode == REFIT else pkg.BVH_UPDATED_REBUILD) if accel == 1 else pkg.BVH_UPDATED_NONE
            assert r.accel_update_info()["action"] == want
            films[tag] = _film(r, spp, accel)
            assert not np.array_equal(before[0], films[tag][0])          # the sphere did move
    key = "cornell_bvh" if accel == 1 else "cornell_brute"
    assert from_device_memory[key + "_action"] == (pkg.BVH_UPDATED_REFIT if accel == 1 else pkg.BVH_UPDATED_NONE)
    assert from_device_memory[key + "_moved"]
    films["device"] = (from_device_memory[key + "_mean"], from_device_memory[key + "_m2"])
    for tag in ("refit", "rebuild", "device"):
        assert np.array_equal(films[tag][0], films["fresh"][0]) and np.array_equal(films[tag][1], films["fresh"][1]), tag
    assert films["fresh"][0][..., :3].max() > 0


def _records_scene(pkg):
    sc = pkg.host_scene.random_triangle_scene(4000, width=48, height=48)
    return sc, deform((sc.xs, sc.ys, sc.zs), 0.1)


def test_device_records_equal_the_host_packer(pkg, from_device_memory):
    """The record kernel against the host packer: after update_vertices_device and after update_vertices of the same soup,
    films (whose samples read TriIsect and TriPost, the normal included) agree in every bit under BVH and under brute
    force, as do the refitted trees."""
    sc, moved = _records_scene(pkg)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(8)
        r.set_accel(1)
        r.set_accel_update(REFIT)
        r.update_vertices(*moved)
        bvh, (nodes, pairs), brute = _film(r, 4, 1), r.download_accel(), _film(r, 4, 0)
    d = from_device_memory
    assert np.array_equal(bvh[0], d["records_bvh_mean"]) and np.array_equal(bvh[1], d["records_bvh_m2"])
    assert np.array_equal(brute[0], d["records_brute_mean"]) and np.array_equal(brute[1], d["records_brute_m2"])
    assert np.array_equal(nodes, d["records_nodes"]) and np.array_equal(pairs, d["records_pairs"])
    assert np.array_equal(bvh[0], brute[0]) and bvh[0][..., :3].max() > 0


def test_area_lights_survive_an_update(upd, pkg):
    """The PBRT Cornell box (emissive triangles) with a non-emissive box moved: the film after the update equals the film of
    a fresh upload followed by the same upload_area_lights."""
    hs = pkg.host_scene.load_pbrt(GOLDEN / "pbrt" / "cornell_box.pbrt")
    hs.set_resolution(64, 64)
    assert len(hs.area_tri) > 0
    emissive_mats = set(hs.mat_id[hs.area_tri].tolist())
    mat = [m for m in np.unique(hs.mat_id)[::-1] if m not in emissive_mats and (hs.mat_id == m).sum() >= 10][0]   # a box: 12 triangles
    sel = hs.mat_id == mat
    assert not np.isin(hs.area_tri, np.flatnonzero(sel)).any()
    xs, ys, zs = hs.xs.copy(), hs.ys.copy(), hs.zs.copy()
    ext = max(float(np.ptp(hs.xs[:, :3])), float(np.ptp(hs.ys[:, :3])), float(np.ptp(hs.zs[:, :3])))
    xs[sel, :3] += np.float32(0.08 * ext)
    for accel in (1, 0):
        upd.set_accel_update(REFIT)
        upd.upload_scene(hs)
        upd.set_limits(hs.max_depth)
        before = _film(upd, 8, accel)
        upd.update_vertices(xs, ys, zs)
        updated = _film(upd, 8, accel)
        upd.set_accel(0)
        upd.upload_triangles(xs, ys, zs, hs.mat_id)             # clears the emissive-triangle list
        upd.upload_area_lights(hs.area_tri, hs.area_le)
        fresh = _film(upd, 8, accel)
        assert np.array_equal(updated[0], fresh[0]) and np.array_equal(updated[1], fresh[1])
        assert not np.array_equal(updated[0], before[0]) and updated[0][..., :3].max() > 0


def test_textures_survive_an_update(upd, pkg, tmp_path):
    """three_boxes.json with a texture on its floor, updated to other positions and then back to its own: it renders its
    original film, textures and UVs untouched."""
    src = GOLDEN / "json_scene"
    shutil.copy(src / "sky_32x16.png", tmp_path / "sky_32x16.png")
    shutil.copy(GOLDEN / "scene_test" / "res" / "textures" / "chippedPaint" / "Paint_Chipped_1K_albedo.png", tmp_path / "albedo.png")
    d = json.loads((src / "three_boxes.json").read_text())
    d["textures"] = [{"name": "paint", "type": "diffuse", "path": "./albedo.png"}]
    [m for m in d["materials"] if "oren-nayar-dielectric" in m][0]["diffuse"] = "paint"
    (tmp_path / "textured.json").write_text(json.dumps(d))
    hs = pkg.host_scene.load_json(tmp_path / "textured.json")
    assert hs.tex_desc is not None
    for accel in (1, 0):
        upd.set_accel_update(REFIT)
        upd.upload_scene(hs)
        upd.set_limits(hs.max_depth)
        original = _film(upd, 8, accel)
        upd.update_vertices(*deform((hs.xs, hs.ys, hs.zs), 0.3))
        away = _film(upd, 8, accel)
        upd.update_vertices(hs.xs, hs.ys, hs.zs)
        back = _film(upd, 8, accel)
        assert not np.array_equal(away[0], original[0])
        assert np.array_equal(back[0], original[0]) and np.array_equal(back[1], original[1])
    with pkg.Renderer(0) as plain:                              # the texture is what is being rendered
        hs.tex_desc = None
        plain.upload_scene(hs)
        plain.set_limits(hs.max_depth)
        assert not np.array_equal(_film(plain, 8, 1)[0], original[0])


@pytest.mark.parametrize("builder", BUILDERS)
def test_rebuild_mode_equals_a_fresh_upload(upd, pkg, builder):
    soup = _soup_for(pkg, 20000)
    moved = deform(soup, 1.0)
    _start(upd, soup, builder, REBUILD)
    upd.update_vertices(*moved)
    rec = upd.accel_update_info()
    assert rec["action"] == pkg.BVH_UPDATED_REBUILD and rec["updates_since_build"] == 0 and rec["sah_cost"] == 0
    assert rec["update_ms"] >= upd.accel_build_info()["build_ms"] > 0
    nodes, pairs = upd.download_accel()
    upd.upload_triangles(*moved, np.zeros(20000, np.uint32))
    fresh_nodes, fresh_pairs = upd.download_accel()
    assert np.array_equal(pairs, fresh_pairs)
    _assert_same_nodes(nodes, fresh_nodes, "rebuild against fresh upload")


@pytest.mark.parametrize("builder", BUILDERS)
def test_auto_mode_refits_until_the_cost_passes_the_ratio(upd, pkg, builder):
    soup = _soup_for(pkg, 20000)
    _start(upd, soup, builder, AUTO, 2.0)
    smooth = deform(soup, 0.1)
    upd.update_vertices(*smooth)
    rec = upd.accel_update_info()
    print(f"A = 0.1: cost ratio {rec['sah_cost'] / rec['sah_cost_at_build']:.4f}")
    assert rec["action"] == pkg.BVH_UPDATED_REFIT and rec["updates_since_build"] == 1
    assert rec["sah_cost"] <= 2.0 * rec["sah_cost_at_build"]
    shuffled = permuted(soup)
    upd.update_vertices(*shuffled)
    rec = upd.accel_update_info()
    assert rec["action"] == pkg.BVH_UPDATED_REBUILD_AFTER_REFIT and rec["updates_since_build"] == 0
    nodes, pairs = upd.download_accel()
    c = pkg.bvh_check(nodes, pairs, *shuffled)
    assert c["ok"], c
    if builder == DEVICE:
        ref = pkg.lbvh_reference(*shuffled)
        assert np.array_equal(pairs, ref["pairs"])
        _assert_same_nodes(nodes, ref["nodes"], "rebuild after refit against the restatement of a fresh build")
    else:
        with pkg.Renderer(0) as fresh:
            fresh.upload_triangles(*shuffled, np.zeros(20000, np.uint32))
            fresh.set_accel(1)
            fc = pkg.bvh_check(*fresh.download_accel(), *shuffled)
        assert fc["ok"] and abs(c["sah_cost"] - fc["sah_cost"]) <= 1e-9 * fc["sah_cost"]
    assert abs(rec["sah_cost"] - c["sah_cost"]) <= 1e-9 * c["sah_cost"] and rec["sah_cost_at_build"] == rec["sah_cost"]


@pytest.mark.parametrize("builder", BUILDERS)
def test_cost_of_the_record_is_the_checkers(upd, pkg, builder):
    soup = _soup_for(pkg, 20000)
    _start(upd, soup, builder, REFIT)
    built = pkg.bvh_check(*upd.download_accel(), *soup)["sah_cost"]
    for amplitude in (0.1, 1.0):
        moved = deform(soup, amplitude)
        upd.update_vertices(*moved)
        rec, c = _assert_cost_agrees(pkg, upd, *upd.download_accel(), moved)
        assert abs(rec["sah_cost_at_build"] - built) <= 1e-9 * built
        assert rec["sah_cost"] != rec["sah_cost_at_build"]


def test_brute_force_update_drops_the_tree(upd, pkg):
    soup = _soup_for(pkg, 777)
    _start(upd, soup, HOST, REFIT)
    upd.set_accel(0)
    upd.update_vertices(*deform(soup, 0.1))
    assert upd.accel_update_info()["action"] == pkg.BVH_UPDATED_NONE
    assert upd.accel_build_info()["nodes"] == 0                  # no tree, as after an upload under brute force
    with pytest.raises(pkg.DmtError):
        upd.download_accel()


def test_update_errors(upd, pkg):
    with pkg.Renderer(0) as r:
        z = np.zeros((4, 4), np.float32)
        with pytest.raises(pkg.DmtError, match=r"\(3\)"):       # DMT_ERR_STATE: nothing uploaded yet
            r.update_vertices(z, z, z)
        with pytest.raises(pkg.DmtError, match=r"\(3\)"):
            r.update_vertices_device(0, 0)
        for ratio in (1.0, 0.5, 0.0, -3.0, float("nan"), float("inf")):
            with pytest.raises(pkg.DmtError, match=r"\(1\)"):   # DMT_ERR_INVALID
                r.set_accel_update(AUTO, ratio)
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):
            r.set_accel_update(3)
        r.set_accel_update(AUTO, 1.5)
        r.set_accel_update(REFIT, float("nan"))                 # ignored outside AUTO
        xs, ys, zs = _random_soup(100, 5)
        r.upload_triangles(xs, ys, zs, np.zeros(100, np.uint32))
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):       # a wrong count
            r.update_vertices(xs[:99], ys[:99], zs[:99])
        with pytest.raises(pkg.DmtError, match=r"\(1\)"):
            r.update_vertices_device(0, 100)                    # a null device pointer
        e = np.zeros((0, 4), np.float32)
        r.upload_triangles(e, e, e, np.zeros(0, np.uint32))
        r.update_vertices(e, e, e)                              # the empty soup: a no-op
        r.update_vertices_device(0, 0)


def test_a_render_in_flight_finishes_on_the_old_records(pkg):
    original, moved = _moved_cornell(pkg)
    original.set_resolution(128, 128)
    with pkg.Renderer(0) as r:
        r.upload_scene(original)
        r.set_limits(8)
        r.set_accel(1)
        r.set_accel_update(REFIT)
        want = _film(r, 64, 1)
        r.film_clear()
        r.render(64)                                            # asynchronous: still running when the update arrives
        r.update_vertices(moved.xs, moved.ys, moved.zs)
        r.sync()                                                # DMT_OK: every chunk folded exactly once
        got = r.download_film()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        after = _film(r, 64, 1)
        assert not np.array_equal(after[0], want[0])
