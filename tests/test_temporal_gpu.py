"""Temporal accumulation on the GPU (dmt_denoise_temporal).  The reprojection kernel is checked against
the numpy restatement (tests/temporal_ref.py) on synthetic inputs with real motion and on the Cornell box with a moved box;
the accumulation against the plain mean of the frames; alpha = 1 against dmt_denoise; its invariance under a common
translation of scene and camera; the history across update_vertices against update_vertices_device; the surface plane
against the camera-ray and closest-hit probes; the C ABI's invariants; and the quality on two scenes against dmt_denoise of
the last frame alone.

Where a device result is compared with the restatement, only the restatement's near-threshold mask is left out, and a mask
over temporal_ref.MASK_CAP of the pixels fails the test."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as T
from conftest import GOLDEN
from test_temporal import moving_pair

pytestmark = pytest.mark.gpu

F = np.float32
RES = 64
# lower bounds of RMSE(dmt_denoise of frame 8) / RMSE(dmt_denoise_temporal at frame 8), 8 frames of 4 spp at 256 x 256 with
# the defaults and AOVs of 4 spp: at most 0.75 of the measured ratios (profiles/temporal/sweep.txt: 1.490 and
# 1.039; the renders are deterministic).  The ratio must also exceed 1.
QUALITY = {"cornell": 1.1, "c3_sphere_veranda": 0.77}


def _soup(verts):
    """[n, 9] raw vertices -> the xs, ys, zs of dmt_upload_triangles"""
    v = np.asarray(verts, F).reshape(-1, 3, 3)
    out = [np.zeros((v.shape[0], 4), F) for _ in range(3)]
    for a in range(3):
        out[a][:, :3] = v[:, :, a]
    return out


def _close(got, ref, keep, what):
    scale = float(np.abs(ref[keep]).mean())
    np.testing.assert_allclose(got[keep], ref[keep], rtol=1e-4, atol=1e-4 * scale, err_msg=what)


def _mask_ok(mask):
    share = float(mask.mean())
    print(f"near-threshold mask: {int(mask.sum())} pixels, {100 * share:.3f} %")
    assert share <= T.MASK_CAP, share
    return ~mask


@pytest.fixture(scope="module")
def cb(pkg):
    r = pkg.Renderer(0)
    sc = pkg.host_scene.cornell_box(RES, RES)
    r.upload_scene(sc)
    r.set_limits(5)
    yield r, sc
    r.close()


def _fresh(r, sc):
    r.upload_scene(sc)
    r.set_accel(0)
    r.set_camera(sc.camera)
    r.temporal_reset()


def _frame(r, j, spp=4, aov_spp=1):
    """frame j of an animation: its own film from sample offset spp j, and the feature planes"""
    r.film_clear()
    r.render(spp, sample_offset=spp * j)
    r.render_aovs(aov_spp)
    return r.download_film()


# ---- (a) device vs restatement, synthetic ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_a_reprojection_matches_the_restatement(pkg, seed):
    h, w = 50, 80  # not a multiple of the 64 x 4 block
    a, b = moving_pair(h, w, seed)
    with pkg.Renderer(0) as r:
        r.upload_triangles(*_soup(a["verts"]), np.zeros(a["verts"].shape[0], np.uint32))
        r.set_camera(a["camera"])
        r.upload_aovs(a["albedo"], a["normal"], a["position"])
        r.upload_aov_surface(a["surface"])
        mean_a, m2_a = a["film"](3)
        out_a = r.denoise_temporal(film=(mean_a, m2_a))
        ref_a, hist, info_a = T.step(None, mean_a, m2_a, a["albedo"], a["normal"], a["position"], a["surface"], a["verts"], a["verts"],
                                     a["camera"])
        cv, ln = r.download_history()
        assert np.array_equal(cv[..., :3].view(np.uint32), hist["c"].view(np.uint32))  # a reset copies the current plane
        assert np.array_equal(ln, hist["h"])
        every = np.ones((h, w), bool)
        _close(out_a, ref_a, every, "frame A, filtered")
        ia = r.temporal_info()
        assert (ia["frames"], ia["reprojected"], ia["reset"]) == (1, 0, info_a["reset"])
        r.update_vertices(*_soup(b["verts"]))
        r.set_camera(b["camera"])
        r.upload_aovs(b["albedo"], b["normal"], b["position"])
        r.upload_aov_surface(b["surface"])
        for params in (None, dict(alpha=0.0, normal_threshold=0.5, plane_threshold=8.0)):
            mean_b, m2_b = b["film"](4)
            # the restatement continues from the device's own history, so that nothing but this call is compared
            cv, ln = r.download_history()
            hist_dev = T.history(cv[..., :3], cv[..., 3], ln, hist["normal"], hist["position"], hist["camera"])
            out_b = r.denoise_temporal(temporal=params, film=(mean_b, m2_b))
            ref_b, hist_b, info = T.step(hist_dev, mean_b, m2_b, b["albedo"], b["normal"], b["position"], b["surface"], b["verts"],
                                         a["verts"] if params is None else b["verts"], b["camera"], temporal=params)
            keep = _mask_ok(info["mask"])
            cv2, ln2 = r.download_history()
            _close(cv2[..., :3], hist_b["c"], keep, "accumulated colour")
            _close(cv2[..., 3], hist_b["v"], keep, "accumulated variance")
            np.testing.assert_allclose(ln2[keep], hist_b["h"][keep], rtol=0, atol=1e-4, err_msg="history length")
            ib = r.temporal_info()
            masked = int(info["mask"].sum())
            assert abs(ib["reprojected"] - info["reprojected"]) <= masked and abs(ib["reset"] - info["reset"]) <= masked
            assert ib["reprojected"] + ib["reset"] == int((b["albedo"][..., 3] > 0).sum())
            assert ib["reprojected"] > 0 and ib["temporal_ms"] > 0
            # the a-trous passes run unchanged on the new history: restated on the device's own plane, every pixel
            fc, fv = cv2[..., :3], cv2[..., 3]
            for i in range(DR.DEFAULTS["iterations"]):
                fc, fv = DR.atrous_pass(fc, fv, b["albedo"], b["normal"], b["position"], 1 << i, DR.theta(b["camera"]),
                                        *(DR.DEFAULTS[k] for k in ("sigma_normal", "sigma_position", "sigma_albedo", "sigma_luminance")))
            _close(out_b[..., :3], fc, every, "filtered")
            hist = dict(hist_b, normal=b["normal"], position=b["position"], camera=b["camera"])
        r.temporal_reset()
        mean_b, m2_b = b["film"](5)
        out0 = r.denoise_temporal({"iterations": 0}, film=(mean_b, m2_b))
        assert np.array_equal(out0[..., :3].view(np.uint32), mean_b[..., :3].view(np.uint32))  # after a reset: the film itself


def test_a_device_pointer_updates_keep_the_history_frames_vertices(tmp_path):
    """Frame A, an update to B's vertices, frame B (the synthetic pair of the test above, seed 1), four ways in one child
    process (tests/_temporal_device_worker.py: torch must open the GPU before the HIP library does): update_vertices,
    update_vertices_device from a torch tensor, and each with an update to the midpoint first.  k_temporal reads only the
    planes, the two cameras and the two raw-vertex arrays; after B those hold the same floats whichever way they arrived,
    and the history frame's vertices are A's in all four runs, so everything agrees bit for bit.  Were the history frame's
    vertices snapshotted again by the second update, they would be the midpoint's and `reprojected` would move."""
    out = tmp_path / "out.npz"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve().parent / "_temporal_device_worker.py"), str(out)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    d = dict(np.load(out))
    frames, reprojected, reset = (int(x) for x in d["host_info"])
    print(f"host: frames {frames}, reprojected {reprojected}, reset {reset}")
    assert frames == 2 and reprojected > 0
    for tag in ("device", "host_twice", "device_twice"):
        print(f"{tag}: (frames, reprojected, reset) {tuple(int(x) for x in d[tag + '_info'])}")
        assert np.array_equal(d[tag + "_info"], d["host_info"]), tag
        for plane in ("out", "cv", "len"):
            assert np.array_equal(d[f"{tag}_{plane}"].view(np.uint32), d[f"host_{plane}"].view(np.uint32)), (tag, plane)


def test_a_camera_projection_probe_matches_the_host(cb, pkg):
    r, sc = cb
    rng = np.random.default_rng(5)
    P = rng.uniform(-2, 2, (4096, 3)).astype(F) + np.array([0, 3, 0], F)
    xy_d, depth_d = r.test_camera_project(P)
    xy_h, depth_h = pkg.camera_project(sc.camera, P)
    assert np.array_equal(depth_d, depth_h)
    # same order of operations; the device divides by reciprocal and one residual step, the host by IEEE division
    np.testing.assert_allclose(xy_d, xy_h, rtol=0, atol=2 * 2.0 ** -23 * RES)
    assert (xy_d == xy_h).mean() > 0.99


# ---- (b), (c), (d) the Cornell box -------------------------------------------------------------------------------------
def _static_run(r, sc, k=8, temporal=None):
    """k frames of 4 spp of the unmoved scene; returns (outputs, histories, films)"""
    _fresh(r, sc)
    outs, hists, used = [], [], []
    for j in range(k):
        film = _frame(r, j)
        used.append(film)
        outs.append(r.denoise_temporal({"iterations": 0}, temporal))
        hists.append(r.download_history())
    return outs, hists, used


def test_b_alpha_zero_accumulates_the_plain_mean(cb):
    r, sc = cb
    try:
        outs, hists, _ = _static_run(r, sc, temporal={"alpha": 0.0})
        r.film_clear()
        r.render(32)
        mean32, _ = r.download_film()
        a, _, _ = r.download_aovs()
        covered = a[..., 3] > 0
        assert covered.mean() > 0.9
        for j, (_, ln) in enumerate(hists):
            assert np.array_equal(ln, np.where(covered, F(j + 1), F(0))), j
        info = r.temporal_info()
        assert info["frames"] == 8 and info["reprojected"] == int(covered.sum()) and info["reset"] == 0
        _close(outs[-1][..., :3], mean32[..., :3], np.ones_like(covered), "mean of 8 x 4 spp vs 32 spp")
    finally:
        _fresh(r, sc)


def test_c_alpha_one_is_dmt_denoise_bit_for_bit(cb):
    r, sc = cb
    try:
        _fresh(r, sc)
        for j in range(3):
            _frame(r, j, aov_spp=4)
            got = r.denoise_temporal(temporal={"alpha": 1.0})
            want = r.denoise()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), j
        info = r.temporal_info()
        assert info["frames"] == 3 and info["reprojected"] > 0
    finally:
        _fresh(r, sc)


def test_d_common_translation_of_scene_and_camera_changes_nothing(pkg):
    """The path tracer's own films are not compared (a translated scene rounds differently along every path): both runs
    accumulate the static run's films, so that the difference is the reprojection's alone.

    Resolution 32 x 32, from the number format: under a common translation the motion is not exactly 0 but a few quanta of
    the fp32 film coordinate, q = 2^-23 x 16 = 1.9e-6 pixels for fx in [16, 32).  Bilinear weights (1 - e, e) shrink the
    reprojected variance by the factor sum w^2 = 1 - 2 e, whatever the sign of the motion, so 7 blends at e of one to three
    quanta lose 3 to 8 parts in 10^5 of it against the static run (measured: 7.5e-5 at the worst pixel after 7 blends): under
    the comparison's rtol of 1e-4.  At 64 x 64 the quantum doubles and the same sum reaches the tolerance (measured: one
    pixel at 1.36e-4 after 5 blends); DESIGN.md 4.12 states this growth with resolution as a limitation."""
    res = 32
    sc = pkg.host_scene.cornell_box(res, res)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(5)
        outs0, hists0, films = _static_run(r, sc, temporal={"alpha": 0.0})
        move = (0.011, -0.023, 0.017)
        _fresh(r, sc)
        mask = np.zeros((res, res), bool)
        hist = None
        outs1, hists1 = [], []
        verts_prev = None
        for j in range(8):
            d = np.asarray(move, F) * F(j)
            xs, ys, zs = np.asarray(sc.xs, F) + d[0], np.asarray(sc.ys, F) + d[1], np.asarray(sc.zs, F) + d[2]
            r.update_vertices(xs, ys, zs)
            cam = np.ascontiguousarray(sc.camera, np.uint8).copy()
            cam.view(np.float32)[3:6] += d
            r.set_camera(cam)
            r.render_aovs(1)
            aovs, surface = r.download_aovs(), r.download_aov_surface()
            verts = T.verts9(xs, ys, zs)
            outs1.append(r.denoise_temporal({"iterations": 0}, {"alpha": 0.0}, film=films[j]))
            _, new, info = T.step(hist, *films[j], *aovs, surface, verts, verts if verts_prev is None else verts_prev, cam,
                                  temporal={"alpha": 0.0}, denoise={"iterations": 0})
            mask |= info["mask"]
            cv, ln = r.download_history()
            hists1.append((cv, ln))
            hist = T.history(cv[..., :3], cv[..., 3], ln, aovs[1], aovs[2], cam)  # continue from the device's history
            verts_prev = verts
        keep = _mask_ok(mask)
        assert (hists0[-1][1] == 8).mean() > 0.9
        for j in range(8):
            np.testing.assert_allclose(hists1[j][1][keep], hists0[j][1][keep], rtol=0, atol=1e-4, err_msg=f"h, frame {j}")
            for what, got, ref in (("colour", hists1[j][0][..., :3], hists0[j][0][..., :3]), ("variance", hists1[j][0][..., 3], hists0[j][0][..., 3]),
                                   ("output", outs1[j][..., :3], outs0[j][..., :3])):
                err = np.abs(got[keep] - ref[keep]) / np.maximum(np.abs(ref[keep]), 1e-30)
                print(f"frame {j} {what}: worst relative difference {float(err.max()):.3e}")
                _close(got, ref, keep, f"{what}, frame {j}")


# ---- (e) disocclusion --------------------------------------------------------------------------------------------------
def test_e_a_moved_box_resets_what_it_uncovers(cb):
    r, sc = cb
    try:
        _fresh(r, sc)
        film0 = _frame(r, 0)
        aov0, surf0 = r.download_aovs(), r.download_aov_surface()
        r.denoise_temporal()
        cv, ln = r.download_history()
        hist = T.history(cv[..., :3], cv[..., 3], ln, aov0[1], aov0[2], sc.camera)
        xs = np.asarray(sc.xs, F).copy()
        box = np.asarray(sc.mat_id) == 0
        xs[box] += F(0.35)
        r.update_vertices(xs, sc.ys, sc.zs)
        film1 = _frame(r, 1)
        aov1, surf1 = r.download_aovs(), r.download_aov_surface()
        out = r.denoise_temporal()
        cv1, ln1 = r.download_history()
        ref, new, info = T.step(hist, *film1, *aov1, surf1, T.verts9(xs, sc.ys, sc.zs), T.verts9(sc.xs, sc.ys, sc.zs), sc.camera)
        keep = _mask_ok(info["mask"])
        _close(cv1[..., :3], new["c"], keep, "colour")
        _close(cv1[..., 3], new["v"], keep, "variance")
        np.testing.assert_allclose(ln1[keep], new["h"][keep], rtol=0, atol=1e-4)
        tri0, tri1 = surf0[..., 0].astype(int), surf1[..., 0].astype(int)
        on_box0, on_box1 = (tri0 >= 0) & (tri0 < 8), (tri1 >= 0) & (tri1 < 8)
        same_wall = (tri0 == tri1) & (tri1 >= 16)                 # a wall, the floor or the ceiling in both frames
        uncovered = on_box0 & ~on_box1 & (tri1 >= 16)             # the box stood before this wall pixel
        assert same_wall.sum() > 1000 and uncovered.sum() > 20, (same_wall.sum(), uncovered.sum())
        assert (ln1[same_wall & keep] == 2).all()
        assert (ln1[uncovered & keep] == 1).all()
        # the box itself moved by a fraction of a pixel grid: its interior reprojects with bilinear taps
        moved = on_box0 & on_box1 & (tri0 == tri1) & keep
        assert (ln1[moved] == 2).mean() > 0.8
        info_d = r.temporal_info()
        masked = int(info["mask"].sum())
        assert abs(info_d["reprojected"] - info["reprojected"]) <= masked and abs(info_d["reset"] - info["reset"]) <= masked
    finally:
        _fresh(r, sc)


# ---- (f) the surface plane ---------------------------------------------------------------------------------------------
def test_f_surface_plane_is_sample_zeros_hit(cb):
    r, sc = cb
    try:
        _fresh(r, sc)
        r.render_aovs(1)
        one = r.download_aov_surface()
        r.render_aovs(4)
        bf = r.download_aov_surface()
        three = r.download_aovs()
        r.set_accel(1)
        r.render_aovs(4)
        bvh = r.download_aov_surface()
        assert np.array_equal(bf.view(np.uint32), bvh.view(np.uint32))
        for x, y in zip(three, r.download_aovs()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        r.set_accel(0)
        yy, xx = np.mgrid[0:RES, 0:RES]
        px, py = xx.ravel(), yy.ravel()
        first = np.full(px.size, -1)
        first_od = np.zeros((px.size, 2, 3))
        for s in range(4):
            o, d = r.test_camera_rays(px, py, np.full_like(px, s))
            tri, _ = r.test_closest_hit(o, d)
            take = (first < 0) & (tri >= 0)
            first[take] = tri[take]
            first_od[take, 0], first_od[take, 1] = o[take], d[take]
            if s == 0:
                assert np.array_equal(one[..., 0].ravel(), tri.astype(F))  # aov_spp = 1: sample 0 or nothing
        got = bf.reshape(-1, 4)
        assert np.array_equal(got[:, 0], first.astype(F))
        hit = first >= 0
        assert hit.mean() > 0.9
        assert np.array_equal(got[:, 3], hit.astype(F)) and (got[~hit, 1:] == 0).all()
        # the barycentrics: float64 Moeller-Trumbore on the probe's ray
        V = T.verts9(sc.xs, sc.ys, sc.zs).reshape(-1, 3, 3).astype(np.float64)[np.maximum(first, 0)]
        o, d = first_od[:, 0], first_od[:, 1]
        e0, e1 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        pv = np.cross(d, e1)
        det = np.einsum("ij,ij->i", e0, pv)
        tv = o - V[:, 0]
        with np.errstate(all="ignore"):
            u = np.einsum("ij,ij->i", tv, pv) / det
            v = np.einsum("ij,ij->i", d, np.cross(tv, e0)) / det
        np.testing.assert_allclose(got[hit, 1], u[hit], rtol=0, atol=2e-5)
        np.testing.assert_allclose(got[hit, 2], v[hit], rtol=0, atol=2e-5)
    finally:
        _fresh(r, sc)


# ---- (g) non-interference ----------------------------------------------------------------------------------------------
def test_g_film_and_aovs_are_untouched_and_sequences_repeat(cb, pkg):
    r, sc = cb
    try:
        _fresh(r, sc)

        def sequence():
            outs = []
            for j in range(3):
                _frame(r, j, aov_spp=2)
                outs.append(r.denoise_temporal())
            return outs
        first = sequence()
        mean0, m20 = r.download_film()
        aov0, surf0 = r.download_aovs(), r.download_aov_surface()
        r.denoise_temporal()
        mean1, m21 = r.download_film()
        assert np.array_equal(mean0.view(np.uint32), mean1.view(np.uint32)) and np.array_equal(m20.view(np.uint32), m21.view(np.uint32))
        for x, y in zip(aov0 + (surf0,), r.download_aovs() + (r.download_aov_surface(),)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        r.temporal_reset()
        assert r.temporal_info()["frames"] == 0
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*no history"):
            r.download_history()
        again = sequence()
        for x, y in zip(first, again):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert r.temporal_info()["history_bytes"] >= RES * RES * (4 * 16 + 2 * 4) + 26 * 36
    finally:
        _fresh(r, sc)


def test_g_a_context_without_temporal_calls_has_no_history(pkg):
    sc = pkg.host_scene.cornell_box(32, 32)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(3)
        r.render(4)
        r.render_aovs(2)
        r.denoise()
        r.update_vertices(sc.xs, sc.ys, sc.zs)
        info = r.temporal_info()
        assert info == dict(frames=0, reprojected=0, reset=0, temporal_ms=0.0, history_bytes=0)
        r.denoise_temporal()
        assert r.temporal_info()["history_bytes"] > 0


def test_g_refusals(cb, pkg):
    r, sc = cb
    try:
        _fresh(r, sc)
        film = _frame(r, 0)
        for t in ({"alpha": -0.1}, {"alpha": 1.5}, {"alpha": float("nan")}, {"normal_threshold": float("inf")},
                  {"plane_threshold": 0.0}, {"plane_threshold": -1.0}, {"plane_threshold": float("nan")}):
            with pytest.raises(pkg.DmtError, match=r"failed \(1\)"):
                r.denoise_temporal(temporal=t)
        with pytest.raises(pkg.DmtError, match=r"failed \(1\)"):
            r.denoise_temporal({"iterations": 11})
        r.denoise_temporal()
        before = r.download_history()
        bad = film[1].copy()
        bad[7, 9, 3] = 1
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*fewer than 2 samples"):
            r.denoise_temporal(film=(film[0], bad))
        after = r.download_history()  # a refused call leaves the history as it was
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
        assert r.temporal_info()["frames"] == 1
        a, n, x = r.download_aovs()
        r.upload_aovs(a, n, x)  # drops the surface plane
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*surface plane"):
            r.denoise_temporal()
        with pytest.raises(pkg.DmtError, match=r"failed \(3\)"):
            r.download_aov_surface()
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*size"):
            r.upload_aov_surface(np.zeros((RES + 1, RES, 4), F))
        r.denoise()  # the spatial filter needs no surface plane
        # a new soup and a new resolution reset the history
        r.render_aovs(1)
        r.denoise_temporal()
        assert r.temporal_info()["frames"] == 2
        r.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
        r.upload_scene(sc)
        _frame(r, 1)
        r.denoise_temporal()
        info = r.temporal_info()
        assert info["frames"] == 1 and info["reprojected"] == 0
        small = pkg.host_scene.cornell_box(32, 32)
        r.set_camera(small.camera)
        # at once, not at the next temporal call: the old resolution's history is no longer there to download
        assert r.temporal_info()["frames"] == 0
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*no history"):
            r.download_history()
        _frame(r, 2)
        r.denoise_temporal()
        info = r.temporal_info()
        assert info["frames"] == 1 and info["reprojected"] == 0
        assert r.download_history()[1].shape == (32, 32)
    finally:
        _fresh(r, sc)


# ---- (h) quality -------------------------------------------------------------------------------------------------------
def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean(axis=-1)).mean())


def quality_scene(pkg, name):
    hs = pkg.host_scene
    if name == "cornell":
        return hs.cornell_box(256, 256), 8, False
    return hs.load_json(GOLDEN / "c3" / "c3_sphere_veranda.json"), 12, True


def quality_run(pkg, name, temporal=None, frames=8, spp=4, aov_spp=4):
    """(reference, dmt_denoise of the last frame alone, dmt_denoise_temporal at the last frame)"""
    sc, depth, bvh = quality_scene(pkg, name)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(depth)
        if bvh:
            r.set_accel(1)
        r.film_clear()
        r.render(4096, sample_offset=64)  # independent of the frames' samples 0 .. 31
        ref, _ = r.download_film()
        for j in range(frames):
            _frame(r, j, spp, aov_spp)
            tem = r.denoise_temporal(temporal=temporal)
        alone = r.denoise()
    return ref, alone, tem


@pytest.mark.parametrize("name", sorted(QUALITY))
def test_h_quality(pkg, name):
    ref, alone, tem = quality_run(pkg, name)
    e0, e1 = _rmse(alone, ref), _rmse(tem, ref)
    bright = tem[..., :3].mean() / ref[..., :3].mean() - 1
    print(f"{name}: RMSE dmt_denoise of frame 8 {e0:.5f}, temporal {e1:.5f}, ratio {e0 / e1:.3f}, brightness {100 * bright:+.3f} %")
    assert e0 / e1 > 1
    assert e1 * QUALITY[name] <= e0, (e0, e1, e0 / e1)
    assert abs(bright) < 0.01
