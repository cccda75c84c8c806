"""Thin-lens camera on the GPU (dmt_set_lens): the device code against its host twin, the lens-free film
against the film of a context that never heard of a lens, every render path against the single-sample probe, the sampler
table's third plane, adaptive sampling, the circle of confusion in the feature pass, and autofocus."""
import ctypes as C

import numpy as np
import pytest

import lens_ref as LR

pytestmark = pytest.mark.gpu

R, D = LR.LENS_R, LR.LENS_D
OFF, FORCE = 0, 2


@pytest.fixture(scope="module")
def cams(O):
    a = O.cornell_box(64, 64).camera.copy()
    b = np.zeros(11, np.float32)
    b[0:3], b[3:6], b[9], b[10] = (0.3, 1.0, -0.2), (1.5, -2.0, 0.75), 28.0, 36.0
    b.view(np.int32)[6:9] = (48, 32, 1)
    return a, b.view(np.uint8).copy()


@pytest.fixture(scope="module")
def e_host(pkg, cams):
    return LR.measure_e_host(pkg, cams)


@pytest.fixture()
def ctx(pkg):
    """a context of the test's own: the lens is context state, and no other module's tests may inherit one"""
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


# ---- 7. device against host twin ---------------------------------------------------------------------
def test_device_against_host_twin(ctx, pkg, cams, e_host):
    print(f"e_host = {e_host:.3e}")
    for (w, h), cam in zip(LR.FRAMES, cams):
        px, py, s = LR.cases(w, h)
        ctx.set_camera(cam)
        ctx.set_lens(R, D)
        assert ctx.lens_info() == (np.float32(R), np.float32(D))
        _, _, u_host = pkg.lens_rays(cam, R, D, px, py, s)
        assert ctx.test_lens_values(px, py, s).tobytes() == u_host.tobytes()
        o, d = ctx.test_camera_rays(px, py, s)
        o64, d64, _, _ = LR.rays64(cam, R, D, px, py, s)
        dev_d, dev_o = np.abs(d - d64).max(), np.abs(o - o64).max() / LR.origin_scale(cam, R)
        print(f"{w}x{h}: device - float64: direction {dev_d:.3e}, origin {dev_o:.3e} (bound {4 * e_host:.3e})")
        assert dev_d <= 4 * e_host and dev_o <= 4 * e_host
        # the lens survives set_camera; radius 0 gives the pinhole rays again
        ctx.set_camera(cam)
        assert ctx.lens_info() == (np.float32(R), np.float32(D))
        ctx.set_lens(0.0, 1.0)
        o0, d0 = ctx.test_camera_rays(px, py, s)
        o64, d64, _, _ = LR.rays64(cam, 0.0, 1.0, px, py, s)
        assert np.abs(d0 - d64).max() <= 4 * e_host and np.abs(o0 - o64).max() == 0


def test_set_lens_arguments(ctx):
    nan, inf = float("nan"), float("inf")
    lib = ctx._lib
    for r, d in ((-1.0, 1.0), (nan, 1.0), (inf, 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, nan), (0.1, inf)):
        assert lib.dmt_set_lens(ctx._ctx, C.c_float(r), C.c_float(d)) == 1  # DMT_ERR_INVALID
    assert ctx.lens_info() == (0.0, 1.0)  # the default, untouched by refused calls
    ctx.set_lens(0.25, 3.0)
    for d in (0.0, -1.0, nan, inf):  # radius 0: the distance is ignored
        ctx.set_lens(0.0, d)
    assert ctx.lens_info() == (0.0, 3.0)


# ---- 8. the lens-free film is unchanged ----------------------------------------------------------------
def test_lens_free_film_is_unchanged(ctx, pkg, O):
    sc = O.cornell_box(64, 64)
    with pkg.Renderer(0) as plain:  # never sees dmt_set_lens
        plain.upload_scene(sc)
        plain.set_limits(8)
        want = _film(plain, 16)
    ctx.upload_scene(sc)
    ctx.set_limits(8)
    ctx.set_lens(0.0, 1.0)
    assert _same(_film(ctx, 16), want)
    ctx.set_lens(R, D)
    blurred = _film(ctx, 16)
    assert not _same(blurred, want) and np.isfinite(blurred[0]).all()
    ctx.set_lens(0.0, 7.0)
    assert _same(_film(ctx, 16), want)


# ---- 9. every path prepares the same rays ----------------------------------------------------------
def test_every_path_prepares_the_same_rays(ctx, O):
    """Per sample s, a 1-spp render at s into a cleared film holds the sample itself and must equal dmt_test_trace_samples
    (the pattern of test_trace_samples_run_the_render_kernel); the 8-spp film must equal the in-order fold of those samples,
    which the library's one welford_update performs when the same eight are rendered by successive 1-spp calls (its
    v_rcp_f32 has no host restatement).  Brute force, BVH megakernel and the wavefront form must agree bit for bit."""
    w = h = 16
    spp = 8
    ctx.upload_scene(O.cornell_box(w, h))
    ctx.set_limits(6)
    ctx.set_lens(R, D)
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.reshape(-1).astype(np.int32), yy.reshape(-1).astype(np.int32)
    films = {}
    for name, accel, strategy in (("brute", 0, 0), ("bvh", 1, 1), ("wavefront", 1, 2)):
        ctx.set_accel(accel)
        ctx.set_bvh_strategy(strategy)
        if name != "wavefront":
            for s in range(spp):
                mean, m2 = _film(ctx, 1, offset=s)
                L = ctx.test_trace_samples(px, py, np.full(px.size, s, np.int32))
                assert np.isfinite(L).all() and L.max() > 0
                assert L.tobytes() == mean[py, px, :3].tobytes(), (name, s, np.abs(L - mean[py, px, :3]).max())
                assert (m2[..., 3] == 1).all()
            ctx.film_clear()
            for s in range(spp):
                ctx.render(1, sample_offset=s)
            ctx.sync()
            folded = ctx.download_film()
        films[name] = _film(ctx, spp)
        if name != "wavefront":
            assert _same(films[name], folded), name
    ctx.set_accel(0)
    ctx.set_bvh_strategy(0)
    assert _same(films["bvh"], films["brute"])
    assert _same(films["wavefront"], films["bvh"])
    ctx.set_lens(0.0, 1.0)
    assert not _same(_film(ctx, spp), films["brute"])  # the lens did change the rays


# ---- 10. sampler table ---------------------------------------------------------------------------------
def test_sampler_table_with_a_lens(ctx, O):
    """160 x 136 is more than one Halton period each way.  One call of 8 samples from sample 3: computed against tabulated,
    then with 4-sample chunks and a budget of 1.5 chunks at 48 bytes per entry, which makes two slices."""
    w, h, spp, off = 160, 136, 8, 3
    ctx.upload_scene(O.cornell_box(w, h))
    ctx.set_limits(4)
    ctx.set_lens(R, D)
    ctx.set_sampler_table(OFF)
    want = _film(ctx, spp, offset=off)
    ctx.set_sampler_table(FORCE)
    assert _same(_film(ctx, spp, offset=off), want)
    ctx.set_chunk(4)
    ctx.set_sampler_table(FORCE, int(1.5 * 4 * 128 * 128 * 48))
    assert _same(_film(ctx, spp, offset=off), want)
    ctx.set_sampler_table(OFF)
    assert _same(_film(ctx, spp, offset=off), want)  # 4-sample chunks, computed
    # and the table did carry lens rays: the pinhole film differs
    ctx.set_lens(0.0, 1.0)
    ctx.set_sampler_table(FORCE)
    assert not _same(_film(ctx, spp, offset=off), want)


# ---- 11. adaptive sampling -----------------------------------------------------------------------------
def test_adaptive_with_a_lens(ctx, O):
    res, step, max_spp, min_spp = 32, 8, 32, 8
    ctx.upload_scene(O.cornell_box(res, res))
    ctx.set_limits(5)
    ctx.set_lens(R, D)
    ctx.film_clear()
    copies = [(np.zeros((res, res, 4), np.float32), np.zeros((res, res, 4), np.float32))]
    for k in range(max_spp // step):
        ctx.render(step, sample_offset=k * step)
        copies.append(ctx.download_film())
    mean16, m216 = copies[2]
    n = m216[..., 3].astype(np.float64)
    err = np.sqrt(m216[..., :3].astype(np.float64).sum(-1) / (n * (n - 1))) / np.maximum(mean16[..., :3].astype(np.float64).sum(-1), 1e-3)
    thr = float(np.median(err))
    ctx.film_clear()
    ctx.render_adaptive(thr, max_spp, step, min_spp=min_spp)
    ctx.sync()
    mean, m2 = ctx.download_film()
    cnt = m2[..., 3]
    assert (np.mod(cnt, step) == 0).all() and cnt.min() >= min_spp
    stopped = cnt < max_spp
    assert 0.1 < stopped.mean() < 0.95, stopped.mean()
    k = (cnt / step).astype(np.int64)
    yy, xx = np.mgrid[0:res, 0:res]
    ref_mean, ref_m2 = np.stack([c[0] for c in copies])[k, yy, xx], np.stack([c[1] for c in copies])[k, yy, xx]
    assert mean.tobytes() == ref_mean.tobytes() and m2.tobytes() == ref_m2.tobytes()


# ---- 12. circle of confusion -----------------------------------------------------------------------
THETA = 36.0 / (20.0 * 64)  # sensor_size / (focal_length * height): one pixel's angle (csrc/denoise.hpp)


def _quad_scene(pkg, depth, half, edge):
    """one matte quad facing a camera at the origin that looks down +y: x in [edge, half], z in [-half, half] at y = depth"""
    H = pkg.host_scene
    L = H.load_host_library()
    q = np.array([[edge, depth, -half], [half, depth, -half], [half, depth, half], [edge, depth, half]], np.float32)
    T = np.array([(q[0], q[1], q[2]), (q[0], q[2], q[3])], np.float32)
    xs, ys, zs = (np.concatenate([T[:, :, k], np.zeros((2, 1), np.float32)], 1) for k in range(3))
    rec = np.zeros(32, np.uint8)
    L.dmt_host_make_oren_nayar(np.array([0.7, 0.7, 0.7], np.float32).ctypes.data_as(C.c_void_p), C.c_float(0.5), rec.ctypes.data_as(C.c_void_p))
    cam = np.zeros(11, np.float32)
    cam[0:3], cam[9], cam[10] = (0, 1, 0), 20.0, 36.0
    cam.view(np.int32)[6:9] = (64, 64, 1)
    none = np.zeros((0, 32), np.uint8)
    return H.ArrayScene(xs, ys, zs, np.zeros(2, np.uint32), rec[None], none, none, cam.view(np.uint8))


def _aovs(r, spp=64):
    r.render_aovs(spp)
    r.sync()
    albedo, _, position = r.download_aovs()
    return albedo[..., 3].copy(), position[..., :3].copy()


def test_quad_in_focus_is_sharp(ctx, pkg, e_host):
    """The quad lies in the plane of focus: every lens ray of a film position meets it where the pinhole ray does."""
    depth = 4.0
    ctx.upload_scene(_quad_scene(pkg, depth, 4.5, 0.37 * THETA * depth))  # the edge crosses a pixel column off its borders
    cov0, pos0 = _aovs(ctx)
    partial = np.nonzero(((cov0 > 0) & (cov0 < 1)).any(0))[0]
    assert partial.size == 1, partial  # the one column the edge crosses
    keep = np.ones(64, bool)
    keep[partial[0]] = False
    assert set(np.unique(cov0[:, keep])) == {0.0, 1.0}
    ctx.set_lens(0.3, depth)
    cov, pos = _aovs(ctx)
    assert cov[:, keep].tobytes() == cov0[:, keep].tobytes()
    hit = (cov0 == 1) & keep[None, :]
    dev = np.abs(pos[hit] - pos0[hit]).max()
    print(f"in focus: position differs by {dev:.3e} (bound {8 * e_host * depth:.3e})")
    assert dev <= 8 * e_host * depth


def test_quad_out_of_focus_blurs_by_the_circle_of_confusion(ctx, pkg):
    focus, z = 4.0, 8.0
    radius = 12 * THETA * z * focus / (2 * abs(z - focus))  # predicted blur diameter: 12 pixel columns
    predicted = 2 * radius * abs(z - focus) / (z * focus * THETA)
    assert abs(predicted - 12) < 1e-9
    ctx.upload_scene(_quad_scene(pkg, z, 12.0, 0.37 * THETA * z))
    cov0, _ = _aovs(ctx)
    assert int(((cov0.mean(0) > 0) & (cov0.mean(0) < 1)).sum()) == 1
    ctx.set_lens(radius, focus)
    cov, _ = _aovs(ctx)
    col = cov.mean(0)  # coverage of a pixel column: 64 rows x 64 samples
    blurred = int(((col > 0) & (col < 1)).sum())
    print(f"out of focus: {blurred} partially covered columns, predicted {predicted:.2f}")
    assert abs(blurred - predicted) <= 2
    assert col.min() == 0 and col.max() == 1  # sharp again away from the edge


# ---- 13. autofocus ---------------------------------------------------------------------------------
def test_autofocus(ctx, pkg, O):
    sc = O.cornell_box(64, 64)
    ctx.upload_scene(sc)
    xf = LR.camera_xf(sc.camera)
    fwd = xf["fwd"].astype(np.float64)
    fx, fy = 20.5, 20.5  # a pixel centre over the back wall (the plane y = 4, left of and above the boxes)
    for accel in (0, 1):
        ctx.set_accel(accel)
        dist = ctx.focus_distance_at(fx, fy)
        o64, d64, _ = LR.lens_ray64(xf, np.float32(fx), np.float32(fy), 0.0, 1.0, (0.0, 0.0))
        tri, t = ctx.test_closest_hit(o64.astype(np.float32)[None], d64.astype(np.float32)[None])
        assert tri[0] >= 0 and abs(dist - 4.0) < 1e-4  # the back wall's depth
        want = float(t[0]) * float(d64 @ fwd)
        # the two rays differ by a rounding per direction component, the hit distances by a few more
        assert abs(dist - want) <= 32 * 2.0 ** -23 * want, (dist, want)
        hit = o64 + float(t[0]) * d64
        xy, depth = pkg.camera_project(sc.camera, hit[None])
        assert abs(xy[0, 0] - fx) <= 1e-3 and abs(xy[0, 1] - fy) <= 1e-3, xy  # 2^-20 of the point is 3e-5 pixels here
        assert abs(depth[0] - dist) <= 32 * 2.0 ** -23 * want
    ctx.set_accel(0)
    # a ray into the void: left of the quad of the circle-of-confusion scenes
    ctx.upload_scene(_quad_scene(pkg, 4.0, 4.5, 0.0))
    d = C.c_float(-1)
    miss_x, hit_x = 8.5, 56.5  # the quad covers x >= 0, the right half of the frame
    assert ctx._lib.dmt_focus_distance_at(ctx._ctx, C.c_float(miss_x), C.c_float(32.5), C.byref(d)) == 3  # DMT_ERR_STATE
    assert ctx.focus_distance_at(hit_x, 32.5) == pytest.approx(4.0, rel=1e-6)
    with pytest.raises(pkg.DmtError, match="leaves the scene"):
        ctx.focus_distance_at(miss_x, 32.5)
