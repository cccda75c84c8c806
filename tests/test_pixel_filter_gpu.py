"""Pixel reconstruction filters on the GPU (dmt_set_pixel_filter): the device's film positions against the
host twin, the default against a context that never heard of a filter, every render path against the single-sample probe,
the sampler table's warped jitter plane, adaptive sampling, the filter's CDF read off a step edge in the feature pass, a flat
field, and a motion row."""
import ctypes as C

import numpy as np
import pytest

import lens_ref as LR
import motion_ref as MR
import pixel_filter_ref as PF

pytestmark = pytest.mark.gpu

GAUSS = PF.GAUSS  # (kind, 1.5, 0.5)
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
    """a context of the test's own: the filter is context state, and no other module's tests may inherit one"""
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


# ---- 5. the probe ----------------------------------------------------------------------------------
def test_film_positions_equal_the_host_twin(ctx, pkg, cams, e_host):
    print(f"e_host = {e_host:.3e}")
    for (w, h), cam in zip(LR.FRAMES, cams):
        px, py, s = LR.cases(w, h, n=128)
        ctx.set_camera(cam)
        for name, (kind, radius, param) in sorted(PF.FILTERS.items()) + [("default", (PF.BOX, 0.5, 0.0))]:
            ctx.set_pixel_filter(kind, radius, param)
            info = ctx.pixel_filter_info()
            assert (info["kind"], info["radius"], info["active"]) == (kind, np.float32(radius), name != "default")
            got = ctx.test_film_positions(px, py, s)
            want = pkg.pixel_filter_positions(w, h, kind, radius, param, px, py, s)
            assert got.tobytes() == want.tobytes(), (name, np.abs(got - want).max())
        # the camera rays go through those positions: float64 rays fed the host twin's positions, pinhole and lens
        ctx.set_pixel_filter(*GAUSS)
        ctx.set_camera(cam)  # the filter survives set_camera
        assert ctx.pixel_filter_info()["active"]
        pos = pkg.pixel_filter_positions(w, h, *GAUSS, px, py, s)
        xf, p = LR.camera_xf(cam), LR.halton_params(w, h)
        for lens_r, lens_d in ((0.0, 1.0), (R, D)):
            ctx.set_lens(lens_r, lens_d)
            o, d = ctx.test_camera_rays(px, py, s)
            o64, d64 = np.zeros((len(px), 3)), np.zeros((len(px), 3))
            for i in range(len(px)):
                u = LR.lens_values(LR.halton_index(p, int(px[i]), int(py[i]), int(s[i]))) if lens_r > 0 else (0.0, 0.0)
                o64[i], d64[i], _ = LR.lens_ray64(xf, pos[i, 0], pos[i, 1], lens_r, lens_d, u)
            dev_d, dev_o = np.abs(d - d64).max(), np.abs(o - o64).max()
            if lens_r > 0:
                dev_o /= LR.origin_scale(cam, lens_r)
            print(f"{w}x{h} lens {lens_r}: device - float64: direction {dev_d:.3e}, origin {dev_o:.3e} (bound {4 * e_host:.3e})")
            assert dev_d <= 4 * e_host and (dev_o <= 4 * e_host if lens_r > 0 else dev_o == 0)  # a pinhole's origin is the camera position


def test_set_pixel_filter_arguments(ctx):
    nan, inf = float("nan"), float("inf")
    lib = ctx._lib
    default = dict(kind=PF.BOX, radius=0.5, param=0.0, active=False)
    assert ctx.pixel_filter_info() == default
    refused = [(PF.TENT, r, 0.0) for r in (0.0, -1.0, 8.5, nan, inf)] + [(PF.GAUSSIAN, 1.5, s) for s in (0.0, -0.5, nan, inf)]
    refused += [(-1, 1.0, 0.0), (4, 1.0, 0.0)]
    for kind, radius, param in refused:
        assert lib.dmt_set_pixel_filter(ctx._ctx, kind, C.c_float(radius), C.c_float(param)) == 1  # DMT_ERR_INVALID
    assert ctx.pixel_filter_info() == default  # untouched by refused calls
    ctx.set_pixel_filter("gaussian", 1.5, 0.5)
    for kind, radius, param in refused:
        assert lib.dmt_set_pixel_filter(ctx._ctx, kind, C.c_float(radius), C.c_float(param)) == 1
    assert ctx.pixel_filter_info() == dict(kind=PF.GAUSSIAN, radius=1.5, param=0.5, active=True)
    ctx.set_pixel_filter(PF.BOX, 1.0)
    assert ctx.pixel_filter_info() == dict(kind=PF.BOX, radius=1.0, param=0.0, active=True)  # a wider box is a filter


# ---- 6. the default is unchanged -----------------------------------------------------------------------
def test_default_film_is_unchanged(ctx, pkg, O):
    sc = O.cornell_box(64, 64)
    with pkg.Renderer(0) as plain:  # never sees dmt_set_pixel_filter
        plain.upload_scene(sc)
        plain.set_limits(8)
        want = _film(plain, 16)
    ctx.upload_scene(sc)
    ctx.set_limits(8)
    ctx.set_pixel_filter(PF.BOX, 0.5)
    assert _same(_film(ctx, 16), want)
    ctx.set_pixel_filter(*GAUSS)
    ctx.upload_scene(sc)  # the filter survives an upload
    assert ctx.pixel_filter_info()["active"]
    soft = _film(ctx, 16)
    assert not _same(soft, want) and np.isfinite(soft[0]).all() and np.isfinite(soft[1]).all()
    ctx.set_pixel_filter(PF.BOX, 0.5)
    assert _same(_film(ctx, 16), want)


# ---- 7. every path prepares the same rays ----------------------------------------------------------
def test_every_path_prepares_the_same_rays(ctx, O):
    """The pattern of the lens test of this name, under Gaussian 1.5 / 0.5: per sample s a 1-spp render at s equals
    dmt_test_trace_samples, the 8-spp film equals the in-order fold of successive 1-spp calls, and brute force, the BVH
    megakernel and the wavefront form agree bit for bit."""
    w = h = 16
    spp = 8
    ctx.upload_scene(O.cornell_box(w, h))
    ctx.set_limits(6)
    ctx.set_pixel_filter(*GAUSS)
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
    ctx.set_pixel_filter(PF.BOX, 0.5)
    assert not _same(_film(ctx, spp), films["brute"])  # the filter did change the rays


# ---- 8. sampler table ----------------------------------------------------------------------------------
def test_sampler_table_with_a_filter(ctx, pkg, O):
    """160 x 136 is more than one Halton period each way.  One call of 8 samples from sample 3: computed against tabulated,
    then with 4-sample chunks and a budget of 1.5 chunks, which makes two slices; 40 bytes per entry, 48 with a lens."""
    w, h, spp, off = 160, 136, 8, 3
    ctx.upload_scene(O.cornell_box(w, h))
    ctx.set_limits(4)
    films = []
    for lens, entry in ((None, 40), ((R, D), 48)):
        ctx.set_pixel_filter(*GAUSS)
        if lens:
            ctx.set_lens(*lens)
        ctx.set_chunk(0)
        ctx.set_sampler_table(OFF)
        want = _film(ctx, spp, offset=off)
        ctx.set_sampler_table(FORCE)
        assert _same(_film(ctx, spp, offset=off), want)
        ctx.set_chunk(4)
        ctx.set_sampler_table(FORCE, int(1.5 * 4 * 128 * 128 * entry))
        assert _same(_film(ctx, spp, offset=off), want)
        ctx.set_sampler_table(OFF)
        assert _same(_film(ctx, spp, offset=off), want)  # 4-sample chunks, computed
        films.append(want)
    # the table's jitter plane is the warped jitter
    ctx.set_lens(0.0, 1.0)
    _, jit = ctx.test_sampler_table(w, h, off, 2)
    yy, xx = np.mgrid[0:128, 0:128]
    pxs, pys = xx.reshape(-1).astype(np.int32), yy.reshape(-1).astype(np.int32)
    pos = pkg.pixel_filter_positions(w, h, *GAUSS, pxs, pys, np.full(pxs.size, off + 1, np.int32))
    formed = (jit[1].reshape(-1, 2) - np.float32(0.5) + np.float32(0.5)) + np.stack([pxs, pys], 1).astype(np.float32)
    assert formed.astype(np.float32).tobytes() == pos.tobytes()
    # and the table did carry the filter: the box film differs from both
    ctx.set_pixel_filter(PF.BOX, 0.5)
    ctx.set_sampler_table(FORCE)
    box = _film(ctx, spp, offset=off)
    assert not _same(box, films[0]) and not _same(box, films[1]) and not _same(films[0], films[1])


# ---- 9. adaptive sampling ------------------------------------------------------------------------------
def test_adaptive_with_a_filter(ctx, O):
    res, step, max_spp, min_spp = 32, 8, 32, 8
    ctx.upload_scene(O.cornell_box(res, res))
    ctx.set_limits(5)
    ctx.set_pixel_filter(*GAUSS)
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


# ---- 10. step edge: the filter's CDF in the film ---------------------------------------------------
THETA = 36.0 / (20.0 * 64)  # sensor_size / (focal_length * height): one pixel's angle (csrc/denoise.hpp)


def _quad_scene(pkg, depth, half, edge):
    """one matte quad facing a camera at the origin that looks down +y: x in [edge, half], z in [-half, half] at y = depth
    (the geometry of the lens tests' scene of this name)"""
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


def test_step_edge_shows_the_filters_cdf(ctx, pkg):
    """The coverage the feature pass reports for a pixel next to a straight vertical edge is the share of the pixel's film
    positions beyond the edge, i.e. the filter's CDF sampled by the pixel's own samples.  A position within 1e-4 px of the
    edge may fall either way (one fp32 ulp at raster coordinate 64 is 7.6e-6, and the ray set-up and hit test add a handful
    of roundings): the pixel gets one sample of allowance for each, and at most 5 % of the pixels may need any."""
    depth, spp, cols = 4.0, 64, np.arange(29, 36)
    kind, radius, sigma = GAUSS
    edge = np.float32(0.37 * THETA * depth)
    sc = _quad_scene(pkg, depth, 4.5, edge)
    ctx.upload_scene(sc)
    ctx.set_pixel_filter(kind, radius, sigma)
    ctx.render_aovs(spp)
    ctx.sync()
    albedo, _, _ = ctx.download_aovs()
    cov = albedo[..., 3]
    xy, _ = pkg.camera_project(sc.camera, np.array([[edge, depth, 0.0]], np.float32))
    edge_x = float(xy[0, 0])
    assert cols[0] + radius + 1 < edge_x < cols[-1] - radius, edge_x  # the columns of the test hold the whole transition
    yy, xx = np.meshgrid(np.arange(64), cols, indexing="ij")
    pxs, pys = np.repeat(xx.reshape(-1), spp).astype(np.int32), np.repeat(yy.reshape(-1), spp).astype(np.int32)
    ss = np.tile(np.arange(spp), xx.size).astype(np.int32)
    fx = pkg.pixel_filter_positions(64, 64, kind, radius, sigma, pxs, pys, ss)[:, 0].astype(np.float64).reshape(64, cols.size, spp)
    beyond = (fx > edge_x).sum(-1)
    allowance = (np.abs(fx - edge_x) <= 1e-4).sum(-1)
    got = cov[:, cols].astype(np.float64) * spp
    print(f"edge at raster x {edge_x:.5f}; pixels with an allowance: {int((allowance > 0).sum())} of {allowance.size}; "
          f"largest |coverage - share| in samples: {np.abs(got - beyond).max():.3f}")
    assert (allowance > 0).mean() <= 0.05
    assert (np.abs(got - beyond) <= allowance).all(), np.argwhere(np.abs(got - beyond) > allowance)[:8]
    partial = ((beyond > 0) & (beyond < spp)).any(0)
    assert partial.sum() >= 3  # the Gaussian does spread the edge over several columns
    # columns farther than radius + 1 from the edge are exactly 0 or 1
    centres = np.arange(64) + 0.5
    assert (cov[:, centres < edge_x - (radius + 1)] == 0).all() and (cov[:, centres > edge_x + (radius + 1)] == 1).all()


# ---- 11. flat field ------------------------------------------------------------------------------------
def test_flat_field_is_exact(ctx, O):
    """A constant environment and no geometry: every sample returns the light's radiance whatever its film position, and
    every weight is 1, so every pixel holds that radiance exactly."""
    sc = O.cornell_box(16, 16)
    ctx.upload_scene(sc)
    e = np.zeros((0, 4), np.float32)
    ctx.upload_triangles(e, e, e, np.zeros(0, np.uint32))
    ctx.set_pixel_filter(PF.TENT, 2.0)
    mean, m2 = _film(ctx, 16)
    env = np.float16(0.1).astype(np.float32)  # the Cornell scene's constant environment, a half in its record
    assert (mean[..., :3] == env).all() and (m2[..., 3] == 16).all() and (m2[..., :3] == 0).all()


# ---- 12. a motion row: no table, through the tail ------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_motion_row_traces_the_filtered_positions(ctx, O, accel):
    res, s = 32, 5
    sc = O.cornell_box(res, res)
    _, k1 = MR.cornell_keys(sc, offsets=((0.9, 0.3, 0.8), (-0.8, -0.4, 0.9)))
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_accel(accel)
    ctx.set_motion(*k1)
    plain = _film(ctx, 1, offset=s)
    ctx.set_pixel_filter(*GAUSS)
    mean, m2 = _film(ctx, 1, offset=s)
    idx = np.random.default_rng(3).choice(res * res, 64, replace=False)
    px, py = (idx % res).astype(np.int32), (idx // res).astype(np.int32)
    L = ctx.test_trace_samples(px, py, np.full(64, s, np.int32))
    assert (m2[py, px, 3] == 1).all() and np.isfinite(L).all() and L.max() > 0
    assert L.tobytes() == mean[py, px, :3].tobytes(), np.abs(L - mean[py, px, :3]).max()
    assert not _same((mean, m2), plain)
    ctx.set_accel(0)
