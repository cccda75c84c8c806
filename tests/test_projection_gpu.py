"""Camera projections on the GPU (dmt_set_projection): the device code against the float64 restatement within
a multiple of the host twin's own error, perspective films untouched, every render path against the single-sample probe,
images that are the model's, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import lens_ref as LR
import projection_ref as PR

pytestmark = pytest.mark.gpu

OFF, AUTO, FORCE = 0, 1, 2
F = np.float32


@pytest.fixture(scope="module")
def cases(O):
    return PR.cases(O)


@pytest.fixture(scope="module")
def e_host(pkg, cases):
    return PR.measure_e_host(pkg, [c for c, _ in cases])


@pytest.fixture()
def ctx(pkg):
    """a context of the test's own: the projection is context state, and no other module's tests may inherit one"""
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


# ---- 6. device against the twin --------------------------------------------------------------------------
def test_device_against_host_twin(ctx, pkg, cases, e_host):
    """The device differs from the host twin in its reciprocal, its rsqrt and sincos_bounded, about 1 ulp each: at most
    4 x e_host from float64, the margin of test_lens_gpu.py::test_device_against_host_twin.  Once under the default filter
    (the sampler's own film positions), once under a tent of radius 2 (positions from dmt_test_film_positions, which leave
    the film at its borders)."""
    print(f"e_host = {e_host:.3e}")
    worst = 0.0
    for cam, _ in cases:
        w, h = LR.camera_xf(cam)["width"], LR.camera_xf(cam)["height"]
        px, py, s = LR.cases(w, h)
        ctx.set_camera(cam)
        for filt in (None, (pkg.FILTER_TENT, 2.0)):
            ctx.set_pixel_filter(*(filt or (pkg.FILTER_BOX, 0.5)))
            xy = ctx.test_film_positions(px, py, s)
            if filt is None:
                p = LR.halton_params(w, h)
                want = np.array([LR.film_position(p, int(x), int(y), LR.halton_index(p, int(x), int(y), int(k))) for x, y, k in zip(px, py, s)], F)
                assert xy.tobytes() == want.tobytes()
            for kind, param in PR.MODELS:
                ctx.set_projection(kind, param)
                assert ctx.projection_info() == {"kind": kind, "param": F(param)}
                o, d = ctx.test_camera_rays(px, py, s)
                o64, d64 = PR.rays64(cam, kind, param, xy)
                dev_d, dev_o = np.abs(d - d64).max(), np.abs(o - o64).max() / PR.origin_scale(cam)
                worst = max(worst, dev_d, dev_o)
                print(f"{w}x{h} filter {filt} kind {kind} ({param}): device - float64: direction {dev_d:.3e}, origin {dev_o:.3e} (bound {4 * e_host:.3e})")
                assert dev_d <= 4 * e_host and dev_o <= 4 * e_host
            ctx.set_projection("perspective")
    print(f"device - float64, largest: {worst:.3e}")


# ---- 7. perspective is untouched -------------------------------------------------------------------------
def test_perspective_is_untouched(ctx, pkg, O):
    sc = O.cornell_box(64, 64)
    with pkg.Renderer(0) as plain:  # never sees dmt_set_projection
        plain.upload_scene(sc)
        plain.set_limits(8)
        want = _film(plain, 16)
    ctx.upload_scene(sc)
    ctx.set_limits(8)
    ctx.set_projection(pkg.PROJECTION_PERSPECTIVE)
    assert _same(_film(ctx, 16), want)
    ctx.set_projection("orthographic", 2.0)
    ortho = _film(ctx, 16)
    assert not _same(ortho, want) and np.isfinite(ortho[0]).all() and ortho[0][..., :3].max() > 0
    # the projection survives dmt_set_camera and an upload
    ctx.set_camera(sc.camera)
    assert ctx.projection_info() == {"kind": 1, "param": 2.0}
    ctx.upload_scene(sc)
    assert ctx.projection_info() == {"kind": 1, "param": 2.0}
    assert _same(_film(ctx, 16), ortho)
    ctx.set_projection("perspective", 5.0)
    assert ctx.projection_info() == {"kind": 0, "param": 0.0}
    assert _same(_film(ctx, 16), want)


# ---- 8. every path prepares the same rays ------------------------------------------------------------------
@pytest.mark.parametrize("kind,param", [(PR.ORTHOGRAPHIC, 1.5), (PR.EQUIRECT, 0.0)])
def test_every_path_prepares_the_same_rays(ctx, O, kind, param):
    """The pattern of test_lens_gpu.py::test_every_path_prepares_the_same_rays: per sample, a 1-spp film equals
    dmt_test_trace_samples bit for bit; the 8-spp film equals the in-order fold; brute force, the BVH megakernel, the
    wavefront form, the sampler table off / on / forced and an adaptive render that masks nothing agree bit for bit.  One leg
    more under a medium and one under motion: rows that only consume the prepared ray."""
    w = h = 16
    spp = 8
    sc = O.cornell_box(w, h)
    ctx.upload_scene(sc)
    ctx.set_limits(6)
    ctx.set_projection(kind, param)
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.reshape(-1).astype(np.int32), yy.reshape(-1).astype(np.int32)
    # the probe's camera rays are the model's (and so, below, are the films')
    o, d = ctx.test_camera_rays(px, py, np.zeros(px.size, np.int32))
    p = LR.halton_params(w, h)
    xy = np.array([LR.film_position(p, int(x), int(y), LR.halton_index(p, int(x), int(y), 0)) for x, y in zip(px, py)], F)
    o64, d64 = PR.rays64(sc.camera, kind, param, xy)
    assert np.abs(d - d64).max() <= 1e-5 and np.abs(o - o64).max() <= 1e-5
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
            for mode in (OFF, FORCE, AUTO):
                ctx.set_sampler_table(mode)
                assert _same(_film(ctx, spp), films[name]), (name, mode)
    ctx.set_accel(0)
    ctx.set_bvh_strategy(0)
    assert _same(films["bvh"], films["brute"])
    assert _same(films["wavefront"], films["bvh"])
    ctx.film_clear()
    ctx.render_adaptive(0.0, spp, spp)  # threshold 0: no pixel stops early, one round of all samples
    ctx.sync()
    assert _same(ctx.download_film(), films["brute"])
    # a medium and motion: 1-spp films against the probe, computed against tabulated
    for leg in ("medium", "motion"):
        if leg == "medium":
            ctx.set_medium(0.4, albedo=(0.8, 0.8, 0.8), g=0.2, box_min=(-1.0, 0.5, -1.0), box_max=(1.0, 3.5, 1.0))
        else:
            ctx.clear_medium()
            ctx.set_motion(sc.xs + np.float32(0.05), sc.ys, sc.zs)
        ctx.set_sampler_table(OFF)
        mean, _ = _film(ctx, 1, offset=2)
        L = ctx.test_trace_samples(px, py, np.full(px.size, 2, np.int32))
        assert np.isfinite(L).all() and L.tobytes() == mean[py, px, :3].tobytes(), leg
        want = _film(ctx, spp)
        ctx.set_sampler_table(FORCE)
        assert _same(_film(ctx, spp), want), leg
        ctx.set_sampler_table(AUTO)
    ctx.set_projection("perspective")
    assert not _same(_film(ctx, spp), want)  # the projection did change the rays


# ---- 9. the image is the model's ---------------------------------------------------------------------------
def _quad_scene(pkg, depth, x0, x1, z0, z1, res=32):
    """one matte quad facing a level camera at the origin that looks down +y: [x0, x1] x [z0, z1] at y = depth"""
    H = pkg.host_scene
    L = H.load_host_library()
    q = np.array([[x0, depth, z0], [x1, depth, z0], [x1, depth, z1], [x0, depth, z1]], np.float32)
    T = np.array([(q[0], q[1], q[2]), (q[0], q[2], q[3])], np.float32)
    xs, ys, zs = (np.concatenate([T[:, :, k], np.zeros((2, 1), np.float32)], 1) for k in range(3))
    rec = np.zeros(32, np.uint8)
    L.dmt_host_make_oren_nayar(np.array([0.7, 0.7, 0.7], np.float32).ctypes.data_as(C.c_void_p), C.c_float(0.5), rec.ctypes.data_as(C.c_void_p))
    cam = np.zeros(11, np.float32)
    cam[0:3], cam[9], cam[10] = (0, 1, 0), 20.0, 36.0
    cam.view(np.int32)[6:9] = (res, res, 1)
    none = np.zeros((0, 32), np.uint8)
    return H.ArrayScene(xs, ys, zs, np.zeros(2, np.uint32), rec[None], none, none, cam.view(np.uint8))


def _coverage(r):
    r.render_aovs(64)
    r.sync()
    albedo, _, _ = r.download_aovs()
    return albedo[..., 3] > 0.5


def test_orthographic_image_is_a_parallel_projection(ctx, pkg):
    """A view of height 4 on a 32 x 32 film: a pixel is 1/8 scene unit.  The model goes through cameraFromRaster and keeps
    its half-pixel convention (film coordinate 0 maps to -sw / 2 + psx / 2): pixel column i spans x in
    [-2 + (i + 0.5) / 8, -2 + (i + 1.5) / 8] and row j spans z in [2 - (j + 1.5) / 8, 2 - (j + 0.5) / 8] (right is +x and up is
    +z for this camera).  The quad's edges lie a
    quarter pixel outside pixel boundaries, so the pixels it covers by more than half are exactly columns 10 .. 21 and rows
    6 .. 17, at depth 2 and at depth 5 alike; under the perspective camera the two depths give different rectangles."""
    px_size = 4.0 / 32
    x0, x1 = -2 + 10.5 * px_size - 0.25 * px_size, -2 + 22.5 * px_size + 0.25 * px_size
    z1, z0 = 2 - 6.5 * px_size + 0.25 * px_size, 2 - 18.5 * px_size - 0.25 * px_size
    want = np.zeros((32, 32), bool)
    want[6:18, 10:22] = True
    got = {}
    for depth in (2.0, 5.0):
        ctx.upload_scene(_quad_scene(pkg, depth, x0, x1, z0, z1))
        ctx.set_projection("orthographic", 4.0)
        got[depth] = _coverage(ctx)
        assert (got[depth] == want).all(), (depth, np.argwhere(got[depth] != want))
        ctx.set_projection("perspective")
        got[-depth] = _coverage(ctx)
    assert (got[-2.0] != got[-5.0]).any()


@pytest.mark.parametrize("kind,param", [(PR.EQUIRECT, 0.0), (PR.FISHEYE, 180.0)])
def test_angular_image_is_the_env_map_along_the_rays(ctx, pkg, kind, param):
    """An env map (16 x 8 texels) all around and one small triangle ahead.  path_shade adds the env map seen by a path ray
    at depth 0 UNWEIGHTED (st.L + st.beta * Le with beta = 1 and L = 0; the MIS weight applies from depth 1 on, as
    core-render.cpp:154-163 has it), so for every sample whose probe ray misses, the 1-spp film value is the device's own env
    evaluation of that ray's direction bit for bit.  At most 1 % of the samples may be left out as hits: a condition, sized
    by tests/test_projection.py::test_env_scene_triangle_share."""
    H = pkg.host_scene
    L = H.load_host_library()
    w, h = PR.ENV_FRAME
    T = PR.ENV_TRIANGLE[None]
    xs, ys, zs = (np.concatenate([T[:, :, k], np.zeros((1, 1), np.float32)], 1) for k in range(3))
    rec = np.zeros(32, np.uint8)
    L.dmt_host_make_oren_nayar(np.array([0.7, 0.7, 0.7], np.float32).ctypes.data_as(C.c_void_p), C.c_float(0.5), rec.ctypes.data_as(C.c_void_p))
    none = np.zeros((0, 32), np.uint8)
    ctx.upload_scene(H.ArrayScene(xs, ys, zs, np.zeros(1, np.uint32), rec[None], none, none, PR.env_scene_camera()))
    rng = np.random.default_rng(5)
    ctx.upload_envmap(rng.uniform(0.1, 2.0, (8, 16, 3)).astype(np.float32))
    ctx.set_limits(4)
    ctx.set_projection(kind, param)
    # a plain scene under an env map: the brute-force row (k_megakernel_env) is one of the two compiled without the
    # projection's tail and refuses; the BVH row renders
    _refused(ctx, pkg, lambda: ctx.render(1))
    _refused(ctx, pkg, lambda: ctx.test_trace_samples([0], [0], [0]))
    ctx.set_accel(1)
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.reshape(-1).astype(np.int32), yy.reshape(-1).astype(np.int32)
    o, d = ctx.test_camera_rays(px, py, np.zeros(px.size, np.int32))
    tri, _ = ctx.test_closest_hit(o, d)
    miss = tri < 0
    assert 1.0 - miss.mean() <= 0.01, 1.0 - miss.mean()
    Le = ctx.test_envmap(np.zeros((px.size, 2), np.float32), d)["Le_dir"]
    mean, m2 = _film(ctx, 1)
    film = mean[py, px, :3]
    assert (m2[..., 3] == 1).all() and Le[miss].min() > 0
    assert film[miss].tobytes() == Le[miss].tobytes(), np.abs(film[miss] - Le[miss]).max()
    # the film is not one colour: the fisheye's front hemisphere alone holds 64 of the map's 128 texels, of which the nearest-texel
    # lookups of 512 samples must see at least a quarter
    assert len(np.unique(film[miss], axis=0)) > 16


# ---- 10. refusals ------------------------------------------------------------------------------------------
def _refused(ctx, pkg, call):
    with pytest.raises(pkg.DmtError) as e:
        call()
    assert "dmt_set_projection" in str(e.value), str(e.value)
    return str(e.value)


def test_refusals(ctx, pkg, O):
    lib = ctx._lib
    sc = O.cornell_box(32, 32)
    ctx.upload_scene(sc)
    ctx.set_limits(4)
    nan, inf = float("nan"), float("inf")
    # bad arguments: DMT_ERR_INVALID, the state untouched
    ctx.set_projection("fisheye", 120.0)
    for kind, param in ((-1, 0.0), (4, 0.0), (1, 0.0), (1, -2.0), (1, nan), (1, inf), (3, 0.0), (3, 361.0), (3, nan)):
        assert lib.dmt_set_projection(ctx._ctx, kind, C.c_float(param)) == 1
        assert ctx.projection_info() == {"kind": 3, "param": 120.0}
    # a lens under the projection, and the projection under a lens: DMT_ERR_STATE both ways
    assert lib.dmt_set_lens(ctx._ctx, C.c_float(0.1), C.c_float(2.0)) == 3
    _refused(ctx, pkg, lambda: ctx.set_lens(0.1, 2.0))
    assert ctx.lens_info() == (0.0, 1.0) and ctx.projection_info() == {"kind": 3, "param": 120.0}
    ctx.set_lens(0.0, 2.0)  # radius 0 is the pinhole: accepted
    ctx.set_projection("perspective")
    ctx.set_lens(0.1, 2.0)
    assert lib.dmt_set_projection(ctx._ctx, 2, C.c_float(0)) == 3
    _refused(ctx, pkg, lambda: ctx.set_projection("equirect"))
    assert ctx.projection_info() == {"kind": 0, "param": 0.0} and ctx.lens_info() == (F(0.1), 2.0)
    ctx.set_lens(0.0, 1.0)
    # autofocus
    assert ctx.focus_distance_at(16.0, 16.0) > 0
    ctx.set_projection("orthographic", 2.0)
    _refused(ctx, pkg, lambda: ctx.focus_distance_at(16.0, 16.0))
    # the denoisers: refused, and the temporal history is what it was
    ctx.set_projection("perspective")
    _film(ctx, 8)
    ctx.render_aovs(4)
    ctx.denoise_temporal()
    before, hist = ctx.temporal_info(), ctx.download_history()
    ctx.set_projection("equirect")
    ctx.render_aovs(4)  # works: it traces the film's own rays
    ctx.sync()
    _refused(ctx, pkg, lambda: ctx.denoise())
    _refused(ctx, pkg, lambda: ctx.denoise_temporal())
    after, hist2 = ctx.temporal_info(), ctx.download_history()
    assert {k: before[k] for k in ("frames", "history_bytes")} == {k: after[k] for k in ("frames", "history_bytes")}
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hist, hist2))
    assert ctx.projection_info() == {"kind": 2, "param": 0.0}
    ctx.set_projection("perspective")
    ctx.render_aovs(4)
    ctx.denoise_temporal()
    assert ctx.temporal_info()["frames"] == before["frames"] + 1


def test_texture_filter_is_refused(ctx, pkg):
    """the first-hit texture filter's footprints are the pinhole's differentials: a render that would use it is refused"""
    scene = _textured_quad(pkg)
    ctx.upload_scene(scene)
    ctx.upload_textures(*scene.textures)
    ctx.set_texture_filter(pkg.TEXFILTER_REFERENCE)
    ctx.set_limits(3)
    want = _film(ctx, 2)  # perspective: renders
    ctx.set_projection("fisheye", 90.0)
    ctx.film_clear()
    _refused(ctx, pkg, lambda: ctx.render(2))
    _refused(ctx, pkg, lambda: ctx.test_trace_samples([0], [0], [0]))  # the probe shades with the same bodies
    assert ctx.projection_info() == {"kind": 3, "param": 90.0}
    ctx.set_texture_filter(pkg.TEXFILTER_LEVEL0)
    assert np.isfinite(_film(ctx, 2)[0]).all()  # level-0 lookups run under the projection
    ctx.set_projection("perspective")
    ctx.set_texture_filter(pkg.TEXFILTER_REFERENCE)
    assert _same(_film(ctx, 2), want)


def _textured_quad(pkg):
    """the quad of _quad_scene with one 4 x 4 diffuse texture (layout: include/dmt_hip.h dmt_upload_textures)"""
    sc = _quad_scene(pkg, 3.0, -1.0, 1.0, -1.0, 1.0)
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (16, 4), dtype=np.uint8)
    desc = np.array([[0, 4, 4]], np.int32)
    mat_tex = np.array([[0, 0xFFFFFFFF, 0xFFFFFFFF, 0]], np.uint32)
    uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
    sc.textures = (rgba, desc, mat_tex, uv)
    return sc
