"""The camera layer's state (csrc/camera_state.hpp): a long-lived context that reached a camera configuration by a route -- the
lens or the filter set before or after the camera, another filter first, to the default and back, radius 0 with another
distance and back, the other resolution and back, a bound film kept and given up, a scene re-upload, refused calls between --
renders the same film, byte for byte, as a fresh context that was given that configuration directly, and answers
dmt_lens_info, dmt_pixel_filter_info, dmt_film_device_ptrs, dmt_focus_distance_at and dmt_last_error alike.  The
configurations are {pinhole, lens 0.05 focused on the frame's centre} x {box 0.5, tent 1, Gaussian 1.5 sigma 0.5} x {own
film, bound film} x {brute force, BVH} on the Cornell box at 32 x 32, depth 4, 8 spp; 48 x 32 is the other resolution.
dmt_sync passes after every case.  Every comparison is of bytes, integers or messages."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = "(1)"
SIZE, OTHER, DEPTH, SPP = 32, (48, 32), 4, 8
CENTRE = (16.0, 16.0)
LENS_RADIUS = 0.05
LENSES = ("pinhole", "lens")
FILTERS = {"box": (0, 0.5, 0.0), "tent": (1, 1.0, 0.0), "gaussian": (2, 1.5, 0.5)}
BAD_FILTER = "dmt_set_pixel_filter: a kind DMT_FILTER_BOX .. DMT_FILTER_BLACKMAN_HARRIS, a finite radius in (0, 8], and for the Gaussian a finite sigma > 0"
NO_MASS = "dmt_set_pixel_filter: the Gaussian's sigma is too large for its radius (the profile has no mass)"
BAD_RADIUS = "dmt_set_lens: the radius must be finite and >= 0"
BAD_DISTANCE = "dmt_set_lens: the focus distance must be finite and > 0"
BAD_CAMERA = "dmt_set_camera: bad camera / resolution"
NULL_FILM = "dmt_film_bind: null buffer"


class _World:
    """the Cornell box at both resolutions"""

    def __init__(self, pkg):
        self.scene = pkg.host_scene.cornell_box(SIZE, SIZE)
        self.other = pkg.host_scene.cornell_box(*OTHER)


def _hip_runtime():
    """the HIP runtime the library has brought into the process"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "torch" not in line})
    assert paths, "libdmt_hip.so is loaded and links the HIP runtime"
    return C.CDLL(paths[0])


class _Film:
    """a caller's film: two device arrays of 32 x 32 float4 of this process's own, and their addresses"""
    BYTES = SIZE * SIZE * 16

    def __init__(self):
        self.hip = _hip_runtime()
        self.ptrs = tuple(self._alloc() for _ in range(2))
        assert self.hip.hipDeviceSynchronize() == 0         # the zeroes are in place before any stream writes the arrays

    def _alloc(self):
        ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(ptr), C.c_size_t(self.BYTES)) == 0
        assert self.hip.hipMemset(ptr, 0, C.c_size_t(self.BYTES)) == 0
        return ptr.value

    def read(self, which):
        """the bytes of the mean (0) or the M2 (1) array; the caller has drained the context's stream"""
        out = np.zeros(self.BYTES, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptrs[which]), C.c_size_t(self.BYTES), 2) == 0   # hipMemcpyDeviceToHost
        return out.tobytes()

    def free(self):
        for ptr in self.ptrs:
            assert self.hip.hipFree(C.c_void_p(ptr)) == 0


@pytest.fixture(scope="module")
def W(pkg):
    return _World(pkg)


def _cfg(accel, film, lens, filt):
    return dict(accel=accel, film=film, lens=lens, filt=filt)


def _scene(r, W, accel):
    r.upload_scene(W.scene)
    r.set_limits(DEPTH)
    r.set_accel(accel)


def _lens(r, lens):
    if lens == "lens":
        r.set_lens(LENS_RADIUS, r.focus_distance_at(*CENTRE))
    else:  # radius 0 keeps the distance of the last radius > 0: a new context's 1 goes in first
        r.set_lens(LENS_RADIUS, 1.0)
        r.set_lens(0.0)


def _set(r, c, film):
    """The records of `c` on a context with the scene, the 32 x 32 camera and an own film under it."""
    r.set_pixel_filter(*FILTERS[c["filt"]])
    _lens(r, c["lens"])
    if c["film"] == "bound":
        r.film_bind(*film.ptrs)


def _own_film(r, W):
    """the context's own 32 x 32 film again, whatever it had: only a change of resolution gives a bound film up"""
    r.set_camera(W.other.camera)
    r.set_camera(W.scene.camera)


def _refused(pkg, call, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_INVALID in msg and all(n in msg for n in needles), msg


def _render(r):
    r.film_clear()
    r.render(SPP)
    r.sync()


def _snap(r, pkg, film):
    """What a context shows of its camera state.  A refused call first gives dmt_last_error a known text; then the film of one
    launch on a cleared film and the message it leaves, the lens, the filter, whose film it is, the focus distance at the
    frame's centre, and the message all that leaves."""
    _refused(pkg, lambda: r.set_pixel_filter(7, 1.0), BAD_FILTER)
    _render(r)
    after_render = r.last_error()
    mean, m2 = r.download_film()
    assert np.isfinite(mean).all()
    ptrs = r.film_device_ptrs()
    assert ptrs[0] and ptrs[1]
    whose = "bound" if ptrs == film.ptrs else "own"
    if whose == "bound":  # a bound pointer is the caller's own: the launch wrote the caller's arrays
        assert film.read(0) == mean.tobytes() and film.read(1) == m2.tobytes()
    else:
        assert ptrs[0] not in film.ptrs and ptrs[1] not in film.ptrs
    lens = np.array(r.lens_info(), F).tobytes()
    filt = tuple(sorted(r.pixel_filter_info().items()))
    focus = np.array(r.focus_distance_at(*CENTRE), F).tobytes()
    return mean.tobytes(), m2.tobytes(), after_render, lens, filt, whose, focus, r.last_error()


@pytest.fixture(scope="module")
def fresh(pkg, W):
    """_snap of a fresh context that was given a configuration directly; each configuration is rendered once"""
    memo = {}

    def get(c):
        key = repr(sorted(c.items()))
        if key not in memo:
            r, film = pkg.Renderer(0), _Film()
            try:
                _scene(r, W, c["accel"])
                _set(r, c, film)
                memo[key] = _snap(r, pkg, film)
            finally:
                r.close()
                film.free()
        return memo[key]
    return get


@pytest.fixture(scope="module")
def old(pkg):
    """the long-lived context and the film it binds: every test below goes on from where the one before left it"""
    r, film = pkg.Renderer(0), _Film()
    yield r, film
    r.close()
    film.free()


def _restart(old, W, accel):
    """the scene, the 32 x 32 camera and an own film, whatever lens and filter the context has"""
    r, _ = old
    _scene(r, W, accel)
    _own_film(r, W)


ACCELS = pytest.mark.parametrize("accel", [0, 1])
FILMS = pytest.mark.parametrize("film", ["own", "bound"])


def _targets(accel, film):
    return [_cfg(accel, film, lens, filt) for lens in LENSES for filt in FILTERS]


def test_the_configurations_differ(fresh):
    """what the comparisons below can tell apart: the six lens x filter films of an accel mode are six different films, a
    bound film holds what an own one does, and the infos name the configuration"""
    for accel in (0, 1):
        own = [fresh(c) for c in _targets(accel, "own")]
        bound = [fresh(c) for c in _targets(accel, "bound")]
        assert len({s[:2] for s in own}) == 6
        for a, b in zip(own, bound):
            assert a[:5] == b[:5] and a[6:] == b[6:] and (a[5], b[5]) == ("own", "bound")
            assert a[2] == a[7] == BAD_FILTER                                   # neither a launch nor an info call leaves a message
        assert len({s[3] for s in own}) == 2 and len({s[4] for s in own}) == 3
        assert len({s[6] for s in own}) == 1                                    # the focus probe is a pinhole ray: no lens, no filter


# ---- (a) the lens and the filter before the camera, and after it ----------------------------------------------------------
@ACCELS
@FILMS
def test_lens_and_filter_before_and_after_the_camera(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, film):
        _own_film(r, W)
        focus = r.focus_distance_at(*CENTRE)
        r.set_camera(W.other.camera)
        _set(r, {**c, "film": "own"}, buf)                  # under the other camera: its focus distance is not the target's
        if c["lens"] == "lens":
            r.set_lens(LENS_RADIUS, focus)
        r.set_camera(W.scene.camera)                        # the camera last; the lens and the filter survive it
        if film == "bound":
            r.film_bind(*buf.ptrs)
        assert _snap(r, pkg, buf) == fresh(c)
        _own_film(r, W)
        r.set_lens(0.0), r.set_pixel_filter(0, 0.5)
        _render(r)
        _set(r, c, buf)                                     # the camera first, and a launch has seen it under the defaults
        assert _snap(r, pkg, buf) == fresh(c)
    r.sync()


# ---- (b) another filter first: a stale table would show -------------------------------------------------------------------
@ACCELS
@FILMS
def test_another_filter_first(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, film):
        for other in FILTERS:
            if other != c["filt"]:
                _set(r, {**c, "filt": other}, buf)
                assert _snap(r, pkg, buf) == fresh({**c, "filt": other})
        _set(r, c, buf)
        assert _snap(r, pkg, buf) == fresh(c)
    r.sync()


# ---- (c) to the defaults and back: the table is kept, unread ---------------------------------------------------------------
@ACCELS
@FILMS
def test_to_the_defaults_and_back(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, film):
        _set(r, c, buf)
        assert _snap(r, pkg, buf) == fresh(c)
        _set(r, {**c, "lens": "pinhole", "filt": "box"}, buf)
        default = _snap(r, pkg, buf)
        assert default == fresh({**c, "lens": "pinhole", "filt": "box"})
        assert dict(default[4])["active"] is False
        _set(r, c, buf)
        assert _snap(r, pkg, buf) == fresh(c)
    r.sync()


# ---- (d) radius 0 with another distance, and back --------------------------------------------------------------------------
@ACCELS
@FILMS
def test_radius_zero_ignores_and_keeps_the_distance(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, film):
        _set(r, c, buf)
        kept = r.lens_info()[1]
        r.set_lens(0.0, 7.0)
        assert r.lens_info() == (0.0, kept)                 # the distance given with radius 0 is ignored
        pinhole = _snap(r, pkg, buf)
        assert pinhole[:3] == fresh({**c, "lens": "pinhole"})[:3] and pinhole[4:] == fresh({**c, "lens": "pinhole"})[4:]
        if c["lens"] == "lens":
            r.set_lens(LENS_RADIUS, kept)
        assert _snap(r, pkg, buf) == fresh(c)
    with pkg.Renderer(0) as new:
        new.set_lens(0.0, 7.0)
        assert new.lens_info() == (0.0, 1.0)
    r.sync()


# ---- (e) the other resolution and back -------------------------------------------------------------------------------------
@ACCELS
@FILMS
def test_the_other_resolution_and_back(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, film):
        _set(r, c, buf)
        _render(r)
        r.set_camera(W.other.camera)                        # a new own film, zeroed: a bound one is given up
        wide = r.film_device_ptrs()
        assert wide[0] not in buf.ptrs and wide[1] not in buf.ptrs
        mean, m2 = r.download_film()
        assert mean.shape == (OTHER[1], OTHER[0], 4) and not mean.any() and not m2.any()
        r.render(SPP)
        r.sync()
        assert np.isfinite(r.download_film()[0]).all()
        r.set_camera(W.scene.camera)
        mean, m2 = r.download_film()
        assert mean.shape == (SIZE, SIZE, 4) and not mean.any() and not m2.any()
        assert r.film_device_ptrs()[0] not in buf.ptrs      # back at 32 x 32 the film is the context's own
        if film == "bound":
            r.film_bind(*buf.ptrs)
        assert _snap(r, pkg, buf) == fresh(c)
    r.sync()


# ---- (f) a bound film is kept across a camera of the same size, and given up at another size -------------------------------
@ACCELS
def test_a_bound_film_across_cameras(old, pkg, W, fresh, accel):
    r, buf = old
    _restart(old, W, accel)
    for c in _targets(accel, "bound"):
        _set(r, c, buf)
        _render(r)
        before = buf.read(0)
        r.set_camera(W.scene.camera)                        # the same size: the film and every value in it stay
        assert r.film_device_ptrs() == buf.ptrs and buf.read(0) == before
        assert r.download_film()[0].tobytes() == before
        assert _snap(r, pkg, buf) == fresh(c)
        r.set_camera(W.other.camera)
        assert r.film_device_ptrs()[0] not in buf.ptrs
        r.set_camera(W.scene.camera)
        assert _snap(r, pkg, buf) == fresh({**c, "film": "own"})
        assert buf.read(0) == fresh(c)[0]                  # the caller's arrays were left alone since
    r.sync()


# ---- (g) a scene re-upload between: the layer survives it ------------------------------------------------------------------
@ACCELS
@FILMS
def test_survives_a_scene_upload(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    sc = W.scene
    for c in _targets(accel, film):
        _set(r, c, buf)
        _render(r)
        r.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
        r.upload_bsdfs(sc.bsdfs)
        r.upload_lights(sc.lights, sc.inf_lights)
        r.set_accel(1 - accel)
        _render(r)
        r.set_accel(accel)
        assert _snap(r, pkg, buf) == fresh(c)
    r.sync()


# ---- (h) refused calls between ---------------------------------------------------------------------------------------------
@ACCELS
@FILMS
def test_refused_calls_change_nothing(old, pkg, W, fresh, accel, film):
    r, buf = old
    _restart(old, W, accel)
    no_camera = np.array(W.scene.camera, np.uint8).copy()
    no_camera[24:32] = 0                                    # 0 x 0
    for c in _targets(accel, film):
        _set(r, c, buf)
        _render(r)
        for call, why in [(lambda: r.set_pixel_filter(7, 1.0), BAD_FILTER), (lambda: r.set_pixel_filter(1, 0.0), BAD_FILTER),
                          (lambda: r.set_pixel_filter(1, 9.0), BAD_FILTER), (lambda: r.set_pixel_filter(2, 1.0, 1e9), NO_MASS),
                          (lambda: r.set_lens(-1.0, 2.0), BAD_RADIUS), (lambda: r.set_lens(0.05, 0.0), BAD_DISTANCE),
                          (lambda: r.set_camera(no_camera), BAD_CAMERA), (lambda: r.film_bind(0, buf.ptrs[1]), NULL_FILM),
                          (lambda: r.film_bind(buf.ptrs[0], 0), NULL_FILM)]:
            _refused(pkg, call, why)
            assert r.last_error() == why                    # a refused call changes dmt_last_error
        assert (r.width, r.height) == (SIZE, SIZE)
        assert _snap(r, pkg, buf) == fresh(c)               # and nothing else
    r.sync()
