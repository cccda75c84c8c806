"""The medium layer's state (csrc/medium_state.hpp): a long-lived context that reached a medium configuration by a route --
in another set order, from another box, across uploads and other settings, past refused calls, through the clear calls --
renders the same film, byte for byte, as a fresh context that was given that configuration directly, and its three *_info
calls answer the same field for field.  The configurations are {homogeneous, + grid, + spectrum, + both} x {brute force,
BVH} on the Cornell box.  dmt_sync passes after every case.  Every comparison is of bytes, integers or messages."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = "(1)"
SIZE, DEPTH, SPP = 32, 4, 8
FOG = dict(sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))   # as test_medium_gpu.py
ELSEWHERE = dict(sigma_t=0.9, albedo=(0.5, 0.5, 0.5), g=-0.2, box_min=(-0.5, 1.0, -1.0), box_max=(1.0, 2.0, 0.5))
SPECTRUM = ((1.0, 0.6, 0.3), (0.05, 0.1, 0.2))   # extinction colour, emission
GRIDS = {
    "plume": np.load(GOLDEN / "medium_grid_plume_8.npy"),
    "two": np.array([[[0.0, 0.7]]], F),          # 2 x 1 x 1, one voxel > 0: the smallest support that is not the whole grid
    "zeros": np.zeros((1, 1, 2), F),
}
KINDS = {"homogeneous": (None, None), "grid": ("plume", None), "spectrum": (None, SPECTRUM), "grid+spectrum": ("plume", SPECTRUM)}


def _cfg(accel, medium=FOG, grid=None, spectrum=None):
    """A medium configuration: the medium's record (None: never set), the name of its grid, its spectrum."""
    return dict(accel=accel, medium=medium, grid=grid, spectrum=spectrum)


def _kind(accel, kind, **kw):
    grid, spectrum = KINDS[kind]
    return _cfg(accel, grid=grid, spectrum=spectrum, **kw)


SETTERS = {
    "medium": lambda r, c: r.set_medium(**c["medium"]),
    "grid": lambda r, c: r.set_medium_grid(GRIDS[c["grid"]]),
    "spectrum": lambda r, c: r.set_medium_spectrum(*c["spectrum"]),
}


def _records(c):
    return [k for k in ("medium", "grid", "spectrum") if c[k] is not None]


def _set(r, c, order=None):
    """The records of `c`, set in `order` on a context without a medium."""
    for k in order or _records(c):
        SETTERS[k](r, c)


@pytest.fixture(scope="module")
def scenes(pkg):
    return {n: pkg.host_scene.cornell_box(n, n) for n in (SIZE, 2 * SIZE)}


def _scene(r, scenes, accel):
    r.upload_scene(scenes[SIZE])
    r.set_limits(DEPTH)
    r.set_accel(accel)


def _plain(v):
    return v.tobytes() if isinstance(v, np.ndarray) else v


def _infos(r):
    return tuple(tuple(sorted((k, _plain(v)) for k, v in info.items())) for info in (r.medium_info(), r.medium_grid_info(), r.medium_spectrum_info()))


def _snap(r):
    """The film of one launch on a cleared film, and every field of the three *_info calls."""
    r.film_clear()
    r.render(SPP)
    r.sync()
    mean, m2 = r.download_film()
    assert np.isfinite(mean).all()
    return mean.tobytes(), m2.tobytes(), _infos(r)


@pytest.fixture(scope="module")
def fresh(pkg, scenes):
    """_snap of a fresh context that was given a configuration directly; each configuration is rendered once"""
    memo = {}

    def get(c):
        key = repr(sorted(c.items()))
        if key not in memo:
            r = pkg.Renderer(0)
            try:
                _scene(r, scenes, c["accel"])
                _set(r, c)
                memo[key] = _snap(r)
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


def _restart(old, scenes, accel):
    if old.width != SIZE:
        _scene(old, scenes, accel)
    old.set_accel(accel)
    old.clear_medium()


def _refused(pkg, call, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_INVALID in msg and all(n in msg for n in needles), msg


ACCELS = pytest.mark.parametrize("accel", [0, 1])
ALL_KINDS = pytest.mark.parametrize("kind", list(KINDS))


def test_the_configurations_differ(fresh):
    """what the comparisons below can tell apart: the eight films and the film without a medium are nine different films"""
    for accel in (0, 1):
        films = {fresh(_kind(accel, kind))[:2] for kind in KINDS} | {fresh(_cfg(accel, medium=None))[:2]}
        assert len(films) == len(KINDS) + 1


# ---- (a) set order ---------------------------------------------------------------------------------------------------
@ACCELS
@pytest.mark.parametrize("order", list(itertools.permutations(("spectrum", "grid", "medium"))), ids="-".join)
def test_set_order(old, scenes, fresh, accel, order):
    c = _kind(accel, "grid+spectrum")
    _restart(old, scenes, accel)
    _set(old, c, order)
    assert _snap(old) == fresh(c)
    old.sync()


# ---- (b) box move ----------------------------------------------------------------------------------------------------
@ACCELS
@ALL_KINDS
def test_box_move(old, scenes, fresh, accel, kind):
    """the grid's cell size and support bounds are of the box a launch finds, not of the box the grid was uploaded under"""
    c = _kind(accel, kind)
    if kind == "grid":
        c["grid"] = "two"
    _restart(old, scenes, accel)
    _set(old, {**c, "medium": ELSEWHERE})
    if kind == "grid+spectrum":
        assert _snap(old) == fresh({**c, "medium": ELSEWHERE})   # and a launch has seen the other box
    old.set_medium(**c["medium"])
    assert _snap(old) == fresh(c)
    old.sync()


# ---- (c) survival ----------------------------------------------------------------------------------------------------
@ACCELS
@ALL_KINDS
def test_survives_uploads_camera_lens_accel_and_a_larger_render(old, scenes, fresh, accel, kind):
    c = _kind(accel, kind)
    _restart(old, scenes, accel)
    _set(old, c)
    infos = _infos(old)
    _scene(old, scenes, 1 - accel)                # a scene re-upload, the other accel
    old.set_lens(0.05, 4.0)
    old.set_camera(scenes[2 * SIZE].camera)       # four times the pixels
    assert _infos(old) == infos
    old.film_clear()
    old.render(SPP)
    old.sync()
    old.set_lens(0.0)
    old.set_camera(scenes[SIZE].camera)
    old.set_accel(accel)
    assert _snap(old) == fresh(c)
    old.sync()


# ---- (d) refused calls between ---------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime the library has brought into the process"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "torch" not in line})
    assert paths, "libdmt_hip.so is loaded and links the HIP runtime"
    return C.CDLL(paths[0])


def _refused_device_grid(pkg, r, density, *needles):
    """dmt_set_medium_grid_device with `density` in device memory of this process's own"""
    hip = _hip_runtime()
    nz, ny, nx = density.shape
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(density.nbytes)) == 0
    try:
        assert hip.hipMemcpy(ptr, density.ctypes.data_as(C.c_void_p), C.c_size_t(density.nbytes), 1) == 0   # hipMemcpyHostToDevice
        _refused(pkg, lambda: r._check(r._lib.dmt_set_medium_grid_device(r._ctx, ptr, nx, ny, nz), "dmt_set_medium_grid_device"), *needles)
    finally:
        assert hip.hipFree(ptr) == 0


@ACCELS
@ALL_KINDS
def test_refused_calls_change_nothing(old, pkg, scenes, fresh, accel, kind):
    c = _kind(accel, kind)
    _restart(old, scenes, accel)
    _set(old, c)
    infos = _infos(old)
    bad = np.ones((2, 3, 4), F)
    bad[1, 2, 3] = np.nan
    _refused(pkg, lambda: old.set_medium(**{**ELSEWHERE, "g": 1.0}), "dmt_set_medium: g must be in (-1, 1)")
    _refused(pkg, lambda: old.set_medium_grid(bad), "dmt_set_medium_grid: every density must be finite and >= 0; voxel (3, 2, 1) is not")
    _refused_device_grid(pkg, old, bad, "dmt_set_medium_grid_device: every density must be finite and >= 0; voxel (3, 2, 1) is not")
    _refused(pkg, lambda: old.set_medium_spectrum((0, 0, 0), (1, 1, 1)), "dmt_set_medium_spectrum: the extinction colour must not be all zero")
    assert _infos(old) == infos
    assert _snap(old) == fresh(c)
    old.sync()


# ---- (e) clear rules -------------------------------------------------------------------------------------------------
@ACCELS
def test_clear_rules(old, scenes, fresh, accel):
    c = _kind(accel, "grid+spectrum")
    _restart(old, scenes, accel)
    _set(old, c)
    old.clear_medium_grid()
    assert _snap(old) == fresh(_kind(accel, "spectrum"))
    old.set_medium_grid(GRIDS[c["grid"]])
    old.clear_medium_spectrum()
    assert _snap(old) == fresh(_kind(accel, "grid"))
    old.set_medium_spectrum(*SPECTRUM)
    assert _infos(old) == fresh(c)[2]
    old.clear_medium()
    assert _snap(old) == fresh(_cfg(accel, medium=None))
    old.sync()


# ---- (f) degenerate records ------------------------------------------------------------------------------------------
@ACCELS
def test_degenerate_records(old, scenes, fresh, accel):
    none = fresh(_cfg(accel, medium=None))
    _restart(old, scenes, accel)
    # sigma_t == 0, with a grid and a spectrum present
    c = _kind(accel, "grid+spectrum", medium={**FOG, "sigma_t": 0.0})
    _set(old, c)
    snap = _snap(old)
    assert snap[:2] == none[:2] and snap == fresh(c)
    assert not old.medium_info()["active"]
    assert old.medium_grid_info()["present"] and not old.medium_grid_info()["active"]
    assert old.medium_spectrum_info()["present"] and not old.medium_spectrum_info()["active"]
    # a grid without a density > 0
    old.clear_medium()
    c = _cfg(accel, grid="zeros")
    _set(old, c)
    snap = _snap(old)
    assert snap[:2] == none[:2] and snap == fresh(c)
    g = old.medium_grid_info()
    assert g["present"] and not g["active"] and g["positive"] == 0 and g["support_min"] > g["support_max"]
    assert not old.medium_info()["active"]
    # three equal channel extinctions and no emission: the grey rows, at k = 2 sigma_t
    old.clear_medium()
    c = _cfg(accel, spectrum=((2.0, 2.0, 2.0), (0.0, 0.0, 0.0)))
    _set(old, c)
    snap = _snap(old)
    assert snap[:2] == fresh(_cfg(accel, medium={**FOG, "sigma_t": float(F(2) * F(FOG["sigma_t"]))}))[:2] and snap == fresh(c)
    s = old.medium_spectrum_info()
    assert s["present"] and not s["active"] and s["k"].tolist() == [F(2) * F(FOG["sigma_t"])] * 3
    assert old.medium_info()["active"]
    old.clear_medium()
    old.sync()
