"""The light layer's state (csrc/light_state.hpp): a long-lived context that reached a light configuration by a route -- the
mode set before or after the lights, another list or another env map first, the mode taken through the others, past a tree
too deep for the walk, across emissive triangles and textures that come and go, past refused calls and other uploads --
renders the same film, byte for byte, as a fresh context that was given that configuration directly, answers
dmt_test_light_tree and dmt_test_envmap with the same bytes or the same refusal, and leaves the same dmt_last_error.  The
configurations are {list A, list B} x sampling mode {0, 1, 2} x {no env map, a 16 x 8 map} x {brute force, BVH} on the Cornell
box.  dmt_sync passes after every case.  Every comparison is of bytes, integers or messages."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_light_tree_select as T

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = "(1)"
SIZE, DEPTH, SPP = 32, 4, 8
MODES, ENVS = (0, 1, 2), (None, 16)
UNKNOWN_MODE = "dmt_set_light_sampling: unknown mode"
BAD_RESOLUTION = "dmt_upload_envmap: resolution must be powers of two >= 8 with width == 2 * height"
ZERO_QUATERNION = "dmt_upload_envmap: zero quaternion"
TOO_DEEP_NOTE = "light tree: its depth of 61 exceeds the walk's guard of 60 levels; the uniform pick is used instead"
AREA_TRI, AREA_LE = [20], [[5, 5, 5]]


def _env_rgb(width):
    """a width x width/2 map from a seeded generator"""
    return np.random.default_rng(900 + width).uniform(0.05, 2.0, (width // 2, width, 3)).astype(F)


def _into_the_box(L):
    """the lights of a set of test_light_tree_select (around (0, 6, 0), +-3) moved under the Cornell box's ceiling"""
    L = L.copy()
    pos = L[:, 8:20].copy().view(F).reshape(-1, 3)
    pos[:] = (pos - F([0, 6, 0])) * F([0.3, 0.083, 0.3]) + F([0.0, 2.0, 0.6])
    L[:, 8:20] = pos.view(np.uint8).reshape(-1, 12)
    return L


class _World:
    """the Cornell box, the light lists by name, a texture set for it, and the probes' inputs"""

    def __init__(self, pkg):
        H = pkg.host_scene.load_host_library()
        f3 = lambda v: np.ascontiguousarray(v, F).ctypes.data_as(C.c_void_p)
        self.scenes = {n: pkg.host_scene.cornell_box(n, n) for n in (SIZE, 2 * SIZE)}
        sc = self.scenes[SIZE]
        distant, sky = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
        H.dmt_host_make_directional_light(f3([0.4, 0.4, 0.3]), f3([0.2, 0.6, -0.7]), C.c_float(0.0), distant.ctypes.data_as(C.c_void_p))
        H.dmt_host_make_environmental_light(f3([0.3, 0.4, 0.6]), sky.ctypes.data_as(C.c_void_p))
        A, B = _into_the_box(T.light_set(pkg, "n3")), _into_the_box(T.light_set(pkg, "n17"))
        none = np.zeros((0, 32), np.uint8)
        # name -> (point / spot / directional records, infinite records)
        self.lists = {
            "A": (A, none), "B": (B, none),
            "chain61": (T.light_set(pkg, "chain61", chain_yz=(2.0, 0.5)), none),   # the near end of the chain is inside the box
            "distant": (np.concatenate([A, distant[None]]), none),
            "none": (none, none),
            "infinite": (none, sky[None]),
        }
        tris, bsdfs = len(sc.mat_id), np.asarray(sc.bsdfs, np.uint8).size // 32
        rng = np.random.default_rng(77)
        mat_tex = np.full((bsdfs, 4), 0xFFFFFFFF, np.uint32)
        mat_tex[:, 3] = 0                      # anisotropy 0.f
        mat_tex[:, 0] = 0                      # every material takes its albedo from the one texture
        self.textures = (rng.integers(0, 256, (16, 4), dtype=np.uint8), np.array([[0, 4, 4]], np.int32), mat_tex, rng.uniform(0, 1, (tris, 6)).astype(F))
        k = 24
        self.p = (rng.uniform(-1.0, 1.0, (k, 3)) * [1.0, 1.0, 1.0] + [0.0, 1.5, 0.5]).astype(F)
        nrm = rng.normal(size=(k, 3))
        self.n = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
        self.u = ((np.arange(k) + 0.5) / k).astype(F)
        self.u2 = rng.uniform(0, 1, (k, 2)).astype(F)


@pytest.fixture(scope="module")
def W(pkg):
    return _World(pkg)


def _cfg(accel, lights, mode, env=None):
    """A light configuration: the name of its list, its sampling mode, its env map's width (None: never uploaded)."""
    return dict(accel=accel, lights=lights, mode=mode, env=env)


def _scene(r, W, accel):
    r.upload_scene(W.scenes[SIZE])
    r.set_limits(DEPTH)
    r.set_accel(accel)


def _lights(r, W, name):
    r.upload_lights(*W.lists[name])


def _env(r, width):
    if width is None:
        r.clear_envmap()
    else:
        r.upload_envmap(_env_rgb(width))


def _set(r, W, c):
    """The records of `c` on a context with the scene under it."""
    _lights(r, W, c["lights"])
    r.set_light_sampling(c["mode"])
    _env(r, c["env"])


def _refused(pkg, call, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_INVALID in msg and all(n in msg for n in needles), msg


def _answer(pkg, call):
    """what a probe answers: the bytes of its outputs, or its refusal"""
    try:
        out = call()
    except pkg.DmtError as e:
        return str(e)
    return tuple(v.tobytes() for v in (out.values() if isinstance(out, dict) else out))


def _render(r):
    r.film_clear()
    r.render(SPP)
    r.sync()


def _snap(r, pkg, W):
    """What a context shows of its light state.  A refused call first gives dmt_last_error a known text; then the film of one
    launch on a cleared film and the message that launch leaves, the two probes' answers, and the message they leave."""
    _refused(pkg, lambda: r.set_light_sampling(3), UNKNOWN_MODE)
    _render(r)
    after_render = r.last_error()
    mean, m2 = r.download_film()
    assert np.isfinite(mean).all()
    tree = _answer(pkg, lambda: r.test_light_tree(W.p, W.n, W.u, 0.5))
    env = _answer(pkg, lambda: r.test_envmap(W.u2, W.n))
    return mean.tobytes(), m2.tobytes(), after_render, tree, env, r.last_error()


@pytest.fixture(scope="module")
def fresh(pkg, W):
    """_snap of a fresh context that was given a configuration directly; each configuration is rendered once"""
    memo = {}

    def get(c):
        key = repr(sorted(c.items()))
        if key not in memo:
            r = pkg.Renderer(0)
            try:
                _scene(r, W, c["accel"])
                _set(r, W, c)
                memo[key] = _snap(r, pkg, W)
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


def _restart(old, W, accel):
    """the plain scene again (no emissive triangles, no textures), whatever lights, mode and env map the context has"""
    _scene(old, W, accel)
    old.upload_area_lights([], np.zeros((0, 3), F))
    old.set_lens(0.0)


ACCELS = pytest.mark.parametrize("accel", [0, 1])
LISTS = pytest.mark.parametrize("lights", ["A", "B"])


def _targets(accel, lights):
    return [_cfg(accel, lights, mode, env) for mode in MODES for env in ENVS]


def _other(lights):
    return "B" if lights == "A" else "A"


def test_the_configurations_differ(fresh):
    """what the comparisons below can tell apart: the twelve films of an accel mode are twelve different films, the trees
    answer the probe in modes 1 and 2 and the env map's probe answers with a map"""
    for accel in (0, 1):
        snaps = [fresh(c) for lights in "AB" for c in _targets(accel, lights)]
        assert len({s[:2] for s in snaps}) == 12
    for lights in "AB":
        for mode, env in itertools.product(MODES, ENVS):
            s = fresh(_cfg(0, lights, mode, env))
            assert isinstance(s[3], tuple) == (mode != 0) and isinstance(s[4], tuple) == (env is not None)
            assert s[2] == UNKNOWN_MODE                     # a launch leaves no message of its own
            assert s[2:] == fresh(_cfg(1, lights, mode, env))[2:]               # the probes do not depend on the accel mode
        assert fresh(_cfg(0, lights, 1))[3] != fresh(_cfg(0, lights, 2))[3]
        assert "uniformly" in fresh(_cfg(0, lights, 0))[3] and "no env map uploaded" in fresh(_cfg(0, lights, 0))[4]


# ---- (a) the mode before the lights, and after them ----------------------------------------------------------------------
@ACCELS
@LISTS
def test_mode_before_and_after_the_lights(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    for c in _targets(accel, lights):
        _env(old, c["env"])
        old.set_light_sampling(c["mode"])
        _lights(old, W, lights)
        assert _snap(old, pkg, W) == fresh(c)               # the mode first
        old.set_light_sampling(0)
        _lights(old, W, lights)
        _render(old)
        old.set_light_sampling(c["mode"])
        assert _snap(old, pkg, W) == fresh(c)               # the lights first, and a launch has seen them under mode 0
    old.sync()


# ---- (b) the other list first: a stale tree would show -------------------------------------------------------------------
@ACCELS
@LISTS
def test_the_other_list_first(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    for c in _targets(accel, lights):
        _set(old, W, {**c, "lights": _other(lights)})
        assert _snap(old, pkg, W) == fresh({**c, "lights": _other(lights)})
        _lights(old, W, lights)
        assert _snap(old, pkg, W) == fresh(c)
    old.sync()


# ---- (c) the mode taken through the others: both node buffers are live at once -------------------------------------------
@ACCELS
@LISTS
@pytest.mark.parametrize("tour", [(1, 2, 1), (2, 1, 2), (1, 0, 1)], ids=lambda t: "".join(map(str, t)))
def test_mode_tour(old, pkg, W, fresh, accel, lights, tour):
    _restart(old, W, accel)
    for env in ENVS:
        _env(old, env)
        _lights(old, W, lights)
        for mode in tour:
            old.set_light_sampling(mode)
            assert _snap(old, pkg, W) == fresh(_cfg(accel, lights, mode, env))
        old.set_light_sampling(tour[-1])                    # the mode it has: nothing is invalidated
        assert _snap(old, pkg, W) == fresh(_cfg(accel, lights, tour[-1], env))
    old.sync()


# ---- (d) a tree too deep for the walk ------------------------------------------------------------------------------------
@ACCELS
def test_too_deep_is_cleared_by_an_upload_and_by_a_mode_change_and_only_by_them(old, pkg, W, fresh, accel):
    _restart(old, W, accel)
    old.clear_envmap()
    old.set_light_sampling(0)
    _lights(old, W, "chain61")
    uniform = fresh(_cfg(accel, "chain61", 0))
    assert _snap(old, pkg, W) == uniform
    old.set_light_sampling(1)
    deep = _snap(old, pkg, W)
    assert deep == fresh(_cfg(accel, "chain61", 1))
    assert deep[:2] == uniform[:2] and deep[2] == TOO_DEEP_NOTE and "too deep" in deep[3] and "(61 levels)" in deep[3]
    # only the launch that finds out leaves the note; the next one runs the uniform rows without a word
    again = _snap(old, pkg, W)
    assert again[:2] == deep[:2] and again[2] == UNKNOWN_MODE and again[3:] == deep[3:]
    # what does not clear it: the same mode again, other uploads, the camera, the lens, an env map
    old.set_light_sampling(1)
    sc = W.scenes[SIZE]
    old.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
    old.upload_bsdfs(sc.bsdfs)
    old.set_camera(sc.camera)
    old.set_lens(0.0)
    old.upload_envmap(_env_rgb(16))
    old.clear_envmap()
    assert _snap(old, pkg, W) == again
    # a mode change clears it: the launch finds out again, under either tree
    for mode in (2, 1):
        old.set_light_sampling(mode)
        assert _snap(old, pkg, W) == fresh(_cfg(accel, "chain61", mode))
    # an upload clears it
    for lights, mode in itertools.product("AB", (1, 2)):
        _lights(old, W, "chain61")
        old.set_light_sampling(1)
        _render(old)
        assert old.last_error() == TOO_DEEP_NOTE
        if mode == 2:
            old.set_light_sampling(2)                       # a mode change, then the upload
            _render(old)
        _lights(old, W, lights)
        old.set_light_sampling(mode)
        for env in ENVS:
            _env(old, env)
            assert _snap(old, pkg, W) == fresh(_cfg(accel, lights, mode, env))
    old.sync()


# ---- (e) a directional record in the list --------------------------------------------------------------------------------
@ACCELS
@LISTS
def test_a_list_with_a_directional_light_first(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    old.clear_envmap()
    for mode in MODES:
        _lights(old, W, "distant")
        old.set_light_sampling(mode)
        snap = _snap(old, pkg, W)
        assert snap == fresh(_cfg(accel, "distant", mode))
        assert snap[:2] == fresh(_cfg(accel, "distant", 0))[:2]              # the uniform rows, whatever the mode
        assert ("keeps the uniform pick" if mode else "uniformly") in snap[3]
        _lights(old, W, lights)
        assert _snap(old, pkg, W) == fresh(_cfg(accel, lights, mode))
    old.sync()


# ---- (f) emissive triangles and textures come and go: the tree rows return with the tree that was there -------------------
@ACCELS
@LISTS
def test_emissive_triangles_and_textures_come_and_go(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    for c in _targets(accel, lights):
        _set(old, W, c)
        want = fresh(c)
        assert _snap(old, pkg, W) == want
        old.upload_area_lights(AREA_TRI, AREA_LE)
        with_area = _snap(old, pkg, W)
        assert with_area[:2] != want[:2] and with_area[4] == want[4]
        assert c["mode"] == 0 or "keeps the uniform pick" in with_area[3]
        old.upload_area_lights([], np.zeros((0, 3), F))     # the lights are not uploaded again
        assert _snap(old, pkg, W) == want
        old.upload_textures(*W.textures)
        with_tex = _snap(old, pkg, W)
        assert with_tex[4] == want[4]
        assert c["mode"] == 0 or (with_tex[:2] != want[:2] and "keeps the uniform pick" in with_tex[3])
        old.upload_textures(None, None, None, None)
        assert _snap(old, pkg, W) == want
    old.sync()


# ---- (g) the env map's route ---------------------------------------------------------------------------------------------
@ACCELS
@LISTS
def test_env_map_route(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    _lights(old, W, lights)
    for mode in MODES:
        old.set_light_sampling(mode)
        with_map, without = fresh(_cfg(accel, lights, mode, 16)), fresh(_cfg(accel, lights, mode))
        old.clear_envmap()
        old.clear_envmap()                                  # on a context without a map
        assert _snap(old, pkg, W) == without
        old.upload_envmap(_env_rgb(32))                     # another map of another size first
        other = _snap(old, pkg, W)
        assert other == fresh(_cfg(accel, lights, mode, 32)) and other[:2] != with_map[:2]
        old.upload_envmap(_env_rgb(16))
        assert _snap(old, pkg, W) == with_map
        old.upload_envmap(_env_rgb(32))                     # the larger one again: a smaller allocation does not linger
        old.upload_envmap(_env_rgb(16))
        assert _snap(old, pkg, W) == with_map
        old.clear_envmap()                                  # upload -> clear equals never uploaded
        assert _snap(old, pkg, W) == without
    old.sync()


# ---- (h) refused calls between -------------------------------------------------------------------------------------------
@ACCELS
@LISTS
def test_refused_calls_change_nothing(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    for c in _targets(accel, lights):
        _set(old, W, c)
        _render(old)
        _refused(pkg, lambda: old.upload_envmap(np.ones((6, 12, 3), F)), BAD_RESOLUTION)
        _refused(pkg, lambda: old.upload_envmap(np.ones((16, 16, 3), F)), BAD_RESOLUTION)
        _refused(pkg, lambda: old.upload_envmap(_env_rgb(32), quat=(0, 0, 0, 0)), ZERO_QUATERNION)
        _refused(pkg, lambda: old.set_light_sampling(3), UNKNOWN_MODE)
        assert _snap(old, pkg, W) == fresh(c)
    old.sync()


# ---- (i) other uploads and settings between: the layer survives them -----------------------------------------------------
@ACCELS
@LISTS
def test_survives_triangles_bsdfs_camera_and_lens(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    sc, large = W.scenes[SIZE], W.scenes[2 * SIZE]
    for c in _targets(accel, lights):
        _set(old, W, c)
        _render(old)
        old.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
        old.upload_bsdfs(sc.bsdfs)
        old.set_lens(0.05, 4.0)
        old.set_camera(large.camera)                        # four times the pixels
        old.set_accel(1 - accel)
        _render(old)
        old.set_lens(0.0)
        old.set_camera(sc.camera)
        old.set_accel(accel)
        assert _snap(old, pkg, W) == fresh(c)
    old.sync()


# ---- (j) empty lists count as uploaded -----------------------------------------------------------------------------------
@ACCELS
@pytest.mark.parametrize("lights", ["none", "infinite"])
def test_a_zero_count_list_and_a_list_of_infinite_lights_only(old, pkg, W, fresh, accel, lights):
    _restart(old, W, accel)
    for mode, env in itertools.product(MODES, ENVS):
        c = _cfg(accel, lights, mode, env)
        _set(old, W, {**c, "lights": "B"})
        _render(old)
        _lights(old, W, lights)
        snap = _snap(old, pkg, W)                           # it renders: the scene is complete
        assert snap == fresh(c)
        assert ("more than one light" if mode else "uniformly") in snap[3]
        assert snap[:2] == fresh(_cfg(accel, lights, 0, env))[:2]
    assert fresh(_cfg(accel, "none", 0))[:2] != fresh(_cfg(accel, "infinite", 0))[:2]
    old.sync()
