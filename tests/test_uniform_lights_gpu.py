"""One-record light lists through the scalar path (path_shade; RenderParams::uniformLights): a context reads lights[0] and
infLights[0] by scalar loads where the uniform pick runs over one record, and DMT_UNIFORM_LIGHTS=0, read when a context is
created, keeps the lane's pick and vector loads for every list.  dmt_uniform_lights_info shows that the switch reached the
launches of the two contexts.  Their films are equal byte for byte: for list sizes on both sides of one, on the brute-force,
BVH, env-map and BVH env-map rows (the last keeps the lane's pick in either context); for each kind of record, so that
every arm of the type switches runs on scalar registers; where emissive triangles make the pick run over two entries; under
both light-tree modes; and on a long-lived context whose list is replaced, against fresh contexts of either kind.  Frames are 64 x 64 x 8 spp at a bounce cap of 8 on Cornell's geometry.
After every render dmt_sync passes and the scheduler's counters show every work item folded once, no wave leaving early and
every parked hit taken back."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
SIZE, SPP, DEPTH = 64, 8, 8
ENV = "DMT_UNIFORM_LIGHTS"
ROWS = ("brute", "bvh", "env", "bvh_env")   # (bvh_env: a row uniform_lights_row leaves out)
AREA_TRI, AREA_LE = [20], [[5, 5, 5]]


def _ctx(pkg, on):
    """a context with the scalar path on (the default: the variable unset) or off"""
    saved = os.environ.pop(ENV, None)
    try:
        if not on:
            os.environ[ENV] = "0"
        return pkg.Renderer(0)
    finally:
        os.environ.pop(ENV, None)
        if saved is not None:
            os.environ[ENV] = saved


@pytest.fixture(scope="module")
def pair(pkg):
    """(default context, DMT_UNIFORM_LIGHTS=0 context): every case below sets its whole configuration on both"""
    on, off = _ctx(pkg, True), _ctx(pkg, False)
    yield on, off
    on.close()
    off.close()


class _World:
    def __init__(self, pkg):
        H = pkg.host_scene.load_host_library()
        f3 = lambda v: np.ascontiguousarray(v, F).ctypes.data_as(C.c_void_p)
        out = lambda: np.zeros(32, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.scene = pkg.host_scene.cornell_box(SIZE, SIZE)
        assert self.scene.lights.shape[0] == 1 and self.scene.inf_lights.shape[0] == 1
        spot = np.ascontiguousarray(self.scene.lights[0])
        assert int(spot[4:8].copy().view(np.uint32)[0]) >> 16 != int(self.scene.inf_lights[0][4:8].copy().view(np.uint32)[0]) >> 16
        point, enclosing, distant, sky2 = out(), out(), out(), out()
        inside = [0.0, 1.8, 0.6]                                                # under the box's ceiling
        H.dmt_host_make_point_light(f3([3, 2.5, 2]), f3(inside), C.c_float(0.02), p(point))
        H.dmt_host_make_point_light(f3([3, 2.5, 2]), f3(inside), C.c_float(1.1), p(enclosing))   # surfaces within 1.1 of it: the hadT / cosine-hemisphere arms
        H.dmt_host_make_directional_light(f3([0.9, 0.8, 0.7]), f3([0.2, 0.6, -0.7]), C.c_float(0.0), p(distant))
        H.dmt_host_make_environmental_light(f3([0.2, 0.5, 0.9]), p(sky2))
        self.kinds = {"spot": spot, "point": point, "enclosing": enclosing, "directional": distant}
        self.lights = np.stack([spot, point])
        self.inf = np.stack([np.ascontiguousarray(self.scene.inf_lights[0]), sky2])
        self.env_rgb = np.random.default_rng(1234).uniform(0.05, 2.0, (8, 16, 3)).astype(F)


@pytest.fixture(scope="module")
def W(pkg):
    return _World(pkg)


def _render(r):
    """(mean bytes, m2 bytes) of one frame on a cleared film; dmt_sync and the fold counters"""
    r.film_clear()
    r.sched_diag(reset=True)
    r.render(SPP)
    r.sync()
    mean, m2 = r.download_film()
    d = r.sched_diag(reset=True)
    assert d["folds"] == d["launched"] > 0 and d["early_exits"] == 0 and d["ggx_parked"] == d["ggx_resumed"], d
    assert np.isfinite(mean).all()
    return mean.tobytes(), m2.tobytes()


def _configure(r, W, row, lights, inf, mode=0, area=False):
    r.upload_scene(W.scene)
    r.set_limits(DEPTH)
    r.set_accel(1 if row.startswith("bvh") else 0)
    if row.endswith("env"):
        r.upload_envmap(W.env_rgb)
    else:
        r.clear_envmap()
    r.upload_area_lights(AREA_TRI if area else [], np.asarray(AREA_LE if area else np.zeros((0, 3)), F))
    r.upload_lights(lights, inf)
    r.set_light_sampling(mode)


def _both(pair, W, row, lights, inf, **kw):
    films = []
    for r in pair:
        _configure(r, W, row, lights, inf, **kw)
        films.append(_render(r))
    assert films[0] == films[1], (row, len(lights), len(inf), kw)
    return films[0]


def test_the_switch_reaches_the_launch(pkg, pair):
    """what every comparison below rests on: the default context passes the switch to its launches, the DMT_UNIFORM_LIGHTS=0
    context does not (dmt_uniform_lights_info reads it where a launch's arguments are filled), and any other value keeps it"""
    on, off = pair
    assert on.uniform_lights_info() is True and off.uniform_lights_info() is False
    os.environ[ENV] = "1"
    try:
        r = pkg.Renderer(0)
    finally:
        os.environ.pop(ENV, None)
    try:
        assert r.uniform_lights_info() is True
    finally:
        r.close()


@pytest.mark.parametrize("row", ROWS)
def test_list_sizes_on_both_sides_of_one(pair, W, row):
    films = {}
    for nl, ni in ((1, 1), (1, 0), (0, 1), (2, 1), (1, 2), (0, 0)):
        films[nl, ni] = _both(pair, W, row, W.lights[:nl], W.inf[:ni])
    # what the comparison can tell apart: the lists change the film (the constant environment only where no map hides it)
    assert films[1, 1] != films[2, 1] and films[1, 0] != films[0, 0]
    if not row.endswith("env"):
        assert len(set(films.values())) == 6


@pytest.mark.parametrize("row", ROWS)
def test_every_kind_of_single_record(pair, W, row):
    films = [_both(pair, W, row, rec[None], W.inf[:1]) for rec in W.kinds.values()]
    assert len(set(films)) == len(W.kinds)
    # the same records without an infinite light: the miss arm's list is empty, the hit arm's has one record
    _both(pair, W, row, W.kinds["enclosing"][None], W.inf[:0])


@pytest.mark.parametrize("row", ROWS)
def test_one_light_and_one_emissive_triangle(pair, W, row):
    """the pick runs over two entries (nAll == 2): the lane's pick, whatever the switch says"""
    with_area = _both(pair, W, row, W.lights[:1], W.inf[:1], area=True)
    assert with_area != _both(pair, W, row, W.lights[:1], W.inf[:1])


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("row", ROWS)
def test_light_tree_modes(pair, W, row, mode):
    """one record keeps the uniform rows under either tree mode; two records run the tree rows, which the switch leaves alone"""
    one = _both(pair, W, row, W.lights[:1], W.inf[:1], mode=mode)
    assert one == _both(pair, W, row, W.lights[:1], W.inf[:1])
    two = _both(pair, W, row, W.lights, W.inf[:1], mode=mode)
    assert two != one


@pytest.mark.parametrize("row", ["brute", "bvh"])
def test_a_replaced_record_on_a_long_lived_context(pkg, W, row):
    """one light, then two, then ONE OTHER light through dmt_upload_lights alone: each film is the film of a fresh context that
    was given those lights directly (a record left in the scalar cache would show), with the switch on and with it off"""
    def fresh(lights, inf, on):
        r = _ctx(pkg, on)
        try:
            _configure(r, W, row, lights, inf)
            return _render(r)
        finally:
            r.close()

    steps = [(W.lights[:1], W.inf[:1]), (W.lights, W.inf[:1]), (W.lights[1:], W.inf[1:]), (W.kinds["directional"][None], W.inf[:1])]
    old = _ctx(pkg, True)
    try:
        assert old.uniform_lights_info() is True
        _configure(old, W, row, *steps[0])
        seen = []
        for k, (lights, inf) in enumerate(steps):
            if k:
                old.upload_lights(lights, inf)
            seen.append(_render(old))
            assert seen[-1] == fresh(lights, inf, True), k
            assert seen[-1] == fresh(lights, inf, False), k
        assert len(set(seen)) == len(steps)
    finally:
        old.close()
