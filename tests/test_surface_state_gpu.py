"""The surface-attribute layer's state (surface_state.hpp): a context that reaches a state by a route renders the same film,
and answers the same *_info, as a fresh context that was given that state directly.  Routes through re-uploads of the soup,
the BSDFs and the textures (what each drops and keeps), refused uploads, mismatching texture tables, and the four first-hit
kernel variants with their refused pairs.  Every comparison is of bytes or integers."""
import numpy as np
import pytest

import cutout_ref as CR

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = "(1)", "(3)"
SPP, DEPTH = 4, 4
AREA_TRI, AREA_LE = [20], [[5, 5, 5]]
NO_OPACITY = {"cutout_triangles": 0, "cutout_materials": 0, "cutoff": 0.0}


class _Scene:
    """the Cornell box plus three cutout cards (32 triangles, four small textures), its smooth normals and a key 1"""

    def __init__(self, O, pkg):
        yy, xx = np.mgrid[0:16, 0:16]
        vary = (127.5 + 120 * np.sin(xx * 0.9) * np.cos(yy * 0.7)).astype(np.uint8)
        alphas = [CR.checker(16, 20, 235, 2), vary, np.full((8, 8), 255, np.uint8), np.zeros((4, 4), np.uint8)]
        meshes = [(T, uv * F(1.6) - F(0.3), tex) for (T, uv), tex in zip(CR.cornell_cards(), (1, 1, 0))]
        self.sc = sc = CR.CutScene(O.cornell_box(32, 32), meshes, alphas)
        self.n = sc.tri_count
        self.normals = pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0)
        self.key1 = [np.asarray(a, F).copy() for a in (sc.xs, sc.ys, sc.zs)]
        self.key1[0][26:] += F(0.2)  # the cards move


@pytest.fixture(scope="module")
def S(O, pkg):
    return _Scene(O, pkg)


def _upload(r, S, accel, tex=False, opacity=False, normals=False, area=False):
    sc = S.sc
    r.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
    r.upload_bsdfs(sc.bsdfs)
    r.upload_lights(sc.lights, sc.inf_lights)
    r.set_camera(sc.camera)
    if tex:
        r.upload_textures(sc.tex_rgba, sc.tex_desc, sc.mat_tex, sc.tri_uv)
    if normals:
        r.upload_vertex_normals(S.normals)
    if opacity:
        r.upload_opacity(sc.mat_opacity, 0.5)
    if area:
        r.upload_area_lights(AREA_TRI, AREA_LE)
    r.set_limits(DEPTH)
    r.set_accel(accel)


def _snap(r):
    """what a context shows of its state: the film's bytes and the two *_info answers"""
    r.film_clear()
    r.render(SPP)
    r.sync()
    mean, m2 = r.download_film()
    return mean.tobytes(), m2.tobytes(), r.vertex_normals_info(), r.opacity_info()


@pytest.fixture(scope="module")
def fresh(pkg, S):
    """_snap of a fresh context that was given a state directly; each (accel, state) is rendered once for the module"""
    memo = {}

    def get(accel, **state):
        key = (accel,) + tuple(sorted(state.items()))
        if key not in memo:
            r = pkg.Renderer(0)
            try:
                _upload(r, S, accel, **state)
                memo[key] = _snap(r)
            finally:
                r.close()
        return memo[key]
    return get


@pytest.fixture()
def ctx(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _refused(pkg, call, code, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert code in msg and all(n in msg for n in needles), msg


# ---- (a) what drops the opacity records -------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_opacity_route(ctx, pkg, S, fresh, accel):
    sc = S.sc
    textured, cutout = fresh(accel, tex=True), fresh(accel, tex=True, opacity=True)
    assert cutout[:2] != textured[:2] and cutout[3] == {"cutout_triangles": 6, "cutout_materials": 3, "cutoff": 0.5}
    _upload(ctx, S, accel, tex=True, opacity=True)
    for again in (lambda: ctx.upload_textures(sc.tex_rgba, sc.tex_desc, sc.mat_tex, sc.tri_uv), lambda: ctx.upload_bsdfs(sc.bsdfs)):
        again()
        assert _snap(ctx) == textured
        ctx.upload_opacity(sc.mat_opacity, 0.5)
        assert _snap(ctx) == cutout


# ---- (b) emissive triangles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_emissive_triangle_route(ctx, pkg, S, fresh, accel):
    sc = S.sc
    plain, lit = fresh(accel), fresh(accel, area=True)
    assert lit[:2] != plain[:2]
    _upload(ctx, S, accel, area=True)
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)  # the same soup again: the list was of the one replaced
    assert _snap(ctx) == plain
    ctx.upload_area_lights(AREA_TRI, AREA_LE)
    assert _snap(ctx) == lit
    ctx.upload_area_lights(AREA_TRI, AREA_LE)
    assert _snap(ctx) == lit
    ctx.update_vertices(sc.xs, sc.ys, sc.zs)              # the same positions: kept
    assert _snap(ctx) == lit
    _refused(pkg, lambda: ctx.upload_area_lights([S.n], AREA_LE), ERR_INVALID, "outside the uploaded soup")
    assert _snap(ctx) == plain                            # a refused list leaves none


@pytest.mark.parametrize("accel", [0, 1])
def test_emissive_triangles_before_any_soup(ctx, pkg, S, fresh, accel):
    ctx.upload_area_lights(AREA_TRI, AREA_LE)
    _upload(ctx, S, accel)
    assert _snap(ctx) == fresh(accel)


# ---- (c) vertex normals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_vertex_normal_route(ctx, pkg, S, fresh, accel):
    sc = S.sc
    textured, smooth = fresh(accel, tex=True), fresh(accel, tex=True, normals=True)
    assert smooth[:2] != textured[:2] and smooth[2]["triangles"] == S.n and smooth[2]["smooth_triangles"] > 0
    _upload(ctx, S, accel, tex=True, normals=True)
    ctx.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
    ctx.upload_textures(sc.tex_rgba, sc.tex_desc, sc.mat_tex, sc.tri_uv)
    assert _snap(ctx) == textured
    ctx.upload_vertex_normals(S.normals)
    assert _snap(ctx) == smooth


# ---- (d) a refused texture upload -------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_refused_texture_upload_leaves_no_textures(ctx, pkg, S, fresh, accel):
    sc = S.sc
    _upload(ctx, S, accel, tex=True, opacity=True)
    bad = sc.mat_tex.copy()
    bad[1, 0] = len(sc.tex_desc)
    _refused(pkg, lambda: ctx.upload_textures(sc.tex_rgba, sc.tex_desc, bad, sc.tri_uv), ERR_INVALID, "does not exist")
    snap = _snap(ctx)
    assert snap == fresh(accel) and snap[3] == NO_OPACITY


# ---- (e) texture tables of another soup -------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_texture_tables_of_another_soup_are_refused(ctx, pkg, S, accel):
    sc = S.sc
    _upload(ctx, S, accel, tex=True)
    m = S.n - 1  # one triangle fewer; the textures stay
    ctx.upload_triangles(np.asarray(sc.xs)[:m], np.asarray(sc.ys)[:m], np.asarray(sc.zs)[:m], sc.mat_id[:m])
    ctx.upload_vertex_normals(S.normals[:m])
    at = ([0, 27], [0.2, 0.3], [0.25, 0.1])
    rd = [[0, 1, 0], [0, 1, 0]]
    mismatch = "texture tables do not match"
    calls = {
        "render": (lambda: ctx.render(1), mismatch),
        "render_aovs": (lambda: ctx.render_aovs(1), mismatch),
        "test_material": (lambda: ctx.test_material(*at, [[0, 0, 1], [0, 0, 1]]), mismatch),
        # (this probe names the same mismatch in words of its own)
        "test_shading_normal": (lambda: ctx.test_shading_normal(*at, rd, mapped=True), "textures (matching the uploaded BSDFs / triangles) first"),
        "test_texture_filter": (lambda: ctx.test_texture_filter(*at, [0, 1]), "dmt_test_texture_filter"),
    }
    for name, (call, needle) in calls.items():
        _refused(pkg, call, ERR_STATE, needle)
    ctx.upload_textures(sc.tex_rgba, sc.tex_desc, sc.mat_tex, sc.tri_uv[:m])
    for name, (call, _) in calls.items():
        call()
    ctx.sync()


# ---- (f) the first-hit kernel variants --------------------------------------------------------------------------
VARIANTS = {"none": dict(tex=True), "vertex normals": dict(tex=True, normals=True), "motion": dict(), "opacity": dict(tex=True, opacity=True)}


# (motion: brute force only -- the logged path is traced without a tree)
@pytest.mark.parametrize("variant,accel", [(v, a) for v in VARIANTS for a in (0, 1) if (v, a) != ("motion", 1)])
def test_first_hit_variants(ctx, pkg, S, variant, accel):
    _upload(ctx, S, accel, **VARIANTS[variant])
    if variant == "motion":
        ctx.set_motion(*S.key1)
    ctx.render_aovs(1)
    ctx.sync()
    surface = ctx.download_aov_surface()
    on_card = np.argwhere((surface[..., 3] == 1) & (surface[..., 0] >= 26))
    assert len(on_card) > 0
    py, px = (int(v) for v in on_card[len(on_card) // 2])
    s = 2
    rec, L = ctx.test_trace_log(px, py, s)
    assert rec.shape[0] >= 1
    want = ctx.test_trace_samples([px], [py], [s])[0]
    assert L.tobytes() == want.tobytes(), (L, want)


@pytest.mark.parametrize("accel", [0, 1])
def test_first_hit_variants_do_not_combine(ctx, pkg, S, accel):
    sc = S.sc

    def both_refuse(needle):
        _refused(pkg, lambda: ctx.render_aovs(1), ERR_STATE, "dmt_render_aovs", needle)
        _refused(pkg, lambda: ctx.test_trace_log(16, 16, 0), ERR_STATE, "dmt_test_trace_log", needle)
    _upload(ctx, S, accel, normals=True)
    ctx.set_motion(*S.key1)
    both_refuse("vertex normals")
    ctx.clear_vertex_normals()
    ctx.upload_textures(sc.tex_rgba, sc.tex_desc, sc.mat_tex, sc.tri_uv)
    ctx.upload_opacity(sc.mat_opacity, 0.5)
    both_refuse("opacity")           # opacity + motion
    ctx.clear_motion()
    ctx.upload_vertex_normals(S.normals)
    both_refuse("opacity")           # opacity + normals
    ctx.clear_vertex_normals()
    ctx.render_aovs(1)
    ctx.test_trace_log(16, 16, 0)
    ctx.sync()
