"""First-hit texture filtering on the GPU (DMT_TEXFILTER_REFERENCE): the device lookup against the numpy
restatement (texfilter_ref.py), the eight filtering kernel rows against the single-sample test kernel, the film
invariants with the filter on, that it filters, and the reference's textured teapot."""
import numpy as np
import pytest

import texfilter_ref as R
from conftest import GOLDEN
from test_kernel_rows_gpu import _blend_scene
from test_parity_gpu import _textured_cornell

pytestmark = pytest.mark.gpu

REF = 1  # DMT_TEXFILTER_REFERENCE


def _quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def _checker_scene(O, res=64, spp_field=4, minify=False):
    """The Cornell box's materials, light and camera (at the origin, looking down +y) over large planes textured with a
    256^2 checker of 1-texel cells.  A camera-space tangent frame is built per hit from the camera's smallest pixel
    differentials in an arbitrary frame, so a UV derivative is only near 0 when a UV axis barely varies: the floor
    (u along the depth axis, v ~ 1e-7 x) and the wall (v along x) reach EWA, the far floor the [fix 4] cap, the rotated
    quad (both UV axes scaled alike) trilinear.  minify: the floor with u = 8 x, v = 8 y instead."""
    sc = O.cornell_box(res, res)
    tris, uvs = [], []
    for t in _quad((-40, 3, -2), (40, 3, -2), (40, 120, -2), (-40, 120, -2)):
        tris.append(t)
        uvs.append([c for p in t for c in ((p[0] * 8, p[1] * 8) if minify else (p[1] * 2, p[0] * 1e-7))])
    for t in _quad((-30, 30, -2), (-5, 30, -2), (-5, 30, 20), (-30, 30, 20)):
        tris.append(t)
        uvs.append([c for p in t for c in (p[2] * 1e-7, p[0] / 1.5)])
    ca, sa = np.cos(0.52), np.sin(0.52)
    for t in _quad((5, 25, -2), (30, 25, -2), (30, 25, 20), (5, 25, 20)):
        tris.append(t)
        uvs.append([c for p in t for c in ((ca * p[0] - sa * p[2]) / 5, (sa * p[0] + ca * p[2]) / 5)])
    P = np.array(tris, np.float32)
    n = P.shape[0]
    xs, ys, zs = (np.zeros((n, 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = P[:, :, 0], P[:, :, 1], P[:, :, 2]
    s2 = O.Scene(xs, ys, zs, np.zeros(n, np.uint32), sc.bsdfs, sc.lights, sc.inf_lights, sc.camera)
    s2.camera[32:36] = np.array([spp_field], np.int32).view(np.uint8)
    yy, xx = np.mgrid[0:256, 0:256]
    c = (((xx + yy) % 2) * 255).astype(np.uint8)
    img = np.stack([c, c, c, np.full_like(c, 255)], -1)
    none = 0xFFFFFFFF
    mt = np.full((sc.bsdfs.shape[0], 4), none, np.uint32)
    mt[:, 3] = np.float32(1).view(np.uint32)
    mt[0, 0] = 0   # material 0 (Oren-Nayar): the checker as albedo
    s2.set_textures(img.reshape(-1, 4), np.array([[0, 256, 256]], np.int32), mt, np.array(uvs, np.float32))
    return s2, img, P


def _reset(renderer):
    renderer.set_texture_filter(0)
    renderer.set_accel(0)
    renderer.clear_envmap()
    renderer.upload_textures(None, None, None, None)


def _render(renderer, spp, offset=0):
    renderer.film_clear()
    renderer.render(spp, sample_offset=offset)
    renderer.sync()
    return renderer.download_film()


def _probe_scene(O, n_ewa=2000, n_tri=1000, seed=11):
    """Probes of the device lookup.  A UV derivative is only near 0 (the EWA branch) when a UV gradient is orthogonal to
    dpdx or dpdy, whose directions come from the camera's differentials in an arbitrary frame: so each EWA probe sits on a
    small floor triangle of its own whose u gradient is orthogonal to the restated dpdx at the probe, with gradients
    scaled to 1..200 texels per pixel along the other axes (the far, flat ones reach the [fix 4] cap).  Trilinear probes
    lie on the rotated quad of _checker_scene.  Returns (scene, [256^2 checker, 4096 x 16 checker], P, tri, bu, bv, tex)."""
    base, img, P0 = _checker_scene(O)
    fp = R.footprint(R.parse_camera(base.camera))
    rng = np.random.default_rng(seed)
    y = np.exp(rng.uniform(np.log(4.0), np.log(300.0), n_ewa))
    x = rng.uniform(-0.3, 0.3, n_ewa) * y
    p = np.stack([x, y, np.full(n_ewa, -2.0)], -1).astype(np.float32)
    dpdx, dpdy = R.hit_dpdxy(fp, p, np.tile(np.array([0, 0, 1], np.float32), (n_ewa, 1)))
    dx, dy = dpdx[:, :2].astype(np.float64), dpdy[:, :2].astype(np.float64)
    perp = np.stack([-dx[:, 1], dx[:, 0]], -1) / np.linalg.norm(dx, axis=1)[:, None]
    along = dx / np.linalg.norm(dx, axis=1)[:, None]
    ratio = np.abs((perp * dy).sum(1)) / np.linalg.norm(dx, axis=1)
    # |gu| |dpdx| <= 0.05 keeps dudx (~1e-6 of it in float) below FLT_EPSILON; two thirds of the probes use a 4096 x 16 checker,
    # on which the same bound allows u footprints of ~50-200 texels against ~1 in v: the ellipses that reach the cap
    wide = np.arange(n_ewa) >= n_ewa // 3
    W, H = np.where(wide, 4096.0, 256.0), np.where(wide, 16.0, 256.0)
    hi = np.clip(0.05 * W * ratio, 2.0, 200.0)
    a = np.exp(rng.uniform(np.where(wide, np.log(hi) - 0.5, 0.0), np.log(hi)))     # texels of u per pixel along y
    b = np.exp(rng.uniform(np.where(wide, np.log(0.5), 0.0), np.where(wide, np.log(2.0), np.log(20.0))))  # v along x
    gu = perp * (a / (W * np.abs((perp * dy).sum(1))))[:, None]
    gv = along * (b / (H * np.linalg.norm(dx, axis=1)))[:, None]
    e = (0.25 * y)[:, None]   # large: float positions and UVs then carry the UV gradients to ~1e-7
    offs = np.stack([np.concatenate([-e, -e], 1), np.concatenate([e, -e], 1), np.concatenate([0 * e, e], 1)], 1)   # n, 3, 2
    tris = np.concatenate([p[:, None, :2] + offs, np.full((n_ewa, 3, 1), -2.0)], 2)
    uc, vc = rng.uniform(0, 1, n_ewa), rng.uniform(0, 1, n_ewa)
    uv = np.stack([(offs * gu[:, None]).sum(2) + uc[:, None], (offs * gv[:, None]).sum(2) + vc[:, None]], 2).reshape(n_ewa, 6)
    Pq = P0[4:6]   # the rotated quad
    tri_q = rng.integers(0, 2, n_tri)
    P = np.concatenate([tris.astype(np.float32), Pq]).astype(np.float32)
    uvs = np.concatenate([uv.astype(np.float32), base.tri_uv[4:6]])
    n = P.shape[0]
    xs, ys, zs = (np.zeros((n, 4), np.float32) for _ in range(3))
    xs[:, :3], ys[:, :3], zs[:, :3] = P[:, :, 0], P[:, :, 1], P[:, :, 2]
    sc = O.Scene(xs, ys, zs, np.zeros(n, np.uint32), base.bsdfs, base.lights, base.inf_lights, base.camera)
    yy, xx = np.mgrid[0:16, 0:4096]
    c = (((xx + yy) % 2) * 255).astype(np.uint8)
    img2 = np.stack([c, c, c, np.full_like(c, 255)], -1)
    sc.set_textures(np.concatenate([base.tex_rgba, img2.reshape(-1, 4)]), np.array([[0, 256, 256], [65536, 4096, 16]], np.int32),
                    base.mat_tex, uvs)
    tri = np.concatenate([np.arange(n_ewa), n_ewa + tri_q]).astype(np.int32)
    tex = np.concatenate([wide.astype(np.int32), np.zeros(n_tri, np.int32)])
    bu = np.concatenate([np.full(n_ewa, 0.25), rng.uniform(0.02, 0.96, n_tri)]).astype(np.float32)
    bv = np.concatenate([np.full(n_ewa, 0.5), rng.uniform(0.02, 0.98, n_tri) * (1 - bu[n_ewa:])]).astype(np.float32)
    return sc, [img, img2], P, tri, bu, bv, tex


def test_probe_equals_restatement(renderer, O):
    sc, imgs, P, tri, bu, bv, tex = _probe_scene(O)
    N = tri.shape[0]
    fp = R.footprint(R.parse_camera(sc.camera))
    chains = [R.mip_chain(im) for im in imgs]
    p0, p1, p2 = P[tri, 0], P[tri, 1], P[tri, 2]
    p = p0 + bu[:, None] * (p1 - p0) + bv[:, None] * (p2 - p0)
    ng = np.cross(p2 - p0, p1 - p0)
    ng = (ng / np.linalg.norm(ng, axis=1)[:, None]).astype(np.float32)
    uv = sc.tri_uv[tri]
    d, cross_margin = R.hit_differentials(fp, p, ng, p0, p1, p2, uv)
    # the footprint must not collapse under the 1e-6 cross-product test (it does at small scene scales)
    assert (cross_margin > 0.5).all() and np.all(np.any(d != 0, axis=1))
    ref = []
    for i in range(N):
        w0 = np.float32(1) - bu[i] - bv[i]
        s = w0 * uv[i, 0] + bu[i] * uv[i, 2] + bv[i] * uv[i, 4]
        t = w0 * uv[i, 1] + bu[i] * uv[i, 3] + bv[i] * uv[i, 5]
        ref.append(R.lookup(chains[tex[i]], s, t, d[i]))
    renderer.upload_scene(sc)
    try:
        rgb, branch, lod = renderer.test_texture_filter(tri, bu, bv, tex, 0)
        rgb1, branch1, lod1 = renderer.test_texture_filter(tri, bu, bv, tex, 1)
    finally:
        _reset(renderer)
    rb = np.array([r["branch"] for r in ref])
    margin = np.array([r["margin"] for r in ref])
    keep = margin > 1e-3   # probes away from the branch and level thresholds
    assert keep.mean() > 0.9, keep.mean()
    for b in (1, 2, 3):
        assert ((rb == b) & keep).sum() >= 100, (b, np.bincount(rb))
    rl = np.array([r["lod"] for r in ref])
    bad = np.nonzero(keep & (branch != rb))[0]
    assert bad.size == 0, [(int(i), int(branch[i]), int(rb[i]), float(lod[i]), float(rl[i]), float(margin[i]), d[i].tolist()) for i in bad[:8]]
    assert np.array_equal(np.floor(lod[keep]), np.floor(rl[keep]))
    assert np.abs(lod[keep] - rl[keep]).max() <= 1e-5
    rr = np.array([r["rgb"] for r in ref])
    err = np.abs(rgb - rr).max(axis=1)
    assert err[keep & (rb == 1)].max() <= 2e-5
    # EWA weights come from a 128-entry table indexed by r2, and a box of hundreds of texels almost always holds one whose
    # r2 lies within float rounding of a bin edge (rgb_margin): such a texel may take the neighbouring weight on one side,
    # which moves the result by (weight step) / (sum of weights).  Most probes agree to 2e-5; none by more than that bound.
    ewa = keep & (rb >= 2)
    assert np.quantile(err[ewa], 0.9) <= 2e-5 and err[ewa].max() <= 2e-3, (np.quantile(err[ewa], [0.5, 0.9, 1.0]))
    # later hits: the level-0 lookup, the same device function the level-0 rows run
    assert (branch1 == 0).all() and (lod1 == 0).all()
    lvl0 = np.array([R.bilinear(chains[k][0], r0, r1) for k, r0, r1 in zip(tex,
        (np.float32(1) - bu - bv) * uv[:, 0] + bu * uv[:, 2] + bv * uv[:, 4],
        (np.float32(1) - bu - bv) * uv[:, 1] + bu * uv[:, 3] + bv * uv[:, 5])])
    assert np.abs(rgb1 - lvl0).max() <= 1e-6
    zero = branch == 0
    assert np.array_equal(rgb[zero], rgb1[zero])


@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("env", [False, True])
@pytest.mark.parametrize("kind", ["tex", "blend"])
def test_filter_rows_trace_samples_equal_render(renderer, pkg, O, tmp_path, kind, env, accel):
    """The filtering rows' version of test_trace_samples_run_the_render_kernel: a 1-spp render at sample s into a cleared
    film holds each sample itself; the test kernel's radiance of (pixel, s) must equal it exactly."""
    sc = _blend_scene(pkg, tmp_path) if kind == "blend" else _textured_cornell(O, pkg, 32)
    s = 5
    renderer.upload_area_lights([], np.zeros((0, 3), np.float32))
    renderer.upload_scene(sc)
    if env:
        renderer.upload_envmap(pkg.host_scene.synthetic_sky(16))
    else:
        renderer.clear_envmap()
    renderer.set_limits(6)
    renderer.set_accel(accel)
    renderer.set_partition(0, 1)
    try:
        renderer.set_texture_filter(REF)
        mean, m2 = _render(renderer, 1, s)
        idx = np.random.default_rng(3).choice(renderer.width * renderer.height, 64, replace=False)
        px, py = (idx % renderer.width).astype(np.int32), (idx // renderer.width).astype(np.int32)
        L = renderer.test_trace_samples(px, py, np.full(64, s, np.int32))
    finally:
        _reset(renderer)
    assert np.array_equal(m2[py, px, 3], np.ones(64, np.float32))
    assert np.isfinite(L).all() and L.max() > 0
    assert np.array_equal(L, mean[py, px, :3]), np.abs(L - mean[py, px, :3]).max()


@pytest.mark.parametrize("scene", ["textured_cornell", "checker"])
def test_filter_invariants(renderer, pkg, O, scene):
    sc = _textured_cornell(O, pkg, 48) if scene == "textured_cornell" else _checker_scene(O, 48, 32)[0]
    if scene == "textured_cornell":
        sc.camera[32:36] = np.array([32], np.int32).view(np.uint8)
    renderer.upload_scene(sc)
    renderer.set_limits(4)
    renderer.set_partition(0, 1)
    try:
        before, _ = _render(renderer, 8)
        renderer.set_texture_filter(REF)
        brute, brute_m2 = _render(renderer, 32)
        renderer.film_clear()
        renderer.render(16, sample_offset=0)
        renderer.render(16, sample_offset=16)
        renderer.sync()
        chunked, chunked_m2 = renderer.download_film()
        renderer.set_accel(1)
        bvh, bvh_m2 = _render(renderer, 32)
        renderer.set_accel(0)
        renderer.set_texture_filter(0)
        after, _ = _render(renderer, 8)
    finally:
        _reset(renderer)
    assert np.isfinite(brute).all()
    assert np.array_equal(bvh, brute) and np.array_equal(bvh_m2, brute_m2)
    assert np.array_equal(chunked, brute) and np.array_equal(chunked_m2, brute_m2)
    assert np.array_equal(after, before)
    assert not np.array_equal(brute[..., :3], _level0_film(renderer, sc))


def _level0_film(renderer, sc):
    renderer.upload_scene(sc)
    renderer.set_limits(4)
    try:
        mean, _ = _render(renderer, 32)
    finally:
        _reset(renderer)
    return mean[..., :3]


def test_filter_reduces_texture_variance(renderer, O):
    """A minified checker lit by one point light (the Cornell spot as a point light, no environment), max depth 1: the only
    per-sample variation is the texture lookup (and the smooth 1 / d^2 falloff over a pixel)."""
    sc, _, _ = _checker_scene(O, 64, 16, minify=True)
    lights = sc.lights.copy()
    lights.view(np.uint16).reshape(-1, 16)[0, 3] = 0   # light type (high half of word 1): spot -> point
    sc.lights, sc.inf_lights = lights, np.zeros((0, 32), np.uint8)
    renderer.upload_scene(sc)
    renderer.set_limits(1)
    renderer.set_partition(0, 1)
    try:
        m0, v0 = _render(renderer, 16)
        renderer.set_texture_filter(REF)
        m1, v1 = _render(renderer, 16)
    finally:
        _reset(renderer)
    region = (slice(36, 46), slice(0, 64))   # lit floor rows where the footprint is live and the level is 2 or more
    a, b = m0[region][..., :3].mean(), m1[region][..., :3].mean()
    assert a > 0 and abs(b - a) <= 0.05 * a, (a, b)
    var0 = (v0[region][..., :3] / (v0[region][..., 3:4] - 1)).mean()
    var1 = (v1[region][..., :3] / (v1[region][..., 3:4] - 1)).mean()
    assert var1 < 0.25 * var0, (var0, var1)


def test_reference_teapot_with_filter(renderer, pkg, O):
    """scene_test.json's teapot at 256^2, 32 spp: the filtered film differs from the level-0 film only where the camera
    ray's first hit is textured.  Elsewhere the paths are the same numbers (the filter draws no random numbers, and later
    hits use level 0 in both modes), so the films agree bit for bit there."""
    hs = pkg.host_scene.load_json(GOLDEN / "scene_test" / "scene_test.json")
    sc = O.Scene(hs.xs, hs.ys, hs.zs, hs.mat_id, hs.bsdfs, hs.lights, hs.inf_lights, hs.camera)
    sc.set_envmap(hs.env_rgb)
    sc.set_textures(hs.tex_rgba, hs.tex_desc, hs.mat_tex, hs.tri_uv)
    sc.set_resolution(256, 256)
    sc.camera[32:36] = np.array([32], np.int32).view(np.uint8)
    renderer.upload_scene(sc)
    renderer.set_limits(hs.max_depth)
    renderer.set_accel(1)
    renderer.set_partition(0, 1)
    cam = R.parse_camera(sc.camera)
    # first hits of a 5x5 grid per pixel (corners included): a pixel is "untextured" when none of them is textured
    g = np.linspace(0.0, 1.0, 5)
    yy, xx, gy, gx = np.meshgrid(np.arange(256), np.arange(256), g, g, indexing="ij")
    cfr, rfc = (m.astype(np.float64) for m in R.camera_matrices(cam))
    fx, fy = (xx + gx).ravel(), (yy + gy).ravel()
    pc = np.stack([cfr[0] * fx + cfr[12], cfr[5] * fy + cfr[13], np.full_like(fx, cfr[14])], -1)
    pc /= np.linalg.norm(pc, axis=1)[:, None]
    d = pc @ np.stack([rfc[0:3], rfc[4:7], rfc[8:11]])
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.tile(rfc[12:15], (d.shape[0], 1))
    try:
        renderer.set_texture_filter(0)
        m0, _ = _render(renderer, 32)
        renderer.kernel_time(reset=True)
        renderer.set_texture_filter(REF)
        m1, _ = _render(renderer, 32)
        tri, _ = renderer.test_closest_hit(np.array(o, np.float32), np.array(d, np.float32))
    finally:
        _reset(renderer)
    mt = np.asarray(hs.mat_tex, np.uint32).reshape(-1, 4)
    textured_mat = (mt[:, :3] != 0xFFFFFFFF).any(axis=1)
    textured_mat = textured_mat | np.concatenate([textured_mat[1:], [False]])   # a blend pair's metallic map sits in its second row
    mid = np.asarray(hs.mat_id, np.uint32)
    hit_tex = np.where(tri >= 0, textured_mat[mid[np.maximum(tri, 0)]], False).reshape(256, 256, 25).any(axis=2)
    assert np.isfinite(m1).all()
    plain = ~hit_tex
    assert plain.sum() > 1000 and hit_tex.sum() > 1000
    assert np.array_equal(m1[plain], m0[plain]), np.abs(m1[plain] - m0[plain]).max()
    assert not np.array_equal(m1[hit_tex], m0[hit_tex])
