"""GPU tests of smooth shading: the device's shading normal against tests/vnormal_ref.py, the *_vn kernel
rows, films against the oracle, the feature pass, and the states the feature refuses."""
import numpy as np
import pytest

import vnormal_ref as V
from conftest import GOLDEN, film_rmse
from test_parity_gpu import REL, RMSE_TOL, _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _film(renderer, spp, offset=0):
    renderer.film_clear()
    renderer.render(spp, sample_offset=offset)
    renderer.sync()
    return renderer.download_film()


def _reset(renderer):
    renderer.clear_vertex_normals()
    renderer.set_accel(0)
    renderer.clear_envmap()
    renderer.upload_textures(None, None, None, None)
    renderer.upload_area_lights([], np.zeros((0, 3), np.float32))


@pytest.fixture(scope="module")
def sphere(O):
    """The Cornell box (flat) with the radial-normal icosphere, plus two triangles in free space: one whose three normals
    sum to zero (in the plane of the face, 120 degrees apart) and one whose normals all point against the stored face normal
    (its normals at vertices 1 and 2 are equal, so that weights bu = -bv cancel them exactly)."""
    sc, n9 = V.sphere_scene(O, 64)
    extra = np.array([[[1.2, 1.0, 1.2], [1.6, 1.0, 1.2], [1.4, 1.0, 1.6]], [[-1.6, 1.0, 1.2], [-1.2, 1.0, 1.2], [-1.4, 1.0, 1.6]]], np.float32)
    add = lambda old, ax: np.concatenate([old, np.concatenate([extra[:, :, ax], np.zeros((2, 1), np.float32)], 1)])
    sc2 = O.Scene(add(sc.xs, 0), add(sc.ys, 1), add(sc.zs, 2), np.concatenate([sc.mat_id, np.full(2, 1, np.uint32)]), sc.bsdfs, sc.lights,
                  sc.inf_lights, sc.camera)
    fn, _ = V.face_normals(sc2.xs, sc2.ys, sc2.zs)
    c, s = np.cos(2 * np.pi / 3), np.sin(2 * np.pi / 3)
    zero_sum = np.array([[1, 0, 0], [c, 0, s], [c, 0, -s]], np.float32)  # the face lies in y = 1
    against = np.tile(-fn[-1], (3, 1)) + np.array([[0.1, 0, 0], [0, 0, 0.1], [0, 0, 0.1]], np.float32)  # n1 == n2: identical words
    n9 = np.concatenate([n9, zero_sum.reshape(1, 9), against.reshape(1, 9).astype(np.float32)])
    return sc2, n9.astype(np.float32), fn


# ---- 1. the probe against the restatement ---------------------------------------------------------------------------
def test_shading_normal_matches_the_restatement(renderer, O, sphere):
    """4 096 cases over all triangles.  Budget of a smooth case whose sum has length |n|: the inputs are unit vectors, three
    products and two sums (about five roundings of 2^-24 on values <= 1) leave an absolute error near 3e-7 in the sum, the
    normalisation divides it by |n| and adds one more rounding -- 1e-6 per component for |n| >= 1/2, which is every case
    here: the sphere's neighbouring normals are 20 degrees apart, and the zero-sum triangle is probed at its corners
    (|n| = 1) and along its edges only up to |n| = 1/2.  At that triangle's centroid the 16-bit words leave a sum near 1e-5,
    well above the 1e-12 fall-back in l2 and ill-conditioned: there the test asks for a unit vector in ngFacing's hemisphere.
    The short-sum fall-back itself is reached exactly: on the triangle with n1 == n2 (identical words), bu = +-2^66 and
    bv = -bu give w0 = fl(fl(1 - bu) - bv) = 0 and products that are exact whether or not they are fused, so the sum is
    exactly zero.  The non-finite fall-back is reached through NaN and infinite bu."""
    sc, n9, fn = sphere
    rng = np.random.default_rng(7)
    ntri = sc.tri_count
    n = 4096
    tri = rng.integers(0, ntri, n).astype(np.int32)
    tri[:ntri] = np.arange(ntri)                      # every triangle at least once
    bu, bv = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    over = bu + bv > 1
    bu[over], bv[over] = 1 - bu[over], 1 - bv[over]
    k = np.arange(n)
    bu[k % 8 == 1], bv[k % 8 == 2] = 0, 0             # the edges bu = 0 and bv = 0
    e = k % 8 == 3
    bv[e] = np.float32(1) - bu[e]                     # the edge bu + bv = 1
    for j, (a, b) in enumerate([(0, 0), (1, 0), (0, 1)]):
        c = k % 16 == 4 + 4 * j
        bu[c], bv[c] = a, b                           # the corners
    zs, ag = ntri - 2, ntri - 1
    tri[tri == zs] = ag                               # the zero-sum triangle: only at the well-conditioned points below
    special = np.arange(ntri, ntri + 64)              # the two special triangles, 32 cases each
    tri[special[:32]], tri[special[32:]] = zs, ag
    corners = np.array([(0, 0), (1, 0), (0, 1)], np.float32)
    t = np.linspace(0, 1, 9, dtype=np.float32)[:, None]
    edge = np.concatenate([corners[[0]] * (1 - t * 0.33) + corners[[1]] * t * 0.33,   # along the edges, away from their middles:
                           corners[[1]] * (1 - t * 0.33) + corners[[2]] * t * 0.33,   # |n| >= 0.57 for normals 120 degrees apart
                           corners[[2]] * (1 - t * 0.33) + corners[[0]] * t * 0.33])
    zs_uv = np.concatenate([corners, edge, [[1 / 3, 1 / 3]], [[1 / 3, 1 / 3]]]).astype(np.float32)[:32]
    bu[special[:32]], bv[special[:32]] = zs_uv[:, 0], zs_uv[:, 1]
    centroid = np.zeros(n, bool)
    centroid[special[30:32]] = True
    rd = rng.standard_normal((n, 3)).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    grazing = np.abs((rd * fn[tri]).sum(1)) < 0.05
    rd[grazing] = fn[tri[grazing]]                    # (no case where the sign of dot(rd, n) hangs on a rounding)
    side = np.where(k % 2 == 0, -1.0, 1.0).astype(np.float32)[:, None]                # both sides of every face
    rd = (rd * np.sign((rd * fn[tri]).sum(1, keepdims=True)) * side).astype(np.float32)
    # the second fall-back: a sum whose squared length is not finite
    inf_cases = special[32:36]
    bu[inf_cases] = [np.nan, np.inf, -np.inf, np.nan]
    # the first fall-back: a sum of squared length below 1e-12 (here exactly zero)
    zero_cases = special[36:40]
    big = np.float32(2.0 ** 66)
    bu[zero_cases], bv[zero_cases] = [big, -big, big, -big], [-big, big, -big, big]
    renderer.upload_scene(sc)
    try:
        renderer.upload_vertex_normals(n9)
        info = renderer.vertex_normals_info()
        got = renderer.test_shading_normal(tri, bu, bv, rd)
    finally:
        _reset(renderer)
    assert info == {"triangles": ntri, "smooth_triangles": 82}
    words, smooth = V.pack_records(n9)
    ngf, d = V.facing_normal(fn[tri], rd)
    assert (d > 0).sum() == n // 2 and (d < 0).sum() == n // 2
    ref, fallback, l2 = V.shading_normal(O, words, smooth, tri, bu, bv, ngf)
    assert fallback[~smooth[tri]].all() and fallback[inf_cases].all() and fallback[zero_cases].all() and (l2[zero_cases] == 0).all()
    usual = np.ones(n, bool)
    usual[inf_cases], usual[zero_cases] = False, False
    assert not fallback[smooth[tri] & usual].any()
    assert np.array_equal(got[fallback].view(np.uint32), ngf[fallback].view(np.uint32))   # ngFacing bit for bit
    ok = ~fallback & ~centroid
    assert l2[ok].min() >= 0.25
    err = np.abs(got[ok].astype(np.float64) - ref[ok])
    print("smooth cases", int(ok.sum()), "max |device - restatement|", err.max(), "shortest sum", np.sqrt(l2[ok].min()))
    assert err.max() < 1e-6, err.max()
    # the face whose normals all point against it: the result is the interpolated normal, negated into ngFacing's hemisphere
    a = ok & (tri == ag)
    assert a.sum() >= 24 and ((got[a] * ngf[a]).sum(1) > 0.9).all()
    c = got[centroid].astype(np.float64)
    assert np.abs(np.linalg.norm(c, axis=1) - 1).max() < 1e-6 and ((c * ngf[centroid]).sum(1) >= 0).all()


# ---- 2. each new row is the kernel that renders ---------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("row", ["plain", "env", "tex", "env_tex"])
def test_each_vn_row_is_the_kernel_that_renders(renderer, pkg, O, row, accel):
    """As test_kernel_rows_gpu: a 1-spp render at sample 5 into a cleared film equals dmt_test_trace_samples exactly."""
    if "tex" in row:
        sc = _textured_cornell(O, pkg, 32, env="env" in row)
    else:
        sc = O.cornell_box(32, 32)
        if row == "env":
            sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    n9 = pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0)  # the two octahedra become round, the walls' corners lean
    s = 5
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_accel(accel)
    renderer.set_partition(0, 1)
    try:
        flat, _ = _film(renderer, 1, s)
        renderer.upload_vertex_normals(n9)
        info = renderer.vertex_normals_info()
        mean, m2 = _film(renderer, 1, s)
        idx = np.random.default_rng(3).choice(renderer.width * renderer.height, 64, replace=False)
        px, py = (idx % renderer.width).astype(np.int32), (idx // renderer.width).astype(np.int32)
        L = renderer.test_trace_samples(px, py, np.full(64, s, np.int32))
    finally:
        _reset(renderer)
    assert info == {"triangles": sc.tri_count, "smooth_triangles": sc.tri_count}
    assert np.array_equal(m2[py, px, 3], np.ones(64, np.float32))
    assert np.isfinite(L).all() and L.max() > 0
    assert np.array_equal(L, mean[py, px, :3]), np.abs(L - mean[py, px, :3]).max()
    assert not np.array_equal(mean, flat)  # and it is not the parent row's kernel


def test_trace_log_and_adaptive_rounds_shade_with_the_vn_row(renderer, pkg, O):
    sc = O.cornell_box(32, 32)
    n9 = pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0)
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_partition(0, 1)
    try:
        renderer.upload_vertex_normals(n9)
        px, py, ss = np.array([5, 16, 27, 9], np.int32), np.array([20, 16, 8, 29], np.int32), np.array([0, 3, 1, 2], np.int32)
        L = renderer.test_trace_samples(px, py, ss)
        logs = np.array([renderer.test_trace_log(int(x), int(y), int(s))[1] for x, y, s in zip(px, py, ss)])
        renderer.film_clear()
        for k in range(2):  # an adaptive film equals the uniform film of the same rounds
            renderer.render(2, sample_offset=2 * k)
        renderer.sync()
        uniform, um2 = renderer.download_film()
        renderer.film_clear()
        renderer.render_adaptive(0.0, 4, 2, min_spp=4)  # (min_spp = max_spp: no pixel stops early, not even one without variance)
        renderer.sync()
        adaptive, am2 = renderer.download_film()
    finally:
        _reset(renderer)
    assert np.array_equal(logs, L)
    assert np.array_equal(adaptive, uniform) and np.array_equal(am2, um2)


# ---- 3. normals equal to the face normals change nothing visible, against the oracle ----------------------------------
@pytest.fixture(scope="module")
def plain_films(O, pkg):
    out = {}
    for env in (False, True):
        sc = O.cornell_box(64, 64)
        if env:
            sc.set_envmap(pkg.host_scene.synthetic_sky(16))
        out[env] = O.render(sc, 32, max_depth=6, threads=8)[:2]
    return out


@pytest.mark.parametrize("accel, env", [(0, False), (1, False), (0, True), (1, True)])
def test_face_normals_as_vertex_normals_match_the_oracle(renderer, pkg, O, plain_films, accel, env):
    """Cornell 64^2 x 32 spp x depth 6 with n0 = n1 = n2 = the fp32 face normal: the only differences from the flat kernels
    are the 16-bit octahedral round trip and the normalisation of the sum."""
    sc = O.cornell_box(64, 64)
    if env:
        sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    fn, ok = V.face_normals(sc.xs, sc.ys, sc.zs)
    assert ok.all()
    back = V.decode_words(O, V.octa_words(fn))
    moved = V.angle_between(back, fn)
    assert moved.max() < 1e-4, moved.max()  # the condition the bound rests on
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_accel(accel)
    renderer.set_partition(0, 1)
    try:
        renderer.upload_vertex_normals(np.tile(fn, (1, 3)))
        mean, m2 = _film(renderer, 32)
    finally:
        _reset(renderer)
    om, om2 = plain_films[env]
    scale = float(om[..., :3].mean())
    rmse = film_rmse(mean, om)
    print("round trip moves the normals by at most", moved.max(), "rad; film RMSE", rmse, "scale", scale)
    assert np.array_equal(m2[..., 3], om2[..., 3]) and np.isfinite(mean).all()
    assert rmse < RMSE_TOL * max(1.0, scale), rmse


# ---- 4. tilted normals, against the oracle's normal-map path ------------------------------------------------------------
@pytest.fixture(scope="module")
def tilted(O):
    """Scene A (every material Oren-Nayar under one 1x1 normal map), its oracle film, the plain film, and the vertex normals
    of scene B: per triangle the world-space normal the map produces."""
    def opaque():
        sc = O.cornell_box(64, 64)
        cols = [(0.7, 0.3, 0.2), (0.2, 0.6, 0.7), (0.73, 0.73, 0.73), (0.73, 0.73, 0.73), (0.73, 0.73, 0.73), (0.63, 0.06, 0.06), (0.14, 0.45, 0.09)]
        sc.bsdfs = np.stack([O.make_oren_nayar(cols[i % len(cols)], 0.3) for i in range(sc.bsdfs.shape[0])])
        return sc
    A, B = opaque(), opaque()
    mt = np.tile(np.array([NONE, NONE, 0, np.float32(1.0).view(np.uint32)], np.uint32), (A.bsdfs.shape[0], 1))
    A.set_textures(np.array([[178, 96, 230, 255]], np.uint8), np.array([[0, 1, 1]], np.int32), mt, np.zeros((A.tri_count, 6), np.float32))
    fn, _ = V.face_normals(A.xs, A.ys, A.zs)
    # one-sidedness, which decides ngFacing: every logged hit of a triangle sees it from the same side
    side = np.zeros(A.tri_count, np.int32)
    cam = A.camera[12:24].view(np.float32).astype(np.float64)
    rng = np.random.default_rng(11)
    for _ in range(300):
        rec, _L = O.trace_log(A, int(rng.integers(0, 64)), int(rng.integers(0, 64)), int(rng.integers(0, 32)), max_depth=6)
        prev = cam
        for r in rec:
            t = int(r[0])
            if t < 0:
                break
            pos = r[1:4].astype(np.float64)
            sgn = 1 if np.dot(pos - prev, fn[t]) > 0 else -1
            assert side[t] in (0, sgn), ("triangle seen from both sides", t)
            side[t] = sgn
            prev = pos
    assert (side != 0).sum() >= 20
    ngf = np.where((side > 0)[:, None], -fn, fn).astype(np.float32)  # never hit: either sign
    third = np.full(A.tri_count, 1 / 3, np.float32)
    m = O.material_at_hit(A, np.arange(A.tri_count), third, third, ngf)[1]
    assert ((m * ngf).sum(1) > 0.5).all() and ((m * ngf).sum(1) < 0.99).all()  # tilted, within ngFacing's hemisphere
    film_a = O.render(A, 32, max_depth=6, threads=8)[:2]
    film_plain = O.render(B, 32, max_depth=6, threads=8)[0]
    return B, np.tile(m, (1, 3)).astype(np.float32), film_a, film_plain


@pytest.mark.parametrize("accel", [0, 1])
def test_tilted_normals_match_the_oracles_normal_map(renderer, O, tilted, accel):
    B, n9, (om, om2), plain = tilted
    scale = float(om[..., :3].mean())
    assert film_rmse(om, plain) > 5e-3 * scale  # the tilt does change the picture
    renderer.upload_scene(B)
    renderer.set_limits(6)
    renderer.set_accel(accel)
    renderer.set_partition(0, 1)
    try:
        renderer.upload_vertex_normals(n9)
        mean, m2 = _film(renderer, 32)
    finally:
        _reset(renderer)
    rmse = film_rmse(mean, om)
    print("film RMSE of B against the oracle's A", rmse, "A against plain", film_rmse(om, plain), "scale", scale)
    assert np.array_equal(m2[..., 3], om2[..., 3]) and np.isfinite(mean).all()
    assert rmse < RMSE_TOL * max(1.0, scale), rmse


# ---- 5. brute force and BVH are bit-identical -----------------------------------------------------------------------
def test_brute_force_and_bvh_films_are_byte_equal(renderer, sphere):
    sc, n9, _ = sphere
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_partition(0, 1)
    try:
        renderer.upload_vertex_normals(n9)
        films = []
        for accel in (0, 1):
            renderer.set_accel(accel)
            films.append(_film(renderer, 16))
    finally:
        _reset(renderer)
    assert np.isfinite(films[0][0]).all() and films[0][0][..., :3].max() > 0
    assert films[0][0].tobytes() == films[1][0].tobytes() and films[0][1].tobytes() == films[1][1].tobytes()


# ---- 6. a normal map on top of smooth normals -----------------------------------------------------------------------
def test_normal_map_perturbs_the_smooth_normal(renderer, O, sphere):
    """dmt_test_shading_normal_mapped: the existing normal-map formula (the oracle's material_at_hit) taken around the
    interpolated normal, every case within REL and the absolute floor of the project's function-level comparisons
    (test_parity_gpu.close).  The map is one texel, so its lookup is exact at any UV and the comparison is about the frame
    around the smooth normal; lookups and their quantisation are tests/shading_sweep.py's subject."""
    sc0, n9, fn = sphere
    sc = O.Scene(sc0.xs, sc0.ys, sc0.zs, sc0.mat_id, sc0.bsdfs, sc0.lights, sc0.inf_lights, sc0.camera)
    rng = np.random.default_rng(13)
    mt = np.tile(np.array([NONE, NONE, 0, np.float32(1.0).view(np.uint32)], np.uint32), (sc.bsdfs.shape[0], 1))
    sc.set_textures(np.array([[178, 96, 230, 255]], np.uint8), np.array([[0, 1, 1]], np.int32), mt,
                    rng.uniform(-0.5, 2.5, (sc.tri_count, 6)).astype(np.float32))
    n = 1024
    tri = rng.integers(26, 26 + 80, n).astype(np.int32)  # the sphere's triangles
    bu, bv = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    over = bu + bv > 1
    bu[over], bv[over] = 1 - bu[over], 1 - bv[over]
    rd = rng.standard_normal((n, 3)).astype(np.float32)
    renderer.upload_scene(sc)
    try:
        renderer.upload_vertex_normals(n9)
        smooth_ns = renderer.test_shading_normal(tri, bu, bv, rd)
        got = renderer.test_shading_normal(tri, bu, bv, rd, mapped=True)
    finally:
        _reset(renderer)
    words, smooth = V.pack_records(n9)
    ngf, _ = V.facing_normal(fn[tri], rd)
    ref_ns = V.shading_normal(O, words, smooth, tri, bu, bv, ngf)[0].astype(np.float32)
    assert np.abs(smooth_ns - ref_ns).max() < 1e-6
    ref = O.material_at_hit(sc, tri, bu, bv, ref_ns)[1]
    assert np.abs(ref - ref_ns).max() > 0.05  # the map does tilt it
    print("max |device - restatement|", np.abs(got - ref).max())
    assert np.allclose(got, ref, rtol=REL, atol=1e-6), np.abs(got - ref).max()


# ---- 7. the feature pass --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [0, 1])
def test_aov_normal_plane_holds_the_smooth_normal(renderer, sphere, accel):
    sc, n9, _ = sphere
    renderer.upload_scene(sc)
    renderer.set_accel(accel)
    try:
        renderer.render_aovs(1)
        renderer.sync()
        albedo0, normal0, position0 = renderer.download_aovs()
        renderer.upload_vertex_normals(n9)
        renderer.render_aovs(1)
        renderer.sync()
        albedo, normal, position = renderer.download_aovs()
        surface = renderer.download_aov_surface()
        h, w = normal.shape[:2]
        py, px = np.mgrid[0:h, 0:w]
        px, py = px.reshape(-1).astype(np.int32), py.reshape(-1).astype(np.int32)
        o, d = renderer.test_camera_rays(px, py, np.zeros_like(px))
        tri, _t = renderer.test_closest_hit(o, d)
        surf = surface.reshape(-1, 4)
        on = (tri >= 26) & (tri < 26 + 80)
        ns = renderer.test_shading_normal(tri[on], surf[on, 1], surf[on, 2], d[on])
    finally:
        _reset(renderer)
    assert on.sum() > 100 and np.array_equal(surf[on, 0].astype(np.int32), tri[on])
    assert np.abs(normal.reshape(-1, 4)[on, :3] - ns).max() < 1e-6
    assert np.abs(normal.reshape(-1, 4)[on, :3] - normal0.reshape(-1, 4)[on, :3]).max() > 0.05  # round now
    assert albedo.tobytes() == albedo0.tobytes() and position.tobytes() == position0.tobytes()
    off = ~on
    assert np.array_equal(normal.reshape(-1, 4)[off], normal0.reshape(-1, 4)[off])  # flat triangles and misses: as before


# ---- 8. state -------------------------------------------------------------------------------------------------------
def _blend_scene(pkg, tmp_path):
    import json
    src = GOLDEN / "json_scene"
    d = json.loads((src / "three_boxes.json").read_text())
    d["materials"][1]["metallic"] = 0.35
    d["materials"][0]["metallic"] = 0.6
    (tmp_path / "sky_32x16.png").write_bytes((src / "sky_32x16.png").read_bytes())
    (tmp_path / "blend.json").write_text(json.dumps(d))
    return pkg.host_scene.load_json(tmp_path / "blend.json")


@pytest.mark.parametrize("what", ["area", "blend", "ltree", "ltree2", "texfilter", "motion", "wavefront", "stats"])
def test_refused_combinations_answer_with_a_state_error(renderer, pkg, O, tmp_path, what):
    sc = O.cornell_box(32, 32)
    match = {"area": "emissive triangles", "blend": "blend materials", "ltree": "light tree", "ltree2": "light tree",
             "texfilter": "texture filter", "motion": "motion blur", "wavefront": "wavefront BVH strategy", "stats": "counting kernels"}[what]
    if what == "blend":
        sc = _blend_scene(pkg, tmp_path)
    elif what in ("ltree", "ltree2"):
        sc = _many_lights_cornell(O, pkg, 32)
    elif what == "texfilter":
        sc = _textured_cornell(O, pkg, 32)
    renderer.upload_scene(sc)
    renderer.set_limits(4)
    renderer.set_partition(0, 1)
    try:
        renderer.upload_vertex_normals(pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0))
        if what == "area":
            renderer.upload_area_lights([20], [[5, 5, 5]])
        elif what in ("ltree", "ltree2"):
            renderer.set_light_sampling(1 if what == "ltree" else 2)
        elif what == "texfilter":
            renderer.set_texture_filter(pkg.binding.TEXFILTER_REFERENCE)
        elif what == "motion":
            renderer.set_motion(sc.xs, sc.ys, sc.zs)
        elif what in ("wavefront", "stats"):
            renderer.set_accel(1)
            if what == "wavefront":
                renderer.set_bvh_strategy(2)
        with pytest.raises(pkg.DmtError, match=r"\(3\).*vertex normals.*" + match):  # DMT_ERR_STATE
            if what == "stats":
                renderer.render_stats(1)
            else:
                renderer.render(1)
        if what == "motion":
            with pytest.raises(pkg.DmtError, match=r"\(3\).*vertex normals.*motion blur"):
                renderer.test_trace_log(3, 4, 0)
    finally:
        renderer.set_light_sampling(0)
        renderer.set_texture_filter(pkg.binding.TEXFILTER_LEVEL0)
        renderer.set_bvh_strategy(0)
        renderer.clear_motion()
        _reset(renderer)


def test_upload_validation_and_lifetime(renderer, pkg, O):
    sc = O.cornell_box(32, 32)
    n9 = pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0)
    renderer.upload_scene(sc)
    renderer.set_limits(4)
    renderer.set_partition(0, 1)
    try:
        with pytest.raises(pkg.DmtError, match=r"\(1\).*count differs"):  # DMT_ERR_INVALID
            renderer.upload_vertex_normals(n9[:-1])
        bad = n9.copy()
        bad[7, 4] = np.nan
        with pytest.raises(pkg.DmtError, match=r"\(1\).*triangle 7 "):
            renderer.upload_vertex_normals(bad)
        bad = n9.copy()
        bad[11, 3:6] = 0  # one zero normal among three
        with pytest.raises(pkg.DmtError, match=r"\(1\).*triangle 11 "):
            renderer.upload_vertex_normals(bad)
        assert renderer.vertex_normals_info() == {"triangles": 0, "smooth_triangles": 0}  # a refused upload leaves none
        mixed = n9.copy()
        mixed[16:] = 0  # the walls flat, the octahedra smooth
        renderer.upload_vertex_normals(mixed * np.float32(3.5))  # any length: normalised on the host
        assert renderer.vertex_normals_info() == {"triangles": 26, "smooth_triangles": 16}
        smooth_film = _film(renderer, 4)[0]
        renderer.update_vertices(sc.xs, sc.ys, sc.zs)  # keeps them, like UVs and materials
        assert renderer.vertex_normals_info() == {"triangles": 26, "smooth_triangles": 16}
        assert np.array_equal(_film(renderer, 4)[0], smooth_film)
        renderer.clear_vertex_normals()
        cleared = _film(renderer, 4)
        renderer.upload_vertex_normals(mixed)
        renderer.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)  # drops them
        assert renderer.vertex_normals_info() == {"triangles": 0, "smooth_triangles": 0}
        dropped = _film(renderer, 4)
    finally:
        _reset(renderer)
    with pkg.Renderer(0) as fresh:  # a context that never had normals
        fresh.upload_scene(sc)
        fresh.set_limits(4)
        fresh.set_partition(0, 1)
        never = _film(fresh, 4)
    assert not np.array_equal(smooth_film, never[0])
    assert cleared[0].tobytes() == never[0].tobytes() and cleared[1].tobytes() == never[1].tobytes()
    assert dropped[0].tobytes() == never[0].tobytes()


# ---- 9. defaults untouched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell", "c3_sphere_veranda"])
def test_films_without_normals_survive_an_upload_and_clear_cycle(renderer, pkg, O, scene):
    if scene == "cornell":
        sc = O.cornell_box(64, 64)
        n9 = pkg.smooth_normals(sc.xs, sc.ys, sc.zs, 180.0)
    else:
        sc = pkg.host_scene.load_json(GOLDEN / "c3" / "c3_sphere_veranda.json").set_resolution(64, 64)
        n9 = sc.tri_normals
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_partition(0, 1)
    try:
        before = _film(renderer, 16)
        renderer.upload_vertex_normals(n9)
        with_normals = _film(renderer, 16)
        renderer.clear_vertex_normals()
        after = _film(renderer, 16)
    finally:
        _reset(renderer)
    assert np.isfinite(with_normals[0]).all() and not np.array_equal(with_normals[0], before[0])
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
