"""The denoiser on the GPU (dmt_render_aovs, dmt_denoise).  The filter is checked against the numpy
restatement (tests/denoise_ref.py) on synthetic inputs; the feature buffers against a restatement built from the camera-ray
and closest-hit probes, on plain, textured (texfilter_ref's level-0 lookups, normal maps) and blended-metallic materials; the
invariants of the C ABI; the quality on three scenes; and the CLI."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as R
import texfilter_ref as TR
from conftest import GOLDEN
from test_kernel_rows_gpu import _blend_scene
from test_parity_gpu import _textured_cornell

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
RES = 64


@pytest.fixture(scope="module")
def cb(pkg):
    r = pkg.Renderer(0)
    sc = pkg.host_scene.cornell_box(RES, RES)
    r.upload_scene(sc)
    r.set_limits(5)
    yield r, sc
    r.close()


def _reset(r, sc):
    r.set_accel(0)
    r.set_partition(0, 1)
    r.set_camera(sc.camera)


def _synthetic(h, w, seed):
    """film + AOVs: noise over planes with depth steps, albedo edges, a background region, N from 2 to 10^4"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.zeros((h, w, 4), np.float32)
    a[..., :3] = np.where(((xx // 7 + yy // 5) % 3 == 0)[..., None], [0.9, 0.4, 0.2], [0.3, 0.7, 0.5])
    a[..., :3] += rng.uniform(0, 0.02, (h, w, 3)).astype(np.float32)
    a[..., 3] = 1
    n = np.zeros((h, w, 4), np.float32)
    tilt = np.where(xx < w // 3, 0.0, np.where(xx < 2 * w // 3, 0.4, -0.7)).astype(np.float32)
    n[..., 0], n[..., 2] = tilt, 1
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    depth = np.where(yy < h // 2, 2.0, 2.6).astype(np.float32) + 0.01 * xx
    x = np.stack([xx * 0.01, yy * 0.01, depth, depth * 1.1], -1).astype(np.float32)
    bg = (xx > w - 12) & (yy < 9)
    a[bg], n[bg], x[bg] = 0, 0, 0
    a[5:9, 3:7, 3] = 0.5  # partial coverage
    N = np.exp(rng.uniform(np.log(2), np.log(1e4), (h, w))).round().astype(np.float32)
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = a[..., :3] * 0.6 + rng.normal(0, 0.2, (h, w, 3)).astype(np.float32) / np.sqrt(N)[..., None]
    mean[bg, :3] = 0.05
    m2 = np.zeros((h, w, 4), np.float32)
    m2[..., :3] = rng.uniform(0.005, 0.2, (h, w, 3)).astype(np.float32) * (N[..., None] - 1)
    m2[..., 3] = N
    return mean, m2, a, n, x


def test_filter_matches_the_restatement(cb, pkg):
    r, sc = cb
    h, w = 50, 80  # not a multiple of the 64 x 4 block
    cam = sc.camera.copy()
    cam[24:32] = np.array([w, h], np.int32).view(np.uint8)
    try:
        r.set_camera(cam)
        th = R.theta(cam)
        for seed in (1, 2):
            mean, m2, a, n, x = _synthetic(h, w, seed)
            r.upload_aovs(a, n, x)
            for k in range(7):
                got = r.denoise({"iterations": k}, film=(mean, m2))
                ref = R.denoise(mean, m2, a, n, x, th, iterations=k)
                if k == 0:
                    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
                else:
                    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref[..., :3]).mean()),
                                               err_msg=f"seed {seed}, K = {k}")
            p = dict(iterations=3, sigma_normal=16.0, sigma_position=4.0, sigma_albedo=0.5, sigma_luminance=1.0)
            got = r.denoise(p, film=(mean, m2))
            ref = R.denoise(mean, m2, a, n, x, th, **p)
            np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref[..., :3]).mean()))
    finally:
        _reset(r, sc)


def _restated_aovs(r, sc, aov_spp):
    """the AOVs from dmt_test_camera_rays + dmt_test_closest_hit + the BSDF records' fp16 W (float32 sums in sample order)"""
    h, w = sc.height, sc.width
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.ravel(), yy.ravel()
    tris = np.stack([sc.xs[:, :3], sc.ys[:, :3], sc.zs[:, :3]], -1).astype(np.float64)  # [n, vertex, xyz]
    W = sc.bsdfs[:, :6].copy().view(np.float16).astype(np.float32)  # w0 = W.x | W.y, w1.lo = W.z
    sw, sn, sp = (np.zeros((h * w, 3), np.float32) for _ in range(3))
    st, hits = np.zeros(h * w, np.float32), np.zeros(h * w, np.int64)
    for s in range(aov_spp):
        o, d = r.test_camera_rays(px, py, np.full_like(px, s))
        tri, t = r.test_closest_hit(o, d)
        hit = tri >= 0
        T = tris[np.maximum(tri, 0)]
        nf = np.cross(T[:, 2] - T[:, 0], T[:, 1] - T[:, 0])
        nf /= np.linalg.norm(nf, axis=-1, keepdims=True)
        nf = np.where((np.einsum("ij,ij->i", d, nf) > 0)[:, None], -nf, nf).astype(np.float32)
        pos = (o.astype(np.float64) + t[:, None].astype(np.float64) * d).astype(np.float32)
        Wh = W[sc.mat_id[np.maximum(tri, 0)]]
        sw = np.where(hit[:, None], sw + Wh, sw)
        sn = np.where(hit[:, None], sn + nf, sn)
        sp = np.where(hit[:, None], sp + pos, sp)
        st = np.where(hit, st + t, st)
        hits += hit
    hf = np.maximum(hits, 1).astype(np.float32)
    albedo = np.concatenate([sw / np.float32(aov_spp), (hits / aov_spp)[:, None]], -1)
    ln = np.linalg.norm(sn, axis=-1, keepdims=True)
    normal = np.concatenate([np.where(ln >= 1e-6, sn / np.maximum(ln, 1e-30), 0), np.zeros((h * w, 1))], -1)
    position = np.concatenate([sp / hf[:, None], (st / hf)[:, None]], -1)
    position[hits == 0] = 0
    return [v.reshape(h, w, 4).astype(np.float32) for v in (albedo, normal, position)]


@pytest.mark.parametrize("aov_spp", [1, 4])
def test_aovs_match_independent_hits(cb, aov_spp):
    r, sc = cb
    _reset(r, sc)
    r.render_aovs(aov_spp)
    got = r.download_aovs()
    want = _restated_aovs(r, sc, aov_spp)
    assert (got[0][..., 3] > 0).mean() > 0.9
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-6, err_msg="albedo")
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=2e-6, err_msg="normal")
    # the device's hit point is p0 + u e0 + v e1, the restatement's o + t d: equal to a few ulps of the coordinates
    np.testing.assert_allclose(got[2][..., :3], want[2][..., :3], rtol=0, atol=1e-5, err_msg="position")
    np.testing.assert_allclose(got[2][..., 3], want[2][..., 3], rtol=1e-6, atol=0, err_msg="t")


NONE = 0xFFFFFFFF


def _first_hits(r, sc):
    """camera sample 0 of every pixel: triangle, barycentrics (u of p1, v of p2; float64 Moeller-Trumbore on the probe's
    ray) and the face-forwarded geometric normal"""
    h, w = sc.height, sc.width
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.ravel(), yy.ravel()
    o, d = r.test_camera_rays(px, py, np.zeros_like(px))
    tri, _ = r.test_closest_hit(o, d)
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4)[:, :3] for a in (sc.xs, sc.ys, sc.zs))
    T = np.stack([xs, ys, zs], -1).astype(np.float64)[np.maximum(tri, 0)]
    o, d = o.astype(np.float64), d.astype(np.float64)
    e0, e1 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    pv = np.cross(d, e1)
    det = np.einsum("ij,ij->i", e0, pv)
    tv = o - T[:, 0]
    u = np.einsum("ij,ij->i", tv, pv) / det
    v = np.einsum("ij,ij->i", d, np.cross(tv, e0)) / det
    ng = np.cross(e1, e0)
    ng /= np.linalg.norm(ng, axis=-1, keepdims=True)
    ng = np.where((np.einsum("ij,ij->i", d, ng) > 0)[:, None], -ng, ng).astype(np.float32)
    return tri, u, v, ng


def _texture(sc, k):
    first, w, h = (int(x) for x in sc.tex_desc[k])
    return np.asarray(sc.tex_rgba, np.uint8).reshape(-1, 4)[first:first + w * h].reshape(h, w, 4)


def _normal_mapped(sc, k, s, t, ng):
    """apply_material_textures' normal map: level-0 lookup, 10-bit quantisation, Frame::fromZ(ng) by gram_schmidt"""
    F = np.float32
    n = TR.bilinear(_texture(sc, k), s, t, normal=True)
    n = np.trunc(n * F(1023) + F(0.5)) / F(1023)
    n = n / np.sqrt(np.dot(n, n))
    if abs(ng[0] - ng[1]) > 1e-3 or abs(ng[0] - ng[2]) > 1e-3:
        a = np.array([ng[2] - ng[1], ng[0] - ng[2], ng[1] - ng[0]], F)
    else:
        a = np.array([ng[2] - ng[1], ng[0] + ng[2], -ng[1] - ng[0]], F)
    a = a / np.sqrt(np.dot(a, a))
    b = np.cross(ng, a)
    ns = a * n[0] + b * n[1] + ng * n[2]
    return ns / np.sqrt(np.dot(ns, ns))


def _assert_close_but_quantised(got, want, quantum, what):
    """equal to float rounding, except where an fp16 / 10-bit rounding of the restatement's slightly different texture
    coordinate flips to the neighbouring step (a few pixels)"""
    err = np.abs(got - want).max(-1)
    assert err.max() <= 3 * quantum, (what, float(err.max()))
    assert (err > 2e-5).mean() < 0.03, (what, float((err > 2e-5).mean()))


def test_textured_aovs_match_level0_bilinear_lookups(renderer, pkg, O):
    """_textured_cornell: an albedo + roughness + normal-mapped Oren-Nayar sphere, a normal-mapped GGX sphere, an albedo-only
    floor and a normal-map-only wall; one sample per pixel, so the AOVs are the hit's W and shading normal themselves"""
    sc = _textured_cornell(O, pkg, RES)
    renderer.upload_scene(sc)
    renderer.set_accel(0)
    renderer.set_partition(0, 1)
    renderer.render_aovs(1)
    albedo, normal, _ = (a.reshape(-1, 4) for a in renderer.download_aovs())
    tri, u, v, ng = _first_hits(renderer, sc)
    W = sc.bsdfs[:, :6].copy().view(np.float16).astype(np.float32)
    kind = sc.bsdfs[:, 6:8].copy().view(np.uint16)[:, 0]
    mt = np.asarray(sc.mat_tex, np.uint32).reshape(-1, 4)
    uv = np.asarray(sc.tri_uv, np.float32).reshape(-1, 6).astype(np.float64)
    want_a, want_n = np.zeros((tri.size, 3), np.float32), np.zeros((tri.size, 3), np.float32)
    textured_albedo = mapped = 0
    for i in np.nonzero(tri >= 0)[0]:
        m = int(sc.mat_id[tri[i]])
        q = uv[tri[i]]
        w0 = 1 - u[i] - v[i]
        s, t = w0 * q[0] + u[i] * q[2] + v[i] * q[4], w0 * q[1] + u[i] * q[3] + v[i] * q[5]
        want_a[i] = W[m]
        if mt[m, 0] != NONE and kind[m] == 0:  # Oren-Nayar albedo patched from the texture, stored as fp16
            c = TR.bilinear(_texture(sc, int(mt[m, 0])), s, t)
            want_a[i] = np.clip(c, 0, 1).astype(np.float16).astype(np.float32)
            textured_albedo += 1
        want_n[i] = ng[i]
        if mt[m, 2] != NONE:
            want_n[i] = _normal_mapped(sc, int(mt[m, 2]), s, t, ng[i])
            mapped += 1
    hit = tri >= 0
    assert textured_albedo > 300 and mapped > 300, (textured_albedo, mapped)
    assert np.array_equal(albedo[:, 3], hit.astype(np.float32))
    _assert_close_but_quantised(albedo[hit, :3], want_a[hit], 2.0 ** -11, "albedo")
    _assert_close_but_quantised(normal[hit, :3], want_n[hit], 1.0 / 1023, "normal")


def test_blend_aovs_mix_the_two_records(renderer, pkg, tmp_path):
    """BS_GGX_BLEND pairs (three_boxes.json with fractional metallic): W = (1 - m) W_diel + m W_cond, where the dielectric
    record holds m in W.x.  The records' other W fields are set to distinct values here so that the mix is visible."""
    sc = _blend_scene(pkg, tmp_path)
    kind = sc.bsdfs[:, 6:8].copy().view(np.uint16)[:, 0]
    blend = np.nonzero(kind == 4)[0]
    assert blend.size == 2
    f16 = lambda *x: np.array(x, np.float16).view(np.uint8)  # noqa: E731
    for b in blend:
        sc.bsdfs[b, 2:6] = f16(0.8, 0.6)                   # W_diel.y, W_diel.z (W.x holds m)
        sc.bsdfs[b + 1, 0:6] = f16(0.5, 0.25, 0.75)        # W_cond
    renderer.upload_scene(sc)
    renderer.set_accel(0)
    renderer.set_partition(0, 1)
    renderer.render_aovs(1)
    albedo = renderer.download_aovs()[0].reshape(-1, 4)
    tri, _, _, _ = _first_hits(renderer, sc)
    W = sc.bsdfs[:, :6].copy().view(np.float16).astype(np.float32)
    F = np.float32
    seen = 0
    for i in np.nonzero(tri >= 0)[0]:
        m = int(sc.mat_id[tri[i]])
        if kind[m] == 4:
            mix = W[m, 0]
            want = np.array([F(1), W[m, 1], W[m, 2]], F) * (F(1) - mix) + W[m + 1] * mix
            seen += 1
        else:
            want = W[m]
        assert np.abs(albedo[i, :3] - want).max() <= 1e-6, (i, m, albedo[i], want)
    assert seen > 100, seen


def test_aovs_are_bitwise_equal_under_bvh_and_partition(cb):
    r, sc = cb
    try:
        r.render_aovs(4)
        bf = r.download_aovs()
        r.set_accel(1)
        r.render_aovs(4)
        bvh = r.download_aovs()
        r.set_accel(0)
        r.set_partition(1, 3)
        r.render_aovs(4)
        part = r.download_aovs()
    finally:
        _reset(r, sc)
    for a, b, c in zip(bf, bvh, part):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_film_and_aovs_are_untouched_and_calls_repeat(cb):
    r, sc = cb
    _reset(r, sc)
    r.film_clear()
    r.render(8)
    r.render_aovs(4)
    mean0, m20 = r.download_film()
    aov0 = r.download_aovs()
    out1 = r.denoise()
    out2 = r.denoise()
    mean1, m21 = r.download_film()
    aov1 = r.download_aovs()
    assert np.array_equal(out1.view(np.uint32), out2.view(np.uint32))
    assert np.array_equal(mean0.view(np.uint32), mean1.view(np.uint32)) and np.array_equal(m20.view(np.uint32), m21.view(np.uint32))
    for a, b in zip(aov0, aov1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ref = R.denoise(mean0, m20, *aov0, R.theta(sc.camera))
    np.testing.assert_allclose(out1, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref[..., :3]).mean()))
    assert (out1[..., 3] == 1).all()
    # the context's film and the same film passed from the host give the same image
    assert np.array_equal(r.denoise(film=(mean0, m20)).view(np.uint32), out1.view(np.uint32))


def test_refusals(cb, pkg):
    r, sc = cb
    _reset(r, sc)
    r.film_clear()
    r.render(4)
    r.render_aovs(2)
    mean, m2 = r.download_film()
    bad = m2.copy()
    bad[7, 9, 3] = 1
    with pytest.raises(pkg.DmtError, match=r"failed \(3\).*fewer than 2 samples"):
        r.denoise(film=(mean, bad))
    nan = mean.copy()
    nan[1, 2, 0] = np.nan
    with pytest.raises(pkg.DmtError, match=r"failed \(3\)"):
        r.denoise(film=(nan, m2))
    for p in ({"iterations": 11}, {"iterations": -1}, {"sigma_normal": 0.0}, {"sigma_albedo": -1.0},
              {"sigma_luminance": float("nan")}, {"sigma_position": float("inf")}):
        with pytest.raises(pkg.DmtError, match=r"failed \(1\)"):
            r.denoise(p)
    try:
        r.set_partition(1, 2)
        r.film_clear()
        r.render(4)
        with pytest.raises(pkg.DmtError, match=r"failed \(3\).*partition"):
            r.denoise()
    finally:
        _reset(r, sc)
    a, n, x = r.download_aovs()
    r.upload_aovs(*(np.concatenate([v, v[:8]], 0) for v in (a, n, x)))
    with pytest.raises(pkg.DmtError, match=r"failed \(3\).*AOVs are"):
        r.denoise(film=(mean, m2))
    r.render_aovs(2)  # back to the frame's size


def test_adaptive_film_denoises(cb):
    r, sc = cb
    _reset(r, sc)
    r.film_clear()
    r.render_adaptive(0.1, 32, 4, min_spp=4)
    r.render_aovs(4)
    mean, m2 = r.download_film()
    assert (m2[..., 3] >= 4).all()
    got = r.denoise()
    ref = R.denoise(mean, m2, *r.download_aovs(), R.theta(sc.camera))
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref[..., :3]).mean()))


# lower bounds of RMSE(noisy) / RMSE(denoised) at 16 spp with the defaults: the measured ratios (DESIGN.md 4.11, 8.13 /
# 2.13 / 1.88) with margin -- the renders are deterministic, the margin covers changes of the renderer's own noise
QUALITY = {"cornell": 4.0, "c3_sphere_veranda": 1.6, "teapot": 1.4}


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean(axis=-1)).mean())


def _quality_scene(pkg, name):
    """(scene, bounce cap, BVH) as tools/diag_denoise.py measures them"""
    hs = pkg.host_scene
    if name == "cornell":
        return hs.cornell_box(256, 256), 8, False
    if name == "c3_sphere_veranda":
        return hs.load_json(GOLDEN / "c3" / "c3_sphere_veranda.json"), 12, True
    return hs.load_json(GOLDEN / "scene_test" / "scene_test.json").set_resolution(256, 256), 8, True


@pytest.mark.parametrize("name", sorted(QUALITY))
def test_quality(pkg, name):
    sc, depth, bvh = _quality_scene(pkg, name)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(depth)
        if bvh:
            r.set_accel(1)
        r.film_clear()
        r.render(4096, sample_offset=64)  # independent of the 16-spp film
        ref, _ = r.download_film()
        r.film_clear()
        r.render(16)
        noisy, _ = r.download_film()
        r.render_aovs(4)
        den = r.denoise()
    e0, e1 = _rmse(noisy, ref), _rmse(den, ref)
    assert e1 * QUALITY[name] <= e0, (e0, e1, e0 / e1)
    assert abs(den[..., :3].mean() / ref[..., :3].mean() - 1) < 0.01


def test_cli_denoise_writes_the_extra_png_and_nothing_else_changes(tmp_path):
    plain, den = tmp_path / "plain", tmp_path / "den"
    plain.mkdir(), den.mkdir()
    base = [str(EXE), "--width", "64", "--height", "64", "--spp", "16", "--kspp", "8", "--max-depth", "5"]
    r1 = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run(base + ["--denoise", "--aov-spp", "2", "--time", "-o", str(den)], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert sorted(p.name for p in den.iterdir()) == sorted([p.name for p in plain.iterdir()] + ["output-16_denoised.png"])
    for p in plain.iterdir():
        assert (den / p.name).read_bytes() == p.read_bytes(), p.name
    assert any("denoise:" in l and "AOVs" in l for l in r2.stdout.splitlines())
