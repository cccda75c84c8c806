"""GPU tests of the display transform (dmt_display) against tests/display_ref.py: the histogram and the
metering, the identity with the PNG writer's rule, the curves, the bloom pyramid, the quantisers, the device-pointer entry,
the invariants on a rendered film, and the CLI.  Frames of a few thousand pixels; every case runs in well under a second.

Measured on an MI355X (the curves' largest |error| against float64 over test_display.curve_inputs(), device / host twin):
see DESIGN.md 4.23."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import display_ref as D  # noqa: E402
from test_display import PAIRS, ULP1, curve_inputs, host_curve_errors  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
F = np.float32
# auto exposure, bloom, a curve with a division, a transfer function with a pow, the dither: every stage has work
PARAMS_ALL_STAGES = dict(auto_exposure=1, exposure_ev=0.5, bloom_levels=3, bloom_strength=0.4, tone=D.TONE_ACES,
                         oetf=D.OETF_SRGB, quantiser=D.QUANT_DITHER)


def make_plane(h, w, seed, stops=20.0):
    """rgb spanning 2 * stops stops around 1 with zeros, negatives, NaN and inf sprinkled in; w = 1"""
    rng = np.random.default_rng(seed)
    p = np.ones((h, w, 4), F)
    p[..., :3] = (2.0 ** rng.uniform(-stops, stops, (h, w, 3))).astype(F)
    flat = p.reshape(-1, 4)
    n = flat.shape[0]
    for k, v in enumerate((0.0, -0.0, -3.5, np.nan, np.inf, -np.inf)):
        idx = rng.integers(0, n, max(n // 23, 1))
        flat[idx, (k + np.arange(idx.size)) % 3] = v
    flat[rng.integers(0, n, max(n // 31, 1)), :3] = 0.0  # whole pixels the meter skips
    if n > 2:
        flat[1, :3] = [np.nan, np.inf, -1.0]              # one pixel, two non-finite components: counted once
    return p


def camera(pkg, w, h):
    return pkg.host_scene.cornell_box(w, h).camera


@pytest.fixture(scope="module")
def r(pkg):
    with pkg.Renderer(0) as ren:
        yield ren


def show(r, pkg, plane, over, want=("float", "u8")):
    h, w = plane.shape[:2]
    if (r.width, r.height) != (w, h):
        r.set_camera(camera(pkg, w, h))
    return r.display(over, image=plane, want=want)


def assert_close_bloom(got, ref):
    """the a-trous filter's tolerance of tests/test_denoise_gpu.py"""
    ref = np.asarray(ref, np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref).mean()))


# ---- 1. histogram ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(50, 80), (1, 1), (257, 3)])
def test_histogram_and_metering(r, pkg, w, h):
    plane = make_plane(h, w, seed=w + h)
    over = dict(auto_exposure=1, exposure_ev=-0.5)
    show(r, pkg, plane, over, want="u8")
    info = r.display_info()
    hist, skipped, nonfinite = D.histogram(plane[..., :3])
    assert np.array_equal(info["histogram"], hist)
    assert info["counted"] == int(hist.sum()) and info["skipped"] == skipped
    assert info["counted"] + info["skipped"] == w * h
    assert info["nonfinite"] == nonfinite
    avg, scale = pkg.display_metering(info["histogram"], over)
    assert info["scale"].tobytes() == scale.tobytes() and info["avg_log2"] == avg
    assert (info["width"], info["height"]) == (w, h)


def test_histogram_all_skipped_falls_back_to_the_manual_scale(r, pkg):
    plane = np.zeros((3, 5, 4), F)
    plane[0, 0, :3] = [np.nan, -1.0, 0.0]
    show(r, pkg, plane, dict(auto_exposure=1, exposure_ev=2.0), want="u8")
    info = r.display_info()
    assert info["counted"] == 0 and info["skipped"] == 15 and info["nonfinite"] == 1 and info["scale"] == F(4.0)


# ---- 2. identity with the PNG writer --------------------------------------------------------------
def test_linear_truncate_is_the_png_writers_rule(r, pkg):
    rng = np.random.default_rng(2)
    plane = rng.uniform(-1.0, 3.0, (80, 50, 4)).astype(F)
    plane[0, :4, :3] = [[0.0, 1.0, 0.5], [1.0 / 255, 254.999 / 255, 2.0 / 255], [-0.0, 1e-40, 0.999999], [0.00392, 0.00393, 1.0000001]]
    u8 = show(r, pkg, plane, dict(tone=D.TONE_LINEAR, oetf=D.OETF_LINEAR, quantiser=D.QUANT_TRUNCATE), want="u8")
    ref, _ = pkg.host_scene.film_to_rgb8(plane, np.ones_like(plane))
    assert np.array_equal(u8[..., :3], ref)
    assert (u8[..., 3] == 255).all()
    assert r.display_info()["nonfinite"] == 0 and r.display_info()["levels"] == 0


# ---- 3. curves ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_errors(pkg):
    return host_curve_errors(pkg)


@pytest.mark.parametrize("tone,oetf", PAIRS)
def test_curves_on_the_device(r, pkg, host_errors, tone, oetf):
    x = curve_inputs()
    plane = np.ones((1, x.shape[0], 4), F)
    plane[0, :, :3] = x
    over = dict(tone=D.TONES[tone], oetf=D.OETFS[oetf])
    out = show(r, pkg, plane, over, want="float")
    ref = D.curve64(x, D.params(**over))
    err = float(np.abs(out[0, :, :3].astype(np.float64) - ref).max())
    bound = max(4 * host_errors[(tone, oetf)], ULP1)
    print(f"{tone}/{oetf}: device max |err| = {err:.3e}, host twin = {host_errors[(tone, oetf)]:.3e}, bound = {bound:.3e}")
    assert (out[..., 3] == 1).all()
    assert err <= bound


# ---- 4. bloom -------------------------------------------------------------------------------------
LIN = dict(tone=D.TONE_LINEAR, oetf=D.OETF_LINEAR)


def _bloom_case(r, pkg, plane, levels, strength=0.7):
    over = dict(LIN, bloom_levels=levels, bloom_strength=strength)
    out = show(r, pkg, plane, over, want="float")
    c, info = D.exposed(plane, D.params(**over))
    assert r.display_info()["levels"] == info["levels"]
    assert_close_bloom(out[..., :3], np.clip(c, 0, 1))
    return out, info["levels"]


def test_bloom_single_bright_pixel(r, pkg):
    plane = np.zeros((23, 37, 4), F)
    plane[9, 30, :3] = [1.0, 0.5, 0.25]
    out, levels = _bloom_case(r, pkg, plane, 3)
    assert levels == 3
    # mean-preserving but for the clamped borders, and spread: the neighbours light up, the peak drops
    assert out[9, 30, 0] < 1.0 and out[9, 29, 0] > 0 and out[12, 33, 0] > 0
    out8, levels8 = _bloom_case(r, pkg, plane, 8)
    assert levels8 == 4  # floor(log2(23))


@pytest.mark.parametrize("levels,used", [(1, 1), (3, 3), (8, 5)])
def test_bloom_noise_plane(r, pkg, levels, used):
    plane = np.random.default_rng(4).uniform(0, 1, (80, 50, 4)).astype(F)
    _, got = _bloom_case(r, pkg, plane, levels)
    assert got == used  # 8 is clipped to floor(log2(50)) = 5


@pytest.mark.parametrize("w,h,used", [(1, 1, 0), (2, 3, 1), (3, 2, 1)])
def test_bloom_tiny_frames(r, pkg, w, h, used):
    plane = np.random.default_rng(w).uniform(0, 1, (h, w, 4)).astype(F)
    _, got = _bloom_case(r, pkg, plane, 8)
    assert got == used


def test_bloom_off_is_bit_identical(r, pkg):
    plane = make_plane(80, 50, seed=6, stops=3.0)
    base = dict(auto_exposure=1, quantiser=D.QUANT_DITHER)
    f0, u0 = show(r, pkg, plane, base)
    for off in (dict(bloom_levels=3, bloom_strength=0.0), dict(bloom_levels=0, bloom_strength=0.5)):
        f1, u1 = show(r, pkg, plane, dict(base, **off))
        assert r.display_info()["levels"] == 0
        assert f1.tobytes() == f0.tobytes() and u1.tobytes() == u0.tobytes()
    f2, _ = show(r, pkg, plane, dict(base, bloom_levels=3, bloom_strength=0.5))
    assert f2.tobytes() != f0.tobytes()


# ---- 5. quantisers --------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [D.QUANT_TRUNCATE, D.QUANT_ROUND, D.QUANT_DITHER])
def test_quantisers_byte_for_byte(r, pkg, q):
    h, w = 21, 19
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    plane = np.ones((h, w, 4), F)
    g = ((xx + yy * w) / (h * w - 1)).astype(F)  # 0 .. 1 over the frame, a fraction of a code per pixel in the dark end
    plane[..., 0], plane[..., 1], plane[..., 2] = g * F(0.05), g, g * F(1.2)
    over = dict(tone=D.TONE_LINEAR, oetf=D.OETF_LINEAR, quantiser=q)
    out4, u8 = show(r, pkg, plane, over)
    assert np.array_equal(u8, D.quantise(out4, D.params(**over)))
    assert (u8[..., 3] == 255).all() and (out4[..., 3] == 1).all()
    over = dict(quantiser=q)  # and under the default curve
    out4, u8 = show(r, pkg, plane, over)
    assert np.array_equal(u8, D.quantise(out4, D.params(**over)))
    if q == D.QUANT_DITHER:  # the Bayer phase shows: a constant plane gives a pattern of period 8
        flat = np.full((h, w, 4), 100.3 / 255, F)
        u = show(r, pkg, flat, dict(tone=D.TONE_LINEAR, oetf=D.OETF_LINEAR, quantiser=q), want="u8")[..., 0]
        assert set(np.unique(u)) == {100, 101} and np.array_equal(u[:8, :8], u[8:16, 8:16]) and not np.array_equal(u[:8, :8], u[1:9, :8])


# ---- 6. device pointers ---------------------------------------------------------------------------
def test_device_pointer_entry_matches_the_host_entry(tmp_path):
    out = tmp_path / "out.npz"
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "_display_device_worker.py"), str(out)], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    z = np.load(out)
    film = make_plane(50, 80, seed=11)
    for tag in ("auto", "manual"):
        for a, b in (("host", "dev"), ("host", "bound"), ("src_host", "src_dev")):
            assert z[f"{tag}_{a}_f"].tobytes() == z[f"{tag}_{b}_f"].tobytes(), (tag, a, b)
            assert z[f"{tag}_{a}_u"].tobytes() == z[f"{tag}_{b}_u"].tobytes(), (tag, a, b)
        assert z[f"{tag}_src_host_u"].tobytes() != z[f"{tag}_host_u"].tobytes()
    _, skipped, nonfinite = D.histogram(film[..., :3])
    assert list(z["auto_dev_info"]) == [50 * 80 - skipped, skipped, nonfinite, 3]
    assert list(z["manual_dev_info"]) == [0, 0, nonfinite, 0] and z["manual_dev_scale"] == F(0.5)
    assert z["only_f"].tobytes() == z["auto_host_f"].tobytes() and z["only_u"].tobytes() == z["auto_host_u"].tobytes()
    assert int(z["both_null_refused"]) == 1
    assert z["film_after"].tobytes() == film.tobytes()  # the bound film is read, never written


# ---- 7. invariants on a rendered film -------------------------------------------------------------
def test_display_of_a_rendered_film(pkg):
    scene = pkg.host_scene.cornell_box(64, 64)
    with pkg.Renderer(0) as ren:
        ren.upload_scene(scene)
        ren.set_limits(5)
        ren.render(spp=16)
        mean0, m20 = ren.download_film()
        ren.render_aovs(2)
        den0 = ren.denoise()
        over = dict(auto_exposure=1)
        out4, u8 = ren.display(over)
        info = ren.display_info()
        den1 = ren.denoise()
        mean1, m21 = ren.download_film()
        assert mean1.tobytes() == mean0.tobytes() and m21.tobytes() == m20.tobytes()
        assert den1.tobytes() == den0.tobytes()
        # against the restatement on the downloaded mean: histogram, metering and quantiser exactly
        p = D.params(**over)
        c, ref = D.exposed(mean0, p)
        assert np.array_equal(info["histogram"], ref["histogram"]) and info["nonfinite"] == 0
        assert info["counted"] + info["skipped"] == 64 * 64
        assert info["scale"].tobytes() == pkg.display_metering(info["histogram"], over)[1].tobytes()
        assert abs(float(info["scale"]) - float(ref["scale"])) <= float(np.spacing(ref["scale"]))
        assert np.array_equal(u8, D.quantise(out4, p))
        # the float plane: the curves' rule, the host twin's error on these very values
        c = (info["scale"] * D.scrub(mean0[..., :3])[0]).astype(F)
        ref64 = D.curve64(c, p)
        host_err = float(np.abs(pkg.display_curve(c, over).astype(np.float64) - ref64).max())
        err = float(np.abs(out4[..., :3].astype(np.float64) - ref64).max())
        print(f"rendered film, aces/srgb: device max |err| = {err:.3e}, host twin = {host_err:.3e}")
        assert err <= max(4 * host_err, ULP1)
        assert 0.05 < float(out4[..., :3].mean()) < 0.95  # a picture, neither black nor clipped
        # with bloom, linear curve: the pyramid's tolerance
        over = dict(LIN, auto_exposure=1, bloom_levels=4, bloom_strength=0.5)
        out4 = ren.display(over, want="float")
        cb, _ = D.exposed(mean0, D.params(**over))
        assert_close_bloom(out4[..., :3], np.clip(cb, 0, 1))
        assert ren.download_film()[0].tobytes() == mean0.tobytes()


def test_refusals_on_a_context(pkg):
    with pkg.Renderer(0) as ren:
        with pytest.raises(pkg.DmtError, match="camera"):
            ren.display()
        with pytest.raises(pkg.DmtError, match="no display call"):
            ren.display_info()
        ren.set_camera(camera(pkg, 8, 4))
        plane = make_plane(4, 8, seed=1, stops=2.0)
        ren.display(dict(exposure_ev=1.0), image=plane)
        before = ren.display_info()
        for bad, what in ((dict(key=0.0), "key"), (dict(bloom_levels=9), "bloom_levels"), (dict(tone=7), "tone"),
                          (dict(white=-1.0), "white"), (dict(low_fraction=0.6, high_fraction=0.6), "fraction"),
                          (dict(exposure_ev=np.nan), "finite")):
            with pytest.raises(pkg.DmtError, match=what):
                ren.display(bad, image=plane)
        with pytest.raises(pkg.DmtError, match="both null"):
            ren.display_device(None, None, None, None)
        ren.set_partition(0, 2)
        with pytest.raises(pkg.DmtError, match="combine"):
            ren.display()
        after = ren.display_info()  # the refused calls left the record as it was
        assert after["scale"] == before["scale"] == F(2.0) and after["nonfinite"] == before["nonfinite"]
        out = ren.display(dict(exposure_ev=1.0), image=plane, want="u8")  # a plane is still welcome
        assert out.shape == (4, 8, 4)


# ---- 8. CLI ---------------------------------------------------------------------------------------
def test_cli_display_writes_the_extra_png_and_nothing_else_changes(pkg, tmp_path):
    plain, disp = tmp_path / "plain", tmp_path / "disp"
    plain.mkdir(), disp.mkdir()
    base = [str(EXE), "--width", "32", "--height", "32", "--spp", "16", "--kspp", "8", "--max-depth", "5"]
    r1 = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run(base + ["--tonemap", "aces", "--exposure", "auto", "--oetf", "srgb", "--hdr", "--time", "-o", str(disp)],
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert sorted(p.name for p in disp.iterdir()) == sorted([p.name for p in plain.iterdir()] + ["output-16_display.png", "output-16.pfm"])
    for p in plain.iterdir():
        assert (disp / p.name).read_bytes() == p.read_bytes(), p.name
    assert {"output-16.png", "output-16_sqrt_mse.png"} <= {p.name for p in plain.iterdir()}
    assert any("display:" in l and "metered" in l for l in r2.stdout.splitlines())
    film = np.ones((32, 32, 4), F)
    film[..., :3] = D.read_pfm(disp / "output-16.pfm")
    with pkg.Renderer(0) as ren:
        ren.set_camera(camera(pkg, 32, 32))
        u8 = ren.display(dict(tone=D.TONE_ACES, auto_exposure=1, oetf=D.OETF_SRGB), image=film, want="u8")
    assert np.array_equal(D.read_png_rgb8(disp / "output-16_display.png"), u8[..., :3])
    assert len(np.unique(u8[..., :3])) > 32


def test_cli_display_of_the_denoised_plane(tmp_path):
    r = subprocess.run([str(EXE), "--width", "32", "--height", "32", "--spp", "16", "--kspp", "8", "--max-depth", "5", "--denoise",
                        "--aov-spp", "2", "--tonemap", "reinhard", "--white", "3", "--bloom", "0.2", "--dither", "-o", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["output-16.png", "output-16_denoised.png", "output-16_denoised_display.png",
                                                          "output-16_display.png", "output-16_sqrt_mse.png"]
    film, den = D.read_png_rgb8(tmp_path / "output-16_display.png"), D.read_png_rgb8(tmp_path / "output-16_denoised_display.png")
    assert film.shape == den.shape == (32, 32, 3) and not np.array_equal(film, den)
    # the same transform of a smoother plane: neighbouring pixels differ less
    rough = [float(np.abs(np.diff(x.astype(np.int32), axis=1)).mean()) for x in (film, den)]
    assert rough[1] < rough[0], rough
