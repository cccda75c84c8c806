"""The denoiser without a GPU (dmt_render_aovs / dmt_denoise): the C ABI declares the entry points and the
parameter layout, the binding wraps them, the numpy restatement (tests/denoise_ref.py) has the filter's properties, and the
CLI rejects bad --denoise / --aov-spp values before it creates a context."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_ref as R
from test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
NEW = ("dmt_render_aovs", "dmt_upload_aovs", "dmt_download_aovs", "dmt_denoise_defaults", "dmt_denoise")


def _decl(name):
    text = (ROOT / "include" / "dmt_hip.h").read_text()
    m = re.search(r"\b(int|dmt_denoise_params) " + name + r"\(", text)
    decl = text[m.start():]
    return " ".join(decl[:decl.index(";")].split())


def test_header_declares_the_denoiser():
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert _decl("dmt_render_aovs") == "int dmt_render_aovs(dmt_ctx* ctx, uint32_t aov_spp)"
    assert _decl("dmt_upload_aovs") == ("int dmt_upload_aovs(dmt_ctx* ctx, const float* albedo4, const float* normal4, "
                                        "const float* position4, int width, int height)")
    assert _decl("dmt_download_aovs") == "int dmt_download_aovs(dmt_ctx* ctx, float* albedo4, float* normal4, float* position4)"
    assert _decl("dmt_denoise_defaults") == "dmt_denoise_params dmt_denoise_defaults(void)"
    assert _decl("dmt_denoise") == ("int dmt_denoise(dmt_ctx* ctx, const dmt_denoise_params* params, const float* mean4, "
                                    "const float* m24, float* out4, float* kernel_ms)")


def test_params_layout():
    text = (ROOT / "include" / "dmt_hip.h").read_text()
    body = re.search(r"typedef struct dmt_denoise_params \{(.*?)\} dmt_denoise_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int32_t iterations", "float sigma_normal", "float sigma_position", "float sigma_albedo", "float sigma_luminance"]


def test_library_and_binding(pkg):
    lib = pkg.load_library()
    from cuda_optix_pathtracing_amd import binding
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTED_SYMBOLS, s
    for m in ("render_aovs", "upload_aovs", "download_aovs", "denoise"):
        assert callable(getattr(binding.Renderer, m, None)), m
    d = binding.denoise_defaults()
    assert d["iterations"] == R.DEFAULTS["iterations"]
    for k in ("sigma_normal", "sigma_position", "sigma_albedo", "sigma_luminance"):
        assert np.float32(d[k]) == np.float32(R.DEFAULTS[k]), k


def test_null_context_is_invalid(pkg):
    import ctypes as C
    lib = pkg.load_library()
    out = np.zeros(4, np.float32)
    assert lib.dmt_render_aovs(None, C.c_uint32(4)) == 1
    assert lib.dmt_download_aovs(None, None, None, None) == 1
    assert lib.dmt_denoise(None, None, None, None, out.ctypes.data_as(C.c_void_p), None) == 1


# ---- the restatement -----------------------------------------------------------------------------------------------
def _scene(h=24, w=32, seed=3, split=False, background=False):
    """noisy film + AOVs of a few planes; split: left and right halves face opposite ways"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[..., :3] = np.where((xx // 8 % 2 == 0)[..., None], [0.8, 0.5, 0.3], [0.2, 0.6, 0.9])
    albedo[..., 3] = 1
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., 2] = 1
    position = np.stack([xx * 0.01, yy * 0.01, np.where(yy < h // 2, 0.0, 0.3), np.full_like(xx, 2.0)], -1).astype(np.float32)
    if split:
        normal[:, w // 2:, 2] = -1
    if background:
        albedo[:4, :6] = 0
        normal[:4, :6] = 0
        position[:4, :6] = 0
    n = rng.integers(2, 64, (h, w)).astype(np.float32)
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = albedo[..., :3] * 0.7 + rng.normal(0, 0.1, (h, w, 3)).astype(np.float32)
    m2 = np.zeros((h, w, 4), np.float32)
    m2[..., :3] = rng.uniform(0.01, 0.5, (h, w, 3)) * (n[..., None] - 1)
    m2[..., 3] = n
    return mean, m2, albedo, normal, position


TH = np.float32(0.002)


def test_zero_iterations_is_the_identity():
    mean, m2, a, n, x = _scene()
    out = R.denoise(mean, m2, a, n, x, TH, iterations=0)
    assert np.array_equal(out[..., :3].view(np.uint32), mean[..., :3].view(np.uint32))
    assert (out[..., 3] == 1).all()


def test_constant_image_stays_constant():
    mean, m2, a, n, x = _scene()
    mean[..., :3] = np.float32(0.375)
    out = R.denoise(mean, m2, a, n, x, TH, iterations=5)
    assert np.allclose(out[..., :3], 0.375, rtol=1e-5, atol=0)


def test_weights_are_normalised_convex_combinations():
    mean, m2, a, n, x = _scene(seed=8)
    c, v, _ = R.initial(mean, m2)
    c1, v1 = R.atrous_pass(c, v, a, n, x, 2, TH, 128.0, 1.0, 0.1, 4.0)
    w = R.tap_weights(c, v, a, n, x, 2, TH, 128.0, 1.0, 0.1, 4.0)
    sw = sum(w.values())
    # the result is sum (w / sum w) c_q: within [min, max] of the taps that took part
    lo, hi = np.full_like(c, np.inf), np.full_like(c, -np.inf)
    for (dx, dy), wq in w.items():
        cq, _ = R._shift(c, dy * 2, dx * 2)
        use = (wq > 0)[..., None]
        lo, hi = np.where(use, np.minimum(lo, cq), lo), np.where(use, np.maximum(hi, cq), hi)
    assert (c1 >= lo - 1e-6).all() and (c1 <= hi + 1e-6).all()
    assert (sw >= w[(0, 0)]).all() and (w[(0, 0)] > 0).all()
    assert (v1 <= v.max() + 1e-6).all() and (v1 >= 0).all()


def test_pixels_across_a_normal_discontinuity_never_mix():
    """n_p . n_q <= 0 gives a tap weight of 0.  (Over several passes the variance blur g_p, which carries no edge weight,
    still couples the two sides' luminance terms, so the check is exact for one pass and a bound for five.)"""
    mean, m2, a, n, x = _scene(split=True)
    w = mean.shape[1]
    mean2 = mean.copy()
    mean2[:, w // 2:, :3] += np.float32(5.0)  # change only the colours of the side that faces away
    one, one2 = (R.denoise(m, m2, a, n, x, TH, iterations=1) for m in (mean, mean2))
    assert np.array_equal(one[:, :w // 2].view(np.uint32), one2[:, :w // 2].view(np.uint32))
    five = R.denoise(mean2, m2, a, n, x, TH, iterations=5)
    assert five[:, :w // 2, :3].max() <= mean2[:, :w // 2, :3].max() + 1e-6
    assert five[:, w // 2:, :3].min() >= mean2[:, w // 2:, :3].min() - 1e-6


def test_background_pixels_pass_through_and_feed_no_one():
    mean, m2, a, n, x = _scene(background=True)
    out = R.denoise(mean, m2, a, n, x, TH, iterations=4)
    assert np.array_equal(out[:4, :6, :3].view(np.uint32), mean[:4, :6, :3].view(np.uint32))
    mean2 = mean.copy()
    mean2[:4, :6, :3] = np.float32(100.0)
    out2 = R.denoise(mean2, m2, a, n, x, TH, iterations=4)
    cover = a[..., 3] > 0
    assert np.array_equal(out[cover].view(np.uint32), out2[cover].view(np.uint32))


def test_filter_reduces_noise_of_a_flat_region():
    rng = np.random.default_rng(1)
    h, w = 32, 32
    a = np.zeros((h, w, 4), np.float32)
    a[..., :3], a[..., 3] = 0.5, 1
    n = np.zeros((h, w, 4), np.float32)
    n[..., 2] = 1
    x = np.zeros((h, w, 4), np.float32)
    x[..., 3] = 2
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = 0.4 + rng.normal(0, 0.05, (h, w, 1)).astype(np.float32)
    m2 = np.zeros((h, w, 4), np.float32)
    m2[..., :3], m2[..., 3] = 0.05 ** 2 * 16 * 15, 16  # the variance of the mean = the noise's
    out = R.denoise(mean, m2, a, n, x, TH)
    assert out[..., :3].std() < 0.25 * mean[..., :3].std()
    assert abs(float(out[..., :3].mean()) - float(mean[..., :3].mean())) < 0.01 * 0.4


def test_refused_pixels_are_reported():
    mean, m2, a, n, x = _scene()
    m2[3, 4, 3] = 1
    with pytest.raises(ValueError):
        R.denoise(mean, m2, a, n, x, TH)
    mean, m2, a, n, x = _scene()
    mean[0, 0, 1] = np.nan
    assert R.initial(mean, m2)[2].sum() == 1


# ---- CLI -------------------------------------------------------------------------------------------------------------
def _run(*args):
    assert EXE.exists(), "run __graft_entry__.build()"
    return subprocess.run([str(EXE), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, message", [
    (("--aov-spp",), "missing value"),
    (("--aov-spp", "8"), "--aov-spp needs --denoise"),
    (("--denoise", "--aov-spp", "0"), "invalid --aov-spp"),
    (("--denoise", "--aov-spp", "-3"), "invalid --aov-spp"),
    (("--denoise", "--aov-spp", "70000"), "invalid --aov-spp"),
])
def test_cli_rejects_bad_denoise_values_before_any_gpu_call(args, message):
    r = _run(*args)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert "dmt_ctx_create" not in r.stderr and "Running HIP Kernel" not in r.stdout


def test_cli_help_lists_denoise_flags():
    h = _run("--help")
    assert h.returncode == 0
    for flag in ("--denoise", "--aov-spp <N>", "_denoised.png"):
        assert flag in h.stdout, flag
