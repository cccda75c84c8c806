"""numpy restatement of the display transform (include/dmt_hip.h): the yardstick of tests/test_display.py and
tests/test_display_gpu.py.  float32, one rounding per operation, for the parts that are compared bit for bit (scrub,
luminance, bin, exposure, quantiser); float64 for the metering and for the curves, which are compared under a tolerance;
float32 in the library's order for the bloom pyramid."""
import numpy as np

F = np.float32
TONE_LINEAR, TONE_REINHARD, TONE_ACES, TONE_HABLE = 0, 1, 2, 3
OETF_LINEAR, OETF_SRGB, OETF_GAMMA22 = 0, 1, 2
QUANT_TRUNCATE, QUANT_ROUND, QUANT_DITHER = 0, 1, 2
TONES = {"linear": TONE_LINEAR, "reinhard": TONE_REINHARD, "aces": TONE_ACES, "hable": TONE_HABLE}
OETFS = {"linear": OETF_LINEAR, "srgb": OETF_SRGB, "gamma22": OETF_GAMMA22}
DEFAULTS = dict(auto_exposure=0, exposure_ev=0.0, key=0.18, low_fraction=0.10, high_fraction=0.05, bloom_levels=0,
                bloom_strength=0.0, tone=TONE_ACES, white=0.0, oetf=OETF_SRGB, quantiser=QUANT_ROUND)

# the standard 8 x 8 Bayer index matrix, M[y][x]
BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                   [48, 16, 56, 24, 50, 18, 58, 26],
                   [12, 44, 4, 36, 14, 46, 6, 38],
                   [60, 28, 52, 20, 62, 30, 54, 22],
                   [3, 35, 11, 43, 1, 33, 9, 41],
                   [51, 19, 59, 27, 49, 17, 57, 25],
                   [15, 47, 7, 39, 13, 45, 5, 37],
                   [63, 31, 55, 23, 61, 29, 53, 21]], np.float32)


def read_pfm(path):
    """A little-endian RGB Portable Float Map -> (H, W, 3) float32, top row first"""
    blob = open(path, "rb").read()
    magic, size, scale, data = blob.split(b"\n", 3)
    assert magic == b"PF" and float(scale) < 0, (magic, scale)
    w, h = (int(v) for v in size.split())
    return np.frombuffer(data, "<f4").reshape(h, w, 3)[::-1].copy()


def read_png_rgb8(path):
    """An 8-bit RGB PNG whose scanlines all carry filter 0 (what the library's writer emits) -> (H, W, 3) uint8"""
    import struct
    import zlib
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        body = blob[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 2)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3).copy()


def params(**kw):
    p = dict(DEFAULTS)
    assert not set(kw) - set(p), sorted(set(kw) - set(p))
    p.update(kw)
    return p


def white_of(p):
    return float(p["white"]) if p["white"] > 0 else (11.2 if p["tone"] == TONE_HABLE else 4.0)


def scrub(rgb):
    """stage 0 on (..., 3) float32: (scrubbed, per-pixel flag of a non-finite component).  A component that is not finite
    or carries the sign bit becomes +0."""
    rgb = np.asarray(rgb, F)
    bad = ~np.isfinite(rgb)
    return np.where(bad | np.signbit(rgb), F(0), rgb).astype(F), bad.any(axis=-1)


def lum(rgb):
    """(0.2126 r + 0.7152 g) + 0.0722 b, float32, each operation rounded"""
    rgb = np.asarray(rgb, F)
    return ((F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]).astype(F)


def bin_of(y):
    """the histogram bin from the float's bits: clamp((bits >> 20) - 888, 0, 255); -1 for y <= 0 and NaN"""
    y = np.asarray(y, F)
    bits = y.view(np.uint32).astype(np.int64)
    k = np.clip((bits >> 20) - 888, 0, 255)
    return np.where(y > 0, k, -1).astype(np.int32)  # (NaN > 0 is false; +inf lands in bin 255)


def histogram(rgb):
    """(counts uint32[256], skipped, nonfinite) of a (..., 3) plane"""
    s, bad = scrub(rgb)
    k = bin_of(lum(s)).reshape(-1)
    return np.bincount(k[k >= 0], minlength=256).astype(np.uint32), int((k < 0).sum()), int(bad.sum())


def metering(hist, p):
    """(avg_log2, scale) in float64, scale rounded to float32 once"""
    h = np.asarray(hist, np.float64)
    T = h.sum()
    manual = F(2.0 ** float(F(p["exposure_ev"])))
    if T == 0:
        return 0.0, manual
    lo, hi = float(F(p["low_fraction"])) * T, (1.0 - float(F(p["high_fraction"]))) * T
    below = np.concatenate([[0.0], np.cumsum(h)[:-1]])
    ov = np.maximum(np.minimum(below + h, hi) - np.maximum(below, lo), 0.0)
    k = np.arange(256)
    L = np.floor(k / 8) - 16 + np.log2(1 + ((k % 8) + 0.5) / 8)
    mass = 0.0
    total = 0.0
    for i in range(256):  # the library's order of summation
        if h[i] and ov[i] > 0:
            mass += ov[i]
            total += ov[i] * L[i]
    if not mass > 0:
        return 0.0, manual
    avg = total / mass
    return avg, F(float(F(p["key"])) / 2.0 ** avg * 2.0 ** float(F(p["exposure_ev"])))


def bloom_levels_used(w, h, p):
    if p["bloom_levels"] <= 0 or p["bloom_strength"] <= 0:
        return 0
    return min(int(p["bloom_levels"]), int(np.floor(np.log2(min(w, h)))))


def _down(B):
    h, w = B.shape[:2]
    ys, xs = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    y0, y1 = np.minimum(2 * ys, h - 1), np.minimum(2 * ys + 1, h - 1)
    x0, x1 = np.minimum(2 * xs, w - 1), np.minimum(2 * xs + 1, w - 1)
    a, b = B[y0][:, x0], B[y0][:, x1]
    c, d = B[y1][:, x0], B[y1][:, x1]
    return (((a + b) + (c + d)) * F(0.25)).astype(F)


def _up2(C, h, w):
    hc, wc = C.shape[:2]
    x = np.arange(w)
    xi = x >> 1
    xn = np.clip(xi + np.where(x & 1, 1, -1), 0, wc - 1)
    R = (F(0.75) * C[:, xi] + F(0.25) * C[:, xn]).astype(F)  # rows
    y = np.arange(h)
    yi = y >> 1
    yn = np.clip(yi + np.where(y & 1, 1, -1), 0, hc - 1)
    return (F(0.75) * R[yi] + F(0.25) * R[yn]).astype(F)     # then columns


def bloom(c, p):
    """stage 2 on the exposed (H, W, 3) float32 plane"""
    h, w = c.shape[:2]
    K = bloom_levels_used(w, h, p)
    if K == 0:
        return c
    B = [c]
    for _ in range(K):
        B.append(_down(B[-1]))
    U = B[K]
    for l in range(K - 1, -1, -1):
        U = (B[l] + _up2(U, *B[l].shape[:2])).astype(F)
    bl = (U / F(K + 1)).astype(F)
    return (c + F(p["bloom_strength"]) * (bl - c)).astype(F)


def curve64(c, p):
    """stages 3 + 4 in float64 on exposed values (..., 3)"""
    c = np.asarray(c, np.float64)
    tone, W = p["tone"], white_of(p)
    with np.errstate(all="ignore"):
        if tone == TONE_REINHARD:
            L = (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]
            Ld = L * (1 + L / (W * W)) / (1 + L)
            k = np.where(L > 0, Ld / np.where(L > 0, L, 1.0), 0.0)
            t = c * k[..., None]
        elif tone == TONE_ACES:
            t = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14)
        elif tone == TONE_HABLE:
            A, B, Cc, D, E, Fh = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30

            def f(x):
                return (x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * Fh) - E / Fh
            t = f(2 * c) / f(W)
        else:
            t = c
        t = np.clip(t, 0.0, 1.0)
        if p["oetf"] == OETF_SRGB:
            t = np.where(t <= 0.0031308, 12.92 * t, 1.055 * t ** (1 / 2.4) - 0.055)
        elif p["oetf"] == OETF_GAMMA22:
            t = t ** (1 / 2.2)
    return np.clip(t, 0.0, 1.0)


def quantise(out, p):
    """stage 5 on the float output (H, W, >= 3) float32 -> (H, W, 4) uint8"""
    v = np.asarray(out, F)[..., :3]
    h, w = v.shape[:2]
    q = p["quantiser"]
    if q == QUANT_ROUND:
        bias = np.full((h, w), 0.5, F)
    elif q == QUANT_DITHER:
        yy, xx = np.meshgrid(np.arange(h) & 7, np.arange(w) & 7, indexing="ij")
        bias = ((BAYER8[yy, xx] + F(0.5)) / F(64)).astype(F)
    else:
        bias = np.zeros((h, w), F)
    t = (v * F(255)).astype(F)
    u = (t + bias[..., None]).astype(F)
    rgb = np.floor(np.minimum(u, F(255))).astype(np.uint8)
    return np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=-1)


def exposed(plane, p):
    """stages 0 - 2: (the exposed and bloomed (H, W, 3) float32 plane, info dict with histogram, counted, skipped,
    nonfinite, avg_log2, scale, levels)"""
    rgb = np.asarray(plane, F)[..., :3]
    s, bad = scrub(rgb)
    info = dict(histogram=np.zeros(256, np.uint32), counted=0, skipped=0, nonfinite=int(bad.sum()), avg_log2=0.0)
    if p["auto_exposure"]:
        info["histogram"], info["skipped"], _ = histogram(rgb)
        info["counted"] = int(info["histogram"].sum())
        info["avg_log2"], scale = metering(info["histogram"], p)
    else:
        scale = F(2.0 ** float(F(p["exposure_ev"])))
    info["scale"] = F(scale)
    info["levels"] = bloom_levels_used(rgb.shape[1], rgb.shape[0], p)
    c = (F(scale) * s).astype(F)
    return bloom(c, p), info


def display(plane, p):
    """the whole transform: (float output (H, W, 4) in float64 precision of the curves, info).  The bytes are
    quantise() of a float32 plane: the caller decides which (the device's own, for the byte-exact check)."""
    c, info = exposed(plane, p)
    o = curve64(c, p)
    return np.concatenate([o, np.ones(o.shape[:-1] + (1,))], axis=-1), info
