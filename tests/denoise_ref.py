"""numpy restatement of dmt_denoise: spatial SVGF, i.e. the edge-avoiding a-trous wavelet filter of
Dammertz et al. 2010 with the variance-guided luminance term of Schied et al. 2017, on the first-hit feature buffers of
dmt_render_aovs.

Every quantity is float32 and every expression is evaluated in the order the device kernels (k_denoise_init, k_atrous in
csrc/denoise.hpp) evaluate it, so the GPU's output matches this module to the rounding of exp / pow / sqrt / division.
The AOVs are not packed (fp32 planes), so nothing here has to mirror a quantisation.
"""
import numpy as np

F = np.float32
H5 = (F(1 / 16), F(0.25), F(0.375), F(0.25), F(1 / 16))   # a-trous kernel h(dx), dx = -2 .. 2
B3 = (F(0.25), F(0.5), F(0.25))                           # variance blur, dx = -1 .. 1
LUM = (F(0.2126), F(0.7152), F(0.0722))                   # Rec. 709 luminance
DEFAULTS = dict(iterations=4, sigma_normal=128.0, sigma_position=1.0, sigma_albedo=0.1, sigma_luminance=32.0)  # dmt_denoise_defaults


def theta(camera44):
    """one pixel's angle: sensor height / (focal length * image height), from the 44-byte dmt_camera"""
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    height = F(cam[28:32].view(np.int32)[0])
    focal, sensor = cam[36:40].view(np.float32)[0], cam[40:44].view(np.float32)[0]
    return F(sensor / (focal * height))


def initial(mean, m2):
    """c0 = mean.xyz, v0 = (M2.x + M2.y + M2.z) / (3 N (N - 1)), and the mask of the pixels dmt_denoise refuses"""
    mean, m2 = np.asarray(mean, F), np.asarray(m2, F)
    n = m2[..., 3]
    with np.errstate(all="ignore"):
        v = ((m2[..., 0] + m2[..., 1]) + m2[..., 2]) / ((F(3) * n) * (n - F(1)))
    bad = ~(n >= 2) | ~np.isfinite(mean[..., :3]).all(-1) | ~np.isfinite(m2).all(-1)
    return mean[..., :3].copy(), v.astype(F), bad


def _shift(a, oy, ox):
    """a[p + (oy, ox)] for every pixel p, and whether that tap lies inside the image (zeros outside)"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        ok[y0:y1, x0:x1] = True
    return out, ok


def luminance(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def tap_weights(c, v, albedo, normal, position, step, th, sigma_normal, sigma_position, sigma_albedo, sigma_luminance):
    """the 25 weights of one pass, {(dx, dy): H x W array}; 0 where a tap is skipped (outside the image, no coverage)"""
    albedo, normal, position = np.asarray(albedo, F), np.asarray(normal, F), np.asarray(position, F)
    sn, sx, sa, sl, th = F(sigma_normal), F(sigma_position), F(sigma_albedo), F(sigma_luminance), F(th)
    h_p = albedo[..., 3] > 0
    n_p, x_p, a_p = normal[..., :3], position[..., :3], albedo[..., :3]
    gs, gw = np.zeros_like(v), np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, ok = _shift(v, dy, dx)
            kk = B3[dx + 1] * B3[dy + 1]
            gs = np.where(ok, gs + kk * vq, gs)
            gw = np.where(ok, gw + kk, gw)
    l_p = luminance(c)
    with np.errstate(all="ignore"):
        lden = sl * np.sqrt(gs / gw) + F(1e-10)
        xden = (sx * position[..., 3]) * th
    a2 = sa * sa
    weights = {}
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            kk = H5[dx + 2] * H5[dy + 2]
            if dx == 0 and dy == 0:
                weights[(dx, dy)] = np.full_like(v, kk)
                continue
            oy, ox = dy * step, dx * step
            aq, ok = _shift(albedo, oy, ox)
            nq, _ = _shift(normal, oy, ox)
            xq, _ = _shift(position, oy, ox)
            cq, _ = _shift(c, oy, ox)
            ok = ok & (aq[..., 3] > 0) & h_p
            with np.errstate(all="ignore"):
                nd = (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]
                wn = np.power(np.maximum(F(0), nd), sn)
                d = xq[..., :3] - x_p
                pd = np.abs((n_p[..., 0] * d[..., 0] + n_p[..., 1] * d[..., 1]) + n_p[..., 2] * d[..., 2])
                dist = F(step) * np.sqrt(F(dx * dx + dy * dy))
                wx = np.exp(-pd / (xden * dist))
                da = a_p - aq[..., :3]
                wa = np.exp(-((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) / a2)
                wl = np.exp(-np.abs(l_p - luminance(cq)) / lden)
                w = (((kk * wn) * wx) * wa) * wl
            weights[(dx, dy)] = np.where(ok, w, F(0)).astype(F)
    return weights


def atrous_pass(c, v, albedo, normal, position, step, th, sigma_normal, sigma_position, sigma_albedo, sigma_luminance):
    """one pass at step s = `step`: (c_{i+1}, v_{i+1}); pixels without coverage pass through"""
    weights = tap_weights(c, v, albedo, normal, position, step, th, sigma_normal, sigma_position, sigma_albedo, sigma_luminance)
    sw, sc, sv = np.zeros_like(v), np.zeros_like(c), np.zeros_like(v)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            w = weights[(dx, dy)]
            cq, ok = _shift(c, dy * step, dx * step)
            vq, _ = _shift(v, dy * step, dx * step)
            sw = sw + w
            sc = sc + w[..., None] * cq
            sv = sv + (w * w) * vq
    with np.errstate(all="ignore"):
        c1 = sc / sw[..., None]
        v1 = sv / (sw * sw)
    h_p = np.asarray(albedo, F)[..., 3] > 0
    return np.where(h_p[..., None], c1, c).astype(F), np.where(h_p, v1, v).astype(F)


def denoise(mean, m2, albedo, normal, position, th, iterations=DEFAULTS["iterations"], sigma_normal=DEFAULTS["sigma_normal"],
            sigma_position=DEFAULTS["sigma_position"], sigma_albedo=DEFAULTS["sigma_albedo"],
            sigma_luminance=DEFAULTS["sigma_luminance"]):
    """the denoised image, H x W x 4 float32 with w = 1 (dmt_denoise's out4)"""
    c, v, bad = initial(mean, m2)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} pixels have N < 2 or a non-finite mean / M2")
    for i in range(iterations):
        c, v = atrous_pass(c, v, albedo, normal, position, 1 << i, th, sigma_normal, sigma_position, sigma_albedo, sigma_luminance)
    out = np.ones(c.shape[:2] + (4,), F)
    out[..., :3] = c
    return out
