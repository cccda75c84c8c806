"""numpy restatement of the pixel filter (include/dmt_hip.h dmt_set_pixel_filter).

Two layers, as in lens_ref.py.  The analytic side is float64: each kind's 1-D profile over w = x / radius in [-1, 1], its
normalised density and CDF in closed form, written here from the filters' definitions and independent of the library's
integration.  The sampling side is exact: the warp r' = 0.5 + radius * W(r) of a sample's film jitter through a table of 257
float32 knots, with the one fmaf as exact rational arithmetic rounded once, and the film position formed from r' as
lens_ref.film_position forms it from r, which give the host twin's and the device's values bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

import lens_ref as LR

F = np.float32
BOX, TENT, GAUSSIAN, BLACKMAN_HARRIS = 0, 1, 2, 3
KNOTS = 257

# the filters of the tests: (kind, radius, param); pbrt-v4's defaults for the tent and the Gaussian
FILTERS = {
    "box1": (BOX, 1.0, 0.0),
    "tent": (TENT, 2.0, 0.0),
    "gaussian": (GAUSSIAN, 1.5, 0.5),
    "gaussian2": (GAUSSIAN, 2.0, 0.5),
    "blackman-harris": (BLACKMAN_HARRIS, 2.0, 0.0),
}
GAUSS = FILTERS["gaussian"]

_BH = (0.35875, 0.48829, 0.14128, 0.01168)


# ---- the analytic filters, float64 -----------------------------------------------------------------
def _raw_pdf(kind, radius, param, w):
    """the profile f1(radius w), not normalised"""
    w = np.asarray(w, np.float64)
    if kind == BOX:
        return np.ones_like(w)
    if kind == TENT:
        return 1.0 - np.abs(w)
    if kind == GAUSSIAN:  # pbrt-v4: max(0, G(x) - G(radius)); the common factor 1 / sqrt(2 pi sigma^2) drops out
        s = float(F(param)) / float(F(radius))
        return np.maximum(0.0, np.exp(-w * w / (2 * s * s)) - math.exp(-1.0 / (2 * s * s)))
    t = 0.5 * (w + 1.0)
    a0, a1, a2, a3 = _BH
    return a0 - a1 * np.cos(2 * np.pi * t) + a2 * np.cos(4 * np.pi * t) - a3 * np.cos(6 * np.pi * t)


def _raw_cdf(kind, radius, param, w):
    """the integral of _raw_pdf from -1 to w, in closed form"""
    w = np.asarray(w, np.float64)
    if kind == BOX:
        return w + 1.0
    if kind == TENT:
        return np.where(w <= 0, 0.5 * (1 + w) ** 2, 1.0 - 0.5 * (1 - w) ** 2)
    if kind == GAUSSIAN:
        s = float(F(param)) / float(F(radius))
        a = 1.0 / (s * math.sqrt(2.0))
        erf = np.vectorize(math.erf)
        return s * math.sqrt(math.pi / 2) * (erf(a * w) + math.erf(a)) - math.exp(-1.0 / (2 * s * s)) * (w + 1.0)
    t = 0.5 * (w + 1.0)
    a0, a1, a2, a3 = _BH
    return 2.0 * (a0 * t - a1 * np.sin(2 * np.pi * t) / (2 * np.pi) + a2 * np.sin(4 * np.pi * t) / (4 * np.pi)
                  - a3 * np.sin(6 * np.pi * t) / (6 * np.pi))


def cdf(kind, radius, param, w):
    """the normalised analytic CDF over w in [-1, 1]"""
    return _raw_cdf(kind, radius, param, w) / float(_raw_cdf(kind, radius, param, 1.0))


def pdf_max(kind, radius, param):
    """the largest normalised density (every profile here peaks at w = 0)"""
    return float(_raw_pdf(kind, radius, param, 0.0)) / float(_raw_cdf(kind, radius, param, 1.0))


def warp64(knots, u):
    """W(u) of the tabulated filter in float64 (for the between-knot deviation, which is not a bitwise matter)"""
    k = np.asarray(knots, np.float64)
    s = np.asarray(u, np.float64) * 256.0
    i = np.minimum(s.astype(np.int64), 255)
    return k[i] + (s - i) * (k[i + 1] - k[i])


def between_knot_deviation(kind, radius, param, knots, per_bin=64):
    """max over a fine grid of u of |analytic CDF(W_table(u)) - u|: how far the rendered (tabulated) filter is from the
    analytic one"""
    u = (np.arange(256 * per_bin) + 0.5) / (256 * per_bin)
    return float(np.abs(cdf(kind, radius, param, warp64(knots, u)) - u).max())


# ---- the warp and the film position, exact -----------------------------------------------------------
def _round_signed(q):
    q = Fraction(q)
    if q == 0:
        return F(0)
    return LR.round_f32(q) if q > 0 else F(-LR.round_f32(-q))


def warp(knots, radius, u):
    """r' = 0.5 + radius * W(u), float32 as filter_warp (csrc/pt_device.hpp) computes it: 256 u and its fraction are exact,
    one float32 difference of knots, one fmaf, one product, one sum"""
    u = F(u)
    s = F(u * F(256))
    assert Fraction(float(s)) == Fraction(float(u)) * 256
    i = min(int(s), 255)
    t = F(s - F(i))
    assert Fraction(float(t)) == Fraction(float(s)) - i
    d = F(F(knots[i + 1]) - F(knots[i]))
    w = _round_signed(Fraction(float(t)) * Fraction(float(d)) + Fraction(float(F(knots[i]))))
    return F(F(0.5) + F(F(radius) * w))


def film_coord(r, p):
    return F(F(F(F(r) - F(0.5)) + F(0.5)) + F(p))


def positions(w, h, knots, radius, pxs, pys, ss):
    """film positions [n, 2] of the cases under the tabulated filter (knots None: unfiltered, lens_ref.film_position)"""
    p = LR.halton_params(w, h)
    out = np.zeros((len(pxs), 2), F)
    for k, (px, py, s) in enumerate(zip(pxs, pys, ss)):
        hidx = LR.halton_index(p, int(px), int(py), int(s))
        if knots is None:
            out[k] = LR.film_position(p, int(px), int(py), hidx)
        else:
            rx, ry = LR.pixel2d(p, hidx)
            out[k] = film_coord(warp(knots, radius, rx), int(px)), film_coord(warp(knots, radius, ry), int(py))
    return out


def jitter(w, h, pxs, pys, ss):
    """the unwarped jitter [n, 2] of the cases, exact"""
    p = LR.halton_params(w, h)
    return np.array([LR.pixel2d(p, LR.halton_index(p, int(px), int(py), int(s))) for px, py, s in zip(pxs, pys, ss)], F)
