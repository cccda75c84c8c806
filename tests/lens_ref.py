"""numpy restatement of the thin-lens camera (include/dmt_hip.h dmt_set_lens).

Two layers.  The sampler side is exact: the Halton index of (pixel, sample), the film jitter and the Owen-scrambled radical
inverse are integer arithmetic plus one fmaf per digit, and the fmaf is emulated in exact rational arithmetic rounded once
to float32, so these functions give the device's and the host twin's values bit for bit.  The ray side is float64 on the
float32 camera matrices of dmt_set_camera: what the fp32 code approximates, fed the exact lens values and film positions.

`e_host` is the measured distance between the host twin (dmt_lens_rays) and that float64 restatement over CASES; the
tolerances of the lens tests are multiples of it (see measure_e_host).
"""
import functools
from fractions import Fraction

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
ONE_MINUS_EPS = F(0.99999994)


# ---- exact float32 helpers -------------------------------------------------------------------------
def round_f32(q):
    """A non-negative rational rounded once to the nearest float32, ties to even (normal range)."""
    q = Fraction(q)
    if q == 0:
        return F(0)
    assert q > 0
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and e > -120
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    k = n.numerator // n.denominator
    r = n - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and (k & 1)):
        k += 1
    v = F(float(k * ulp))  # k ulp has at most 25 significant bits only when it carried to 2^24: exact in double, and in float32
    assert Fraction(float(v)) == k * ulp
    return v


def fmaf(a, b, c):
    """fmaf(a, b, c) for non-negative float32 arguments: the exact a b + c rounded once."""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def mix_bits32(v):
    v &= M32
    v ^= v >> 16
    v = (v * 0x7FEB352D) & M32
    v ^= v >> 15
    v = (v * 0x846CA68B) & M32
    v ^= v >> 16
    return v


def owen_seed(dim):
    return mix_bits32(1 + (dim << 4))


def owen_radical_inverse(base, seed, index):
    """The reference's scrambled radical inverse as its loop is written: per digit mix_bits32(seed ^ prefix), the 32-bit
    wrapping sum, the digit modulo the base, fmaf; digit 0 has the empty prefix; clamped below 1."""
    inv_base = F(1) / F(base)
    result, inv_pow, rev = F(0), inv_base, 0
    index = int(index)
    while index > 0:
        nxt, digit = divmod(index, base)
        s = (digit + mix_bits32(seed ^ rev)) & M32
        result = fmaf(F(s % base), inv_pow, result)
        rev = (rev * base + digit) & M32
        inv_pow = F(inv_pow * inv_base)
        index = nxt
    return min(result, ONE_MINUS_EPS)


def radical_inverse(base, index):
    inv_base = F(1) / F(base)
    result, inv_pow = F(0), inv_base
    index = int(index)
    while index > 0:
        nxt, digit = divmod(index, base)
        result = fmaf(F(digit), inv_pow, result)
        inv_pow = F(inv_pow * inv_base)
        index = nxt
    return min(result, ONE_MINUS_EPS)


def lens_values(h):
    """(u10, u11) of Halton index h: dimensions 10 and 11, bases 31 and 37"""
    return owen_radical_inverse(31, owen_seed(10), h), owen_radical_inverse(37, owen_seed(11), h)


# ---- the sampler's index and film jitter -----------------------------------------------------------
def halton_params(w, h):
    out = []
    for res, base in ((w, 2), (h, 3)):
        scale, ex = 1, 0
        while scale < min(res, 128):
            scale, ex = scale * base, ex + 1
        out.append((scale, ex))
    (s0, e0), (s1, e1) = out
    return dict(scale0=s0, exp0=e0, scale1=s1, exp1=e1, inv0=pow(s1, -1, s0) if s0 > 1 else 0, inv1=pow(s0, -1, s1) if s1 > 1 else 0)


def halton_index(p, px, py, s):
    stride = p["scale0"] * p["scale1"]

    def inv_radical(v, base, digits):
        r = 0
        for _ in range(digits):
            r, v = r * base + v % base, v // base
        return r

    idx = inv_radical(px % 128, 2, p["exp0"]) * (stride // p["scale0"]) * p["inv0"]
    idx += inv_radical(py % 128, 3, p["exp1"]) * (stride // p["scale1"]) * p["inv1"]
    return idx % stride + s * stride


def pixel2d(p, h):
    a = h >> p["exp0"]
    rev = int("{:032b}".format(a)[::-1], 2)
    rx = min(F(F(rev) * F(2.3283064365386963e-10)), ONE_MINUS_EPS)
    return rx, radical_inverse(3, h // p["scale1"])


# ---- the rays, float64 -----------------------------------------------------------------------------
def camera_fields(camera44):
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    f, i = cam.view(np.float32), cam.view(np.int32)
    return f[0:3].copy(), f[3:6].copy(), int(i[6]), int(i[7]), F(f[9]), F(f[10])


def camera_xf(camera44):
    """dmt_set_camera's two matrices as float32 values (the host code's expressions): right / up / fwd / pos and the
    camera-from-raster entries psx, psy, tx, ty, focal"""
    d, pos, w, h, focal_mm, sensor_mm = camera_fields(camera44)

    def normalize(v):
        inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return np.array([v[0] * inv, v[1] * inv, v[2] * inv], F)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)

    fwd = normalize(d.astype(F))
    right = normalize(cross(fwd, np.array([0, 0, 1], F)))
    up = cross(right, fwd)
    mm = F(0.001)
    sensor_w = sensor_mm * F(w) / F(h)
    focal, sh, sw = focal_mm * mm, sensor_mm * mm, sensor_w * mm
    psx, psy = sw / F(w), sh / F(h)
    return dict(right=right, up=up, fwd=fwd, pos=pos.astype(F), focal=F(focal), psx=F(psx), psy=F(psy),
                tx=F(F(-0.5) * sw + F(0.5) * psx), ty=F(F(0.5) * sh - F(0.5) * psy), width=w, height=h)


def sample_uniform_disk64(u0, u1):
    """sample_uniform_disk (csrc/pt_device.hpp; the 3 pi / 4 branch is the reference's) in float64"""
    a, b = 2.0 * float(u0) - 1.0, 2.0 * float(u1) - 1.0
    if a == 0.0 and b == 0.0:
        return 0.0, 0.0
    if abs(a) > abs(b):
        rho, phi = a, (np.pi / 4) * (b / a)
    else:
        rho, phi = b, (3 * np.pi / 4) * (a / b)
    return rho * np.cos(phi), rho * np.sin(phi)


def film_position(p, px, py, h):
    """(fx, fy) of the sample, float32 as camera_ray_jittered forms it"""
    rx, ry = pixel2d(p, h)
    return F(F(F(rx - F(0.5)) + F(0.5)) + F(px)), F(F(F(ry - F(0.5)) + F(0.5)) + F(py))


def lens_ray64(xf, fx, fy, R, D, u):
    """the section-1 formulas of the issue in float64: returns (o, d, l) with l the lens offset in the lens plane"""
    right, up, fwd, pos = (xf[k].astype(np.float64) for k in ("right", "up", "fwd", "pos"))
    pc = np.array([float(xf["psx"]) * float(fx) + float(xf["tx"]), -float(xf["psy"]) * float(fy) + float(xf["ty"]), float(xf["focal"])])
    R, D = float(F(R)), float(F(D))  # the library takes them as float32
    if R > 0:
        ft = D / pc[2]
        pf = np.array([pc[0] * ft, pc[1] * ft, D])
        dx, dy = sample_uniform_disk64(*u)
        l = np.array([R * dx, R * dy])
    else:
        pf, l = pc, np.zeros(2)
    o = pos + right * l[0] + up * l[1]
    v = right * (pf[0] - l[0]) + up * (pf[1] - l[1]) + fwd * pf[2]
    return o, v / np.sqrt(v @ v), l


def rays64(camera44, R, D, pxs, pys, ss):
    """float64 rays of the cases, fed the exact lens values and film positions: (o [n, 3], d [n, 3], lens2 [n, 2] float32,
    halton indices [n])"""
    xf = camera_xf(camera44)
    p = halton_params(xf["width"], xf["height"])
    n = len(pxs)
    o, d, u2, hs = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 2), F), np.zeros(n, np.int64)
    for i, (px, py, s) in enumerate(zip(pxs, pys, ss)):
        h = halton_index(p, int(px), int(py), int(s))
        u = lens_values(h)
        fx, fy = film_position(p, int(px), int(py), h)
        o[i], d[i], _ = lens_ray64(xf, fx, fy, R, D, u)
        u2[i], hs[i] = u, h
    return o, d, u2, hs


# ---- the cases of the lens tests -------------------------------------------------------------------
LENS_R, LENS_D = 0.05, 2.5   # scene units; the Cornell box's back wall is at depth 4
FRAMES = ((64, 64), (48, 32))


def cases(w, h, n=256, seed=11):
    """n cases of a w x h frame; s up to 4095 so that every digit position of bases 31 and 37 occurs (31^2 = 961 < 4096 x
    stride), with sample 4095 and the frame's corners among them"""
    rng = np.random.default_rng(seed + w)
    px, py = rng.integers(0, w, n), rng.integers(0, h, n)
    s = rng.integers(0, 4096, n)
    px[:4], py[:4], s[:4] = (0, w - 1, 0, w - 1), (0, 0, h - 1, h - 1), (0, 4095, 4095, 1)
    return px.astype(np.int32), py.astype(np.int32), s.astype(np.int32)


def origin_scale(camera44, R):
    """what a deviation of a ray origin is measured against: the larger of |camera position| and the lens radius"""
    return max(float(np.abs(camera_fields(camera44)[1]).max()), float(R))


@functools.lru_cache(maxsize=None)
def _measure(lens_rays, cams):
    e = 0.0
    for (w, h), cam in zip(FRAMES, cams):
        cam = np.frombuffer(cam, np.uint8)
        px, py, s = cases(w, h)
        o, d, _ = lens_rays(cam, LENS_R, LENS_D, px, py, s)
        o64, d64, _, _ = rays64(cam, LENS_R, LENS_D, px, py, s)
        e = max(e, float(np.abs(d - d64).max()), float(np.abs(o - o64).max()) / origin_scale(cam, LENS_R))
    return e


def measure_e_host(pkg, cams):
    """e_host: the largest deviation of dmt_lens_rays from the float64 restatement over the 512 cases -- of a direction
    component, or of an origin component relative to origin_scale.  Measured, not fixed in advance (DESIGN.md 4.13 records
    the value)."""
    return _measure(pkg.lens_rays, tuple(np.ascontiguousarray(c, np.uint8).tobytes() for c in cams))
