"""numpy restatement of the participating medium (include/dmt_hip.h dmt_set_medium) and the scenes of its
tests.

Three layers.  medium_u and the clip are exact: integer arithmetic, and float32 operations in the stated order with the
reciprocal correctly rounded (numpy's float32 division), so they give the device's and the host twins' values bit for bit.
The phase function, the transmittance and the free flight are float64: what the fp32 code approximates.  The camera rays
build on lens_ref's sampler and camera matrices, vectorised in float64 (the film jitter to ~1e-9 of a pixel, which only
feeds statistical checks and a 1e-5 bound).
"""
import numpy as np

import lens_ref as LR

F = np.float32
PARALLEL = F(2.0) ** -100


# ---- exact: the free-flight number and the clip --------------------------------------------------------------
def medium_u(h, depth):
    x = LR.mix_bits32(int(h) ^ LR.mix_bits32((0x9E3779B9 * (int(depth) + 1)) & LR.M32))
    return F(x >> 8) * F(2.0 ** -24)


def segment_f32(lo, hi, o, d, t_hit):
    """one ray; returns (t0, t1, hit) as dmt_medium_segment states the arithmetic"""
    lo, hi, o, d = (np.asarray(a, F) for a in (lo, hi, o, d))
    t0, t1, outside = F(0), F(t_hit), False
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            if abs(d[a]) < PARALLEL:
                outside = outside or bool(o[a] < lo[a]) or bool(o[a] > hi[a])
                continue
            inv = F(1) / d[a]
            ta, tb = F(F(lo[a] - o[a]) * inv), F(F(hi[a] - o[a]) * inv)
            tn, tf = (ta, tb) if ta < tb else (tb, ta)
            t0 = tn if tn > t0 else t0
            t1 = tf if tf < t1 else t1
    if outside:
        t1 = t0
    return t0, t1, bool(t0 < t1)


# ---- float64: what the fp32 code approximates -------------------------------------------------------------------
def hg64(g, c):
    """p_HG(c), c = dot(wo, wi), from the float32 inputs taken as exact"""
    g, c = float(F(g)), np.asarray(c, F).astype(np.float64)
    return (1.0 - g * g) / (4.0 * np.pi * (1.0 + g * g + 2.0 * g * c) ** 1.5)


def clip64(lo, hi, o, d, t_end):
    """vectorised float64 clip of rays (o, d: [n, 3]) against the box, intersected with [0, t_end]: (t0, t1), empty where
    t0 >= t1.  Rays of the test scenes have no zero direction component."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    t0 = np.maximum(np.minimum(ta, tb).max(-1), 0.0)
    t1 = np.minimum(np.maximum(ta, tb).min(-1), t_end)
    return t0, t1


def length64(lo, hi, o, d, t_end):
    t0, t1 = clip64(lo, hi, o, d, t_end)
    return np.maximum(t1 - t0, 0.0)


# ---- the camera rays of whole pixels, vectorised ------------------------------------------------------------------
def _radical_inverse(base, idx):
    idx = np.asarray(idx, np.int64).copy()
    out, scale = np.zeros(idx.shape), 1.0 / base
    while (idx > 0).any():
        out += (idx % base) * scale
        idx //= base
        scale /= base
    return out


def camera_rays64(camera44, pxs, pys, ss):
    """float64 pinhole rays (o [n, 3], d [n, 3]) and Halton indices [n] of samples ss of pixels (pxs, pys), as
    lens_ref.rays64 with radius 0"""
    xf = LR.camera_xf(camera44)
    p = LR.halton_params(xf["width"], xf["height"])
    pxs, pys, ss = (np.asarray(a, np.int64) for a in (pxs, pys, ss))
    base = np.zeros(pxs.shape, np.int64)
    for key in set(zip(pxs.tolist(), pys.tolist())):
        base[(pxs == key[0]) & (pys == key[1])] = LR.halton_index(p, key[0], key[1], 0)
    h = base + ss * (p["scale0"] * p["scale1"])
    a = h >> p["exp0"]
    rev = np.zeros(a.shape, np.int64)
    for bit in range(32):
        rev |= ((a >> bit) & 1) << (31 - bit)
    fx = rev * 2.0 ** -32 + pxs
    fy = _radical_inverse(3, h // p["scale1"]) + pys
    right, up, fwd, pos = (xf[k].astype(np.float64) for k in ("right", "up", "fwd", "pos"))
    pcx = float(xf["psx"]) * fx + float(xf["tx"])
    pcy = -float(xf["psy"]) * fy + float(xf["ty"])
    v = pcx[:, None] * right + pcy[:, None] * up + float(xf["focal"]) * fwd
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.broadcast_to(pos, d.shape).copy(), d, h


def pixel_samples(w, h, spp):
    """every sample 0..spp-1 of every pixel of a w x h film: (pxs, pys, ss) int32, pixel-major"""
    yy, xx, kk = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xx.reshape(-1).astype(np.int32), yy.reshape(-1).astype(np.int32), kk.reshape(-1).astype(np.int32)


# ---- scenes (z is up: the camera's up vector is derived from +z) ------------------------------------------------
LIGHT_POS = np.array([0.25, 2.5, 5.0])
CAM_POS = np.array([0.0, 0.0, 1.0])
SLAB = ((-30.0, -30.0, 2.0), (30.0, 30.0, 3.0))      # between the floor (z = 0) and the light, above the camera: no camera ray enters it
ROOM = ((-30.0, -30.0, -1.0), (30.0, 30.0, 6.0))     # holds the camera, the floor's visible part and the light


def camera(res, pos=CAM_POS, direction=(0.0, 1.0, -0.6), focal=50.0, sensor=36.0):
    """a DeviceCamera record; with focal 50 the half angle is 19.8 degrees, so every ray of the default camera points
    between 11 and 51 degrees below the horizon"""
    cam = np.zeros(11, F)
    cam[0:3], cam[3:6], cam[9], cam[10] = direction, pos, focal, sensor
    cam.view(np.int32)[6:9] = (res, res, 1)
    return cam.view(np.uint8)


def _soup(tris):
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    return tuple(np.concatenate([T[:, :, k], np.zeros((T.shape[0], 1), F)], 1) for k in range(3))


def floor_scene(O, res, intensity=40.0):
    """a matte floor quad at z = 0 under a point light of radius 0 (a delta light: sampled towards its centre), a camera
    one unit above the floor looking down at it, no infinite light"""
    q = np.array([[-20, -4, 0], [20, -4, 0], [20, 16, 0], [-20, 16, 0]], F)
    xs, ys, zs = _soup([(q[0], q[1], q[2]), (q[0], q[2], q[3])])
    light = O.make_point_light((intensity,) * 3, LIGHT_POS.astype(F), 0.0)
    none = np.zeros((0, 32), np.uint8)
    return O.Scene(xs, ys, zs, np.zeros(2, np.uint32), O.make_oren_nayar((0.7, 0.7, 0.7), 0.5)[None], light[None], none, camera(res))


VOID_LIGHT = np.array([0.4, 1.5, 1.9])  # inside VOID_BOX; see void_scene


def void_scene(O, res, light=True, env=False):
    """nothing to see: one tiny triangle far behind the camera (a scene needs a triangle), a camera at the origin looking
    along +y.  light: a radius-0 point light at VOID_LIGHT, above the view frustum (half angle 19.8 degrees; the light is
    51 degrees up), so every camera ray passes it at more than 0.5 units.  env: one constant infinite light of radiance 1."""
    xs, ys, zs = _soup([((0, -1000, 0), (1e-3, -1000, 0), (0, -1000, 1e-3))])
    none = np.zeros((0, 32), np.uint8)
    lights = O.make_point_light((8.0,) * 3, VOID_LIGHT.astype(F), 0.0)[None] if light else none
    inf = O.make_env_light((1.0, 1.0, 1.0))[None] if env else none
    cam = camera(res, pos=(0.0, 0.0, 0.0), direction=(0.0, 1.0, 0.0))
    return O.Scene(xs, ys, zs, np.zeros(1, np.uint32), O.make_oren_nayar((0.7, 0.7, 0.7), 0.5)[None], lights, inf, cam)


VOID_BOX = ((-2.0, 0.5, -2.0), (2.0, 3.5, 2.0))     # in front of the camera: camera rays enter at y = 0.5
FURNACE_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))  # around the camera; optical depth 2 across a side at sigma_t = 1


def light_intensity(light32):
    """the rgb intensity of a packed light record (fp16 x 3)"""
    return np.ascontiguousarray(light32, np.uint8).reshape(32)[:6].view(np.float16).astype(np.float64)


def floor_shadow(o, d):
    """where camera rays (float64) meet the floor z = 0, and their shadow rays to the light: (t_hit, P, unit direction to
    the light, distance)"""
    t = -o[:, 2] / d[:, 2]
    P = o + t[:, None] * d
    v = LIGHT_POS - P
    dist = np.linalg.norm(v, axis=1)
    return t, P, v / dist[:, None], dist
