"""numpy restatement of the first-hit texture filter (DMT_TEXFILTER_REFERENCE) for the tests.

Restates the reference's CPU renderer (paths relative to its src/core/):
  MIP chain      private/core-texture.cu:340-540   makeRGBMipmappedTexture (level count, 2x2 box average, toByte)
  footprint      private/core-render.cpp:928-980   minDifferentialsFromCamera (512 rays along the film diagonal)
  dp/dxy         private/core-texture.cu:55-87     approximate_dp_dxy (+ Transform::rotateFromTo,
                                                   private/cudautils/cudautils-transform.cu:87-147)
  dp/du, dp/dv   private/core-render.cpp:209-226
  duv            private/core-texture.cu:123-258   duv_From_dp_dxy, the #else branch
  zeroing        private/core-render.cpp:264-268
  lookup         private/core-material.cpp:20-175  sampleBilinearTexel, sampleTrilinear, sampleMippedTexture
  EWA            private/core-texture.cu:595-748   computeTextureLOD_from_dudv, EWAFormula
and the build's [fix 1-5] (csrc/dmt_hip.hip).  The per-hit differentials are evaluated in double and the lookups in float32,
each in the device code's order of operations, so that the tests can compare the GPU's probes against them; `margin`
values say how far a probe is from the thresholds where one float rounding would change a discrete decision.
"""
import math

import numpy as np

F = np.float32
EWA_LUT_SIZE = 128
EWA_MAX_TEXELS = 1024.0   # [fix 4]
MAX_ANISOTROPY = 8.0      # core-texture.h:210
FLT_EPSILON = float(np.finfo(np.float32).eps)


def ewa_lut():
    """exp(-2 i / 127) - exp(-2), rounded to float (tools/gen_ewa_lut.py)."""
    return np.array([math.exp(-2.0 * i / (EWA_LUT_SIZE - 1)) - math.exp(-2.0) for i in range(EWA_LUT_SIZE)], np.float32)


LUT = ewa_lut()


# ---- MIP chain ------------------------------------------------------------------------------------------------------
def mip_level_count(w, h):
    n = 0
    while w > 0 or h > 0:
        n, w, h = n + 1, w >> 1, h >> 1
    return n


def mip_chain(img):
    """img: (h, w, 4) uint8 -> [level 0, level 1, ...] (each (max(1, h >> l), max(1, w >> l), 4) uint8).  Texel = the
    float average of the 2x2 parent block (c00 + c10 + c01 + c11, left to right, times 0.25), toByte-truncated; [fix 1]
    where a parent axis has one texel, the 1x2 / 2x1 block that exists (times 0.5); other than power-of-two sides drop
    the last odd row / column of a level."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    levels = [img]
    for l in range(1, mip_level_count(w, h)):
        prev = levels[-1].astype(np.float32) / F(255)
        ph, pw = prev.shape[:2]
        ch, cw = max(1, h >> l), max(1, w >> l)
        x1, y1 = pw >= 2, ph >= 2
        s = prev[0:2 * ch:2, 0:2 * cw:2][:ch, :cw]
        if x1:
            s = s + prev[0:2 * ch:2, 1:2 * cw:2][:ch, :cw]
        if y1:
            s = s + prev[1:2 * ch:2, 0:2 * cw:2][:ch, :cw]
        if x1 and y1:
            s = s + prev[1:2 * ch:2, 1:2 * cw:2][:ch, :cw]
        scale = F(0.25) if (x1 and y1) else F(0.5) if (x1 or y1) else F(1)
        t = (scale * s) * F(255)
        levels.append(np.clip(t, F(0), F(255)).astype(np.uint8))
    return levels


# ---- camera ------------------------------------------------------------------------------------------------------------
def parse_camera(cam44):
    b = np.ascontiguousarray(cam44, np.uint8).reshape(44)
    f = b.view(np.float32)
    i = b.view(np.int32)
    return dict(dir=f[0:3].copy(), pos=f[3:6].copy(), width=int(i[6]), height=int(i[7]), spp=int(i[8]), focal=F(f[9]),
                sensor=F(f[10]))


def camera_matrices(cam):
    """cameraFromRaster / worldFromCamera as dmt_set_camera builds them (float32, column-major 4x4)."""
    W, H = F(cam["width"]), F(cam["height"])
    sensorW = cam["sensor"] * W / H
    MM = F(0.001)
    focal, sh, sw = cam["focal"] * MM, cam["sensor"] * MM, sensorW * MM
    psx, psy = sw / W, sh / H
    tx = F(-0.5) * sw + F(0.5) * psx
    ty = F(0.5) * sh - F(0.5) * psy
    cfr = np.zeros(16, np.float32)
    cfr[0], cfr[5], cfr[10], cfr[12], cfr[13], cfr[14], cfr[15] = psx, -psy, 1, tx, ty, focal, 1

    def hnorm(a):
        inv = F(1) / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        return np.array([a[0] * inv, a[1] * inv, a[2] * inv], np.float32)

    def hcross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)

    fwd = hnorm(cam["dir"])
    right = hnorm(hcross(fwd, np.array([0, 0, 1], np.float32)))
    up = hcross(right, fwd)
    rfc = np.zeros(16, np.float32)
    rfc[0:3], rfc[4:7], rfc[8:11], rfc[12:15], rfc[15] = right, up, fwd, cam["pos"], 1
    return cfr, rfc


def _point(m, p):
    m = m.astype(np.float64)
    return np.array([m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12], m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13],
                     m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14]])


def _dir(m, v):
    m = m.astype(np.float64)
    return np.array([m[0] * v[0] + m[4] * v[1] + m[8] * v[2], m[1] * v[0] + m[5] * v[1] + m[9] * v[2],
                     m[2] * v[0] + m[6] * v[1] + m[10] * v[2]])


def _dirT(m, v):
    m = m.astype(np.float64)
    return np.array([m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[4] * v[0] + m[5] * v[1] + m[6] * v[2],
                     m[8] * v[0] + m[9] * v[1] + m[10] * v[2]])


def _norm(a):
    return a / math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))


def _dot(a, b):
    return float(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def generate_ray(cam, px, py):
    """generateRay (core-render.cpp:916-926) at film position (px, py): origin and unit direction, float64."""
    cfr, rfc = camera_matrices(cam)
    pCam = _point(cfr, (px, py, 0.0))
    return _point(rfc, (0.0, 0.0, 0.0)), _norm(_dir(rfc, _norm(pCam)))


def raster_of_direction(cam, d):
    """Inverse of generate_ray: the film position whose camera ray has direction d."""
    cfr, rfc = camera_matrices(cam)
    dc = _dirT(rfc, np.asarray(d, np.float64))
    p = dc * (float(cfr[14]) / dc[2])
    return (p[0] - float(cfr[12])) / float(cfr[0]), (p[1] - float(cfr[13])) / float(cfr[5])


def footprint(cam):
    """minDifferentialsFromCamera in double, as dmt_texture_footprint evaluates it: dict(cfr (3x4), min_dx, min_dy,
    spp_scale) and the rotation of renderFromCamera (`rfc_rot`, column-major 9 floats)."""
    cf, rf = camera_matrices(cam)
    pos = np.array([rf[12], rf[13], rf[14]], np.float64)
    tr = _dirT(rf, pos)
    cfr = np.zeros((3, 4), np.float64)
    for r in range(3):
        cfr[r, :3] = rf[4 * r:4 * r + 3]
        cfr[r, 3] = -tr[r]
    o = _point(cf, (0, 0, 0))
    dxCam, dyCam = _point(cf, (1, 0, 0)) - o, _point(cf, (0, 1, 0)) - o
    minX = minY = np.full(3, np.inf)
    for i in range(512):
        f = i / 511.0
        pCam = _point(cf, (f * cam["width"], f * cam["height"], 0.0))
        d = _norm(_dir(rf, _norm(pCam)))
        rx = _norm(_dir(rf, _dirT(rf, d) + dxCam))
        ry = _norm(_dir(rf, _dirT(rf, d) + dyCam))
        if d[0] != d[1] or d[0] != d[2]:   # gramSchmidt (cudautils-vecmath.cu:960-969)
            g = np.array([d[2] - d[1], d[0] - d[2], d[1] - d[0]])
        else:
            g = np.array([d[2] - d[1], d[0] + d[2], -d[1] - d[0]])
        fx = _norm(g)
        fy = np.array([d[1] * fx[2] - d[2] * fx[1], d[2] * fx[0] - d[0] * fx[2], d[0] * fx[1] - d[1] * fx[0]])

        def local(v):
            return np.array([_dot(v, fx), _dot(v, fy), _dot(v, d)])

        df, dxf, dyf = _norm(local(d)), _norm(local(rx)), _norm(local(ry))
        ex, ey = dxf - df, dyf - df
        if _dot(ex, ex) < _dot(minX, minX):
            minX = ex
        if _dot(ey, ey) < _dot(minY, minY):
            minY = ey
    scale = max(0.125, 1.0 / math.sqrt(max(cam["spp"], 1)))
    rot = np.array([rf[0], rf[1], rf[2], rf[4], rf[5], rf[6], rf[8], rf[9], rf[10]], np.float32)
    return dict(cfr=cfr.astype(np.float32), min_dx=minX.astype(np.float32), min_dy=minY.astype(np.float32),
                spp_scale=np.float32(scale), rfc_rot=rot)


D = np.float64


# ---- per-hit differentials (double, as the device evaluates them; vectorised over hits) -------------------------------------------------------------
def _v(a):
    return np.asarray(a, np.float64)


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(a):
    return a / np.sqrt(_dot3(a, a))[..., None]


def _mul3(m, v):  # column-major 3x3 per hit (..., 9)
    return np.stack([m[..., 0] * v[..., 0] + m[..., 3] * v[..., 1] + m[..., 6] * v[..., 2],
                     m[..., 1] * v[..., 0] + m[..., 4] * v[..., 1] + m[..., 7] * v[..., 2],
                     m[..., 2] * v[..., 0] + m[..., 5] * v[..., 1] + m[..., 8] * v[..., 2]], -1)


def _mul3T(m, v):
    return np.stack([m[..., 0] * v[..., 0] + m[..., 1] * v[..., 1] + m[..., 2] * v[..., 2],
                     m[..., 3] * v[..., 0] + m[..., 4] * v[..., 1] + m[..., 5] * v[..., 2],
                     m[..., 6] * v[..., 0] + m[..., 7] * v[..., 1] + m[..., 8] * v[..., 2]], -1)


def _inv3(m):
    c0 = m[..., 4] * m[..., 8] - m[..., 7] * m[..., 5]
    c1 = m[..., 7] * m[..., 2] - m[..., 1] * m[..., 8]
    c2 = m[..., 1] * m[..., 5] - m[..., 4] * m[..., 2]
    inv = D(1) / (m[..., 0] * c0 + m[..., 3] * c1 + m[..., 6] * c2)
    r = [c0 * inv, c1 * inv, c2 * inv,
         (m[..., 6] * m[..., 5] - m[..., 3] * m[..., 8]) * inv, (m[..., 0] * m[..., 8] - m[..., 6] * m[..., 2]) * inv,
         (m[..., 3] * m[..., 2] - m[..., 0] * m[..., 5]) * inv,
         (m[..., 3] * m[..., 7] - m[..., 6] * m[..., 4]) * inv, (m[..., 6] * m[..., 1] - m[..., 0] * m[..., 7]) * inv,
         (m[..., 0] * m[..., 4] - m[..., 3] * m[..., 1]) * inv]
    return np.stack(r, -1)


def rotate_from_to_z(f):
    """Transform::rotateFromTo(f, +z) per hit, column-major 9 floats (cudautils-transform.cu:87-147)."""
    n = f.shape[0]
    R = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64), (n, 1))
    cosT = f[:, 2]
    gen = ~(cosT > D(1) - D(1e-6)) & ~(cosT < D(-1) + D(1e-6))
    x, y, z = f[:, 1], -f[:, 0], np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        s = np.sqrt(x * x + y * y + z * z)
        kk = (D(1) - cosT) / (s * s)
    vx = [np.zeros(n, np.float64), -z, y, z, np.zeros(n, np.float64), -x, -y, x, np.zeros(n, np.float64)]
    vx2 = [-y * y - z * z, x * y, x * z, x * y, -x * x - z * z, y * z, x * z, y * z, -x * x - y * y]
    at = [0, 3, 6, 1, 4, 7, 2, 5, 8]
    for i in range(9):
        R[gen, at[i]] += (vx[i] + vx2[i] * kk)[gen]
    opp = cosT < D(-1) + D(1e-6)
    for j in np.nonzero(opp)[0]:   # case 2 (not reached by a camera ray: camera-space z > 0)
        fr = f[j]
        o = np.array([1, 0, 0], np.float64) if not abs(float(fr[0])) > 0.99 else np.array([0, 1, 0], np.float64)
        a = _normalize(_cross3(fr, o))
        X, Y, Z, cc = a[0], a[1], a[2], D(-1)
        tt = D(1) - cc
        R[j] = [tt * X * X + cc, tt * X * Y - Z, tt * Z * X + Y, tt * X * Y + Z, tt * Y * Y + cc, tt * Y * Z - X,
                tt * Z * X - Y, tt * Y * Z + X, tt * Z * Z + cc]
    return R


def hit_dpdxy(fp, p, ng):
    """approximate_dp_dxy (core-texture.cu:55-87) at camera-ray hits p with normals ng (any orientation), in double."""
    p, ng = _v(p), _v(ng)
    n = p.shape[0]
    c = _v(fp["cfr"]).reshape(3, 4)
    pC = np.stack([c[r, 0] * p[:, 0] + c[r, 1] * p[:, 1] + c[r, 2] * p[:, 2] + c[r, 3] for r in range(3)], -1)
    rfc = np.tile(_v(fp["rfc_rot"]), (n, 1))
    R = rotate_from_to_z(_normalize(pC))
    Ri = _inv3(R)
    pD = _mul3(R, pC)
    nD = _mul3T(Ri, _mul3T(rfc, ng))
    dd = nD[:, 2] * pD[:, 2]
    mdx, mdy = _v(fp["min_dx"]), _v(fp["min_dy"])
    xd = _normalize(np.tile(np.array([mdx[0], mdx[1], D(1) + mdx[2]], np.float64), (n, 1)))
    yd = _normalize(np.tile(np.array([mdy[0], mdy[1], D(1) + mdy[2]], np.float64), (n, 1)))
    tx = -(D(0) - dd) / _dot3(nD, xd)
    ty = -(D(0) - dd) / _dot3(nD, yd)
    sc = D(fp["spp_scale"])
    dpdx = sc * _mul3(rfc, _mul3(Ri, xd * tx[:, None] - pD))
    dpdy = sc * _mul3(rfc, _mul3(Ri, yd * ty[:, None] - pD))
    return dpdx, dpdy


def hit_differentials(fp, p, ng, p0, p1, p2, uv):
    """UV differentials (dudx, dudy, dvdx, dvdy) of camera-ray hits (tex_footprint in csrc/dmt_hip.hip: double, rounded to float).
    p, ng, p0, p1, p2: (n, 3); uv: (n, 6).  Returns (d (n, 4), margin (n,)): margin = relative distance of
    |cross(dpdx, dpdy)| from the 1e-6 zeroing threshold (inf where that test does not decide)."""
    p0, p1, p2, uv = (_v(a) for a in (p0, p1, p2, uv))
    n = p0.shape[0]
    dpdx, dpdy = hit_dpdxy(fp, p, ng)
    cr = _cross3(dpdx, dpdy)
    crl = np.sqrt(_dot3(cr, cr))
    out = np.zeros((n, 4), np.float32)
    margin = np.abs(crl / D(1e-6) - 1).astype(np.float64)
    live = crl >= D(1e-6)
    dp1, dp2 = p1 - p0, p2 - p0
    du1, dv1, du2, dv2 = uv[:, 2] - uv[:, 0], uv[:, 3] - uv[:, 1], uv[:, 4] - uv[:, 0], uv[:, 5] - uv[:, 1]
    detUv = du1 * dv2 - dv1 * du2
    live &= detUv != 0   # [fix 5]
    with np.errstate(all="ignore"):
        inv = D(1) / detUv
        dpdu = (dv2[:, None] * dp1 - dv1[:, None] * dp2) * inv[:, None]
        dpdv = (-du2[:, None] * dp1 + du1[:, None] * dp2) * inv[:, None]
        for j in np.nonzero(live)[0]:
            out[j] = _duv(dpdu[j], dpdv[j], dpdx[j], dpdy[j])
    return out, margin


def _duv(dpdu, dpdv, dpdx, dpdy):
    """duv_From_dp_dxy (core-texture.cu:123-258) for one hit; returns (dudx, dudy, dvdx, dvdy)."""
    def ln(v):
        return np.sqrt(_dot3(v, v))

    rdpdy = dpdy
    if ln(dpdx - dpdy) < D(1e-12) * max(D(1), ln(dpdx)):
        nn = _cross3(dpdu, dpdv)
        nl = ln(nn)
        if nl < D(1e-12):
            nn = _cross3(dpdu, dpdx)
            nl = ln(nn)
            if nl < D(1e-12):
                nn = _cross3(dpdv, dpdx)
                nl = ln(nn)
        if nl < D(1e-12):
            nn = np.array([0, 0, 1], np.float64)
        rdpdy = dpdy + _normalize(nn) * (D(1e-6) * max(D(1), ln(dpdx)))
    a00, a01, a11 = _dot3(dpdu, dpdu), _dot3(dpdu, dpdv), _dot3(dpdv, dpdv)
    b0x, b1x, b0y, b1y = _dot3(dpdu, dpdx), _dot3(dpdv, dpdx), _dot3(dpdu, rdpdy), _dot3(dpdv, rdpdy)
    det = a00 * a11 - a01 * a01
    if abs(det) < D(1e-8):
        return 0, 0, 0, 0
    if not np.isinf(det) and abs(det) > D(1e-12):
        inv = D(1) / det
        dudx, dvdx = (a11 * b0x - a01 * b1x) * inv, (a00 * b1x - a01 * b0x) * inv
        dudy, dvdy = (a11 * b0y - a01 * b1y) * inv, (a00 * b1y - a01 * b0y) * inv
    else:
        lam = D(1e-6) * max(D(1), max(a00, a11))
        r00, r11, r01 = a00 + lam, a11 + lam, a01
        rdet = r00 * r11 - r01 * r01
        if not np.isinf(rdet) and abs(rdet) > 0:
            inv = D(1) / rdet
            dudx, dvdx = (r11 * b0x - r01 * b1x) * inv, (r00 * b1x - r01 * b0x) * inv
            dudy, dvdy = (r11 * b0y - r01 * b1y) * inv, (r00 * b1y - r01 * b0y) * inv
        else:
            nn = _cross3(dpdu, dpdv)
            nl = ln(nn)
            if nl < D(1e-12):
                nn = _cross3(dpdu, dpdx)
                nl = ln(nn)
                if nl < D(1e-12):
                    nn = _cross3(dpdv, dpdx)
                    nl = ln(nn)
            nn = np.array([0, 0, 1], np.float64) if nl < D(1e-12) else _normalize(nn)
            gu, gv = _normalize(_cross3(nn, dpdv)), _normalize(_cross3(dpdu, nn))
            dudx, dvdx, dudy, dvdy = _dot3(gu, dpdx), _dot3(gv, dpdx), _dot3(gu, rdpdy), _dot3(gv, rdpdy)

    def cl(x):
        return np.float32(0) if np.isinf(x) else np.float32(min(max(x, -1e8), 1e8))

    return cl(dudx), cl(dudy), cl(dvdx), cl(dvdy)


# ---- lookups -----------------------------------------------------------------------------------------------------------
def _mirror(c, size):
    p = size * 2
    c = np.mod(c, p)
    return np.where(c < size, c, p - c - 1)


def _texel(level, s, t):
    h, w = level.shape[:2]
    return level[_mirror(np.asarray(t), h), _mirror(np.asarray(s), w), :3].astype(np.float32) / F(255)


def bilinear(level, s, t, normal=False):
    """sampleBilinearTexel (core-material.cpp:20-56) on one level."""
    h, w = level.shape[:2]
    x, y = F(s) * F(w) - F(0.5), F(t) * F(h) - F(0.5)
    fx, fy = np.floor(x), np.floor(y)
    x0, y0 = int(fx), int(fy)
    tx, ty = x - fx, y - fy
    c00, c10, c01, c11 = _texel(level, x0, y0), _texel(level, x0 + 1, y0), _texel(level, x0, y0 + 1), _texel(level, x0 + 1, y0 + 1)
    c = lerp(lerp(c00, c10, tx), lerp(c01, c11, tx), ty)
    if normal:
        c[0], c[1] = c[0] * F(2) - F(1), c[1] * F(2) - F(1)
    return c


def lerp(a, b, t):
    """cudautils-color.cuh:112-114."""
    return a if t <= 0 else (b if t >= 1 else (F(1) - F(t)) * a + F(t) * b)


def ewa_box(w, h, s, t, d0, d1):
    d0x, d0y, d1x, d1y = F(d0[0]) * F(w), F(d0[1]) * F(h), F(d1[0]) * F(w), F(d1[1]) * F(h)
    sx, sy = int(F(s) * F(w) - F(0.5)), int(F(t) * F(h) - F(0.5))
    A = d0y * d0y + d1y * d1y + F(1)
    B = F(-2) * (d0x * d0y + d1x * d1y)
    C = d0x * d0x + d1x * d1x + F(1)
    invF = F(1) / (A * C - F(0.25) * B * B)
    A, B, C = A * invF, B * invF, C * invF
    invDet = F(1) / (A * C - F(0.25) * B * B)
    uR, vR = np.sqrt(max(C * invDet, F(0))), np.sqrt(max(A * invDet, F(0)))
    s0, s1 = np.ceil(F(sx) - uR), np.floor(F(sx) + uR)
    t0, t1 = np.ceil(F(sy) - vR), np.floor(F(sy) + vR)
    count = (s1 - s0 + F(1)) * (t1 - t0 + F(1))
    cx, cy = float(F(s) * F(w) - F(0.5)), float(F(t) * F(h) - F(0.5))
    edges = (cx, cy, float(F(sx) - uR), float(F(sx) + uR), float(F(sy) - vR), float(F(sy) + vR))
    return dict(A=A, B=B, C=C, sx=sx, sy=sy, s0=s0, s1=s1, t0=t0, t1=t1, count=float(count), centre=(cx, cy),
                edge_dist=min(abs(e - round(e)) for e in edges))   # texels from the nearest truncation / rounding edge


def ewa(level, s, t, d0, d1, normal=False):
    """EWAFormula (core-texture.cu:664-748) with [fix 4]; returns (rgb, margin): margin = the smallest distance, in LUT
    bins, of a texel's r2 * 128 from a bin edge or from the r2 < 1 edge (where a rounding would move one weight)."""
    h, w = level.shape[:2]
    b = ewa_box(w, h, s, t, d0, d1)

    def tex(si, ti):
        c = _texel(level, si, ti)
        if normal:
            c = c.copy()
            c[..., 0], c[..., 1] = c[..., 0] * F(2) - F(1), c[..., 1] * F(2) - F(1)
        return c

    margin = np.inf
    if b["count"] <= EWA_MAX_TEXELS:
        tt, ss = np.meshgrid(np.arange(int(b["t0"]), int(b["t1"]) + 1), np.arange(int(b["s0"]), int(b["s1"]) + 1), indexing="ij")
        ssf, ttf = ss.astype(np.float32) - F(b["sx"]), tt.astype(np.float32) - F(b["sy"])
        r2 = b["A"] * ssf * ssf + b["B"] * ssf * ttf + b["C"] * ttf * ttf
        inside = r2 < F(1)
        x = r2.astype(np.float64) * EWA_LUT_SIZE
        near = (x < EWA_LUT_SIZE + 1) & ((ssf != 0) | (ttf != 0))   # the centre's r2 is exactly 0 on both sides
        if near.any():
            margin = float(np.abs(x[near] - np.round(x[near])).min())
        idx = np.minimum(r2 * F(EWA_LUT_SIZE), F(EWA_LUT_SIZE - 1)).astype(np.int32)
        wts = np.where(inside, LUT[np.clip(idx, 0, EWA_LUT_SIZE - 1)], F(0)).astype(np.float32)
        sumW = F(0)
        acc = np.zeros(3, np.float32)
        for i, j in zip(*np.nonzero(inside)):  # in the device's loop order (rows, then columns)
            acc = acc + tex(int(ss[i, j]), int(tt[i, j])) * wts[i, j]
            sumW = F(sumW + wts[i, j])
        if sumW > 0:
            cx, cy = b["centre"]
            margin = min(margin, abs(cx - round(cx)) * EWA_LUT_SIZE, abs(cy - round(cy)) * EWA_LUT_SIZE)
            return acc / sumW, margin
    return tex(b["sx"], b["sy"]), margin


def lod_minor(d, w, h):
    """computeTextureLOD_from_dudv's lod_minor (core-texture.cu:595-662), in double as the device evaluates it (the
    smaller eigenvalue of a long, thin footprint is a difference of nearly equal numbers); returned as float32."""
    dudx, dudy, dvdx, dvdy = (float(np.float32(x)) for x in d)
    a0, a1, b0, b1 = dudx * w, dvdx * h, dudy * w, dvdy * h
    E, Fm, G = a0 * a0 + a1 * a1, b0 * b0 + b1 * b1, a0 * b0 + a1 * b1
    eps = 1e-12
    trace = E + Fm
    det = E * Fm - G * G
    if det < 0 and det > -eps:
        det = 0.0
    if trace <= eps:
        return F(0)
    discr = max(trace * trace - 4.0 * det, 0.0)
    l2 = 0.5 * (trace - math.sqrt(discr))
    if l2 < 0 and l2 > -eps:
        l2 = 0.0
    sigma = math.sqrt(l2) if l2 > 0 else 0.0
    return F(max(0.0, math.log2(sigma))) if sigma > 0 else F(0)


def lookup(levels, s, t, d, normal=False):
    """sampleMippedTexture (core-material.cpp:83-175) with [fix 2-4].  levels: mip_chain(); d = (dudx, dudy, dvdx, dvdy).
    Returns dict(rgb, branch, lod, margin): branch 0 level 0, 1 trilinear, 2 EWA, 3 EWA at a raised level; margin = the
    smallest relative distance of a branch-deciding quantity from its threshold; rgb_margin as ewa()."""
    dudx, dudy, dvdx, dvdy = (F(x) for x in d)
    h, w = levels[0].shape[:2]
    L = len(levels)
    if dudx == 0 and dudy == 0 and dvdx == 0 and dvdy == 0:
        return dict(rgb=bilinear(levels[0], s, t, normal), branch=0, lod=0.0, margin=np.inf, rgb_margin=np.inf)
    dx, dy = np.array([dudx, dvdx], np.float32), np.array([dudy, dvdy], np.float32)
    lx, ly = dx[0] * dx[0] + dx[1] * dx[1], dy[0] * dy[0] + dy[1] * dy[1]
    d0, d1 = (dx, dy.copy()) if lx > ly else (dy, dx.copy())
    shorter, longer = np.sqrt(d1[0] * d1[0] + d1[1] * d1[1]), np.sqrt(d0[0] * d0[0] + d0[1] * d0[1])
    a = np.abs(np.array([dudx, dudy, dvdx, dvdy], np.float64))
    someNear = bool((a < FLT_EPSILON).any())
    nz = a[a > 0]
    margin = float(np.abs(np.log2(nz / FLT_EPSILON)).min()) if nz.size else np.inf
    if lx != ly:
        margin = min(margin, abs(float(lx) - float(ly)) / max(float(lx), float(ly)))
    if not someNear or shorter == 0:   # [fix 3]
        dud, dvd = max(abs(dudx), abs(dudy)), max(abs(dvdx), abs(dvdy))
        rho = max(dud * F(w), dvd * F(h))
        lod = max(np.log2(max(rho, F(1e-8))), F(0))
        ilod = min(max(int(np.floor(lod)), 0), L - 1)
        tl = F(lod - F(ilod))
        if lod > 0:
            margin = min(margin, abs(float(lod) - round(float(lod))))
        c0 = bilinear(levels[ilod], s, t, normal)
        c1 = bilinear(levels[min(ilod + 1, L - 1)], s, t, normal)   # [fix 2]
        return dict(rgb=lerp(c0, c1, tl), branch=1, lod=float(lod), margin=margin, rgb_margin=np.inf)
    den = shorter * F(MAX_ANISOTROPY)
    if den < longer:
        d1 = d1 * (longer / den)
        margin = min(margin, abs(float(longer) / float(den) - 1))
    lam = lod_minor((dudx, dudy, dvdx, dvdy), w, h)
    ilod = min(max(int(np.floor(lam)), 0), L - 1)
    tl = F(lam - F(ilod))
    if lam > 0:
        margin = min(margin, abs(float(lam) - round(float(lam))))
    raised = False
    while ilod < L - 1:
        lh, lw = levels[ilod].shape[:2]
        box = ewa_box(lw, lh, s, t, d0, d1)
        cnt = box["count"]
        margin = min(margin, abs(cnt - EWA_MAX_TEXELS - 0.5) / EWA_MAX_TEXELS)
        if abs(cnt - EWA_MAX_TEXELS) <= (box["s1"] - box["s0"] + 1) + (box["t1"] - box["t0"] + 1) + 2:
            margin = min(margin, box["edge_dist"] / 10)   # one row or column more or less would cross the cap
        if cnt <= EWA_MAX_TEXELS:
            break
        ilod, raised = ilod + 1, True
    c0, m0 = ewa(levels[ilod], s, t, d0, d1, normal)
    c1, m1 = ewa(levels[min(ilod + 1, L - 1)], s, t, d0, d1, normal)   # [fix 2]
    return dict(rgb=lerp(c0, c1, tl), branch=3 if raised else 2, lod=float(ilod) + float(tl), margin=margin,
                rgb_margin=min(m0, m1))
