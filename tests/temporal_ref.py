"""numpy restatement of dmt_denoise_temporal's reprojection: the world-to-film projection
(dmt_camera_project), the surface point under two vertex sets, the 2 x 2 history taps with their tests, the blend and its
variance.  Every quantity is float32 and every expression is evaluated in the order k_temporal (csrc/denoise.hpp) evaluates
it, so the device matches this module to the rounding of its divisions.

Next to its outputs `accumulate` returns a near-threshold mask: the pixels where one of its own tap tests lies within a
relative 1e-4 of its threshold, or where u / v lies within 1e-3 of an integer while a tap on the far side of that integer
would fail a test.  Only those pixels may be left out of a device-vs-restatement comparison (a tap the two sides decide
differently changes the result discontinuously).  The second reason is applied more narrowly than that, in two ways.  A
pixel whose motion is exactly zero is never masked for it: both sides compute the identical u = px from identical inputs,
so their floors agree.  And it needs one of the restatement's own taps of weight >= 1e-3 to fail as well: if the device
floors the other way, its taps are the restatement's large-weight ones plus the far one at a weight below 1e-3 in place of
the near one at such a weight, and while every large-weight tap counts on both sides the two results differ by less than
that weight times the taps' contrast, with |u_device - u_restatement| (a few ulps of the film coordinate) as the weight
that matters.  (Without this a motion of rounding size, as under a common translation of scene and camera, would mask
every pixel at the image border and at every silhouette, where the far tap fails but carries no weight on either side.)
"""
import numpy as np

import denoise_ref as DR

F = np.float32
DEFAULTS = dict(alpha=0.2, normal_threshold=0.9, plane_threshold=2.0)  # dmt_temporal_defaults
H_MAX = F(65536)
MASK_REL = 1e-4     # a test within this relative distance of its threshold
MASK_INT = 1e-3     # u / v within this distance of an integer
MASK_CAP = 0.01     # a comparison that leaves out more than this share of the pixels has failed


def camera_fields(camera44):
    cam = np.ascontiguousarray(camera44, np.uint8).reshape(44)
    f = cam.view(np.float32)
    i = cam.view(np.int32)
    return f[0:3].copy(), f[3:6].copy(), int(i[6]), int(i[7]), F(f[9]), F(f[10])


def make_camera(direction, pos, width, height, focal=20.0, sensor=36.0, spp=1):
    """a 44-byte dmt_camera"""
    cam = np.zeros(11, np.float32)
    cam[0:3], cam[3:6], cam[9], cam[10] = direction, pos, focal, sensor
    cam.view(np.int32)[6:9] = (width, height, spp)
    return cam.view(np.uint8).copy()


def _normalize(v):
    inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return np.array([v[0] * inv, v[1] * inv, v[2] * inv], F)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def proj_xf(camera44):
    """what dmt_set_camera's two matrices give the projection: right / up / fwd / pos, focal, tx, ty, ipx, ipy (float32,
    the host code's expressions)"""
    d, pos, w, h, focal_mm, sensor_mm = camera_fields(camera44)
    fwd = _normalize(d.astype(F))
    right = _normalize(_cross(fwd, np.array([0, 0, 1], F)))
    up = _cross(right, fwd)
    mm = F(0.001)
    sensor_w = sensor_mm * F(w) / F(h)
    focal, sh, sw = focal_mm * mm, sensor_mm * mm, sensor_w * mm
    psx, psy = sw / F(w), sh / F(h)
    tx = F(-0.5) * sw + F(0.5) * psx
    ty = F(0.5) * sh - F(0.5) * psy
    return dict(right=right, up=up, fwd=fwd, pos=pos.astype(F), focal=F(focal), tx=F(tx), ty=F(ty), ipx=F(1) / psx, ipy=F(1) / -psy)


def project(xf, p):
    """render-space points [..., 3] -> (fx, fy, depth), dmt_camera_project's order of operations"""
    p = np.asarray(p, F)
    d = [p[..., a] - xf["pos"][a] for a in range(3)]
    dot = lambda r: (r[0] * d[0] + r[1] * d[1]) + r[2] * d[2]  # noqa: E731
    cx, cy, cz = dot(xf["right"]), dot(xf["up"]), dot(xf["fwd"])
    with np.errstate(all="ignore"):
        s = xf["focal"] / cz
        fx = (cx * s - xf["tx"]) * xf["ipx"]
        fy = (cy * s - xf["ty"]) * xf["ipy"]
    return fx.astype(F), fy.astype(F), cz.astype(F)


def verts9(xs, ys, zs):
    """the soup of dmt_upload_triangles (n x 4 each, lane 3 unused) as 9 floats per triangle: p0, p1, p2"""
    xs, ys, zs = (np.asarray(a, F).reshape(-1, 4)[:, :3] for a in (xs, ys, zs))
    return np.stack([xs, ys, zs], -1).reshape(-1, 9).astype(F)


def surface_point(v9, tri, bu, bv):
    """X = w0 p0 + bu p1 + bv p2, w0 = (1 - bu) - bv, left to right per component"""
    v = np.asarray(v9, F)[tri]
    bu, bv = np.asarray(bu, F), np.asarray(bv, F)
    w0 = (F(1) - bu) - bv
    return np.stack([(w0 * v[..., a] + bu * v[..., 3 + a]) + bv * v[..., 6 + a] for a in range(3)], -1).astype(F)


def accumulate(cur_c, cur_v, albedo, normal, surface, verts_cur, verts_prev, cam_cur, hist, alpha=DEFAULTS["alpha"],
               normal_threshold=DEFAULTS["normal_threshold"], plane_threshold=DEFAULTS["plane_threshold"], motion=None):
    """One k_temporal.  cur_c [H, W, 3], cur_v [H, W]: k_denoise_init's plane (denoise_ref.initial); the current AOVs; the
    raw vertices of this frame and of the history's; cam_cur: the current 44-byte camera; hist: None (reset) or a dict with
    c, v, h, normal, position, camera (what `history` returns).  Returns (c, v, h, info): info = dict(reprojected, reset,
    mask, weights [H, W, 4] (the counted taps' bilinear weights, tap order (0,0) (1,0) (0,1) (1,1)), u, v).
    motion: (mx, my) to use in place of the two projections' difference (property tests of the taps alone)."""
    cur_c, cur_v = np.asarray(cur_c, F), np.asarray(cur_v, F)
    albedo, normal, surface = np.asarray(albedo, F), np.asarray(normal, F), np.asarray(surface, F)
    H, W = cur_v.shape
    yy, xx = np.mgrid[0:H, 0:W]
    covered = albedo[..., 3] > 0
    out_c, out_v = cur_c.copy(), cur_v.copy()
    out_h = np.where(covered, F(1), F(0)).astype(F)
    mask = np.zeros((H, W), bool)
    weights = np.zeros((H, W, 4), F)
    uu, vv = xx.astype(F), yy.astype(F)
    reproj = np.zeros((H, W), bool)
    if hist is not None:
        ntri = np.asarray(verts_cur).shape[0]
        with np.errstate(all="ignore"):
            have = covered & (surface[..., 0] >= 0) & (surface[..., 0] < F(ntri))
        tri = np.where(have, surface[..., 0], 0).astype(np.int64)
        bu, bv = surface[..., 1], surface[..., 2]
        Xc, Xp = surface_point(verts_cur, tri, bu, bv), surface_point(verts_prev, tri, bu, bv)
        xf_c, xf_p = proj_xf(cam_cur), proj_xf(hist["camera"])
        th_prev = DR.theta(hist["camera"])
        fxc, fyc, _ = project(xf_c, Xc)
        fxp, fyp, dp = project(xf_p, Xp)
        with np.errstate(all="ignore"):
            mx, my = fxp - fxc, fyp - fyc
            if motion is not None:
                mx, my = np.full((H, W), motion[0], F), np.full((H, W), motion[1], F)
            uu, vv = xx.astype(F) + mx, yy.astype(F) + my
            inr = (dp > 0) & (uu > -1) & (uu < F(W)) & (vv > -1) & (vv < F(H))
        have = have & inr
        us, vs = np.where(have, uu, 0).astype(F), np.where(have, vv, 0).astype(F)
        fu0, fv0 = np.floor(us), np.floor(vs)
        iu, iv = fu0.astype(np.int64), fv0.astype(np.int64)
        fu, fv = us - fu0, vs - fv0
        nt, pt = F(normal_threshold), F(plane_threshold)
        hn, hx = np.asarray(hist["normal"], F), np.asarray(hist["position"], F)
        hc, hv, hh = np.asarray(hist["c"], F), np.asarray(hist["v"], F), np.asarray(hist["h"], F)

        def tap_tests(qx, qy):
            """(passes every test, some test is near its threshold) of the history tap (qx, qy) for every pixel"""
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            nq, xq, hq = hn[cy, cx], hx[cy, cx], hh[cy, cx]
            with np.errstate(all="ignore"):
                nd = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                pd = np.abs((nq[..., 0] * (Xp[..., 0] - xq[..., 0]) + nq[..., 1] * (Xp[..., 1] - xq[..., 1]))
                            + nq[..., 2] * (Xp[..., 2] - xq[..., 2]))
                lim = (pt * xq[..., 3]) * th_prev
                live = ok & (hq >= 1)
                passes = live & (nd >= nt) & (pd <= lim)
                near = live & ((np.abs(nd - nt) <= MASK_REL * abs(nt)) | (np.abs(pd - lim) <= MASK_REL * np.abs(lim)))
            return passes, near

        sw, sv, sh = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        own_fails = np.zeros((H, W), bool)
        for t in range(4):
            ox, oy = t & 1, t >> 1
            qx, qy = iu + ox, iv + oy
            w = ((fu if ox else F(1) - fu) * (fv if oy else F(1) - fv)).astype(F)
            passes, near = tap_tests(qx, qy)
            use = have & (w > 0) & passes
            mask |= have & (w > 0) & near
            own_fails |= have & (w >= MASK_INT) & ~passes  # a tap of real weight
            cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            wz = np.where(use, w, F(0))
            weights[..., t] = wz
            sw = sw + wz
            sc = sc + wz[..., None] * np.where(use[..., None], hc[cy, cx], F(0))
            sv = sv + (wz * wz) * np.where(use, hv[cy, cx], F(0))
            sh = sh + wz * np.where(use, hh[cy, cx], F(0))
        reproj = have & (sw > 0)
        with np.errstate(all="ignore"):
            h = np.minimum(sh / sw + F(1), H_MAX)
            a = np.maximum(F(alpha), F(1) / h)
            pc, pv = sc / sw[..., None], sv / (sw * sw)
            b = F(1) - a
            bc = pc + a[..., None] * (cur_c - pc)
            bvv = (b * b) * pv + (a * a) * cur_v
        blend = reproj & (a < 1)
        out_c = np.where(blend[..., None], bc, cur_c).astype(F)
        out_v = np.where(blend, bvv, cur_v).astype(F)
        out_h = np.where(reproj, h, out_h).astype(F)
        # u / v close to an integer: the taps across it, which the device takes instead if it floors the other way
        moving = have & own_fails & ((mx != 0) | (my != 0))
        ru, rv = np.rint(us), np.rint(vs)
        near_u, near_v = moving & (np.abs(us - ru) < MASK_INT), moving & (np.abs(vs - rv) < MASK_INT)
        far_x = np.where(fu0 == ru, ru - 1, ru + 1).astype(np.int64)   # the column beyond the integer, seen from u
        far_y = np.where(fv0 == rv, rv - 1, rv + 1).astype(np.int64)
        for oy in (0, 1):
            mask |= near_u & ~tap_tests(far_x, iv + oy)[0]
        for ox in (0, 1):
            mask |= near_v & ~tap_tests(iu + ox, far_y)[0]
        mask |= near_u & near_v & ~tap_tests(far_x, far_y)[0]
    reset = covered & ~reproj
    info = dict(reprojected=int(reproj.sum()), reset=int(reset.sum()), mask=mask, weights=weights, u=uu, v=vv)
    return out_c, out_v, out_h, info


def history(c, v, h, normal, position, camera44):
    """the history a call leaves: its accumulated plane, and the normal / position planes and the camera of its frame"""
    return dict(c=np.asarray(c, F), v=np.asarray(v, F), h=np.asarray(h, F), normal=np.asarray(normal, F).copy(),
                position=np.asarray(position, F).copy(), camera=np.ascontiguousarray(camera44, np.uint8).copy())


def step(hist, mean, m2, albedo, normal, position, surface, verts_cur, verts_prev, camera44, temporal=None, denoise=None):
    """One dmt_denoise_temporal: (out4, new history, info).  hist None: after a reset."""
    t = dict(DEFAULTS)
    t.update(temporal or {})
    d = dict(DR.DEFAULTS)
    d.update(denoise or {})
    c0, v0, bad = DR.initial(mean, m2)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} pixels have N < 2 or a non-finite mean / M2")
    c, v, h, info = accumulate(c0, v0, albedo, normal, surface, verts_cur, verts_prev, camera44, hist, **t)
    new = history(c, v, h, normal, position, camera44)
    th = DR.theta(camera44)
    fc, fv = c, v
    for i in range(int(d["iterations"])):
        fc, fv = DR.atrous_pass(fc, fv, albedo, normal, position, 1 << i, th, d["sigma_normal"], d["sigma_position"], d["sigma_albedo"],
                                d["sigma_luminance"])
    out = np.ones(c.shape[:2] + (4,), F)
    out[..., :3] = fc
    return out, new, info
