"""numpy restatement of the heterogeneous medium (include/dmt_hip.h dmt_set_medium_grid): the voxel march.

Two layers.  march_f32 is exact: float32 operations in the stated order, one scalar at a time, with the reciprocals correctly
rounded (numpy's float32 division), so it gives the device's and the host twin's values bit for bit.  pieces64_many /
tau64_many are what the fp32 march approximates: every ray cut at every plane of the grid it crosses (the float32 plane
positions taken as exact), the extinction integrated piece by piece in float64, vectorised over rays.  medium_ref supplies the clip and is left untouched.
"""
import numpy as np

import medium_ref as MR

F = np.float32
INF = F(np.inf)


class Grid:
    """density [nz, ny, nx] in the box [lo, hi], with the values the library derives on upload"""

    def __init__(self, lo, hi, density):
        self.lo, self.hi = np.asarray(lo, F), np.asarray(hi, F)
        self.density = np.ascontiguousarray(density, F)
        nz, ny, nx = self.density.shape
        self.n = (nx, ny, nz)
        self.cell = [F(F(self.hi[a] - self.lo[a]) / F(self.n[a])) for a in range(3)]
        self.inv_cell = [F(F(1) / self.cell[a]) for a in range(3)]
        self.planes = [np.array([self.plane(a, i) for i in range(self.n[a] + 1)], F) for a in range(3)]
        pos = np.argwhere(self.density > 0)  # (z, y, x)
        self.positive = int(pos.shape[0])
        if self.positive:
            self.imin = tuple(int(pos[:, 2 - a].min()) for a in range(3))
            self.imax = tuple(int(pos[:, 2 - a].max()) for a in range(3))
        else:
            self.imin, self.imax = (0, 0, 0), (-1, -1, -1)
        self.slo = np.array([self.plane(a, self.imin[a]) for a in range(3)], F)
        self.shi = np.array([self.plane(a, self.imax[a] + 1) for a in range(3)], F)

    def plane(self, a, i):
        return self.hi[a] if i == self.n[a] else F(self.lo[a] + F(F(i) * self.cell[a]))


def _entry(p, lo, inv_cell, imin, imax):
    f = np.floor(F(F(p - lo) * inv_cell))
    if not f >= F(imin):
        return imin
    return imax if f > F(imax) else int(f)


def march_f32(G, sigma_t, o, d, t_end, tau_target):
    """one ray -> (tau, ts, collided, steps) as dmt_medium_grid_march states the arithmetic"""
    o, d = np.asarray(o, F), np.asarray(d, F)
    sigma_t, t_end, tau_target = F(sigma_t), F(t_end), F(tau_target)
    if not G.positive:
        return F(0), F(0), False, 0
    with np.errstate(over="ignore", invalid="ignore"):
        t0, t1, hit = MR.segment_f32(G.slo, G.shi, o, d, t_end)
        if not hit:
            return F(0), F(0), False, 0
        par = [bool(abs(d[a]) < MR.PARALLEL) for a in range(3)]
        inv = [F(0) if par[a] else F(F(1) / d[a]) for a in range(3)]
        step = [1 if d[a] > 0 else -1 for a in range(3)]
        i = [_entry(F(o[a] + F(t0 * d[a])), G.lo[a], G.inv_cell[a], G.imin[a], G.imax[a]) for a in range(3)]
        tc, tau, steps = t0, F(0), 0
        while True:
            steps += 1
            tn3 = [INF if par[a] else F(F(G.plane(a, i[a] + (1 if step[a] > 0 else 0)) - o[a]) * inv[a]) for a in range(3)]
            ax, tn = 0, tn3[0]
            if tn3[1] < tn:
                ax, tn = 1, tn3[1]
            if tn3[2] < tn:
                ax, tn = 2, tn3[2]
            te = tn if tn < t1 else t1
            seg = F(te - tc)
            if not seg > 0:
                seg = F(0)
            s = F(sigma_t * G.density[i[2], i[1], i[0]])
            dtau = F(s * seg)
            if s > 0 and F(tau + dtau) >= tau_target:
                ts = F(tc + F(np.float64(F(tau_target - tau)) / np.float64(s)))
                return tau, (ts if ts < te else te), True, steps
            tau = F(tau + dtau)
            tc = tc if tc > te else te
            if not tn < t1:
                break
            i[ax] += step[ax]
            if i[ax] < G.imin[ax] or i[ax] > G.imax[ax]:
                break
    return tau, F(0), False, steps


def pieces64_many(G, sigma_t, o, d, t_end):
    """float64, vectorised over rays (o, d: [n, 3]; t_end: [n] or a number): every ray over [0, t_end] cut at every grid
    plane inside the support box -> (t [n, K + 1] ascending break points from t0 to t1, s [n, K] the extinction
    sigma_t * density of each piece).  K is the same for every ray: planes a ray does not cross inside its segment give
    pieces of length 0, and so does a ray that misses the support (all its break points are equal).  The float32 inputs
    and plane positions are taken as exact; a point in a plane belongs to the voxel above it, clamped to the support, as
    in the march."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = o.shape[0]
    t0, t1 = np.zeros(n), np.broadcast_to(np.asarray(t_end, np.float64), (n,)).copy()
    miss = np.full(n, not G.positive)
    cuts = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            par = np.abs(d[:, a]) < float(MR.PARALLEL)
            lo, hi = float(G.slo[a]), float(G.shi[a])
            miss |= par & ((o[:, a] < lo) | (o[:, a] > hi))
            ta, tb = (lo - o[:, a]) / d[:, a], (hi - o[:, a]) / d[:, a]
            t0 = np.where(par, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(par, t1, np.minimum(t1, np.maximum(ta, tb)))
            inner = G.planes[a][G.imin[a] + 1:G.imax[a] + 1].astype(np.float64) if G.positive else np.zeros(0)
            c = (inner[None, :] - o[:, a:a + 1]) / d[:, a:a + 1]
            cuts.append(np.where(par[:, None], -np.inf, c))
    miss |= ~(t0 < t1)
    t0, t1 = np.where(miss, 0.0, t0), np.where(miss, 0.0, t1)
    t = np.concatenate([t0[:, None], t1[:, None]] + cuts, axis=1)
    t = np.sort(np.clip(t, t0[:, None], t1[:, None]), axis=1)
    mid = 0.5 * (t[:, 1:] + t[:, :-1])
    idx = []
    for a in range(3):
        p = o[:, a:a + 1] + np.where(np.isfinite(mid), mid, 0.0) * d[:, a:a + 1]
        i = np.searchsorted(G.planes[a].astype(np.float64), p.reshape(-1), side="right").reshape(p.shape) - 1
        idx.append(np.clip(i, max(G.imin[a], 0), max(G.imax[a], 0)))
    s = float(F(sigma_t)) * G.density[idx[2], idx[1], idx[0]].astype(np.float64)
    return t, s


def tau64_many(G, sigma_t, o, d, t_end, upto=None):
    """float64 optical depths [n] of the segments, or of their parts t <= upto [n]"""
    t, s = pieces64_many(G, sigma_t, o, d, t_end)
    if upto is not None:
        t = np.minimum(t, np.asarray(upto, np.float64).reshape(-1, 1))
    with np.errstate(invalid="ignore"):
        return np.where(s > 0, s * (t[:, 1:] - t[:, :-1]), 0.0).sum(1)


def pieces64(G, sigma_t, o, d, t_end):
    """one ray: (t [k + 1], s [k]) with the pieces of length 0 kept; two empty arrays when the ray misses the support"""
    t, s = pieces64_many(G, sigma_t, o, d, t_end)
    if not t[0, 0] < t[0, -1]:
        return np.zeros(0), np.zeros(0)
    return t[0], s[0]


def tau64(G, sigma_t, o, d, t_end, upto=None):
    """float64 optical depth of one segment, or of its part t <= upto"""
    return float(tau64_many(G, sigma_t, o, d, t_end, None if upto is None else [upto])[0])


def clip64(G, o, d, t_end):
    """(t0, t1) of the float64 clip of one ray against the support box, (0, 0) when empty"""
    t, _ = pieces64_many(G, 1.0, o, d, t_end)
    return float(t[0, 0]), float(t[0, -1])


def bound(G, sigma_t, steps, t0, t1):
    """the stated error bound of the fp32 march's optical depth against float64"""
    return float(F(sigma_t)) * float(G.density.max()) * (steps + 2) * 2.0 ** -22 * max(abs(t0), abs(t1), 1.0)


# ---- grids and rays of the tests ------------------------------------------------------------------------------
BOX = ((-1.0, 0.5, -0.25), (2.0, 1.5, 0.75))


def make_grids(rng):
    """the three grids of the tests as (name, density [nz, ny, nx]): 1x1x1, 2x3x5 (nx = 2, ny = 3, nz = 5), 16^3 with about
    40 % zeros"""
    g16 = rng.uniform(0.1, 2.0, (16, 16, 16)).astype(F)
    g16[rng.uniform(size=g16.shape) < 0.4] = 0
    return [("1x1x1", np.full((1, 1, 1), 1.25, F)), ("2x3x5", rng.uniform(0.1, 2.0, (5, 3, 2)).astype(F)), ("16^3", g16)]


def make_rays(rng, n, lo=BOX[0], hi=BOX[1]):
    """n rays around the box: half aimed at it, half random; origins inside; an axis-parallel ray in a face plane and one
    ulp outside it; t_end inside the box, beyond it and +inf; tau_target 0, finite and +inf -> (o, d, t_end, tau_target)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = rng.uniform(-4, 4, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d[: n // 2] = rng.uniform(lo, hi, (n // 2, 3)) - o[: n // 2]
    k = n // 8
    o[:k] = rng.uniform(lo, hi, (k, 3)).astype(F)  # origins inside
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o[k], d[k] = (-5, F(hi[1]), 0.25), (1, 0, 0)                       # in a face plane
    o[k + 1], d[k + 1] = (-5, np.nextafter(F(hi[1]), INF), 0.25), (1, 0, 0)  # one ulp outside it
    o[k + 2], d[k + 2] = (0.5, 1.0, 5), (0, 0, -1)
    t_end = rng.uniform(0, 8, n).astype(F)
    t_end[rng.uniform(size=n) < 0.4] = INF
    target = (-np.log1p(-rng.uniform(0, 1, n)) * 1.5).astype(F)
    sel = rng.uniform(size=n)
    target[sel < 0.3] = INF
    target[(sel >= 0.3) & (sel < 0.35)] = 0
    return o, d, t_end, target
