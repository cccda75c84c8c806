"""Float64 twins of the light-tree selection (csrc/light_tree.hpp lt_select, csrc/light_tree_ref.hpp ltr_select), in numpy.

Not fp32 copies: the node fields are the fp32 values the device reads (pkg.light_tree_nodes), every operation on them is done
in float64.  What the fp32 code decides by a comparison, the twin decides too and reports how close the call was, so that a
test can tell a rounding difference at a decision from a wrong selection.

  intervals(nodes, p, n)                 DMT_LIGHTS_TREE: the partition of [0, 1) into one interval of u per light
  select(nodes, p, n, u, start, prec)    DMT_LIGHTS_TREE_REFERENCE: cut + walks, with a decision margin per case
"""
import numpy as np

LEAF = 0x80000000
ONE_MINUS = float(np.float32(0.99999994))     # the clamp of a remapped u
FLOOR = float(np.float32(1e-20))              # lt_importance's floor of the squared distance
MAX_SPLIT = 4                                 # kLightTreeMaxSplitSize
REF_MAX_DEPTH = 60                            # kLightTreeRefMaxDepth


def _f(nodes, name):
    return nodes[name].astype(np.float64)


def _safe_sqrt(x):
    return np.sqrt(np.fmax(0.0, x))           # fmaxf(0, NaN) = 0


# ---- DMT_LIGHTS_TREE ---------------------------------------------------------------------------------------------------------
def importance(nodes, idx, p, n):
    """lt_importance of node idx (scalar) at points p [k,3] with normals n [k,3] -> [k]."""
    lo, hi, phi = _f(nodes, "lo")[idx], _f(nodes, "hi")[idx], float(nodes["phi"][idx])
    c, d = 0.5 * (lo + hi), hi - lo
    half = 0.5 * np.sqrt((d * d).sum())
    w = p - c
    d2 = (w * w).sum(-1)
    dist2 = np.fmax(np.fmax(d2, half), FLOOR)
    outside = (d2 >= half * half) & (d2 > 0.0)
    with np.errstate(all="ignore"):
        s2 = np.where(outside, (half * half) / np.where(outside, d2, 1.0), 0.0)
        sin_b = np.where(outside, np.sqrt(s2), 0.0)
        cos_b = np.where(outside, np.sqrt(np.fmax(0.0, 1.0 - s2)), -1.0)
        cos_i = np.where(d2 > 0.0, np.abs((w * n).sum(-1) / np.sqrt(np.where(d2 > 0.0, d2, 1.0))), 1.0)
        sin_i = np.sqrt(np.fmax(0.0, 1.0 - cos_i * cos_i))
        cos_ib = np.where(cos_i > cos_b, 1.0, cos_i * cos_b + sin_i * sin_b)
        return np.fmax(phi * cos_ib / dist2, 0.0)


def intervals(nodes, p, n):
    """For each shading point the partition of [0, 1) that lt_select's walk induces: (light [k,m], lo [k,m], hi [k,m]) with one
    column per leaf in leaf order (left before right), hi - lo the float64 probability.  Where both children of a node have no
    importance, its whole interval goes to the first leaf below it with light -1 and the other leaves below get empty ones."""
    p, n = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(n, np.float64).reshape(-1, 3)
    k = p.shape[0]
    light, los, his = [], [], []
    stack = [(0, np.zeros(k), np.ones(k), np.zeros(k, bool))]
    while stack:
        at, a, b, dead = stack.pop()
        ref = int(nodes["ref"][at])
        if ref & LEAF:
            light.append(np.where(dead, -1, ref & (LEAF - 1))), los.append(a), his.append(b)
            continue
        i0, i1 = importance(nodes, ref, p, n), importance(nodes, ref + 1, p, n)
        total = i0 + i1
        dead = dead | ~(total > 0.0)
        with np.errstate(all="ignore"):
            mid = np.where(dead, b, a + (b - a) * (i0 / np.where(dead, 1.0, total)))
        stack.append((ref + 1, mid, b, dead))
        stack.append((ref, a, mid, dead))           # popped first: leaf order
    return np.stack(light, 1).astype(np.int64), np.stack(los, 1), np.stack(his, 1)


def locate(part, u):
    """Cases u [k,j] of the points of a partition -> (light [k,j], probability [k,j], distance of u to the nearest boundary
    between two intervals [k,j])."""
    light, lo, hi = part
    u = np.asarray(u, np.float64)
    inner = hi[:, :-1]                                                   # the ends of all intervals but the last
    col = (u[:, :, None] >= inner[:, None, :]).sum(-1)                   # the first interval whose end lies beyond u
    rows = np.arange(light.shape[0])[:, None]
    dist = np.abs(u[:, :, None] - inner[:, None, :]).min(-1) if inner.shape[1] else np.full(u.shape, np.inf)
    return light[rows, col], (hi - lo)[rows, col], dist


# ---- DMT_LIGHTS_TREE_REFERENCE -----------------------------------------------------------------------------------------------
def ref_importance(nodes, idx, p, n):
    """ltr_importance of nodes idx [k] at p [k,3], n [k,3] -> (importance [k], margin [k] of its two discontinuous comparisons)."""
    lo, hi = _f(nodes, "lo")[idx], _f(nodes, "hi")[idx]
    phi, axis = _f(nodes, "phi")[idx], _f(nodes, "w")[idx]
    cos_o, cos_e = _f(nodes, "cosTheta_o")[idx], _f(nodes, "cosTheta_e")[idx]
    with np.errstate(all="ignore"):
        c = (lo + hi) / 2.0
        d = p - c
        len2 = (d * d).sum(-1)
        w = d * (1.0 / np.sqrt(len2))[:, None]                            # len2 == 0: 0 x inf = NaN, as the code
        sin_o = _safe_sqrt(1.0 - cos_o * cos_o)
        e = hi - lo
        dist2 = np.fmax(len2, np.sqrt((e * e).sum(-1)) * 0.5)
        cos_w = (w * axis).sum(-1)
        sin_w = _safe_sqrt(1.0 - cos_w * cos_w)
        h = hi - c
        radius2 = (h * h).sum(-1)
        outside = ~(len2 < radius2)
        s2 = radius2 / len2
        sin_b = np.where(outside, np.sqrt(s2), 0.0)
        cos_b = np.where(outside, _safe_sqrt(1.0 - s2), -1.0)
        sub_cos = lambda sa, ca, sb, cb: np.where(ca > cb, 1.0, ca * cb + sa * sb)
        sub_sin = lambda sa, ca, sb, cb: np.where(ca > cb, 0.0, sa * cb - ca * sb)
        cos_wo, sin_wo = sub_cos(sin_w, cos_w, sin_o, cos_o), sub_sin(sin_w, cos_w, sin_o, cos_o)
        cos_p = sub_cos(sin_wo, cos_wo, sin_b, cos_b)
        cut = cos_p <= cos_e                                              # false for NaN
        cos_i = np.abs((w * n).sum(-1))
        sin_i = _safe_sqrt(1.0 - cos_i * cos_i)
        cos_ib = sub_cos(sin_i, cos_i, sin_b, cos_b)
        imp = np.where(cut, 0.0, np.fmax(phi * cos_ib * cos_p / dist2, 0.0))
        big = np.maximum(len2, radius2)
        m_sphere = np.where(big > 0.0, np.abs(len2 - radius2) / np.where(big > 0.0, big, 1.0), np.inf)   # 0 against 0 is exact in fp32 too
        m_cone = np.where(np.isnan(cos_p), np.inf, np.abs(cos_p - cos_e))
    return imp, np.minimum(m_sphere, m_cone)


def split_heuristic(nodes, p):
    """ltr_split_heuristic of every node at points p [k,3] -> (heuristic [k,m], margin [k,m] of its `a > 0` branch)."""
    lo, hi = _f(nodes, "lo")[None], _f(nodes, "hi")[None]
    with np.errstate(all="ignore"):
        c = (lo + hi) / 2.0
        d = p[:, None, :] - c
        e = hi - lo
        half = np.sqrt((e * e).sum(-1)) * 0.5
        dist = _safe_sqrt(np.fmax((d * d).sum(-1), half))
        a, b = np.fmax(dist - half, 0.0), dist + half
        ok = (a > 0.0) & (b > 0.0)
        sa, sb = np.where(ok, a, 1.0), np.where(ok, b, 1.0)
        amb = sa - sb
        r = 1.0 / (sa * sb)
        g_e2 = np.where(ok, r * r, 0.0)
        g_var = np.where(ok, amb * (sa * sa + sa * sb + sb * sb) / (3.0 * amb * sa ** 3 * sb ** 3) - r * r, 0.0)
        cnt = nodes["numEmitters"].astype(np.float64)[None]
        mean = _f(nodes, "phi")[None] / cnt
        e_var = _f(nodes, "varPhi")[None]
        sigma2 = (e_var * g_var + e_var * g_e2 + mean * mean * g_var) * (cnt * cnt)
        heur = np.sqrt(np.sqrt(np.fmax(1.0 / (1.0 + np.sqrt(sigma2)), 0.0)))
        big = np.maximum(dist, half)
        margin = np.where(big > 0.0, np.abs(dist - half) / np.where(big > 0.0, big, 1.0), np.inf)
    leaf = (nodes["light"] & LEAF) != 0
    return np.where(leaf[None], 1.0, heur), np.where(leaf[None], np.inf, margin)


def _cut(nodes, heur, hmargin, precision):
    """lightTreeAdaptiveSplit at one point (heur, hmargin: rows of split_heuristic) -> (cut node indices, margin)."""
    if int(nodes["light"][0]) & LEAF:
        return [0], np.inf
    cut, margin = [], np.inf
    parents, siblings = [], [0]
    while (siblings or parents) and len(cut) < MAX_SPLIT:
        if siblings:
            s = siblings.pop()
            enough = heur[s] >= precision
            if len(cut) + 1 == MAX_SPLIT:
                cut.append(s)                                             # the last slot takes the node whatever its heuristic
                continue
            margin = min(margin, abs(heur[s] - precision), hmargin[s])
            if enough:
                cut.append(s)
            elif not (int(nodes["light"][s]) & LEAF) and len(parents) < REF_MAX_DEPTH + 4:
                parents.append(s)
        else:
            at = parents.pop()
            left = int(nodes["left"][at])
            siblings += [left, left + 1]
    return cut, margin


def select(nodes, p, n, u, start, precision=0.5):
    """ltr_select at cases (p [k,3], n [k,3], u [k]) -> (indices [k,4] (-1 = none), pmfs [k,4], count [k], margin [k]).
    margin: the smallest distance, over the comparisons that change the control flow discontinuously, between the two sides --
    the bounding-sphere test (relative), the cone test, the split heuristic against `precision` (and its own `a > 0` branch),
    and each child choice |up - w0| / sum divided by how much the walks so far have stretched u."""
    p, n = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(n, np.float64).reshape(-1, 3)
    u = np.asarray(u, np.float64).reshape(-1).copy()
    k = p.shape[0]
    points, inverse = np.unique(p, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    heur, hmargin = split_heuristic(nodes, points)
    cuts = np.full((points.shape[0], MAX_SPLIT), -1, np.int64)
    cut_margin = np.zeros(points.shape[0])
    for j in range(points.shape[0]):
        c, cut_margin[j] = _cut(nodes, heur[j], hmargin[j], precision)
        cuts[j, :len(c)] = c
    cuts, margin = cuts[inverse], cut_margin[inverse].copy()
    idx, pmfs, count = np.full((k, MAX_SPLIT), -1, np.int64), np.zeros((k, MAX_SPLIT)), np.zeros(k, np.int64)
    amp = np.ones(k)
    leaf_of = (nodes["light"] & LEAF) != 0
    left_of = nodes["left"].astype(np.int64)
    for slot in range(MAX_SPLIT):
        at = cuts[:, slot].copy()
        walking = at >= 0
        pmf = np.full(k, float(start))
        for _ in range(REF_MAX_DEPTH + 4):
            rows = np.nonzero(walking)[0]
            if rows.size == 0:
                break
            a = at[rows]
            leaf = leaf_of[a]
            done = rows[leaf]                                            # a leaf: selected where it has importance here
            if done.size:
                imp, m = ref_importance(nodes, at[done], p[done], n[done])
                margin[done] = np.minimum(margin[done], m)
                hit = done[imp > 0.0]
                idx[hit, count[hit]], pmfs[hit, count[hit]] = nodes["light"][at[hit]] & (LEAF - 1), pmf[hit]
                count[hit] += 1
                walking[done] = False
            rows = rows[~leaf]
            if rows.size == 0:
                continue
            l = left_of[at[rows]]
            w0, m0 = ref_importance(nodes, l, p[rows], n[rows])
            w1, m1 = ref_importance(nodes, l + 1, p[rows], n[rows])
            margin[rows] = np.minimum(margin[rows], np.minimum(m0, m1))
            none = (w0 == 0.0) & (w1 == 0.0)
            walking[rows[none]] = False                                  # this cut node yields no light
            rows, l, w0, w1 = rows[~none], l[~none], w0[~none], w1[~none]
            total = w0 + w1
            up = u[rows] * total
            second = w0 <= up
            with np.errstate(all="ignore"):
                margin[rows] = np.minimum(margin[rows], np.abs(up - w0) / total / amp[rows])
                acc, wc = np.where(second, w0, 0.0), np.where(second, w1, w0)
                pmf[rows] *= wc / total
                u[rows] = np.fmin((up - acc) / wc, ONE_MINUS)
                amp[rows] *= total / wc
            at[rows] = l + second
    return idx, pmfs, count, margin
