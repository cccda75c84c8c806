"""Float64 twin of the emitter tree's selection (csrc/emitter_tree.hpp et_importance / et_select / et_pmf), in numpy, and the
structural checks of a built tree.

Not an fp32 copy: the node fields are the fp32 values host and device read (pkg.emitter_tree_nodes), every operation on them
is done in float64.  What the fp32 code decides by a comparison, the twin decides too and reports how close the call was.

  importance(nodes, idx, p, n)     -> (importance [k], margin [k])
  intervals(nodes, p, n)           the partition of [0, 1) into one interval of u per emitter, and per interval the smallest
                                   margin met on the way to it
  locate(part, u)                  cases -> (emitter, probability, distance of u to an interval end, margin of the walk)
  check_structure(nodes, trails, lengths, count, guard)

Margins.  Only one comparison of et_importance is discontinuous: `len2 >= radius2`, where cos theta_b jumps from 0 to -1;
its margin is |len2 - radius2| / max(len2, radius2).  The others -- `cos theta' <= 0` and the three clamped subtractions
(cos a > cos b ? 1 : cos(a - b)) -- have both sides agree at equality.  The twin does not take that on trust: wherever such a
comparison is within EPS it measures the jump between its two sides (in cosine units), and counts the comparison into the
margin if the jump exceeds EPS.  A walk's margin is the smallest over both children of every node on its path.
"""
import numpy as np

LEAF = 0x80000000
ONE_MINUS = float(np.float32(0.99999994))
FLOOR = float(np.float32(1e-20))
EPS = 1e-6
MAX_DEPTH = 60                                # kEmitterTreeMaxDepth


def _f(nodes, name):
    return nodes[name].astype(np.float64)


def _safe_sqrt(x):
    return np.sqrt(np.fmax(0.0, x))


def _branch(lhs, rhs, a, b):
    """lhs > rhs ? a : b, and the margin of the comparison: |lhs - rhs| where it is within EPS AND its sides differ by more than EPS."""
    close = (np.abs(lhs - rhs) < EPS) & (np.abs(a - b) > EPS)
    return np.where(lhs > rhs, a, b), np.where(close, np.abs(lhs - rhs), np.inf)


def importance(nodes, idx, p, n):
    """et_importance of node idx (scalar) at points p [k,3] with normals n [k,3] -> (importance [k], margin [k])."""
    lo, hi, phi = _f(nodes, "lo")[idx], _f(nodes, "hi")[idx], float(nodes["phi"][idx])
    axis, cos_o = _f(nodes, "axis")[idx], float(nodes["cosO"][idx])
    with np.errstate(all="ignore"):
        c, d = 0.5 * (lo + hi), hi - lo
        radius2 = 0.25 * (d * d).sum()
        w = p - c
        len2 = (w * w).sum(-1)
        d2 = np.fmax(np.fmax(len2, radius2), FLOOR)
        outside = (len2 >= radius2) & (len2 > 0.0)
        s2 = np.where(outside, radius2 / np.where(outside, len2, 1.0), 0.0)
        sin_b = np.where(outside, np.sqrt(s2), 0.0)
        cos_b = np.where(outside, _safe_sqrt(1.0 - s2), -1.0)
        big = np.maximum(len2, radius2)
        margin = np.where(big > 0.0, np.abs(len2 - radius2) / np.where(big > 0.0, big, 1.0), np.inf)   # 0 against 0 is exact in fp32 too
        wi = w * np.where(len2 > 0.0, 1.0 / np.sqrt(np.where(len2 > 0.0, len2, 1.0)), 0.0)[:, None]
        cos_w = (wi * axis).sum(-1)
        sin_w = _safe_sqrt(1.0 - cos_w * cos_w)
        sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
        cos_x, m1 = _branch(cos_w, cos_o, 1.0, cos_w * cos_o + sin_w * sin_o)
        sin_x = np.where(cos_w > cos_o, 0.0, sin_w * cos_o - cos_w * sin_o)
        cos_p, m2 = _branch(cos_x, cos_b, 1.0, cos_x * cos_b + sin_x * sin_b)
        cut = ~(cos_p > 0.0)
        # `cos_p <= 0 -> 0`: the two sides are 0 and a product with the factor cos_p, so the jump, in cosine units, is |cos_p|
        # itself: within EPS of the comparison it is below EPS by construction, and the comparison never enters the margin
        cos_i = np.abs((wi * n).sum(-1))
        sin_i = _safe_sqrt(1.0 - cos_i * cos_i)
        cos_ib, m4 = _branch(cos_i, cos_b, 1.0, cos_i * cos_b + sin_i * sin_b)
        imp = np.where(cut, 0.0, np.fmax(phi * cos_p * cos_ib / d2, 0.0))
    return imp, np.minimum(np.minimum(margin, m1), np.minimum(m2, m4))


def intervals(nodes, p, n):
    """For each shading point the partition of [0, 1) that et_select's walk induces: (emitter [k,m], lo [k,m], hi [k,m],
    margin [k,m]) with one column per leaf in leaf order (left before right), hi - lo the float64 probability.  Where neither
    child of a node has importance, its whole interval goes to the first leaf below it with emitter -1 and the other leaves
    below get empty ones."""
    p, n = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(n, np.float64).reshape(-1, 3)
    k = p.shape[0]
    emitter, los, his, margins = [], [], [], []
    root = int(nodes["ref"][0])
    if root & LEAF:
        imp, m = importance(nodes, 0, p, n)
        return (np.where(imp > 0.0, root & (LEAF - 1), -1)[:, None].astype(np.int64), np.zeros((k, 1)), np.ones((k, 1)), m[:, None])
    stack = [(root, np.zeros(k), np.ones(k), np.zeros(k, bool), np.full(k, np.inf))]
    while stack:
        ref, a, b, dead, margin = stack.pop()
        if ref & LEAF:
            emitter.append(np.where(dead, -1, ref & (LEAF - 1))), los.append(a), his.append(b), margins.append(margin)
            continue
        (i0, m0), (i1, m1) = importance(nodes, ref, p, n), importance(nodes, ref + 1, p, n)
        total = i0 + i1
        dead = dead | ~(total > 0.0)
        margin = np.minimum(margin, np.minimum(m0, m1))
        with np.errstate(all="ignore"):
            mid = np.where(dead, b, a + (b - a) * (i0 / np.where(dead, 1.0, total)))
        stack.append((int(nodes["ref"][ref + 1]), mid, b, dead, margin))
        stack.append((int(nodes["ref"][ref]), a, mid, dead, margin))       # popped first: leaf order
    return np.stack(emitter, 1).astype(np.int64), np.stack(los, 1), np.stack(his, 1), np.stack(margins, 1)


def locate(part, u):
    """Cases u [k,j] of the points of a partition -> (emitter [k,j], probability [k,j], distance of u to the nearest boundary
    between two intervals [k,j], margin of the walk to that interval [k,j])."""
    emitter, lo, hi, margin = part
    u = np.asarray(u, np.float64)
    inner = hi[:, :-1]
    col = (u[:, :, None] >= inner[:, None, :]).sum(-1)
    rows = np.arange(emitter.shape[0])[:, None]
    dist = np.abs(u[:, :, None] - inner[:, None, :]).min(-1) if inner.shape[1] else np.full(u.shape, np.inf)
    return emitter[rows, col], (hi - lo)[rows, col], dist, margin[rows, col]


def per_emitter(part, count):
    """The probability of every emitter index under a partition [k, count]."""
    emitter, lo, hi, _ = part
    out = np.zeros((emitter.shape[0], count))
    for j in range(emitter.shape[1]):
        ok = emitter[:, j] >= 0
        out[ok, emitter[ok, j]] += (hi - lo)[ok, j]
    return out


# ---- structure ---------------------------------------------------------------------------------------------------------------
def _angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


def _theta(cos_o):
    return np.pi if cos_o <= -1.0 else float(np.arccos(min(1.0, cos_o)))


def check_structure(nodes, trails, lengths, count, guard=MAX_DEPTH):
    """Every emitter in exactly one leaf, its trail leads there, every child's box, flux and stored cone inside its
    parent's, depth (levels) within the guard.  Returns the depth."""
    assert len(nodes) == 2 * count - 1
    ref = nodes["ref"].astype(np.int64)
    leaf = (ref & LEAF) != 0
    assert sorted((ref[leaf] & (LEAF - 1)).tolist()) == list(range(count))
    lo, hi, phi, axis, cos_o = _f(nodes, "lo"), _f(nodes, "hi"), _f(nodes, "phi"), _f(nodes, "axis"), _f(nodes, "cosO")
    depth, stack, seen = 0, [(0, 1)], 0
    while stack:
        at, level = stack.pop()
        depth, seen = max(depth, level), seen + 1
        if leaf[at]:
            continue
        l = int(ref[at])
        assert 0 < l and l + 1 < len(nodes)
        assert phi[at] <= (phi[l] + phi[l + 1]) * (1 + 1e-6) + 1e-30 and phi[at] >= max(phi[l], phi[l + 1]) * (1 - 1e-6)
        for c in (l, l + 1):
            assert (lo[c] >= lo[at]).all() and (hi[c] <= hi[at]).all(), (at, c)
            tp, tc = _theta(cos_o[at]), _theta(cos_o[c])
            assert tp >= np.pi or _angle(axis[at], axis[c]) + tc <= tp + 1e-9, (at, c, tp, tc, _angle(axis[at], axis[c]))
            stack.append((c, level + 1))
    assert seen == len(nodes)
    assert depth <= guard
    for e in range(count):
        at, bits = 0, int(trails[e])
        assert 0 <= lengths[e] <= depth - 1
        for k in range(int(lengths[e])):
            assert not leaf[at]
            at = int(ref[at]) + ((bits >> k) & 1)
        assert leaf[at] and (int(ref[at]) & (LEAF - 1)) == e, e
        assert bits >> int(lengths[e]) == 0
    return depth
