"""numpy restatement of the medium's spectrum (include/dmt_hip.h dmt_set_medium_spectrum): the event at the
end of a path segment -- the channel choice, the target, collision or pass, the one-sample balance-heuristic weights.

Two layers, as medium_ref.  The hash and the channel choice are exact: integer arithmetic and float32 operations in the
stated order, so they give the device's and the host twin's decisions bit for bit.  The target and the weights are float64:
what the fp32 code approximates; the target is then rounded once to float32, as the definition states it.
"""
import numpy as np

F = np.float32
CHOICE_STREAM = 2 ** 31  # the depth offset of the channel choice's hash stream


def mix_bits32(v):
    """lens_ref.mix_bits32, vectorised over uint64 arrays holding 32-bit values"""
    v = np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return v ^ (v >> np.uint64(16))


def medium_u(h, depth):
    """medium_ref.medium_u for arrays: float32 in [0, 1), exact"""
    h, depth = np.asarray(h, np.uint64), np.asarray(depth, np.uint64)
    x = mix_bits32(h ^ mix_bits32((np.uint64(0x9E3779B9) * ((depth + np.uint64(1)) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)))
    return (x >> np.uint64(8)).astype(F) * F(2.0 ** -24)


def channels(k):
    """(m, q float32 [3]) of channel extinctions k: the reference channel (largest k, lowest index on a tie) and
    q_c = fl32(k_c / k_m), correctly rounded (numpy's float32 division)"""
    k = np.asarray(k, F)
    m = int(np.argmax(k))
    return m, (k / k[m]).astype(F)


def choose(beta, h, depth):
    """the channel choice, exact: (j [n] with -1 for an all-zero beta, p float64 [n, 3])"""
    b = np.asarray(beta, F).reshape(-1, 3)
    s01 = (b[:, 0] + b[:, 1]).astype(F)
    total = (s01 + b[:, 2]).astype(F)
    x = (medium_u(h, np.asarray(depth, np.uint64) + np.uint64(CHOICE_STREAM)) * total).astype(F)
    j = np.where(x < b[:, 0], 0, np.where(x < s01, 1, 2))
    j = np.where((j == 2) & ~(b[:, 2] > 0), np.where(b[:, 1] > 0, 1, 0), j)
    j = np.where((j == 1) & ~(b[:, 1] > 0), 0, j)
    ok = total > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        p = b.astype(np.float64) / b.astype(np.float64).sum(1, keepdims=True)
    return np.where(ok, j, -1), np.where(ok[:, None], p, 0.0)


def event64(k, beta, h, depth, tau_seg):
    """the event of n segments -> dict(channel [n], collided [n] bool, tau_at [n] float64, weight [n, 3] float64, tau [n, 3]
    the channels' optical depths at the event)"""
    _, q32 = channels(k)
    q = q32.astype(np.float64)
    tau_seg = np.asarray(tau_seg, F).astype(np.float64)
    j, p = choose(beta, h, depth)
    n = j.shape[0]
    qj = q[np.maximum(j, 0)]
    u = medium_u(h, depth).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.where(qj > 0, -np.log1p(-u) / np.where(qj > 0, qj, 1.0), np.inf).astype(F).astype(np.float64)  # rounded once, as stated
    collided = (j >= 0) & (T < tau_seg)
    tau_at = np.where(collided, T, tau_seg)
    with np.errstate(invalid="ignore"):
        tau = np.where(q[None, :] > 0, q[None, :] * tau_at[:, None], 0.0)
    t = np.exp(-tau)
    num = np.where(collided[:, None], q[None, :] * t, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = num / (p * num).sum(1, keepdims=True)
    w = np.where((j >= 0)[:, None], w, 1.0)
    assert w.shape == (n, 3)
    return dict(channel=j.astype(np.int32), collided=collided, tau_at=tau_at, weight=w, tau=tau, p=p, T=T)


def small_u_indices(depth, count, span=1 << 20):
    """the `count` Halton indices below `span` whose free-flight number at `depth` is smallest (u near 0)"""
    h = np.arange(span, dtype=np.uint64)
    u = medium_u(h, np.full(span, depth, np.uint64))
    return h[np.argsort(u, kind="stable")[:count]].astype(np.uint32)


def make_cases(rng, k, n):
    """n cases for channel extinctions k -> (beta [n, 3], h [n], depth [n], tau_seg [n]) float32 / uint32: throughputs with
    a zero channel and with two, u near 0, tau_seg = +inf, and tau_seg one float below, at and one float above the target"""
    beta = rng.uniform(0.05, 2.0, (n, 3)).astype(F)
    zero = rng.uniform(size=n)
    rows = np.nonzero(zero < 0.10)[0]
    beta[rows, rng.integers(0, 3, rows.size)] = 0
    two = zero < 0.03
    beta[two] = 0
    beta[two, rng.integers(0, 3, int(two.sum()))] = rng.uniform(0.1, 2.0, int(two.sum())).astype(F)
    beta[:4] = 0  # no event at all
    h = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, 9, n).astype(np.uint32)
    h[4:68], depth[4:68] = small_u_indices(3, 64), 3
    tau_seg = rng.uniform(0.01, 6.0, n).astype(F)
    tau_seg[rng.uniform(size=n) < 0.03] = np.inf
    near = np.nonzero(rng.uniform(size=n) < 0.12)[0]
    T = event64(k, beta, h, depth, tau_seg)["T"].astype(F)
    fin = near[np.isfinite(T[near]) & (T[near] > 0)]
    third = fin.size // 3
    tau_seg[fin[:third]] = np.nextafter(T[fin[:third]], F(0))
    tau_seg[fin[third:2 * third]] = T[fin[third:2 * third]]
    tau_seg[fin[2 * third:]] = np.nextafter(T[fin[2 * third:]], F(np.inf))
    return beta, h, depth, tau_seg


# the channel extinctions of the probe tests: three well apart, a channel with k = 0, the reference channel first, a tie
K_SETS = ((0.2, 0.8, 2.0), (1.0, 0.0, 2.0), (3.0, 1.0, 0.0), (0.7, 0.7, 0.1))


def compare(got, k, beta, h, depth, tau_seg):
    """a twin's or the probe's outputs against event64 -> (decisions agree, kept share, worst relative weight error over
    the kept cases: every channel's optical depth <= 8)"""
    ref = event64(k, beta, h, depth, tau_seg)
    same = bool((got["channel"] == ref["channel"]).all() and (got["collided"] == ref["collided"]).all())
    keep = (ref["tau"] <= 8).all(1)
    w, want = got["weight"].astype(np.float64)[keep], ref["weight"][keep]
    err = np.abs(w - want) / np.where(want > 0, want, 1.0)
    return same, float(keep.mean()), float(err.max()), ref
