#!/usr/bin/env python3
"""What motion blur costs: kernel time of the *_motion rows against their static twins, on one build in one
process, parent-row and motion-row launches alternating round by round (the order rotates).

Key 1 = key 0 ("zero displacement") keeps the tree's shape and every ray, so the difference is the price of the mechanism:
the delta records, the fmafs, the rebuilt post-hit record, and the samples computed instead of read from the sampler table
(static_table_off isolates that last part).  On the large scene a second point displaces every triangle by a random vector
of one mean edge length, which shows what the looser union boxes cost on top.

Workloads: the Cornell box 1024 x 1024 x 256 spp (brute force and BVH) and 1 M random triangles 512 x 512 x 64 spp (BVH).
Prints one JSON line per workload.  Usage: python tools/diag_motion.py [--rounds 3] [--warmup 1] [--small]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402


def soup(scene):
    return tuple(np.ascontiguousarray(a, np.float32).reshape(-1) for a in (scene.xs, scene.ys, scene.zs))


def displaced(k0, scale, seed=1):
    """every triangle moved rigidly by a random vector of length `scale`"""
    rng = np.random.default_rng(seed)
    n = k0[0].size // 4
    d = rng.normal(size=(n, 3))
    d *= scale / np.linalg.norm(d, axis=1, keepdims=True)
    return tuple((a.reshape(n, 4) + np.concatenate([np.repeat(d[:, k:k + 1], 3, 1), np.zeros((n, 1))], 1).astype(np.float32)).reshape(-1).astype(np.float32)
                 for k, a in enumerate(k0))


def mean_edge(k0):
    T = np.stack([a.reshape(-1, 4)[:, :3] for a in k0], axis=2).astype(np.float64)
    return float(np.mean([np.linalg.norm(T[:, i] - T[:, (i + 1) % 3], axis=1).mean() for i in range(3)]))


def measure(pkg, name, scene, accel, spp, depth, rounds, warmup, with_displacement):
    k0 = soup(scene)
    configs = ["static", "static_table_off", "motion_zero"] + (["motion_displaced"] if with_displacement else [])
    times = {c: [] for c in configs}
    info = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        r.set_accel(accel)
        edge = mean_edge(k0)
        keys = {"motion_zero": k0, "motion_displaced": displaced(k0, edge) if with_displacement else None}

        def run(c):
            if c.startswith("motion"):
                r.set_motion(*keys[c])
                info[c] = r.motion_info()
            else:
                r.clear_motion()
            r.set_sampler_table(0 if c == "static_table_off" else 1)
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(spp)
            r.sync()
            ms = r.kernel_time(reset=True)[0]
            if c.startswith("motion"):
                info[c]["kernel"] = r.kernel_info()
            else:
                info["static"] = {"kernel": r.kernel_info()}
            return ms

        for k in range(warmup + rounds):
            order = configs[k % len(configs):] + configs[:k % len(configs)]
            for c in order:
                ms = run(c)
                if k >= warmup:
                    times[c].append(ms)
        r.clear_motion()
        r.set_sampler_table(1)
    med = {c: statistics.median(times[c]) for c in configs}
    out = {"workload": name, "accel": "bvh" if accel else "brute", "spp": spp, "max_depth": depth, "rounds": rounds,
           "mean_edge": round(edge, 6),
           "kernel_ms": {c: round(med[c], 3) for c in configs},
           "spread": {c: round((max(times[c]) - min(times[c])) / med[c], 4) for c in configs},
           "cost_vs_static": {c: round(med[c] / med["static"] - 1.0, 4) for c in configs if c != "static"},
           "cost_vs_static_table_off": {c: round(med[c] / med["static_table_off"] - 1.0, 4) for c in configs if c.startswith("motion")},
           "info": info}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a quick pass over small versions of the workloads")
    args = ap.parse_args()
    pkg = graft.load_package()
    H = pkg.host_scene
    res, spp, ntri, res2, spp2 = (128, 16, 20000, 64, 4) if args.small else (1024, 256, 1000000, 512, 64)
    for accel in (0, 1):
        measure(pkg, f"cornell_{res}x{res}", H.cornell_box(res, res), accel, spp, 8, args.rounds, args.warmup, False)
    measure(pkg, f"random_{ntri}_{res2}x{res2}", H.random_triangle_scene(ntri, width=res2, height=res2), 1, spp2, 8, args.rounds, args.warmup, True)


if __name__ == "__main__":
    main()
