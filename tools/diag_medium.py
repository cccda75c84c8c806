#!/usr/bin/env python3
"""What the participating medium costs: kernel time of the *_medium rows against their static twins, on one
build in one process, static and medium launches alternating round by round (the order rotates).

medium_outside: the medium is set but its box lies outside the scene, so no segment meets it and the film is the static
one; the difference is the price of the mechanism alone -- the clip of every path segment and every shadow segment, and
the row's registers.  medium_od2: the box is the scene's bounds with an optical depth of 2 across its longest side, white
fog, g = 0.5: paths scatter, which adds vertices (and changes the picture, so this column is a capability cost).

Workloads: the Cornell box 1024 x 1024 x 256 spp, brute force and BVH.  Prints one JSON line per workload.
Usage: python tools/diag_medium.py [--rounds 3] [--warmup 1] [--small]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402


def bounds(scene):
    lo = np.array([np.asarray(a, np.float32).reshape(-1, 4)[:, :3].min() for a in (scene.xs, scene.ys, scene.zs)], np.float64)
    hi = np.array([np.asarray(a, np.float32).reshape(-1, 4)[:, :3].max() for a in (scene.xs, scene.ys, scene.zs)], np.float64)
    return lo, hi


def measure(pkg, name, scene, accel, spp, depth, rounds, warmup):
    lo, hi = bounds(scene)
    side = float((hi - lo).max())
    media = {"medium_outside": dict(sigma_t=2.0 / side, albedo=(1, 1, 1), g=0.5, box_min=hi + side, box_max=hi + 2 * side),
             "medium_od2": dict(sigma_t=2.0 / side, albedo=(1, 1, 1), g=0.5, box_min=lo, box_max=hi)}
    configs = ["static", "medium_outside", "medium_od2"]
    times = {c: [] for c in configs}
    info = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        r.set_accel(accel)

        def run(c):
            if c == "static":
                r.clear_medium()
            else:
                r.set_medium(**media[c])
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(spp)
            r.sync()
            ms = r.kernel_time(reset=True)[0]
            info[c] = {"kernel": r.kernel_info()}
            return ms

        for k in range(warmup + rounds):
            order = configs[k % len(configs):] + configs[:k % len(configs)]
            for c in order:
                ms = run(c)
                if k >= warmup:
                    times[c].append(ms)
        r.clear_medium()
    med = {c: statistics.median(times[c]) for c in configs}
    out = {"workload": name, "accel": "bvh" if accel else "brute", "spp": spp, "max_depth": depth, "rounds": rounds,
           "sigma_t": round(2.0 / side, 6),
           "kernel_ms": {c: round(med[c], 3) for c in configs},
           "spread": {c: round((max(times[c]) - min(times[c])) / med[c], 4) for c in configs},
           "cost_vs_static": {c: round(med[c] / med["static"] - 1.0, 4) for c in configs if c != "static"},
           "info": info}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a quick pass over a small version of the workloads")
    args = ap.parse_args()
    pkg = graft.load_package()
    H = pkg.host_scene
    res, spp = (128, 16) if args.small else (1024, 256)
    for accel in (0, 1):
        measure(pkg, f"cornell_{res}x{res}", H.cornell_box(res, res), accel, spp, 8, args.rounds, args.warmup)


if __name__ == "__main__":
    main()
