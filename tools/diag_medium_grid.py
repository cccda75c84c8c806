#!/usr/bin/env python3
"""What the heterogeneous medium costs: kernel time of the *_medium_grid rows against the *_medium rows,
on one build in one process, the configurations alternating round by round (the order rotates), medians from
dmt_kernel_time -- the method of tools/diag_medium.py.

The medium is the scene's bounds with an optical depth of 2 across the longest side, white fog, g = 0.5.
homogeneous: dmt_set_medium alone (the *_medium rows).  const_32 / const_128: the same fog as a constant grid of density
1 -- the same picture up to rounding, so the difference is the price of the march alone, at 32 and at 128 voxels per side.
plume_128: a 128^3 grid that is 1 inside the central half of every axis (one eighth of the voxels) and 0 elsewhere, which
shows what the support box saves: segments outside it never enter the loop.

steps: the mean number of march iterations over the segments that meet the support, from the device probe
(dmt_test_medium_grid) on 65 536 segments between two uniform points of the box -- a stand-in for path and shadow
segments, not a count taken inside the render kernel.

Workloads: the Cornell box 1024 x 1024 x 256 spp, depth 8, brute force and BVH.  Prints one JSON line per workload.
Usage: python tools/diag_medium_grid.py [--rounds 3] [--warmup 1] [--small]"""
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


def grids():
    plume = np.zeros((128, 128, 128), np.float32)
    plume[32:96, 32:96, 32:96] = 1.0
    return {"const_32": np.ones((32, 32, 32), np.float32), "const_128": np.ones((128, 128, 128), np.float32), "plume_128": plume}


def mean_steps(r, lo, hi, sigma_t, dens, n=65536):
    rng = np.random.default_rng(5)
    a, b = rng.uniform(lo, hi, (n, 3)), rng.uniform(lo, hi, (n, 3))
    length = np.linalg.norm(b - a, axis=1)
    out = r.test_medium_grid(lo, hi, sigma_t, dens, a, (b - a) / length[:, None], length, np.full(n, np.inf))
    met = out["steps"] > 0
    return round(float(out["steps"][met].mean()), 2), round(float(met.mean()), 3)


def measure(pkg, name, scene, accel, spp, depth, rounds, warmup):
    lo, hi = bounds(scene)
    side = float((hi - lo).max())
    fog = dict(sigma_t=2.0 / side, albedo=(1, 1, 1), g=0.5, box_min=lo, box_max=hi)
    G = grids()
    configs = ["homogeneous"] + list(G)
    times = {c: [] for c in configs}
    info, steps = {}, {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        r.set_accel(accel)
        r.set_medium(**fog)
        for c, dens in G.items():
            steps[c] = dict(zip(("mean_steps", "segments_meeting_support"), mean_steps(r, lo, hi, fog["sigma_t"], dens)))

        def run(c):
            if c == "homogeneous":
                r.clear_medium_grid()
            else:
                r.set_medium_grid(G[c])
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
           "cost_vs_homogeneous": {c: round(med[c] / med["homogeneous"] - 1.0, 4) for c in configs if c != "homogeneous"},
           "steps": steps, "info": info}
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
