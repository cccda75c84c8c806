#!/usr/bin/env python3
"""What the medium's spectrum costs: kernel time of each *_rgb row against its grey twin, on one build in
one process, the two configurations alternating round by round (the order swaps), medians from dmt_kernel_time -- the
method of tools/diag_medium.py -- and each row's registers, LDS and resident blocks from dmt_kernel_info.

The fog is that of the tests: sigma_t 0.6, albedo (0.9, 0.8, 0.7), g 0.4 in a box inside the Cornell box.  grey: the fog
alone; rgb: the same fog with the extinction colour (0.25, 1, 2.5), so the reference channel marches at 2.5 times the grey
extinction (more collisions: part of the ratio is the picture, not the code).  rgb_same_depth: sigma_t / 2.5 with that
colour, so that the reference channel's extinction is the grey one.  The grid rows: the same with a constant 32^3 grid.

Workload: the Cornell box 256 x 256 x 64 spp, depth 8; brute force and BVH, without and with an env map.  Prints one JSON
line per row pair.
Usage: python tools/diag_medium_spectrum.py [--rounds 5] [--warmup 1]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

FOG = dict(sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))
COLOUR = (0.25, 1.0, 2.5)


def measure(pkg, scene, accel, env, grid, res, spp, depth, rounds, warmup):
    configs = ["grey", "rgb", "rgb_same_depth"]
    times = {c: [] for c in configs}
    info = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        if env:
            r.upload_envmap(np.random.default_rng(2).uniform(0.0, 2.0, (8, 16, 3)).astype(np.float32))
        r.set_limits(depth)
        r.set_accel(accel)
        r.set_medium(**FOG)
        if grid:
            r.set_medium_grid(np.ones((32, 32, 32), np.float32))

        def run(c):
            r.set_medium(**{**FOG, "sigma_t": FOG["sigma_t"] / (2.5 if c == "rgb_same_depth" else 1.0)})
            if c == "grey":
                r.clear_medium_spectrum()
            else:
                r.set_medium_spectrum(COLOUR)
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(spp)
            r.sync()
            ms = r.kernel_time(reset=True)[0]
            info[c] = r.kernel_info()
            return ms

        for k in range(warmup + rounds):
            for c in configs[k % 3:] + configs[:k % 3]:
                ms = run(c)
                if k >= warmup:
                    times[c].append(ms)
    med = {c: statistics.median(times[c]) for c in configs}
    row = "k_megakernel" + ("_bvh" if accel else "") + ("_env" if env else "") + "_medium" + ("_grid" if grid else "") + "_rgb"
    print(json.dumps({"row": row, "workload": f"cornell_{res}x{res}x{spp}", "max_depth": depth, "rounds": rounds,
                      "kernel_ms": {c: round(med[c], 3) for c in configs},
                      "spread": {c: round((max(times[c]) - min(times[c])) / med[c], 4) for c in configs},
                      "rgb_over_grey": round(med["rgb"] / med["grey"], 4), "rgb_same_depth_over_grey": round(med["rgb_same_depth"] / med["grey"], 4),
                      "info": info}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    args = ap.parse_args()
    pkg = graft.load_package()
    scene = pkg.host_scene.cornell_box(args.res, args.res)
    for grid in (False, True):
        for env in (False, True):
            for accel in (0, 1):
                measure(pkg, scene, accel, env, grid, args.res, args.spp, 8, args.rounds, args.warmup)


if __name__ == "__main__":
    main()
