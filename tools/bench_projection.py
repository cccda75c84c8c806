#!/usr/bin/env python3
"""What a camera projection costs: the flagship Cornell configuration of bench.py (1024 x 1024, 1024 spp,
bounce cap 8, brute force) rendered under the perspective camera and under each other model, on one build in one process.

The configurations alternate round by round (the order rotates), as in tools/bench_lens.py; the figure per configuration is
the median of its rounds' kernel times (HIP events), the spread (max - min) / median.  A projection changes which rays are
traced, so most of a difference is the scene seen through other rays (an equirect film looks at all six walls), not the
projection's arithmetic in the cold tail.

Prints one JSON line.  Usage: python tools/bench_projection.py [--rounds 3] [--spp 1024] [--res 1024] [--warmup 1]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--ortho-height", type=float, default=2.0)
    ap.add_argument("--fisheye-fov", type=float, default=150.0)
    args = ap.parse_args()
    pkg = graft.load_package()
    scene = pkg.host_scene.cornell_box(args.res, args.res)
    configs = {"perspective": ("perspective", 0.0), "orthographic": ("orthographic", args.ortho_height), "equirect": ("equirect", 0.0),
               "fisheye": ("fisheye", args.fisheye_fov)}
    names = list(configs)
    times = {n: [] for n in names}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(args.max_depth)
        for k in range(args.warmup + args.rounds):
            for n in names[k % len(names):] + names[:k % len(names)]:
                r.set_projection(*configs[n])
                r.film_clear()
                r.sync()
                r.kernel_time(reset=True)
                r.render(args.spp)
                r.sync()
                ms = r.kernel_time(reset=True)[0]
                if k >= args.warmup:
                    times[n].append(ms)
        r.set_projection("perspective")
    med = {n: statistics.median(times[n]) for n in names}
    out = {"workload": f"cornell_{args.res}x{args.res}_{args.spp}spp_{args.max_depth}bounces", "rounds": args.rounds,
           "kernel_ms": {n: round(med[n], 3) for n in names},
           "spread": {n: round((max(times[n]) - min(times[n])) / med[n], 4) for n in names},
           "relative_to_perspective": {n: round(med[n] / med["perspective"] - 1.0, 4) for n in names if n != "perspective"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
