#!/usr/bin/env python3
"""What a pixel filter costs: the flagship Cornell configuration of bench.py (1024 x 1024, 1024 spp, bounce
cap 8, brute force) rendered with the filter off (box 0.5, the default) and on (Gaussian, radius 1.5, sigma 0.5), with the
sampler table off (computed sample preparation: the filter runs in prepare_sample's cold tail) and forced (the table's jitter
plane holds the warped jitter: the main path runs, no tail), on one build in one process.

The four configurations alternate round by round (the order rotates), so clock drift and neighbours on the machine hit all
of them alike; the figure per configuration is the median of its rounds' kernel times (HIP events), and the spread is
(max - min) / median over the rounds.  A filter changes which rays are traced, so part of the difference is the scene seen
through other rays, not the filter arithmetic.

Prints one JSON line.  Usage: python tools/bench_pixel_filter.py [--rounds 5] [--spp 1024] [--res 1024] [--warmup 1]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--kind", default="gaussian", choices=["box", "tent", "gaussian", "blackman-harris"])
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--sigma", type=float, default=0.5)
    args = ap.parse_args()
    pkg = graft.load_package()
    scene = pkg.host_scene.cornell_box(args.res, args.res)
    filters = {"off": ("box", 0.5, 0.0), "on": (args.kind, args.radius, args.sigma)}
    configs = [(f, table) for table in ("table_off", "table_force") for f in ("off", "on")]
    times = {c: [] for c in configs}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(args.max_depth)

        def run(f, table):
            r.set_pixel_filter(*filters[f])
            r.set_sampler_table(0 if table == "table_off" else 2)
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(args.spp)
            r.sync()
            return r.kernel_time(reset=True)[0]

        for k in range(args.warmup + args.rounds):
            order = configs[k % len(configs):] + configs[:k % len(configs)]
            for c in order:
                ms = run(*c)
                if k >= args.warmup:
                    times[c].append(ms)
        r.set_pixel_filter("box", 0.5)
        r.set_sampler_table(1)
    out = {"workload": f"cornell_{args.res}x{args.res}_{args.spp}spp_{args.max_depth}bounces", "rounds": args.rounds,
           "filter": {"kind": args.kind, "radius": args.radius, "sigma": args.sigma}, "kernel_ms": {}, "spread": {}, "cost": {}}
    med = {}
    for c in configs:
        name = f"filter_{c[0]}/{c[1]}"
        med[c] = statistics.median(times[c])
        out["kernel_ms"][name] = round(med[c], 3)
        out["spread"][name] = round((max(times[c]) - min(times[c])) / med[c], 4)
    for table in ("table_off", "table_force"):
        out["cost"][f"filter_on/{table}"] = round(med[("on", table)] / med[("off", table)] - 1.0, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
