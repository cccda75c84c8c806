#!/usr/bin/env python3
"""What a thin lens costs: the flagship Cornell configuration of bench.py (1024 x 1024, 1024 spp, bounce cap
8, brute force) rendered with the lens off and on, with the sampler table off and forced, on one build in one process.

The four configurations alternate round by round (the order rotates), so clock drift and neighbours on the machine hit all
of them alike; the figure per configuration is the median of its rounds' kernel times (HIP events), and the spread is
(max - min) / median over the rounds.  A lens changes which rays are traced, so part of the difference is the scene seen
through other rays, not the lens arithmetic; the probe line isolates the arithmetic by timing a lens whose radius is too
small to move any ray visibly (1e-6 scene units).

Prints one JSON line.  Usage: python tools/bench_lens.py [--rounds 5] [--spp 1024] [--res 1024] [--warmup 1]"""
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
    ap.add_argument("--lens-radius", type=float, default=0.05)
    ap.add_argument("--focus-distance", type=float, default=4.0, help="the Cornell box's back wall")
    args = ap.parse_args()
    pkg = graft.load_package()
    scene = pkg.host_scene.cornell_box(args.res, args.res)
    lenses = {"off": 0.0, "on": args.lens_radius, "tiny": 1e-6}
    configs = [(lens, table) for table in ("table_off", "table_force") for lens in ("off", "on", "tiny")]
    times = {c: [] for c in configs}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(args.max_depth)

        def run(lens, table):
            r.set_lens(lenses[lens], args.focus_distance)
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
        r.set_lens(0.0, 1.0)
        r.set_sampler_table(1)
    out = {"workload": f"cornell_{args.res}x{args.res}_{args.spp}spp_{args.max_depth}bounces", "rounds": args.rounds,
           "lens_radius": args.lens_radius, "focus_distance": args.focus_distance, "kernel_ms": {}, "spread": {}, "cost": {}}
    med = {}
    for c in configs:
        name = f"lens_{c[0]}/{c[1]}"
        med[c] = statistics.median(times[c])
        out["kernel_ms"][name] = round(med[c], 3)
        out["spread"][name] = round((max(times[c]) - min(times[c])) / med[c], 4)
    for table in ("table_off", "table_force"):
        out["cost"][f"lens_on/{table}"] = round(med[("on", table)] / med[("off", table)] - 1.0, 4)
        out["cost"][f"lens_tiny/{table}"] = round(med[("tiny", table)] / med[("off", table)] - 1.0, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
