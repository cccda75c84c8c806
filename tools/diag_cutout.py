#!/usr/bin/env python3
"""What alpha cutouts cost: kernel time (dmt_kernel_time) of the *_tex_cut rows against their parent *_tex
rows on one build in one process, the configurations alternating round by round (the order rotates); medians of the measured
rounds after the warm-up rounds.

Workload: the Cornell box with the three cards of the cutout tests (tests/cutout_ref.py), under both accel modes, with and
without the sky.  Configurations:
  tex         no opacity upload: the parent row
  cut_opaque  every card's opacity texture is A = 255: the new row runs, every candidate passes (the price of carrying it)
  cut_half    a two-texel checker of A = 20 / 235 under cutoff 0.5: about half of the candidate hits on the cards are cut
Prints one JSON line per (accel, env).
Usage: python tools/diag_cutout.py [--size 512] [--spp 64] [--rounds 5] [--warmup 1]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
import cutout_ref as CR  # noqa: E402

F = np.float32


def scene(O, pkg, size, tex, env):
    base = O.cornell_box(size, size)
    alphas = [CR.checker(16, 20, 235, 2), np.full((8, 8), 255, np.uint8)]
    meshes = [(T, uv * F(1.6) - F(0.3), tex) for T, uv in CR.cornell_cards()]
    return CR.CutScene(base, meshes, alphas, env=pkg.host_scene.synthetic_sky(16) if env else None)


def measure(pkg, O, size, spp, depth, accel, env, rounds, warmup):
    scenes = {"tex": scene(O, pkg, size, 1, env), "cut_opaque": scene(O, pkg, size, 1, env), "cut_half": scene(O, pkg, size, 0, env)}
    configs = list(scenes)
    times = {c: [] for c in configs}
    info = {}
    with pkg.Renderer(0) as r:
        def run(c):
            r.upload_scene(scenes[c], opacity=c != "tex")
            r.set_limits(depth)
            r.set_accel(accel)
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(spp)
            r.sync()
            ms = r.kernel_time(reset=True)[0]
            info[c] = {"kernel": r.kernel_info(), "opacity": r.opacity_info()}
            return ms

        for k in range(warmup + rounds):
            order = configs[k % 3:] + configs[:k % 3]
            for c in order:
                ms = run(c)
                if k >= warmup:
                    times[c].append(ms)
    med = {c: statistics.median(times[c]) for c in configs}
    print(json.dumps({"workload": "cornell_cards", "accel": "bvh" if accel else "brute", "env": bool(env), "width": size, "height": size,
                      "spp": spp, "max_depth": depth, "triangles": scenes["tex"].tri_count, "rounds": rounds,
                      "kernel_ms": {c: round(med[c], 3) for c in configs},
                      "all_ms": {c: [round(t, 3) for t in times[c]] for c in configs},
                      "spread": {c: round((max(times[c]) - min(times[c])) / med[c], 4) for c in configs},
                      "cost_opaque_vs_tex": round(med["cut_opaque"] / med["tex"] - 1.0, 4),
                      "cost_half_vs_tex": round(med["cut_half"] / med["tex"] - 1.0, 4), "info": info}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    pkg = graft.load_package()
    O = graft.load_oracle()
    O.build()
    for accel in (0, 1):
        for env in (False, True):
            measure(pkg, O, args.size, args.spp, args.depth, accel, env, args.rounds, args.warmup)


if __name__ == "__main__":
    main()
