#!/usr/bin/env python3
"""What smooth shading costs: kernel time of the *_vn rows with the files' normals against their parent
rows, on one build in one process, flat and smooth launches alternating round by round (the order rotates).

Workloads: the reference's sphere.fbx under its veranda map (BASELINE config 3: c3_sphere_veranda.json, 256 x 256 x 2048 spp,
depth 12; env row) and its scene_test.json (teapot.fbx in chipped paint, 256 x 256 x 32 spp, depth 12; env + texture row),
each under both accel modes, at the files' own size.  Prints one JSON line per workload.
An experimental build of the library is measured through DMT_HIP_LIB (binding.library_path).
Usage: python tools/diag_vertex_normals.py [--rounds 3] [--warmup 1] [--small] [--only WORKLOAD]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402


def measure(pkg, name, scene, accel, spp, depth, rounds, warmup):
    configs = ["flat", "file_normals"]
    times = {c: [] for c in configs}
    info = {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        r.set_accel(accel)

        def run(c):
            if c == "flat":
                r.clear_vertex_normals()
            else:
                r.upload_vertex_normals(scene.tri_normals)
            r.film_clear()
            r.sync()
            r.kernel_time(reset=True)
            r.render(spp)
            r.sync()
            ms = r.kernel_time(reset=True)[0]
            info[c] = {"kernel": r.kernel_info(), "normals": r.vertex_normals_info()}
            return ms

        for k in range(warmup + rounds):
            order = configs[k % 2:] + configs[:k % 2]
            for c in order:
                ms = run(c)
                if k >= warmup:
                    times[c].append(ms)
    med = {c: statistics.median(times[c]) for c in configs}
    print(json.dumps({"workload": name, "accel": "bvh" if accel else "brute", "width": scene.width, "height": scene.height, "spp": spp,
                      "max_depth": depth, "triangles": scene.tri_count, "rounds": rounds,
                      "kernel_ms": {c: round(med[c], 3) for c in configs},
                      "all_ms": {c: [round(t, 3) for t in times[c]] for c in configs},
                      "spread": {c: round((max(times[c]) - min(times[c])) / med[c], 4) for c in configs},
                      "cost_vs_flat": round(med["file_normals"] / med["flat"] - 1.0, 4), "info": info}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a quick pass: 64 x 64 and at most 16 spp")
    ap.add_argument("--only", default=None, help="one workload: c3_sphere_veranda or scene_test")
    args = ap.parse_args()
    pkg = graft.load_package()
    golden = ROOT / "tests" / "golden"
    for name, path in (("c3_sphere_veranda", golden / "c3" / "c3_sphere_veranda.json"), ("scene_test", golden / "scene_test" / "scene_test.json")):
        if args.only and args.only != name:
            continue
        scene = pkg.host_scene.load_json(path)
        spp = scene.spp
        if args.small:
            scene.set_resolution(64, 64)
            spp = min(spp, 16)
        for accel in (0, 1):
            measure(pkg, name, scene, accel, spp, scene.max_depth, args.rounds, args.warmup)


if __name__ == "__main__":
    main()
