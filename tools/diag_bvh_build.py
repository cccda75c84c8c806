#!/usr/bin/env python3
"""Diagnostic (GPU box): the two builders of the DMT_ACCEL_BVH tree side by side.

    diag_bvh_build.py                 every step below, each in a child process of its own under its own time limit,
                                      stopping at the first that fails; output also in profiles/bvh_build/
    diag_bvh_build.py steps NAME...   only the named steps of that list (build_1M build_16M render_c4 render_cornell trace_1M)
    diag_bvh_build.py build N         build time host vs device, end to end (dmt_accel_build_info), median of five after
                                      one warm-up, builders alternated; SAH cost of both trees; temporary device memory
    diag_bvh_build.py render c4|cornell   kernel-timed render rate at 1024^2 x 64 spp under each tree, builders alternated
    diag_bvh_build.py trace N         six device builds and nothing else: the program for
                                      rocprofv3 --kernel-trace --stats -- python tools/diag_bvh_build.py trace N
"""
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "profiles" / "bvh_build"
HOST, DEVICE = 0, 1
NAMES = {0: "host", 1: "device", 2: "host after an abandoned device build"}


def package():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    return g.load_package()


def soup_scene(pkg, n):
    return pkg.host_scene.random_triangle_scene(n, width=1024, height=1024)


def build(n):
    pkg = package()
    scene = soup_scene(pkg, n)
    times, cost, recs = {HOST: [], DEVICE: []}, {}, {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_accel(1)                                  # host build: the warm-up of that side
        for rep in range(6):                            # rep 0 = warm-up of the device side (allocates its temporaries)
            for mode in (DEVICE, HOST):
                r.set_accel_build(mode)                 # a change of mode rebuilds at once
                rec = r.accel_build_info()
                assert rec["builder"] == mode, rec
                if rep:
                    times[mode].append(rec["build_ms"])
                recs[mode] = rec
                if rep == 5:
                    nodes, pairs = r.download_accel()
                    c = pkg.bvh_check(nodes, pairs, scene.xs, scene.ys, scene.zs)
                    assert c["ok"], c
                    cost[mode] = c["sah_cost"]
    for mode in (HOST, DEVICE):
        rec = recs[mode]
        print(f"{n} triangles, {NAMES[mode]:6s} builder: median {statistics.median(times[mode]):10.3f} ms  (min {min(times[mode]):.3f}, max "
              f"{max(times[mode]):.3f}; five builds after one warm-up)  nodes {rec['nodes']}  pairs {rec['pairs']}  depth {rec['depth']}  "
              f"SAH cost {cost[mode]:.2f}  temporaries {rec['temp_bytes'] / 1e6:.1f} MB")
    print(f"{n} triangles: build time host / device = {statistics.median(times[HOST]) / statistics.median(times[DEVICE]):.1f}, "
          f"SAH cost device / host = {cost[DEVICE] / cost[HOST]:.3f}")


def render(which):
    pkg = package()
    res, spp = 1024, 64
    scene = soup_scene(pkg, 1_000_000) if which == "c4" else pkg.host_scene.cornell_box(res, res)
    rate = {HOST: [], DEVICE: []}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(8)
        r.set_accel(1)
        for rep in range(4):                            # rep 0 = warm-up
            for mode in (HOST, DEVICE):
                r.set_accel_build(mode)
                assert r.accel_build_info()["builder"] == mode
                r.film_clear()
                r.kernel_time(reset=True)
                r.render(spp)
                r.render(spp, sample_offset=spp)
                ms, launches = r.kernel_time(reset=True)
                if rep:
                    rate[mode].append(res * res * spp / (ms / launches) / 1e3)
        if which == "cornell":
            nodes, pairs = r.download_accel()
            dev_cost = pkg.bvh_check(nodes, pairs, scene.xs, scene.ys, scene.zs)["sah_cost"]
            r.set_accel_build(HOST)
            nodes, pairs = r.download_accel()
            print(f"cornell: SAH cost host {pkg.bvh_check(nodes, pairs, scene.xs, scene.ys, scene.zs)['sah_cost']:.3f}, device {dev_cost:.3f}")
    h, d = statistics.median(rate[HOST]), statistics.median(rate[DEVICE])
    print(f"{which} {res}x{res}x{spp} spp, kernel-timed, three alternated rounds of two launches: host tree {h:.1f} Msamples/s "
          f"({min(rate[HOST]):.1f} .. {max(rate[HOST]):.1f}), device tree {d:.1f} Msamples/s ({min(rate[DEVICE]):.1f} .. {max(rate[DEVICE]):.1f}), "
          f"device / host = {d / h:.3f}")


def trace(n):
    pkg = package()
    scene = soup_scene(pkg, n)
    with pkg.Renderer(0) as r:
        r.set_accel_build(DEVICE)
        r.upload_scene(scene)
        r.set_accel(1)
        for _ in range(5):
            r.upload_triangles(scene.xs, scene.ys, scene.zs, scene.mat_id)
        print(r.accel_build_info())


def everything(only):
    OUT.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    tracedir = OUT / "trace_1M"                         # a run of its own: kernel trace and statistics, no counters with it
    steps = [("build_1M", me + ["build", "1000000"], 240), ("build_16M", me + ["build", "16000000"], 900),
             ("render_c4", me + ["render", "c4"], 300), ("render_cornell", me + ["render", "cornell"], 300),
             ("trace_1M", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tracedir), "-o", "trace", "--"] + me +
              ["trace", "1000000"], 300)]
    for name, cmd, limit in steps:                      # each step under its own limit; nothing more after a failure
        if only and name not in only:
            continue
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        text = p.stdout
        if name == "trace_1M" and p.returncode == 0:    # six builds: the per-kernel totals of the trace, largest first
            for f in sorted(tracedir.rglob("*kernel_stats.csv")):
                text += "".join(f.read_text().splitlines(keepends=True)[:24])
        (OUT / (name + ".txt")).write_text(text)
        print(text, end="", flush=True)
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}")
            return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 1 or sys.argv[1] == "steps":    # steps NAME...: only those of the steps above
        sys.exit(everything(sys.argv[2:]))
    {"build": lambda: build(int(sys.argv[2])), "render": lambda: render(sys.argv[2]), "trace": lambda: trace(int(sys.argv[2]))}[sys.argv[1]]()
