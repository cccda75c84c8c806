#!/usr/bin/env python3
"""Diagnostic (GPU box): in-place vertex updates and the device-side BVH refit.

    diag_bvh_refit.py                 every step below, each in a child process of its own under its own time limit,
                                      stopping at the first that fails; output also in profiles/bvh_refit/
    diag_bvh_refit.py steps NAME...   only the named steps of that list (refit_1M refit_16M paths_1M render_c4 trace_1M)
    diag_bvh_refit.py refit N         update_ms of a refit (records made on the device) of the host builder's and of the
                                      device builder's tree against a rebuild by either builder (build_ms), all in one
                                      process, alternated, median of five after one warm-up
    diag_bvh_refit.py paths N         end to end (wall clock around the call): update_vertices, update_vertices_device and
                                      upload_triangles, refit and rebuild
    diag_bvh_refit.py render          config 4 (1 M triangles, 1024^2 x 64 spp, cap 8), kernel-timed: the tree refitted to a
                                      displacement of amplitude A against the tree built fresh on the same positions
    diag_bvh_refit.py trace N         six refits from device memory and nothing else: the program for
                                      rocprofv3 --kernel-trace --stats -- python tools/diag_bvh_refit.py trace N
"""
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "profiles" / "bvh_refit"
HOST, DEVICE = 0, 1
REBUILD, REFIT = 0, 1
NAMES = {HOST: "host SAH", DEVICE: "device LBVH"}


def package():
    import torch
    torch.cuda.init()                                   # torch opens the GPU before the HIP library does (as bench.py does it)
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    return g.load_package()


def deform(soup, amplitude, phase=0.0):
    """p + A sin(1.3 p' + phase), axes rotated: the smooth field of tests/test_bvh_refit.py"""
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4) for a in soup)
    out = [np.zeros_like(xs) for _ in range(3)]
    src = (ys, zs, xs)
    base = (xs, ys, zs)
    for a in range(3):
        out[a][:, :3] = (base[a][:, :3].astype(np.float64) + amplitude * np.sin(1.3 * src[a][:, :3].astype(np.float64) + (0.3, 1.1, 2.0)[a] + phase)).astype(np.float32)
    return tuple(out)


def verts9(soup):
    return np.ascontiguousarray(np.stack([a[:, :3] for a in soup], -1).reshape(-1, 9), np.float32)


def med(v):
    return f"median {statistics.median(v):10.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def refit(n):
    pkg = package()
    import torch
    scene = pkg.host_scene.random_triangle_scene(n, width=1024, height=1024)
    soup = (scene.xs, scene.ys, scene.zs)
    frames = [torch.from_numpy(verts9(deform(soup, 0.1, phase=p))).to("cuda:0") for p in (0.0, 1.7)]
    torch.cuda.synchronize()
    refit_ms, build_ms, ratio, temp = {HOST: [], DEVICE: []}, {HOST: [], DEVICE: []}, {}, {}
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_accel(1)
        r.set_accel_update(REFIT)
        for rep in range(6):                            # rep 0 = warm-up (allocates the temporaries of both sides)
            for mode in (DEVICE, HOST):
                r.set_accel_build(mode)                 # a change of mode rebuilds at once, from the context's current positions
                rec = r.accel_build_info()
                assert rec["builder"] == mode, rec
                r.update_vertices_device(frames[rep & 1].data_ptr(), n)
                u = r.accel_update_info()
                assert u["action"] == pkg.BVH_UPDATED_REFIT, u
                if rep:
                    build_ms[mode].append(rec["build_ms"]), refit_ms[mode].append(u["update_ms"])
                ratio[mode], temp[mode] = u["sah_cost"] / u["sah_cost_at_build"], u["temp_bytes"]
    for mode in (HOST, DEVICE):
        print(f"{n} triangles, {NAMES[mode]:11s} tree: rebuild (build_ms) {med(build_ms[mode])}   refit from device memory (update_ms) "
              f"{med(refit_ms[mode])}   cost after / at build {ratio[mode]:.4f}   refit scratch {temp[mode] / 1e6:.1f} MB")
    print(f"{n} triangles: device rebuild / refit of the device tree = {statistics.median(build_ms[DEVICE]) / statistics.median(refit_ms[DEVICE]):.2f}, "
          f"host rebuild / refit of the host tree = {statistics.median(build_ms[HOST]) / statistics.median(refit_ms[HOST]):.1f}  "
          "(update_ms holds the record kernel, the copy of the records to the host mirrors, the cull plan on the host, the refit and its cost)")


def paths(n):
    pkg = package()
    import torch
    scene = pkg.host_scene.random_triangle_scene(n, width=1024, height=1024)
    soup = (scene.xs, scene.ys, scene.zs)
    host_frames = [deform(soup, 0.1, phase=p) for p in (0.0, 1.7)]
    dev_frames = [torch.from_numpy(verts9(f)).to("cuda:0") for f in host_frames]
    torch.cuda.synchronize()
    wall = {}
    with pkg.Renderer(0) as r:
        r.set_accel_build(DEVICE)
        r.upload_scene(scene)
        r.set_accel(1)
        variants = [("update_vertices, refit", REFIT, "host"), ("update_vertices_device, refit", REFIT, "device"),
                    ("update_vertices, rebuild (device builder)", REBUILD, "host"), ("update_vertices_device, rebuild (device builder)", REBUILD, "device"),
                    ("upload_triangles (device builder)", None, "upload")]
        for rep in range(6):
            for name, mode, how in variants:
                if mode is not None:
                    r.set_accel_update(mode)
                f = rep & 1
                t0 = time.perf_counter()
                if how == "host":
                    r.update_vertices(*host_frames[f])
                elif how == "device":
                    r.update_vertices_device(dev_frames[f].data_ptr(), n)
                else:
                    r.upload_triangles(*host_frames[f], scene.mat_id)
                ms = (time.perf_counter() - t0) * 1e3
                if rep:
                    wall.setdefault(name, []).append((ms, r.accel_update_info()["update_ms"] if how != "upload" else r.accel_build_info()["build_ms"]))
    for name, v in wall.items():
        print(f"{n} triangles, {name:50s}: wall clock {med([a for a, _ in v])}   its record ({'build_ms' if 'upload' in name else 'update_ms'}) "
              f"median {statistics.median([b for _, b in v]):.3f} ms")


def render():
    pkg = package()
    res, spp, n = 1024, 64, 1_000_000
    scene = pkg.host_scene.random_triangle_scene(n, width=res, height=res)
    soup = (scene.xs, scene.ys, scene.zs)

    def rate(r):
        out = []
        for rep in range(4):                            # rep 0 = warm-up
            r.film_clear()
            r.kernel_time(reset=True)
            r.render(spp)
            r.render(spp, sample_offset=spp)
            ms, launches = r.kernel_time(reset=True)
            if rep:
                out.append(res * res * spp / (ms / launches) / 1e3)
        return out

    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(8)
        r.set_accel(1)
        r.set_accel_update(REFIT)
        for mode in (HOST, DEVICE):
            for amplitude in (0.01, 0.1, 1.0, 5.0):
                moved = deform(soup, amplitude)
                r.set_accel_build(mode)
                r.upload_triangles(*soup, scene.mat_id)             # the topology of the undeformed soup
                r.update_vertices(*moved)
                u = r.accel_update_info()
                assert u["action"] == pkg.BVH_UPDATED_REFIT and r.accel_build_info()["builder"] == mode
                refitted = rate(r)
                r.upload_triangles(*moved, scene.mat_id)            # built fresh on the same positions
                fresh = rate(r)
                a, b = statistics.median(refitted), statistics.median(fresh)
                print(f"c4 {res}x{res}x{spp} spp, {NAMES[mode]:11s} tree, A = {amplitude:<5}: cost after / at build {u['sah_cost'] / u['sah_cost_at_build']:8.4f}   "
                      f"refitted {a:7.1f} Msamples/s ({min(refitted):.1f} .. {max(refitted):.1f})   fresh {b:7.1f} ({min(fresh):.1f} .. {max(fresh):.1f})   "
                      f"refitted / fresh = {a / b:.3f}", flush=True)


def trace(n):
    pkg = package()
    import torch
    scene = pkg.host_scene.random_triangle_scene(n, width=1024, height=1024)
    soup = (scene.xs, scene.ys, scene.zs)
    frames = [torch.from_numpy(verts9(deform(soup, 0.1, phase=p))).to("cuda:0") for p in (0.0, 1.7)]
    torch.cuda.synchronize()
    with pkg.Renderer(0) as r:
        r.set_accel_build(DEVICE)
        r.upload_scene(scene)
        r.set_accel(1)
        r.set_accel_update(REFIT)
        for k in range(6):
            r.update_vertices_device(frames[k & 1].data_ptr(), n)
        print(r.accel_build_info(), r.accel_update_info())


def everything(only):
    OUT.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    tracedir = OUT / "trace_1M"                         # a run of its own: kernel trace and statistics, no counters with it
    steps = [("refit_1M", me + ["refit", "1000000"], 240), ("refit_16M", me + ["refit", "16000000"], 900),
             ("paths_1M", me + ["paths", "1000000"], 300), ("render_c4", me + ["render"], 400),
             ("trace_1M", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tracedir), "-o", "trace", "--"] + me +
              ["trace", "1000000"], 300)]
    for name, cmd, limit in steps:                      # each step under its own limit; nothing more after a failure
        if only and name not in only:
            continue
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
        text = p.stdout
        if name == "trace_1M" and p.returncode == 0:    # one device build and six refits: the per-kernel totals, largest first
            for f in sorted(tracedir.rglob("*kernel_stats.csv")):
                text += "".join(f.read_text().splitlines(keepends=True)[:28])
        (OUT / (name + ".txt")).write_text(text)
        print(text, end="", flush=True)
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}")
            return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 1 or sys.argv[1] == "steps":    # steps NAME...: only those of the steps above
        sys.exit(everything(sys.argv[2:]))
    {"refit": lambda: refit(int(sys.argv[2])), "paths": lambda: paths(int(sys.argv[2])), "render": render,
     "trace": lambda: trace(int(sys.argv[2]))}[sys.argv[1]]()
