"""Temporal accumulation: the sweep behind dmt_temporal_defaults and the cost of k_temporal.

    python tools/diag_temporal.py sweep > profiles/temporal/sweep.txt
    python tools/diag_temporal.py pan   > profiles/temporal/sweep_pan.txt
    python tools/diag_temporal.py cost  > profiles/temporal/cost.txt
    python tools/diag_temporal.py updates > profiles/temporal/updates.txt

sweep: Cornell box and c3_sphere_veranda at 256 x 256, 8 frames of 4 spp (sample offsets 0, 4, ..), reference 4096 spp from
sample offset 64.  Frames and feature planes are rendered once per scene and aov_spp, then every (alpha, normal_threshold,
plane_threshold) accumulates the same films.  Per row: RMSE of dmt_denoise of frame 8 alone / RMSE of the temporal output
at frame 8, and the temporal output's brightness error.
pan: the Cornell box with the camera moving 0.04 sideways per frame and one box moving 0.05 per frame the other way (so
that pixels are disoccluded every frame); reference = 4096 spp of the last frame's scene.  Every parameter is swept.
updates: what keeping the raw vertices costs a vertex update once a temporal call was made: 1 M random triangles, device
builder, refit; wall clock and update_ms of update_vertices / update_vertices_device before any temporal call, and
afterwards with a temporal call between the updates (every update then snapshots the history frame's vertices).
cost: HIP-event time of k_temporal and of one k_atrous pass at 1024^2 and 4096^2 (warm-up, median of 5)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean(axis=-1)).mean())


def scene(pkg, name):
    hs = pkg.host_scene
    if name == "cornell":
        return hs.cornell_box(256, 256), 8, False
    return hs.load_json(GOLDEN / "c3" / "c3_sphere_veranda.json"), 12, True


def sweep(pkg):
    alphas, nts, pts = (0.0, 0.05, 0.1, 0.2, 0.4), (0.5, 0.9, 0.99), (0.5, 2.0, 8.0)
    for name in ("cornell", "c3_sphere_veranda"):
        sc, depth, bvh = scene(pkg, name)
        with pkg.Renderer(0) as r:
            r.upload_scene(sc)
            r.set_limits(depth)
            if bvh:
                r.set_accel(1)
            r.film_clear()
            r.render(4096, sample_offset=64)
            ref, _ = r.download_film()
            films = []
            for j in range(8):
                r.film_clear()
                r.render(4, sample_offset=4 * j)
                films.append(r.download_film())
            for aov_spp in (1, 4):
                r.render_aovs(aov_spp)
                alone = r.denoise(film=films[-1])
                e0 = rmse(alone, ref)
                print(f"{name} aov_spp {aov_spp}: dmt_denoise of frame 8 alone RMSE {e0:.5f} brightness "
                      f"{100 * (alone[..., :3].mean() / ref[..., :3].mean() - 1):+.3f} %")
                print("  alpha  n_thr  p_thr   RMSE     ratio  brightness  reprojected")
                for a in alphas:
                    for nt in nts:
                        for pt in pts:
                            if (nt != 0.9 and pt != 2.0):
                                continue  # one axis at a time around the starting point
                            r.temporal_reset()
                            for j in range(8):
                                out = r.denoise_temporal(temporal=dict(alpha=a, normal_threshold=nt, plane_threshold=pt), film=films[j])
                            e1 = rmse(out, ref)
                            info = r.temporal_info()
                            print(f"  {a:5.2f}  {nt:5.2f}  {pt:5.1f}  {e1:.5f}  {e0 / e1:6.3f}  {100 * (out[..., :3].mean() / ref[..., :3].mean() - 1):+8.3f} %"
                                  f"  {info['reprojected']:7d}", flush=True)


def pan(pkg):
    sc, depth, _ = scene(pkg, "cornell")
    xs0 = np.asarray(sc.xs, np.float32)
    box = np.asarray(sc.mat_id) == 0

    def pose(r, j):
        xs = xs0.copy()
        xs[box] -= np.float32(0.05 * j)
        r.update_vertices(xs, sc.ys, sc.zs)
        cam = np.ascontiguousarray(sc.camera, np.uint8).copy()
        cam.view(np.float32)[3] += np.float32(0.04 * j)
        r.set_camera(cam)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(depth)
        pose(r, 7)
        r.film_clear()
        r.render(4096, sample_offset=64)
        ref, _ = r.download_film()
        for aov_spp in (1, 4):
            def run(t):
                r.temporal_reset()
                for j in range(8):
                    pose(r, j)
                    r.film_clear()
                    r.render(4, sample_offset=4 * j)
                    r.render_aovs(aov_spp)
                    out = r.denoise_temporal(temporal=t)
                return out, r.denoise(), r.temporal_info()
            _, alone, _ = run(None)
            e0 = rmse(alone, ref)
            print(f"cornell pan aov_spp {aov_spp}: dmt_denoise of frame 8 alone RMSE {e0:.5f} brightness "
                  f"{100 * (alone[..., :3].mean() / ref[..., :3].mean() - 1):+.3f} %")
            print("  alpha  n_thr  p_thr   RMSE     ratio  brightness  reprojected   reset")
            for a in (0.0, 0.1, 0.2, 0.4):
                for nt in (0.5, 0.9, 0.99):
                    for pt in (0.5, 1.0, 2.0, 4.0, 8.0):
                        if nt != 0.9 and pt != 2.0:
                            continue
                        out, _, info = run(dict(alpha=a, normal_threshold=nt, plane_threshold=pt))
                        e1 = rmse(out, ref)
                        print(f"  {a:5.2f}  {nt:5.2f}  {pt:5.1f}  {e1:.5f}  {e0 / e1:6.3f}  {100 * (out[..., :3].mean() / ref[..., :3].mean() - 1):+8.3f} %"
                              f"  {info['reprojected']:7d}  {info['reset']:6d}", flush=True)


def cost(pkg):
    for res in (1024, 4096):
        sc = pkg.host_scene.cornell_box(res, res)
        with pkg.Renderer(0) as r:
            r.upload_scene(sc)
            r.set_limits(3)
            r.render(2)
            r.render_aovs(1)
            tt, t1, t0 = [], [], []
            for i in range(6):  # the first is the warm-up
                r.denoise_temporal({"iterations": 1})
                tt.append(r.temporal_info()["temporal_ms"])
                r.denoise({"iterations": 1})
                t1.append(r.denoise_ms)
                r.denoise({"iterations": 0})
                t0.append(r.denoise_ms)
            info = r.temporal_info()
            kt, ka = float(np.median(tt[1:])), float(np.median(t1[1:]) - np.median(t0[1:]))
            print(f"{res} x {res}: k_temporal {kt:.4f} ms, one k_atrous pass {ka:.4f} ms (init + pass {np.median(t1[1:]):.4f}, init "
                  f"{np.median(t0[1:]):.4f}), ratio {kt / ka:.2f}; reprojected {info['reprojected']}, history {info['history_bytes']} bytes",
                  flush=True)


def updates(pkg, n=1 << 20):
    import time
    import torch
    sc = pkg.host_scene.random_triangle_scene(n, width=256, height=256)
    base = [np.asarray(a, np.float32).reshape(-1, 4) for a in (sc.xs, sc.ys, sc.zs)]
    host = [tuple(a + np.float32(0.01 * k) for a in base) for k in (0, 1)]
    dev = [torch.from_numpy(np.ascontiguousarray(np.stack([a[:, :3] for a in f], -1).reshape(-1, 9))).to("cuda:0") for f in host]
    torch.cuda.synchronize()
    with pkg.Renderer(0) as r:
        r.set_accel_build(pkg.BVH_BUILD_DEVICE)
        r.upload_scene(sc)
        r.set_accel(1)
        r.set_accel_update(pkg.BVH_UPDATE_REFIT)
        r.set_limits(2)
        for phase in ("no temporal call yet", "a temporal call between updates"):
            for how in ("update_vertices", "update_vertices_device"):
                wall, rec = [], []
                for rep in range(6):
                    if phase.startswith("a "):
                        r.film_clear()
                        r.render(2)
                        r.render_aovs(1)
                        r.denoise_temporal({"iterations": 0})
                    r.sync()
                    t0 = time.perf_counter()
                    if how == "update_vertices":
                        r.update_vertices(*host[rep & 1])
                    else:
                        r.update_vertices_device(dev[rep & 1].data_ptr(), n)
                    r.sync()
                    if rep:
                        wall.append((time.perf_counter() - t0) * 1e3), rec.append(r.accel_update_info()["update_ms"])
                print(f"{n} triangles, {phase:32s} {how:24s}: wall clock median {np.median(wall):8.3f} ms, update_ms median {np.median(rec):8.3f} ms",
                      flush=True)
        print(f"history bytes {r.temporal_info()['history_bytes']}")


if __name__ == "__main__":
    pkg = graft.load_package()
    {"sweep": sweep, "pan": pan, "cost": cost, "updates": updates}[sys.argv[1]](pkg)
