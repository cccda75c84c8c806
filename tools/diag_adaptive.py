#!/usr/bin/env python3
"""Diagnostic (GPU box): adaptive sampling (dmt_render_adaptive) against uniform films on two scenes.

For each scene: a reference film from samples [cap, 2 cap) (independent of every film measured, so its own noise adds to
every RMSE alike); uniform films of cap/16 .. cap spp in one launch each; adaptive films (cap as the cap, cap/16 as the
round and the minimum) at several thresholds.  Reported per film: samples traced, kernel time (HIP events; every round
counts), Msamples/s, RMSE against the reference, and for an adaptive film the RMSE of a uniform film of EQUAL kernel time
(log-log interpolation of the uniform curve).  One JSON line per scene at the end.

  python3 tools/diag_adaptive.py [--quick]
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
hs = pkg.host_scene
QUICK = "--quick" in sys.argv


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean(axis=-1)).mean())


def interp_equal_time(curve, ms):
    """RMSE of a uniform film whose kernel time is `ms`, log-log interpolated (None outside the measured range)"""
    t = np.log([c["kernel_ms"] for c in curve])
    e = np.log([c["rmse"] for c in curve])
    x = np.log(ms)
    if x < t.min() or x > t.max():
        return None
    return float(np.exp(np.interp(x, t, e)))


def measure(name, scene, depth, cap, bvh, thresholds):
    out = {"scene": name, "width": scene.width, "height": scene.height, "max_depth": depth, "cap_spp": cap}
    pixels = scene.width * scene.height
    step = cap // 16
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        if bvh:
            r.set_accel(1)
        r.film_clear(); r.render(step); r.sync()  # warm-up (code object load, first-touch allocations)
        r.film_clear(); r.render(cap, sample_offset=cap)
        ref, _ = r.download_film()
        r.kernel_time(reset=True)
        curve = []
        for spp in (step, 2 * step, 4 * step, 8 * step, cap):
            r.film_clear(); r.sync(); r.kernel_time(reset=True)
            r.render(spp)
            ms, _ = r.kernel_time(reset=True)
            mean, _ = r.download_film()
            curve.append({"spp": spp, "samples": pixels * spp, "kernel_ms": ms, "msamples_s": pixels * spp / ms / 1e3,
                          "rmse": rmse(mean, ref)})
            print(f"{name} uniform  {spp:5d} spp: {ms:9.2f} ms  {pixels * spp / ms / 1e3:8.1f} Msamples/s  RMSE {curve[-1]['rmse']:.4e}",
                  flush=True)
        out["uniform"] = curve
        ad = []
        for thr in thresholds:
            r.film_clear(); r.sync(); r.kernel_time(reset=True)
            rounds, samples = r.render_adaptive(thr, cap, step, min_spp=step)
            ms, launches = r.kernel_time(reset=True)
            mean, m2 = r.download_film()
            e = rmse(mean, ref)
            eq = interp_equal_time(curve, ms)
            ad.append({"threshold": thr, "rounds": rounds, "launches": launches, "samples": samples,
                       "mean_spp": samples / pixels, "kernel_ms": ms, "msamples_s": samples / ms / 1e3, "rmse": e,
                       "uniform_rmse_at_equal_time": eq, "stopped_early": float((m2[..., 3] < cap).mean())})
            print(f"{name} adaptive thr {thr:<6g}: {rounds:2d} rounds {samples / pixels:7.1f} spp avg  {ms:9.2f} ms  "
                  f"{samples / ms / 1e3:8.1f} Msamples/s  RMSE {e:.4e}  uniform at equal time "
                  f"{'n/a' if eq is None else f'{eq:.4e}'}", flush=True)
        out["adaptive"] = ad
    return out


def main():
    results = []
    cap = 256 if QUICK else 1024
    results.append(measure("cornell", hs.cornell_box(1024, 1024), 8, cap, False, (0.01, 0.02, 0.05, 0.1)))
    c3 = hs.load_json(ROOT / "tests" / "golden" / "c3" / "c3_sphere_veranda.json")
    results.append(measure("c3_sphere_veranda", c3, 12, 512 if QUICK else 2048, True, (0.01, 0.02, 0.05, 0.1)))
    for res in results:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
