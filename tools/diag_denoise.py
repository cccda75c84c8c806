#!/usr/bin/env python3
"""Diagnostic (GPU box): the denoiser (dmt_render_aovs + dmt_denoise).

Quality: per scene, a reference film of 4096 spp from samples [64, 64 + 4096) (independent of the films measured), films of
4 / 16 / 64 spp from sample 0, each denoised with the defaults (AOVs of 4 spp); RMSE of noisy and denoised film against the
reference, their ratio, and the mean brightness of the denoised film relative to the reference's.
Cost: AOV pass and per-pass filter time (HIP events via dmt_denoise's kernel_ms, warm-up first, median of 5) at 1024^2 and
4096^2 on the Cornell box, for K = 0 (validation pass only), 1 and 5.  One JSON line at the end.
--sigma-luminance S / --iterations K denoise with those values instead of the library's defaults (the other parameters
keep theirs).  --sweep prints the grid that chose the defaults instead: Cornell box and c3_sphere_veranda at 4 / 16 / 64
spp, RMSE ratio and brightness for sigma_luminance in 4 .. 64 and K in 4, 5 (profiles/denoise/sweep_sigma_l_K.txt).

  python3 tools/diag_denoise.py [--quick] [--sigma-luminance S] [--iterations K] [--out FILE]
  python3 tools/diag_denoise.py --sweep
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
hs = pkg.host_scene
QUICK = "--quick" in sys.argv


def _arg(name, conv):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else None


PARAMS = {k: v for k, v in (("sigma_luminance", _arg("--sigma-luminance", float)), ("iterations", _arg("--iterations", int)))
          if v is not None}


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d ** 2).mean(axis=-1)).mean())


def quality(name, scene, depth, bvh, ref_spp):
    out = []
    with pkg.Renderer(0) as r:
        r.upload_scene(scene)
        r.set_limits(depth)
        if bvh:
            r.set_accel(1)
        r.film_clear()
        r.render(ref_spp, sample_offset=64)
        ref, _ = r.download_film()
        r.render_aovs(4)
        for spp in (4, 16, 64):
            r.film_clear()
            r.render(spp)
            noisy, _ = r.download_film()
            den = r.denoise(PARAMS)
            e0, e1 = rmse(noisy, ref), rmse(den, ref)
            row = {"scene": name, "spp": spp, "rmse_noisy": e0, "rmse_denoised": e1, "ratio": e0 / e1,
                   "brightness": float(den[..., :3].mean() / ref[..., :3].mean())}
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def cost(res, reps=5):
    out = []
    sc = hs.cornell_box(res, res)
    with pkg.Renderer(0) as r:
        r.upload_scene(sc)
        r.set_limits(8)
        r.film_clear()
        r.render(4)
        r.sync()
        r.render_aovs(4)  # warm-up
        r.sync()
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r.render_aovs(4)
            r.sync()
            walls.append((time.perf_counter() - t0) * 1e3)
        row = {"res": res, "aov_4spp_ms_wall": float(np.median(walls))}
        for k in (0, 1, 5):
            r.denoise({"iterations": k})  # warm-up
            ms = [(r.denoise({"iterations": k}), r.denoise_ms)[1] for _ in range(reps)]
            row[f"denoise_K{k}_ms"] = float(np.median(ms))
        row["per_pass_ms"] = (row["denoise_K5_ms"] - row["denoise_K0_ms"]) / 5
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def sweep():
    """the sigma_luminance x K grid behind the defaults"""
    scenes = (("cornell", hs.cornell_box(256, 256), 8, False),
              ("c3", hs.load_json(ROOT / "tests" / "golden" / "c3" / "c3_sphere_veranda.json"), 12, True))
    for name, sc, depth, bvh in scenes:
        with pkg.Renderer(0) as r:
            r.upload_scene(sc)
            r.set_limits(depth)
            if bvh:
                r.set_accel(1)
            r.film_clear()
            r.render(4096, sample_offset=64)
            ref, _ = r.download_film()
            r.render_aovs(4)
            for spp in (4, 16, 64):
                r.film_clear()
                r.render(spp)
                noisy, _ = r.download_film()
                print(name, spp, "noisy", round(rmse(noisy, ref), 5), "bright",
                      round(float(noisy[..., :3].mean() / ref[..., :3].mean()), 4), flush=True)
                for sl in (4, 8, 16, 32, 64):
                    for k in (4, 5):
                        den = r.denoise({"sigma_luminance": sl, "iterations": k})
                        print(name, spp, "sl", sl, "K", k, "ratio", round(rmse(noisy, ref) / rmse(den, ref), 3),
                              "bright", round(float(den[..., :3].mean() / ref[..., :3].mean()), 4), flush=True)


def main():
    if "--sweep" in sys.argv:
        sweep()
        return
    res = {"quality": [], "cost": [], "params": PARAMS}
    ref_spp = 1024 if QUICK else 4096
    res["quality"] += quality("cornell_256", hs.cornell_box(256, 256), 8, False, ref_spp)
    c3 = hs.load_json(ROOT / "tests" / "golden" / "c3" / "c3_sphere_veranda.json")
    res["quality"] += quality("c3_sphere_veranda", c3, 12, True, ref_spp)
    teapot = hs.load_json(ROOT / "tests" / "golden" / "scene_test" / "scene_test.json").set_resolution(256, 256)
    res["quality"] += quality("scene_test_teapot_256", teapot, 8, True, ref_spp)
    for r in ((1024,) if QUICK else (1024, 4096)):
        res["cost"] += cost(r)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        Path(sys.argv[sys.argv.index("--out") + 1]).write_text(line + "\n")


if __name__ == "__main__":
    main()
