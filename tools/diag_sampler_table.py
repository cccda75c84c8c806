#!/usr/bin/env python3
"""Diagnostic (GPU box): the sampler table's two constants.  Kernel time of a flagship call (Cornell 1024 x 1024 x 1024 spp)
under table budgets of 128 MiB .. 1 GiB and with the table off, then Cornell frames of 1 .. 16 Halton periods with the
table off and forced: where the table starts to pay ("Sampler table"; profiles/sampler_table/)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g
pkg = g.load_package()
MIB = 1 << 20


def timed(r, spp, reps):
    out = []
    for _ in range(reps + 1):
        r.film_clear()
        r.sync()
        r.kernel_time(reset=True)
        r.render(spp)
        ms, n = r.kernel_time(reset=True)
        assert n == 1
        out.append(ms)
    return out[1:]


with pkg.Renderer(0) as r:
    r.upload_scene(pkg.host_scene.cornell_box(1024, 1024))
    r.set_limits(8)
    for rnd in range(2):
        for budget in (128, 256, 512, 1024):
            r.set_sampler_table(1, budget * MIB)
            t = timed(r, 1024, 3)
            print(f"flagship 1024x1024x1024spp budget {budget:5d} MiB: " + " ".join(f"{x:.2f}" for x in t) + " ms", flush=True)
    r.set_sampler_table(0)
    t = timed(r, 1024, 3)
    print("flagship table off: " + " ".join(f"{x:.2f}" for x in t) + " ms", flush=True)
    for res, spp in ((128, 2048), (160, 2048), (192, 2048), (256, 2048), (384, 512), (512, 64), (512, 512)):
        r.upload_scene(pkg.host_scene.cornell_box(res, res))
        r.set_limits(8)
        row = []
        for rnd in range(2):
            for mode in (0, 2):
                r.set_sampler_table(mode)
                row.append((mode, min(timed(r, spp, 3))))
        print(f"cornell {res}x{res}x{spp}spp ratio {res * res / 16384:.2f}: " + " ".join(f"{'off' if m == 0 else 'force'} {x:.3f}" for m, x in row) + " ms",
              flush=True)
