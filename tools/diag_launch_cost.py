#!/usr/bin/env python3
"""Diagnostic (GPU box): host cost of a launch: wall time of the dmt_render call alone (the enqueue; the stream is drained outside the timer
every 32 calls), 64 x 64 Cornell box, 1 spp per launch, brute force.  Prints one JSON line; DMT_HIP_LIB selects another build of the library for an A/B run."""
import json, os, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g
pkg = g.load_package()
scene = pkg.host_scene.cornell_box(64, 64)
with pkg.Renderer(0) as r:
    r.upload_scene(scene); r.set_limits(8)
    for i in range(64):
        r.render(1, sample_offset=i)
    r.sync()
    total, n = 0.0, 0
    for batch in range(64):
        t0 = time.perf_counter()
        for i in range(32):
            r.render(1, sample_offset=64 + n + i)
        total += time.perf_counter() - t0
        n += 32
        r.sync()
print(json.dumps({"lib": Path(os.environ["DMT_HIP_LIB"]).parent.name if os.environ.get("DMT_HIP_LIB") else "in-tree", "launches": n, "host_us_per_launch": round(total / n * 1e6, 3)}))
