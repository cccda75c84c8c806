#!/usr/bin/env python3
"""Diagnostic (GPU box): the work of the brute-force pass's culled clusters.

Needs the counting build: make -C cuda-optix-pathtracing_amd/csrc variant NAME=cullcount DEFS=-DDMT_CULL_COUNTS=1, then
DMT_HIP_LIB=.../variants/libdmt_hip_cullcount.so python tools/diag_cull_counts.py [res] [spp] [depth].  Prints, per trace
call of a wave, the rays, the bound hits and compacted (ray, triangle) tasks per cluster kind, and the task passes.
"""
import ctypes
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g
pkg = g.load_package()
res = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
depth = int(sys.argv[3]) if len(sys.argv) > 3 else 8
scene = pkg.host_scene.cornell_box(res, res)
lib = pkg.binding.load_library()
out = (ctypes.c_ulonglong * 16)()
with pkg.Renderer(0) as r:
    r.upload_scene(scene)
    r.set_limits(depth)
    assert lib.dmt_diag_cull_counts(out, 1) == 0
    r.film_clear(); r.render(spp); r.sync()
    assert lib.dmt_diag_cull_counts(out, 1) == 0
c = [int(x) for x in out]
calls = max(c[0], 1)
print(f"{res}x{res} x {spp} spp, depth {depth}: {c[0]} trace calls (per wave), {c[1] / calls:.1f} closest + {c[2] / calls:.1f} "
      f"shadow rays per call")
for kind, name in ((0, "sphere"), (1, "box")):
    print(f"  {name:6s}: bound hits per call {c[4 + kind] / calls:6.2f} closest ({c[4 + kind] / max(c[1], 1):.3f} per closest ray), "
          f"{c[6 + kind] / calls:6.2f} shadow ({c[6 + kind] / max(c[2], 1):.3f} per shadow ray); tasks per call {c[8 + kind] / calls:7.2f}")
print(f"  task passes per call {c[3] / calls:.3f}, tasks per pass {(c[8] + c[9]) / max(c[3], 1):.1f}")
