"""Subprocess body of the update_vertices_device tests: vertices handed over as a torch tensor's data_ptr().

A process of its own because torch has to open the GPU before the HIP library does (as bench.py does it).  Writes one npz:
the Cornell parity scene updated to its moved positions from device memory (film under BVH and under brute force), and the
4 000-triangle scene of test_device_records_equal_the_host_packer (films under both, the refitted tree)."""
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from test_bvh_refit import deform  # noqa: E402
from test_bvh_refit_gpu import REFIT, _film, _moved_cornell, _records_scene  # noqa: E402

pkg = graft.load_package()
out = {}


def update_from_tensor(r, soup):
    v = np.ascontiguousarray(np.stack([np.asarray(a)[:, :3] for a in soup], -1).reshape(-1, 9), np.float32)   # p0 xyz, p1 xyz, p2 xyz
    t = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()                                   # the tensor's writes before the context's stream reads them
    r.update_vertices_device(t.data_ptr(), v.shape[0])
    return t                                                    # kept alive by the caller


original, moved = _moved_cornell(pkg)
for accel, tag in ((1, "bvh"), (0, "brute")):
    with pkg.Renderer(0) as r:
        r.upload_scene(original)
        r.set_limits(8)
        r.set_accel(accel)
        r.set_accel_update(REFIT)
        before = _film(r, 16, accel)
        keep = update_from_tensor(r, (moved.xs, moved.ys, moved.zs))
        out[f"cornell_{tag}_action"] = np.int32(r.accel_update_info()["action"])
        out[f"cornell_{tag}_mean"], out[f"cornell_{tag}_m2"] = _film(r, 16, accel)
        out[f"cornell_{tag}_moved"] = np.bool_(not np.array_equal(before[0], out[f"cornell_{tag}_mean"]))

sc, soup = _records_scene(pkg)
with pkg.Renderer(0) as r:
    r.upload_scene(sc)
    r.set_limits(8)
    r.set_accel(1)
    r.set_accel_update(REFIT)
    keep = update_from_tensor(r, soup)
    out["records_bvh_mean"], out["records_bvh_m2"] = _film(r, 4, 1)
    out["records_nodes"], out["records_pairs"] = r.download_accel()
    out["records_brute_mean"], out["records_brute_m2"] = _film(r, 4, 0)
np.savez(sys.argv[1], **out)
print("ok")
