"""Subprocess body of test_temporal_gpu's update-path test: temporal accumulation across update_vertices and across
update_vertices_device from a torch tensor's data_ptr().

A process of its own because torch has to open the GPU before the HIP library does (as tests/_refit_device_worker.py).
Writes one npz: for each of the four runs (host, device, host twice, device twice) the filtered output of frame B, the
history and (frames, reprojected, reset)."""
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from test_temporal import moving_pair  # noqa: E402
from test_temporal_gpu import _soup  # noqa: E402

pkg = graft.load_package()
a, b = moving_pair(50, 80, seed=1)
film_a, film_b = a["film"](3), b["film"](4)
middle = ((a["verts"].astype(np.float64) + b["verts"].astype(np.float64)) / 2).astype(np.float32)
keep = []  # the tensors handed over, alive until the end


def frame(r, s, film):
    r.set_camera(s["camera"])
    r.upload_aovs(s["albedo"], s["normal"], s["position"])
    r.upload_aov_surface(s["surface"])
    return r.denoise_temporal(film=film)


def host(r, verts):
    r.update_vertices(*_soup(verts))


def device(r, verts):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)  # p0 xyz, p1 xyz, p2 xyz
    t = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()                                     # the tensor's writes before the context's stream reads them
    r.update_vertices_device(t.data_ptr(), v.shape[0])
    keep.append(t)


out = {}
for tag, update, steps in (("host", host, (b["verts"],)), ("device", device, (b["verts"],)),
                           ("host_twice", host, (middle, b["verts"])), ("device_twice", device, (middle, b["verts"]))):
    with pkg.Renderer(0) as r:
        r.upload_triangles(*_soup(a["verts"]), np.zeros(a["verts"].shape[0], np.uint32))
        frame(r, a, film_a)
        for verts in steps:
            update(r, verts)
        out[tag + "_out"] = frame(r, b, film_b)
        out[tag + "_cv"], out[tag + "_len"] = r.download_history()
        info = r.temporal_info()
        out[tag + "_info"] = np.array([info["frames"], info["reprojected"], info["reset"]], np.int64)
np.savez(sys.argv[1], **out)
print("ok")
