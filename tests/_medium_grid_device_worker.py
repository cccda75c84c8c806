"""Subprocess body of the set_medium_grid device-pointer test: density grids handed over as torch tensors.

A process of its own because torch has to open the GPU before the HIP library does (as tests/_refit_device_worker.py).
Writes one npz: the Cornell film and the grid's info after a host upload and after a device-pointer upload of the plume
fixture, the messages of the refused tensors, and the info of an all-zero tensor."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
O = graft.load_oracle()
out = {}
PLUME = np.load(ROOT / "tests" / "golden" / "medium_grid_plume_8.npy")
FOG = dict(sigma_t=1.2, albedo=(0.9, 0.8, 0.7), g=0.4, box_min=(-1.5, 0.5, -1.5), box_max=(1.5, 3.5, 1.5))  # as test_medium_grid_gpu.py


def _film(r, spp):
    r.film_clear()
    r.render(spp)
    r.sync()
    return r.download_film()


def refused(call):
    try:
        call()
    except pkg.DmtError as e:
        return str(e)
    return ""


with pkg.Renderer(0) as r:
    r.upload_scene(O.cornell_box(32, 32))
    r.set_limits(6)
    r.set_medium(**FOG)
    r.set_medium_grid(PLUME)
    out["host_info"] = json.dumps(r.medium_grid_info())
    out["host_mean"], out["host_m2"] = _film(r, 16)
    r.clear_medium_grid()
    t = torch.from_numpy(PLUME.copy()).to("cuda:0")
    r.set_medium_grid(t)
    del t  # the context holds its own copy
    torch.cuda.empty_cache()
    out["device_info"] = json.dumps(r.medium_grid_info())
    out["device_mean"], out["device_m2"] = _film(r, 16)
    # the same errors, from the device's own scan: the first offending voxel
    bad = torch.ones((2, 3, 4), dtype=torch.float32, device="cuda:0")
    bad[1, 2, 3], bad[1, 0, 0] = -1.0, float("nan")
    out["refused_values"] = refused(lambda: r.set_medium_grid(bad))
    out["refused_dtype"] = refused(lambda: r.set_medium_grid(bad.double()))
    out["refused_strides"] = refused(lambda: r.set_medium_grid(torch.ones((2, 3, 4), dtype=torch.float32, device="cuda:0")[:, :, ::2]))
    out["refused_size"] = refused(lambda: r.set_medium_grid(torch.ones((1, 1, 513), dtype=torch.float32, device="cuda:0")))
    out["after_info"] = json.dumps(r.medium_grid_info())
    out["after_mean"], out["after_m2"] = _film(r, 16)
    r.set_medium_grid(torch.zeros((2, 2, 2), dtype=torch.float32, device="cuda:0"))
    out["zeros_info"] = json.dumps(r.medium_grid_info())
np.savez(sys.argv[1], **out)
print("ok")
