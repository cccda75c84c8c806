"""Subprocess body of the spectrum's device-pointer test: a density grid handed over as a torch tensor under a spectrum.

A process of its own because torch has to open the GPU before the HIP library does (as tests/_medium_grid_device_worker.py).
Writes one npz: the Cornell film and the spectrum's info after a host upload and after a device-pointer upload of the plume
fixture, and the film of the grey grid rows."""
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


def _info(r):
    return json.dumps({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.medium_spectrum_info().items()})


with pkg.Renderer(0) as r:
    r.upload_scene(O.cornell_box(32, 32))
    r.set_limits(6)
    r.set_medium(**FOG)
    r.set_medium_grid(PLUME)
    out["grey_mean"], out["grey_m2"] = _film(r, 16)
    r.set_medium_spectrum((0.25, 1.0, 2.5), (0.0, 0.1, 0.2))
    out["host_info"] = _info(r)
    out["host_mean"], out["host_m2"] = _film(r, 16)
    r.clear_medium_grid()
    t = torch.from_numpy(PLUME.copy()).to("cuda:0")
    r.set_medium_grid(t)
    del t  # the context holds its own copy
    torch.cuda.empty_cache()
    out["device_info"] = _info(r)
    out["device_grid_active"] = np.array(r.medium_grid_info()["active"])
    out["device_mean"], out["device_m2"] = _film(r, 16)
np.savez(sys.argv[1], **out)
print("ok")
