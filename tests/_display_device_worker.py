"""Subprocess body of test_display_gpu's device-pointer test: dmt_display_device on torch tensors against dmt_display on
the same data, with the film bound to a torch tensor (the null source) and with an explicit source plane.

A process of its own because torch has to open the GPU before the HIP library does (as tests/_temporal_device_worker.py).
Writes one npz with the host call's and the device call's outputs of every case."""
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from test_display_gpu import PARAMS_ALL_STAGES, make_plane  # noqa: E402

pkg = graft.load_package()
H, W = 50, 80
film, other = make_plane(H, W, seed=11), make_plane(H, W, seed=12)
SENTINEL = 77
out = {}


def tensors():
    t = (torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda:0"),
         torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()  # torch fills them on its own stream; the context writes them on another
    return t


with pkg.Renderer(0) as r:
    r.set_camera(pkg.host_scene.cornell_box(W, H).camera)
    mean_t = torch.from_numpy(film).to("cuda:0")
    m2_t = torch.zeros_like(mean_t)
    src_t = torch.from_numpy(other).to("cuda:0")
    torch.cuda.synchronize()  # the tensors' writes before the context's stream reads them
    r.film_bind(mean_t.data_ptr(), m2_t.data_ptr())
    for tag, params in (("auto", PARAMS_ALL_STAGES), ("manual", dict(exposure_ev=-1.0))):
        # the null source: the bound film, through both entry points, against the same plane passed from the host
        out[f"{tag}_host_f"], out[f"{tag}_host_u"] = r.display(params, image=film)
        out[f"{tag}_bound_f"], out[f"{tag}_bound_u"] = r.display(params)
        o4, o8 = tensors()
        r.display_device(params, None, o4.data_ptr(), o8.data_ptr())
        info = r.display_info()  # waits for the stream
        out[f"{tag}_dev_f"], out[f"{tag}_dev_u"] = o4.cpu().numpy(), o8.cpu().numpy()
        out[f"{tag}_dev_info"] = np.array([info["counted"], info["skipped"], info["nonfinite"], info["levels"]], np.int64)
        out[f"{tag}_dev_scale"] = np.float32(info["scale"])
        # an explicit source
        out[f"{tag}_src_host_f"], out[f"{tag}_src_host_u"] = r.display(params, image=other)
        o4, o8 = tensors()
        r.display_device(params, src_t.data_ptr(), o4.data_ptr(), o8.data_ptr())
        r.sync()
        out[f"{tag}_src_dev_f"], out[f"{tag}_src_dev_u"] = o4.cpu().numpy(), o8.cpu().numpy()
    # each output alone: the other tensor is never handed over
    o4, o8 = tensors()
    r.display_device(PARAMS_ALL_STAGES, None, o4.data_ptr(), None)
    r.sync()
    out["only_f"] = o4.cpu().numpy()
    o4, o8 = tensors()
    r.display_device(PARAMS_ALL_STAGES, None, None, o8.data_ptr())
    r.sync()
    out["only_u"] = o8.cpu().numpy()
    try:
        r.display_device(PARAMS_ALL_STAGES, None, None, None)
        out["both_null_refused"] = np.array(0)
    except pkg.DmtError:
        out["both_null_refused"] = np.array(1)
    out["film_after"] = mean_t.cpu().numpy()
np.savez(sys.argv[1], **out)
print("ok")
