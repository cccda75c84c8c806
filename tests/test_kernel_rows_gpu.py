"""The kernel table (csrc/dmt_hip.hip DMT_MEGAKERNELS): dmt_test_trace_samples shades with the body of the kernel
dmt_render launches, for every feature row a small scene reaches."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from test_parity_gpu import _many_lights_cornell, _textured_cornell

pytestmark = pytest.mark.gpu


def _blend_scene(pkg, tmp_path):
    """three_boxes.json with gold at 0.35 and glass at 0.6 metallic (test_fractional_metallic_blend_vs_oracle's scene)."""
    src = GOLDEN / "json_scene"
    d = json.loads((src / "three_boxes.json").read_text())
    d["materials"][1]["metallic"] = 0.35
    d["materials"][0]["metallic"] = 0.6
    (tmp_path / "sky_32x16.png").write_bytes((src / "sky_32x16.png").read_bytes())
    (tmp_path / "blend.json").write_text(json.dumps(d))
    return pkg.host_scene.load_json(tmp_path / "blend.json")


@pytest.mark.parametrize("accel", [0, 1])
@pytest.mark.parametrize("row", ["plain", "env", "area", "env_area", "tex", "blend", "ltree", "ltree2"])
def test_trace_samples_run_the_render_kernel(renderer, pkg, O, tmp_path, row, accel):
    """A 1-spp render at sample s into a cleared film holds each sample itself (Welford mean of one value); the test
    kernel's radiance of (pixel, s) must equal it exactly."""
    if row == "blend":
        sc, mode = _blend_scene(pkg, tmp_path), 0
    elif row == "tex":
        sc, mode = _textured_cornell(O, pkg, 32), 0
    elif row in ("ltree", "ltree2"):
        sc, mode = _many_lights_cornell(O, pkg, 32), 1 if row == "ltree" else 2
    else:
        sc, mode = O.cornell_box(32, 32), 0
        if "area" in row:
            sc.set_area_lights([20], [[5, 5, 5]])
        if "env" in row:
            sc.set_envmap(pkg.host_scene.synthetic_sky(16))
    s = 5
    renderer.upload_area_lights([], np.zeros((0, 3), np.float32))
    renderer.upload_scene(sc)
    renderer.set_limits(6)
    renderer.set_accel(accel)
    renderer.set_partition(0, 1)
    try:
        renderer.set_light_sampling(mode)
        renderer.film_clear()
        renderer.render(1, sample_offset=s)
        renderer.sync()
        mean, m2 = renderer.download_film()
        idx = np.random.default_rng(3).choice(renderer.width * renderer.height, 64, replace=False)
        px, py = (idx % renderer.width).astype(np.int32), (idx // renderer.width).astype(np.int32)
        L = renderer.test_trace_samples(px, py, np.full(64, s, np.int32))
    finally:
        renderer.set_light_sampling(0)
        renderer.set_accel(0)
        renderer.clear_envmap()
        renderer.upload_textures(None, None, None, None)
        renderer.upload_area_lights([], np.zeros((0, 3), np.float32))
    assert np.array_equal(m2[py, px, 3], np.ones(64, np.float32))
    assert np.isfinite(L).all() and L.max() > 0
    assert np.array_equal(L, mean[py, px, :3]), np.abs(L - mean[py, px, :3]).max()
