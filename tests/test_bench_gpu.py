"""bench.py end to end on one GPU: a plain run is the headline alone, --full adds the CPU baseline and its parity band."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(*args):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", *args],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    assert d["config"]["workload"] == "cornell_1024x1024_1024spp_8bounces" and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["film_ok"] is True
    assert d["cpu_baseline"] is None and d["parity"] is None and d["secondary"] is None
    assert d["roofline"]["frac"] is not None                     # committed counters + live kernel time, no run of its own
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == ["m2.npy", "mean.npy"]


def test_full_adds_the_cpu_baseline_and_its_parity_band():
    d = _bench("--full", "--workload", "cornell_512x512_64spp_4bounces", "--cpu-band-rows", "4")
    assert d["full"] is True and d["film_ok"] is True
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert d["parity"]["rows"] == 4 and d["parity"]["rmse_vs_cpu_rows"] < d["parity"]["tolerance"]
