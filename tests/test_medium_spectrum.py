"""The medium's spectrum without a GPU (dmt_set_medium_spectrum): the host twin of the event against the
float64 restatement, the identities of the one-sample balance heuristic on the twin's outputs, the second hash stream,
argument errors of the host twin, the CLI's flag checks and the JSON scene keys."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import medium_spectrum_ref as SR

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
N = 16384  # per set of channel extinctions: 65536 cases over SR.K_SETS


@pytest.fixture(scope="module")
def cases():
    """(k, beta, h, depth, tau_seg) per entry of SR.K_SETS, made once"""
    return [(k, *SR.make_cases(np.random.default_rng(100 + i), k, N)) for i, k in enumerate(SR.K_SETS)]


# ---- 1. the twin against float64 -----------------------------------------------------------------------------
def test_host_twin_equals_the_restatement(pkg, cases):
    worst, kept, total = 0.0, 0, 0
    counts, expect, var = np.zeros(3), np.zeros(3), np.zeros(3)
    for k, beta, h, depth, tau_seg in cases:
        got = pkg.medium_spectrum_event(k, beta, h, depth, tau_seg)
        same, keep, err, ref = SR.compare(got, k, beta, h, depth, tau_seg)
        assert same, k
        worst, kept, total = max(worst, err), kept + keep * N, total + N
        # the generator's own share of cases with every optical depth <= 8, before any output is looked at
        assert keep > 0.9, (k, keep)
        # what the cases are made to hold
        assert (ref["channel"] == -1).sum() == 4 and (got["weight"][ref["channel"] == -1] == 1).all()
        assert np.isinf(tau_seg).mean() > 0.01 and (beta == 0).any(1).mean() > 0.05 and (SR.medium_u(h, depth) < 1e-4).sum() >= 64
        T = ref["T"].astype(F)
        assert ((tau_seg == T).sum() > 100 and (tau_seg == np.nextafter(T, F(0))).sum() > 100 and (tau_seg == np.nextafter(T, F(np.inf))).sum() > 100)
        assert 0.2 < got["collided"].mean() < 0.8
        # on a collision tau_at is the target, on a pass the segment's depth
        assert (got["tau_at"][got["collided"]] == T[got["collided"]]).all() and (got["tau_at"][~got["collided"]] == tau_seg[~got["collided"]]).all()
        # no channel with p == 0 is ever returned
        j = got["channel"]
        ev = j >= 0
        assert (beta[ev, j[ev]] > 0).all()
        for c in range(3):
            counts[c] += (j == c).sum()
            expect[c] += ref["p"][:, c].sum()
            var[c] += (ref["p"][:, c] * (1 - ref["p"][:, c])).sum()
    print(f"host twin: worst relative weight error {worst:.3e} over {kept / total:.3f} of {total} cases; channel counts {counts} against {np.round(expect, 1)}")
    assert worst <= 4e-6
    assert (np.abs(counts - expect) <= 6 * np.sqrt(var)).all()


# ---- 2. identities -------------------------------------------------------------------------------------------
def test_weights_conserve_the_throughput_sum(pkg, cases):
    """sum_c beta_c w_c = sum_c beta_c for collision and pass alike: sum_c p_c w_c = 1 by construction"""
    worst = {True: 0.0, False: 0.0}
    for k, beta, h, depth, tau_seg in cases:
        got = pkg.medium_spectrum_event(k, beta, h, depth, tau_seg)
        b, w = beta.astype(np.float64), got["weight"].astype(np.float64)
        assert np.isfinite(w).all() and (w >= 0).all()
        rel = np.abs((b * w).sum(1) - b.sum(1)) / np.maximum(b.sum(1), 1e-30)
        for coll in (True, False):
            sel = got["collided"] == coll
            assert sel.sum() > 1000
            worst[coll] = max(worst[coll], float(rel[sel].max()))
    print(f"sum of beta after / before - 1: collision {worst[True] / 2.0 ** -24:.2f}, pass {worst[False] / 2.0 ** -24:.2f} (units of 2^-24)")
    assert worst[True] <= 8 * 2.0 ** -24 and worst[False] <= 8 * 2.0 ** -24


@pytest.mark.parametrize("k", SR.K_SETS)
def test_pass_weight_times_pass_probability_is_the_transmittance(pkg, k):
    """E over (u, v) of the pass weight times the pass indicator = e^(-tau_c).  The choice v picks j with probability p_j;
    given j the set of u that pass is {u: -log(1 - u) / q_j >= tau_seg}, of measure e^(-q_j tau_seg) exactly; the pass weight
    depends on neither.  The weight is the twin's; the measure is checked against the twin's decisions per channel."""
    rng = np.random.default_rng(17)
    _, q = SR.channels(k)
    q = q.astype(np.float64)
    for beta, tau_seg in (((1.0, 1.0, 1.0), 0.9), ((0.3, 1.7, 0.05), 2.5), ((0.9, 0.0, 0.5), 0.4)):
        n = 30000
        h, depth = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 9, n).astype(np.uint32)
        b = np.tile(np.asarray(beta, F), (n, 1))
        got = pkg.medium_spectrum_event(k, b, h, depth, np.full(n, tau_seg, F))
        passed = ~got["collided"]
        w = np.unique(got["weight"][passed], axis=0)
        assert w.shape == (1, 3)  # one pass weight, whatever u and v were
        p = np.asarray(beta, F).astype(np.float64) / np.asarray(beta, F).astype(np.float64).sum()
        measure = np.exp(-q * float(F(tau_seg)))
        for j in range(3):  # the twin's decisions have that measure
            sel = got["channel"] == j
            assert (sel.sum() == 0) == (p[j] == 0)
            if sel.sum():
                assert abs(passed[sel].mean() - measure[j]) <= 6 * np.sqrt(measure[j] * (1 - measure[j]) / sel.sum()) + 1e-12
        expectation = (p * measure).sum() * w[0].astype(np.float64)
        assert np.abs(expectation / measure - 1).max() <= 8 * 2.0 ** -24 + 4e-6, (k, beta, expectation, measure)


def test_choice_stream_is_independent_of_the_free_flight_stream(pkg):
    """the choice stream's offset is 2^31, beyond every depth dmt_set_limits admits: it is as good a stream as any"""
    n = 1 << 20
    rng = np.random.default_rng(23)
    for name, h in (("consecutive", np.arange(n, dtype=np.uint64) + 12345), ("strided", np.arange(n, dtype=np.uint64) * 31104 % 2 ** 32),  # 128 * 243: a pixel's samples; distinct
                    ("random", rng.integers(0, 2 ** 32, n, dtype=np.uint64))):
        for depth in (0, 3):
            d = np.full(n, depth, np.uint64)
            u, v = SR.medium_u(h, d).astype(np.float64), SR.medium_u(h, d + np.uint64(SR.CHOICE_STREAM)).astype(np.float64)
            corr = float(np.corrcoef(u, v)[0, 1])
            assert abs(corr) <= 6 / np.sqrt(n), (name, depth, corr)
            thirds = np.bincount((v * 3).astype(int), minlength=3) / n
            assert np.abs(thirds - 1 / 3).max() <= 6 * np.sqrt(2 / 9 / n), (name, depth, thirds)
            cells = np.bincount((u * 16).astype(int) * 16 + (v * 16).astype(int), minlength=256)
            chi2 = float(((cells - n / 256) ** 2 / (n / 256)).sum())
            assert abs(chi2 - 255) <= 6 * np.sqrt(2 * 255), (name, depth, chi2)
    hh = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
    dd = (rng.integers(0, 9, 256) + SR.CHOICE_STREAM).astype(np.uint32)
    assert pkg.medium_values(hh, dd).tobytes() == SR.medium_u(hh, dd).tobytes()  # the twin's hash takes the offset depth as it is


# ---- 3. argument errors of the host twin -----------------------------------------------------------------------
def test_host_twin_refuses_bad_extinctions(pkg):
    one = (np.ones((1, 3), F), [1], [0], [1.0])
    for k in ((0, 0, 0), (-1, 1, 1), (1, np.nan, 1), (1, 1, np.inf)):
        with pytest.raises(pkg.DmtError):
            pkg.medium_spectrum_event(k, *one)
    out = pkg.medium_spectrum_event((0, 0, 2), *one)
    assert out["channel"][0] in (0, 1, 2) and np.isfinite(out["weight"]).all()
    assert pkg.medium_spectrum_event((1, 2, 3), np.zeros((0, 3), F), [], [], [])["weight"].shape == (0, 3)


# ---- 4. the CLI ----------------------------------------------------------------------------------------------
def test_cli_medium_spectrum_options():
    """--medium-extinction and --medium-emission: in the help, their values checked, before any GPU is touched"""
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("-h")
    assert h.returncode == 0
    for flag in ("--medium-extinction <R> <G> <B>", "--medium-emission <R> <G> <B>"):
        assert flag in h.stdout, flag
    for args, word in ((("--medium", "1", "--medium-extinction", "1", "-0.5", "1"), "invalid --medium-extinction"),
                       (("--medium", "1", "--medium-extinction", "0", "0", "0"), "invalid --medium-extinction"),
                       (("--medium", "1", "--medium-extinction", "1", "nan", "1"), "invalid --medium-extinction"),
                       (("--medium", "1", "--medium-extinction", "1", "x", "1", "--medium-emission", "inf", "0", "0"), "invalid --medium-emission"),
                       (("--medium", "1", "--medium-emission", "1", "-2", "1"), "invalid --medium-emission"),
                       (("--medium", "1", "--medium-extinction", "1", "2"), "Unknown option"),  # a bad triple
                       (("--medium", "1", "--medium-emission", "1"), "Unknown option"),
                       (("--medium-extinction", "1", "2", "3"), "need --medium"), (("--medium-emission", "1", "2", "3"), "need --medium"),
                       (("--medium", "1", "--medium-extinction", "1", "2", "3", "--denoise"), "exclude each other")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr[:300])


# ---- 5. the JSON keys ----------------------------------------------------------------------------------------
def _with_medium(tmp_path, medium):
    src = GOLDEN / "json_scene" / "three_boxes.json"
    data = json.loads(src.read_text())
    data["medium"] = medium
    for p in src.parent.iterdir():  # the scene's files sit beside it
        if p.name != src.name and p.is_file():
            (tmp_path / p.name).write_bytes(p.read_bytes())
    out = tmp_path / "fog.json"
    out.write_text(json.dumps(data))
    return out


def test_json_medium_spectrum_keys(pkg, tmp_path):
    H = pkg.host_scene
    base = {"sigma_t": 0.25, "albedo": [0.9, 0.8, 0.7], "g": 0.5, "min": [-1, -2, -3], "max": [1, 2, 3]}
    grey = H.load_json(str(_with_medium(tmp_path, base)))
    assert grey.medium["extinction"].tolist() == [1, 1, 1] and grey.medium["emission"].tolist() == [0, 0, 0]
    rgb = H.load_json(str(_with_medium(tmp_path, {**base, "extinction": [0.25, 1, 2.5], "emission": [1, 2, 4]})))
    m = rgb.medium
    assert m["extinction"].tolist() == [0.25, 1, 2.5] and m["emission"].tolist() == [1, 2, 4]
    only = H.load_json(str(_with_medium(tmp_path, {**base, "emission": [0, 0.5, 0]}))).medium
    assert only["extinction"].tolist() == [1, 1, 1] and only["emission"].tolist() == [0, 0.5, 0]
    # everything else loads byte for byte as without the keys
    assert (m["sigma_t"], m["g"]) == (0.25, 0.5)
    for key in ("albedo", "box_min", "box_max"):
        assert m[key].tobytes() == grey.medium[key].tobytes()
    for name in ("xs", "ys", "zs", "mat_id", "bsdfs", "lights", "inf_lights", "camera"):
        assert getattr(rgb, name).tobytes() == getattr(grey, name).tobytes(), name
    assert rgb.lens == grey.lens and (rgb.max_depth, rgb.spp) == (grey.max_depth, grey.spp) and rgb.medium_grid is None
    assert H.load_json(str(GOLDEN / "json_scene" / "three_boxes.json")).medium is None
    for bad, word in (({**base, "extinction": [1, 2]}, "three numbers"), ({**base, "extinction": 2}, "three numbers"),
                      ({**base, "extinction": [1, -1, 1]}, "extinction"), ({**base, "extinction": [0, 0, 0]}, "all zero"),
                      ({**base, "emission": [1, "a", 1]}, "three numbers"), ({**base, "emission": [1, -0.5, 1]}, "emission"),
                      ({**base, "sigma_t": [1, 1, 1]}, "finite number"), ({**base, "colour": [1, 1, 1]}, "extraneous"),
                      ({"extinction": [1, 1, 1], "min": [0, 0, 0], "max": [1, 1, 1]}, "lacking")):
        with pytest.raises(ValueError, match=word):
            H.load_json(str(_with_medium(tmp_path, bad)))
