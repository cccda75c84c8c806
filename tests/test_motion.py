"""Motion blur, host side: the sample times against an exact restatement, the vertex interpolation against
float64, the motion tree's invariants at both keys, and the argument checks that need no context.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import lens_ref as LR
import motion_ref as MR

F = np.float32


def _cases(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, w, n).astype(np.int32), rng.integers(0, h, n).astype(np.int32),
            np.concatenate([np.arange(8), rng.integers(0, 5000, n - 8)]).astype(np.int32))


def test_shutter_times(pkg):
    """dmt_shutter_times: inside [open, close], equal to open when the shutter is an instant, and the exact restatement of
    the base-41 scrambled radical inverse through one fmaf, bit for bit, on 200 samples of two frames."""
    digits = 0
    for (w, h), seed in (((64, 64), 1), ((48, 32), 2)):
        px, py, s = _cases(w, h, 100, seed)
        for open_, close in ((0.0, 1.0), (0.2, 0.7), (0.3, 0.3), (1.0, 1.0)):
            t = pkg.shutter_times(w, h, open_, close, px, py, s)
            assert t.dtype == F and (t >= F(open_)).all() and (t <= F(close)).all()
            if open_ == close:
                assert (t == F(open_)).all()
            ref = np.array([MR.shutter_time(w, h, px[i], py[i], s[i], open_, close) for i in range(len(px))], F)
            assert t.tobytes() == ref.tobytes(), (w, h, open_, close, np.abs(t - ref).max())
        p = LR.halton_params(w, h)
        digits = max(digits, max(LR.halton_index(p, int(px[i]), int(py[i]), int(s[i])) for i in range(len(px))))
        t01 = pkg.shutter_times(w, h, 0.0, 1.0, px, py, s)
        assert len(np.unique(t01)) > 90 and 0.3 < t01.mean() < 0.7  # a sequence, not a constant
    assert digits > 41 ** 4  # indices of five base-41 digits: the loop runs past its first steps


def test_motion_positions(pkg):
    rng = np.random.default_rng(3)
    k0, k1 = MR.random_keys(64, seed=11)
    # t = 0: key 0, bytes
    out = pkg.motion_positions(*k0, *k1, 0.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, k0))
    # dyadic inputs: exact
    g0, g1 = MR.random_keys(64, seed=12, grid=2.0 ** -6)
    for t in (0.25, 0.5, 1.0):
        out = pkg.motion_positions(*g0, *g1, t)
        for a, p0, p1 in zip(out, g0, g1):
            assert np.array_equal(a.astype(np.float64), p0.astype(np.float64) + t * (p1.astype(np.float64) - p0.astype(np.float64)))
    # random inputs: within 1 ulp of float64.  Two roundings: d = fl(p1 - p0), off by half an ulp of |p1 - p0| and scaled by
    # t <= 1, and the fmaf's own, half an ulp of the result.  So the ulp is taken at the larger of |p1 - p0| and |result|
    # (where the difference cancels it is the difference's rounding that is left).
    for t in rng.uniform(0, 1, 8).astype(F):
        out = pkg.motion_positions(*k0, *k1, float(t))
        for a, p0, p1 in zip(out, k0, k1):
            ref = p0.astype(np.float64) + float(t) * (p1.astype(np.float64) - p0.astype(np.float64))
            ulp = np.spacing(np.maximum(np.abs(ref), np.abs(p1.astype(np.float64) - p0.astype(np.float64))).astype(F)).astype(np.float64)
            lanes = np.arange(a.size) % 4 != 3
            assert (np.abs(a.astype(np.float64) - ref)[lanes] <= ulp[lanes]).all()
            assert np.array_equal(a[~lanes], p0[~lanes])  # the pad lane is key 0's


def test_motion_tree_holds_both_keys(pkg, O):
    scenes = {"cornell": MR.cornell_keys(O.cornell_box(32, 32)), "random300": MR.random_keys(300)}
    for n in (1, 2, 3):
        scenes[f"floor{n}"] = MR.floor_keys(n)
    for name, (k0, k1) in scenes.items():
        n = k0[0].size // 4
        r = pkg.motion_bvh_validate(*k0, *k1)
        assert r["ok"], (name, r)
        assert r["node_count"] >= 1 and r["depth"] >= 1 and (n + 1) // 2 <= r["pair_count"] <= n
        # teeth (pure numpy): key 1 leaves the triangles' own key-0 boxes, which bound the leaves of a tree built from key 0
        # alone -- such a tree would not contain key 1
        escaped = MR.key1_escapes_key0_boxes(k0, k1)
        assert escaped >= {"cornell": 16, "random300": 200}.get(name, n), (name, escaped)
    # equal keys: the motion tree is the static tree
    k0, _ = MR.random_keys(300)
    assert pkg.motion_bvh_validate(*k0, *k0)["node_count"] == pkg.bvh_validate(*k0)["node_count"]


def test_arguments(pkg):
    one = np.zeros(1, np.int32)
    nan, inf = float("nan"), float("inf")
    for open_, close in ((-0.1, 0.5), (0.5, 0.4), (0.0, 1.5), (nan, 1.0), (0.0, nan), (0.0, inf), (-inf, 0.0)):
        with pytest.raises(pkg.DmtError):
            pkg.shutter_times(64, 64, open_, close, one, one, one)
    with pytest.raises(pkg.DmtError):
        pkg.shutter_times(64, 64, 0.0, 1.0, np.array([64], np.int32), one, one)  # outside the frame
    with pytest.raises(pkg.DmtError):
        pkg.shutter_times(64, 64, 0.0, 1.0, one, one, np.array([-1], np.int32))
    with pytest.raises(pkg.DmtError):
        pkg.shutter_times(0, 64, 0.0, 1.0, one, one, one)
    k0, k1 = MR.floor_keys(2)
    for t in (nan, inf):
        with pytest.raises(pkg.DmtError):
            pkg.motion_positions(*k0, *k1, t)
    lib = pkg.load_library()
    from cuda_optix_pathtracing_amd import binding
    for name in ("dmt_set_motion", "dmt_clear_motion", "dmt_set_shutter", "dmt_motion_info", "dmt_shutter_times", "dmt_motion_positions",
                 "dmt_motion_bvh_validate", "dmt_test_shutter_times", "dmt_test_closest_hit_at"):
        assert name in binding.EXPORTED_SYMBOLS and hasattr(lib, name)
    # no context: refused before anything is touched
    assert lib.dmt_set_motion(None, None, None, None, C.c_size_t(0)) != 0
    assert lib.dmt_clear_motion(None) != 0
    assert lib.dmt_set_shutter(None, C.c_float(0.0), C.c_float(1.0)) != 0
    assert lib.dmt_motion_info(None, None, None, None, None, None, None) != 0
    assert lib.dmt_motion_bvh_validate(None, None, None, None, None, None, C.c_size_t(3), None, None, None) != 0


def test_cli_flags(pkg):
    """--shutter and --motion-scene: in the help, their values checked, and a key 1 of another triangle count is an error --
    all before any GPU is touched."""
    import subprocess
    from conftest import GOLDEN, ROOT
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("-h")
    assert h.returncode == 0 and "--shutter <OPEN> <CLOSE>" in h.stdout and "--motion-scene <file>" in h.stdout
    for bad in (("0.5", "0.25"), ("-0.1", "1"), ("0", "1.5"), ("nan", "1")):
        r = run("--shutter", *bad)
        assert r.returncode == 1 and "invalid --shutter" in r.stderr, (bad, r.stderr)
    boxes, cornell = GOLDEN / "json_scene" / "three_boxes.json", GOLDEN / "pbrt" / "cornell_box.pbrt"
    r = run("--scene", str(boxes), "--motion-scene", str(cornell))
    assert r.returncode == 1 and "key 1 must move the same triangles" in r.stderr, r.stderr
    r = run("--motion-scene", str(GOLDEN / "json_scene" / "no_such_file.json"))
    assert r.returncode == 1 and "motion scene" in r.stderr, r.stderr
