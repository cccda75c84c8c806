"""The heterogeneous medium without a GPU (dmt_set_medium_grid): the host twin of the voxel march against
the numpy restatement bit for bit and against exact float64 integration, its invariants, the fixture's support, argument
errors, the .npy reader, the CLI's flag checks and the JSON scene key."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import medium_grid_ref as GR

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FIXTURE = GOLDEN / "medium_grid_plume_8.npy"
F = np.float32
SIGMA = 1.5
LO, HI = GR.BOX


@pytest.fixture(scope="module")
def grids():
    return [(name, GR.Grid(LO, HI, dens)) for name, dens in GR.make_grids(np.random.default_rng(41))]


def _march(pkg, G, o, d, t_end, target, sigma=SIGMA):
    return pkg.medium_grid_march(G.lo, G.hi, sigma, G.density, o, d, t_end, target)


# ---- the march against the float32 restatement -------------------------------------------------------------------
def test_march_equals_the_float32_restatement(pkg, grids):
    for k, (name, G) in enumerate(grids):
        o, d, t_end, target = GR.make_rays(np.random.default_rng(100 + k), 600)
        got = _march(pkg, G, o, d, t_end, target)
        want = [GR.march_f32(G, SIGMA, o[i], d[i], t_end[i], target[i]) for i in range(o.shape[0])]
        tau, ts = np.array([w[0] for w in want], F), np.array([w[1] for w in want], F)
        coll, steps = np.array([w[2] for w in want]), np.array([w[3] for w in want], np.int32)
        assert (got["collided"] == coll).all() and (got["steps"] == steps).all(), name
        assert got["tau"].tobytes() == tau.tobytes() and got["ts"].tobytes() == ts.tobytes(), name
        # the cases are there: rays that miss, pass and collide; targets 0 and +inf; segments that end inside the box
        assert (steps == 0).any() and coll.any() and (~coll & (steps > 0)).any(), name
        assert (coll & (target == 0)).any() and (np.isinf(target) & (steps > 0)).any(), name


def test_face_plane_rays(pkg, grids):
    """an axis-parallel ray in a face plane of the box marches the voxels behind that face; one ulp outside it misses"""
    _, G = grids[1]
    o = np.array([[-5, HI[1], 0.25], [-5, np.nextafter(F(HI[1]), F(np.inf)), 0.25]], F)
    d = np.array([[1, 0, 0], [1, 0, 0]], F)
    r = _march(pkg, G, o, d, [np.inf, np.inf], [np.inf, np.inf])
    assert r["steps"].tolist() == [2, 0] and r["tau"][0] > 0 and r["tau"][1] == 0
    want = GR.tau64(G, SIGMA, o[0], d[0], np.inf)
    assert abs(float(r["tau"][0]) - want) <= GR.bound(G, SIGMA, 2, 4.0, 7.0)


# ---- the march against float64 --------------------------------------------------------------------------------------
def test_march_against_float64(pkg, grids):
    worst = 0.0
    for k, (name, G) in enumerate(grids):
        o, d, t_end, target = GR.make_rays(np.random.default_rng(200 + k), 1500)
        r = _march(pkg, G, o, d, t_end, target)
        seg, _ = pkg.medium_segment(G.slo, G.shi, o, d, t_end)
        nx, ny, nz = G.n
        assert (r["steps"] <= nx + ny + nz).all(), name
        checked = 0
        for i in np.flatnonzero(r["steps"] > 0):
            t0, t1 = GR.clip64(G, o[i], d[i], t_end[i])
            if not np.isfinite(t1):
                continue
            b = GR.bound(G, SIGMA, int(r["steps"][i]), t0, t1)
            if r["collided"][i]:
                assert seg[i, 0] <= r["ts"][i] <= seg[i, 1], (name, i)
                err = abs(GR.tau64(G, SIGMA, o[i], d[i], t_end[i], upto=r["ts"][i]) - float(target[i]))
            else:
                err = abs(float(r["tau"][i]) - GR.tau64(G, SIGMA, o[i], d[i], t_end[i]))
            worst = max(worst, err / b)
            assert err <= b, (name, i, err, b)
            checked += 1
        assert checked > 300, name
    print(f"fp32 march against float64: the worst case is {worst:.3f} of the bound")


def test_constant_grid_is_the_homogeneous_medium(pkg):
    """density 1 everywhere: the optical depth is sigma_t * (t1 - t0) of dmt_medium_segment"""
    for shape in ((1, 1, 1), (5, 3, 2), (16, 16, 16)):
        G = GR.Grid(LO, HI, np.ones(shape, F))
        o, d, t_end, _ = GR.make_rays(np.random.default_rng(7), 1000)
        r = _march(pkg, G, o, d, t_end, np.full(o.shape[0], np.inf, F))
        seg, hit = pkg.medium_segment(LO, HI, o, d, t_end)
        assert ((r["steps"] > 0) == hit).all() and not r["collided"].any() and 0.2 < hit.mean() < 0.9
        want = SIGMA * (seg[:, 1].astype(np.float64) - seg[:, 0]) * hit
        b = SIGMA * (r["steps"] + 2) * 2.0 ** -22 * np.maximum(np.maximum(np.abs(seg[:, 0]), np.abs(seg[:, 1])), 1.0)
        fin = np.isfinite(seg[:, 1]) | ~hit
        assert (np.abs(r["tau"] - np.where(hit, want, 0.0))[fin] <= b[fin]).all(), shape


def test_zero_target_collides_at_the_entry_of_the_first_dense_voxel(pkg):
    dens = np.zeros((1, 1, 4), F)
    dens[0, 0, 2:] = (0.5, 2.0)
    dens[0, 0, 0] = 1e-3  # keeps the support at the whole box
    G = GR.Grid((0, 0, 0), (4, 1, 1), dens)
    o, d = np.array([[-1, 0.5, 0.5]] * 3, F), np.array([[1, 0, 0]] * 3, F)
    r = _march(pkg, G, o, d, [np.inf] * 3, [0.0, 0.25, np.inf], sigma=1.0)
    assert r["collided"].tolist() == [True, True, False]
    assert r["ts"][0] == 1.0 and r["steps"].tolist() == [1, 3, 4]           # the first voxel has s > 0
    assert abs(float(r["ts"][1]) - (3.0 + (0.25 - 1e-3) / 0.5)) < 1e-6     # 1e-3 in voxel 0, nothing in voxel 1, the rest in voxel 2
    assert abs(float(r["tau"][2]) - (1e-3 + 0.5 + 2.0)) < 1e-6


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_fixture_and_its_support(pkg):
    dens = np.load(FIXTURE)
    assert dens.shape == (8, 8, 8) and dens.dtype == np.dtype("<f4") and FIXTURE.stat().st_size < 4096
    G = GR.Grid((0, 0, 0), (8, 8, 8), dens)
    assert (G.imin, G.imax) == ((1, 1, 1), (6, 6, 7)) and G.positive == 168
    assert G.slo.tolist() == [1, 1, 1] and G.shi.tolist() == [7, 7, 8]
    # a ray through the empty border never enters the loop; one through the plume walks the support's six voxels, not eight
    o, d = np.array([[-1, 0.5, 4.5], [-1, 3.5, 4.5]], F), np.array([[1, 0, 0]] * 2, F)
    r = _march(pkg, G, o, d, [np.inf] * 2, [np.inf] * 2, sigma=1.0)
    assert r["steps"].tolist() == [0, 6] and r["tau"][0] == 0
    assert abs(float(r["tau"][1]) - float(dens[4, 3, :].astype(np.float64).sum())) < 1e-5


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_host_twin_refuses_bad_arguments(pkg):
    o, d, t = np.zeros((1, 3), F), np.ones((1, 3), F), np.ones(1, F)
    ok = np.ones((2, 2, 2), F)
    pkg.medium_grid_march(LO, HI, 1.0, ok, o, d, t, t)
    for dens in (np.full((2, 2, 2), np.nan, F), np.full((2, 2, 2), -1.0, F), np.full((1, 1, 1), np.inf, F), np.ones((1, 1, 513), F), np.ones((513, 1, 1), F)):
        with pytest.raises(pkg.DmtError):
            pkg.medium_grid_march(LO, HI, 1.0, dens, o, d, t, t)
    for lo, hi, sigma in (((0, 0, 0), (1, 0, 1), 1.0), ((0, 0, 0), (1, 1, 1), -1.0), ((0, 0, 0), (1, 1, 1), float("nan"))):
        with pytest.raises(pkg.DmtError):
            pkg.medium_grid_march(lo, hi, sigma, ok, o, d, t, t)
    with pytest.raises(AssertionError):
        pkg.medium_grid_march(LO, HI, 1.0, np.ones((2, 2), F), o, d, t, t)
    # an all-zero grid is an empty medium
    r = pkg.medium_grid_march(LO, HI, 1.0, np.zeros((2, 2, 2), F), np.array([[-5, 1, 0.25]], F), np.array([[1, 0, 0]], F), [np.inf], [0.0])
    assert r["steps"][0] == 0 and not r["collided"][0] and r["tau"][0] == 0


# ---- the .npy reader ----------------------------------------------------------------------------------------------------
def _npy(version, descr="<f4", fortran=False, shape=(2, 3, 4), data=None):
    header = f"{{'descr': '{descr}', 'fortran_order': {fortran}, 'shape': {tuple(shape)!r}, }}"
    lenbytes = 2 if version[0] == 1 else 4
    pad = -(6 + 2 + lenbytes + len(header) + 1) % 64
    header = (header + " " * pad + "\n").encode()
    if data is None:
        data = np.arange(int(np.prod(shape)), dtype="<f4").tobytes()
    return b"\x93NUMPY" + bytes(version) + len(header).to_bytes(lenbytes, "little") + header + data


def test_npy_reader(pkg, tmp_path):
    H = pkg.host_scene
    want = np.arange(24, dtype=F).reshape(2, 3, 4)
    for version in ((1, 0), (2, 0)):
        p = tmp_path / f"v{version[0]}.npy"
        p.write_bytes(_npy(version))
        assert np.load(p).tobytes() == want.tobytes()  # numpy reads what the test wrote
        got = H.read_npy_grid(p)
        assert got.shape == (2, 3, 4) and got.tobytes() == want.tobytes()
    assert H.read_npy_grid(FIXTURE).tobytes() == np.load(FIXTURE).tobytes()
    np.save(tmp_path / "saved.npy", want)
    assert H.read_npy_grid(tmp_path / "saved.npy").tobytes() == want.tobytes()
    cases = {
        "f8.npy": (_npy((1, 0), descr="<f8"), "dtype '<f8'"),
        "big.npy": (_npy((1, 0), descr=">f4"), "dtype '>f4'"),
        "fortran.npy": (_npy((1, 0), fortran=True), "Fortran order"),
        "short.npy": (_npy((1, 0))[:-4], "truncated: 96 bytes of data expected, 92 found"),
        "header.npy": (_npy((2, 0))[:40], "truncated .npy header"),
        "2d.npy": (_npy((1, 0), shape=(4, 6)), "2 dimensions"),
        "huge.npy": (_npy((1, 0), shape=(1, 1, 513), data=b""), "1 .. 512"),
        "v3.npy": (_npy((3, 0)), "version 3.0"),
        "text.npy": (b"not an array at all", "magic"),
    }
    for name, (blob, word) in cases.items():
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(ValueError, match=word):
            H.read_npy_grid(tmp_path / name)
    with pytest.raises(ValueError, match="cannot open"):
        H.read_npy_grid(tmp_path / "missing.npy")


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_medium_grid_option(tmp_path):
    """--medium-grid: in the help, and checked before any GPU is touched"""
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("-h")
    assert h.returncode == 0 and "--medium-grid <FILE>" in h.stdout
    (tmp_path / "f8.npy").write_bytes(_npy((1, 0), descr="<f8"))
    for args, word in ((("--medium-grid", str(FIXTURE)), "needs a medium"),
                       (("--medium", "0", "--medium-grid", str(FIXTURE)), "needs a medium"),
                       (("--medium", "1", "--medium-grid", str(tmp_path / "missing.npy")), "cannot open"),
                       (("--medium", "1", "--medium-grid", str(tmp_path / "f8.npy")), "dtype '<f8'"),
                       (("--medium", "1", "--medium-grid"), "Unknown option")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr[:300])


# ---- the JSON key ----------------------------------------------------------------------------------------------------------
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


def test_json_grid_key(pkg, tmp_path):
    H = pkg.host_scene
    fog = {"sigma_t": 0.25, "albedo": [0.9, 0.8, 0.7], "g": 0.5, "min": [-1, -2, -3], "max": [1, 2, 3]}
    plain = H.load_json(str(_with_medium(tmp_path, fog)))
    assert plain.medium_grid is None
    (tmp_path / "plume.npy").write_bytes(FIXTURE.read_bytes())
    grid = H.load_json(str(_with_medium(tmp_path, {**fog, "grid": "plume.npy"})))
    assert grid.medium_grid.shape == (8, 8, 8) and grid.medium_grid.tobytes() == np.load(FIXTURE).tobytes()
    # everything else loads byte for byte as without the key
    for name in ("xs", "ys", "zs", "mat_id", "bsdfs", "lights", "inf_lights", "camera"):
        assert getattr(grid, name).tobytes() == getattr(plain, name).tobytes(), name
    assert grid.lens == plain.lens and (grid.max_depth, grid.spp) == (plain.max_depth, plain.spp)
    assert all(np.array_equal(grid.medium[k], plain.medium[k]) for k in plain.medium)
    assert H.load_json(str(GOLDEN / "json_scene" / "three_boxes.json")).medium_grid is None
    (tmp_path / "f8.npy").write_bytes(_npy((1, 0), descr="<f8"))
    for bad, word in (({**fog, "grid": "missing.npy"}, "cannot open"), ({**fog, "grid": 3}, "path string"), ({**fog, "grid": "f8.npy"}, "dtype '<f8'")):
        with pytest.raises(ValueError, match=word):
            H.load_json(str(_with_medium(tmp_path, bad)))
