"""The participating medium without a GPU (dmt_set_medium): the host twins against the numpy restatement
(the free-flight numbers and the clip bit for bit, Henyey-Greenstein against float64), the restatement's own camera rays
against lens_ref's exact ones, argument errors, the CLI's flag checks and the JSON scene key."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lens_ref as LR
import medium_ref as MR

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
G_VALUES = (-0.9, -0.3, 0.0, 0.3, 0.9)
HG_REL = 4e-6


# ---- medium_u ----------------------------------------------------------------------------------------------
def test_medium_values_equal_the_restatement(pkg):
    rng = np.random.default_rng(3)
    h = np.concatenate([[0, 1, 2, 0x7FFFFFFF, 0xFFFFFFFF], rng.integers(0, 2 ** 31, 195)]).astype(np.uint32)
    hh, dd = np.repeat(h, 9), np.tile(np.arange(9, dtype=np.uint32), h.size)
    got = pkg.medium_values(hh, dd)
    want = np.array([MR.medium_u(a, b) for a, b in zip(hh, dd)], F)
    assert got.tobytes() == want.tobytes()
    assert (got >= 0).all() and (got < 1).all()
    assert abs(float(got.mean()) - 0.5) < 6 / np.sqrt(12 * got.size)  # a hash, but a fair one


# ---- the clip ----------------------------------------------------------------------------------------------
LO, HI = np.array([-1.0, 0.5, -0.25], F), np.array([2.0, 1.5, 0.75], F)


def segment_cases():
    rng = np.random.default_rng(7)
    inf = np.inf
    o, d, t = [], [], []

    def add(oo, dd, tt=inf):
        dd = np.asarray(dd, np.float64)
        o.append(oo), d.append(dd / np.linalg.norm(dd)), t.append(tt)

    centre = (LO + HI) / 2
    for _ in range(200):  # through faces: from outside towards a point inside, and past the box
        p = rng.uniform(-4, 4, 3)
        add(p, rng.uniform(LO, HI) - p)
        add(p, rng.normal(size=3))
    for c in ((LO[0], LO[1], LO[2]), (HI[0], HI[1], HI[2]), (LO[0], HI[1], LO[2])):  # corners, and edges through their midpoints
        add(np.array(c) - (1, 2, 3), (1, 2, 3))
        add(np.array(c) + (3, -1, 2), (-3, 1, -2))
    add(np.array([LO[0], LO[1], 0.1]) - (1, 1, 0), (1, 1, 0))       # an edge, in the plane z = 0.1
    add(np.array([HI[0], 1.0, HI[2]]) - (2, 0, 2), (2, 0, 2))
    for axis in range(3):  # axis-parallel rays: inside, in a face plane (both faces), just outside, and backwards
        e = np.eye(3)[axis]
        for face in (LO, HI):
            for other in range(3):
                if other == axis:
                    continue
                p = centre.astype(np.float64).copy()
                p[other] = face[other]                      # in the face plane
                add(p - 5 * e, e), add(p + 5 * e, -e), add(p, e)
                p[other] = np.nextafter(F(face[other]), F(face[other] + (1 if face is HI else -1)))  # one ulp outside
                add(p - 5 * e, e)
        add(centre - 5 * e, e), add(centre, e), add(centre, -e)
    for _ in range(60):  # origins inside
        add(rng.uniform(LO, HI), rng.normal(size=3))
    for _ in range(40):  # boxes behind the origin
        p = rng.uniform(LO, HI) + rng.normal(size=3) * 0.1
        dd = rng.normal(size=3)
        add(p + 6 * dd / np.linalg.norm(dd), dd)
    for _ in range(80):  # t_hit inside the box, before it, beyond it, and zero
        p = rng.uniform(-4, 4, 3)
        dd = rng.uniform(LO, HI) - p
        add(p, dd, float(np.linalg.norm(dd)) * rng.choice([0.0, 0.3, 1.0, 1.7]))
    return np.array(o, F), np.array(d, F), np.array(t, F)


def test_medium_segment_equals_the_float32_restatement(pkg):
    o, d, t = segment_cases()
    seg, hit = pkg.medium_segment(LO, HI, o, d, t)
    want = [MR.segment_f32(LO, HI, o[i], d[i], t[i]) for i in range(o.shape[0])]
    ws = np.array([(a, b) for a, b, _ in want], F)
    wh = np.array([h for _, _, h in want])
    assert seg.tobytes() == ws.tobytes()
    assert (hit == wh).all()
    assert 0.3 < hit.mean() < 0.9  # the cases are of both kinds
    # and against the float64 clip where the segment is comfortably non-empty
    t0, t1 = MR.clip64(LO, HI, o.astype(np.float64), d.astype(np.float64), t.astype(np.float64))
    nz = (np.abs(d) > 1e-6).all(1) & (t1 - t0 > 1e-3)
    assert hit[nz].all() and np.abs(seg[nz, 0] - t0[nz]).max() < 1e-5 and np.abs(seg[nz, 1] - t1[nz]).max() < 1e-5


def test_medium_segment_face_plane_and_parallel_rules(pkg):
    """a parallel ray in a face plane is inside; one ulp beyond it is outside; a ray that starts on the far face leaves at once"""
    c = ((LO + HI) / 2).astype(F)
    o = np.array([[-5, HI[1], c[2]], [-5, np.nextafter(HI[1], F(9)), c[2]], [HI[0], c[1], c[2]]], F)
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0]], F)
    seg, hit = pkg.medium_segment(LO, HI, o, d, np.full(3, np.inf, F))
    assert hit.tolist() == [True, False, False]
    assert seg[0].tolist() == [4.0, 7.0]


# ---- Henyey-Greenstein ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", G_VALUES)
def test_phase_hg_eval_against_float64(pkg, g):
    c = np.concatenate([np.linspace(-1, 1, 2001), [-1.0, 1.0, 0.0]]).astype(F)
    got = pkg.phase_hg(g, cosine=c).astype(np.float64)
    want = MR.hg64(g, c)
    rel = np.abs(got - want) / want
    print(f"g = {g}: max relative error {rel.max():.3e}")
    assert rel.max() <= HG_REL
    # a density over the sphere: 2 pi * integral over the cosine = 1
    x = np.linspace(-1, 1, 200001)
    y = MR.hg64(g, x.astype(F))
    assert abs(2 * np.pi * float(((y[1:] + y[:-1]) / 2 * np.diff(x)).sum()) - 1) < 1e-3


@pytest.mark.parametrize("g", G_VALUES)
def test_phase_hg_sample(pkg, g):
    rng = np.random.default_rng(11)
    n = 20000
    wo = rng.normal(size=(n, 3))
    wo[:3] = np.eye(3)
    wo[3] = (1, 1, 1)  # the frame's other branch
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(F)
    u = rng.uniform(0, 1, (n, 2)).astype(F)
    u[:4, 0] = (0.0, 0.99999994, 0.5, 0.25)
    wi, pdf = pkg.phase_hg(g, wo=wo, u=u)
    assert np.abs(np.linalg.norm(wi.astype(np.float64), axis=1) - 1).max() < 4e-6
    # the pdf at the sampled direction is the evaluation there.  The cosine of (wo, wi) carries a few ulp of 1
    # (|dc| <= 4 * 2^-24 from the frame and the products), which the lobe's slope |dp/dc| / p <= 3 |g| / (1 - |g|)^2 magnifies
    c = (wo.astype(np.float64) * wi.astype(np.float64)).sum(1)
    ev = pkg.phase_hg(g, cosine=c.astype(F))
    bound = HG_REL + 8 * 2.0 ** -24 * 3 * abs(g) / (1 - abs(g)) ** 2
    assert (np.abs(ev - pdf) / pdf).max() <= bound
    # mean cosine against the direction of travel (-wo) is g: the cosine is bounded by 1, so its variance is <= 1
    assert abs(float((-c).mean()) - g) <= 6 / np.sqrt(n)


def test_camera_rays_restatement_matches_lens_ref(O):
    """the vectorised float64 rays the statistical GPU tests use are lens_ref's exact ones to well below their tolerances"""
    cam = MR.floor_scene(O, 8).camera
    px, py, s = np.array([0, 7, 3, 5, 2], np.int32), np.array([0, 7, 4, 1, 6], np.int32), np.array([0, 4095, 17, 1000, 333], np.int32)
    o, d, h = MR.camera_rays64(cam, px, py, s)
    o2, d2, _, h2 = LR.rays64(cam, 0.0, 1.0, px, py, s)
    assert (h == h2).all()
    assert np.abs(o - o2).max() == 0 and np.abs(d - d2).max() < 1e-7


# ---- argument errors ---------------------------------------------------------------------------------------
def test_host_twins_refuse_bad_arguments(pkg):
    o, d, t = np.zeros((1, 3), F), np.ones((1, 3), F), np.ones(1, F)
    for lo, hi in (((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, np.inf, 1)), ((0, np.nan, 0), (1, 1, 1)), ((2, 0, 0), (1, 1, 1))):
        with pytest.raises(pkg.DmtError):
            pkg.medium_segment(lo, hi, o, d, t)
    for g in (1.0, -1.0, 1.5, float("nan")):
        with pytest.raises(pkg.DmtError):
            pkg.phase_hg(g, cosine=np.zeros(1, F))


# ---- the CLI -----------------------------------------------------------------------------------------------
def test_cli_medium_options():
    """--medium and its companions: in the help, their values checked, before any GPU is touched"""
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("-h")
    assert h.returncode == 0
    for flag in ("--medium <SIGMA_T>", "--medium-albedo <R> <G> <B>", "--medium-g <G>", "--medium-box <X0> <Y0> <Z0> <X1> <Y1> <Z1>"):
        assert flag in h.stdout, flag
    for args, word in ((("--medium", "-1"), "invalid --medium:"), (("--medium", "nan"), "invalid --medium:"),
                       (("--medium", "1", "--medium-g", "1"), "invalid --medium-g"),
                       (("--medium", "1", "--medium-g", "-1.5"), "invalid --medium-g"),
                       (("--medium", "1", "--medium-albedo", "0.5", "1.5", "0.5"), "invalid --medium-albedo"),
                       (("--medium", "1", "--medium-albedo", "0.5", "-0.1", "0.5"), "invalid --medium-albedo"),
                       (("--medium", "1", "--medium-box", "0", "0", "0", "1", "0", "1"), "invalid --medium-box"),
                       (("--medium", "1", "--medium-box", "0", "0", "0", "1", "inf", "1"), "invalid --medium-box"),
                       (("--medium-g", "0.5"), "need --medium"), (("--medium-albedo", "1", "1", "1"), "need --medium"),
                       (("--medium-box", "0", "0", "0", "1", "1", "1"), "need --medium"),
                       (("--medium", "1", "--denoise"), "exclude each other"),
                       (("--medium", "1", "--medium-box", "0", "0", "0"), "Unknown option")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr[:300])


# ---- the JSON key ------------------------------------------------------------------------------------------
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


def test_json_medium_key(pkg, tmp_path):
    H = pkg.host_scene
    src = GOLDEN / "json_scene" / "three_boxes.json"
    plain = H.load_json(str(src))
    assert plain.medium is None
    fog = H.load_json(str(_with_medium(tmp_path, {"sigma_t": 0.25, "albedo": [0.9, 0.8, 0.7], "g": 0.5, "min": [-1, -2, -3], "max": [1, 2, 3]})))
    m = fog.medium
    assert (m["sigma_t"], m["g"]) == (0.25, 0.5)
    assert m["albedo"].tolist() == [F(0.9), F(0.8), F(0.7)] and m["box_min"].tolist() == [-1, -2, -3] and m["box_max"].tolist() == [1, 2, 3]
    # everything else loads byte for byte as without the key
    for name in ("xs", "ys", "zs", "mat_id", "bsdfs", "lights", "inf_lights", "camera"):
        assert getattr(fog, name).tobytes() == getattr(plain, name).tobytes(), name
    assert fog.lens == plain.lens and (fog.max_depth, fog.spp) == (plain.max_depth, plain.spp)
    dflt = H.load_json(str(_with_medium(tmp_path, {"sigma_t": 1, "min": [0, 0, 0], "max": [1, 1, 1]}))).medium
    assert dflt["albedo"].tolist() == [1, 1, 1] and dflt["g"] == 0
    for bad, word in (({"sigma_t": -1, "min": [0, 0, 0], "max": [1, 1, 1]}, "sigma_t"), ({"min": [0, 0, 0], "max": [1, 1, 1]}, "lacking"),
                      ({"sigma_t": 1, "min": [0, 0, 0], "max": [1, 0, 1]}, "below"), ({"sigma_t": 1, "g": 1, "min": [0, 0, 0], "max": [1, 1, 1]}, "'g'"),
                      ({"sigma_t": 1, "albedo": [2, 0, 0], "min": [0, 0, 0], "max": [1, 1, 1]}, "albedo"),
                      ({"sigma_t": 1, "min": [0, 0], "max": [1, 1, 1]}, "three numbers"),
                      ({"sigma_t": 1, "density": 2, "min": [0, 0, 0], "max": [1, 1, 1]}, "extraneous"), (3, "object")):
        with pytest.raises(ValueError, match=word):
            H.load_json(str(_with_medium(tmp_path, bad)))
