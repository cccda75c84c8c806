"""Alpha cutouts without a GPU (dmt_upload_opacity): the host twin of the opacity lookup against the numpy
restatement bit for bit, the JSON loader's "opacity" texture type and material keys, and the CLI option."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cutout_ref as CR
from conftest import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_cutout_fixture as MK  # noqa: E402

F = np.float32
FIX = GOLDEN / "cutout"
SCENE = FIX / "cards.json"


def _textures(rng):
    """1x1, 1x7, 5x3 and 16x16; the alpha bytes include 0, 127, 128 and 255 (on the cutoffs 0, 0.5 -> 127.5, and 1)"""
    special = np.array([0, 127, 128, 255], np.uint8)
    alphas = [np.array([[128]], np.uint8), rng.choice(special, (7, 1)), rng.integers(0, 256, (3, 5)).astype(np.uint8),
              np.where(rng.random((16, 16)) < 0.5, rng.choice(special, (16, 16)), rng.integers(0, 256, (16, 16))).astype(np.uint8)]
    assert [a.shape[::-1] for a in alphas] == [(1, 1), (1, 7), (5, 3), (16, 16)]
    rgba, desc = CR.pack_textures(alphas)
    rgba[:, :3] = rng.integers(0, 256, (rgba.shape[0], 3))  # the colour bytes must not matter
    return rgba, desc


def _cases(rng, n, desc):
    tex = rng.integers(0, desc.shape[0], n).astype(np.int32)
    uv6 = rng.uniform(-3.0, 4.0, (n, 6)).astype(F)  # negative and beyond 1: the mirror wrap
    bu = rng.uniform(0, 1, n).astype(F)
    bv = (rng.uniform(0, 1, n).astype(F) * (F(1) - bu)).astype(F)
    k = n // 8  # corners and edges of the triangle
    bu[:k], bv[:k] = 0, 0
    bu[k:2 * k], bv[k:2 * k] = 1, 0
    bu[2 * k:3 * k], bv[2 * k:3 * k] = 0, 1
    bv[3 * k:4 * k] = 0
    bu[4 * k:5 * k] = 0
    bv[5 * k:6 * k] = F(1) - bu[5 * k:6 * k]
    # texel centres: UVs on a texel grid at the corners, so that alpha8 is a texture byte itself (and lands ON a cutoff8)
    j = slice(6 * k, 7 * k)
    w, h = desc[tex[j], 1].astype(np.float64), desc[tex[j], 2].astype(np.float64)
    cx, cy = (rng.integers(-20, 40, k) + 0.5) / w, (rng.integers(-20, 40, k) + 0.5) / h
    uv6[j] = np.stack([cx, cy, cx, cy, cx, cy], 1).astype(F)
    return tex, uv6, bu, bv


@pytest.mark.parametrize("cutoff", [0.0, 0.5, 1.0, 0.25, 128 / 255])
def test_opacity_eval_equals_the_restatement(pkg, cutoff):
    rng = np.random.default_rng(11)
    rgba, desc = _textures(rng)
    n = 4000
    tex, uv6, bu, bv = _cases(rng, n, desc)
    a, ok = pkg.opacity_eval(rgba, desc, tex, uv6, bu, bv, cutoff)
    ref = CR.alpha8(rgba, desc, tex, uv6, bu, bv)
    assert a.dtype == F and a.tobytes() == ref.tobytes(), np.abs(a - ref).max()
    assert np.array_equal(ok, CR.passes(ref, cutoff))
    assert (a >= 0).all() and (a <= 255).all()
    # the cases do cover the ground: every texture, both verdicts (cutoff 0 passes everything), and alpha8 ON the cutoff
    assert len(np.unique(tex)) == 4
    c8 = F(cutoff) * F(255)
    if cutoff == 0.0:
        assert ok.all()
    else:
        assert ok.any() and (~ok).any()
    if c8 == np.floor(c8):
        assert (a == c8).sum() >= 10 and ok[a == c8].all()  # >= : a hit exactly on the cutoff passes
    assert ((a > 0) & (a < 255) & (a != np.floor(a))).sum() > n // 4  # genuinely interpolated values


def test_opacity_eval_on_texel_centres_returns_the_bytes(pkg):
    a8 = MK.decal_alpha()
    rgba, desc = CR.pack_textures([a8])
    yy, xx = np.mgrid[0:4, 0:4]
    cx, cy = ((xx.ravel() + 0.5) / 4).astype(F), ((yy.ravel() + 0.5) / 4).astype(F)
    uv6 = np.stack([cx, cy, cx, cy, cx, cy], 1)
    z = np.zeros(16, F)
    a, ok = pkg.opacity_eval(rgba, desc, np.zeros(16, np.int32), uv6, z + F(0.25), z + F(0.5), 0.5)
    assert np.array_equal(a, a8.ravel().astype(F)) and np.array_equal(ok, a8.ravel() >= 128)
    # mirror wrap: u -> -u and u -> 2 - u read the same texel
    for m in (np.array([-1, 1], F), np.array([1, -1], F)):
        uvm = uv6 * np.tile(m, 3)
        assert np.array_equal(pkg.opacity_eval(rgba, desc, np.zeros(16, np.int32), uvm, z, z, 0.5)[0], a)
    uv2 = np.tile(np.array([2, 0], F), 3) - uv6 * np.tile(np.array([1, -1], F), 3)
    assert np.array_equal(pkg.opacity_eval(rgba, desc, np.zeros(16, np.int32), uv2, z, z, 0.5)[0], a)


def test_opacity_eval_checks_its_arguments(pkg):
    rgba, desc = CR.pack_textures([CR.checker(4)])
    one = (np.zeros(1, np.int32), np.zeros((1, 6), F), np.zeros(1, F), np.zeros(1, F))
    pkg.opacity_eval(rgba, desc, *one, 0.5)
    for cutoff in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(pkg.DmtError):
            pkg.opacity_eval(rgba, desc, *one, cutoff)
    with pytest.raises(pkg.DmtError):  # texture index out of range
        pkg.opacity_eval(rgba, desc, np.ones(1, np.int32), *one[1:], 0.5)
    with pytest.raises(pkg.DmtError):  # descriptor past the texel array
        pkg.opacity_eval(rgba, np.array([[0, 4, 5]], np.int32), *one, 0.5)
    # any finite or non-finite UV reads inside the texture (coordinates are clamped before the conversion to int)
    wild = np.array([[1e30, -1e30, np.inf, -np.inf, np.nan, 3e9]], F)
    a, _ = pkg.opacity_eval(rgba, desc, np.zeros(1, np.int32), wild, np.full(1, 0.3, F), np.full(1, 0.3, F), 0.5)
    assert a.shape == (1,)


# ---- the JSON loader ---------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_writes(tmp_path):
    MK.main(tmp_path)
    for name in ("cards.json", "leaf_rgba_8x8.png", "fence_grey_5x3.png", "decal_ga_4x4.png", "sky_8x8.png"):
        assert (tmp_path / name).read_bytes() == (FIX / name).read_bytes(), name


def test_json_scene_with_opacity(pkg):
    sc = pkg.host_scene.load_json(SCENE)
    assert sc.bsdfs.shape[0] == 4 and sc.tri_count == 2 + 2 + 2 + 12
    assert sc.mat_opacity is not None and sc.mat_opacity.tolist() == [CR.NONE, 0, 1, CR.NONE]
    assert sc.opacity_cutoff == F(0.25)
    assert sc.tex_desc.tolist() == [[0, 8, 8], [64, 5, 3], [79, 4, 4]]
    want = np.concatenate([MK.leaf_alpha().ravel(), MK.fence_alpha().ravel(), MK.decal_alpha().ravel()])
    assert np.array_equal(sc.tex_rgba[:, 3], want)                               # A = the file's alpha byte / the grey byte
    assert (sc.tex_rgba[:, :3] == sc.tex_rgba[:, 3:4]).all()                      # RGB = the same byte
    assert sc.mat_tex.shape == (4, 4) and (sc.mat_tex[:, :3] == CR.NONE).all()   # no colour texture anywhere
    assert sc.tri_uv.shape == (sc.tri_count, 6)
    # world members in key order: box (solid), canopy (leafmat), gate (fencemat), ground (chalk)
    assert sc.mat_id.tolist() == [3] * 12 + [1] * 2 + [2] * 2 + [0] * 2
    # the host twin on the loaded arrays: the centre of the leaf card is leaf, its corner is hole
    tri = 12
    uv = sc.tri_uv[tri].reshape(3, 2)
    bary = np.array([[0, 0], [1, 0], [0, 1]], F)  # (bu, bv) of the corners
    i, j = next((i, j) for i in range(3) for j in range(i + 1, 3) if (np.abs(uv[i] - uv[j]) == 1).all())  # the card's diagonal
    mid = (bary[i] + bary[j]) / 2
    a, ok = pkg.opacity_eval(sc.tex_rgba, sc.tex_desc, [0, 0], sc.tri_uv[[tri, tri]], [mid[0], 0.0], [mid[1], 0.0], sc.opacity_cutoff)
    assert ok.tolist() == [True, False] and a[0] == 255 and a[1] == 0


def _variant(tmp_path, edit):
    d = json.loads(SCENE.read_text())
    edit(d)
    for f in FIX.glob("*.png"):
        shutil.copy(f, tmp_path / f.name)
    p = tmp_path / "scene.json"
    p.write_text(json.dumps(d))
    return p


def _strip(d):
    d["textures"] = []
    for m in d["materials"]:
        m.pop("opacity", None), m.pop("opacity-cutoff", None)


def test_json_scene_without_the_keys_has_no_opacity(pkg, tmp_path):
    plain = pkg.host_scene.load_json(_variant(tmp_path, _strip))
    full = pkg.host_scene.load_json(SCENE)
    assert plain.mat_opacity is None and plain.opacity_cutoff is None
    assert plain.tex_desc is None and plain.tri_uv is None  # nothing textured: the plain kernels run, as before
    for k in ("xs", "ys", "zs", "mat_id", "bsdfs", "lights", "camera"):
        assert np.array_equal(getattr(plain, k), getattr(full, k)), k
    assert pkg.host_scene.load_json(GOLDEN / "json_scene" / "three_boxes.json").mat_opacity is None


@pytest.mark.parametrize("edit, needle", [
    (lambda d: d["materials"][1].update(opacity="nope"), "'opacity' texture name should be an existing named texture"),
    (lambda d: d["materials"][1].update(opacity=3), "'opacity' should be an opacity texture name"),
    (lambda d: d["textures"][0].update(type="roughness") or d["materials"][2].update({"opacity-cutoff": 0.25}),
     "expect 1 channel"),  # (the 4-channel file is no roughness texture)
    (lambda d: d["textures"].append({"name": "rough", "type": "roughness", "path": "fence_grey_5x3.png"}) or d["materials"][1].update(opacity="rough"),
     "should point to a 'opacity' texture"),
    (lambda d: d["materials"][1].update({"opacity-cutoff": 1.5}), "'opacity-cutoff' should be a number in [0, 1]"),
    (lambda d: d["materials"][1].update({"opacity-cutoff": -0.1}), "'opacity-cutoff' should be a number in [0, 1]"),
    (lambda d: d["materials"][1].update({"opacity-cutoff": "half"}), "'opacity-cutoff' should be a number in [0, 1]"),
    (lambda d: d["materials"][0].update({"opacity-cutoff": 0.5}), "'opacity-cutoff' needs an 'opacity' texture"),
    (lambda d: d["materials"][2].update({"opacity-cutoff": 0.75}), "should share one 'opacity-cutoff'"),
    (lambda d: d["textures"][0].update(path="sky_8x8.png"), "opacity expects 1, 2 or 4 channels"),
])
def test_json_loader_rejects_bad_opacity_keys(pkg, tmp_path, edit, needle):
    with pytest.raises(Exception) as e:
        pkg.host_scene.load_json(_variant(tmp_path, edit))
    assert needle in str(e.value), str(e.value)


def test_default_cutoff_is_a_half(pkg, tmp_path):
    def edit(d):
        for m in d["materials"]:
            m.pop("opacity-cutoff", None)
    assert pkg.host_scene.load_json(_variant(tmp_path, edit)).opacity_cutoff == F(0.5)


# ---- the CLI ---------------------------------------------------------------------------------------------------
def test_cli_lists_cutouts():
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("--help")
    assert h.returncode == 0 and "--cutouts <on|off>" in h.stdout and "off:" in h.stdout[h.stdout.index("--cutouts"):]
    r = run("--cutouts", "maybe")
    assert r.returncode == 1 and "invalid --cutouts" in r.stderr, r.stderr
