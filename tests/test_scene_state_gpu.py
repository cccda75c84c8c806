"""The scene layer's state (csrc/scene_state.hpp): a long-lived context that reached a soup and a BSDF array by a route --
triangles then BSDFs or the reverse, another soup or another array first, a blend pair that comes and goes, past the refused
blend record without its conductor, dmt_update_vertices to another pose and back -- renders the same film, byte for byte,
under brute force and under the BVH, as a fresh context that was given them directly, or refuses with the same message.  The
four refusals of a soup whose material index is outside the BSDF array keep their own texts.  Both DMT_BRUTE_CULL levels
below the default run the route in a process of their own and give the default's films.  dmt_sync passes after every case.
Every comparison is of bytes, integers or messages."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
ERR_INVALID = "(1)"
SIZE, DEPTH, SPP = 32, 4, 8
LONE_BLEND = "dmt_upload_bsdfs: a blend record (type 4) must be followed by its GGX conductor record"
OUTSIDE_RENDER = "dmt_render: a triangle's material index is outside the BSDF array"
OUTSIDE_PROBE = "dmt_test_trace_samples: material index outside the BSDF array"
OUTSIDE_AOVS = "dmt_render_aovs: material index outside the BSDF array"
OUTSIDE_OPACITY = "dmt_upload_opacity: material index outside the BSDF array"


class _World:
    """the Cornell box; its soups and BSDF arrays by name"""

    def __init__(self, pkg, tmp):
        sc = self.scene = pkg.host_scene.cornell_box(SIZE, SIZE)
        xs, ys, zs = (np.array(a, F).reshape(-1, 4) for a in (sc.xs, sc.ys, sc.zs))
        mat = np.array(sc.mat_id, np.uint32)
        bsdfs = np.array(sc.bsdfs, np.uint8).reshape(-1, 32)
        keep = len(mat) - 1                                 # the last mesh: the last run of one material
        while keep > 0 and mat[keep - 1] == mat[-1]:
            keep -= 1
        last = np.arange(len(mat)) >= keep
        src = GOLDEN / "json_scene"
        d = json.loads((src / "three_boxes.json").read_text())
        d["materials"][1]["metallic"] = 0.3
        shutil.copy(src / "sky_32x16.png", tmp / "sky_32x16.png")
        (tmp / "scene.json").write_text(json.dumps(d))
        pair = np.array(pkg.host_scene.load_json(tmp / "scene.json").bsdfs, np.uint8).reshape(-1, 32)[1:3]
        moved = xs.copy()
        moved[last, :3] += F(0.125)
        flat = lambda a: np.ascontiguousarray(a, F).reshape(-1)
        # name -> (xs, ys, zs, material ids)
        self.soups = {
            "box": (flat(xs), flat(ys), flat(zs), mat),
            "moved": (flat(moved), flat(ys), flat(zs), mat),
            "short": (flat(xs[:keep]), flat(ys[:keep]), flat(zs[:keep]), mat[:keep]),                  # without the last mesh
            "blendbox": (flat(xs), flat(ys), flat(zs), np.where(last, len(bsdfs), mat).astype(np.uint32)),  # the last mesh of a material behind the array
        }
        self.bsdfs = {
            "plain": bsdfs,
            "swapped": np.ascontiguousarray(bsdfs[::-1]),    # another array of the same length
            "blend": np.concatenate([bsdfs, pair]),          # the pair: what "blendbox" names
            "lone": np.concatenate([bsdfs, pair[:1]]),       # refused: a blend record without its conductor
        }
        self.pair = pair


@pytest.fixture(scope="module")
def W(pkg, tmp_path_factory):
    return _World(pkg, tmp_path_factory.mktemp("scene_state"))


def _cfg(soup, bsdfs):
    return dict(soup=soup, bsdfs=bsdfs)


TARGETS = [_cfg("box", "plain"), _cfg("box", "swapped"), _cfg("short", "plain"), _cfg("moved", "plain"), _cfg("blendbox", "blend"),
           _cfg("box", "blend"),                            # the blend rows over a soup that names no blend material
           _cfg("blendbox", "plain")]                       # refused: a material index is outside the array


def _rest(r, W):
    """what a launch needs beside the two records"""
    sc = W.scene
    r.upload_lights(sc.lights, sc.inf_lights)
    r.set_camera(sc.camera)
    r.set_limits(DEPTH)


def _refused(pkg, call, *needles):
    with pytest.raises(pkg.DmtError) as e:
        call()
    msg = str(e.value)
    assert ERR_INVALID in msg and all(n in msg for n in needles), msg


def _film(r, pkg, accel):
    """the film of one launch on a cleared film under an accel mode, as bytes; or the launch's refusal"""
    try:
        r.set_accel(accel)
        r.film_clear()
        r.render(SPP)
        r.sync()
    except pkg.DmtError as e:
        return str(e)
    mean, m2 = r.download_film()
    assert np.isfinite(mean).all()
    return mean.tobytes() + m2.tobytes()


def _snap(r, pkg, W):
    """What a context shows of its scene state.  A refused upload first gives dmt_last_error a known text; then the films under
    brute force and the BVH, or their refusals, and the message all that leaves."""
    _refused(pkg, lambda: r.upload_bsdfs(W.bsdfs["lone"]), LONE_BLEND)
    brute, bvh = _film(r, pkg, 0), _film(r, pkg, 1)
    r.set_accel(0)
    return brute, bvh, r.last_error()


@pytest.fixture(scope="module")
def fresh(pkg, W):
    """_snap of a fresh context that was given a soup and a BSDF array directly; each pair is rendered once"""
    memo = {}

    def get(c):
        key = repr(sorted(c.items()))
        if key not in memo:
            with pkg.Renderer(0) as r:
                r.upload_triangles(*W.soups[c["soup"]])
                r.upload_bsdfs(W.bsdfs[c["bsdfs"]])
                _rest(r, W)
                memo[key] = _snap(r, pkg, W)
        return memo[key]
    return get


@pytest.fixture(scope="module")
def old(pkg, W):
    """the long-lived context: every test below goes on from where the one before left it"""
    r = pkg.Renderer(0)
    r.upload_triangles(*W.soups["box"])
    r.upload_bsdfs(W.bsdfs["plain"])
    _rest(r, W)
    yield r
    r.close()


def test_the_configurations_differ(fresh):
    """what the comparisons below can tell apart: five films that differ, and one refusal"""
    snaps = [fresh(c) for c in TARGETS]
    assert all(isinstance(s[0], bytes) and isinstance(s[1], bytes) for s in snaps[:-1])
    assert len({s[0] for s in snaps[:5]}) == 5 and len({s[1] for s in snaps[:5]}) == 5
    assert all(s[2] == LONE_BLEND for s in snaps[:-1])      # a launch leaves no message of its own
    brute, bvh, last = snaps[-1]
    assert ERR_INVALID in brute and OUTSIDE_RENDER in brute and brute == bvh and last == OUTSIDE_RENDER


# ---- (a) triangles then BSDFs, and the reverse -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", TARGETS, ids=lambda c: c["soup"] + "-" + c["bsdfs"])
def test_either_order(old, pkg, W, fresh, c):
    old.upload_triangles(*W.soups[c["soup"]])
    old.upload_bsdfs(W.bsdfs[c["bsdfs"]])
    assert _snap(old, pkg, W) == fresh(c)
    old.upload_triangles(*W.soups["box"]), old.upload_bsdfs(W.bsdfs["plain"])
    old.upload_bsdfs(W.bsdfs[c["bsdfs"]])
    old.upload_triangles(*W.soups[c["soup"]])
    assert _snap(old, pkg, W) == fresh(c)
    with pkg.Renderer(0) as new:                            # and on a context that has seen neither
        new.upload_bsdfs(W.bsdfs[c["bsdfs"]])
        new.upload_triangles(*W.soups[c["soup"]])
        _rest(new, W)
        assert _snap(new, pkg, W) == fresh(c)
    old.sync()


# ---- (b) another soup or another BSDF array first: a stale record, count or cull table would show --------------------------
@pytest.mark.parametrize("c", TARGETS, ids=lambda c: c["soup"] + "-" + c["bsdfs"])
def test_another_soup_or_array_first(old, pkg, W, fresh, c):
    for other in TARGETS:
        if other == c:
            continue
        old.upload_triangles(*W.soups[other["soup"]])
        old.upload_bsdfs(W.bsdfs[other["bsdfs"]])
        _film(old, pkg, 0), _film(old, pkg, 1)              # launches have seen it, and a tree was built over it
        if other["soup"] != c["soup"]:
            old.upload_triangles(*W.soups[c["soup"]])
        if other["bsdfs"] != c["bsdfs"]:
            old.upload_bsdfs(W.bsdfs[c["bsdfs"]])
        assert _snap(old, pkg, W) == fresh(c)
    old.sync()


# ---- (c) a blend pair comes and goes ---------------------------------------------------------------------------------------
def test_a_blend_pair_comes_and_goes(old, pkg, W, fresh):
    old.upload_triangles(*W.soups["box"])
    for _ in range(2):
        old.upload_bsdfs(W.bsdfs["plain"])
        assert _snap(old, pkg, W) == fresh(_cfg("box", "plain"))
        _refused(pkg, lambda: old.upload_bsdfs(W.bsdfs["lone"]), LONE_BLEND)   # refused: the plain array stays, with its count
        _refused(pkg, lambda: old.upload_bsdfs(np.concatenate([W.bsdfs["plain"], W.pair[:1], W.bsdfs["plain"][:1]])), LONE_BLEND)
        assert _snap(old, pkg, W) == fresh(_cfg("box", "plain"))
        old.upload_bsdfs(W.bsdfs["blend"])                  # the pair comes: the blend rows run
        assert _snap(old, pkg, W) == fresh(_cfg("box", "blend"))
        old.upload_triangles(*W.soups["blendbox"])          # and a mesh takes it
        assert _snap(old, pkg, W) == fresh(_cfg("blendbox", "blend"))
        old.upload_bsdfs(W.bsdfs["plain"])                  # the pair goes under the mesh that names it
        assert _snap(old, pkg, W) == fresh(_cfg("blendbox", "plain"))
        _refused(pkg, lambda: old.upload_bsdfs(W.bsdfs["lone"]), LONE_BLEND)
        assert _snap(old, pkg, W) == fresh(_cfg("blendbox", "plain"))
        old.upload_triangles(*W.soups["box"])
    old.sync()


# ---- (d) dmt_update_vertices to another pose and back ----------------------------------------------------------------------
@pytest.mark.parametrize("bsdfs", ["plain", "blend"])
def test_update_vertices_to_another_pose_and_back(old, pkg, W, fresh, bsdfs):
    old.upload_triangles(*W.soups["box"])
    old.upload_bsdfs(W.bsdfs[bsdfs])
    for _ in range(2):
        for accel in (0, 1):                                # the update under either mode: it keeps or drops the tree
            old.set_accel(accel)
            old.update_vertices(*W.soups["moved"][:3])
            if bsdfs == "plain":
                assert _snap(old, pkg, W) == fresh(_cfg("moved", "plain"))
            old.set_accel(accel)
            old.update_vertices(*W.soups["box"][:3])
            assert _snap(old, pkg, W) == fresh(_cfg("box", bsdfs))
    old.sync()


# ---- (e) a material index outside the BSDF array: four refusals, each with its own text ------------------------------------
def test_the_four_refusals_keep_their_texts(old, pkg, W, fresh):
    px = np.zeros(1, np.int32)
    n = len(W.bsdfs["plain"])
    tris = len(W.soups["blendbox"][3])
    mat_tex = np.full((n, 4), 0xFFFFFFFF, np.uint32)
    mat_tex[:, 3] = 0
    mat_tex[:, 0] = 0
    textures = (np.full((16, 4), 200, np.uint8), np.array([[0, 4, 4]], np.int32), mat_tex, np.zeros((tris, 6), F))
    for first in ("soup", "array"):
        old.upload_triangles(*W.soups["box"]), old.upload_bsdfs(W.bsdfs["blend"])
        if first == "soup":
            old.upload_triangles(*W.soups["blendbox"]), old.upload_bsdfs(W.bsdfs["plain"])
        else:
            old.upload_bsdfs(W.bsdfs["plain"]), old.upload_triangles(*W.soups["blendbox"])
        for accel in (0, 1):
            old.set_accel(accel)
            for call, why in [(lambda: old.render(1), OUTSIDE_RENDER), (lambda: old.test_trace_samples(px, px, px), OUTSIDE_PROBE),
                              (lambda: old.render_aovs(1), OUTSIDE_AOVS)]:
                _refused(pkg, call, why)
                assert old.last_error() == why
        old.upload_textures(*textures)                      # dmt_upload_opacity asks for textures first
        try:
            _refused(pkg, lambda: old.upload_opacity(np.full(n, 0xFFFFFFFF, np.uint32)), OUTSIDE_OPACITY)
            assert old.last_error() == OUTSIDE_OPACITY
        finally:
            old.upload_textures(None, None, None, None)
        assert _snap(old, pkg, W) == fresh(_cfg("blendbox", "plain"))
        old.upload_bsdfs(W.bsdfs["blend"])                  # the array grows to hold the index: everything runs
        assert _snap(old, pkg, W) == fresh(_cfg("blendbox", "blend"))
    old.sync()


# ---- (f) DMT_BRUTE_CULL, read when a context is created: the levels below the default, each in a process of its own -------
def _route_digest(pkg, W):
    """one sha256 over the films of a route on a new context: the reverse order, another soup first, a pose and back"""
    h = hashlib.sha256()
    with pkg.Renderer(0) as r:
        r.upload_bsdfs(W.bsdfs["blend"])
        r.upload_triangles(*W.soups["short"])
        _rest(r, W)
        for soup in ("short", "blendbox", "box"):
            r.upload_triangles(*W.soups[soup])
            for accel in (0, 1):
                h.update(_film(r, pkg, accel))
        r.set_accel(0)
        for pose in ("moved", "box"):
            r.update_vertices(*W.soups[pose][:3])
            for accel in (0, 1):
                h.update(_film(r, pkg, accel))
        r.sync()
    return h.hexdigest()


@pytest.mark.parametrize("level", [0, 1])
def test_brute_cull_levels_give_the_same_films(pkg, W, monkeypatch, level):
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    want = _route_digest(pkg, W)
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "_scene_state_worker.py")], capture_output=True, text=True,
                       env=dict(os.environ, DMT_BRUTE_CULL=str(level)), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["level"] == str(level) and out["digest"] == want, out
