"""CPU tests of smooth shading's host side: dmt_smooth_normals against its restatement, the FBX reader's
normal layer, the loaders' tri_normals, and the octahedral words of the record (tests/vnormal_ref.py)."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

import vnormal_ref as V
from conftest import GOLDEN, ROOT

sys.path.insert(0, str(ROOT / "tools"))
import make_fbx_fixture as fx  # noqa: E402


def _soa(T):
    """[n, 3 corners, xyz] -> xs, ys, zs in the upload layout"""
    T = np.asarray(T, np.float32)
    return tuple(np.concatenate([T[:, :, k], np.zeros((T.shape[0], 1), np.float32)], 1) for k in range(3))


def _unit_cube():
    P = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, c, d in quads:
        tris += [(P[a], P[b], P[c]), (P[a], P[c], P[d])]
    return np.array(tris, np.float32)


# ---- the record's words -------------------------------------------------------------------------------------------
def test_the_reference_encoder_cannot_carry_normals(O):
    """Why the record is not written with the reference's octaFromDir as it stands: it clamps to [0, 1] before rounding."""
    d = np.array([0.3, 0.5, 0.81], np.float32)
    w = O.lib().oracle_octa_from_dir(d.ctypes.data_as(C.c_void_p))
    assert (w & 0xFFFF) in (0, 1) and (w >> 16) in (0, 1)


def test_octahedral_round_trip_is_within_1e_4_rad(O):
    rng = np.random.default_rng(2)
    d = rng.standard_normal((4096, 3))
    d = np.concatenate([d, np.eye(3), -np.eye(3), [[1, 1, 1], [-1, -1, -1], [1, -1, 0], [0, 1, -1]]])
    d = V.normalise_host(d)
    back = V.decode_words(O, V.octa_words(d)).astype(np.float64)
    ang = V.angle_between(back, d)
    assert ang.max() < 1e-4, ang.max()
    axis = ang[4096:4102]
    assert axis.max() < 3e-5, axis  # axis-aligned normals: about 1.5e-5


# ---- dmt_smooth_normals -------------------------------------------------------------------------------------------
def test_smooth_normals_match_the_restatement(pkg):
    T, _ = V.icosphere(center=(0.3, -1.0, 2.0), radius=1.7)
    rng = np.random.default_rng(4)
    cube = _unit_cube() * np.float32(0.75) + np.float32(3.0)
    fan = rng.standard_normal((1, 3)).astype(np.float32) + rng.standard_normal((12, 3, 3)).astype(np.float32) * np.float32(0.5)
    fan[:, 0] = fan[0, 0]  # twelve random triangles around one shared vertex
    soup = np.concatenate([T, cube, fan])
    xs, ys, zs = _soa(soup)
    for crease in (180.0, 60.0, 25.0, 0.0):
        got = pkg.smooth_normals(xs, ys, zs, crease)
        ref = V.smooth_normals(xs, ys, zs, crease)
        assert got.shape == (soup.shape[0], 9) and np.abs(got - ref).max() < 1e-6, (crease, np.abs(got - ref).max())
        assert np.allclose(np.linalg.norm(got.reshape(-1, 3), axis=1), 1.0, atol=1e-6)


def test_smooth_normals_of_a_unit_cube(pkg):
    xs, ys, zs = _soa(_unit_cube())
    fn, ok = V.face_normals(xs, ys, zs)
    assert ok.all()
    hard = pkg.smooth_normals(xs, ys, zs, 30.0).reshape(12, 3, 3)
    assert np.abs(hard - fn[:, None, :]).max() < 1e-7  # every corner: its face normal
    soft = pkg.smooth_normals(xs, ys, zs, 180.0).reshape(12, 3, 3)
    P = np.stack([xs[:, :3], ys[:, :3], zs[:, :3]], -1)  # corners
    # normalize(+-1, +-1, +-1), on the side the stored normals point to (this cube is wound counter-clockwise seen from
    # outside, so cross(e1, e0) points inwards).  What the angle weighting is for: a corner touches one or two triangles per face
    side = np.sign((fn * (P.mean(1) - 0.5)).sum(1))
    assert (side == side[0]).all()
    want = side[0] * (2.0 * P - 1.0) / np.sqrt(3.0)
    assert np.abs(soft - want).max() < 1e-6, np.abs(soft - want).max()


def test_a_zero_area_triangle_comes_out_flat(pkg):
    T = _unit_cube()
    deg = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[1, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)  # collinear; two corners equal
    xs, ys, zs = _soa(np.concatenate([T, deg]))
    got = pkg.smooth_normals(xs, ys, zs, 180.0)
    assert np.array_equal(got[12:], np.zeros((2, 9), np.float32))
    assert np.array_equal(got[:12], pkg.smooth_normals(*_soa(T), 180.0))  # and contribute nothing to their neighbours


# ---- FBX ----------------------------------------------------------------------------------------------------------
WITH_NORMALS = [GOLDEN / "c3" / "sphere.fbx", GOLDEN / "scene_test" / "res" / "fbx" / "teapot.fbx", GOLDEN / "fbx" / "uv_sphere_normals_maya_yup_rh.fbx"]
WITHOUT_NORMALS = [GOLDEN / "fbx" / n for n in ("ball.fbx", "uv_sphere_trs.fbx", "uv_sphere_blender_zup_rh.fbx", "uv_sphere_maya_yup_rh.fbx",
                                                "uv_sphere_target_zup_lh.fbx", "uv_sphere_xup_lh.fbx")]


@pytest.mark.parametrize("path", WITH_NORMALS, ids=lambda p: p.name)
def test_fbx_normals_are_unit_and_agree_with_the_winding(pkg, path):
    """Every corner normal lies on one side of its triangle, the same for the whole file: the side of cross(e0, e1), which
    these counter-clockwise files turn outwards.  The STORED face normal is TriPost's cross(e1, e0), the opposite one, so the
    dot product with it is negative throughout (hit_finish flips the stored normal against the ray either way)."""
    T = pkg.host_scene.read_fbx(path)
    N = pkg.host_scene.read_fbx_normals(path)
    assert N.shape == T.shape and N.dtype == np.float32
    fn, ok = V.face_normals(*_soa(T))
    flat = (N == 0).all(axis=(1, 2))  # a triangle with a corner whose file normal is unusable stays flat: nine zeros
    assert not (flat & ok).any()      # (teapot.fbx: the 96 zero-area triangles at the poles of its patches, and no other)
    assert np.abs(np.linalg.norm(N[~flat].astype(np.float64), axis=2) - 1.0).max() < 1e-6
    ok = ok & ~flat
    d = (N.astype(np.float64) * fn[:, None, :]).sum(2)
    assert (-d[ok] > 0).all(), (int((-d[ok] <= 0).sum()), (-d[ok]).min())


def test_fbx_normals_go_through_the_inverse_transpose(pkg):
    v, p = fx.uv_sphere()
    axes = fx.AXIS_FIXTURES["maya_yup_rh"]
    want = fx.expected_normals(v, p, fx.FIXTURE["R"], fx.FIXTURE["S"], axes)
    path = GOLDEN / "fbx" / "uv_sphere_normals_maya_yup_rh.fbx"
    got = pkg.host_scene.read_fbx_normals(path)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-5, np.abs(got - want).max()
    # the fixture is what it says: the same triangles as its twin without normals (mirrored: the winding reverses), under a
    # scaling under which the plain transform of a normal would be wrong by far more than the bound
    assert np.array_equal(pkg.host_scene.read_fbx(path), pkg.host_scene.read_fbx(GOLDEN / "fbx" / "uv_sphere_maya_yup_rh.fbx"))
    assert np.array_equal(pkg.host_scene.read_fbx(path), fx.expected_triangles(v, p, axes=axes, **fx.FIXTURE))
    plain = fx.expected_normals(v, p, fx.FIXTURE["R"], tuple(1.0 / s for s in fx.FIXTURE["S"]), axes)
    assert np.abs(plain - want).max() > 0.1


def test_fbx_normal_mappings(pkg, tmp_path):
    """By control point (ByVertice) the same normals come out as by polygon vertex; a mapping the reader does not know
    (ByPolygon: one normal per face) is not misread as another: the mesh stays flat."""
    v, p = fx.uv_sphere()
    axes = fx.AXIS_FIXTURES["maya_yup_rh"]
    want = fx.expected_normals(v, p, fx.FIXTURE["R"], fx.FIXTURE["S"], axes)
    per_vertex = v / np.linalg.norm(v, axis=1, keepdims=True)
    fx.write(tmp_path / "by_vertex.fbx", v, p, axes=axes, normals=per_vertex, normals_mapping="ByVertice", **fx.FIXTURE)
    got = pkg.host_scene.read_fbx_normals(tmp_path / "by_vertex.fbx")
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-5
    fx.write(tmp_path / "by_polygon.fbx", v, p, axes=axes, normals=per_vertex[:len(p)], normals_mapping="ByPolygon", **fx.FIXTURE)
    assert pkg.host_scene.read_fbx_normals(tmp_path / "by_polygon.fbx").shape == (0, 3, 3)
    assert pkg.host_scene.read_fbx(tmp_path / "by_polygon.fbx").shape == (want.shape[0], 3, 3)


@pytest.mark.parametrize("path", WITHOUT_NORMALS, ids=lambda p: p.name)
def test_fbx_without_a_normal_layer_gives_an_empty_array(pkg, path):
    assert pkg.host_scene.read_fbx_normals(path).shape == (0, 3, 3)


# ---- loaders ------------------------------------------------------------------------------------------------------
def test_json_loader_fills_tri_normals(pkg):
    sc = pkg.host_scene.load_json(GOLDEN / "c3" / "c3_sphere_veranda.json")
    assert sc.tri_normals is not None and sc.tri_normals.shape == (sc.tri_count, 9)
    smooth = ~(sc.tri_normals == 0).all(1)
    assert smooth.any()
    n = sc.tri_normals[smooth].reshape(-1, 3).astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    fn, ok = V.face_normals(sc.xs, sc.ys, sc.zs)
    d = (sc.tri_normals.reshape(-1, 3, 3).astype(np.float64) * fn[:, None, :]).sum(2)
    assert (-d[smooth & ok] > 0).all()  # the instance transform carried them along with the positions (stored normal: cross(e1, e0))
    boxes = pkg.host_scene.load_json(GOLDEN / "json_scene" / "three_boxes.json")
    assert boxes.tri_normals is None   # cubes and planes carry none


def test_pbrt_loader_fills_tri_normals(pkg, tmp_path):
    (tmp_path / "n.pbrt").write_text('''
LookAt 0 -4 0  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "rgb" "integer xresolution" 32 "integer yresolution" 32
WorldBegin
AttributeBegin
  Scale 2 1 0.5
  Shape "trianglemesh" "integer indices" [0 1 2] "point3 P" [0 0 0  1 0 0  0 0 1] "normal N" [0 -1 0  0.6 -0.8 0  0 -0.8 0.6]
AttributeEnd
Shape "trianglemesh" "integer indices" [0 1 2] "point3 P" [0 1 0  1 1 0  0 1 1]
''')
    sc = pkg.host_scene.load_pbrt(tmp_path / "n.pbrt")
    assert sc.tri_normals.shape == (2, 9) and np.array_equal(sc.tri_normals[1], np.zeros(9, np.float32))
    # inverse transpose of Scale(2, 1, 0.5), then the loader's mirror in x and its corner order (0, 2, 1)
    raw = np.array([[0, -1, 0], [0.6, -0.8, 0], [0, -0.8, 0.6]]) / np.array([2.0, 1.0, 0.5])
    raw /= np.linalg.norm(raw, axis=1, keepdims=True)
    raw[:, 0] *= -1.0
    assert np.abs(sc.tri_normals[0].reshape(3, 3) - raw[[0, 2, 1]]).max() < 1e-6


def _records_hash(sc):
    h = hashlib.sha256()
    for a in (sc.xs, sc.ys, sc.zs, sc.mat_id, sc.bsdfs, sc.lights, sc.tri_uv if sc.tri_uv is not None else np.zeros(0, np.float32)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# _records_hash of what the loaders gave before tri_normals existed: taken on the parent commit (598a832, built) by running
# this function there on host_scene.load_json / load_pbrt of the same four files under tests/golden/.
PINNED = {
    "c3/c3_sphere_veranda.json": "dc201d5054d2ea1ff0d5b3a9b205e7cacb8b12f069249c0d2c045eea64358d76",
    "scene_test/scene_test.json": "7105160b63a173679e97daea87df91282cac4e7b3efad52634f4b9e270377f66",
    "json_scene/three_boxes.json": "f4672205f633eeaa1dc537f757cc15faac9dc319555b3213489010845d3d8762",
    "pbrt/cornell_box.pbrt": "9eaef1ede8b25d1864dbe67a1e2e0e93c7633aeb6e8036aa332da07f0ca1dd30",
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_packed_records_of_existing_scenes_are_unchanged(pkg, name):
    load = pkg.host_scene.load_pbrt if name.endswith(".pbrt") else pkg.host_scene.load_json
    assert _records_hash(load(GOLDEN / name)) == PINNED[name]


def test_cli_shading_normals_option():
    """--shading-normals: in the help, its value checked, `file` refused for a scene without normals, not combined with
    --motion-scene -- all before any GPU is touched."""
    import subprocess
    exe = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"
    assert exe.exists(), "run __graft_entry__.build()"
    run = lambda *a: subprocess.run([str(exe), *a], capture_output=True, text=True, timeout=60)
    h = run("-h")
    assert h.returncode == 0 and "--shading-normals <off|file|smooth[:DEG]>" in h.stdout
    for bad in ("on", "smooth:", "smooth:-1", "smooth:181", "smooth:30x", "files"):
        r = run("--shading-normals", bad)
        assert r.returncode == 1 and "invalid --shading-normals" in r.stderr, (bad, r.stderr)
    boxes = GOLDEN / "json_scene" / "three_boxes.json"
    r = run("--scene", str(boxes), "--shading-normals", "file")
    assert r.returncode == 1 and "carry no vertex normals" in r.stderr, r.stderr
    r = run("--scene", str(boxes), "--motion-scene", str(boxes), "--shading-normals", "smooth:40")
    assert r.returncode == 1 and "exclude each other" in r.stderr, r.stderr
