"""Camera projections without a GPU (dmt_set_projection): the host twin against the float64 restatement
(tests/projection_ref.py), geometry that needs no tolerance, the inverse and the round trip, the argument checks, the JSON
keys, and the size of the triangle the GPU suite puts in front of its angular cameras."""
import ctypes as C
import json
import shutil
from pathlib import Path

import numpy as np
import pytest

import lens_ref as LR
import projection_ref as PR

GOLDEN = Path(__file__).resolve().parent / "golden"
F = np.float32


@pytest.fixture(scope="module")
def cases(O):
    return PR.cases(O)


def _fwd(cam):
    return LR.camera_xf(cam)["fwd"].astype(np.float64)


# ---- 1. host twin against float64 ----------------------------------------------------------------------
def test_host_twin_against_float64(pkg, cases):
    e_host = PR.measure_e_host(pkg, [c for c, _ in cases])
    print(f"e_host = {e_host:.3e}")
    assert e_host < 1e-5  # fp32 arithmetic, not a wrong formula (a wrong one is off by 1e-2 and more)
    for cam, xy in cases:
        for kind, param in PR.MODELS:
            o, d = pkg.projection_rays(cam, kind, param, xy)
            o64, d64 = PR.rays64(cam, kind, param, xy)
            assert np.abs(d - d64).max() <= e_host and np.abs(o - o64).max() <= e_host * PR.origin_scale(cam)
            assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 1).max() <= 2.0 ** -22
            if kind != PR.ORTHOGRAPHIC:  # the camera position, exactly
                assert (o == LR.camera_fields(cam)[1].astype(F)[None, :]).all()
    # perspective: dmt_lens_rays' pinhole rays through the same film positions
    cam, _ = cases[0]
    w, h = PR.FRAMES[0]
    px, py, s = LR.cases(w, h)
    p = LR.halton_params(w, h)
    xy = np.array([LR.film_position(p, int(x), int(y), LR.halton_index(p, int(x), int(y), int(k))) for x, y, k in zip(px, py, s)], F)
    o, d = pkg.projection_rays(cam, PR.PERSPECTIVE, 0.0, xy)
    o0, d0, _ = pkg.lens_rays(cam, 0.0, 1.0, px, py, s)
    assert o.tobytes() == o0.tobytes() and d.tobytes() == d0.tobytes()


# ---- 2. geometry that needs no tolerance -----------------------------------------------------------------
def test_geometry(pkg, cases):
    for cam, xy in cases:
        w, h = LR.camera_xf(cam)["width"], LR.camera_xf(cam)["height"]
        fwd = _fwd(cam)
        up = LR.camera_xf(cam)["up"].astype(np.float64)
        centre = np.array([[w / 2, h / 2]], F)
        # the forward column, normalised once in fp32: what every model must return at the film's centre
        want = fwd.astype(F)
        inv = F(1) / np.sqrt(F(F(want[0] * want[0] + want[1] * want[1]) + want[2] * want[2]))
        for kind, param in PR.MODELS:
            _, d = pkg.projection_rays(cam, kind, param, centre)
            assert np.abs(d[0] - fwd).max() <= 2.0 ** -22, (kind, d[0], fwd)
            if kind in (PR.ORTHOGRAPHIC, PR.FISHEYE):  # no trigonometry at the centre: the column itself, bit for bit
                assert (d[0] == (want * inv).astype(F)).all()
        _, d = pkg.projection_rays(cam, PR.ORTHOGRAPHIC, 3.0, xy)
        assert (d == d[0][None, :]).all()  # all bit-equal
        top = np.stack([np.linspace(0, w, 33), np.full(33, 0.25)], 1).astype(F)
        _, d = pkg.projection_rays(cam, PR.EQUIRECT, 0.0, top)
        assert ((d.astype(np.float64) @ up) > 0).all()
        # left and right edges meet behind the camera
        _, d = pkg.projection_rays(cam, PR.EQUIRECT, 0.0, np.array([[0, h / 2], [w, h / 2]], F))
        assert np.abs(d[0] + fwd).max() <= 1e-6 and np.abs(d[1] + fwd).max() <= 1e-6
        # fisheye: a film corner makes the angle fov / 2 with dir.  theta = r s in fp32: r carries 1.5 units of 2^-24
        # (one rounding of x^2 + y^2, whose terms are exact, and the square root's), s about 5 (three products and one
        # division on the host, and the square root), their product one more: 8 units relative to theta.  The direction's
        # components then carry the sine's and cosine's error, the 3 x 3 transform's and the normalisation's, about 8 units
        # absolute.  Bound: (8 theta + 8) 2^-24.
        corners = np.array([[0, 0], [w, 0], [0, h], [w, h]], F)
        for fov in (150.0, 360.0, 20.0):
            _, d = pkg.projection_rays(cam, PR.FISHEYE, fov, corners)
            d = d.astype(np.float64)
            ang = np.arctan2(np.linalg.norm(np.cross(d, fwd), axis=1), d @ fwd)
            theta = np.radians(fov / 2)
            bound = (8 * theta + 8) * 2.0 ** -24
            print(f"fisheye {fov}: corner angle off by {np.abs(ang - theta).max():.3e} (bound {bound:.3e})")
            assert np.abs(ang - theta).max() <= bound


# ---- 3. the inverse and the round trip -------------------------------------------------------------------
def test_project_against_float64_and_round_trip(pkg, cases):
    worst = 0.0
    for cam, xy in cases:
        for kind, param in PR.MODELS:
            o, d = pkg.projection_rays(cam, kind, param, xy)
            keep = PR.away_from_singular(cam, kind, param, xy)
            assert keep.sum() > 100
            for t in (0.5, 3.0, 40.0):
                p = (o.astype(np.float64) + t * d.astype(np.float64)).astype(F)
                got, depth = pkg.projection_project(cam, kind, param, p)
                want, depth64 = PR.project64(cam, kind, param, p)
                ref, trip = np.abs(got.astype(np.float64) - want), np.abs(got.astype(np.float64) - xy)
                if kind == PR.EQUIRECT:  # the left and the right edge are one meridian: film x is taken modulo the width
                    width = LR.camera_xf(cam)["width"]
                    ref[:, 0], trip[:, 0] = np.minimum(ref[:, 0], width - ref[:, 0]), np.minimum(trip[:, 0], width - trip[:, 0])
                err_ref, err_trip = ref[keep].max(), trip[keep].max()
                worst = max(worst, err_ref, err_trip)
                assert err_ref <= 1e-3 and err_trip <= 1e-3, (kind, param, t, err_ref, err_trip)
                assert np.abs(depth - depth64).max() <= 1e-5 * max(t, 1.0)
                if kind != PR.ORTHOGRAPHIC:
                    assert np.abs(depth - t).max() <= 1e-5 * max(t, 1.0)
    print(f"largest distance to the float64 inverse / the film position: {worst:.3e} px (bound 1e-3)")


# ---- 4. arguments ----------------------------------------------------------------------------------------
def test_arguments(pkg, cases):
    lib = pkg.load_library()
    cam, xy = cases[0]
    xy = np.ascontiguousarray(xy[:4])
    o, d = np.zeros((4, 3), F), np.zeros((4, 3), F)
    pc, pxy, po, pd = (a.ctypes.data_as(C.c_void_p) for a in (cam, xy, o, d))
    dep = np.zeros(4, F)
    nan, inf = float("nan"), float("inf")
    bad = [(-1, 0.0), (4, 0.0), (PR.ORTHOGRAPHIC, 0.0), (PR.ORTHOGRAPHIC, -1.0), (PR.ORTHOGRAPHIC, nan), (PR.ORTHOGRAPHIC, inf),
           (PR.FISHEYE, 0.0), (PR.FISHEYE, -10.0), (PR.FISHEYE, 360.5), (PR.FISHEYE, nan), (PR.FISHEYE, inf)]
    for kind, param in bad:
        assert lib.dmt_projection_rays(pc, kind, C.c_float(param), 4, pxy, po, pd) == 1, (kind, param)
        assert lib.dmt_projection_project(pc, kind, C.c_float(param), 4, po, pxy, dep.ctypes.data_as(C.c_void_p)) == 1, (kind, param)
    assert lib.dmt_projection_rays(None, 0, C.c_float(0), 4, pxy, po, pd) == 1
    assert lib.dmt_projection_rays(pc, 0, C.c_float(0), -1, pxy, po, pd) == 1
    assert lib.dmt_projection_rays(pc, 0, C.c_float(0), 4, None, po, pd) == 1
    assert lib.dmt_projection_rays(pc, 0, C.c_float(0), 0, None, None, None) == 0
    assert lib.dmt_set_projection(None, 0, C.c_float(0)) != 0 and lib.dmt_projection_info(None, None, None) != 0
    # param is ignored by perspective and equirect
    for kind in (PR.PERSPECTIVE, PR.EQUIRECT):
        a = pkg.projection_rays(cam, kind, 0.0, xy)
        for param in (-3.0, nan, inf):
            b = pkg.projection_rays(cam, kind, param, xy)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(pkg.DmtError):
        pkg.projection_rays(cam, "cylindrical", 0.0, xy)
    # orthographic with param = sensor D / focal frames depth D as the perspective camera does
    _, _, _, _, focal, sensor = LR.camera_fields(cam)
    D = 3.5
    xyc = PR.film_positions(*PR.FRAMES[0])
    o, d = pkg.projection_rays(cam, PR.PERSPECTIVE, 0.0, xyc)
    p = (o.astype(np.float64) + (D / (d.astype(np.float64) @ _fwd(cam)))[:, None] * d.astype(np.float64)).astype(F)  # at depth D
    got, depth = pkg.projection_project(cam, PR.ORTHOGRAPHIC, float(sensor) * D / float(focal), p)
    want, depth_p = pkg.camera_project(cam, p)
    assert np.abs(got - want).max() <= 1e-3 and np.abs(depth - depth_p).max() <= 1e-5 * D


# ---- 5. JSON ---------------------------------------------------------------------------------------------
PACK_KEYS = ("xs", "ys", "zs", "mat_id", "bsdfs", "lights", "inf_lights", "camera")


def _arrays(s):
    return [np.asarray(getattr(s, k)).tobytes() for k in PACK_KEYS]


def test_fixtures_without_the_keys_pack_as_before(pkg):
    """tests/golden/projection/json_pack_sha256.json holds the SHA-256 of every packed array of three fixtures as the loader
    packed them before it knew the projection keys: a scene without the keys loads byte for byte as it did."""
    import hashlib
    H = pkg.host_scene
    pinned = json.loads((GOLDEN / "projection" / "json_pack_sha256.json").read_text())
    assert len(pinned) == 3
    for rel, want in pinned.items():
        s = H.load_json(GOLDEN / rel)
        got = {k: hashlib.sha256(np.ascontiguousarray(getattr(s, k)).tobytes()).hexdigest() for k in PACK_KEYS}
        assert got == {k: want[k] for k in PACK_KEYS}, rel
        assert list(s.lens) == want["lens"] and s.projection == (0, 0.0)


def test_json_keys(pkg, tmp_path):
    H = pkg.host_scene
    shutil.copytree(GOLDEN / "json_scene", tmp_path / "s")
    src = tmp_path / "s" / "three_boxes.json"
    plain = H.load_json(GOLDEN / "json_scene" / "three_boxes.json")
    assert plain.projection == (0, 0.0) and H.load_json(GOLDEN / "lens" / "lens_boxes.json").projection == (0, 0.0)
    assert H.cornell_box().projection == (0, 0.0)
    base = json.loads(src.read_text())

    def load(**keys):
        d = json.loads(json.dumps(base))
        d["camera"].update(keys)
        (tmp_path / "s" / "p.json").write_text(json.dumps(d))
        return H.load_json(tmp_path / "s" / "p.json")

    for keys, want in ((dict(projection="orthographic", orthoHeight=2.5), (PR.ORTHOGRAPHIC, 2.5)), (dict(projection="equirect"), (PR.EQUIRECT, 0.0)),
                       (dict(projection="fisheye", fisheyeFov=180), (PR.FISHEYE, 180.0))):
        s = load(**keys)
        assert s.projection == want
        assert _arrays(s) == _arrays(plain)  # the keys change nothing else the loader packs
    for keys in (dict(projection="cylindrical"), dict(projection=2), dict(projection="orthographic"), dict(projection="orthographic", orthoHeight=0),
                 dict(projection="orthographic", orthoHeight="tall"), dict(orthoHeight=2.0), dict(projection="equirect", orthoHeight=2.0),
                 dict(projection="fisheye"), dict(projection="fisheye", fisheyeFov=0), dict(projection="fisheye", fisheyeFov=361),
                 dict(projection="equirect", fisheyeFov=90), dict(projection="equirect", lensRadius=0.1, focusDistance=2.0)):
        with pytest.raises(ValueError):
            load(**keys)
    # the file as it is packs as before: the same bytes through a copy
    assert _arrays(H.load_json(src)) == _arrays(plain)


def test_abi_and_binding(pkg):
    from cuda_optix_pathtracing_amd import binding
    lib = pkg.load_library()
    for name in ("dmt_set_projection", "dmt_projection_info", "dmt_projection_rays", "dmt_projection_project"):
        assert name in binding.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert (pkg.PROJECTION_PERSPECTIVE, pkg.PROJECTION_ORTHOGRAPHIC, pkg.PROJECTION_EQUIRECT, pkg.PROJECTION_FISHEYE) == (0, 1, 2, 3)
    assert pkg.PROJECTION_KINDS == {"perspective": 0, "orthographic": 1, "equirect": 2, "fisheye": 3}


# ---- 9 (its CPU part). the triangle in front of the angular cameras stays under the cap ------------------
def test_env_scene_triangle_share():
    for kind, param in ((PR.EQUIRECT, 0.0), (PR.FISHEYE, 180.0)):
        cam, xy = PR.env_scene_samples()
        o, d = PR.rays64(cam, kind, param, xy)
        share = PR.hits_triangle64(o, d, PR.ENV_TRIANGLE.astype(np.float64)).mean()
        print(f"kind {kind}: {100 * share:.3f} % of the float64 rays meet the triangle (cap 1 %)")
        assert share <= 0.005  # half the cap: the fp32 rays may move a sample across an edge
