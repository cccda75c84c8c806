"""The shading sweep on the device: bsdf_prepare / sample_bsdf / eval_bsdf (dmt_test_bsdf_ng), sample_light / eval_light
(dmt_test_light) and the material patch (dmt_test_material) against the CPU oracle, on the cases the oracle's own
conditioning filter keeps (tests/shading_sweep.py).

Bound per record: at most h + 2 kept cases may depart, h being the number of kept cases that escape the filter under a
second set of 16 perturbations of the REFERENCE (recomputed here).  The device is one further evaluation where h is a
union over sixteen, so the bound sits an order of magnitude above the reference's per-evaluation rate -- room for FMA
contraction and the device libm -- while a systematic error fails a whole cell (hundreds of cases).  No cell may have
more than 2 % of its kept cases departing, and every output of a kept case must be finite, compared or not.

Measured on an MI355X: one departing kept case in all (light spot_wide, 1 of 441, h 2), none for the 30 BSDF records.
Material probe: 512 hits per scene, 3 and 1 of them on a quantisation boundary, no record differing.

Mutants of the device code, each library run once by hand against this sweep and against test_bsdf_prepare_sample_eval:
ax / ay swapped in ggx_aniso_lambda fails 8 records here (and 2 of the golden lattice's, gold_aniso among them); the
specular threshold at 1.1e-3 fails the two code-66 records; ns for ng in sample_ggx's reflection reject fails 20; ior
dropped from eval_ggx's refracted term for eta < 1 fails diel_inv_a03 and diel_inv_a10 -- the golden lattice passes under
these three.  invEta dropped from sample_ggx's refracted term changes nothing anywhere: every refraction is flagged delta
(bsdf.cu:531), so that term is dead code."""
import numpy as np
import pytest

import shading_sweep as S

pytestmark = pytest.mark.gpu


def _check(s, cont, flags, what):
    fail = s.failures(cont, flags)
    per_cell = {c: (int(fail[s.cell_mask(c)].sum()), int(s.kept[s.cell_mask(c)].sum())) for c in s.cells}
    print(what, "failing", int(fail.sum()), "of", int(s.kept.sum()), "kept; h", s.h, per_cell)
    if fail.any():
        i = np.flatnonzero(fail)[:4]
        cols = S.BSDF_COLS if cont.shape[1] == len(S.BSDF_COLS) else S.LIGHT_COLS
        for k in i:
            bad = ~S.within(cont[k], s.cont[k], s.rel, s.abs_)
            print("  case", int(k), s.cells[int(s.x["cell"][k])], "flags", flags[k].astype(int), "ref", s.flags[k].astype(int),
                  [(cols[j], float(cont[k, j]), float(s.cont[k, j])) for j in np.flatnonzero(bad)])
    with np.errstate(invalid="ignore"):
        assert np.isfinite(cont[s.kept]).all(), what
    assert int(fail.sum()) <= s.h + 2, (what, int(fail.sum()), s.h)
    for c, (nf, nk) in per_cell.items():
        assert nf <= 0.02 * nk, (what, c, nf, nk)


@pytest.fixture(scope="module")
def tex_records(renderer, O):
    """tex0 .. tex3 from the device's material probe; they must be the oracle's."""
    def probe(scene, tri, bu, bv, ng):
        renderer.upload_scene(scene)
        try:
            return renderer.test_material(tri, bu, bv, ng)[0]
        finally:
            renderer.upload_textures(None, None, None, None)
    dev = S.material_records(O, probe)
    ref = S.material_records(O)
    for k in ref:
        assert np.array_equal(dev[k], ref[k]), k
    return dev


@pytest.mark.parametrize("name", S.BSDF_RECORD_NAMES)
def test_bsdf_sweep(renderer, O, tex_records, name):
    s = S.bsdf_sweep(O, name, tex_records.get(name))
    cont, flags = S.device_bsdf(renderer, s.rec, s.x)
    _check(s, cont, flags, name)
    # fp16-quantised prepared terms: equal except on the rare rounding-boundary case (test_bsdf_prepare_sample_eval's bound)
    assert np.mean(cont[s.kept, 0:6] != s.cont[s.kept, 0:6]) < 0.02


@pytest.mark.parametrize("name", S.LIGHT_NAMES)
def test_light_sweep(renderer, O, name):
    s = S.light_sweep(O, name)
    cont, flags = S.device_light(renderer, s.rec, s.x)
    _check(s, cont, flags, "light " + name)


# ---- material patch --------------------------------------------------------------------------------------------------
RAMP = np.array([[0, 1, 64, 127, 128, 191, 254, 255], [1, 2, 65, 126, 129, 190, 253, 254]], np.uint8)


def _tex8(kind):
    """8 x 8 texels over the bytes 0, 1, 127, 128, 254 and 255: two ramps on alternating rows.  Gentle, so that a lookup moves
    by about an ulp when (s, t) do (a high-contrast map moves it by tens of ulps, and a fifth of all hits then sits on a
    boundary of the 16-bit alpha), and without a plateau of 255, where every lookup would be exactly 1.0 = the top code."""
    x = RAMP[np.arange(8) % 2]                    # [row, column]
    y = x.T[::-1]
    out = np.full((8, 8, 4), 255, np.uint8)
    if kind == "normal":
        out[..., 0], out[..., 1], out[..., 2] = x, y, 255 - np.minimum(x, y) // 2
    elif kind == "roughness":
        out[..., 0] = out[..., 1] = out[..., 2] = x
    else:
        out[..., 0] = out[..., 1] = out[..., 2] = y
    assert set([0, 1, 127, 128, 254, 255]) <= set(out[..., 0].ravel().tolist())
    return np.ascontiguousarray(out).reshape(-1, 4)


def _mapped_scene(O):
    """The Cornell box with 8 x 8 normal, roughness and metallic maps: an Oren-Nayar wall (roughness + normal map), a GGX
    conductor whose anisotropy 2.5 drives alpha_x into the clamp, and two fractional-metallic pairs -- one with a metallic
    map and anisotropy 0.4, one with the record's constant fraction."""
    sc = O.cornell_box(32, 32)
    rng = np.random.default_rng(11)
    nb = sc.bsdfs.shape[0]
    gold = S.GOLD
    extra = [O.make_ggx_conductor(gold[0], gold[1], 0.9, 0.3, 0.2),
             O.make_ggx_blend_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.4, 1.5, 0.2, 0.3, 0.5), O.make_ggx_conductor(gold[0], gold[1], 0.4, 0.2, 0.3),
             O.make_ggx_blend_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.0, 1.5, 0.2, 0.2, 0.35), O.make_ggx_conductor(gold[0], gold[1], 0.0, 0.2, 0.2)]
    bsdfs = np.concatenate([sc.bsdfs, np.stack(extra)])
    mat = sc.mat_id.copy()
    n = mat.shape[0]
    mat[np.arange(n) % 5 == 1] = nb          # conductor
    mat[np.arange(n) % 5 == 2] = nb + 1      # pair with a metallic map
    mat[np.arange(n) % 5 == 3] = nb + 3      # pair with a constant fraction
    mat[np.arange(n) % 5 == 4] = 0           # the Oren-Nayar wall
    out = O.Scene(sc.xs, sc.ys, sc.zs, mat, bsdfs, sc.lights, sc.inf_lights, sc.camera)
    tex = [_tex8("normal"), _tex8("roughness"), _tex8("metallic")]
    desc = np.array([[0, 8, 8], [64, 8, 8], [128, 8, 8]], np.int32)
    none, f = 0xFFFFFFFF, lambda v: int(np.float32(v).view(np.uint32))
    mt = np.full((bsdfs.shape[0], 4), none, np.uint32)
    mt[:, 3] = f(1.0)
    mt[0] = [none, 1, 0, f(1.0)]
    mt[nb] = [none, 1, 0, f(2.5)]
    mt[nb + 1] = [none, 1, 0, f(0.4)]
    mt[nb + 2] = [2, 1, 0, f(0.4)]           # the pair's second row: metallic map in the first slot
    mt[nb + 3] = [none, 1, none, f(1.7)]
    mt[nb + 4] = [none, 1, none, f(1.7)]
    uv = (rng.uniform(-0.5, 2.0, (n, 1, 2)) + rng.uniform(-0.5, 0.5, (n, 3, 2))).reshape(n, 6).astype(np.float32)  # mirror wrap included
    out.set_textures(np.concatenate(tex), desc, mt, uv)
    return out


def _hits(scene, seed, count=512):
    """random (tri, bu, bv) plus triangle corners and edges; every material of the scene gets the same share of the hits"""
    rng = np.random.default_rng(seed)
    mats = np.unique(scene.mat_id)
    tri = np.array([rng.choice(np.flatnonzero(scene.mat_id == mats[i % mats.size])) for i in range(count)], np.int32)
    bu = rng.random(count, dtype=np.float32)
    bv = (rng.random(count, dtype=np.float32) * (np.float32(1) - bu)).astype(np.float32)
    k = np.arange(count)
    corner = k < 48
    bu[corner], bv[corner] = np.float32([0, 1, 0])[k[corner] % 3], np.float32([0, 0, 1])[k[corner] % 3]
    edge = (k >= 48) & (k < 144)
    e = k[edge] % 3
    t = rng.random(int(edge.sum()), dtype=np.float32)
    bu[edge] = np.where(e == 0, t, np.where(e == 1, 0, t)).astype(np.float32)
    bv[edge] = np.where(e == 0, 0, np.where(e == 1, t, np.float32(1) - t)).astype(np.float32)
    return tri, bu, bv, S.triangle_normals(scene)[tri]


@pytest.mark.parametrize("which", ["textured_cornell", "mapped"])
def test_material_probe(renderer, O, which):
    """apply_material_textures and blend_metallic at (tri, bu, bv): the patched record(s) byte for byte, the metallic
    fraction exactly, the normal-mapped ns within the camera-direction tolerance of test_camera_rays (rel 1e-5, abs
    2e-7).  Exempt are the hits at which the ORACLE's own records or ns change when its texture lookups move by up to two
    ulps: there a lookup sits within rounding of a quantisation boundary (uint16 alpha, fp16 terms, the
    normal's 10 bits).  At most 1 % of the hits."""
    scene = S.textured_cornell(O) if which == "textured_cornell" else _mapped_scene(O)
    tri, bu, bv, ng = _hits(scene, 3 if which == "mapped" else 4)
    renderer.upload_scene(scene)
    try:
        rec, ns, rec2, mix = renderer.test_material(tri, bu, bv, ng)
    finally:
        renderer.upload_textures(None, None, None, None)
    orec, ons, orec2, omix = O.material_at_hit(scene, tri, bu, bv, ng)
    ns_close = lambda a, b: np.isclose(a, b, rtol=1e-5, atol=2e-7).all(axis=1)
    # The lookups themselves are moved: by one ulp for the filter's own rounding (the device contracts a (1 - w) + b w into
    # FMAs) and by a second for that of (s, t).  Moving (bu, bv) by an ulp instead does not do: where a barycentric is small
    # it leaves (s, t) as they were (the device differed at two such hits that it did not flag), and on the textured Cornell
    # box, whose UVs span three repeats of a checker, it moves a lookup by tens of ulps and flags 1.4 % of the hits.
    boundary = np.zeros(tri.shape[0], bool)
    for ulps in (-2, -1, 1, 2):
        r, n_, r2, _ = O.material_at_hit(scene, tri, bu, bv, ng, lookup_ulps=ulps)
        boundary |= (r != orec).any(axis=1) | (r2 != orec2).any(axis=1) | ~ns_close(n_, ons)
    types = orec.view(np.uint16).reshape(-1, 16)[:, 3]
    patched = (orec != scene.bsdfs[scene.mat_id[tri]]).any(axis=1)
    print(which, "boundary hits", int(boundary.sum()), "of", tri.shape[0], "types", np.bincount(types, minlength=5), "patched", int(patched.sum()),
          "records differing", int((rec != orec).any(axis=1).sum()), int((rec2 != orec2).any(axis=1).sum()), "mix differing", int((mix != omix).sum()),
          "ns beyond tolerance", int((~ns_close(ns, ons)).sum()))
    assert boundary.mean() <= 0.01
    assert patched.sum() > 100 and (ons != ng).any(axis=1).sum() > 100     # the maps do act on these hits
    if which == "mapped":
        assert (types == 4).sum() >= 64 and (omix != 0).sum() >= 64 and np.unique(omix).size > 16
    m = ~boundary
    assert np.isfinite(ns).all() and np.isfinite(mix).all()
    assert np.array_equal(rec[m], orec[m]) and np.array_equal(rec2[m], orec2[m])
    # the fraction: the record's constant exactly; a metallic map's bilinear lookup is not quantised, so it is compared as
    # every function-level float of test_parity_gpu is (REL = 2e-5, abs 1e-6)
    mapped_mix = scene.mat_tex[np.minimum(scene.mat_id[tri] + 1, scene.mat_tex.shape[0] - 1), 0] != 0xFFFFFFFF
    const = ~(mapped_mix & (types == 4))
    assert np.array_equal(mix[const], omix[const]) and np.allclose(mix, omix, rtol=2e-5, atol=1e-6)
    assert ns_close(ns[m], ons[m]).all()
