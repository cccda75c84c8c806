"""Case generator and conditioning filter of the shading sweep (tests/test_shading_sweep.py on the CPU,
tests/test_shading_sweep_gpu.py on the device).

The sweep drives bsdf_prepare / sample_bsdf / eval_bsdf and sample_light / eval_light through the branches a random
lattice never reaches: the specular switch, dielectric variants, tangent-frame switches, a shading normal that differs
from the geometric one, boundary draws.  Those inputs are ill-conditioned in ANY fp32 implementation (at grazing wo a
1-ulp change of wo moves a refracted f by tens of per cent), so the REFERENCE ALONE decides which cases are comparable:

  * the oracle is evaluated at the exact inputs and at 16 copies in which every component of the direction and position
    inputs (ns, ng, wo, wi; position and normal for lights) moves by a seeded random 0, +-1 or +-2 ulp; u2 and uc stay;
  * a case is excluded when a discrete output (delta, refract, pdf != 0, eval pdf != 0, valid, finiteness) differs in any
    copy, when the spread of a continuous output over the copies exceeds a quarter of that output's tolerance, or when
    the oracle's own output is not finite;
  * moved inputs cannot show what internal rounding alone decides, so copy j also moves cos_NH, on its way into the
    distribution term D, and the VNDF's Nh.z by COS_NH_ULPS[j % 5] ulps inside the oracle, and one more copy of the first
    set is the reference's FMA-contracted build (oracle/libdmt_oracle_fma.so) at the exact inputs;
  * a cell that keeps fewer than 32 cases is not compared at all;
  * the tolerances are those of test_bsdf_prepare_sample_eval and test_light_sample_eval (TOL_BSDF / light_tolerances).

The device is never consulted.  `h` is the number of KEPT cases that leave tolerance or flip a flag under a second,
independent set of 16 copies: the reference's own rate of escaping the filter, which bounds what one further evaluation
(the device) may do.

Per-output rules (commented where they are applied): the case stays, the named outputs are not compared, and every
output of the device must still be finite.
  rim draw      u2 on the rim of the unit disk (rim_draw): what is taken from sqrt(1 - r^2) -- the sampled wi, f, pdf, the
                lobe choice, an evaluation at that wi; a light's distance, pLight and Le, and its direction and pdf when it
                is sampled from inside.  Nothing for a specular record, which never reads u2
  sharp lobe    isotropic GGX where one ulp of cos_NH moves D by more than an output's whole tolerance: the reflected
                sample's pdf (alpha^2 < 2.4e-3: codes 66 and alpha 0.02), the evaluations (alpha^2 < 1.2e-4: codes 66)
  eta == 1      F is rounding noise around 0: evaluations on the reflection side, pdf and f of a reflected sample
Per-case rule (the reference is NaN by construction): eta == 1 evaluated at wi == -wo, a zero half vector.

Ranges chosen:
  generic      wo . ns uniform in [0.05, 1], ns == ng
  wo_eq_ns     wo == ns bit for bit
  wo_near_ns   angle(wo, ns) log-uniform in [1e-4, 1e-2]
  grazing      wo . ns uniform in [0.01, 0.05]
  ns_axis      ns one of +-x, +-y, +-z exactly
  ns_x999      |ns.x| uniform in [0.9985, 0.9995] (both sides of tangent_from_phi's 0.999 switch)
  tilt         ns tilted from ng by up to 60 degrees, wo . ng in [0.05, 1]
  tilt_below   ns tilted by 20..60 degrees, wo . ns <= 0 < wo . ng
  wo_below_ng  wo . ng uniform in [-1, 0]
  boundary     generic directions; u2.x, u2.y and uc each one of {0, 0.5, 1 - 2^-24, random}, never all three random (512 cases)
Eval direction by case index mod 3: a random unit wi; the mirror of wo about ns; the wi the oracle's own sample returned.
A case is one input tuple with ALL its compared outputs (prepared terms, sample, eval): one ill-conditioned output drops it.

Measured (python tests/shading_sweep.py): kept fraction per record, its lowest cell, h / kept; cells hold 256 cases.
FLOOR_MISSES lists the floors the reference cannot meet (the alpha 0.02 records' 60 %; tilt_below of the sharp lobes).
  oren_r0            kept 0.999  lowest cell generic      0.996  h  0 / 2814
  oren_r03           kept 0.992  lowest cell grazing      0.938  h  0 / 2794
  oren_rpi2          kept 0.989  lowest cell grazing      0.887  h  0 / 2786
  lambert            kept 1.000  lowest cell tilt         0.996  h  0 / 2815
  cond_c65           kept 0.997  lowest cell tilt_below   0.992  h  0 / 2808
  diel_c65           kept 0.998  lowest cell grazing      0.988  h  0 / 2810
  cond_c66           kept 0.893  lowest cell tilt_below   0.000  h  0 / 2515
  diel_c66           kept 0.891  lowest cell tilt_below   0.000  h  0 / 2509
  cond_a002          kept 0.460  lowest cell tilt_below   0.145  h  0 / 1295
  diel_a002          kept 0.552  lowest cell tilt_below   0.191  h  1 / 1554
  cond_a03           kept 0.940  lowest cell wo_near_ns   0.555  h  0 / 2648
  diel_a03           kept 0.949  lowest cell wo_near_ns   0.559  h  0 / 2672
  cond_a10           kept 0.922  lowest cell wo_near_ns   0.281  h  0 / 2596
  diel_a10           kept 0.931  lowest cell wo_near_ns   0.273  h  0 / 2622
  cond_aniso_lo_hi   kept 0.949  lowest cell wo_near_ns   0.688  h  0 / 2671
  diel_aniso_lo_hi   kept 0.964  lowest cell wo_near_ns   0.688  h  0 / 2714
  cond_aniso_hi_lo   kept 0.941  lowest cell wo_near_ns   0.570  h  0 / 2651
  diel_aniso_hi_lo   kept 0.965  lowest cell wo_near_ns   0.711  h  0 / 2717
  cond_half_spec     kept 0.855  lowest cell grazing      0.703  h  0 / 2407
  diel_half_spec     kept 0.939  lowest cell wo_near_ns   0.816  h  0 / 2645
  diel_inv_a03       kept 0.919  lowest cell wo_near_ns   0.539  h  0 / 2587
  diel_inv_a10       kept 0.891  lowest cell wo_near_ns   0.262  h  0 / 2509
  diel_inv_c65       kept 0.991  lowest cell tilt         0.965  h  0 / 2790
  diel_eta1_a03      kept 0.927  lowest cell wo_near_ns   0.543  h  1 / 2611
  diel_no_refl       kept 0.945  lowest cell wo_near_ns   0.586  h  0 / 2662
  diel_no_trans      kept 0.928  lowest cell wo_near_ns   0.520  h  0 / 2614
  tex0               kept 0.978  lowest cell grazing      0.820  h  0 / 2754
  tex1               kept 0.976  lowest cell grazing      0.789  h  0 / 2748
  tex2               kept 0.935  lowest cell wo_near_ns   0.516  h  0 / 2634
  tex3               kept 0.938  lowest cell wo_near_ns   0.469  h  0 / 2641
  light point_tiny      kept 1.000  lowest cell outside      1.000  h  0 / 512
  light point_medium    kept 0.994  lowest cell boundary_u2  0.992  h  0 / 509
  light point_enclosing kept 1.000  lowest cell inside_hadT0 1.000  h  0 / 768
  light spot_spread     kept 0.977  lowest cell boundary_u2  0.961  h  0 / 750
  light spot_wide       kept 0.861  lowest cell boundary_u2  0.723  h  2 / 441
  light spot_inside     kept 0.952  lowest cell inside_hadT1 0.922  h  0 / 731
  light spot_tiny       kept 1.000  lowest cell outside      1.000  h  0 / 512
  light dir_omc0        kept 1.000  lowest cell anywhere     1.000  h  0 / 512
  light dir_omc001      kept 1.000  lowest cell anywhere     1.000  h  0 / 512
  light env             kept 1.000  lowest cell anywhere     1.000  h  0 / 512
"""
import functools

import numpy as np

N_CELL = 256
N_COPIES = 16
MIN_CELL = 32
SEED_FILTER, SEED_HOLDOUT = 0x51F7, 0xA11CE
ONE_M = np.float32(1.0 - 2.0 ** -24)
BOUNDARY = np.array([0.0, 0.5, ONE_M], np.float32)

BSDF_CELLS = ["generic", "wo_eq_ns", "wo_near_ns", "grazing", "ns_axis", "ns_x999", "tilt", "tilt_below", "wo_below_ng",
              "boundary"]
# cells whose inputs are degenerate on purpose (the oracle may answer with a non-finite value there)
BSDF_DEGENERATE = {"tilt_below"}
GRAZING_COS = (0.01, 0.05)

# (rel, abs) per continuous output, from test_bsdf_prepare_sample_eval: prepared weight / multi-scatter halves within one fp16
# ulp, energy scale 1e-5; sample wi 1e-4 / 2e-6, f 2e-3 / 1e-6, pdf 1e-4 / 1e-7, eta REL; eval (f, pdf) 2e-3 / 1e-6
BSDF_COLS = ["weight"] * 3 + ["ms"] * 3 + ["escale"] + ["wi"] * 3 + ["f"] * 3 + ["pdf", "eta"] + ["eval_f"] * 3 + ["eval_pdf"]
TOL_BSDF = {"weight": (1.1e-3, 1e-6), "ms": (1.1e-3, 1e-7), "escale": (1e-5, 1e-6), "wi": (1e-4, 2e-6), "f": (2e-3, 1e-6),
            "pdf": (1e-4, 1e-7), "eta": (2e-5, 1e-6), "eval_f": (2e-3, 1e-6), "eval_pdf": (2e-3, 1e-6)}
BSDF_FLAGS = ["delta", "refract", "pdf_nonzero", "eval_pdf_nonzero"]

LIGHT_COLS = ["pLight"] * 3 + ["direction"] * 3 + ["pdf", "distance", "factor"] + ["Le"] * 3
LIGHT_FLAGS = ["delta", "valid", "pdf_nonzero"]


def light_tolerances(effectively_delta):
    """test_light_sample_eval's bounds; its looser distance bound belongs to lights with radius << distance, whose
    distance = d cos - sqrt(r^2 - d^2 + d^2 cos^2) cancels catastrophically (light.cu:56-59)."""
    rel_d = 5e-3 if effectively_delta else 1e-4
    return {"pLight": (rel_d, 1e-5), "direction": (1e-4, 2e-6), "pdf": (1e-4, 1e-6), "distance": (rel_d, 1e-6),
            "factor": (2e-5, 1e-6), "Le": (2 * rel_d, 1e-7)}


def _tol_arrays(cols, table):
    return (np.array([table[c][0] for c in cols], np.float64), np.array([table[c][1] for c in cols], np.float64))


# ---- small vector helpers (float64 construction, float32 results) ---------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _frame(n):
    """two unit vectors orthogonal to each unit row of n"""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t = _unit(np.cross(a, n))
    return t, np.cross(n, t)


def _around(n, cos, phi):
    t, b = _frame(n)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    return _unit(cos[:, None] * n + sin[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * b))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _perturb(a, rng):
    """every component moved by 0, +-1 or +-2 ulp"""
    k = rng.integers(-2, 3, a.shape).astype(np.float32)
    return (a + k * np.spacing(np.abs(a))).astype(np.float32)


def _boundary_draws(u):
    """Row j of u [n, k] (k = 2: u2; k = 3: u2 and uc): every component takes 0, 0.5 or 1 - 2^-24 or keeps its random value,
    cycling through all 4^k combinations but the all-random one."""
    n, k = u.shape
    j = np.arange(n) % (4 ** k - 1)
    out = u.copy()
    for c in range(k):
        d = (j // 4 ** c) % 4
        out[:, c] = np.where(d < 3, BOUNDARY[np.minimum(d, 2)], u[:, c])
    return np.ascontiguousarray(out, np.float32)


def rim_draw(u2):
    """A draw on the rim of the unit disk.  sampleUniformDisk (sampling.cu:135-155) maps u2 to a radius
    max(|2 u.x - 1|, |2 u.y - 1|), and its users take sqrt(1 - r^2) of it: the hemisphere's cosine, the VNDF's
    sqrt(1 - t.x^2), and, through the cone's tangent ray, the distance to a light's sphere.  With 1 - r^2 < 1.2e-3 one ulp of
    r^2 (6e-8) moves that difference by more than a quarter of the tightest tolerance (2e-4 / 4 relative on a squared quantity),
    and at u = 0 or 1 - 2^-24 it is 0 or 2.4e-7 depending on how 2 u - 1 and r^2 were rounded.  The outputs taken from that
    square root are not compared at such a draw (see _bsdf_sweep_of, light_sweep); everything else is."""
    a = np.abs(2.0 * u2.astype(np.float64) - 1.0).max(axis=1)
    return 1.0 - a * a < 1.2e-3


# Floors of the sweep that the reference cannot meet, and why: (record, cell) for a cell's 25 %, (record, None) for the
# record's 60 %.  tests/test_shading_sweep.py asserts every other floor, and that these are indeed missed.
FLOOR_MISSES = {
    ("cond_c66", "tilt_below"): "alpha 1e-3 seen from below the shading horizon: sample_ggx_vndf clamps the stretched normal's z at 0 and "
                                "renormalises (alpha x, alpha y, max(0, z)), a vector of rounding size; wi turns by per cents per ulp",
    ("diel_c66", "tilt_below"): "as cond_c66",
    ("cond_a002", "tilt_below"): "as cond_c66, alpha 0.02",
    ("diel_a002", "tilt_below"): "as cond_c66, alpha 0.02",
    ("cond_a002", None): "alpha 0.02: an ulp of cos_NH moves an on-lobe evaluation by 6e-4 against a quarter tolerance of 5e-4, so "
                         "the cases evaluated at the mirror direction and at the own sample (two thirds) mostly drop",
    ("diel_a002", None): "as cond_a002",
}


# ---- BSDF records ----------------------------------------------------------------------------------------------------
def _alpha(code):
    """an alpha that the packers' truncating uint16 quantisation stores as `code`"""
    return (code + 0.5) / 65535.0


GOLD = ([0.18299, 0.42108, 1.37340], [3.42420, 2.34590, 1.77040])
# name -> (alpha_x, alpha_y, phi0)
GGX_ALPHAS = {
    "c65": (_alpha(65), _alpha(65), 0.0),        # the last code below the 1e-3 specular switch ...
    "c66": (_alpha(66), _alpha(66), 0.0),        # ... and the first above it
    "a002": (0.02, 0.02, 0.0),
    "a03": (0.3, 0.3, 0.0),
    "a10": (1.0, 1.0, 0.0),
    "aniso_lo_hi": (0.05, 1.0, 0.7),
    "aniso_hi_lo": (1.0, 0.05, 2.1),
    "half_spec": (5e-4, 0.5, 1.3),               # one alpha below the switch, the other above
}
MATERIAL_HITS = 4  # records taken from the material probe on the textured Cornell box


def plain_bsdf_records(O):
    recs = {
        "oren_r0": O.make_oren_nayar([1.0, 0.5, 0.25], 0.0),
        "oren_r03": O.make_oren_nayar([0.25, 1.0, 0.5], 0.3),
        "oren_rpi2": O.make_oren_nayar([0.5, 0.25, 1.0], float(np.pi / 2)),
        "lambert": O.make_lambert(),
    }
    for tag, (ax, ay, phi0) in GGX_ALPHAS.items():
        recs[f"cond_{tag}"] = O.make_ggx_conductor(GOLD[0], GOLD[1], phi0, ax, ay)
        recs[f"diel_{tag}"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], phi0, 1.5, ax, ay)
    recs["diel_inv_a03"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.0, 1.0 / 1.5, 0.3, 0.3)
    recs["diel_inv_a10"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.0, 1.0 / 1.5, 1.0, 1.0)
    recs["diel_inv_c65"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.0, 1.0 / 1.5, _alpha(65), _alpha(65))
    recs["diel_eta1_a03"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.9, 0.8, 0.7], 0.0, 1.0, 0.3, 0.3)
    recs["diel_no_refl"] = O.make_ggx_dielectric([0.0, 0.0, 0.0], [0.9, 0.8, 0.7], 0.0, 1.5, 0.3, 0.3)
    recs["diel_no_trans"] = O.make_ggx_dielectric([0.5, 0.6, 0.7], [0.0, 0.0, 0.0], 0.0, 1.5, 0.3, 0.3)
    for tag in ("c65", "c66"):
        code = int(tag[1:])
        for kind in ("cond", "diel"):
            h = recs[f"{kind}_{tag}"].view(np.uint16)
            assert h[7] == code and h[8] == code, (kind, tag, h[7], h[8])
    return recs


BSDF_RECORD_NAMES = (["oren_r0", "oren_r03", "oren_rpi2", "lambert"]
                     + [f"{k}_{t}" for t in GGX_ALPHAS for k in ("cond", "diel")]
                     + ["diel_inv_a03", "diel_inv_a10", "diel_inv_c65", "diel_eta1_a03", "diel_no_refl", "diel_no_trans"]
                     + [f"tex{i}" for i in range(MATERIAL_HITS)])


def textured_cornell(O):
    """The textured Cornell box of the film tests: albedo, roughness (anisotropy 0.6 on the dielectric) and normal maps."""
    from test_parity_gpu import _textured_cornell
    return _textured_cornell(O, None, 32)


def triangle_normals(scene):
    """normalize(cross(e1, e0)) per triangle in float32, the winding the intersection routine uses"""
    p = np.stack([scene.xs[:, :3], scene.ys[:, :3], scene.zs[:, :3]], axis=-1).astype(np.float32)  # [tri, vertex, xyz]
    e0, e1 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.cross(e1, e0).astype(np.float32)
    return (n / np.sqrt((n * n).sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)


def material_hits(scene):
    """(tri, bu, bv, ng) of MATERIAL_HITS hits: two on the textured Oren-Nayar material 0, two on the GGX dielectric 1"""
    ng = triangle_normals(scene)
    tri = []
    for mat in (0, 1):
        idx = np.flatnonzero(scene.mat_id == mat)
        assert idx.size >= 1
        tri += [int(idx[0]), int(idx[-1])]
    tri = np.array(tri, np.int32)
    bu = np.array([0.21, 0.55, 0.13, 0.40], np.float32)
    bv = np.array([0.33, 0.20, 0.62, 0.45], np.float32)
    return tri, bu, bv, ng[tri]


def material_records(O, probe=None):
    """tex0 .. tex3: records after the texture patch.  `probe(scene, tri, bu, bv, ng)` returns the patched records; the
    default is the oracle's, the GPU test passes the device probe (and checks that both agree)."""
    scene = textured_cornell(O)
    tri, bu, bv, ng = material_hits(scene)
    recs = (probe or (lambda sc, *a: O.material_at_hit(sc, *a)[0]))(scene, tri, bu, bv, ng)
    return {f"tex{i}": np.ascontiguousarray(recs[i], np.uint8).copy() for i in range(MATERIAL_HITS)}


# ---- BSDF cases ----------------------------------------------------------------------------------------------------
def bsdf_inputs(seed, n=N_CELL):
    """dict(ns, ng, wo, u2, uc, wi, kind, cell): len(BSDF_CELLS) cells of n cases.  wi is filled for eval kinds 0
    (random) and 1 (mirror); kind 2 (the oracle's sampled wi) is filled by bsdf_sweep."""
    rng = np.random.default_rng(seed)
    ns_l, ng_l, wo_l = [], [], []

    def generic_wo(nrm, lo=0.05, hi=1.0):
        return _around(nrm, rng.uniform(lo, hi, n), rng.uniform(0, 2 * np.pi, n))

    order = BSDF_CELLS + ["boundary"]          # the boundary cell twice over: 27 values x draws want their 32 kept cases each
    for cell in order:
        ns = _sphere(rng, n)
        ng = None
        if cell in ("generic", "boundary"):
            wo = generic_wo(ns)
        elif cell == "wo_eq_ns":
            wo = None
        elif cell == "wo_near_ns":
            ang = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), n))
            wo = _around(ns, np.cos(ang), rng.uniform(0, 2 * np.pi, n))
        elif cell == "grazing":
            wo = generic_wo(ns, *GRAZING_COS)
        elif cell == "ns_axis":
            ns = np.zeros((n, 3))
            ns[np.arange(n), np.arange(n) % 3] = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
            wo = generic_wo(ns)
        elif cell == "ns_x999":
            x = rng.uniform(0.9985, 0.9995, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
            phi = rng.uniform(0, 2 * np.pi, n)
            r = np.sqrt(1 - x * x)
            ns = np.stack([x, r * np.cos(phi), r * np.sin(phi)], -1)
            wo = generic_wo(ns)
        elif cell == "tilt":
            ng = ns
            ns = _around(ng, np.cos(np.radians(rng.uniform(0, 60, n))), rng.uniform(0, 2 * np.pi, n))
            wo = generic_wo(ng)
        elif cell == "tilt_below":
            ng = ns
            t, b = _frame(ng)
            az = rng.uniform(0, 2 * np.pi, n)
            a = np.cos(az)[:, None] * t + np.sin(az)[:, None] * b           # tilt direction
            a2 = np.cross(ng, a)
            tilt = np.radians(rng.uniform(20, 60, n))
            ns = _unit(np.cos(tilt)[:, None] * ng + np.sin(tilt)[:, None] * a)
            # wo leans away from the tilt: angle(wo, ng) in (90 - tilt, 90) degrees, so that tilt + angle > 90
            th = np.radians(90) - tilt * rng.uniform(0.05, 0.9, n)
            psi = np.radians(rng.uniform(-15, 15, n))
            wo = _unit(np.cos(th)[:, None] * ng - np.sin(th)[:, None] * (np.cos(psi)[:, None] * a + np.sin(psi)[:, None] * a2))
        elif cell == "wo_below_ng":
            wo = generic_wo(ns, -1.0, 0.0)
        else:
            raise AssertionError(cell)
        ns32 = _f32(ns)
        ns_l.append(ns32)
        ng_l.append(ns32 if ng is None else _f32(ng))
        wo_l.append(ns32.copy() if wo is None else _f32(wo))
    ns, ng, wo = np.concatenate(ns_l), np.concatenate(ng_l), np.concatenate(wo_l)
    total = ns.shape[0]
    cell = np.repeat(np.array([BSDF_CELLS.index(c) for c in order], np.int32), n)
    u2 = rng.random((total, 2), dtype=np.float32)
    uc = rng.random(total, dtype=np.float32)
    bd = np.flatnonzero(cell == BSDF_CELLS.index("boundary"))
    u2[bd, 0], u2[bd, 1], uc[bd] = _boundary_draws(np.stack([u2[bd, 0], u2[bd, 1], uc[bd]], axis=1)).T
    kind = (np.arange(total) % 3).astype(np.int32)
    wi = _f32(_sphere(rng, total))
    d = (wo * ns).sum(axis=1, keepdims=True, dtype=np.float32)
    mirror = (np.float32(2) * d * ns - wo).astype(np.float32)
    wi[kind >= 1] = mirror[kind >= 1]
    # the cells' defining properties, in the float32 values the kernels see
    c = lambda name: cell == BSDF_CELLS.index(name)
    dns, dng = (wo * ns).sum(1, dtype=np.float32), (wo * ng).sum(1, dtype=np.float32)
    assert np.array_equal(wo[c("wo_eq_ns")], ns[c("wo_eq_ns")])
    assert (dns[c("tilt_below")] <= 0).all() and (dng[c("tilt_below")] > 0).all()
    assert (dng[c("wo_below_ng")] <= 0).all()
    x9 = np.abs(ns[c("ns_x999"), 0])
    assert (x9 >= 0.999).sum() >= 64 and (x9 < 0.999).sum() >= 64
    return dict(ns=ns, ng=ng, wo=wo, u2=u2, uc=uc, wi=wi, kind=kind, cell=cell)


def _decode_prepared(rec32):
    n = rec32.shape[0]
    h = rec32.view(np.uint16).reshape(n, 16)
    f = rec32.view(np.float32).reshape(n, 8)
    return (h[:, 0:3].view(np.float16).astype(np.float32), h[:, 7:10].view(np.float16).astype(np.float32), f[:, 2].copy())


def _bsdf_pack(btype, weight, ms, escale, samp, ev):
    """(continuous [n, 19], flags [n, 5]) in BSDF_COLS / BSDF_FLAGS order; the last flag is finiteness"""
    n = samp.shape[0]
    cont = np.zeros((n, len(BSDF_COLS)), np.float32)
    cont[:, 0:3] = weight
    if btype == 0:
        cont[:, 3:6] = ms
    if btype in (1, 2):
        cont[:, 6] = escale
    cont[:, 7:15] = samp[:, 0:8]
    cont[:, 15:19] = ev
    with np.errstate(invalid="ignore"):
        flags = np.stack([samp[:, 8] != 0, samp[:, 9] != 0, samp[:, 6] != 0, ev[:, 3] != 0, np.isfinite(cont).all(axis=1)], axis=1)
    return cont, flags


def bsdf_type(rec):
    return int(np.ascontiguousarray(rec, np.uint8).view(np.uint16)[3])


def ggx_alphas(rec):
    """(alpha_x, alpha_y) of a GGX record, None otherwise"""
    if bsdf_type(rec) not in (1, 2):
        return None
    h = np.ascontiguousarray(rec, np.uint8).view(np.uint16)
    return h[7] / 65535.0, h[8] / 65535.0


def d_ulp_sensitivity(rec):
    """Relative change of the isotropic D = alpha^2 / (pi (1 - c^2 + alpha^2 c^2)^2) at the lobe's centre when c = cos_NH
    moves by one fp32 ulp (6e-8): 2 * 1.2e-7 / alpha^2 (bsdf.cu:366-372).  0 for records without that term."""
    a = ggx_alphas(rec)
    if a is None or a[0] != a[1] or a[0] < 1e-3:
        return 0.0
    return 2.4e-7 / (a[0] * a[1])


def _cols(*names):
    return np.isin(BSDF_COLS, names)


def oracle_bsdf(O, rec, x, contracted=False, cos_nh_ulps=0):
    prepared, samp, ev = O.bsdf_cases_ng(rec, x["ns"], x["ng"], x["wo"], x["u2"], x["uc"], x["wi"], contracted, cos_nh_ulps)
    return _bsdf_pack(bsdf_type(rec), *_decode_prepared(prepared), samp, ev)


def device_bsdf(renderer, rec, x):
    prep, samp, ev = renderer.test_bsdf_ng(rec, x["ns"], x["ng"], x["wo"], x["u2"], x["uc"], x["wi"])
    return _bsdf_pack(bsdf_type(rec), prep[:, 0:3], prep[:, 3:6], prep[:, 6], samp, ev)


# ---- the filter ------------------------------------------------------------------------------------------------------
def within(a, ref, rel, abs_):
    """per component: |a - ref| <= abs + rel |ref| (False where either is not finite)"""
    with np.errstate(invalid="ignore", over="ignore"):
        a64, r64 = a.astype(np.float64), ref.astype(np.float64)
        return np.abs(a64 - r64) <= abs_ + rel * np.abs(r64)


COS_NH_ULPS = (-2, -1, 0, 1, 2)


def condition(evaluate, x, keys, rel, abs_, cmp_cont, cmp_flags, contracted=None, internal=False):
    """Runs the reference at x and at two sets of N_COPIES perturbed copies.  Returns (cont, flags, kept, escaped):
    `kept` marks the comparable cases by the first set, `escaped` the kept cases that leave tolerance or flip a flag
    under the second.  Only the outputs marked in cmp_cont / cmp_flags [case, output] take part (the explicit per-output
    rules); the oracle's own answer must be finite in all of them.
    Moved inputs cannot show what internal rounding alone decides, so, besides its moved inputs,
      * copy j evaluates with cos_NH moved by COS_NH_ULPS[j % 5] ulps inside D (`internal`; BSDFs), and
      * `contracted(x)`, the reference's FMA-contracted build at the exact inputs, is one more copy of the first set."""
    cont, flags = evaluate(x, 0)
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(cont).all(axis=1)
    base = np.where(np.isfinite(cont), cont, 0).astype(np.float64)
    full = abs_ + rel * np.abs(base)
    quarter = 0.25 * full

    def copies(seed):
        rng = np.random.default_rng(seed)
        for j in range(N_COPIES):
            y = dict(x)
            for k in keys:
                y[k] = _perturb(x[k], rng)
            yield evaluate(y, COS_NH_ULPS[j % 5] if internal else 0)

    kept = finite.copy()
    lo, hi = base.copy(), base.copy()
    first = list(copies(SEED_FILTER)) + ([contracted(x)] if contracted is not None else [])
    for c, f in first:
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(c).all(axis=1)
        kept &= ok & ((f == flags) | ~cmp_flags).all(axis=1)
        c = np.where(np.isfinite(c), c, 0).astype(np.float64)
        lo, hi = np.minimum(lo, c), np.maximum(hi, c)
    kept &= (((hi - lo) <= quarter) | ~cmp_cont).all(axis=1)
    escaped = np.zeros_like(kept)
    for c, f in copies(SEED_HOLDOUT):
        with np.errstate(invalid="ignore"):
            bad = ~np.isfinite(c).all(axis=1) | ((f != flags) & cmp_flags).any(axis=1)
            bad |= (~(np.abs(np.where(np.isfinite(c), c, 0).astype(np.float64) - base) <= full) & cmp_cont).any(axis=1)
        escaped |= bad
    escaped &= kept
    return cont, flags, kept, escaped


class Sweep:
    """one record's cases, the oracle's outputs, which outputs are compared, the kept mask and the hold-out escapes"""

    def __init__(self, rec, x, cells, cont, flags, kept, escaped, rel, abs_, cmp_cont, cmp_flags):
        self.rec, self.x, self.cells = rec, x, cells
        self.cont, self.flags, self.kept, self.escaped = cont, flags, kept, escaped
        self.rel, self.abs_, self.cmp_cont, self.cmp_flags = rel, abs_, cmp_cont, cmp_flags
        # A cell of which the filter keeps fewer than MIN_CELL cases is not compared at all: below the count at which a branch
        # counts as reached, the survivors are the cases whose rounding happened to agree in every copy, not comparable ones.
        for c in range(len(cells)):
            m = x["cell"] == c
            if (kept & m).sum() < MIN_CELL:
                kept[m] = False
                escaped[m] = False

    @property
    def h(self):
        return int(self.escaped.sum())

    def cell_mask(self, name):
        return self.x["cell"] == self.cells.index(name)

    def keep_rates(self):
        return {c: float(self.kept[self.cell_mask(c)].mean()) for c in self.cells}

    def failures(self, cont, flags):
        """per kept case: does the implementation under test depart (any output non-finite, a compared flag differs, or a
        compared continuous output out of tolerance)"""
        with np.errstate(invalid="ignore"):
            bad = ~np.isfinite(cont).all(axis=1) | ((flags != self.flags) & self.cmp_flags).any(axis=1)
        bad |= (~within(cont, self.cont, self.rel, self.abs_) & self.cmp_cont).any(axis=1)
        return bad & self.kept


_BSDF_TOL = _tol_arrays(BSDF_COLS, TOL_BSDF)


def _bsdf_sweep_of(O, rec, seed, n):
    x = bsdf_inputs(seed, n)
    # eval kind 2: the wi of the oracle's own sample (on-lobe for reflection and refraction alike); the mirror direction
    # stays where the sample returned nothing
    _, samp, _ = O.bsdf_cases_ng(rec, x["ns"], x["ng"], x["wo"], x["u2"], x["uc"], x["wi"])
    own = (x["kind"] == 2) & (samp[:, 0:3] != 0).any(axis=1) & np.isfinite(samp[:, 0:3]).all(axis=1)
    x["wi"] = x["wi"].copy()
    x["wi"][own] = samp[own, 0:3]
    rel, abs_ = _BSDF_TOL
    total = x["ns"].shape[0]
    cmp_cont = np.ones((total, len(BSDF_COLS)), bool)
    cmp_flags = np.ones((total, len(BSDF_FLAGS) + 1), bool)
    flag = BSDF_FLAGS.index
    btype, alphas = bsdf_type(rec), ggx_alphas(rec)
    specular = alphas is not None and max(alphas) < 1e-3
    reflected = ~(samp[:, 9] != 0)

    # Rule 1, per output: a draw on the rim of the unit disk (rim_draw).  What is taken from sqrt(1 - r^2) -- the sampled wi
    # and with it f, pdf, `pdf != 0`, the lobe choice (and the delta flag that a refraction carries), and an evaluation AT that
    # wi -- is not compared; the prepared terms, eta and the evaluations at the other directions are, and every output must still be finite.  A specular
    # record never reads u2: nothing is exempt there.
    x["rim"] = rim_draw(x["u2"])
    if not specular:
        rim = x["rim"]
        cmp_cont[np.ix_(rim, _cols("wi", "f", "pdf"))] = False
        cmp_flags[rim, flag("pdf_nonzero")] = cmp_flags[rim, flag("refract")] = False
        if btype == 1:      # a rim normal is perpendicular to wo: Fresnel at cos_HO ~ 0 is total reflection or not by rounding,
            cmp_flags[rim, flag("delta")] = False     # and a refraction is flagged delta
        at_own = rim & own
        cmp_cont[np.ix_(at_own, _cols("eval_f", "eval_pdf"))] = False
        cmp_flags[at_own, flag("eval_pdf_nonzero")] = False

    # Rule 2, per output: D(cos_NH) of a sharp isotropic lobe (d_ulp_sensitivity).  Where ONE ulp of cos_NH moves D at the
    # lobe's centre by more than an output's whole tolerance, two correct implementations do not agree on that output in any
    # case that matters: the reflected sample's pdf for alpha^2 < 2.4e-3 (tolerance 1e-4), the evaluations for alpha^2 <
    # 1.2e-4 (2e-3).  Alpha 1e-3 (codes 66): 24 % per ulp, both; alpha 0.02: 6e-4, the pdf only -- its evaluations stay in
    # and the cos_NH copies of the filter decide case by case.  The sampled f never passes through D (0 on reflection, a
    # delta lobe on refraction), nor does a refracted pdf.
    sens = d_ulp_sensitivity(rec)
    if sens > TOL_BSDF["pdf"][0]:
        cmp_cont[np.ix_(reflected, _cols("pdf"))] = False
    if sens > TOL_BSDF["eval_f"][0]:
        cmp_cont[:, _cols("eval_f", "eval_pdf")] = False

    # Rule 3, per output: a dielectric with eta == 1.  fresnel_dielectric has cosT = cosI up to rounding, so F is 0 or
    # ~1e-16 at random and an evaluation on the reflection side (f = F ..., pdf = F / (F + T) ...) is that noise, `pdf != 0`
    # included; so are the pdf and `pdf != 0` of a sample that reflected.  Not compared; the transmission side is.
    x["ill_defined"] = np.zeros(total, bool)
    if btype == 1:
        eta = np.ascontiguousarray(rec, np.uint8).view(np.float16)[9].astype(np.float32)
        below = (x["wi"] * x["ns"]).sum(axis=1, dtype=np.float32) < 0
        if eta == 1.0:
            cmp_cont[np.ix_(~below, _cols("eval_f", "eval_pdf"))] = False
            cmp_flags[~below, flag("eval_pdf_nonzero")] = False
            cmp_cont[np.ix_(reflected, _cols("pdf", "f"))] = False
            cmp_flags[reflected, flag("pdf_nonzero")] = False
        # Rule 4, per case (the reference is NaN by construction): evalGGX normalises the transmission half vector
        # H = ior wi + wo (bsdf.cu:600-603); with eta == 1 the refracted sample is wi == -wo, H == 0, 0 * inf.
        H = np.where(below[:, None], eta * x["wi"] + x["wo"], x["wi"] + x["wo"]).astype(np.float32)
        x["ill_defined"] = (H * H).sum(axis=1, dtype=np.float32) <= np.float32(1e-30)

    cont, flags, kept, escaped = condition(lambda y, k: oracle_bsdf(O, rec, y, False, k), x, ("ns", "ng", "wo", "wi"), rel, abs_,
                                           cmp_cont, cmp_flags, lambda y: oracle_bsdf(O, rec, y, True), internal=True)
    kept &= ~x["ill_defined"]
    escaped &= kept
    return Sweep(rec, x, BSDF_CELLS, cont, flags, kept, escaped, rel, abs_, cmp_cont, cmp_flags)


@functools.lru_cache(maxsize=None)
def _plain_records_cached(O):
    return plain_bsdf_records(O)


_SWEEPS = {}


def bsdf_sweep(O, name, rec=None):
    """The sweep of record `name` (cached).  tex* records come from the oracle's material probe unless `rec` is given."""
    if name not in _SWEEPS:
        if rec is None:
            rec = material_records(O)[name] if name.startswith("tex") else _plain_records_cached(O)[name]
        _SWEEPS[name] = _bsdf_sweep_of(O, rec, 1000 + BSDF_RECORD_NAMES.index(name), N_CELL)
    return _SWEEPS[name]


# ---- lights ---------------------------------------------------------------------------------------------------------
LPOS = np.array([0.5, 2.0, 1.0])
SPOT_DIR = _unit(np.array([0.1, 0.2, -1.0]))


def _shell(rng, n, lo, hi):
    return LPOS + _sphere(rng, n) * rng.uniform(lo, hi, n)[:, None]


def _along_spot(rng, n, lat_lo, lat_hi, radius):
    """positions down the spot's axis, offset sideways by lat_lo..lat_hi radii"""
    t, b = _frame(SPOT_DIR[None])
    phi = rng.uniform(0, 2 * np.pi, n)
    lat = rng.uniform(lat_lo, lat_hi, n) * radius
    return (LPOS + rng.uniform(1.0, 1.5, n)[:, None] * SPOT_DIR
            + lat[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * b))


# name -> (record maker, effectively delta, [(cell, position generator, hadT)])
def light_specs(O):
    box = lambda rng, n: rng.random((n, 3)) * np.array([4, 4, 2.5]) + np.array([-2, 0, -0.5])
    return {
        "point_tiny": (O.make_point_light([1, 2, 3], LPOS, 0.001), True, [("outside", lambda r, n: _shell(r, n, 1.5, 3.0), None)]),
        "point_medium": (O.make_point_light([1, 2, 3], LPOS, 0.75), False, [("outside", lambda r, n: _shell(r, n, 1.0, 3.0), None)]),
        "point_enclosing": (O.make_point_light([1, 2, 3], LPOS, 4.0), False,
                            [("inside_hadT0", lambda r, n: _shell(r, n, 0.2, 3.5), 0), ("inside_hadT1", lambda r, n: _shell(r, n, 0.2, 3.5), 1)]),
        # cosThetaE 0.99: the spread cone is narrower than the cone the sphere subtends at these distances
        "spot_spread": (O.make_spot_light([3, 2, 1], LPOS, SPOT_DIR, 0.995, 0.99, 0.8), False,
                        [("sphere_hit", lambda r, n: _along_spot(r, n, 0.0, 0.5, 0.8), None),
                         ("sphere_miss", lambda r, n: _along_spot(r, n, 1.4, 2.0, 0.8), None)]),
        "spot_wide": (O.make_spot_light([3, 2, 1], LPOS, SPOT_DIR, 0.95, 0.9, 0.3), False, [("outside", lambda r, n: _shell(r, n, 1.0, 3.0), None)]),
        "spot_inside": (O.make_spot_light([3, 2, 1], LPOS, SPOT_DIR, 0.95, 0.9, 2.0), False,
                        [("inside_hadT0", lambda r, n: _shell(r, n, 0.2, 1.8), 0), ("inside_hadT1", lambda r, n: _shell(r, n, 0.2, 1.8), 1)]),
        "spot_tiny": (O.make_spot_light([3, 2, 1], LPOS, SPOT_DIR, 0.95, 0.9, 0.001), True, [("outside", lambda r, n: _shell(r, n, 1.5, 3.0), None)]),
        "dir_omc0": (O.make_directional_light([1, 1, 0.5], _unit(np.array([0.3, -0.2, -1.0])), 0.0), False, [("anywhere", box, None)]),
        "dir_omc001": (O.make_directional_light([1, 1, 0.5], _unit(np.array([0.3, -0.2, -1.0])), 0.01), False, [("anywhere", box, None)]),
        "env": (O.make_env_light([0.1, 0.2, 0.3]), False, [("anywhere", box, None)]),
    }


LIGHT_NAMES = ["point_tiny", "point_medium", "point_enclosing", "spot_spread", "spot_wide", "spot_inside", "spot_tiny",
               "dir_omc0", "dir_omc001", "env"]


def _light_pack(out):
    cont = np.concatenate([out[:, 0:7], out[:, 8:13]], axis=1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        flags = np.stack([out[:, 7] != 0, out[:, 13] != 0, out[:, 6] != 0, np.isfinite(cont).all(axis=1)], axis=1)
    return cont, flags


def oracle_light(O, rec, x, contracted=False):
    return _light_pack(O.light_cases(rec, x["pos"], x["nrm"], x["u2"], x["hadt"], contracted))


def device_light(renderer, rec, x):
    return _light_pack(renderer.test_light(rec, x["pos"], x["nrm"], x["u2"], x["hadt"]))


def light_sweep(O, name):
    key = "light:" + name
    if key in _SWEEPS:
        return _SWEEPS[key]
    rec, eff_delta, cells = light_specs(O)[name]
    rng = np.random.default_rng(2000 + LIGHT_NAMES.index(name))
    names, pos, hadt, u2 = [], [], [], []
    for cname, gen, ht in cells + [("boundary_u2", cells[0][1], cells[0][2])]:
        names.append(cname)
        pos.append(_f32(gen(rng, N_CELL)))
        hadt.append((rng.random(N_CELL) < 0.25).astype(np.int32) if ht is None else np.full(N_CELL, ht, np.int32))
        u = rng.random((N_CELL, 2), dtype=np.float32)
        if cname == "boundary_u2":
            u = _boundary_draws(u)
        u2.append(u)
    total = N_CELL * len(names)
    x = dict(pos=np.concatenate(pos), nrm=_f32(_sphere(rng, total)), u2=np.concatenate(u2), hadt=np.concatenate(hadt),
             cell=np.repeat(np.arange(len(names), dtype=np.int32), N_CELL))
    rel, abs_ = _tol_arrays(LIGHT_COLS, light_tolerances(eff_delta))
    cmp_cont = np.ones((total, len(LIGHT_COLS)), bool)
    cmp_flags = np.ones((total, len(LIGHT_FLAGS) + 1), bool)
    # Per-output rule: a draw on the rim of the disk (rim_draw) at a point or spot light.  sampleUniformCone's direction, cosTheta
    # and pdf are well conditioned there and stay compared; the ray is tangent to the light's sphere, and what is taken from
    # sqrt(r^2 - d^2 sin^2) ~ sqrt(0) is not: distance, pLight, Le.  Sampled from inside the radius, the direction itself comes
    # from sqrt(1 - r^2) (cosine hemisphere, uniform sphere) and is not compared either, nor the pdf and validity that follow it.
    x["rim"] = rim_draw(x["u2"]) & (bsdf_type(rec) in (0, 1))           # LT_POINT, LT_SPOT share the halfword
    cmp_cont[np.ix_(x["rim"], np.isin(LIGHT_COLS, ("distance", "pLight", "Le")))] = False
    inside = np.full(total, name in ("point_enclosing", "spot_inside"))     # every position of these two lies within the radius
    cmp_cont[np.ix_(x["rim"] & inside, np.isin(LIGHT_COLS, ("direction", "pdf")))] = False   # (pdf = cos / pi of that hemisphere)
    cmp_flags[np.ix_(x["rim"] & inside, [LIGHT_FLAGS.index("valid"), LIGHT_FLAGS.index("pdf_nonzero")])] = False
    x["ill_defined"] = np.zeros(total, bool)
    cont, flags, kept, escaped = condition(lambda y, k: oracle_light(O, rec, y), x, ("pos", "nrm"), rel, abs_, cmp_cont, cmp_flags,
                                           lambda y: oracle_light(O, rec, y, True))
    _SWEEPS[key] = Sweep(rec, x, names, cont, flags, kept, escaped, rel, abs_, cmp_cont, cmp_flags)
    return _SWEEPS[key]


def report(O):
    """the table of the module docstring"""
    lines = []
    for name in BSDF_RECORD_NAMES:
        s = bsdf_sweep(O, name)
        rates = s.keep_rates()
        worst = min(rates, key=rates.get)
        lines.append(f"  {name:18s} kept {s.kept.mean():5.3f}  lowest cell {worst:12s} {rates[worst]:5.3f}  h {s.h:2d} / {int(s.kept.sum())}")
    for name in LIGHT_NAMES:
        s = light_sweep(O, name)
        rates = s.keep_rates()
        worst = min(rates, key=rates.get)
        lines.append(f"  light {name:15s} kept {s.kept.mean():5.3f}  lowest cell {worst:12s} {rates[worst]:5.3f}  h {s.h:2d} / {int(s.kept.sum())}")
    return "\n".join(lines)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import __graft_entry__ as graft
    oracle = graft.load_oracle()
    oracle.build()
    print(report(oracle))
    if "-v" in sys.argv:
        for nm in BSDF_RECORD_NAMES:
            print(nm, {k: round(v, 3) for k, v in bsdf_sweep(oracle, nm).keep_rates().items()})
        for nm in LIGHT_NAMES:
            print(nm, {k: round(v, 3) for k, v in light_sweep(oracle, nm).keep_rates().items()})
