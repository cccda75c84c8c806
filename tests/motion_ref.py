"""Shared pieces of the motion-blur tests (include/dmt_hip.h dmt_set_motion): the scenes with their key-1
positions, an exact restatement of the sample time on top of tests/lens_ref.py's sampler, and a numpy check that the
test inputs have teeth.  Soups are the upload layout: xs / ys / zs with 4 floats per triangle (c0, c1, c2, pad)."""
from fractions import Fraction

import numpy as np

import lens_ref as LR

F = np.float32


# ---- the sample time, exactly ------------------------------------------------------------------------
def shutter_time(w, h, px, py, s, open_, close):
    """t = fmaf(close - open, u12, open): u12 the base-41 scrambled radical inverse (dimension 12) of the sample's Halton
    index in exact integer digits and float32 steps, the fmaf in exact rational arithmetic rounded once."""
    hidx = LR.halton_index(LR.halton_params(w, h), int(px), int(py), int(s))
    u = LR.owen_radical_inverse(41, LR.owen_seed(12), hidx)
    span = F(F(close) - F(open_))
    return LR.round_f32(Fraction(float(span)) * Fraction(float(u)) + Fraction(float(F(open_))))


# ---- soups -----------------------------------------------------------------------------------------
def soup(tris):
    """[n, 3 vertices, 3 coordinates] -> xs, ys, zs"""
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    z = np.zeros((T.shape[0], 1), F)
    return tuple(np.ascontiguousarray(np.concatenate([T[:, :, k], z], 1).reshape(-1)) for k in range(3))


def tris_of(xs, ys, zs):
    return np.stack([np.asarray(a, F).reshape(-1, 4)[:, :3] for a in (xs, ys, zs)], axis=2)  # [n, vertex, coordinate]


def cornell_keys(scene, offsets=((1.25, 0.5, 0.75), (-1.5, -0.25, 0.5))):
    """The Cornell box with its two octahedra (materials 0 and 1, 1.0 across) translated by more than their size."""
    T0 = tris_of(scene.xs, scene.ys, scene.zs)
    T1 = T0.copy()
    mat = np.asarray(scene.mat_id)
    for m, off in zip((0, 1), offsets):
        T1[mat == m] += np.asarray(off, F)
    return soup(T0), soup(T1)


def random_keys(n=300, seed=7, extent=2.0, grid=None):
    """n random triangles in a cube of side 2 * extent around (0, 3, 0), each with its own random displacement of up to
    the scene size and a small per-vertex deformation.  grid: snap key 0 and the displacement (one per triangle, no
    deformation) to multiples of it."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, (n, 1, 3)) + np.array([0, 3.0, 0])
    T0 = (c + rng.uniform(-0.35, 0.35, (n, 3, 3))).astype(F)
    d = rng.uniform(-extent, extent, (n, 1, 3))
    if grid is None:
        T1 = (T0 + d + rng.uniform(-0.1, 0.1, (n, 3, 3))).astype(F)
    else:
        T0 = (np.round(T0 / grid) * grid).astype(F)
        T1 = (T0 + np.round(d / grid) * grid).astype(F)
    return soup(T0), soup(T1)


def floor_keys(nfloor):
    """the 1-3-triangle floor of test_bvh_empty_slots_axis_parallel_rays, key 1 lifted and shifted"""
    t = [((-1, 0, -1), (1, 0, -1), (1, 0, 1)), ((-1, 0, -1), (1, 0, 1), (-1, 0, 1)), ((2, 0, 2), (3, 0, 2), (3, 0, 3))][:nfloor]
    T0 = np.asarray(t, F)
    T1 = T0 + np.asarray([0.5, 1.0, -0.25], F)
    return soup(T0), soup(T1)


def key1_escapes_key0_boxes(k0, k1, pad=1e-3):
    """How many triangles have a key-1 vertex outside their own key-0 box (grown by pad): a tree built from key 0 alone
    bounds each leaf by those boxes, so any such triangle would be missed at t = 1."""
    T0, T1 = tris_of(*k0), tris_of(*k1)
    lo, hi = T0.min(1, keepdims=True) - pad, T0.max(1, keepdims=True) + pad
    return int(((T1 < lo) | (T1 > hi)).any((1, 2)).sum())
