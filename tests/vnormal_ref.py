"""numpy restatement of smooth shading (csrc/vnormals.hpp): the per-triangle record, shading_normal_at
and dmt_smooth_normals, plus the scenes the tests share.

The octahedral words.  The device decodes with its unchanged dir_from_octa, restated here through the oracle's
oracle_dir_from_octa.  The oracle's ENCODER (oracle_octa_from_dir, the reference's octaFromDir) clamps a component to
[0, 1] before it rounds, so every direction packs to components 0 or 1 -- test_the_reference_encoder_cannot_carry_normals
pins that -- and the record is written with the same arithmetic clamped at 65535 instead: octa_words below restates
that encoder operation by operation in fp32, so the words are the device's.  Interpolation in float64."""
import ctypes as C

import numpy as np

F = np.float32


def normalise_host(n9):
    """the host's normalisation of an uploaded normal: fp32 components over their float64 length, rounded to fp32"""
    n = np.asarray(n9, np.float32).reshape(-1, 3).astype(np.float64)
    ln = np.sqrt((n * n).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (n / ln).astype(np.float32)


def octa_words(d):
    """uint32 [n] words of fp32 unit directions [n, 3]: encoding.cu:26-37 with the component clamped to [0, 65535]"""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    l1 = (np.abs(d[:, 0]) + np.abs(d[:, 1])).astype(F) + np.abs(d[:, 2])
    px, py, pz = (d[:, 0] / l1).astype(F), (d[:, 1] / l1).astype(F), (d[:, 2] / l1).astype(F)
    sgn = lambda v: np.where(np.signbit(v), F(-1), F(1)).astype(F)
    flip = pz < 0
    x = np.where(flip, ((F(1) - np.abs(py)).astype(F) * sgn(px)).astype(F), px)
    y = np.where(flip, ((F(1) - np.abs(px)).astype(F) * sgn(py)).astype(F), py)

    def comp(v):
        s = (((v + F(1)).astype(F) * F(0.5)).astype(F) * F(65535.0)).astype(F)
        s = np.maximum(np.minimum(s, F(65535.0)), F(0))
        return np.floor(s.astype(np.float64) + 0.5).astype(np.uint32)  # roundf: halves away from zero (s >= 0)

    return (comp(y) << np.uint32(16)) | comp(x)


def decode_words(O, words):
    """fp32 [n, 3]: the oracle's dirFromOcta of each word (the decoder the device restates)"""
    L = O.lib()
    words = np.asarray(words, np.uint32).reshape(-1)
    uniq, inv = np.unique(words, return_inverse=True)
    out = np.zeros((uniq.shape[0], 3), np.float32)
    for i, w in enumerate(uniq):
        L.oracle_dir_from_octa(C.c_uint32(int(w)), out[i].ctypes.data_as(C.c_void_p))
    return out[inv]


def angle_between(a, b):
    """radians [n] between the rows of a and b, by atan2(|a x b|, a . b): exact for small angles, where acos of a dot
    product of fp32 unit vectors is not"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def pack_records(n9):
    """(words uint32 [n, 3], smooth bool [n]) as dmt_upload_vertex_normals makes them; all-zero rows are flat"""
    n9 = np.asarray(n9, np.float32).reshape(-1, 9)
    smooth = ~(n9 == 0).all(1)
    words = np.zeros((n9.shape[0], 3), np.uint32)
    if smooth.any():
        words[smooth] = octa_words(normalise_host(n9[smooth])).reshape(-1, 3)
    return words, smooth


def facing_normal(ng, rd):
    """hit_finish: the stored normal, negated where dot(rd, n) > 0 (fp32 products summed left to right)"""
    ng, rd = np.asarray(ng, np.float32), np.asarray(rd, np.float32)
    d = ((rd[:, 0] * ng[:, 0]).astype(F) + (rd[:, 1] * ng[:, 1]).astype(F)).astype(F) + (rd[:, 2] * ng[:, 2]).astype(F)
    return np.where((d > 0)[:, None], -ng, ng).astype(np.float32), d


def shading_normal(O, words, smooth, tri, bu, bv, ng_facing):
    """float64 [n, 3] and fallback bool [n]: shading_normal_at of records (words, smooth) at the cases; a fallback case
    (flat triangle, or squared length of the sum below 1e-12 / not finite) returns ng_facing itself"""
    tri = np.asarray(tri, np.int64)
    bu, bv = np.asarray(bu, np.float32).astype(np.float64), np.asarray(bv, np.float32).astype(np.float64)
    ngf = np.asarray(ng_facing, np.float32).astype(np.float64)
    dec = decode_words(O, words[tri].reshape(-1)).reshape(-1, 3, 3).astype(np.float64)
    w0 = (np.asarray(1.0, np.float32) - np.asarray(bu, np.float32) - np.asarray(bv, np.float32)).astype(np.float64)  # fp32, as the device
    with np.errstate(invalid="ignore", divide="ignore"):
        n = w0[:, None] * dec[:, 0] + bu[:, None] * dec[:, 1] + bv[:, None] * dec[:, 2]
        l2 = (n * n).sum(1)
        fallback = ~smooth[tri] | ~(l2 >= 1e-12) | ~np.isfinite(l2)
        n = n / np.sqrt(l2)[:, None]
    n = np.where(((n * ngf).sum(1) < 0)[:, None], -n, n)
    return np.where(fallback[:, None], ngf, n), fallback, l2


def face_normals(xs, ys, zs):
    """fp32 [n, 3]: TriPost's stored normal, normalize(cross(e1, e0)) without contraction; zero rows for zero-area triangles"""
    P = np.stack([np.asarray(a, np.float32).reshape(-1, 4)[:, :3] for a in (xs, ys, zs)], -1)  # [n, corner, xyz]
    e0, e1 = (P[:, 1] - P[:, 0]).astype(F), (P[:, 2] - P[:, 0]).astype(F)
    mul = lambda a, b: (a * b).astype(F)
    c = np.stack([(mul(e1[:, 1], e0[:, 2]) - mul(e1[:, 2], e0[:, 1])).astype(F), (mul(e1[:, 2], e0[:, 0]) - mul(e1[:, 0], e0[:, 2])).astype(F),
                  (mul(e1[:, 0], e0[:, 1]) - mul(e1[:, 1], e0[:, 0])).astype(F)], -1)
    l2 = ((mul(c[:, 0], c[:, 0]) + mul(c[:, 1], c[:, 1])).astype(F) + mul(c[:, 2], c[:, 2])).astype(F)
    ok = (l2 > 0) & np.isfinite(l2)
    inv = np.zeros_like(l2)
    inv[ok] = (F(1) / np.sqrt(l2[ok]).astype(F)).astype(F)
    return (c * inv[:, None]).astype(np.float32), ok


def smooth_normals(xs, ys, zs, crease_degrees):
    """float64 [n, 9]: dmt_smooth_normals restated -- corners welded by bit-equal positions (-0 with +0), the fp32 face
    normals of the faces within the crease angle of the corner's own face summed with their interior angles as weights"""
    P = np.stack([np.asarray(a, np.float32).reshape(-1, 4)[:, :3] for a in (xs, ys, zs)], -1)
    n = P.shape[0]
    fn, ok = face_normals(xs, ys, zs)
    fn = fn.astype(np.float64)
    Pd = P.astype(np.float64)
    weld = {}
    for i in range(n):
        if not ok[i]:
            continue
        for c in range(3):
            a, b = Pd[i, (c + 1) % 3] - Pd[i, c], Pd[i, (c + 2) % 3] - Pd[i, c]
            cs = np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))
            key = (P[i, c] + F(0)).tobytes()  # + 0: -0 becomes +0
            weld.setdefault(key, []).append((i, float(np.arccos(np.clip(cs, -1.0, 1.0)))))
    cos_crease = np.cos(np.radians(np.clip(float(crease_degrees), 0.0, 180.0)))
    out = np.zeros((n, 9))
    for i in range(n):
        if not ok[i]:
            continue
        for c in range(3):
            s = np.zeros(3)
            for j, ang in weld[(P[i, c] + F(0)).tobytes()]:
                if j != i and np.dot(fn[i], fn[j]) < cos_crease - 1e-12:
                    continue
                s += ang * fn[j]
            ln = np.linalg.norm(s)
            out[i, 3 * c:3 * c + 3] = s / ln if ln > 1e-12 else fn[i]
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def icosphere(center=(0.0, 2.2, 0.8), radius=0.6):
    """A once-subdivided icosahedron: (triangles float32 [80, 3, 3], radial unit normals float64 [80, 3, 3])"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], np.float64)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    Fc = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
          (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    tris = []
    for a, b, c in Fc:
        A, B, Cc = V[a], V[b], V[c]
        ab, bc, ca = [(p + q) / np.linalg.norm(p + q) for p, q in ((A, B), (B, Cc), (Cc, A))]
        tris += [(A, ab, ca), (B, bc, ab), (Cc, ca, bc), (ab, bc, ca)]
    N = np.array(tris, np.float64)
    T = (N * radius + np.asarray(center, np.float64)).astype(np.float32)
    return T, N


def sphere_scene(O, res):
    """The Cornell box (flat) plus the icosphere in the free space between its two octahedra, material 1.  Returns
    (scene, n9 float32 [tri_count, 9]): zero rows for the box, radial normals for the 80 sphere triangles (the last 80)."""
    sc = O.cornell_box(res, res)
    T, N = icosphere()
    k = T.shape[0]
    add = lambda old, ax: np.concatenate([old, np.concatenate([T[:, :, ax], np.zeros((k, 1), np.float32)], 1)])
    out = O.Scene(add(sc.xs, 0), add(sc.ys, 1), add(sc.zs, 2), np.concatenate([sc.mat_id, np.full(k, 1, np.uint32)]), sc.bsdfs, sc.lights,
                  sc.inf_lights, sc.camera)
    n9 = np.concatenate([np.zeros((sc.tri_count, 9), np.float32), N.reshape(k, 9).astype(np.float32)])
    return out, n9
