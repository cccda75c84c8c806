"""Alpha cutouts (dmt_upload_opacity): a numpy float32 restatement of the opacity lookup and the pass test,
and the small scenes the cutout tests share.  Every operation below is one rounded float32 operation in the documented
order, so the restatement equals the host twin (dmt_opacity_eval) and the device bit for bit."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF


def _mirror(c, size):
    p = 2 * size
    c = np.mod(c, p)  # numpy's mod takes the divisor's sign: already in [0, p)
    return np.where(c < size, c, p - c - 1)


def alpha8(tex_rgba, tex_desc, tex, uv6, bu, bv):
    """alpha8 [n] float32 of texture tex[i] for a triangle with UVs uv6[i] at barycentrics (bu[i], bv[i])"""
    rgba = np.ascontiguousarray(tex_rgba, np.uint8).reshape(-1, 4)
    desc = np.asarray(tex_desc, np.int64).reshape(-1, 3)
    tex = np.asarray(tex, np.int64).reshape(-1)
    uv6 = np.asarray(uv6, F).reshape(-1, 6)
    bu, bv = np.asarray(bu, F).reshape(-1), np.asarray(bv, F).reshape(-1)
    one, half, lim = F(1), F(0.5), F(2.0 ** 30)
    with np.errstate(over="ignore", invalid="ignore"):
        w0 = (one - bu) - bv
        s = (w0 * uv6[:, 0] + bu * uv6[:, 2]) + bv * uv6[:, 4]
        t = (w0 * uv6[:, 1] + bu * uv6[:, 3]) + bv * uv6[:, 5]
        first, w, h = desc[tex, 0], desc[tex, 1], desc[tex, 2]
        x = np.minimum(np.maximum(s * w.astype(F) - half, -lim), lim).astype(F)
        y = np.minimum(np.maximum(t * h.astype(F) - half, -lim), lim).astype(F)
        fx, fy = np.floor(x), np.floor(y)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        tx, ty = (x - fx).astype(F), (y - fy).astype(F)
        xa, xb, ya, yb = _mirror(x0, w), _mirror(x0 + 1, w), _mirror(y0, h), _mirror(y0 + 1, h)
        A = rgba[:, 3].astype(F)
        a00, a10 = A[first + ya * w + xa], A[first + ya * w + xb]
        a01, a11 = A[first + yb * w + xa], A[first + yb * w + xb]
        ax0 = a00 * (one - tx) + a10 * tx
        ax1 = a01 * (one - tx) + a11 * tx
        a = ax0 * (one - ty) + ax1 * ty
    assert a.dtype == F
    return a


def passes(a8, cutoff):
    return a8 >= F(cutoff) * F(255.0)


# ---- textures ---------------------------------------------------------------------------------------------------
def rgba_of_alpha(a):
    """[h, w] alpha bytes -> [h * w, 4] RGBA8 texels with RGB = A (what the JSON loader makes of an opacity texture)"""
    a = np.asarray(a, np.uint8)
    return np.repeat(a.reshape(-1, 1), 4, axis=1)


def pack_textures(alphas):
    """(tex_rgba, tex_desc) of a list of [h, w] alpha arrays, back to back"""
    desc, first = [], 0
    for a in alphas:
        h, w = np.asarray(a).shape
        desc.append([first, w, h])
        first += w * h
    return np.concatenate([rgba_of_alpha(a) for a in alphas]), np.array(desc, np.int32)


def checker(n, lo=0, hi=255, cell=1):
    yy, xx = np.mgrid[0:n, 0:n]
    return np.where(((xx // cell + yy // cell) % 2) == 0, hi, lo).astype(np.uint8)


def gradient(w, h):
    return np.tile(np.linspace(0, 255, w).astype(np.uint8), (h, 1))


# ---- geometry ---------------------------------------------------------------------------------------------------
def soup(T):
    """[n, 3, 3] triangles -> (xs, ys, zs) in upload_triangles' layout"""
    T = np.asarray(T, F)
    out = []
    for c in range(3):
        a = np.zeros((T.shape[0], 4), F)
        a[:, :3] = T[:, :, c]
        out.append(a)
    return tuple(out)


def card(p00, du, dv):
    """two triangles (p00, p00 + du, p00 + du + dv) and (p00, p00 + du + dv, p00 + dv) with UVs (0,0)-(1,1): [2, 3, 3], [2, 6]"""
    p00, du, dv = (np.asarray(v, np.float64) for v in (p00, du, dv))
    T = np.array([[p00, p00 + du, p00 + du + dv], [p00, p00 + du + dv, p00 + dv]]).astype(F)
    uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], F)
    return T, uv


class CutScene:
    """a scene in the upload layout (the attributes Renderer.upload_scene reads): `base` (an oracle scene) plus `meshes`, a
    list of (triangles [m, 3, 3], uv [m, 6], opacity texture index or NONE); each mesh gets a BSDF record of its own, a copy
    of base's record `like`.  skip: meshes left out (their materials and textures stay, so every index stays)"""

    def __init__(self, base, meshes, alphas, cutoff=0.5, like=3, skip=(), env=None, rng_seed=9):
        nb = base.bsdfs.shape[0]
        T0 = np.stack([np.asarray(base.xs)[:, :3], np.asarray(base.ys)[:, :3], np.asarray(base.zs)[:, :3]], axis=2)
        n0 = T0.shape[0]
        tris, mats = [T0], [np.asarray(base.mat_id, np.uint32)]
        uvs = [np.random.default_rng(rng_seed).uniform(-0.5, 2.5, (n0, 6)).astype(F)]
        self.mesh_tris = []
        at = n0
        for k, (T, uv, _) in enumerate(meshes):
            if k in skip:
                self.mesh_tris.append(np.zeros(0, np.int64))
                continue
            tris.append(np.asarray(T, F)), uvs.append(np.asarray(uv, F)), mats.append(np.full(len(T), nb + k, np.uint32))
            self.mesh_tris.append(np.arange(at, at + len(T)))
            at += len(T)
        self.xs, self.ys, self.zs = soup(np.concatenate(tris))
        self.mat_id = np.concatenate(mats)
        self.bsdfs = np.concatenate([base.bsdfs] + [base.bsdfs[like:like + 1]] * len(meshes))
        self.lights, self.inf_lights, self.camera = base.lights, base.inf_lights, base.camera
        self.env_rgb, self.env_quat, self.env_scale = env, np.array([0, 0, 0, 1], F), 1.0
        self.tex_rgba, self.tex_desc = pack_textures(alphas)
        self.mat_tex = np.full((self.bsdfs.shape[0], 4), NONE, np.uint32)
        self.mat_tex[:, 3] = F(1.0).view(np.uint32)
        self.mat_tex[0, 0] = 0  # the Oren-Nayar material of the octahedron takes texture 0 as its albedo: the texture code runs
        self.tri_uv = np.concatenate(uvs)
        self.mat_opacity = np.full(self.bsdfs.shape[0], NONE, np.uint32)
        for k, (_, _, tex) in enumerate(meshes):
            self.mat_opacity[nb + k] = tex
        self.opacity_cutoff = cutoff

    @property
    def tri_count(self):
        return int(self.mat_id.shape[0])


def cornell_cards():
    """the cards of the film tests, in the Cornell box (x in [-2, 2], y in [0, 4], floor z = -0.5, spot light near z = 1.7):
    0 a horizontal card between the light and the floor, 1 a vertical card facing the camera, 2 a slanted card in front of
    the right wall"""
    return [card((-0.9, 1.3, 0.7), (1.8, 0, 0), (0, 1.5, 0)),
            card((-1.6, 2.4, -0.45), (1.3, 0, 0), (0, 0.1, 1.4)),
            card((0.5, 2.9, -0.4), (1.2, 0.5, 0), (0, 0, 1.3))]
