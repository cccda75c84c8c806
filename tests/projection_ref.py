"""float64 restatement of the camera projections (include/dmt_hip.h dmt_set_projection).

The models are restated from their definitions in camera space (x right, y up, z forward) in float64, on the float32
camera matrices of dmt_set_camera (lens_ref.camera_xf): what the fp32 code approximates.  The film positions are float32
values, exact inputs.  `e_host` is the measured distance between the host twin (dmt_projection_rays) and this restatement
over CASES; the device's tolerance is a multiple of it (measure_e_host), as for the lens.
"""
import functools

import numpy as np

import lens_ref as LR

F = np.float32
PERSPECTIVE, ORTHOGRAPHIC, EQUIRECT, FISHEYE = 0, 1, 2, 3
FRAMES = ((64, 32), (48, 32))   # 2 : 1, and not
# (kind, param): the orthographic height frames depth 4 of the Cornell camera's order of size; the fisheye's are a common
# wide angle and the widest one the library takes
MODELS = ((ORTHOGRAPHIC, 3.0), (EQUIRECT, 0.0), (FISHEYE, 150.0), (FISHEYE, 360.0))


def oblique_camera(w, h):
    """the oblique camera of test_lens_gpu.py at w x h"""
    b = np.zeros(11, np.float32)
    b[0:3], b[3:6], b[9], b[10] = (0.3, 1.0, -0.2), (1.5, -2.0, 0.75), 28.0, 36.0
    b.view(np.int32)[6:9] = (w, h, 1)
    return b.view(np.uint8).copy()


def resized(camera44, w, h):
    c = np.ascontiguousarray(camera44, np.uint8).reshape(44).copy()
    c.view(np.int32)[6:8] = (w, h)
    return c


def film_positions(w, h):
    """the film positions of lens_ref.cases (256 seeded samples, as the sampler forms them) plus the film's centre, corners
    and edge midpoints: [n, 2] float32"""
    p = LR.halton_params(w, h)
    px, py, s = LR.cases(w, h)
    xy = [LR.film_position(p, int(x), int(y), LR.halton_index(p, int(x), int(y), int(k))) for x, y, k in zip(px, py, s)]
    xy += [(w / 2, h / 2), (0, 0), (w, 0), (0, h), (w, h), (w / 2, 0), (w / 2, h), (0, h / 2), (w, h / 2)]
    return np.array(xy, F)


N_SPECIAL = 9  # the last rows of film_positions: centre, four corners, four edge midpoints


def ortho_k(camera44, param):
    """k = param / (sensor_size 0.001f) in fp32, as the host forms it once: an input of the model like the matrices"""
    sensor = LR.camera_fields(camera44)[5]
    return F(F(param) / F(sensor * F(0.001)))


def cam_dir64(kind, param, w, h, fx, fy):
    """the camera-space unit direction of the angular models at film position (fx, fy), float64"""
    fx, fy = float(fx), float(fy)
    if kind == EQUIRECT:
        lon, lat = (fx / w - 0.5) * 2.0 * np.pi, (0.5 - fy / h) * np.pi
        return np.array([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)])
    x, y = fx - w / 2.0, h / 2.0 - fy
    r, R = np.hypot(x, y), 0.5 * np.hypot(w, h)
    theta = (r / R) * np.radians(float(F(param)) / 2.0)
    if r == 0.0:
        return np.array([0.0, 0.0, 1.0])
    return np.array([np.sin(theta) * x / r, np.sin(theta) * y / r, np.cos(theta)])


def rays64(camera44, kind, param, xy):
    """float64 rays through the film positions xy [n, 2]: (o [n, 3], d [n, 3])"""
    xf = LR.camera_xf(camera44)
    right, up, fwd, pos = (xf[k].astype(np.float64) for k in ("right", "up", "fwd", "pos"))
    w, h = xf["width"], xf["height"]
    o, d = np.zeros((len(xy), 3)), np.zeros((len(xy), 3))
    for i, (fx, fy) in enumerate(xy):
        if kind == ORTHOGRAPHIC:
            k = float(ortho_k(camera44, param))
            cx = float(xf["psx"]) * float(fx) + float(xf["tx"])
            cy = -float(xf["psy"]) * float(fy) + float(xf["ty"])
            o[i], v = pos + right * (cx * k) + up * (cy * k), fwd
        else:
            c = cam_dir64(kind, param, w, h, fx, fy)
            o[i], v = pos, right * c[0] + up * c[1] + fwd * c[2]
        d[i] = v / np.sqrt(v @ v)
    return o, d


def project64(camera44, kind, param, p):
    """the float64 inverse: render-space points [n, 3] -> (xy [n, 2], depth [n])"""
    xf = LR.camera_xf(camera44)
    right, up, fwd, pos = (xf[k].astype(np.float64) for k in ("right", "up", "fwd", "pos"))
    w, h = xf["width"], xf["height"]
    q = np.asarray(p, np.float64) - pos
    c = np.stack([q @ right, q @ up, q @ fwd], 1)
    if kind == ORTHOGRAPHIC:
        k = float(ortho_k(camera44, param))
        fx = (c[:, 0] / k - float(xf["tx"])) / float(xf["psx"])
        fy = (c[:, 1] / k - float(xf["ty"])) / -float(xf["psy"])
        return np.stack([fx, fy], 1), c[:, 2]
    dist = np.sqrt((c * c).sum(1))
    if kind == EQUIRECT:
        lon, lat = np.arctan2(c[:, 0], c[:, 2]), np.arctan2(c[:, 1], np.hypot(c[:, 0], c[:, 2]))
        return np.stack([(lon / (2 * np.pi) + 0.5) * w, (0.5 - lat / np.pi) * h], 1), dist
    rho = np.hypot(c[:, 0], c[:, 1])
    theta = np.arctan2(rho, c[:, 2])
    r = theta / np.radians(float(F(param)) / 2.0) * (0.5 * np.hypot(w, h))
    ux, uy = (np.divide(c[:, k], rho, out=np.zeros_like(rho), where=rho > 0) for k in (0, 1))
    return np.stack([w / 2.0 + r * ux, h / 2.0 - r * uy], 1), dist


def away_from_singular(camera44, kind, param, xy):
    """the rays the round trip is asked of: an equirect latitude within 80 degrees, a fisheye theta in [5, 175] degrees"""
    xf = LR.camera_xf(camera44)
    w, h = xf["width"], xf["height"]
    xy = np.asarray(xy, np.float64)
    if kind == EQUIRECT:
        return np.abs((0.5 - xy[:, 1] / h) * 180.0) <= 80.0
    if kind == FISHEYE:
        r = np.hypot(xy[:, 0] - w / 2.0, h / 2.0 - xy[:, 1])
        theta = r / (0.5 * np.hypot(w, h)) * float(F(param)) / 2.0
        return (theta >= 5.0) & (theta <= 175.0)
    return np.ones(len(xy), bool)


def origin_scale(camera44):
    """what a deviation of a ray origin is measured against: the larger of |camera position| and one scene unit (the
    orthographic origins of MODELS spread over a few units around the camera)"""
    return max(float(np.abs(LR.camera_fields(camera44)[1]).max()), 1.0)


def hits_triangle64(o, d, tri):
    """Moeller-Trumbore in float64, two-sided, t > 0: which of the rays (o, d: [n, 3]) meet the triangle [3, 3]"""
    p0, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
    pv = np.cross(d, e2)
    det = pv @ e1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - p0
        u = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        v = (d * qv).sum(1) * inv
        t = (qv @ e2) * inv
    return (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)


# The scene the GPU suite looks at through the angular cameras: an env map all around and one small triangle straight ahead
# of a level camera at the origin that looks along +y.  At distance 3 the triangle subtends about 0.0022 sr, a twentieth of
# one of the 32 x 16 film's pixels at the equirect's equator: far below 1 % of the samples (test_env_scene_triangle_share).
ENV_FRAME = (32, 16)
ENV_TRIANGLE = np.array([[-0.1, 3.0, -0.1], [0.1, 3.0, -0.1], [0.0, 3.0, 0.1]], np.float32)


def env_scene_camera():
    w, h = ENV_FRAME
    b = np.zeros(11, np.float32)
    b[0:3], b[9], b[10] = (0.0, 1.0, 0.0), 20.0, 36.0
    b.view(np.int32)[6:9] = (w, h, 1)
    return b.view(np.uint8).copy()


def env_scene_samples():
    """(camera44, film positions [w h, 2] of sample 0 of every pixel, row-major)"""
    w, h = ENV_FRAME
    p = LR.halton_params(w, h)
    xy = [LR.film_position(p, x, y, LR.halton_index(p, x, y, 0)) for y in range(h) for x in range(w)]
    return env_scene_camera(), np.array(xy, F)


def cases(O):
    """[(camera44, xy)]: the Cornell camera and the oblique one, each at both frames"""
    out = []
    for w, h in FRAMES:
        out.append((resized(O.cornell_box(64, 64).camera, w, h), film_positions(w, h)))
        out.append((oblique_camera(w, h), film_positions(w, h)))
    return out


@functools.lru_cache(maxsize=None)
def _measure(projection_rays, cams):
    e = 0.0
    for cam in cams:
        cam = np.frombuffer(cam, np.uint8)
        w, h = LR.camera_xf(cam)["width"], LR.camera_xf(cam)["height"]
        xy = film_positions(w, h)
        for kind, param in MODELS:
            o, d = projection_rays(cam, kind, param, xy)
            o64, d64 = rays64(cam, kind, param, xy)
            e = max(e, float(np.abs(d - d64).max()), float(np.abs(o - o64).max()) / origin_scale(cam))
    return e


def measure_e_host(pkg, cams):
    """e_host: the largest deviation of dmt_projection_rays from the float64 restatement over the cases and MODELS -- of a
    direction component, or of an origin component relative to origin_scale.  Measured, not fixed in advance (DESIGN.md 4.22
    records the value)."""
    return _measure(pkg.projection_rays, tuple(np.ascontiguousarray(c, np.uint8).tobytes() for c in cams))
