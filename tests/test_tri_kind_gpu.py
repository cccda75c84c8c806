"""The per-triangle material kinds (dmt_tri_kind_bits; csrc/surface_state.hpp): the table GGX batching reads to decide which
hits park.  It equals the table computed here from the material ids and the BSDF records; films and parking counters do not
depend on whether it travels in the kernel arguments or as a device array (DMT_TRI_KIND_INLINE=0, read when a context is
created); and it follows a replaced BSDF array and a replaced soup.  Frames are 64 x 64 x 16 spp at a bounce cap of 8.  After
every render dmt_sync passes and the scheduler's counters show every work item folded once, no wave leaving early, and
every parked hit taken back.  Every comparison is of bytes or integers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BS_OREN, BS_GGX_DIEL, BS_GGX_COND = 0, 1, 2
SIZE, SPP, DEPTH = 64, 16, 8


def _types(bsdfs):
    return np.ascontiguousarray(bsdfs, np.uint8).reshape(-1, 32)[:, 4:8].copy().view(np.uint32)[:, 0] >> 16


def _expected(mat_id, bsdfs):
    """bit i of word i // 32: the material of triangle i is a GGX dielectric or conductor"""
    t = _types(bsdfs)
    ggx = np.isin(t[np.asarray(mat_id, np.int64)], (BS_GGX_DIEL, BS_GGX_COND))
    words = np.zeros((len(ggx) + 31) // 32, np.uint32)
    for i in np.flatnonzero(ggx):
        words[i // 32] |= np.uint32(1) << np.uint32(i % 32)
    return words


def _ctx(pkg, monkeypatch, inline=True, cull=True):
    monkeypatch.delenv("DMT_TRI_KIND_INLINE", raising=False)
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    if not inline:
        monkeypatch.setenv("DMT_TRI_KIND_INLINE", "0")
    if not cull:
        monkeypatch.setenv("DMT_BRUTE_CULL", "0")
    r = pkg.Renderer(0)
    monkeypatch.delenv("DMT_TRI_KIND_INLINE", raising=False)
    monkeypatch.delenv("DMT_BRUTE_CULL", raising=False)
    return r


def _render(r, batch=None):
    """(mean bytes, m2 bytes, counters) of one frame on a cleared film; (e): dmt_sync and the fold counters"""
    if batch is not None:
        r.set_ggx_batch(batch)
    r.set_limits(DEPTH)
    r.set_accel(0)
    r.film_clear()
    r.sched_diag(reset=True)
    r.render(SPP)
    r.sync()
    mean, m2 = r.download_film()
    d = r.sched_diag(reset=True)
    assert d["folds"] == d["launched"] > 0 and d["early_exits"] == 0 and d["ggx_parked"] == d["ggx_resumed"], d
    assert np.isfinite(mean).all() and mean[..., :3].max() > 0
    return mean.tobytes(), m2.tobytes(), d


@pytest.fixture(scope="module")
def cornell(pkg):
    sc = pkg.host_scene.cornell_box(SIZE, SIZE)
    assert np.isin(_types(sc.bsdfs), (BS_GGX_DIEL, BS_GGX_COND)).any() and (_types(sc.bsdfs) == BS_OREN).any()
    return sc


@pytest.fixture(scope="module")
def seventy(pkg, cornell):
    """The box with 44 small triangles floating in it, 70 in all: triangles 63 and 64 -- the last that fits the kernel
    arguments' two words and the first bit of the third word -- are of the GGX material, 62 and 65 of an Oren-Nayar one."""
    c = cornell
    t = _types(c.bsdfs)
    ggx, oren = int(np.flatnonzero(np.isin(t, (BS_GGX_DIEL, BS_GGX_COND)))[0]), int(np.flatnonzero(t == BS_OREN)[0])
    n0 = c.mat_id.shape[0]
    assert n0 == 26
    k = np.arange(44)
    x0 = (-1.5 + 0.27 * (k % 11)).astype(np.float32)
    z0 = (0.3 + 0.35 * (k // 11)).astype(np.float32)
    y0 = np.full(44, 1.5, np.float32)
    zero = np.zeros(44, np.float32)
    xs = np.concatenate([c.xs, np.stack([x0, x0 + 0.2, x0, zero], 1)])
    ys = np.concatenate([c.ys, np.stack([y0, y0, y0, zero], 1)])
    zs = np.concatenate([c.zs, np.stack([z0, z0, z0 + 0.25, zero], 1)])
    mat = np.concatenate([c.mat_id, np.where((n0 + k) % 3 == 0, ggx, oren)]).astype(np.uint32)   # (then 63 and 64 GGX, 62 and 65 not)
    mat[[63, 64]] = ggx
    mat[[62, 65]] = oren
    return pkg.host_scene.ArrayScene(xs, ys, zs, mat, c.bsdfs, c.lights, c.inf_lights, c.camera)


@pytest.fixture(scope="module")
def one(pkg, cornell):
    """one triangle of the GGX material"""
    c = cornell
    ggx = int(np.flatnonzero(np.isin(_types(c.bsdfs), (BS_GGX_DIEL, BS_GGX_COND)))[0])
    return pkg.host_scene.ArrayScene(c.xs[:1], c.ys[:1], c.zs[:1], np.array([ggx], np.uint32), c.bsdfs, c.lights, c.inf_lights, c.camera)


# ---- (a) the table is the one computed from the material ids and the records ----------------------------------------
@pytest.mark.parametrize("inline", [True, False])
def test_table_equals_numpy(pkg, monkeypatch, cornell, one, seventy, inline):
    r = _ctx(pkg, monkeypatch, inline)
    try:
        for sc in (cornell, one, seventy):
            r.upload_scene(sc)
            n = sc.mat_id.shape[0]
            want = _expected(sc.mat_id, sc.bsdfs)
            assert want.any()
            assert np.array_equal(r.tri_kind_bits(n), want), n
        want = _expected(seventy.mat_id, seventy.bsdfs)
        assert want.shape[0] == 3 and (want[1] >> 31) & 1 == 1 and (want[1] >> 30) & 1 == 0 and want[2] & 3 == 1
        with pytest.raises(pkg.DmtError):
            r.tri_kind_bits(64)   # room for two words, the table has three
    finally:
        r.close()


def test_uploads_in_either_order(pkg, monkeypatch, seventy):
    """BSDFs before triangles, and material ids beyond the BSDF array (not GGX; such a scene is refused at launch only)"""
    r = _ctx(pkg, monkeypatch)
    try:
        r.upload_bsdfs(seventy.bsdfs)
        assert r.tri_kind_bits(0).shape == (0,)
        r.upload_triangles(seventy.xs, seventy.ys, seventy.zs, seventy.mat_id)
        assert np.array_equal(r.tri_kind_bits(70), _expected(seventy.mat_id, seventy.bsdfs))
        r.upload_bsdfs(seventy.bsdfs[:1])   # one record, Oren-Nayar: every other id is out of range
        assert _types(seventy.bsdfs)[0] == BS_OREN and not r.tri_kind_bits(70).any()
    finally:
        r.close()


# ---- (b) kernel arguments against the device array ------------------------------------------------------------------
def test_cornell_inline_against_array(pkg, monkeypatch, cornell):
    out = []
    for inline in (True, False):
        r = _ctx(pkg, monkeypatch, inline)
        try:
            r.upload_scene(cornell)
            out.append(_render(r))
        finally:
            r.close()
    (m0, v0, d0), (m1, v1, d1) = out
    assert m0 == m1 and v0 == v1
    assert d0["ggx_parked"] > 0
    for key in ("ggx_parked", "ggx_resumed", "ggx_shaded_full"):
        assert d0[key] == d1[key], (key, d0, d1)


# ---- (c) a soup beyond the kernel arguments' two words --------------------------------------------------------------
def test_seventy_triangles_batched_against_unbatched(pkg, monkeypatch, seventy):
    films = []
    for cull in (True, False):
        r = _ctx(pkg, monkeypatch, cull=cull)
        try:
            r.upload_scene(seventy)
            a = _render(r, 32)
            b = _render(r, 0)
        finally:
            r.close()
        assert a[:2] == b[:2]
        assert a[2]["ggx_parked"] == a[2]["ggx_resumed"] > 0 and b[2]["ggx_parked"] == 0, (a[2], b[2])
        films.append(a[:2])
    assert films[0] == films[1]


# ---- (d) one long-lived context follows replaced BSDFs and a replaced soup ------------------------------------------
def _fresh(pkg, monkeypatch, sc, inline):
    r = _ctx(pkg, monkeypatch, inline)
    try:
        r.upload_scene(sc)
        return _render(r)
    finally:
        r.close()


def _hits(d):
    """GGX hits below the cap: parked, or shaded at once because the wave's queue was full"""
    return d["ggx_parked"] + d["ggx_shaded_full"]


@pytest.mark.parametrize("which", ["cornell", "seventy"])
def test_replaced_bsdfs_and_soup(pkg, monkeypatch, cornell, seventy, which):
    sc = {"cornell": cornell, "seventy": seventy}[which]
    n = sc.mat_id.shape[0]
    t = _types(sc.bsdfs)
    oren_row = sc.bsdfs[np.flatnonzero(t == BS_OREN)[0]]
    no_ggx = sc.bsdfs.copy()
    no_ggx[np.isin(t, (BS_GGX_DIEL, BS_GGX_COND))] = oren_row
    moved = pkg.host_scene.ArrayScene(sc.xs, sc.ys, sc.zs, np.roll(sc.mat_id, 5), sc.bsdfs, sc.lights, sc.inf_lights, sc.camera)
    assert not np.array_equal(_expected(moved.mat_id, sc.bsdfs), _expected(sc.mat_id, sc.bsdfs))
    plain = pkg.host_scene.ArrayScene(sc.xs, sc.ys, sc.zs, sc.mat_id, no_ggx, sc.lights, sc.inf_lights, sc.camera)
    inline = which == "cornell"   # (the larger soup's table is a device array either way)
    r = _ctx(pkg, monkeypatch, inline)
    try:
        r.upload_scene(sc)
        first = _render(r)
        assert first[2]["ggx_parked"] > 0
        r.upload_bsdfs(no_ggx)
        assert not r.tri_kind_bits(n).any()
        got = _render(r)
        assert got[2]["ggx_parked"] == 0 and got[:2] == _fresh(pkg, monkeypatch, plain, inline)[:2]
        r.upload_bsdfs(sc.bsdfs)
        back = _render(r)
        assert back[2]["ggx_parked"] > 0 and back[:2] == first[:2]
        r.upload_triangles(moved.xs, moved.ys, moved.zs, moved.mat_id)
        assert np.array_equal(r.tri_kind_bits(n), _expected(moved.mat_id, sc.bsdfs))
        got = _render(r)
        want = _fresh(pkg, monkeypatch, moved, inline)
        assert got[:2] == want[:2] and _hits(got[2]) == _hits(want[2]) and got[2]["ggx_parked"] > 0
        r.upload_triangles(sc.xs, sc.ys, sc.zs, sc.mat_id)
        back = _render(r)
        assert back[:2] == first[:2] and _hits(back[2]) == _hits(first[2])
    finally:
        r.close()
