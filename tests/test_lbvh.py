"""CPU tests of the LBVH builder's host side: the serial restatement of the device builder (dmt_lbvh_reference), the
tree checker (dmt_bvh_check), the exports and the CLI flag.  No GPU needed."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host_side import _soup

EXE = ROOT / "cuda-optix-pathtracing_amd" / "host" / "dmt-megakernel-hip"

# byte offsets in a 64-byte node (csrc/bvh.hpp Bvh4Node)
META, CHILD_BASE, LEAF_REF, QLOX, QHIX = 12, 16, 20, 24, 28


def _checked(pkg, xs, ys, zs, max_depth=48):
    r = pkg.lbvh_reference(xs, ys, zs, max_depth)
    assert not r["abandoned"]
    c = pkg.bvh_check(r["nodes"], r["pairs"], xs, ys, zs)
    n = np.asarray(xs).size // 4
    assert c["ok"], c
    assert c["max_leaf"] <= 2 and c["depth"] <= 48 and c["depth"] == r["depth"]
    assert (n + 1) // 2 <= c["pair_count"] <= max(n, 0)            # n / 2 <= pairs <= n
    assert 1 <= c["node_count"] <= max(n, 1)
    return r, c


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 26, 1000, 50000])
def test_lbvh_reference_invariants(pkg, n):
    xs, ys, zs = _soup(n, n + 1)
    r, c = _checked(pkg, xs, ys, zs)
    if n == 0:
        assert c["node_count"] == 1 and c["pair_count"] == 0 and r["depth"] == 0   # a root without children
    if n == 1:
        assert c["node_count"] == 1 and r["pairs"].tolist() == [[0, 0]]            # a one-triangle leaf repeats its triangle
    if n == 2:
        assert c["node_count"] == 1 and sorted(r["pairs"][0].tolist()) == [0, 1]   # a root with one pair


def test_lbvh_reference_degenerate_inputs(pkg):
    # all triangles identical: every Morton code equal, the triangle index alone orders the keys
    xs, ys, zs = _soup(1, 3)
    xs, ys, zs = np.repeat(xs, 300, 0), np.repeat(ys, 300, 0), np.repeat(zs, 300, 0)
    _checked(pkg, xs, ys, zs)
    # collinear centroids, zero-area triangles: two centroid axes of zero extent
    xs, ys, zs = _soup(200, 4)
    ys[:] = 0; zs[:] = 0
    _checked(pkg, xs, ys, zs)
    # the reference's scene
    s = pkg.host_scene.cornell_box()
    _checked(pkg, s.xs, s.ys, s.zs)
    # far from the origin: the absolute padding terms decide whether the boxes still hold their triangles
    xs, ys, zs = _soup(3000, 11, spread=20.0, size=0.5)
    xs[:, :3] += np.float32(1e4)
    _checked(pkg, xs, ys, zs)


def test_lbvh_reference_is_deterministic(pkg):
    xs, ys, zs = _soup(20000, 5)
    a, b = pkg.lbvh_reference(xs, ys, zs), pkg.lbvh_reference(xs, ys, zs)
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["pairs"].tobytes() == b["pairs"].tobytes()
    assert np.all(a["nodes"][:, 48:] == 0)                                          # the slot's padding is written, as zeros


def test_depth_guard(pkg):
    """300 identical triangles: three 4-wide levels hold at most 64 leaves = 128 triangles, so a bound of 3 must abandon
    the build whatever the tree's shape; the default bound does not."""
    xs, ys, zs = _soup(1, 3)
    xs, ys, zs = np.repeat(xs, 300, 0), np.repeat(ys, 300, 0), np.repeat(zs, 300, 0)
    r = pkg.lbvh_reference(xs, ys, zs, max_depth=3)
    assert r["abandoned"] and r["nodes"].shape[0] == 0 and r["pairs"].shape[0] == 0
    assert not pkg.lbvh_reference(xs, ys, zs)["abandoned"]
    deep = pkg.lbvh_reference(xs, ys, zs)["depth"]
    assert pkg.lbvh_reference(xs, ys, zs, max_depth=deep - 1)["abandoned"]
    assert not pkg.lbvh_reference(xs, ys, zs, max_depth=deep)["abandoned"]


def test_bvh_check_rejects_damaged_trees(pkg):
    """A checker that cannot fail proves nothing."""
    xs, ys, zs = _soup(1000, 1001)
    r = pkg.lbvh_reference(xs, ys, zs)
    nodes, pairs = r["nodes"], r["pairs"]
    assert pkg.bvh_check(nodes, pairs, xs, ys, zs)["ok"]
    two = int(np.flatnonzero(pairs[:, 0] != pairs[:, 1])[0])
    # a triangle listed twice (in the place of a triangle of another leaf)
    p = pairs.copy()
    other = (two + 1) % len(p)
    p[other, 0] = p[two, 0]
    assert not pkg.bvh_check(nodes, p, xs, ys, zs)["ok"]
    # one missing: a pair turned into a one-triangle leaf
    p = pairs.copy()
    p[two, 1] = p[two, 0]
    assert not pkg.bvh_check(nodes, p, xs, ys, zs)["ok"]
    # one pair short
    assert not pkg.bvh_check(nodes, pairs[:-1], xs, ys, zs)["ok"]
    # a plane byte lowered so that a vertex falls outside: the upper x plane of the root's first child next to its lower one
    d = nodes.copy()
    assert d[0, QHIX] > d[0, QLOX] + 1
    d[0, QHIX] = d[0, QLOX] + 1
    assert not pkg.bvh_check(d, pairs, xs, ys, zs)["ok"]
    # childBase pointing at a foreign node
    d = nodes.copy()
    assert (d[0, META + 3] & 0xF) >= 1                                              # the root has inner children
    d[0, CHILD_BASE:CHILD_BASE + 4].view(np.uint32)[0] += 1
    assert not pkg.bvh_check(d, pairs, xs, ys, zs)["ok"]
    # a leaf reference moved to the neighbouring pair
    d = nodes.copy()
    leafy = int(np.flatnonzero((d[:, META + 3] >> 4) > (d[:, META + 3] & 0xF))[0])
    d[leafy, LEAF_REF:LEAF_REF + 4].view(np.uint32)[0] += 1
    assert not pkg.bvh_check(d, pairs, xs, ys, zs)["ok"]
    # the soup moved under the tree
    assert not pkg.bvh_check(nodes, pairs, xs + np.float32(0.5), ys, zs)["ok"]


def test_bvh_check_sah_cost(pkg):
    """One pair under the root: the cost is the pair's box area, counted twice, over the same area."""
    xs, ys, zs = _soup(2, 9)
    r = pkg.lbvh_reference(xs, ys, zs)
    assert pkg.bvh_check(r["nodes"], r["pairs"], xs, ys, zs)["sah_cost"] == 2.0
    xs, ys, zs = _soup(50000, 50001)
    r = pkg.lbvh_reference(xs, ys, zs)
    cost = pkg.bvh_check(r["nodes"], r["pairs"], xs, ys, zs)["sah_cost"]
    assert 100 < cost < 5000                                                        # ~ leaves x (leaf area / root area) x tree overhead


def test_new_entry_points_are_exported(pkg):
    lib = pkg.load_library()
    from cuda_optix_pathtracing_amd import binding
    for name in ("dmt_set_accel_build", "dmt_accel_build_info", "dmt_accel_download", "dmt_lbvh_reference", "dmt_bvh_check"):
        assert hasattr(lib, name) and name in binding.EXPORTED_SYMBOLS
    for name in ("lbvh_reference", "bvh_check", "BVH_BUILD_HOST", "BVH_BUILD_DEVICE"):
        assert hasattr(pkg, name)
    for name in ("set_accel_build", "accel_build_info", "download_accel"):
        assert hasattr(pkg.Renderer, name)
    blob = pkg.library_path().read_bytes()
    assert b"k_fit" in blob and b"k_level_emit" in blob                             # the builder's kernels are in the code object


# ---- CLI -------------------------------------------------------------------------------------------------------------
def _run(*args):
    assert EXE.exists(), "run __graft_entry__.build()"
    return subprocess.run([str(EXE), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, message", [
    (("--bvh", "--bvh-build", "fast"), "invalid --bvh-build"),
    (("--bvh-build", "gpu"), "--bvh-build needs --bvh"),
    (("--bvh", "--bvh-build"), "missing value"),
])
def test_cli_rejects_bad_bvh_build_values_before_any_gpu_call(args, message):
    r = _run(*args)
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert "dmt_ctx_create" not in r.stderr and "Running HIP Kernel" not in r.stdout


def test_cli_help_lists_the_flag():
    h = _run("--help")
    assert h.returncode == 0 and "--bvh-build <host|gpu>" in h.stdout
