"""CPU tests of the BVH refit's host side: the serial restatement of the device refit (dmt_bvh_refit_reference) on trees
of the LBVH restatement.  A refit is a pure function of (topology, new positions): with the soup a tree was built from it
reproduces every byte, with other positions it gives a valid tree of the same topology.  No GPU needed."""
import numpy as np
import pytest

from test_bvh_gpu_build_gpu import _soup_for
from test_lbvh import CHILD_BASE, LEAF_REF, META

AMPLITUDES = (0.01, 0.1, 1.0, 5.0)


def deform(soup, amplitude, phase=0.0):
    """The soup with every vertex displaced by a smooth field, p + A sin(1.3 p' + phase) with the axes rotated (wavelength
    4.8 scene units, many triangles long: neighbours move together, as a deforming mesh's do)."""
    xs, ys, zs = (np.array(a, np.float32).reshape(-1, 4) for a in soup)
    p = np.stack([xs[:, :3], ys[:, :3], zs[:, :3]], -1).astype(np.float64)
    d = amplitude * np.sin(1.3 * p[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.0]) + phase)
    q = (p + d).astype(np.float32)
    out = [np.zeros_like(xs) for _ in range(3)]
    for a in range(3):
        out[a][:, :3] = q[..., a]
    return tuple(out)


def permuted(soup, seed=7):
    """The same triangles handed out to other indices: every pair of the old topology now holds two unrelated triangles."""
    xs, ys, zs = (np.asarray(a, np.float32).reshape(-1, 4) for a in soup)
    perm = np.random.default_rng(seed).permutation(xs.shape[0])
    return xs[perm].copy(), ys[perm].copy(), zs[perm].copy()


def topology(nodes):
    """The words a refit must leave alone: inner | count nibbles, childBase, leafRef of every node."""
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 64)
    return nodes[:, META + 3].copy(), nodes[:, CHILD_BASE:CHILD_BASE + 4].copy(), nodes[:, LEAF_REF:LEAF_REF + 4].copy()


def _tree(pkg, soup):
    r = pkg.lbvh_reference(*soup)
    assert not r["abandoned"]
    return r["nodes"], r["pairs"]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 26, 777, 20000])
def test_refit_with_the_build_soup_is_the_identity(pkg, n):
    soup = _soup_for(pkg, n)
    nodes, pairs = _tree(pkg, soup)
    out = pkg.bvh_refit_reference(nodes, pairs, *soup)
    if not np.array_equal(out, nodes):
        bad = np.flatnonzero((out != nodes).any(axis=1))
        raise AssertionError(f"{bad.size} of {nodes.shape[0]} nodes differ, first {bad[:8]}: refit {out[bad[0]].tolist()} built {nodes[bad[0]].tolist()}")
    assert pkg.bvh_check(out, pairs, *soup)["ok"]


@pytest.mark.parametrize("amplitude", AMPLITUDES)
@pytest.mark.parametrize("n", [5, 777, 20000])
def test_refit_to_a_deformed_soup_is_a_valid_tree_of_the_same_topology(pkg, n, amplitude):
    soup = _soup_for(pkg, n)
    nodes, pairs = _tree(pkg, soup)
    moved = deform(soup, amplitude)
    out = pkg.bvh_refit_reference(nodes, pairs, *moved)
    c = pkg.bvh_check(out, pairs, *moved)
    assert c["ok"] and c["max_leaf"] <= 2, c
    for a, b in zip(topology(out), topology(nodes)):
        assert np.array_equal(a, b)
    assert np.array_equal(out[:, 48:], nodes[:, 48:])          # the slot's padding stays zero
    if amplitude >= 0.1:
        assert not np.array_equal(out, nodes)


@pytest.mark.parametrize("n", [3, 777, 20000])
def test_refit_is_stateless(pkg, n):
    """To S' and back to S: nothing of the old boxes is read, so the tree of S comes back in every byte."""
    soup = _soup_for(pkg, n)
    nodes, pairs = _tree(pkg, soup)
    away = pkg.bvh_refit_reference(nodes, pairs, *deform(soup, 1.0))
    assert not np.array_equal(away, nodes)
    assert np.array_equal(pkg.bvh_refit_reference(away, pairs, *soup), nodes)


def test_cost_ratios_the_auto_mode_test_relies_on(pkg):
    """Preconditions of the GPU test of DMT_BVH_UPDATE_AUTO with max_cost_ratio = 2, from the restatement alone: a smooth
    displacement of 0.1 keeps the cost within 1.1x of the builder's, handing the triangles out to other indices raises it
    more than tenfold."""
    soup = _soup_for(pkg, 20000)
    nodes, pairs = _tree(pkg, soup)
    built = pkg.bvh_check(nodes, pairs, *soup)["sah_cost"]

    def ratio(moved):
        c = pkg.bvh_check(pkg.bvh_refit_reference(nodes, pairs, *moved), pairs, *moved)
        assert c["ok"]
        return c["sah_cost"] / built

    smooth, shuffled = ratio(deform(soup, 0.1)), ratio(permuted(soup))
    print(f"SAH cost over the builder's: A = 0.1 {smooth:.4f}, permuted {shuffled:.1f}")
    assert smooth < 1.1
    assert shuffled > 10


def test_inconsistent_trees_are_refused(pkg):
    soup = _soup_for(pkg, 26)
    nodes, pairs = _tree(pkg, soup)
    inner = nodes[:, META + 3] & 0xF
    count = nodes[:, META + 3] >> 4
    assert inner[0] > 0
    bad = nodes.copy()
    bad[0, CHILD_BASE:CHILD_BASE + 4] = 0                       # the root's first child would be the root
    with pytest.raises(pkg.DmtError, match=r"\(3\)"):           # DMT_ERR_STATE
        pkg.bvh_refit_reference(bad, pairs, *soup)
    leafy = int(np.flatnonzero(count > inner)[0])
    bad = nodes.copy()
    bad[leafy, LEAF_REF:LEAF_REF + 4] = np.array([0x80000000 + pairs.shape[0]], np.uint32).view(np.uint8)
    with pytest.raises(pkg.DmtError, match=r"\(3\)"):
        pkg.bvh_refit_reference(bad, pairs, *soup)
    bad_pairs = pairs.copy()
    bad_pairs[0, 1] = 26                                        # a triangle outside the soup
    with pytest.raises(pkg.DmtError, match=r"\(3\)"):
        pkg.bvh_refit_reference(nodes, bad_pairs, *soup)


def test_empty_soup_gives_the_one_node_tree(pkg):
    z = np.zeros((0, 4), np.float32)
    r = pkg.lbvh_reference(z, z, z)
    assert r["nodes"].shape == (1, 64) and r["pairs"].shape[0] == 0
    assert np.array_equal(pkg.bvh_refit_reference(r["nodes"], r["pairs"], z, z, z), r["nodes"])


def test_the_binding_lists_the_new_symbols(pkg):
    from cuda_optix_pathtracing_amd import binding
    for s in ("dmt_update_vertices", "dmt_update_vertices_device", "dmt_set_accel_update", "dmt_accel_update_info", "dmt_bvh_refit_reference"):
        assert s in binding.EXPORTED_SYMBOLS and hasattr(pkg.load_library(), s)
    assert (pkg.BVH_UPDATE_REBUILD, pkg.BVH_UPDATE_REFIT, pkg.BVH_UPDATE_AUTO) == (0, 1, 2)
    assert (pkg.BVH_UPDATED_NONE, pkg.BVH_UPDATED_REFIT, pkg.BVH_UPDATED_REBUILD, pkg.BVH_UPDATED_REBUILD_AFTER_REFIT) == (0, 1, 2, 3)
