"""libscc's two host functions for the heatmap's gene rows (include/scc.h):
scc_hclust_complete = stats::hclust(d, "complete") and scc_dendro_reorder =
stats::reorder.dendrogram(as.dendrogram(tree), wts, agglo.FUN = mean), through
ctypes against tests/heatmap_reference.py.  Host code: no GPU needed."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

import heatmap_reference as H
from scconsensus_amd import _native as nat


@pytest.mark.parametrize("n", [2, 3, 64, 500])
def test_complete_matches_reference(n):
    # continuous random distances: no ties, so the complete-linkage tree is unique
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 7)) * rng.uniform(0.2, 3.0, (n, 1))
    d = pdist(X)
    assert len(np.unique(d)) == len(d)
    merge, height, order = nat.hclust_complete(d, n)
    mr, hr, orr = H.hclust_complete(d, n)
    assert np.array_equal(merge, mr)
    assert np.array_equal(order, orr)
    assert height.tobytes() == hr.tobytes()  # bitwise
    assert np.isin(height, d).all()  # heights are entries of the input, unmodified
    assert np.all(np.diff(height) >= 0)


def test_complete_with_duplicated_rows():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((40, 5))
    X[23] = X[7]
    d = pdist(X)
    assert d[H.packed_index(40, 7, 23)] == 0.0
    merge, height, order = nat.hclust_complete(d, 40)
    assert height[0] == 0.0 and merge[0].tolist() == [-8, -24]
    assert np.array_equal(np.sort(height), np.sort(linkage(d, "complete")[:, 2]))
    assert H.is_valid_tree(merge, 40)
    assert sorted(order.tolist()) == list(range(1, 41))
    assert np.array_equal(order, H.merge_order(merge))


def test_complete_rejects_bad_input():
    with pytest.raises(nat.SccError) as e:
        nat.hclust_complete(np.array([1.0, np.inf, 2.0]), 3)
    assert e.value.code == nat.SCC_ERR_NONFINITE
    with pytest.raises(ValueError):
        nat.hclust_complete(np.array([1.0, 2.0]), 3)


def test_reorder_hand_worked():
    mo, order = nat.dendro_reorder(np.array([[-1, -2], [-3, 1]], np.int32), [3.0, 1.0, 2.0])
    assert mo.tolist() == [[-2, -1], [-3, 1]]
    assert order.tolist() == [3, 2, 1]


@pytest.mark.parametrize("n", [2, 3, 17, 300])
def test_reorder_matches_reference_on_random_trees(n):
    rng = np.random.default_rng(1000 + n)
    merge, _, _ = nat.hclust_complete(pdist(rng.standard_normal((n, 4))), n)
    for trial in range(3):
        # trial 2: integer weights, so that sibling values tie and the stable rule decides
        w = rng.standard_normal(n) if trial < 2 else rng.integers(0, 3, n).astype(np.float64)
        mo, order = nat.dendro_reorder(merge, w)
        mr, orr = H.dendro_reorder(merge, w)
        assert np.array_equal(mo, mr)
        assert np.array_equal(order, orr)
        # the same tree: equal leaf sets under every node, rows only swapped
        assert H.leaf_sets(mo) == H.leaf_sets(merge)
        assert np.array_equal(np.sort(mo, axis=1), np.sort(merge, axis=1))
        assert sorted(order.tolist()) == list(range(1, n + 1))


def test_reorder_chain_tree_is_not_recursive():
    # a caterpillar of 50,000 leaves: as deep as it is long
    n = 50000
    merge = np.zeros((n - 1, 2), np.int32)
    merge[0] = [-1, -2]
    merge[1:, 0] = -np.arange(3, n + 1)
    merge[1:, 1] = np.arange(1, n - 1)
    w = np.arange(n, dtype=np.float64)
    mo, order = nat.dendro_reorder(merge, w)
    # every leaf k >= 3 (weight k - 1) is heavier than the mean below it: it moves to the right
    assert np.array_equal(order, np.arange(1, n + 1))
    assert np.array_equal(mo[1:, 0], np.arange(1, n - 1)) and np.array_equal(mo[1:, 1], -np.arange(3, n + 1))


def test_reorder_rejects_a_non_tree():
    with pytest.raises(nat.SccError) as e:
        nat.dendro_reorder(np.array([[-1, -2], [-1, 1]], np.int32), [1.0, 2.0, 3.0])
    assert e.value.code == nat.SCC_ERR_INVALID
