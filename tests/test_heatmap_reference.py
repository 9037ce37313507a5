"""Pins tests/heatmap_reference.py, the restatement the heatmap tests compare
the engine with: the scipy -> R conversion by a brute-force complete linkage,
the dendrogram reorder by a hand-worked tree, the distance, the range and the
block mean by direct formulas.  No GPU, no libscc."""
import numpy as np
from scipy.spatial.distance import pdist

import heatmap_reference as H


def test_complete_linkage_conversion_matches_brute_force():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((6, 9))
    d = pdist(X)
    merge, height, order = H.hclust_complete(d, 6)
    mb, hb, ob = H.hclust_complete_brute(d, 6)
    assert np.array_equal(merge, mb)
    assert np.array_equal(height, hb)  # both are entries of d
    assert np.array_equal(order, ob)
    assert set(height.tolist()) <= set(d.tolist())
    assert H.is_valid_tree(merge, 6)
    assert sorted(order.tolist()) == [1, 2, 3, 4, 5, 6]


def test_reorder_hand_worked():
    # merges (-1, -2), (-3, 1); weights 3, 1, 2: node 1 becomes (-2, -1) with value 2;
    # the root's children tie at 2 and keep (-3, 1); the order is 3, 2, 1
    merge = np.array([[-1, -2], [-3, 1]], np.int32)
    mo, order = H.dendro_reorder(merge, np.array([3.0, 1.0, 2.0]))
    assert mo.tolist() == [[-2, -1], [-3, 1]]
    assert order.tolist() == [3, 2, 1]
    # the input is not modified, and the reordered tree holds the same leaf sets
    assert merge.tolist() == [[-1, -2], [-3, 1]]
    assert H.leaf_sets(mo) == H.leaf_sets(merge)


def test_reorder_puts_lighter_child_first():
    # ((1, 2), 3) with weights 5, 7, 1: node 1 = 6 > 1, so leaf 3 moves to the left
    merge = np.array([[-1, -2], [-3, 1]], np.int32)
    mo, order = H.dendro_reorder(merge, np.array([5.0, 7.0, 1.0]))
    assert mo.tolist() == [[-1, -2], [-3, 1]] and order.tolist() == [3, 1, 2]
    mo, order = H.dendro_reorder(merge, np.array([5.0, 7.0, 9.0]))
    assert mo.tolist() == [[-1, -2], [1, -3]] and order.tolist() == [1, 2, 3]


def test_gene_dist_is_packed_pdist():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((7, 31))
    d = H.gene_dist(X)
    np.testing.assert_allclose(d.astype(np.float64), pdist(X), rtol=1e-14)
    assert d[H.packed_index(7, 5, 2)] == d[H.packed_index(7, 2, 5)]
    np.testing.assert_allclose(float(d[H.packed_index(7, 2, 5)]), np.linalg.norm(X[2] - X[5]), rtol=1e-14)
    X[4] = X[1]
    assert H.gene_dist(X)[H.packed_index(7, 1, 4)] == 0


def test_range_and_means():
    X = np.array([[0.0, -2.0, 0.0], [1.5, 0.25, 3.0]])
    assert H.value_range(X).tolist() == [-2.0, 3.0, 0.0, 3.0]
    np.testing.assert_allclose(H.row_means(X).astype(np.float64), [-2.0 / 3.0, 4.75 / 3.0], rtol=2e-16)


def test_raster_bins():
    X = np.arange(12.0).reshape(2, 6)
    assert H.bin_edges(6, 4) == [0, 1, 3, 4, 6]
    r, bound = H.raster(X, [2, 1], [6, 5, 4, 3, 2, 1], 4)
    assert r.astype(float).tolist() == [[11.0, 9.5, 8.0, 6.5], [5.0, 3.5, 2.0, 0.5]]
    full, _ = H.raster(X, [2, 1], [6, 5, 4, 3, 2, 1], 6)
    assert np.array_equal(full.astype(float), X[::-1, ::-1])
    assert bound[0, 1] == 2 * 2.0 ** -53 * 9.5
