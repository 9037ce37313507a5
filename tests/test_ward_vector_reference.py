"""The centroid NN-chain (ward_vector_reference, the algorithm of
scc_hclust_ward_d2_scores) against the host tree on the distance matrix.

Seeded 15-dimensional Gaussian blobs, the recipe of
test_gpu_hclust_dev._packed("blobs", n).  The two routes round differently
(a weighted mean of centroids against the Lance-Williams update of squared
distances), so the heights agree within a bound and the merges exactly as long
as no two candidate dissimilarities lie within rounding of each other.

The bound: this chain in numpy against scipy's Lance-Williams Ward linkage on
``pdist`` of such blobs gave a worst relative height error of 3.5e-16 at
n = 65, 9.4e-16 at n = 1025 and 1.6e-15 at n = 3000, while the smallest
relative gap between consecutive heights was 2.4e-4, 1.1e-6 and 1.4e-7.
1e-12 leaves three orders of margin over the error and lies five orders below
the smallest gap, so it cannot hide a wrong merge.  The condition on the input
(smallest relative gap of the host heights >= 1e-9) is asserted first.
"""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

import ward_vector_reference as wv
from scconsensus_amd import _native as nat


@pytest.mark.parametrize("n", [65, 1025, 3000])
def test_centroid_chain_equals_host_tree(n):
    x = wv.blobs(n)
    m, h, o = nat.hclust_ward_d2(pdist(x), n)
    wv.assert_tie_free(h)
    mv, hv, ov, scans = wv.ward_vector_tree(x)
    assert np.array_equal(mv, m)
    assert np.array_equal(ov, o)
    rel = np.max(np.abs(hv - h) / h)
    print(f"n={n}: worst relative height error {rel:.3g}, smallest gap {wv.min_relative_gap(h):.3g}, scans {scans}")
    assert rel <= 1e-12
    assert n - 1 <= scans < 3 * n


def test_blobs_are_the_existing_recipe():
    """The points whose pdist test_gpu_hclust_dev._packed("blobs", n) returns."""
    n = 65
    rng = np.random.default_rng(1000 * n)
    k = max(1, min(8, n // 8))
    centers = rng.normal(scale=6.0, size=(k, 15))
    x = centers[rng.integers(0, k, n)] + rng.normal(size=(n, 15))
    assert np.array_equal(wv.blobs(n), x)


def test_duplicates_merge_at_zero_and_tree_is_valid():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 4, size=(65, 2)).astype(np.float64)
    m, h, o, _ = wv.ward_vector_tree(x)
    n_dup = len(x) - len(np.unique(x, axis=0))
    assert np.count_nonzero(h == 0.0) == n_dup
    assert np.all(np.diff(h) >= 0)
    assert sorted(o.tolist()) == list(range(1, 66))
