"""CPU: the neighbour reference the GPU tests compare with (knn_reference)
against sklearn's brute-force NearestNeighbors on blobs, where no two
distances of a row tie, and on an integer lattice, where nearly all do and
only the (distance, index) rule decides."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform
from sklearn.neighbors import NearestNeighbors

import knn_reference as kr
import ward_vector_reference as wv


@pytest.mark.parametrize("n,k", [(17, 1), (17, 16), (257, 15), (1025, 64)])
def test_reference_matches_sklearn_on_blobs(n, k):
    x = wv.blobs(n)
    sq = squareform(pdist(x))
    idx, dist = kr.knn_from_square(sq, k)
    nn = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x)
    sd, si = nn.kneighbors(x)
    assert np.array_equal(si[:, 0], np.arange(n))  # the point itself first: no duplicates in the blobs
    assert np.array_equal(idx, si[:, 1:])
    # sklearn's brute force expands |a|^2 - 2 a.b + |b|^2: a few ulp of the squared norms (~1e2) in d^2
    np.testing.assert_allclose(dist, sd[:, 1:], rtol=1e-9)


def test_reference_excludes_self_and_orders_rows():
    sq = squareform(pdist(wv.blobs(65)))
    idx, dist = kr.knn_from_square(sq, 64)
    assert all(i not in idx[i] for i in range(65))
    assert all(sorted(idx[i]) == [j for j in range(65) if j != i] for i in range(65))
    assert np.all(np.diff(dist, axis=1) >= 0)


@pytest.mark.parametrize("n,k", [(65, 15), (1025, 64)])
def test_reference_breaks_lattice_ties_by_index(n, k):
    x = kr.lattice(n)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)  # small integers: exact
    idx, dist = kr.knn_from_square(np.sqrt(d2), k)
    ties = 0
    for i in range(n):
        key = [(d2[i, j], j) for j in range(n) if j != i]
        key.sort()
        assert [j for _, j in key[:k]] == list(idx[i])
        ties += int(np.sum(np.diff(dist[i]) == 0))
    assert ties > n * k // 2  # most consecutive neighbours tie exactly
    # equal distances appear in index order
    same = np.diff(dist, axis=1) == 0
    assert np.all(np.diff(idx, axis=1)[same] > 0)
