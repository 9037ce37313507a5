"""The k nearest neighbours of every row of a square distance matrix, in the
engine's order (scc_knn_scores): by (distance ascending, index ascending), the
row itself left out.  np.lexsort's last key is the primary one."""
import numpy as np


def knn_from_square(square, k):
    """(idx int32 [n, k], dist float64 [n, k]) of a square matrix, k <= n - 1."""
    D = np.asarray(square, np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and 1 <= k <= n - 1
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k))
    j = np.arange(n)
    for i in range(n):
        order = np.lexsort((j, D[i]))
        order = order[order != i][:k]
        idx[i] = order
        dist[i] = D[i, order]
    return idx, dist


def lattice(n, seed=None):
    """Integer lattice points in 15 dimensions: distances tie exactly and
    massively, so only the tie rule decides the neighbours."""
    rng = np.random.default_rng(77 * n if seed is None else seed)
    return rng.integers(0, 3, (n, 15)).astype(np.float64)


def min_relative_gap(dist_sorted):
    """Per row, the smallest relative gap between consecutive distances."""
    d = np.asarray(dist_sorted, np.float64)
    return np.min(np.diff(d, axis=1) / d[:, 1:], axis=1)
