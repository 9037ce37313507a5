"""CPU: the NumPy restatement of the UMAP stages (umap_reference) has the
properties the device tests rely on: the bisection's defining property, the
fuzzy union's structure against scipy.sparse, draws that are in range and do not
depend on the evaluation order, and a layout that organises blob data."""
import numpy as np
import pytest
import scipy.sparse as sp

import umap_reference as ur


@pytest.fixture(scope="module")
def blob600():
    x, lab = ur.blobs(600, dim=8, n_blobs=6, seed=11)
    idx, dist = ur.knn_table(x, 15)
    return x, lab, idx, dist


@pytest.mark.parametrize("k", [1, 2, 14, 15, 16, 32, 64])
def test_bisection_reaches_the_target_or_the_floor(blob600, k):
    x = blob600[0]
    idx, dist = ur.knn_table(x, k)
    rho, sigma, mid, floor = ur.smooth_knn(dist)
    assert np.array_equal(rho, dist[:, 0])  # tie-free blobs: the first distance is the smallest positive one
    ps = ur.psum_at(dist, rho, sigma)
    hit = np.abs(ps - np.log2(k + 1.0)) < ur.TOL
    floored = sigma == floor
    print(f"k={k}: rows at the target {int(hit.sum())}, at the floor {int(floored.sum())}")
    assert np.all(hit | floored)
    # Blob inputs never reach the floor, except at k = 2: there psum = 1 + exp(-(d2 - d1) / mid), and a
    # row whose two distances nearly tie needs a mid below a thousandth of their mean.
    assert k == 2 or not floored.any()


def test_rows_without_a_positive_distance_and_constant_rows():
    dist = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0], [1.5, 1.5, 1.5], [1.0, 2.0, 3.0]])
    rho, sigma, mid, floor = ur.smooth_knn(dist)
    assert list(rho) == [0.0, 2.0, 1.5, 1.0]
    assert sigma[0] == floor[0] == ur.FLOOR * (ur.fixed_total(dist.sum(axis=1)) / 12.0)  # the global mean
    assert mid[0] == 2.0 ** -64 and mid[2] == 2.0 ** -64  # psum stays k > log2(k + 1): the bisection runs out
    assert sigma[2] == ur.FLOOR * 1.5
    w = ur.directed_weights(dist, rho, sigma)
    assert np.all(w[0] == 1.0) and np.all(w[1] == 1.0) and np.all(w[2] == 1.0) and w[3, 0] == 1.0


def test_fixed_total_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (1, 7, 1024, 1025, 5000):
        x = rng.random(n)
        assert abs(ur.fixed_total(x) - x.sum()) <= 1e-12 * x.sum()


@pytest.mark.parametrize("mix", [1.0, 0.5, 0.0])
def test_union_structure_matches_scipy(blob600, mix):
    _, _, idx, dist = blob600
    n, k = idx.shape
    indptr, cols, vals, rho, sigma = ur.fuzzy_graph(idx, dist, mix)
    w = ur.directed_weights(dist, rho, sigma)
    A = sp.csr_matrix((w.reshape(-1), (np.repeat(np.arange(n), k), idx.reshape(-1))), shape=(n, n))
    P = A.multiply(A.T)
    ref = (mix * (A + A.T - P) + (1.0 - mix) * P).tocsr()
    ref.eliminate_zeros()
    ref.sort_indices()
    got = sp.csr_matrix((vals, cols, indptr), shape=(n, n))
    assert got.has_sorted_indices or np.all([np.all(np.diff(cols[indptr[r]:indptr[r + 1]]) > 0) for r in range(n)])
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(cols, ref.indices)
    np.testing.assert_allclose(vals, ref.data, rtol=1e-14, atol=0)
    assert abs(got - got.T).max() == 0.0  # symmetric to the bit
    assert vals.min() > 0.0 and vals.max() <= 1.0


def test_union_drops_self_entries_and_builds_hub_rows():
    n, k = 300, 4
    idx = np.empty((n, k), np.int32)
    for i in range(n):
        others = [j for j in range(1, n) if j != i][: k - 1] if i else []
        idx[i] = [0] + others if i else [1, 2, 3, 4]
    idx[7, 3] = 7  # its own row: dropped
    w = np.full((n, k), 0.5)
    indptr, cols, vals = ur.union_csr(idx, w)
    assert indptr[1] - indptr[0] == n - 1 and np.array_equal(cols[:n - 1], np.arange(1, n))
    r7 = cols[indptr[7]:indptr[8]]
    assert 7 not in r7


def test_draws_are_in_range_and_order_free():
    rng = np.random.default_rng(3)
    for n in (2, 3, 17, 1025, 1 << 27):
        ctr = rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        v = ur.draw(12345, ctr, n)
        assert v.min() >= 0 and v.max() < n
        perm = rng.permutation(len(ctr))
        assert np.array_equal(ur.draw(12345, ctr[perm], n), v[perm])  # all at once, in another order
        assert [int(ur.draw(12345, ctr[t:t + 1], n)[0]) for t in range(64)] == list(v[:64])  # one by one
    v = ur.draw(0, np.arange(200000, dtype=np.uint64), 10)
    assert np.all(np.abs(np.bincount(v, minlength=10) / 20000.0 - 1.0) < 0.05)  # and spread evenly
    assert not np.array_equal(ur.draw(1, np.arange(64), 1000), ur.draw(2, np.arange(64), 1000))
    c = ur.counters(3, 1000, np.array([5, 6]), np.array([0, 2]))
    assert list(c) == [(3005 << 16), (3006 << 16) + 2]


def test_layout_of_blobs_improves_on_its_initialisation(blob600):
    from sklearn.manifold import trustworthiness
    x, lab, idx, dist = blob600
    assert ur.label_purity(x, lab) == 1.0
    indptr, cols, vals, _, _ = ur.fuzzy_graph(idx, dist)
    init = ur.pca_init(x)
    st = {}
    y = ur.layout(indptr, cols, vals, init, n_epochs=200, seed=1, stats=st)
    again = ur.layout(indptr, cols, vals, init, n_epochs=200, seed=1)
    assert np.array_equal(y, again) and np.all(np.isfinite(y))
    t0, t1 = trustworthiness(x, init, n_neighbors=15), trustworthiness(x, y, n_neighbors=15)
    pur = ur.label_purity(y, lab)
    print(f"trustworthiness {t0:.4f} -> {t1:.4f}, purity {pur:.4f}, extent {np.ptp(y, axis=0)}, "
          f"attractions {st['attractions']}, draws {st['draws']}")
    assert t1 > t0
    assert pur >= 0.99
    assert ur.schedule_counts(indptr, vals, 200) == (st["attractions"], st["draws"])
    assert not np.array_equal(y, ur.layout(indptr, cols, vals, init, n_epochs=200, seed=2))


def test_isolated_vertices_stay_and_inputs_are_untouched(blob600):
    idx, dist = ur.knn_table(blob600[0][:40], 8)
    indptr, cols, vals, _, _ = ur.fuzzy_graph(idx, dist)
    indptr = np.concatenate([indptr, [indptr[-1]] * 3])  # three vertices without edges
    init = np.random.default_rng(2).normal(size=(43, 2))
    keep = [a.copy() for a in (indptr, cols, vals, init)]
    y = ur.layout(indptr, cols, vals, init, n_epochs=10)
    assert np.array_equal(y[40:], init[40:]) and not np.array_equal(y[:40], init[:40])
    assert all(np.array_equal(a, b) for a, b in zip(keep, (indptr, cols, vals, init)))


def test_fitted_constants_are_the_default_pair():
    a, b = ur.find_ab_params(1.0, 0.1)
    assert abs(a - ur.A_DEFAULT) < 1e-6 * a and abs(b - ur.B_DEFAULT) < 1e-6 * b
