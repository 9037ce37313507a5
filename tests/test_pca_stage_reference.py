"""CPU checks of tests/pca_stage_reference.py: the references are exact, the
integer construction holds its invariants, and the "sensitive" float inputs do
defeat plain fp64 (so a kernel that lost its low word, or formed the Gram in
one pass, cannot meet the bounds the GPU tests assert)."""
from fractions import Fraction

import numpy as np
import pytest

import pca_stage_reference as R


def test_two_prod_and_two_sum_are_exact():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(200) * 10.0 ** rng.integers(-8, 9, 200)
    b = rng.standard_normal(200) * 10.0 ** rng.integers(-8, 9, 200)
    p, e = R.two_prod(a, b)
    s, t = R.two_sum(a, b)
    for i in range(200):
        assert Fraction(p[i]) + Fraction(e[i]) == Fraction(a[i]) * Fraction(b[i])
        assert Fraction(s[i]) + Fraction(t[i]) == Fraction(a[i]) + Fraction(b[i])


@pytest.mark.parametrize("kind", ["counts", "mean_dominated", "cancelling"])
def test_dd_gram_equals_fraction_gram(kind):
    n, nu = 40, 7
    X = {"counts": R.lognormal_counts_panel, "mean_dominated": R.mean_dominated_panel,
         "cancelling": R.cancelling_columns}[kind](n, nu, 3)
    m = R.exact_mean_rounded(X)
    hi, lo = R.dd_gram(X, m)
    F = R.fraction_gram(X, m)
    mh, ml = R.centre_dd(X, m)
    A = (np.abs(mh) + np.abs(ml)).T @ (np.abs(mh) + np.abs(ml))
    for i in range(nu):
        for j in range(nu):
            got = Fraction(float(hi[i, j])) + Fraction(float(lo[i, j]))
            # n accurate dd additions (3 u^2 each) and the dropped l*l terms (u^2 each): < 8 n u^2 A
            assert abs(got - F[i][j]) <= Fraction(8 * n, 2 ** 106) * Fraction(float(A[i, j]))
            assert abs(hi[i, j] - float(F[i][j])) <= np.spacing(abs(float(F[i][j])))
    assert np.array_equal(hi, hi.T)


def test_dd_project_equals_fraction_product():
    n, nu, k = 9, 11, 3
    X = R.lognormal_counts_panel(n, nu, 4) + 0.1
    m = R.exact_mean_rounded(X)
    V = np.random.default_rng(4).standard_normal((nu, k))
    hi, lo = R.dd_project(X, m, V)
    Xc = X - m
    for c in range(n):
        for q in range(k):
            ex = sum(Fraction(float(Xc[c, u])) * Fraction(float(V[u, q])) for u in range(nu))
            assert abs(hi[c, q] - float(ex)) <= np.spacing(abs(float(ex)))


@pytest.mark.parametrize("n,nu", [(1, 5), (2, 3), (17, 65), (1100, 70), (2050, 449)])
def test_integer_panel_invariants(n, nu):
    X = R.integer_panel(n, nu, seed=n + nu)
    assert X.dtype == np.int64 and X.shape == (n, nu)
    assert np.all(X.sum(axis=0) % n == 0)
    assert int(np.abs(X).max()) <= 512 + n  # the last row moves by less than n
    Xc = R.centred_int(X)
    assert np.all(Xc.sum(axis=0) == 0)
    G = Xc.T @ Xc
    assert int(np.abs(G).max(initial=0)) < 2 ** 53
    # fp64 reproduces the int64 Gram exactly, in another summation order too
    Xf = Xc.astype(np.float64)
    assert np.array_equal(Xf.T @ Xf, G.astype(np.float64))
    assert np.array_equal(Xf[::-1].T @ Xf[::-1], G.astype(np.float64))
    if (n, nu) == (1100, 70):
        assert int(np.abs(X).max()) <= 1611 and int(np.abs(G).max()) < 4e8


def test_exact_colsum_and_round_to_dd():
    X = np.array([[1e16, 1.0], [1.0, 2.0 ** -60], [-1e16, 1.0]])
    s = R.exact_colsum(X)
    assert s[0] == 1 and s[1] == 2 + Fraction(1, 2 ** 60)
    hi, lo = R.round_to_dd(s[1])
    assert hi == 2.0 and lo == 2.0 ** -60


def test_plain_sums_violate_the_colsum_bound():
    """The cancelling columns defeat np.sum (pairwise) and a sequential fp64
    sum by more than 2^30 times the bound the double-double kernel must meet."""
    X = R.cancelling_columns(1500, 4, seed=11)
    exact = R.exact_colsum(X)
    bound = R.colsum_bound(X)
    for name, s in (("np.sum", R.plain_colsum_np(X)), ("sequential", R.plain_colsum_sequential(X))):
        worst = max(abs(Fraction(float(s[j])) - exact[j]) / bound[j] for j in range(X.shape[1]))
        print(f"{name}: worst error / bound = {float(worst):.3e}")
        assert worst >= 2 ** 30, name
    # the double-double sum the kernels use does meet it (NumPy restatement)
    h = np.zeros(4)
    l = np.zeros(4)
    for c in range(X.shape[0]):
        h, l = R.dd_add(h, l, X[c], np.zeros(4))
    for j in range(4):
        assert abs(Fraction(float(h[j])) + Fraction(float(l[j])) - exact[j]) <= bound[j]


def test_one_pass_gram_violates_the_gram_bound():
    X = R.mean_dominated_panel(1100, 6, seed=12)
    m = R.exact_mean_rounded(X)
    hi, _ = R.dd_gram(X, m)
    bound = R.gram_bound(X)
    worst = np.max(np.abs(R.one_pass_gram(X) - hi) / bound)
    print(f"one-pass Gram: worst error / bound = {worst:.3e}")
    assert worst > 1e3
    # the two-pass fp64 Gram (centre, then multiply) meets it
    Xc = X - m
    assert np.all(np.abs(Xc.T @ Xc - hi) <= bound)
