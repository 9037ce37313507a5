"""Exact references and entrywise error bounds for the PCA stage's parts
(column sums, centred Gram, projection), in plain NumPy / Python.

Nothing here depends on np.longdouble: exactness comes from int64 arithmetic
(integer panels), fractions.Fraction (column sums, small Grams) and a
double-double (Dekker / Veltkamp TwoProd, Knuth TwoSum) accumulation that is
vectorised over the output entries.

Integer panels
    integer_panel(n, nu, seed) has column sums divisible by the TOTAL cell
    count n, so the column means and every centred value are integers.  With
    max |Xc|^T |Xc| < 2^53 every product and every partial sum, in any order
    and any grouping, is an integer below 2^53: a correct fp64 kernel (FMA or
    not, any tile or chunk split) returns the int64 result exactly.

Float inputs
    cancelling_columns: values over 17 decades that cancel in pairs to ~1e-9
    relative (a plain fp64 sum loses everything; a double-double one does not).
    mean_dominated_panel: 1e6 + N(0, 1) per column, on which the one-pass
    formula X^T X - N m m^T loses ~8 digits.
    lognormal_counts_panel: sparse non-negative log1p counts (the workload's
    value distribution).

Bounds (u = 2^-53), all derived from the operation counts, not from any
measured output:
    colsum_bound   n 2^-102 sum|x|
    gram_bound     2 u [(n + 4) A_ij + 2 (|m_i| s_j + |m_j| s_i)]
    project_bound  (nu + 2) u (|Xc| |V|)_cq
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
_SPLIT = 134217729.0  # 2^27 + 1 (Veltkamp)


# ------------------------------------------------------------------ inputs
def integer_panel(n, nu, seed, lo=-512, hi=512):
    """int64 [n][nu] (cells x genes), uniform in [lo, hi], the last row lowered
    by (column sum mod n): every column sum is divisible by n.  Asserts that
    |Xc|^T |Xc| stays below 2^53 (exact fp64 arithmetic in any order)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(lo, hi + 1, size=(n, nu), dtype=np.int64)
    X[-1] -= X.sum(axis=0) % n
    assert np.all(X.sum(axis=0) % n == 0)
    Xc = centred_int(X)
    A = np.abs(Xc).T @ np.abs(Xc)
    assert int(A.max(initial=0)) < 2 ** 53, "integer panel too large for exact fp64"
    assert int(np.abs(X).sum(axis=0).max(initial=0)) < 2 ** 53
    return X


def centred_int(X, n_total=None, col_sums=None):
    """Xc = X - colsum / n_total in int64 (the division must be exact)."""
    X = np.asarray(X, np.int64)
    s = X.sum(axis=0) if col_sums is None else np.asarray(col_sums, np.int64)
    n = X.shape[0] if n_total is None else n_total
    assert np.all(s % n == 0)
    return X - s // n


def cancelling_columns(n, nu, seed):
    """[n][nu]: N(0,1) 10^k with k uniform in -8..8; every even entry is then
    minus its neighbour times (1 + 1e-9 N(0,1))."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, nu)) * 10.0 ** rng.integers(-8, 9, size=(n, nu))
    ev = np.arange(0, n - 1, 2)
    X[ev] = -X[ev + 1] * (1.0 + 1e-9 * rng.standard_normal((len(ev), nu)))
    return X


def mean_dominated_panel(n, nu, seed):
    rng = np.random.default_rng(seed)
    return 1e6 + rng.standard_normal((n, nu))


def lognormal_counts_panel(n, nu, seed, density=0.3):
    """Sparse non-negative log1p counts."""
    rng = np.random.default_rng(seed)
    cnt = rng.negative_binomial(2, 0.25, size=(n, nu)) * (rng.random((n, nu)) < density)
    return np.log1p(cnt.astype(np.float64))


# ------------------------------------------------------------------ exact sums
def exact_colsum(X):
    """Column sums of a float [n][nu] array as a list of Fractions (exact)."""
    X = np.asarray(X, np.float64)
    out = []
    for j in range(X.shape[1]):
        s = Fraction(0)
        for v in X[:, j]:
            s += Fraction(float(v))
        out.append(s)
    return out


def exact_mean_rounded(X, n_total=None, col_sums=None):
    """The exact column mean rounded once to fp64 (Fraction -> float rounds to
    nearest even)."""
    X = np.asarray(X, np.float64)
    s = exact_colsum(X) if col_sums is None else col_sums
    n = X.shape[0] if n_total is None else n_total
    return np.array([float(v / n) for v in s])


def round_to_dd(fr):
    """A Fraction as a double-double (hi = nearest double, lo = nearest double of the rest)."""
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


# ------------------------------------------------------------------ double-double
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly (no FMA: Veltkamp split, Dekker product).  Needs
    |a|, |b| < 2^996 and no underflow in the partial products."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dd_add(xh, xl, yh, yl):
    """Accurate double-double addition (error <= 3 u^2 relative)."""
    sh, sl = two_sum(xh, yh)
    th, tl = two_sum(xl, yl)
    sl = sl + th
    sh, sl = two_sum(sh, sl)
    sl = sl + tl
    return two_sum(sh, sl)


def centre_dd(X, mean):
    """X - mean as a double-double pair of arrays (exact: TwoSum)."""
    return two_sum(np.asarray(X, np.float64), -np.asarray(mean, np.float64))


def dd_matmul(Ah, Al, Bh, Bl):
    """(Ah + Al)^T-free product sum_c (Ah + Al)[c, i] (Bh + Bl)[c, j] as a
    double-double [ni][nj] pair; the l*l term (<= u^2 of the product) is
    dropped.  A: [n][ni], B: [n][nj]; the loop runs over the n terms, every
    step vectorised over (i, j)."""
    n, ni = Ah.shape
    nj = Bh.shape[1]
    if Al is None:
        Al = np.zeros_like(Ah)
    if Bl is None:
        Bl = np.zeros_like(Bh)
    sh = np.zeros((ni, nj))
    sl = np.zeros((ni, nj))
    for c in range(n):
        a, al = Ah[c][:, None], Al[c][:, None]
        b, bl = Bh[c][None, :], Bl[c][None, :]
        p, e = two_prod(a, b)
        e = e + (a * bl + al * b)
        sh, sl = dd_add(sh, sl, p, e)
    return sh, sl


def dd_gram(X, mean):
    """Gram of X centred with `mean` (the exact mean rounded once), the centred
    operands kept exact (double-double): (hi, lo) [nu][nu]."""
    h, l = centre_dd(X, mean)
    return dd_matmul(h, l, h, l)


def dd_project(X, mean, V):
    """(X - mean) V as a double-double pair, (X - mean) ROUNDED to fp64 first
    (the panel the projection kernels read)."""
    Xc = np.asarray(X, np.float64) - np.asarray(mean, np.float64)
    return dd_matmul(Xc.T.copy(), None, np.asarray(V, np.float64), None)


def fraction_gram(X, mean):
    """The same Gram in exact rational arithmetic (small shapes only)."""
    X = np.asarray(X, np.float64)
    n, nu = X.shape
    Xc = [[Fraction(float(X[c, j])) - Fraction(float(mean[j])) for j in range(nu)] for c in range(n)]
    return [[sum(Xc[c][i] * Xc[c][j] for c in range(n)) for j in range(nu)] for i in range(nu)]


# ------------------------------------------------------------------ bounds
def colsum_bound(X):
    """n 2^-102 sum|x| per column, as Fractions.

    A column sum of n values takes at most n - 1 double-double additions whose
    operands are both non-zero (adding an exact zero is exact), whatever the
    tree: the per-chunk dd + double chain, the fold of the chunk partials and
    the wave butterfly.  dd + double (TwoSum, fold the low word, FastTwoSum) is
    within 2 u^2 = 2^-105 of its exact result, dd + dd (TwoSum on both words,
    two FastTwoSum) within 3 u^2 + 13 u^3 < 2^-104; every intermediate is at
    most sum|x| (1 + 2^-100) in magnitude.  So the error is below
    n 2^-104 sum|x|, and the bound keeps a margin of 4."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    return [Fraction(n, 2 ** 102) * sum(Fraction(abs(float(v))) for v in X[:, j]) for j in range(X.shape[1])]


def gram_bound(X, n_total=None, mean=None):
    """2 u [(n + 4) A_ij + 2 (|m_i| s_j + |m_j| s_i)], A = |Xc|^T |Xc|,
    s_j = sum_c |Xc_cj|: any-order accumulation of n products (n u A), one
    rounding of each centred operand (2 u A), a mean good to one ulp shifting a
    whole column (2 u |m| s); the leading 2 covers the second-order terms."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    m = exact_mean_rounded(X, n_total) if mean is None else np.asarray(mean, np.float64)
    Xa = np.abs(X - m)
    A = Xa.T @ Xa
    s = Xa.sum(axis=0)
    am = np.abs(m)
    return 2.0 * U * ((n + 4) * A + 2.0 * (am[:, None] * s[None, :] + am[None, :] * s[:, None]))


def project_bound(Xc, V):
    """(nu + 2) u |Xc| |V|: nu fused or unfused multiply-adds in any order."""
    Xc = np.asarray(Xc, np.float64)
    return (Xc.shape[1] + 2) * U * (np.abs(Xc) @ np.abs(np.asarray(V, np.float64)))


# ------------------------------------------------------------------ plain fp64 (what must NOT pass)
def plain_colsum_np(X):
    return np.sum(np.asarray(X, np.float64), axis=0)


def plain_colsum_sequential(X):
    X = np.asarray(X, np.float64)
    s = np.zeros(X.shape[1])
    for c in range(X.shape[0]):
        s = s + X[c]
    return s


def one_pass_gram(X):
    """X^T X - N m m^T in plain fp64."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    m = X.sum(axis=0) / n
    return X.T @ X - n * np.outer(m, m)
