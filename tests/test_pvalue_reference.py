"""CPU: pin the high-precision p-value references (tests/pvalue_reference.py)
before the GPU sweeps (tests/test_gpu_pvalues.py) trust them.

Each reference is compared with an independent implementation (scipy) and with
the oracle's double-precision restatement of R; the oracle's worst relative
deviation from the reference is printed and stands in every assertion message
(DESIGN.md §1 quotes these figures next to the kernel's).

Bars (none of them taken from what the code under test returns):
  exact Wilcoxon  the oracle and scipy sum at most mn/2 + 1 <= 1,201 positive
                  double quotients: rounding <= 1,201 * 2^-53 = 1.3e-13.  Bar 1e-12.
  normal tail     Cody's rational forms are good to ~1e-16; what is left is
                  exp(-z^2 / 2) of an argument up to 704 rounded in double:
                  704 * 2^-52 = 1.6e-13 relative.  Bar 1e-12.
  Student t       the oracle sums up to 4e7 positive long-double terms
                  (4e7 * 2^-64 = 2e-12) under a prefactor exp(a log x - lbeta) with
                  |a log x| <= 670 in double (1.5e-13).  Bar 1e-10, a tenth of the
                  1e-9 the kernel is held to.  scipy (Boost's ibeta in double) is
                  held to the same 1e-10.
  chi-square      closed form; scipy's igamc in double with exp(-x / 2) as
                  above.  Bar 1e-12."""
import math

import mpmath as mp
import numpy as np
import pytest
from scipy import stats

import oracle as O
import pvalue_reference as R

SIZES = range(3, 50)


def _rel(a, ref):
    return abs(a - ref) / ref if ref > 0 else (0.0 if a == ref else math.inf)


def _sample_with_u(m, n, U):
    """Tie-free x (m values), y (n values) whose Mann-Whitney U of x is U."""
    full, r = divmod(U, n)
    y = np.arange(1, n + 1, dtype=float)
    x = np.r_[n + 1.0 + np.arange(full), ([r + 0.5] if full < m else []), -1.0 - np.arange(max(m - full - 1, 0))]
    assert len(x) == m
    return x, y


def _oracle_exact_p(U, m, n):
    """wilcox.test's rule on the oracle's pwilcox."""
    if U > m * n / 2:
        p = O.pwilcox(U - 1, m, n, lower_tail=False)
    else:
        p = O.pwilcox(U, m, n, lower_tail=True)
    return min(2 * p, 1.0)


def test_u_counts_are_a_distribution():
    for m, n in [(3, 3), (3, 49), (20, 21), (49, 49)]:
        c = R.u_counts(m, n)
        assert len(c) == m * n + 1 and sum(c) == math.comb(m + n, n)
        assert c == c[::-1] and c[0] == 1 and R.u_counts(n, m) == c
    # brute force over every arrangement of a small case
    from itertools import combinations
    m, n = 4, 5
    cnt = [0] * (m * n + 1)
    for pos in combinations(range(m + n), m):
        cnt[sum(p - i for i, p in enumerate(pos))] += 1
    assert tuple(cnt) == R.u_counts(m, n)
    # R's documented identity: the smallest two-sided exact p is 2 / choose(m + n, n)
    assert R.wilcox_exact_p(0, 4, 4) == 2 / math.comb(8, 4)
    assert R.wilcox_exact_p(2 * 16, 4, 4) == 2 / math.comb(8, 4)
    assert R.wilcox_exact_p(2 * 8, 4, 4) == 1.0


def test_exact_wilcoxon_vs_scipy_and_oracle():
    """Every 3 <= m, n <= 49 (both orientations) at a spread of U."""
    rng = np.random.default_rng(11)
    worst_o, worst_s, at_o, at_s = 0.0, 0.0, None, None
    for m in SIZES:
        for n in SIZES:
            mn = m * n
            for U in {0, 1, mn // 2, mn // 2 + 1, mn, int(rng.integers(0, mn + 1))}:
                ref = R.wilcox_exact_p(2 * U, m, n)
                eo = _rel(_oracle_exact_p(U, m, n), ref)
                x, y = _sample_with_u(m, n, U)
                res = stats.mannwhitneyu(x, y, alternative="two-sided", method="exact")
                assert res.statistic == U
                es = _rel(res.pvalue, ref)
                if eo > worst_o:
                    worst_o, at_o = eo, (U, m, n)
                if es > worst_s:
                    worst_s, at_s = es, (U, m, n)
    msg = f"exact Wilcoxon, worst relative deviation: oracle {worst_o:.2e} at {at_o}, scipy {worst_s:.2e} at {at_s}"
    print(msg)
    assert worst_o < 1e-12 and worst_s < 1e-12, msg


def test_normal_tail_vs_oracle():
    worst, at = 0.0, None
    for a in R.Z_GRID + list(np.linspace(0.01, 37.51, 751)):
        for z in (a, -a):
            ref = R.normal_small_tail(z)
            got = min(O.pnorm(z, True), O.pnorm(z, False))
            if not abs(z) < R.PNORM_CUTOFF:
                assert ref == 0.0 and got == 0.0, z
                continue
            assert ref == pytest.approx(0.5 * math.erfc(abs(z) / math.sqrt(2)), rel=1e-9, abs=1e-320)  # the reference itself
            if ref >= 1e-300:
                e = _rel(got, ref)
                if e > worst:
                    worst, at = e, z
    assert math.isnan(R.normal_small_tail(math.nan))
    msg = f"normal tail, worst relative deviation of the oracle: {worst:.2e} at z = {at}"
    print(msg)
    assert worst < 1e-12, msg


def test_wilcox_normal_reference_vs_oracle():
    """The reference's z and p of the normal branch against the oracle's
    wilcox.test on samples that realise (U, T): sizes from 50 up, ties."""
    rng = np.random.default_rng(3)
    worst, at = 0.0, None
    for m, n, levels in [(50, 3, 0), (3, 50, 0), (49, 49, 7), (60, 75, 0), (200, 180, 5), (1000, 900, 0),
                         (1000, 1000, 3)]:
        for shift in (0.0, 0.4, 3.0):
            x, y = rng.normal(shift, 1, m), rng.normal(0, 1, n)
            if levels:
                x, y = np.round(x * levels / 3), np.round(y * levels / 3)
            po, W, T, meth = O.wilcox_test(x, y)
            assert meth == "normal"
            u2, tie = int(round(2 * W)), int(round(T))
            ref = R.wilcox_normal_p(u2, tie, m, n)
            z = R.wilcox_z(u2, tie, m, n)
            # the 50-digit z against the double z (R's operation order) that decides the cut-off
            if ref > 0.0:
                assert ref == pytest.approx(2 * R.normal_small_tail(z), rel=1e-14 * max(1.0, z * z), abs=1e-320)
            if ref >= 1e-300:
                e = _rel(po, ref)
                if e > worst:
                    worst, at = e, (m, n, shift, levels)
            else:
                assert po <= 1e-300
    msg = f"wilcox.test normal branch, worst relative deviation of the oracle: {worst:.2e} at {at}"
    print(msg)
    # z itself carries a few roundings (relative ~4 eps), which the tail turns
    # into z^2 * 4 eps <= 1,408 * 8.9e-16 = 1.3e-12 at the cut-off
    assert worst < 2e-12, msg


def test_t_excluded_share_of_the_grid():
    """The GPU sweep only bounds p below 1e-290 from above; that may cover at
    most 30 % of its grid."""
    grid = R.t_grid()
    small = sum(1 for t, df in grid if R.t_two_sided_p_mp(t, df) < R.P_FLOOR)
    share = small / len(grid)
    print(f"Welch t grid: {len(grid)} points, {small} with p < {R.P_FLOOR:g} ({100 * share:.1f} %)")
    assert share <= 0.30, share


def test_t_reference_vs_scipy_and_oracle():
    worst_o, worst_s, worst_n = {}, 0.0, 0.0
    at_s = at_n = None
    for t, df in R.t_grid():
        pm = R.t_two_sided_p_mp(t, df)
        ref = float(pm)
        if math.isinf(t):
            assert ref == 0.0 and 2 * O.pt(-abs(t), df) == 0.0
            continue
        if t == 0.0:
            assert ref == 1.0
        if pm < R.P_FLOOR:
            continue
        regime = ("normal df > 4e5" if df > R.PT_NORMAL_DF else
                  "nx > 1e100" if 1 + (t / df) * t > 1e100 else "df > t^2" if df > t * t else "df <= t^2")
        eo = _rel(2 * O.pt(-abs(t), df), ref)
        if eo > worst_o.get(regime, (0.0, None))[0] or regime not in worst_o:
            worst_o[regime] = (eo, (t, df))
        # scipy returns the true t tail: compare it with the true tail (the
        # beta route at any df), and note how far R's normal formula is from it
        with mp.workdps(R.DPS):
            true = float(R._t_beta_mp(t, df))
        es = _rel(2 * stats.t.sf(abs(t), df), true)
        if es > worst_s:
            worst_s, at_s = es, (t, df)
        if df > R.PT_NORMAL_DF:
            en = _rel(ref, true)
            if en > worst_n:
                worst_n, at_n = en, (t, df)
    msg = ("Welch t, worst relative deviation from the reference: oracle " +
           ", ".join(f"{k}: {v[0]:.2e} at (t, df) = {v[1]}" for k, v in sorted(worst_o.items())) +
           f"; scipy from the true tail {worst_s:.2e} at {at_s}; R's df > 4e5 formula from the true tail "
           f"{worst_n:.2e} at {at_n}")
    print(msg)
    assert len(worst_o) == 4, msg                   # every regime of pt is on the grid
    assert max(v[0] for v in worst_o.values()) < 1e-10, msg
    assert worst_s < 1e-10, msg


def test_t_regime_nx_1e100():
    """df = 2, |t| = 1e60: pt's asymptotic branch.  For df = 2 the tail has the
    closed form 1 - |t| / sqrt(2 + t^2) = 1 / t^2 (1 - 3 / (2 t^2) + ...)."""
    ref = R.t_two_sided_p(1e60, 2.0)
    assert ref == pytest.approx(1e-120, rel=1e-15)
    assert 2 * O.pt(-1e60, 2.0) == pytest.approx(ref, rel=1e-10)
    assert R.t_two_sided_p(3.0, 2.0) == pytest.approx(1 - 3 / math.sqrt(11), rel=1e-15)


def test_t_two_mpmath_routes_agree():
    """The beta-function route (series / continued fraction) against quadrature
    of the t density, to 1e-30, on a subset that visits each of its branches."""
    pts = [(0.5, 2.0), (1e5, 2.0), (2.0, 7.5), (37.0, 7.5), (1e-3, 19.9), (100.0, 50.0), (5.0, 137.3),
           (math.sqrt(137.3) * (1 + 1e-9), 137.3), (math.sqrt(137.3) * (1 - 1e-9), 137.3), (10.0, 1e3),
           (2.0, 12345.6), (1.0, 1e5), (37.0, 1e5), (0.1, 4e5), (5.0, 4e5)]
    for t, df in pts:
        with mp.workdps(R.DPS):
            a, b = R.t_two_sided_p_mp(t, df), R.t_two_sided_p_quad_mp(t, df)
            assert abs(a - b) <= mp.mpf("1e-30") * a, (t, df, a, b)


def test_pchisq3_reference():
    assert R.pchisq3_upper(-math.inf) == 1.0 and R.pchisq3_upper(-1.0) == 1.0 and R.pchisq3_upper(0.0) == 1.0
    assert R.pchisq3_upper(math.inf) == 0.0 and math.isnan(R.pchisq3_upper(math.nan))
    worst = 0.0
    for x in [1e-300, 1e-8, 1e-3, 0.5, 1.0, 10.0, 100.0, 700.0, 1400.0]:
        ref = R.pchisq3_upper(x)
        worst = max(worst, _rel(stats.chi2.sf(x, 3), ref))
    print(f"pchisq(df = 3) upper tail, worst relative deviation of scipy: {worst:.2e}")
    assert worst < 1e-12, worst
    assert R.pchisq3_upper(1500.0) < 1e-300
