"""High-precision references for the engine's p-value functions.

Plain Python: big integers, ``fractions.Fraction`` and ``mpmath`` at 50 digits.
No engine and no oracle code is in here; tests/test_pvalue_reference.py pins
these functions to scipy and to the oracle, tests/test_gpu_pvalues.py checks the
device functions against them.

Every function takes the doubles (or integers) the device function receives
and returns the double nearest to what R's rule gives in exact arithmetic:

  wilcox_exact_p(u2, m, n)       wilcox.test's exact two-sided p (no ties)
  wilcox_normal_p(u2, tie, m, n) its continuity-corrected normal approximation
  wilcox_z(u2, tie, m, n)        the z of that approximation, in double, R's order
  normal_small_tail(z)           min(pnorm(z), pnorm(-z)) with R's cut-off
  t_two_sided_p(t, df)           2 pt(-|t|, df)
  pchisq3_upper(x)               pchisq(x, 3, lower.tail = FALSE)

The ``*_mp`` variants return the mpmath number before the one rounding (p below
the double range stays a positive mpf, so "below 1e-290" can be asked of it).
"""
import math
from fractions import Fraction
from functools import lru_cache

import mpmath as mp

DPS = 50
PNORM_CUTOFF = 37.5193      # R nmath/pnorm.c: the tail beyond is returned as 0
PT_NORMAL_DF = 4e5          # R nmath/pt.c: normal approximation above
P_FLOOR = 1e-290            # below: R returns 0 or a denormal, which of the two is not pinned

# The grids of the sweeps (shared by the CPU pin and the GPU sweep).
# Welch's df is at least min(n) - 1 = 2; |t| up to 1 / (10 eps), the limit the
# "data are essentially constant" rule leaves; sqrt(df) (1 +- 1e-9) each side
# of the n > x^2 switch is added per df.
T_DF_GRID = [2.0, 2.0001, 2.7, 4.0, 7.5, 19.9, 20.1, 50.0, 137.3, 1e3, 12345.6, 1e5, 3.99e5, 4e5, 4.0001e5, 1e6,
             1e9]
T_ABS_GRID = [0.0, 1e-300, 1e-12, 1e-6, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 37.0, 100.0, 1e3, 1e5, 1e8, 1e12, 4e14]
# z: 0, each side of Cody's two branch changes (and of the eps / 2 rule inside
# the first), the third branch out to the cut-off, and beyond it
_HALF_EPS, _B1, _B2 = 1.1102230246251565e-16, 0.67448975, 5.656854249492380195206754896838
Z_GRID = [0.0, _HALF_EPS, math.nextafter(_HALF_EPS, 1.0), 1e-300, 0.3, math.nextafter(_B1, 0.0), _B1,
          math.nextafter(_B1, 1.0), 1.0, 3.0, 5.65685, math.nextafter(_B2, 0.0), _B2, math.nextafter(_B2, 6.0), 5.65686,
          10.0, 20.0, 30.0, 37.0, 37.5, 37.519, math.nextafter(PNORM_CUTOFF, 0.0), PNORM_CUTOFF, 37.52, 38.5, 40.0,
          1e3, math.inf]
CHISQ_GRID = [-math.inf, -1.0, 0.0, 1e-300, 1e-8, 1.0, 10.0, 100.0, 1400.0, 1500.0, math.inf, math.nan]


def t_grid():
    """(t, df) of the Welch sweep: both signs of every |t|, +-Inf included."""
    out = []
    for df in T_DF_GRID:
        r = math.sqrt(df)
        for a in T_ABS_GRID + [r * (1 - 1e-9), r * (1 + 1e-9), math.inf]:
            out.append((a, df))
            if a != 0.0:
                out.append((-a, df))
    # pt's nx > 1e100 branch, which no t.test reaches (|t| <= 1 / (10 eps))
    out += [(1e60, 2.0), (-1e60, 2.0)]
    return out


def wilcox_u_grid(m, n, rng):
    """U values of the exact sweep at sizes (m, n): both ends, around mn / 2
    (where pwilcox switches tails and wilcox.test picks stat - 1), 8 seeded."""
    mn = m * n
    fixed = [0, 1, 2, mn // 2 - 1, mn // 2, mn // 2 + 1, mn - 1, mn]
    return fixed + [int(v) for v in rng.integers(0, mn + 1, 8)]


# ------------------------------------------------------------------ Wilcoxon, exact
@lru_cache(maxsize=None)
def _u_counts_sorted(i, j):
    """Number of arrangements of i x's and j y's (i <= j) with U = k, k = 0..ij:
    c(i, j, k) = c(i - 1, j, k - j) + c(i, j - 1, k), c(0, j, .) = [1]."""
    if i == 0:
        return (1,)
    a = u_counts(i - 1, j)          # shifted by j
    b = u_counts(i, j - 1)
    out = [0] * (i * j + 1)
    for k, v in enumerate(b):
        out[k] = v
    for k, v in enumerate(a):
        out[k + j] += v
    return tuple(out)


def u_counts(m, n):
    """Counts of the Mann-Whitney U distribution of sample sizes m and n
    (symmetric in m, n), as Python integers."""
    return _u_counts_sorted(min(m, n), max(m, n))


@lru_cache(maxsize=None)
def _u_cum_sorted(i, j):
    out, run = [], 0
    for v in _u_counts_sorted(i, j):
        run += v
        out.append(run)
    return tuple(out)


def wilcox_exact_fraction(u2, m, n):
    """R's two-sided exact p as a Fraction: with stat = u2 / 2, the lower tail
    P(U <= stat) or, when stat > mn / 2, the upper tail P(U > stat - 1);
    doubled and capped at 1 (pwilcox floors its argument)."""
    cum = _u_cum_sorted(min(m, n), max(m, n))      # cum[q] = #{U <= q}
    total = math.comb(m + n, n)
    assert cum[-1] == total

    def below(q):
        return 0 if q < 0 else cum[min(q, m * n)]
    stat = Fraction(int(u2), 2)
    if stat > Fraction(m * n, 2):
        tail = total - below(math.floor(stat - 1))
    else:
        tail = below(math.floor(stat))
    return min(Fraction(2 * tail, total), Fraction(1))


def wilcox_exact_p(u2, m, n):
    return float(wilcox_exact_fraction(u2, m, n))


# ------------------------------------------------------------------ normal
def normal_small_tail_mp(z):
    """The normal tail beyond |z| (no cut-off), at DPS digits."""
    with mp.workdps(DPS):
        return mp.ncdf(-abs(mp.mpf(z)))


def normal_small_tail(z):
    """min(pnorm(z), pnorm(z, lower.tail = FALSE)) as R returns it: exactly 0
    once |z| reaches the cut-off, NaN for NaN."""
    z = float(z)
    if z != z:
        return z
    if not abs(z) < PNORM_CUTOFF:
        return 0.0
    return float(normal_small_tail_mp(z))


def wilcox_z(u2, tie, m, n):
    """wilcox.test.default's z in double arithmetic and R's operation order
    (the number its pnorm sees, which decides the cut-off)."""
    dnx, dny = float(m), float(n)
    z = float(u2) * 0.5 - dnx * dny / 2
    sigma = math.sqrt((dnx * dny / 12) * ((dnx + dny + 1) - float(tie) / ((dnx + dny) * (dnx + dny - 1))))
    corr = 0.5 if z > 0 else (-0.5 if z < 0 else 0.0)
    return (z - corr) / sigma


def wilcox_normal_p_mp(u2, tie, m, n):
    with mp.workdps(DPS):
        mn = mp.mpf(m) * n
        N = mp.mpf(m) + n
        z = mp.mpf(int(u2)) / 2 - mn / 2
        sigma = mp.sqrt((mn / 12) * ((N + 1) - mp.mpf(int(tie)) / (N * (N - 1))))
        corr = mp.mpf(0.5) if z > 0 else (mp.mpf(-0.5) if z < 0 else mp.mpf(0))
        return 2 * mp.ncdf(-abs((z - corr) / sigma))


def wilcox_normal_p(u2, tie, m, n):
    """R's continuity-corrected two-sided normal p with the tie-corrected sigma;
    exactly 0 where the double z is beyond pnorm's cut-off."""
    if not abs(wilcox_z(u2, tie, m, n)) < PNORM_CUTOFF:
        return 0.0
    return float(wilcox_normal_p_mp(u2, tie, m, n))


# ------------------------------------------------------------------ Student t
def _ibeta_prefix(a, b, x, y):
    """x^a y^b / B(a, b) with y = 1 - x given separately."""
    return mp.exp(a * mp.log(x) + b * mp.log(y) - (mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)))


def _ibeta_series(a, b, x, y):
    """I_x(a, b) by DLMF 8.17.8, x^a y^b / (a B) sum (a+b)_n / (a+1)_n x^n:
    positive terms, ratio below x.  Used for x <= 1/2 only."""
    s = term = mp.mpf(1)
    tol = mp.mpf(10) ** (-(mp.mp.dps + 5))
    n = 0
    while term > tol * s:
        term *= (a + b + n) / (a + 1 + n) * x
        s += term
        n += 1
        if n > 200000:
            raise ArithmeticError("incomplete beta series did not converge")
    return _ibeta_prefix(a, b, x, y) / a * s


def _ibeta_cf(a, b, x, y):
    """I_x(a, b) by the continued fraction DLMF 8.17.22 (modified Lentz), for
    x below (a + 1) / (a + b + 2) where it converges quickly."""
    tiny = mp.mpf(10) ** (-10 * mp.mp.dps)
    tol = mp.mpf(10) ** (-(mp.mp.dps + 5))
    K, C, D = mp.mpf(1), mp.mpf(1), mp.mpf(0)
    for j in range(1, 2000000):
        m = j >> 1
        if j & 1:
            d = -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))
        else:
            d = m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m))
        D = 1 + d * D
        D = 1 / (D if D != 0 else tiny)
        C = 1 + d / C
        if C == 0:
            C = tiny
        cd = C * D
        K *= cd
        if abs(cd - 1) < tol:
            return _ibeta_prefix(a, b, x, y) / (a * K)
    raise ArithmeticError("incomplete beta continued fraction did not converge")


def _t_beta_mp(t, df):
    """I_x(df / 2, 1 / 2), x = df / (df + t^2): the series on the side where
    its argument is at most 1/2, the continued fraction in between."""
    t2 = mp.mpf(t) ** 2
    n = mp.mpf(df)
    x, y = n / (n + t2), t2 / (n + t2)
    a, b = n / 2, mp.mpf(1) / 2
    if y == 0:
        return mp.mpf(1)
    if x <= mp.mpf(1) / 2:
        return _ibeta_series(a, b, x, y)
    if x < (a + 1) / (a + b + 2):
        # below the distribution's bulk: p can be tiny, so it is computed
        # directly and never as 1 - (the other side)
        return _ibeta_cf(a, b, x, y)
    # x in the bulk or above (p is of order 1): the complement's series in
    # y <= (b + 1) / (a + b + 2) <= 3/7, whose terms never grow
    return 1 - _ibeta_series(b, a, y, x)


def t_two_sided_p_mp(t, df):
    """2 pt(-|t|, df) at DPS digits (mpf; 0 only for |t| = Inf)."""
    t, df = float(t), float(df)
    with mp.workdps(DPS):
        if t != t or df != df:
            return mp.nan
        if math.isinf(t):
            return mp.mpf(0)
        if df > PT_NORMAL_DF:
            # R: pnorm(x (1 - 1/(4n)) / sqrt(1 + x^2 / (2n))) for n > 4e5
            x, n = mp.mpf(abs(t)), mp.mpf(df)
            return 2 * mp.ncdf(-x * (1 - 1 / (4 * n)) / mp.sqrt(1 + x * x / (2 * n)))
        return +_t_beta_mp(t, df)


def t_two_sided_p(t, df):
    return float(t_two_sided_p_mp(t, df))


def t_two_sided_p_quad_mp(t, df):
    """The same tail by quadrature of the t density over [|t|, Inf): a second
    route that shares nothing with the beta-function code above but lgamma.
    (Slow: for cross-checking a subset only.)"""
    t, df = abs(float(t)), float(df)
    with mp.workdps(DPS + 15):
        n = mp.mpf(df)
        lc = mp.loggamma((n + 1) / 2) - mp.loggamma(n / 2) - mp.log(n * mp.pi) / 2
        t0 = mp.mpf(t)
        # the factor at t0 is taken out so the integrand is 1 at the left end
        l0 = -(n + 1) / 2 * mp.log1p(t0 * t0 / n)

        def f(u):
            return mp.exp(-(n + 1) / 2 * mp.log1p(u * u / n) - l0)

        # local decay length of the density at t0, then doubling steps out to
        # the polynomial tail
        s = (n + t0 * t0) / ((n + 1) * t0) if t0 > 1 else mp.mpf(1)
        pts = [t0]
        step = s
        while len(pts) < 40 and pts[-1] < 64 * (mp.sqrt(n) + t0):
            pts.append(pts[-1] + step)
            step *= 2
        pts.append(mp.inf)
        return +(2 * mp.exp(lc + l0) * mp.quad(f, pts))


# ------------------------------------------------------------------ chi-square, 3 df
def pchisq3_upper_mp(x):
    with mp.workdps(DPS):
        x = mp.mpf(x)
        return mp.erfc(mp.sqrt(x / 2)) + mp.sqrt(2 * x / mp.pi) * mp.exp(-x / 2)


def pchisq3_upper(x):
    """pchisq(x, df = 3, lower.tail = FALSE) in closed form; R's IEEE cases:
    1 for x <= 0 (-Inf included), 0 for +Inf, NaN for NaN."""
    x = float(x)
    if x != x:
        return x
    if x <= 0.0:
        return 1.0
    if math.isinf(x):
        return 0.0
    return float(pchisq3_upper_mp(x))
