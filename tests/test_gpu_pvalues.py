"""GPU: the engine's p-value device functions over their whole domain.

Every differential-expression p goes through wilcox_p (exact table or normal
approximation), t_two_sided, scc_pnorm_small_tail or bimod_pchisq3_upper
(csrc/scc_select.hip, scc_common.hpp).  The datasets of the other tests reach
those functions at a few thousand arguments; here they are swept directly
through the diagnostic entry point scc_diag_pvalues (the same device functions
on arrays), and the same regimes are then driven through scc_de_run on tiny
datasets to show that k_pair_test feeds them correctly.  The reference is
tests/pvalue_reference.py (exact rationals, mpmath at 50 digits), pinned on the
CPU by tests/test_pvalue_reference.py.

Bars:
  exact Wilcoxon  1e-12 relative to the exact rational (the kernel sums at most
                  1,201 double quotients: 1.3e-13).
  normal tail     1e-12 relative where the reference is >= 1e-300, exactly 0
                  from R's cut-off |z| >= 37.5193 on, NaN for NaN.  Through
                  wilcox_p the double z carries its own roundings: with
                  A = (N + 1) / ((N + 1) - T / (N (N - 1))) the cancellation
                  factor of sigma^2, |dz / z| <= (3 + A / 2) 2^-53 and the tail
                  moves by z^2 dz / z: 1,408 * 4.5 * 1.1e-16 = 7e-13 at the
                  cut-off with A <= 3.  The sweep therefore takes A <= 3 over
                  the whole z grid, and heavy cancellation (A ~ 1e3) at |z| <= 1,
                  where the tail moves by at most 1.5 dz / z.
  Welch t         1e-9 relative where the reference is >= 1e-290 (the bar of
                  test_fast_t_test_config_a); below, finite, >= 0 and <= 1e-290.
  bimod tail      1e-9 relative (the bar of test_gpu_bimod.py), exact IEEE cases.
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

import oracle as O
import pvalue_reference as R
from scconsensus_amd import _native as nat
from test_gpu_de import _fast_compare

pytestmark = pytest.mark.gpu

SIZES = range(3, 50)


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


def _rel(got, ref):
    """Relative deviations of arrays (ref > 0)."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return np.abs(got - ref) / ref


def _report(name, err, args):
    i = int(np.argmax(err))
    msg = f"{name}: worst relative deviation {err[i]:.2e} at {args[i]}"
    print(msg)
    return msg


# ===================================================================== direct sweeps
@pytest.fixture(scope="module")
def exact_cases():
    """(u2, m, n) of the exact sweep: every 3 <= m, n <= 49 in both orientations."""
    rng = np.random.default_rng(2024)
    rows = [(2 * U, m, n) for m in SIZES for n in SIZES for U in R.wilcox_u_grid(m, n, rng)]
    return np.array(rows, np.int64)


def test_exact_wilcoxon_every_size(exact_cases):
    u2, m, n = exact_cases.T
    p, exact = nat.diag_pvalues(nat.DIAG_WILCOX, u2=u2, tie=np.zeros_like(u2), m=m, n=n)
    assert exact.all()
    ref = np.array([R.wilcox_exact_p(*row) for row in exact_cases.tolist()])
    assert (ref > 0).all() and np.isfinite(p).all() and (p <= 1.0).all()
    err = _rel(p, ref)
    msg = _report("exact Wilcoxon (kernel)", err, exact_cases.tolist())
    assert err.max() < 1e-12, msg
    # U = mn / 2 with mn even: the lower tail is above 1/2, so p is exactly 1
    mn = m * n
    mid = (mn % 2 == 0) & (u2 == mn)
    assert mid.sum() > 1000
    np.testing.assert_array_equal(p[mid], 1.0)


def test_normal_branch_at_50_cells_and_with_ties(exact_cases):
    """The same statistics with a cluster of 50 cells, or with a tie term, take
    the normal approximation."""
    u2, m, n = exact_cases.T
    zero, six, fifty = np.zeros_like(u2), np.full_like(u2, 6), np.full_like(u2, 50)
    rows = np.concatenate([np.stack([u2, six, m, n], 1),        # one tied pair of values
                           np.stack([u2, zero, fifty, n], 1),   # the size boundary, on either side
                           np.stack([u2, zero, m, fifty], 1),
                           [[2 * 1250, 0, 50, 50]]])
    p, exact = nat.diag_pvalues(nat.DIAG_WILCOX, u2=rows[:, 0], tie=rows[:, 1], m=rows[:, 2], n=rows[:, 3])
    assert not exact.any()                              # every one of the exact sweep's arguments
    # the values on a quarter of them (every size, 4 U each): the reference takes 60 us per p
    rows, p = rows[::4], p[::4]
    ref = np.array([R.wilcox_normal_p(*row) for row in rows.tolist()])
    assert (ref >= 1e-300).all()
    err = _rel(p, ref)
    msg = _report("wilcox_p normal branch below 50 cells with ties / at 50 cells", err, rows.tolist())
    assert err.max() < 1e-12, msg


def test_pnorm_tail_grid():
    z = np.array([s * a for a in R.Z_GRID for s in (1.0, -1.0)] + [math.nan])
    got = nat.diag_pvalues(nat.DIAG_PNORM, a=z)
    ref = np.array([R.normal_small_tail(v) for v in z])
    assert math.isnan(got[-1]) and math.isnan(ref[-1])
    z, got, ref = z[:-1], got[:-1], ref[:-1]
    beyond = ~(np.abs(z) < R.PNORM_CUTOFF)
    assert beyond.sum() >= 10
    np.testing.assert_array_equal(got[beyond], 0.0)     # exactly 0 from R's cut-off on
    big = ~beyond & (ref >= 1e-300)
    err = _rel(got[big], ref[big])
    msg = _report("scc_pnorm_small_tail", err, z[big].tolist())
    assert err.max() < 1e-12, msg
    low = ~beyond & ~big                                # 37.07 < |z| < 37.5193: 1e-300 > p >= 2.3e-308
    assert low.any() and np.isfinite(got[low]).all() and (got[low] > 0).all() and (got[low] < 1e-300).all()
    assert got[z == 0.0].tolist() == [0.5, 0.5]


def _tie_term(N, frac=None, untied=None):
    """sum(t^3 - t) of one group of tied values among N cells."""
    t = N - untied if untied is not None else int(N * frac)
    return t ** 3 - t


def test_wilcox_p_normal_branch_on_the_z_grid():
    """(u2, tie, m, n) built so that z lands on the z grid: sizes up to 2e5,
    a large tie term (80 % of the cells in one tied group: A = 2.05), and at
    |z| <= 1 all but 150 cells tied (A ~ 9e2: sigma^2 is what cancellation leaves)."""
    rows = []
    for m, n in [(50, 50), (49, 50), (50, 3), (1000, 1000), (300, 200000), (200000, 200000)]:
        N = m + n
        for tie, zmax in [(0, math.inf), (_tie_term(N, frac=0.8), math.inf), (_tie_term(N, untied=150), 1.0)]:
            if tie < 0 or (N <= 150 and zmax == 1.0):
                continue
            sigma = math.sqrt((m * n / 12) * ((N + 1) - tie / (N * (N - 1))))
            for a in R.Z_GRID:
                if not a <= min(zmax, 1e3):
                    continue
                for s in (1.0, -1.0):
                    # stat = mn/2 + corr + z sigma, as the nearest reachable 2U in [0, 2mn]
                    u2 = round(m * n + s * (1.0 if a > 0 else 0.0) + 2 * s * a * sigma)
                    rows.append((min(max(u2, 0), 2 * m * n), tie, m, n))
    rows = np.array(sorted(set(rows)), np.int64)
    p, exact = nat.diag_pvalues(nat.DIAG_WILCOX, u2=rows[:, 0], tie=rows[:, 1], m=rows[:, 2], n=rows[:, 3])
    assert not exact.any()
    z = np.array([R.wilcox_z(*row) for row in rows.tolist()])
    ref = np.array([R.wilcox_normal_p(*row) for row in rows.tolist()])
    # the constructed z visit Cody's three branches, the cut-off's two sides and sizes of 2e5
    az = np.abs(z)
    assert (az <= 0.67448975).sum() > 20 and ((az > 0.67448975) & (az <= 5.6568)).sum() > 20
    assert ((az > 5.6569) & (az < 37.0)).sum() > 20 and ((az > 37.0) & (az < R.PNORM_CUTOFF)).sum() >= 4
    assert (az > R.PNORM_CUTOFF).sum() >= 8 and az.max() > 500
    assert (np.abs(az - R.PNORM_CUTOFF) > 1e-12).all()  # none within rounding of the cut-off itself
    beyond = ~(az < R.PNORM_CUTOFF)
    np.testing.assert_array_equal(p[beyond], 0.0)
    big = ~beyond & (ref >= 1e-300)
    err = _rel(p[big], ref[big])
    msg = _report("wilcox_p normal branch on the z grid", err, [tuple(r) for r in rows[big].tolist()])
    assert err.max() < 1e-12, msg
    low = ~beyond & ~big
    assert np.isfinite(p[low]).all() and (p[low] > 0).all() and (p[low] < 1e-300).all()


def _t_regime(t, df):
    if df > R.PT_NORMAL_DF:
        return "normal df > 4e5"
    if 1 + (t / df) * t > 1e100:
        return "nx > 1e100"
    return "df > t^2" if df > t * t else "df <= t^2"


def test_welch_t_grid():
    grid = R.t_grid()
    t = np.array([g[0] for g in grid])
    df = np.array([g[1] for g in grid])
    got = nat.diag_pvalues(nat.DIAG_T, a=t, b=df)
    refm = [R.t_two_sided_p_mp(a, b) for a, b in grid]
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    np.testing.assert_array_equal(got[t == 0.0], 1.0)
    np.testing.assert_array_equal(got[np.isinf(t)], 0.0)
    small = np.array([r < R.P_FLOOR for r in refm])
    assert small.mean() <= 0.30
    assert (got[small] <= R.P_FLOOR).all()              # R: 0 or a denormal there
    ref = np.array([float(r) for r in refm])
    err = np.zeros(len(grid))
    err[~small] = _rel(got[~small], ref[~small])
    worst = {}
    for i in np.flatnonzero(~small & np.isfinite(t)):
        k = _t_regime(t[i], df[i])
        if k not in worst or err[i] > err[worst[k]]:
            worst[k] = i
    assert len(worst) == 4
    msg = "t_two_sided, worst relative deviation per regime: " + "; ".join(
        f"{k}: {err[i]:.2e} at (t, df) = ({float(t[i])!r}, {float(df[i])!r})" for k, i in sorted(worst.items()))
    print(msg)
    assert err.max() < 1e-9, msg
    nan = nat.diag_pvalues(nat.DIAG_T, a=np.array([math.nan, 1.0]), b=np.array([5.0, math.nan]))
    assert np.isnan(nan).all()


def test_bimod_chisq_tail_grid():
    x = np.array(R.CHISQ_GRID)
    got = nat.diag_pvalues(nat.DIAG_PCHISQ3, a=x)
    ref = np.array([R.pchisq3_upper(v) for v in x])
    assert math.isnan(got[-1]) and math.isnan(ref[-1])
    x, got, ref = x[:-1], got[:-1], ref[:-1]
    np.testing.assert_array_equal(got[x <= 0], 1.0)
    assert got[x == math.inf] == 0.0
    fin = (x > 0) & np.isfinite(x) & (ref >= 2.3e-308)    # up to 1400 (2.9e-303); at 1500 the tail is denormal
    assert fin.sum() == 6
    err = _rel(got[fin], ref[fin])
    msg = _report("bimod_pchisq3_upper", err, x[fin].tolist())
    assert err.max() < 1e-9, msg
    assert 0.0 <= got[x == 1500.0][0] < 1e-300


def test_diag_rejects_bad_arguments():
    with pytest.raises(ValueError):
        nat.diag_pvalues(nat.DIAG_T, a=np.zeros(3), b=np.zeros(2))
    with pytest.raises(nat.SccError):
        nat.diag_pvalues(nat.DIAG_WILCOX, u2=[0], tie=[0], m=[0], n=[5])
    assert len(nat.diag_pvalues(nat.DIAG_PNORM, a=np.zeros(0))) == 0


# ===================================================================== through scc_de_run
def _pairs(K):
    return [(i, j) for i in range(K - 1) for j in range(i + 1, K)]


def _brute_u2_tie(x, y):
    """2U of x against y over the definition, and sum(t^3 - t) of c(x, y)."""
    u2 = int(2 * (x[:, None] > y[None, :]).sum() + (x[:, None] == y[None, :]).sum())
    _, cnt = np.unique(np.concatenate([x, y]), return_counts=True)
    return u2, int((cnt.astype(np.int64) ** 3 - cnt).sum())


def _shard_fields(eng, ds, code, K, **kw):
    """Every (pair, gene) cell of a FAST run as the shard carries it: p, u2,
    ties and the flags byte (bit 2: the exact branch answered)."""
    P, G = K * (K - 1) // 2, ds.G
    PG = P * G
    buf = torch.zeros(eng.de_shard_bytes(K, G) // 8, dtype=torch.int64, device="cuda:0")
    eng.de_run_shard(ds, code, K, 0, G, buf.data_ptr(), test_all=True, **kw)
    eng.synchronize()
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().view(np.uint8)
    f64 = raw[: 48 * PG].view(np.float64).reshape(6, P, G)
    i64 = raw[: 48 * PG].view(np.int64).reshape(6, P, G)
    return f64[0], i64[4], i64[5], raw[48 * PG: 49 * PG].reshape(P, G)


SIZE_EDGE = [3, 4, 5, 10, 17, 25, 32, 48, 49, 50]


def _size_boundary_dataset():
    """243 cells in clusters of 3 .. 50 cells, 40 genes (see the test)."""
    rng = np.random.default_rng(77)
    K = len(SIZE_EDGE)
    code = np.repeat(np.arange(K), SIZE_EDGE).astype(np.int32)
    N, G = len(code), 40
    X = np.zeros((G, N))
    for g in range(30):                                 # continuous, positive, cluster effects of mixed size
        X[g] = rng.gamma(3.0, 0.5, N) + 0.05 + rng.uniform(0, 0.8 * (g % 4), K)[code]
    X[30] = 1.0 + code + rng.uniform(0.0, 0.9, N)       # every pair fully separated: U = 0
    X[31] = 12.0 - code + rng.uniform(0.0, 0.9, N)      # ... the other way: U = mn
    X[32] = rng.gamma(3.0, 0.5, N) + 0.05               # clusters 1 (4 cells) and 3 (10 cells): U = mn / 2 = 20
    X[32, code == 3] = 5.0 + rng.uniform(0.0, 1.0, 10)
    X[32, code == 1] = [1.25, 2.5, 8.25, 9.5]
    X[33] = rng.gamma(3.0, 0.5, N) + 0.05               # one zero cell in the whole dataset: still tie-free
    X[33, np.flatnonzero(code == 4)[2]] = 0.0
    X[34] = rng.normal(0.0, 2.0, N)                     # negative values
    X[35] = rng.gamma(3.0, 0.5, N) + 0.05               # two zeros in two clusters: that pair alone is tied
    X[35, np.flatnonzero(code == 2)[0]] = 0.0
    X[35, np.flatnonzero(code == 5)[3]] = 0.0
    X[36] = rng.normal(0.5, 2.0, N)                     # two zeros in one cluster: each of its pairs is tied
    X[36, np.flatnonzero(code == 6)[:2]] = 0.0
    for g in (37, 38, 39):                              # expression-like: half zeros, rounded values
        X[g] = np.where(rng.random(N) < 0.5, np.round(rng.gamma(2.0, 1.0, N), 1) + 0.1, 0.0)
    perm = rng.permutation(N)
    return X[:, perm], code[perm], K


def test_de_run_exact_branch_at_the_size_boundary(eng):
    """Clusters of 3, 4, 5, 10, 17, 25, 32, 48, 49 and 50 cells: every u2 equals
    the brute-force count, every p is within 1e-12 of the reference (exact
    rational below 50 cells without ties, normal otherwise), and flag bit 2 is
    set exactly where the exact branch applies."""
    X, code, K = _size_boundary_dataset()
    ds = eng.dataset_dense(X)
    g = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="all", test_all=True)
    sp, su2, stie, sfl = _shard_fields(eng, ds, code, K)
    np.testing.assert_array_equal(g.p, sp)
    np.testing.assert_array_equal(g.u2, su2)
    n_exact = n_normal = 0
    errs, where = [], []
    for p, (i, j) in enumerate(_pairs(K)):
        m, n = SIZE_EDGE[i], SIZE_EDGE[j]
        for gene in range(X.shape[0]):
            x, y = X[gene, code == i], X[gene, code == j]
            u2, tie = _brute_u2_tie(x, y)
            assert g.u2[p, gene] == u2 and stie[p, gene] == tie, (p, gene)
            exact = m < 50 and n < 50 and tie == 0
            assert bool(sfl[p, gene] & 4) == exact, (p, gene, m, n, tie)
            if tie == (m + n) ** 3 - (m + n):           # every value equal: sigma = 0, R's p is NaN
                assert np.isnan(g.p[p, gene]), (p, gene)
                continue
            ref = R.wilcox_exact_p(u2, m, n) if exact else R.wilcox_normal_p(u2, tie, m, n)
            n_exact += exact
            n_normal += not exact
            errs.append(abs(g.p[p, gene] - ref) / ref)
            where.append((p, gene, m, n, u2, tie))
    assert n_exact > 1200 and n_normal > 300
    # the constructed cases are what they claim to be
    pi = {pr: k for k, pr in enumerate(_pairs(K))}
    assert (g.u2[:, 30] == 0).all() and (g.u2[:, 31] == [2 * SIZE_EDGE[i] * SIZE_EDGE[j] for i, j in _pairs(K)]).all()
    assert g.u2[pi[(1, 3)], 32] == 40 and g.p[pi[(1, 3)], 32] == 1.0 and sfl[pi[(1, 3)], 32] & 4
    assert (stie[:, 33] == 0).all() and (X[33] == 0).sum() == 1
    assert [int(stie[pi[pr], 35]) for pr in [(2, 5), (2, 4), (5, 9)]] == [6, 0, 0]
    assert not sfl[pi[(2, 5)], 35] & 4 and sfl[pi[(2, 4)], 35] & 4
    assert all(stie[pi[pr], 36] == 6 for pr in pi if 6 in pr) and not any(sfl[pi[pr], 36] & 4 for pr in pi if 6 in pr)
    assert not any(sfl[pi[pr], g_] & 4 for pr in pi if 9 in pr for g_ in range(40))   # the 50-cell cluster: normal
    errs = np.array(errs)
    msg = _report("scc_de_run wilcox p at the size boundary", errs, where)
    assert errs.max() < 1e-12, msg


def _two_sample_with_u(m, n, U, rng):
    """Tie-free positive x (m values) and y (n values) with U(x > y) = U."""
    full, r = divmod(U, n)
    y = 1.0 + np.arange(n) / n + rng.uniform(0.0, 0.4 / n, n)           # in (1, 2), increasing
    hi = 3.0 + rng.permutation(full) / m + rng.uniform(0.0, 0.4 / m, full)
    mid = [y[r - 1] + 0.5 / n] if full < m and r > 0 else ([0.75] if full < m else [])
    lo = 0.25 + rng.permutation(max(m - full - 1, 0)) / (4 * m)
    x = np.r_[hi, mid, lo]
    assert len(x) == m
    return x, y


def test_de_run_normal_cutoff(eng):
    """Two clusters of 1,000 cells, 60 tie-free genes whose separation steps z
    from 36 to the largest reachable 38.7: p is exactly 0 from R's cut-off on
    and within 1e-12 before it; BH and the selection with zeros among the p
    agree with the oracle."""
    rng = np.random.default_rng(5)
    m = n = 1000
    G = 60
    sigma = math.sqrt((m * n / 12) * (m + n + 1))
    code = np.repeat([0, 1], m).astype(np.int32)
    X = np.zeros((G, 2 * m))
    want = []
    for gene, z in enumerate(np.linspace(36.0, 38.75, G)):
        U = min(int(round(m * n / 2 + 0.5 + z * sigma)), m * n)
        x, y = _two_sample_with_u(m, n, U, rng)
        if gene % 2:                                    # the mirrored statistic: z < 0
            x, y, U = y, x, m * n - U
        X[gene, :m], X[gene, m:] = rng.permutation(x), rng.permutation(y)
        want.append(2 * U)
    perm = rng.permutation(2 * m)
    X, code = X[:, perm], code[perm]
    ds = eng.dataset_dense(X)
    g = eng.de_run(ds, code, 2, nat.SCC_DE_FAST, fetch="all", test_all=True)
    np.testing.assert_array_equal(g.u2[0], want)
    z = np.array([R.wilcox_z(u2, 0, m, n) for u2 in want])
    ref = np.array([R.wilcox_normal_p(u2, 0, m, n) for u2 in want])
    beyond = ~(np.abs(z) < R.PNORM_CUTOFF)
    assert 15 < beyond.sum() < 35 and (np.abs(np.abs(z) - R.PNORM_CUTOFF) > 1e-6).all()
    assert want[-1] in (0, 2 * m * n)                   # the last gene is fully separated
    np.testing.assert_array_equal(g.p[0][beyond], 0.0)
    assert (ref[~beyond] > 0).all()
    err = _rel(g.p[0][~beyond], ref[~beyond])
    msg = _report("scc_de_run wilcox p before the cut-off", err, list(zip(z[~beyond].tolist(), want)))
    assert err.max() < 1e-12, msg
    gg, o = _fast_compare(eng, ds, X, code, 2)
    assert len(o.row_gene) == G and (o.row_p == 0.0).sum() == beyond.sum() and (o.row_q == 0.0).sum() >= beyond.sum()


def _welch_exact(x, y):
    """t and df of R's Welch t.test from the data in exact rational arithmetic."""
    fx, fy = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
    nx, ny = len(fx), len(fy)
    mx, my = sum(fx) / nx, sum(fy) / ny
    vx, vy = sum((v - mx) ** 2 for v in fx) / (nx - 1), sum((v - my) ** 2 for v in fy) / (ny - 1)
    sx2, sy2 = vx / nx, vy / ny
    with mp.workdps(R.DPS):
        se = mp.sqrt(mp.mpf(sx2.numerator) / sx2.denominator + mp.mpf(sy2.numerator) / sy2.denominator)
        d = mx - my
        t = float(mp.mpf(d.numerator) / d.denominator / se)
    df = (sx2 + sy2) ** 2 / (sx2 ** 2 / (nx - 1) + sy2 ** 2 / (ny - 1))
    return t, float(df)


def _welch_longdouble(x, y):
    """The same from long-double moments (460,000 cells: rationals are too slow)."""
    x, y = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
    nx, ny = len(x), len(y)
    mx, my = x.sum() / nx, y.sum() / ny
    sx2, sy2 = ((x - mx) ** 2).sum() / (nx - 1) / nx, ((y - my) ** 2).sum() / (ny - 1) / ny
    return float((mx - my) / np.sqrt(sx2 + sy2)), float((sx2 + sy2) ** 2 / (sx2 ** 2 / (nx - 1) + sy2 ** 2 / (ny - 1)))


def test_de_run_welch_t_large_df(eng):
    """Two clusters of 230,000 cells: df ~ 4.6e5, pt's normal branch (well clear
    of 4e5, so the engine and the oracle take the same side)."""
    rng = np.random.default_rng(8)
    n = 230000
    code = np.repeat([0, 1], n).astype(np.int32)
    X = np.empty((4, 2 * n))
    X[0] = rng.gamma(4.0, 0.25, 2 * n)                                  # identical in distribution
    X[1] = rng.gamma(4.0, 0.25, 2 * n) + 0.03 * (code == 0)             # strongly shifted: t ~ 20
    X[2] = rng.gamma(4.0, 0.25, 2 * n) + 0.009 * (code == 1)            # t ~ -6
    X[3] = (rng.gamma(4.0, 0.25, 2 * n) - 1.0) * np.where(code == 0, 1.0, 1.2) + 1.5 + 0.004 * (code == 1)  # unequal variances
    perm = rng.permutation(2 * n)
    X, code = X[:, perm], code[perm]
    ds = eng.dataset_dense(X)
    g = eng.de_run(ds, code, 2, nat.SCC_DE_FAST, fetch="all", test_all=True, test="t")
    errs, args = [], []
    for gene in range(4):
        t, df = _welch_longdouble(X[gene, code == 0], X[gene, code == 1])
        assert 4.3e5 < df < 4.6e5, df
        ref = R.t_two_sided_p(t, df)
        assert ref > R.P_FLOOR
        errs.append(abs(g.p[0, gene] - ref) / ref)
        args.append((gene, t, df, ref))
    assert abs(args[0][1]) < 4 and abs(args[1][1]) > 15
    msg = _report("scc_de_run Welch t, df ~ 4.6e5", np.array(errs), args)
    assert max(errs) < 1e-9, msg
    gg, o = _fast_compare(eng, ds, X, code, 2, test="t", log_fc_thrs=0.0, min_per_cent=1.0)
    assert len(o.row_gene) == 4
    assert np.max(np.abs(gg.rows.p - o.row_p) / o.row_p) < 1e-9


def test_de_run_welch_t_small_df(eng):
    """Clusters of 3, 3 and 4 cells.  Cluster 0 is constant in every gene and
    cluster 1 varies, so their Welch df is n - 1 = 2 (3 against cluster 2);
    |t| runs from 1e-6 to 1e10 over the genes."""
    rng = np.random.default_rng(9)
    code = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 2], np.int32)
    ks = list(range(-6, 11))
    X = np.zeros((len(ks), 10))
    for gene, k in enumerate(ks):
        tt = 10.0 ** k
        s = 1.0 if k <= 0 else 10.0 ** (-k)             # se = s / sqrt(3), mean shift = t * se
        X[gene, :3] = 2.0
        X[gene, 3:6] = 2.0 + tt * s / math.sqrt(3) * (-1) ** gene + s * np.array([-1.0, 0.0, 1.0])
        X[gene, 6:] = 2.0 + rng.normal(0.3, 0.5, 4)
    ds = eng.dataset_dense(X)
    g = eng.de_run(ds, code, 3, nat.SCC_DE_FAST, fetch="all", test_all=True, test="t")
    errs, args = [], []
    for p, (i, j) in enumerate(_pairs(3)):
        for gene in range(len(ks)):
            t, df = _welch_exact(X[gene, code == i], X[gene, code == j])
            ref = R.t_two_sided_p(t, df)
            errs.append(abs(g.p[p, gene] - ref) / ref)
            args.append((p, gene, t, df, ref))
    t01 = np.array([abs(a[2]) for a in args if a[0] == 0])
    assert t01.min() < 2e-6 and t01.max() > 5e9
    assert all(a[3] == 2.0 for a in args if a[0] == 0) and all(a[3] == 3.0 for a in args if a[0] == 1)
    msg = _report("scc_de_run Welch t, 3- and 4-cell clusters", np.array(errs), args)
    assert max(errs) < 1e-9, msg
    o = O.de_fast(X, code, 3, test="t", log_fc_thrs=0.0, min_per_cent=1.0)
    r = eng.de_run(ds, code, 3, nat.SCC_DE_FAST, fetch="rows", test="t", log_fc_thrs=0.0, min_per_cent=1.0).rows
    np.testing.assert_array_equal(r.gene, o.row_gene)
    assert np.max(np.abs(r.p - o.row_p) / o.row_p) < 1e-9
