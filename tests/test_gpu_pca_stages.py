"""GPU: every part of the PCA stage alone, against exact references.

The seams are the sharded-PCA calls (scc_pca_shard_colsum / _gram / _project,
one engine per emulated rank) and scc_pca_scores with SCC_CENTER_FUSED on/off.

* Integer panels (tests/pca_stage_reference.integer_panel): the means and the
  centred values are integers and every partial sum stays below 2^53, so the
  column sums, the Gram and the scores with integer vectors must equal the
  int64 results EXACTLY, whatever the tile, chunk or shard split.  A row dropped
  or double-counted in a tail chunk, a padding column that leaks or a column
  read past nu changes an integer.
* Float panels: entrywise bounds from the operation counts
  (pca_stage_reference.colsum_bound / gram_bound / project_bound), against
  Fraction sums and double-double products.  tests/test_pca_stage_reference.py
  shows that a plain fp64 sum and the one-pass Gram miss these bounds by more
  than 2^30 and 10^6.

Shapes: the column-sum kernel uses 512 chunks of ceil(n / 512) rows (empty
chunks below 512 cells, a ragged last chunk above); the Gram switches from
64- to 128-wide tiles at ld > 384 (ld = 448: the idle-wave case), splits
npad / 512 cell chunks of rows rounded to 4 while its loop steps 16 rows, and
the projection gives 16 cells to a wave and 64 to a workgroup.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import pca_stage_reference as R
from scconsensus_amd import _native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    e = nat.Engine(0)
    yield e
    e.close()


def _dataset(eng, X, kind, seed=0, extra=3):
    """A dataset of X.shape[0] cells and nu + extra genes: the panel's columns
    sit at a shuffled subset `genes` (returned, in panel order), the other
    genes hold small integers the PCA must not see."""
    X = np.asarray(X, np.float64)
    N, nu = X.shape
    G = nu + extra
    rng = np.random.default_rng(1000 + seed)
    genes = rng.permutation(G)[:nu].astype(np.int32)
    full = rng.integers(-3, 4, size=(N, G)).astype(np.float64)
    full[:, genes] = X
    if kind == "dense":
        return eng.dataset_dense(full.T), genes
    mask = full != 0.0
    cells, rows = np.nonzero(mask)  # cell-major, genes ascending inside a cell
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    return eng.dataset_csc(indptr, rows.astype(np.int32), full[cells, rows], G, N), genes


def _ready(t):
    """The engine works on a stream of its own: a buffer torch fills or
    assembles must be complete before the engine reads or writes it."""
    torch.cuda.synchronize()
    return t


def _nan(n):
    return _ready(torch.full((n,), NAN, dtype=torch.float64, device=DEV))


def _colsum(eng, ds, genes, lo, hi):
    part = _nan(2 * len(genes))
    eng.pca_shard_colsum(ds, genes, lo, hi, part.data_ptr())
    return part


def _gram(eng, parts, world, nu):
    g = _nan(nu * nu)
    eng.pca_shard_gram(parts.data_ptr(), world, g.data_ptr())
    return g.cpu().numpy().reshape(nu, nu)


def _dd_part(fracs):
    """Exact sums (Fractions or ints) as a device [nu] array of (hi, lo) pairs."""
    out = np.array([R.round_to_dd(Fraction(f)) for f in fracs], np.float64).reshape(-1)
    return _ready(torch.tensor(out, dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------- 1. column sums
COLSUM_N = [1, 2, 15, 16, 17, 511, 512, 513, 1500]


@pytest.mark.parametrize("kind", ["dense", "csc"])
@pytest.mark.parametrize("nu", [1, 63, 64, 65, 300])
def test_colsum_integer_panels_exact(eng, nu, kind):
    """hi == the int64 sum and lo == 0 for every shard [lo, lo + n), lo = 0 and
    lo = 37 (the indptr + cell_lo and dense + cell_lo G offsets)."""
    N = 1537
    X = R.integer_panel(N, nu, seed=nu)
    ds, genes = _dataset(eng, X, kind, seed=nu)
    for lo in (0, 37):
        for n in COLSUM_N:
            p = _colsum(eng, ds, genes, lo, lo + n).cpu().numpy().reshape(nu, 2)
            exact = X[lo:lo + n].sum(axis=0).astype(np.float64)
            assert np.array_equal(p[:, 0], exact), (lo, n)
            assert np.all(p[:, 1] == 0.0), (lo, n)
    ds.close()


@pytest.mark.parametrize("kind", ["dense", "csc"])
@pytest.mark.parametrize("lo", [0, 37])
def test_colsum_cancelling_floats_within_dd_bound(eng, kind, lo):
    """|hi + lo - exact| <= n 2^-102 sum|x| in Fraction arithmetic, and hi is the
    correctly rounded sum or its neighbour.

    The constant (pca_stage_reference.colsum_bound): at most n - 1 of the
    double-double additions have two non-zero operands; dd_add_d (TwoSum, low
    word folded, FastTwoSum) is within 2 u^2 = 2^-105 and dd_add (k_colsum_fold,
    dd_wave_sum_dpp: TwoSum on both words, two FastTwoSum) within 3 u^2 < 2^-104
    of the exact sum of its operands, each at most sum|x| in magnitude: below
    n 2^-104 sum|x|, with a margin of 4.  The plain fp64 sums miss this bound by
    2e10 on the same input (test_pca_stage_reference)."""
    n, nu = 1500, 5
    X = R.cancelling_columns(n, nu, seed=11)
    pad = np.random.default_rng(5).standard_normal((lo, nu)) * 1e9  # rows before the shard: not summed
    ds, genes = _dataset(eng, np.vstack([pad, X]), kind, seed=7)
    p = _colsum(eng, ds, genes, lo, lo + n).cpu().numpy().reshape(nu, 2)
    exact = R.exact_colsum(X)
    bound = R.colsum_bound(X)
    for j in range(nu):
        err = abs(Fraction(float(p[j, 0])) + Fraction(float(p[j, 1])) - exact[j])
        print(f"colsum {kind} lo={lo} col {j}: err/bound = {float(err / bound[j]):.3e}")
        assert err <= bound[j], j
        ex = float(exact[j])
        assert p[j, 0] in (ex, np.nextafter(ex, np.inf), np.nextafter(ex, -np.inf)), j
    ds.close()


# ---------------------------------------------------------------- 2. Gram
GRAM_NU = [1, 15, 16, 17, 63, 64, 65, 129, 384, 385, 448, 449]
GRAM_N = [1, 2, 15, 16, 17, 100, 1023, 1024, 1040, 1100, 2050]
GRAM_SHAPES = sorted({(n, nu) for n in (100, 1100) for nu in GRAM_NU} | {(n, nu) for n in GRAM_N for nu in (65, 449)})


@pytest.mark.parametrize("n,nu", GRAM_SHAPES)
def test_gram_integer_panels_exact(eng, n, nu):
    """Every one of the nu^2 entries written (NaN prefill), exactly symmetric,
    and equal to the int64 Gram of the centred panel."""
    X = R.integer_panel(n, nu, seed=7 * n + nu)
    kind = "csc" if (n + nu) % 2 else "dense"
    ds, genes = _dataset(eng, X, kind, seed=n + nu)
    part = _colsum(eng, ds, genes, 0, n)
    C = _gram(eng, part, 1, nu)
    assert not np.isnan(C).any(), "an entry of the Gram was not written"
    assert np.array_equal(C, C.T)
    Xc = R.centred_int(X)
    assert np.array_equal(C, (Xc.T @ Xc).astype(np.float64))
    ds.close()


SHARD_CUTS = {2: [0, 1099, 1100], 3: [0, 333, 334, 1100], 7: [0, 5, 150, 151, 500, 777, 1001, 1100]}


@pytest.mark.parametrize("nu", [70, 449])
@pytest.mark.parametrize("world", [2, 3, 7])
def test_gram_ragged_shards_sum_to_exact(world, nu):
    """1,100 cells over W ragged shards (no cut a multiple of 16, one shard of a
    single cell), one engine per rank, the parts all-gathered in rank order:
    every shard's Gram is the int64 Gram of its centred rows, and their sum the
    whole one."""
    N = 1100
    cuts = SHARD_CUTS[world]
    X = R.integer_panel(N, nu, seed=world + nu)
    engs = [nat.Engine(0) for _ in range(world)]
    dss = [_dataset(e, X, "csc" if r % 2 else "dense", seed=3) for r, e in enumerate(engs)]
    genes = dss[0][1]
    parts = _ready(torch.cat([_colsum(e, ds, genes, cuts[r], cuts[r + 1])
                              for r, (e, (ds, _)) in enumerate(zip(engs, dss))]))
    sums = parts.cpu().numpy().reshape(world, nu, 2)
    Xc = R.centred_int(X)
    total = np.zeros((nu, nu))
    for r, e in enumerate(engs):
        assert np.array_equal(sums[r, :, 0], X[cuts[r]:cuts[r + 1]].sum(axis=0).astype(np.float64))
        C = _gram(e, parts, world, nu)
        blk = Xc[cuts[r]:cuts[r + 1]]
        assert np.array_equal(C, (blk.T @ blk).astype(np.float64)), r
        total += C  # integers below 2^53: exact in any order
    assert np.array_equal(total, (Xc.T @ Xc).astype(np.float64))
    for (ds, _), e in zip(dss, engs):
        ds.close()
        e.close()


_FLOAT_PANELS = {"counts": R.lognormal_counts_panel, "mean_dominated": R.mean_dominated_panel}


def _float_gram_case(kind, n, nu):
    X = _FLOAT_PANELS[kind](n, nu, seed=n + nu)
    mean = R.exact_mean_rounded(X)
    hi, _ = R.dd_gram(X, mean)
    return X, hi, R.gram_bound(X, mean=mean)


# two chunks / 64-wide tiles, four chunks with rows not a multiple of 16, the 128-wide kernel
@pytest.mark.parametrize("n,nu", [(1100, 70), (2050, 65), (100, 449)])
@pytest.mark.parametrize("kind", ["counts", "mean_dominated"])
def test_gram_float_within_bound(eng, kind, n, nu):
    """|C_ij - Cref_ij| <= 2 u [(n + 4) A_ij + 2 (|m_i| s_j + |m_j| s_i)] against
    the double-double Gram of the panel centred with the exact mean rounded
    once.  On the mean-dominated panel the one-pass formula misses this bound
    by 6e6 (test_pca_stage_reference), as would a mean without its low word."""
    X, ref, bound = _float_gram_case(kind, n, nu)
    ds, genes = _dataset(eng, X, "csc" if kind == "counts" else "dense", seed=n)
    C = _gram(eng, _colsum(eng, ds, genes, 0, n), 1, nu)
    assert np.array_equal(C, C.T)
    ratio = np.abs(C - ref) / np.where(bound > 0, bound, 1.0)
    print(f"gram {kind} ({n}, {nu}): worst err/bound = {ratio.max():.3e}")
    assert np.all(np.abs(C - ref) <= bound)
    ds.close()


@pytest.mark.parametrize("rest_kind", ["real", "cancelling"])
def test_mean_of_parts_is_the_correctly_rounded_mean(eng, rest_kind):
    """The mean the Gram and the scores centre with, read back bit for bit: a
    cell whose panel row is zero projects onto unit vectors as -mean[u]
    exactly.  It must be the exact (own + rest) / N of the four words of the
    two parts, rounded once: dd_add keeps 2^-104 relative under cancellation
    and dd_div_n is within u^2 of the quotient before its last rounding, so
    only an exact value within ~2^-100 relative of a rounding boundary could
    differ (probability ~1e-13 per column).  A mean formed from the high words
    alone is off by up to an ulp on the mean-dominated panel (about half of the
    columns change) and is wrong in every digit when the other rank's sum
    cancels this rank's (the Gram's forward bound cannot see either: centred
    columns sum to zero, so the Gram is insensitive to the mean to first order)."""
    N, nu, lo, hi, zero_cell = 1100, 70, 0, 600, 3
    X = R.mean_dominated_panel(N, nu, seed=21)
    X[zero_cell] = 0.0
    ds, genes = _dataset(eng, X, "dense", seed=21)
    own = _colsum(eng, ds, genes, lo, hi)
    own_h = own.cpu().numpy().reshape(nu, 2)
    own_f = [Fraction(float(a)) + Fraction(float(b)) for a, b in own_h]
    if rest_kind == "real":
        rest_f = R.exact_colsum(X[hi:])
    else:  # the other rank's sum cancels this rank's down to N * 0.37 (u + 1)
        rest_f = [-own_f[u] + N * Fraction(0.37) * (u + 1) for u in range(nu)]
    rest = _dd_part(rest_f)
    rest_h = rest.cpu().numpy().reshape(nu, 2)
    want = np.array([float((own_f[u] + Fraction(float(rest_h[u, 0])) + Fraction(float(rest_h[u, 1]))) / N)
                     for u in range(nu)])
    parts = _ready(torch.cat([own, rest]))
    g = _nan(nu * nu)
    eng.pca_shard_gram(parts.data_ptr(), 2, g.data_ptr())
    got = np.empty(nu)
    for u0 in range(0, nu, 16):
        k = min(16, nu - u0)
        V = np.zeros((nu, 16))
        V[u0 + np.arange(k), np.arange(k)] = 1.0
        Vd = _ready(torch.tensor(V.reshape(-1), dtype=torch.float64, device=DEV))
        sc = _nan(N * 16)
        eng.pca_shard_project(Vd.data_ptr(), sc.data_ptr(), ncomp=k)
        got[u0:u0 + k] = -sc.cpu().numpy().reshape(N, 16)[zero_cell, :k]
    assert np.array_equal(got, want)
    ds.close()


# ---------------------------------------------------------------- 3. fused centring
def _scores_of(eng, ds, genes, N):
    eng.pca_scores(ds, genes)
    return eng.last_pca_scores(N)


@pytest.mark.parametrize("N", [17, 100, 1040, 2050])
@pytest.mark.parametrize("nu", [15, 64, 65, 384])
def test_fused_centring_same_bits(eng, monkeypatch, nu, N):
    """scc_pca_scores with the centring folded into the Gram and the scores
    (the default at ld <= 384) and with the explicit centring pass
    (SCC_CENTER_FUSED=0): the same x - mean[u] either way, so the same bits.  On
    an integer panel both also equal the shard route (colsum, gram,
    scc_pca_shard_scores) bit for bit."""
    k = min(nu, 15)
    for panel in ("integer", "counts"):
        X = R.integer_panel(N, nu, seed=N + nu) if panel == "integer" else R.lognormal_counts_panel(N, nu, N + nu)
        ds, genes = _dataset(eng, X, "csc", seed=N)
        monkeypatch.setenv("SCC_CENTER_FUSED", "1")
        fused = _scores_of(eng, ds, genes, N)
        monkeypatch.setenv("SCC_CENTER_FUSED", "0")
        explicit = _scores_of(eng, ds, genes, N)
        monkeypatch.delenv("SCC_CENTER_FUSED")
        assert fused.shape == (N, k)
        assert np.isfinite(fused).all()
        assert np.array_equal(fused, explicit), panel
        if panel == "integer":
            part = _colsum(eng, ds, genes, 0, N)
            g = _nan(nu * nu)
            eng.pca_shard_gram(part.data_ptr(), 1, g.data_ptr())
            sc = _nan(N * 16)
            eng.pca_shard_scores(g.data_ptr(), sc.data_ptr())
            sc = sc.cpu().numpy().reshape(N, 16)
            assert np.array_equal(sc[:, :k], fused)
            assert np.all(sc[:, k:] == 0.0)
        ds.close()


# ---------------------------------------------------------------- 4. projection
def _shard_setup(eng, X, lo, hi, kind, seed, exact_sums):
    """colsum + gram of the shard [lo, hi) of X as rank 0 of a world of two, the
    other rank's part (the rest of the cells) supplied exactly from the host;
    leaves the engine ready for scc_pca_shard_project."""
    ds, genes = _dataset(eng, X, kind, seed=seed)
    own = _colsum(eng, ds, genes, lo, hi)
    parts = _ready(torch.cat([own, _dd_part(exact_sums)]))
    nu = X.shape[1]
    g = _nan(nu * nu)
    eng.pca_shard_gram(parts.data_ptr(), 2, g.data_ptr())
    return ds


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 300])
@pytest.mark.parametrize("nu", [1, 63, 64, 65, 200])
def test_project_integer_exact_and_row_window(eng, monkeypatch, n, nu):
    """Integer panel, integer vectors in -8..8: rows [37, 37 + n) of the scores
    equal Xc V exactly for k in {1, 2, 15, 16} and both kernels
    (SCC_SCORES_MFMA=1 / 0); vecs columns >= k hold NaN and must not be read
    (score columns >= k are 0.0); every other row of the NaN-prefilled [N][16]
    scores stays untouched."""
    lo, hi = 37, 37 + n
    N = hi + 5
    X = R.integer_panel(N, nu, seed=31 * n + nu)
    rest = X.sum(axis=0) - X[lo:hi].sum(axis=0)
    ds = _shard_setup(eng, X, lo, hi, "csc" if n % 2 else "dense", n + nu, [int(v) for v in rest])
    Xc = R.centred_int(X)[lo:hi]
    rng = np.random.default_rng(n * nu)
    for k in (1, 2, 15, 16):
        if k > nu:
            continue
        V = rng.integers(-8, 9, size=(nu, 16)).astype(np.float64)
        want = (Xc @ V[:, :k].astype(np.int64)).astype(np.float64)
        V[:, k:] = NAN
        Vd = _ready(torch.tensor(V.reshape(-1), dtype=torch.float64, device=DEV))
        for mfma in ("1", "0"):
            monkeypatch.setenv("SCC_SCORES_MFMA", mfma)
            sc = _nan(N * 16)
            eng.pca_shard_project(Vd.data_ptr(), sc.data_ptr(), ncomp=k)
            sc = sc.cpu().numpy().reshape(N, 16)
            assert np.isnan(sc[:lo]).all() and np.isnan(sc[hi:]).all(), (k, mfma)
            assert np.array_equal(sc[lo:hi, :k], want), (k, mfma)
            assert np.all(sc[lo:hi, k:] == 0.0), (k, mfma)
    ds.close()


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_project_float_within_bound(eng, monkeypatch, mfma):
    """|P - Pref| <= (nu + 2) u |Xc| |V| against the double-double product of
    the centred (rounded) panel with the vectors."""
    monkeypatch.setenv("SCC_SCORES_MFMA", mfma)
    n, nu, k, lo = 300, 200, 15, 37
    N = lo + n + 5
    X = R.lognormal_counts_panel(N, nu, seed=9)
    total = R.exact_colsum(X)
    own = R.exact_colsum(X[lo:lo + n])
    ds = _shard_setup(eng, X, lo, lo + n, "csc", 9, [t - o for t, o in zip(total, own)])
    mean = R.exact_mean_rounded(X, col_sums=total)
    V = np.zeros((nu, 16))
    V[:, :k] = np.linalg.qr(np.random.default_rng(2).standard_normal((nu, k)))[0]
    Vd = _ready(torch.tensor(V.reshape(-1), dtype=torch.float64, device=DEV))
    sc = _nan(N * 16)
    eng.pca_shard_project(Vd.data_ptr(), sc.data_ptr(), ncomp=k)
    sc = sc.cpu().numpy().reshape(N, 16)[lo:lo + n]
    ref, _ = R.dd_project(X[lo:lo + n], mean, V[:, :k])
    bound = R.project_bound(X[lo:lo + n] - mean, V[:, :k])
    print(f"project mfma={mfma}: worst err/bound = {np.max(np.abs(sc[:, :k] - ref) / bound):.3e}")
    assert np.all(np.abs(sc[:, :k] - ref) <= bound)
    assert np.all(sc[:, k:] == 0.0)
    ds.close()


# ---------------------------------------------------------------- 5. call order, empty shard
def test_shard_calls_out_of_order_raise():
    e = nat.Engine(0)
    X = R.integer_panel(40, 6, seed=1)
    ds, genes = _dataset(e, X, "dense")
    buf = _nan(40 * 16)
    with pytest.raises(nat.SccError) as err:
        e.pca_shard_gram(buf.data_ptr(), 1, buf.data_ptr())
    assert err.value.code == nat.SCC_ERR_INVALID
    part = _colsum(e, ds, genes, 0, 40)
    for call in (e.pca_shard_eigen, e.pca_shard_project, e.pca_shard_scores):
        with pytest.raises(nat.SccError) as err:
            call(buf.data_ptr(), buf.data_ptr())
        assert err.value.code == nat.SCC_ERR_INVALID
    e.pca_shard_gram(part.data_ptr(), 1, buf.data_ptr())  # in order: accepted
    ds.close()
    e.close()


@pytest.mark.parametrize("kind", ["dense", "csc"])
def test_empty_shard_is_valid_and_writes_zeros(eng, kind):
    """cell_lo == cell_hi (a rank without cells): SCC_OK, zero sums, a zero
    partial Gram, no score row written (include/scc.h)."""
    N, nu = 50, 20
    X = R.integer_panel(N, nu, seed=2)
    ds, genes = _dataset(eng, X, kind)
    own = _colsum(eng, ds, genes, 20, 20)
    assert np.all(own.cpu().numpy() == 0.0)
    parts = _ready(torch.cat([own, _dd_part([int(v) for v in X.sum(axis=0)])]))
    C = _gram(eng, parts, 2, nu)
    assert np.all(C == 0.0)
    V = _ready(torch.ones(nu * 16, dtype=torch.float64, device=DEV))
    sc = _nan(N * 16)
    eng.pca_shard_project(V.data_ptr(), sc.data_ptr(), ncomp=3)
    assert torch.isnan(sc).all()
    ds.close()
