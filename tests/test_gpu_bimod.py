"""GPU parity of the FAST "bimod" test (SCC_TEST_BIMOD; DiffExpTest,
R/reclusterDEConsensusFast.R:93-133) against tests/bimod_reference.py, which
restates the R code from the cell values in long double.

The engine works from per-(gene, cluster) moments of the values > 0 in
float64 / double-double; a CPU float64 model of that form agreed with the
reference to 5.4e-13 relative on every row tested here, so the bar is the one
the t path is held to: p within 1e-9 relative wherever the reference p is
>= 1e-290, and <= 1e-280 where the reference is smaller.  The exact 0s and 1s
of R's IEEE cases are compared for equality."""
import functools

import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

import bimod_reference as B
import oracle as O
from parity_helpers import check_selection
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

P_RTOL = 1e-9
FAST_FIELDS = ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top")
LOOSE = dict(min_per_cent=5.0, log_fc_thrs=0.1)


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


@functools.lru_cache(maxsize=None)
def _case_a():
    d = synth.generate("A", G=300, N=1200, K=5, seed=3)
    names, code = api.select_clusters(d.labels, 10)
    return d, d.dense(), len(names), code


@functools.lru_cache(maxsize=None)
def _ref_a(loose):
    _, X, K, code = _case_a()
    return B.de_bimod(X, code, K, **(LOOSE if loose else {}))


def _check_p(got, want, what="", exact=False):
    """The p bar: 1e-9 relative where the reference p >= 1e-290, <= 1e-280
    where it is smaller (0 included: an infinite statistic or an underflow);
    exact: the reference's 0s and 1s are R's IEEE cases, compared for equality."""
    got, want = np.asarray(got), np.asarray(want)
    print(f"{what}: {len(want)} rows, worst relative p deviation "
          f"{np.max(np.abs(got - want)[want >= 1e-290] / want[want >= 1e-290], initial=0.0):.3g}")
    big = want >= 1e-290
    np.testing.assert_allclose(got[big], want[big], rtol=P_RTOL, atol=0, err_msg=what)
    assert (got[~big] <= 1e-280).all(), what
    for v in (0.0, 1.0) if exact else ():
        np.testing.assert_array_equal(got == v, want == v, err_msg=what)


def _check_against_reference(g, ref, K, q_val_thrs=0.1, top_n=30, exact=False):
    rows = g.rows
    # preconditions on the reference side: no q at the threshold, no near-tied p
    for q, p in zip(ref.q, ref.p):
        assert not np.isnan(p).any()
        assert (np.abs(q - q_val_thrs) > 1e-6 * q_val_thrs).all()
        s = np.sort(p)
        gap = np.diff(s)
        assert ((gap == 0) | (gap > 1e-8 * s[1:])).all()
    np.testing.assert_array_equal(rows.pair_tested, ref.pair_tested)
    assert (rows.u2 == 0).all() and (rows.ties == 0).all()
    starts = np.concatenate([[0], np.cumsum(rows.pair_tested)]).astype(np.int64)
    for k in range(K * (K - 1) // 2):
        sl = slice(int(starts[k]), int(starts[k + 1]))
        o = np.argsort(rows.gene[sl], kind="stable")  # the row order differs: match by gene
        np.testing.assert_array_equal(rows.gene[sl][o], ref.gene[k], err_msg=f"pair {k}: tested genes")
        np.testing.assert_allclose(rows.avg_logfc[sl][o], ref.lfc[k], rtol=1e-12, atol=5e-14)
        np.testing.assert_array_equal(rows.pct1[sl][o], ref.pct1[k])
        np.testing.assert_array_equal(rows.pct2[sl][o], ref.pct2[k])
        _check_p(rows.p[sl][o], ref.p[k], f"pair {k}", exact)
        np.testing.assert_array_equal(rows.de[sl][o], ref.de[k], err_msg=f"pair {k}: kept rows")
        np.testing.assert_array_equal(rows.top[sl][o], ref.top[k], err_msg=f"pair {k}: top_n rows")
    check_selection(rows, g.union, K, q_val_thrs=q_val_thrs, top_n=top_n)
    np.testing.assert_array_equal(g.union, ref.union)


# ---------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("loose", [False, True])
def test_bimod_config_a(eng, loose):
    """Reduced config A: several pieces per gene and cluster sizes that are no
    multiple of the wave (the min / max wave reductions at a wave boundary)."""
    d, X, K, code = _case_a()
    ref = _ref_a(loose)
    assert ref.pair_tested.sum() == (1282 if loose else 157)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    g = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", test="bimod", **(LOOSE if loose else {}))
    _check_against_reference(g, ref, K)
    assert len(g.union) > 20
    # the filters do not depend on the test: the wilcox run tests the same cells
    w = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", **(LOOSE if loose else {}))
    np.testing.assert_array_equal(w.rows.pair_tested, g.rows.pair_tested)
    # dense input: the same bits
    gd = eng.de_run(eng.dataset_dense(X), code, K, nat.SCC_DE_FAST, fetch="rows", test="bimod",
                    **(LOOSE if loose else {}))
    for f in FAST_FIELDS:
        np.testing.assert_array_equal(getattr(gd.rows, f), getattr(g.rows, f), err_msg=f)


def test_bimod_edge_fixture(eng):
    """Negative values, p == 1 rows, small clusters."""
    d = synth.edge_fixture()
    names, code = api.select_clusters(d.labels, 10)
    K, kw = len(names), dict(log_fc_thrs=0.1, min_per_cent=15.0)
    ref = B.de_bimod(d.dense(), code, K, **kw)
    assert ref.pair_tested.sum() == 788 and (np.concatenate(ref.p) == 1.0).sum() == 5
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    g = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", test="bimod", **kw)
    _check_against_reference(g, ref, K)


# ---------------------------------------------------------------- (c), (d)
def test_bimod_degenerate_cases(eng):
    """R's IEEE cases: lrt = +Inf (p = 0), lrt <= 0 and -Inf (p = 1), the
    sd := 1 and n2 = 0 branches, negatives as "not expressed"."""
    X, code = B.degenerate_fixture()
    kw = dict(min_per_cent=1.0, log_fc_thrs=0.0)
    ref = B.de_bimod(X, code, 3, **kw)
    for (gene, (i, j)), want in B.DEGENERATE_EXACT.items():  # precondition: tested, with the stated p
        k = B.pair_list(3).index((i, j))
        assert ref.p[k][list(ref.gene[k]).index(gene)] == want
    assert ref.pair_tested.sum() == 18
    g = eng.de_run(eng.dataset_dense(X), code, 3, nat.SCC_DE_FAST, fetch="rows", test="bimod", **kw)
    _check_against_reference(g, ref, 3, exact=True)
    assert (g.rows.p == 0.0).sum() == 5 and (g.rows.p == 1.0).sum() == 2


def _wave_boundary_matrix():
    """All-equal detection at the wave width: cluster 0 (200 cells) holds n
    values > 0 for n around 64, 128 and 192, all 2.0 (lrt = +Inf, p = 0) or all
    but one (first, 64th or last of them: a finite p)."""
    rng = np.random.default_rng(13)
    code = np.repeat(np.arange(3), 200).astype(np.int32)
    rows = []
    for n in (63, 64, 65, 127, 128, 129, 192):
        for odd in (None, 0, 63, n - 1):
            x = np.zeros(600)
            x[:n] = 2.0
            if odd is not None:
                x[min(odd, n - 1)] = 2.5
            x[200:250] = np.log1p(rng.gamma(2.0, 2.0, 50)) + 0.1
            x[400:440] = np.log1p(rng.gamma(2.0, 2.0, 40)) + 0.1
            rows.append(x)
    return np.array(rows), code


def test_bimod_all_equal_at_wave_boundaries(eng):
    X, code = _wave_boundary_matrix()
    kw = dict(min_per_cent=1.0, log_fc_thrs=0.0)
    ref = B.de_bimod(X, code, 3, **kw)
    assert ref.pair_tested.sum() == 3 * len(X)
    p01 = ref.p[0].reshape(7, 4)  # pair (0, 1): [n][all equal, odd one first / 64th / last]
    assert (p01[:, 0] == 0.0).all() and (p01[:, 1:] > 0.0).all()
    g = eng.de_run(eng.dataset_dense(X), code, 3, nat.SCC_DE_FAST, fetch="rows", test="bimod", **kw)
    _check_against_reference(g, ref, 3, exact=True)


def test_bimod_nan_p_stops(eng):
    """A tested Inf - Inf cell: R's NA p_val_adj ends in stop(); the engine
    returns SCC_ERR_RSTOP, for tested cells only."""
    X, code = B.degenerate_fixture(with_nan_gene=True)
    c = [X[6, code == a] for a in range(3)]
    assert all(np.isnan(B.p_value(c[i], c[j])) for i, j in B.pair_list(3))
    ds = eng.dataset_dense(X)
    with pytest.raises(nat.SccError) as e:
        eng.de_run(ds, code, 3, nat.SCC_DE_FAST, fetch="rows", test="bimod", min_per_cent=1.0, log_fc_thrs=0.0)
    assert e.value.code == nat.SCC_ERR_RSTOP and "bimod" in str(e.value)
    # log_fc_thrs = 5 tests none of those cells: no stop
    assert O.de_fast(X, code, 3, min_per_cent=1.0, log_fc_thrs=5.0).pair_tested.sum() == 0
    g = eng.de_run(ds, code, 3, nat.SCC_DE_FAST, fetch="rows", test="bimod", min_per_cent=1.0, log_fc_thrs=5.0)
    assert g.rows.pair_tested.sum() == 0 and len(g.union) == 0
    # ... nor do cells computed only because test_all is set
    g = eng.de_run(ds, code, 3, nat.SCC_DE_FAST, fetch="all", test="bimod", min_per_cent=1.0, log_fc_thrs=5.0)
    assert np.isnan(g.p[:, 6]).all() and g.p[0, 3] == 0.0 and g.p[0, 4] == 1.0
    # the gene-shard route reports the stop where the cells are computed
    buf = torch.zeros(3 * 7 * 8, dtype=torch.int64, device="cuda:0")
    with pytest.raises(nat.SccError) as e:
        eng.de_run_shard_records(ds, code, 3, 4, 7, buf.data_ptr(), 3 * 3, test="bimod", min_per_cent=1.0,
                                 log_fc_thrs=0.0)
    assert e.value.code == nat.SCC_ERR_RSTOP
    assert eng.de_run_shard_records(ds, code, 3, 0, 6, buf.data_ptr(), 3 * 6, test="bimod", min_per_cent=1.0,
                                    log_fc_thrs=0.0) == 18
    with pytest.raises(nat.SccError) as e:
        eng.de_run(ds, code, 3, nat.SCC_DE_SLOW, q_val_thrs=0.05, fc_thrs=1.5, test="bimod")
    assert e.value.code == nat.SCC_ERR_INVALID


# ---------------------------------------------------------------- (e) routes
def _same_rows(a, b):
    np.testing.assert_array_equal(a.union, b.union)
    for f in FAST_FIELDS:
        np.testing.assert_array_equal(getattr(a.rows, f), getattr(b.rows, f), err_msg=f)


def test_bimod_routes_bitwise(eng):
    """Every FAST route carries the test: the device list, the gene-shard
    records with their finish, the dense shards with theirs, and the fused
    DE + distance call give the one-device result bit for bit."""
    d, X, K, code = _case_a()
    P = K * (K - 1) // 2
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    one = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", test="bimod")
    assert one.rows.pair_tested.sum() == 157
    # a device list [0, 0]
    multi = nat.Engine(0, devices=[0, 0])
    try:
        dm = multi.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
        _same_rows(one, multi.de_run(dm, code, K, nat.SCC_DE_FAST, fetch="rows", test="bimod"))
    finally:
        multi.close()
    # compact records over two gene blocks
    blocks, counts = [], []
    for lo, hi in ((0, 131), (131, d.G)):
        cap = P * (hi - lo)
        buf = torch.full((cap * 8,), -1, dtype=torch.int64, device="cuda:0")
        counts.append(eng.de_run_shard_records(ds, code, K, lo, hi, buf.data_ptr(), cap, test="bimod"))
        blocks.append(buf)
    assert sum(counts) == 157
    stride = max(counts)
    allr = torch.full((2 * stride * 8,), -7, dtype=torch.int64, device="cuda:0")
    for b, (buf, n) in enumerate(zip(blocks, counts)):
        allr[b * stride * 8: b * stride * 8 + n * 8] = buf[: n * 8]
    torch.cuda.synchronize()
    _same_rows(one, eng.de_finish_records(ds, code, K, allr.data_ptr(), counts, stride, fetch="rows", test="bimod"))
    # dense shards, summed as int64 words
    words = eng.de_shard_bytes(K, d.G) // 8
    total = torch.zeros(words, dtype=torch.int64, device="cuda:0")
    for lo, hi in ((0, 77), (77, d.G)):
        sh = torch.zeros(words, dtype=torch.int64, device="cuda:0")
        eng.de_run_shard(ds, code, K, lo, hi, sh.data_ptr(), test="bimod")
        total += sh
    torch.cuda.synchronize()
    _same_rows(one, eng.de_finish(ds, code, K, total.data_ptr(), fetch="rows", test="bimod"))
    # DE + distance in one call
    de, dist = eng.de_distance(ds, code, K, test="bimod")
    np.testing.assert_array_equal(de.union, one.union)
    np.testing.assert_array_equal(dist, eng.distance(ds, one.union))


# ---------------------------------------------------------------- (f) K > 128
def test_bimod_129_clusters(eng):
    """K = 129 through one scc_de_run: three group-pair runs."""
    d = synth.generate("A", G=60, N=9000, K=129, seed=29)
    names, code = api.select_clusters(d.labels, 10)
    assert len(names) == 129
    X = d.dense()
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    g = eng.de_run(ds, code, 129, nat.SCC_DE_FAST, fetch="rows", test="bimod")
    o = O.de_fast(X, code, 129)
    np.testing.assert_array_equal(g.rows.pair_tested, o.pair_tested)
    n = len(o.row_gene)
    mask = np.zeros(n, bool)
    mask[np.random.default_rng(5).choice(n, min(n, 2000), replace=False)] = True
    ref = B.de_bimod(X, code, 129, sample=mask)
    starts = np.concatenate([[0], np.cumsum(o.pair_tested)]).astype(np.int64)
    got, want = [], []
    for k in np.flatnonzero(o.pair_tested):
        sl = slice(int(starts[k]), int(starts[k + 1]))
        order = np.argsort(g.rows.gene[sl], kind="stable")
        np.testing.assert_array_equal(g.rows.gene[sl][order], ref.gene[k])
        keep = ~np.isnan(ref.p[k])
        got.append(g.rows.p[sl][order][keep])
        want.append(ref.p[k][keep])
    got, want = np.concatenate(got), np.concatenate(want)
    assert len(want) == min(n, 2000) and not np.isnan(got).any()
    _check_p(got, want, "K = 129 sample")
    assert (g.rows.u2 == 0).all() and (g.rows.ties == 0).all()
    check_selection(g.rows, g.union, 129)
    assert len(g.union) > 0


# ---------------------------------------------------------------- (g) the API
def test_api_method_bimod(eng):
    d, X, K, code = _case_a()
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    one = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="union", test="bimod")
    names = np.array([f"g{i}" for i in range(d.G)], dtype=object)
    out = api.reclusterDEConsensusFast(X, d.labels, method="bimod", gene_names=names, deepSplitValues=(1,))
    assert out["deGeneUnion"] == list(names[one.union])
    with pytest.raises(NotImplementedError):
        api.reclusterDEConsensusFast(X, d.labels, method="roc")
