"""The rank stage on the dataset's value order (scc_vorder.hip; k_rank_vorder_list in
scc_rank_split.hip, k_rank_mfma16<1, true> in scc_rank_waves.hip) against the per-call value buckets
it replaces (split, re-split, in-wave sort, LDS items), bit for bit on the
fields tests/test_gpu_mirror.py compares.  A dataset that keeps the gene-major
mirror keeps each gene's ascending value order and its bucket cuts; a FAST
Wilcoxon run over the whole gene range walks them and sorts only inside tie groups
(the reference ranks every pair's cells again: R/reclusterDEConsensusFast.R,
the wilcox.test calls of the per-pair loop).  Every comparison asserts which
route ran (scc_diag_rank_last_route): a silent fallback would pass every
equality."""
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

FAST_FIELDS = ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top")
FULL, LEAN, MIRROR = 1, 2, 3  # scc_diag_ingest_last_path
BUCKETS, VORDER = 1, 2        # scc_diag_rank_last_route
MIRROR_SEG = 128              # SCC_MIRROR_SEG


@pytest.fixture(scope="module")
def eng():
    e = nat.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cfg():
    d = synth.generate("A", G=1000, N=1500, K=6, seed=43)
    names, code = api.select_clusters(d.labels, 10)
    return d, code, len(names)


def _same(a, b):
    np.testing.assert_array_equal(a.union, b.union)
    np.testing.assert_array_equal(a.nodg, b.nodg)
    for f in FAST_FIELDS:
        np.testing.assert_array_equal(getattr(a.rows, f), getattr(b.rows, f), err_msg=f)


def _run(eng, ds, code, K, **kw):
    r = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", **kw)
    return r, int(eng.lib.scc_diag_ingest_last_path()), int(eng.lib.scc_diag_rank_last_route())


def _three_calls(eng, d, code, K, **kw):
    """The validating call, the call that builds the mirror and the order, a
    third that reuses them; the dataset and the three results."""
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    first, p1, r1 = _run(eng, ds, code, K, **kw)
    built, p2, r2 = _run(eng, ds, code, K, **kw)
    again, p3, r3 = _run(eng, ds, code, K, **kw)
    assert (p1, p2, p3) == (FULL, MIRROR, MIRROR)
    return ds, (first, built, again), (r1, r2, r3)


def _on_off(eng, ds, code, K, monkeypatch, want_on=VORDER, **kw):
    """The same run on the value order and with SCC_RANK_VORDER=0; the former's result."""
    on, _, r_on = _run(eng, ds, code, K, **kw)
    monkeypatch.setenv("SCC_RANK_VORDER", "0")
    off, _, r_off = _run(eng, ds, code, K, **kw)
    monkeypatch.delenv("SCC_RANK_VORDER")
    assert (r_on, r_off) == (want_on, BUCKETS)
    _same(on, off)
    return on


def test_three_calls_and_both_routes(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds, (first, built, again), routes = _three_calls(eng, d, code, K)
    assert routes == (BUCKETS, VORDER, VORDER)
    _same(built, first)
    _same(again, first)
    _same(_on_off(eng, ds, code, K, monkeypatch), first)
    assert len(first.union) > 20


def test_labels_change_order_stays(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds, _, routes = _three_calls(eng, d, code, K)
    assert routes[1:] == (VORDER, VORDER)
    # another labelling: K = 4, every cluster spread over the whole cell range, 10 % of the cells unkept
    i = np.arange(d.N)
    code2 = np.where(i % 10 == 9, -1, (i % 10) % 4).astype(np.int32)
    r = _on_off(eng, ds, code2, 4, monkeypatch, min_per_cent=5.0, log_fc_thrs=0.0)
    assert len(r.rows.gene) > 0
    # a fresh dataset under the second labelling gives the same
    ds2, (first2, built2, _), routes2 = _three_calls(eng, d, code2, 4, min_per_cent=5.0, log_fc_thrs=0.0)
    assert routes2 == (BUCKETS, VORDER, VORDER)
    _same(r, first2)
    _same(r, built2)


def _tie_matrix():
    """40 genes x 700 cells of small integers.  Cells alternate between five
    clusters (so every tie group's cells do); the last 20 cells are unkept."""
    rng = np.random.default_rng(7)
    G, N, K = 40, 700, 5
    i = np.arange(N)
    code = (i % K).astype(np.int32)
    code[N - 20:] = -1
    X = np.zeros((G, N))
    kept = np.flatnonzero(code >= 0)

    def put(g, vals):
        cells = rng.choice(kept, len(vals), replace=False)
        X[g, np.sort(cells)] = vals

    for g, n in enumerate([1, 2, 63, 64, 65, 128, 129]):  # genes of 1 .. 129 stored values
        put(g, rng.integers(1, 6, n))
    put(7, np.repeat([1, 2, 3], [60, 10, 5]))             # a tie group that would straddle position 64
    put(8, np.repeat([1, 2, 3, 4], [1, 64, 1, 65]))       # tie groups of exactly 64 and of 65
    put(9, np.full(300, 2))                                # one repeated value 300 times
    X[10, :400] = 1 + np.arange(400) // 50                 # groups of 50 consecutive cells
    put(11, rng.choice([-3, -2, -1, 1, 2], 250))           # negative values
    X[12, N - 20:] = rng.integers(1, 4, 20)                # stored in no kept cell
    put(13, 0.5 + np.arange(200))                          # no ties at all
    X[14, i % 10 == 9] = rng.integers(1, 4, N // 10)       # the cells of test_unkept_cluster's dropped cells
    for g in range(15, G):
        lam = np.full(N, 0.6)
        lam[code == g % K] = 3.0
        X[g] = rng.poisson(lam)
    assert [int(np.sum(X[g] != 0)) for g in range(10)] == [1, 2, 63, 64, 65, 128, 129, 75, 131, 300]
    assert not np.any(X[12, code >= 0]) and np.any(X[12] != 0)
    d = synth.from_dense(X, code.astype(str))
    return d, code, K


TIE_KW = dict(min_per_cent=1.0, log_fc_thrs=0.0, test_all=True)


def test_heavy_ties(eng, monkeypatch):
    d, code, K = _tie_matrix()
    ds, (first, built, again), routes = _three_calls(eng, d, code, K, **TIE_KW)
    assert routes == (BUCKETS, VORDER, VORDER)
    _same(built, first)
    _same(again, first)
    r = _on_off(eng, ds, code, K, monkeypatch, **TIE_KW)
    assert len(r.rows.gene) > 0 and np.any(r.rows.ties > 0)


def test_unkept_cluster(eng, monkeypatch):
    """One small cluster unkept: unkept cells inside buckets, at bucket starts
    and inside tie groups; gene 14's entries are all unkept."""
    d, code, K = _tie_matrix()
    i = np.arange(d.N)
    code2 = np.where(i % 10 == 9, -1, code).astype(np.int32)
    assert np.sum(code2 < 0) > 80 and len(np.unique(code2[code2 >= 0])) == K
    ds, (first, built, again), routes = _three_calls(eng, d, code2, K, **TIE_KW)
    assert routes == (BUCKETS, VORDER, VORDER)
    _same(built, first)
    _same(again, first)
    _on_off(eng, ds, code2, K, monkeypatch, **TIE_KW)
    X = d.dense()
    assert np.any(X[14] != 0) and not np.any(X[14, code2 >= 0])


@pytest.mark.parametrize("K,N,test_all", [(12, 2000, True), (16, 2000, True), (17, 2000, True), (17, 2000, False),
                                          (33, 2000, True), (33, 2000, False), (70, 6000, False)])
def test_cluster_counts(eng, K, N, test_all, monkeypatch):
    """K <= 16: every gene on the 16-wide matrix-core kernel.  K > 16 takes the
    order too: the slot kernels (17; 33 and 70 with few tested pairs a gene; 70:
    clusters past 64), and at 33 with every pair tested (528 > 512) the
    matrix-core class."""
    d = synth.generate("A", G=300, N=N, K=K, seed=9, sizes="dirichlet")
    names, code = api.select_clusters(d.labels, 10)
    assert len(names) == K
    ds, (first, built, again), routes = _three_calls(eng, d, code, K, test_all=test_all)
    assert routes == (BUCKETS, VORDER, VORDER)
    _same(built, first)
    _same(again, first)
    r = _on_off(eng, ds, code, K, monkeypatch, test_all=test_all)
    assert len(r.rows.gene) > 0


def test_mirror_fits_order_does_not(eng, cfg, monkeypatch):
    d, code, K = cfg
    nnz = len(d.data)
    mirror = 8 * (d.G + 1) + 4 * d.G + 12 * nnz + 4 * d.G * ((d.N + MIRROR_SEG - 1) // MIRROR_SEG + 1)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    first, p1, r1 = _run(eng, ds, code, K)
    monkeypatch.setenv("SCC_INGEST_MIRROR_MAX_BYTES", str(mirror + 2 * nnz))  # (the order: more than 4 B a value)
    alone, p2, r2 = _run(eng, ds, code, K)
    again, p3, r3 = _run(eng, ds, code, K)
    assert (p1, p2, p3) == (FULL, MIRROR, MIRROR) and (r1, r2, r3) == (BUCKETS, BUCKETS, BUCKETS)
    _same(alone, first)
    _same(again, first)
    monkeypatch.delenv("SCC_INGEST_MIRROR_MAX_BYTES")
    later, p4, r4 = _run(eng, ds, code, K)  # the limit gone: the order is built beside the mirror
    assert (p4, r4) == (MIRROR, VORDER)
    _same(later, first)


def _shards(eng, ds, code, K, bounds):
    nbytes = eng.de_shard_bytes(K, ds.G)
    total = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda:0")
    for lo, hi in bounds:
        buf = torch.full((nbytes // 8,), -1, dtype=torch.int64, device="cuda:0")
        eng.de_run_shard(ds, code, K, lo, hi, buf.data_ptr())
        eng.synchronize()
        assert int(eng.lib.scc_diag_rank_last_route()) == BUCKETS
        total += buf
    torch.cuda.synchronize()
    return eng.de_finish(ds, code, K, total.data_ptr(), fetch="rows")


def test_runs_that_keep_the_buckets(eng, cfg, monkeypatch):
    """SLOW, the t test and a gene shard on a dataset that holds the order: route 1, equal results."""
    d, code, K = cfg
    ds, (first, _, _), routes = _three_calls(eng, d, code, K)
    assert routes[2] == VORDER
    _on_off(eng, ds, code, K, monkeypatch, want_on=BUCKETS, test="t")
    _same(_shards(eng, ds, code, K, [(0, 333), (333, 1000)]), first)
    sub = synth.from_dense(d.dense()[:200], d.labels)
    dss, _, routes = _three_calls(eng, sub, code, K)
    assert routes[2] == VORDER
    kw = dict(q_val_thrs=0.05, fc_thrs=1.5, mean_scaling_factor=5.0)
    s1 = eng.de_run(dss, code, K, nat.SCC_DE_SLOW, fetch="all", **kw)
    assert int(eng.lib.scc_diag_rank_last_route()) == BUCKETS
    monkeypatch.setenv("SCC_RANK_VORDER", "0")
    s2 = eng.de_run(dss, code, K, nat.SCC_DE_SLOW, fetch="all", **kw)
    assert int(eng.lib.scc_diag_rank_last_route()) == BUCKETS
    for f in ("union", "p", "q", "logfc", "u2", "de"):
        np.testing.assert_array_equal(getattr(s2, f), getattr(s1, f), err_msg=f)
