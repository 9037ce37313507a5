"""The rank stage's run rows (scc_rank_waves.hip: k_rank_mfma16<1, true, true> adds the
cross-bucket term inside each run of a gene's buckets and leaves one histogram
row per run; k_rank_cross_runs, scc_rank_cross.hip, sums over those rows) against the route it
replaces at K <= 16 (a row per bucket, k_rank_cross over buckets;
SCC_RANK_RUNS=0), bit for bit.  The reference ranks every pair's cells again
(R/reclusterDEConsensusFast.R, the wilcox.test calls of the per-pair loop): one
case is compared with the oracle.  Every comparison asserts which route ran
(scc_diag_rank_last_route, scc_diag_rank_last_runs): a silent fallback would
pass every equality.

The matrix is laid out for the chunk logic.  Every gene is ranked (test_all),
the bucket list takes the genes in groups of eight consecutive ones, and every
group's bucket count is a multiple of 16, the chunk at this size: whichever
order the groups reserve their slots in, a gene's place inside its chunk is
the one planned here."""
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

import rank_runs_model as rm
import vorder_model as vm
from scconsensus_amd import _native as nat
from scconsensus_amd import synth

pytestmark = pytest.mark.gpu

FAST_FIELDS = ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top")
VORDER = 2      # scc_diag_rank_last_route
CH = 16         # rk_chunk at this size
N, G, K0 = 2500, 48, 12
KW = dict(min_per_cent=1.0, log_fc_thrs=0.0, test_all=True)


def _nbuckets(x):
    v = np.sort(x[x != 0])
    return len(vm.cuts(v)) if len(v) else 0


def _matrix():
    """48 genes x 2500 cells; the planned slots of the genes the cases are about."""
    rng = np.random.default_rng(17)
    X = np.zeros((G, N))

    def distinct(g, n):  # n stored values in (0, 5), no ties: ceil(n / 64) buckets
        cells = np.sort(rng.choice(N, n, replace=False))
        X[g, cells] = rng.permutation(1.0 + np.arange(n)) / 512

    # group 0: five genes of one bucket, the dense gene (40 buckets from slot 5:
    # chunks 0, 1, 2), a gene that ends on a chunk boundary, a gene of exactly CH buckets
    for g, n in enumerate([30, 64, 1, 50, 10]):
        distinct(g, n)
    distinct(5, N)
    distinct(6, 3 * 64)
    distinct(7, CH * 64)
    # group 1: five buckets, a gene of exactly CH buckets from slot 5 (two runs),
    # the tie gene (27 buckets, a tie group of 200 in the middle), one-bucket genes, a filler
    distinct(8, 5 * 64)
    distinct(9, CH * 64 - 20)
    cells = np.sort(rng.choice(N, 1800, replace=False))
    vals = np.concatenate([0.25 + np.arange(800), np.full(200, 900.0), 1000.25 + np.arange(800)])
    vals[100:140] = np.repeat(vals[100:140:4], 4)      # small tie groups inside ordinary buckets
    vals[1500:1530] = np.repeat(vals[1500:1530:3], 3)
    X[10, cells] = rng.permutation(vals) / 512
    for g in (11, 12, 13, 14):
        distinct(g, int(rng.integers(1, 60)))
    distinct(15, 12 * 64)
    # groups 2 .. 5: small counts (ties everywhere, a cluster effect) and a filler
    # gene that brings the group's buckets to a multiple of CH
    code = _code(K0)
    for g0 in range(16, G, 8):
        for g in range(g0, g0 + 7):
            lam = np.full(N, 0.3 + 0.4 * (g % 5))
            lam[code == g % K0] = 3.0
            X[g] = rng.poisson(lam)
        tot = sum(_nbuckets(X[g]) for g in range(g0, g0 + 7))
        distinct(g0 + 7, 64 * (CH - tot % CH))
    return X


def _code(K, unkept=False):
    i = np.arange(N)
    code = (i % K).astype(np.int32)
    code[N - 30:] = -1
    if unkept:  # a whole cluster's worth of cells spread over every bucket
        code[i % 10 == 9] = -1
    return code


@pytest.fixture(scope="module")
def eng():
    e = nat.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(eng):
    """The matrix, its dataset with the mirror and the value order built, the validating call's result."""
    X = _matrix()
    d = synth.from_dense(X, _code(K0).astype(str))
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    code = _code(K0)
    first = eng.de_run(ds, code, K0, nat.SCC_DE_FAST, fetch="rows", **KW)
    assert int(eng.lib.scc_diag_rank_last_route()) != VORDER
    eng.de_run(ds, code, K0, nat.SCC_DE_FAST, fetch="rows", **KW)
    return X, ds, first


def _same(a, b):
    np.testing.assert_array_equal(a.union, b.union)
    np.testing.assert_array_equal(a.nodg, b.nodg)
    for f in FAST_FIELDS:
        np.testing.assert_array_equal(getattr(a.rows, f), getattr(b.rows, f), err_msg=f)


def _run(eng, ds, code, K, want_runs):
    r = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", **KW)
    assert int(eng.lib.scc_diag_rank_last_route()) == VORDER
    assert int(eng.lib.scc_diag_rank_last_runs()) == want_runs
    return r


def _both(eng, ds, code, K, monkeypatch):
    """The same call with run rows and with SCC_RANK_RUNS=0; the former's result."""
    on = _run(eng, ds, code, K, 1)
    monkeypatch.setenv("SCC_RANK_RUNS", "0")
    off = _run(eng, ds, code, K, 0)
    monkeypatch.delenv("SCC_RANK_RUNS")
    _same(on, off)
    assert {5, 9, 10} <= set(on.rows.gene.tolist())  # the dense, the two-run and the tie gene are among the rows
    return on


def test_layout(data):
    """The plan the other cases rely on, from the cut rule and the kernel's chunk rule."""
    X, _, _ = data
    nb = np.array([_nbuckets(X[g]) for g in range(G)])
    assert np.all(nb > 0)
    grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert rm.chunk(int(nb.sum()), grid) == CH
    assert np.all(nb.reshape(-1, 8).sum(axis=1) % CH == 0)
    at = np.concatenate([np.cumsum(nb[g0:g0 + 8]) - nb[g0:g0 + 8] for g0 in range(0, G, 8)])  # slot within the group
    assert list(nb[:5]) == [1] * 5 and list(at[:5]) == [0, 1, 2, 3, 4]     # five genes share chunk 0 ...
    assert (at[5], nb[5]) == (5, 40)                                         # ... with the dense gene's first run
    assert len(rm.run_rows(at[5], nb[5], CH)) == 3 and at[5] % CH != 0
    assert (at[6] + nb[6]) % CH == 0 and at[6] % CH != 0                     # ends on a chunk boundary
    assert (at[7] % CH, nb[7]) == (0, CH)                                    # exactly one chunk
    assert nb[9] == CH and at[9] % CH != 0 and len(rm.run_rows(at[9], nb[9], CH)) == 2
    v = np.sort(X[10][X[10] != 0])
    bk = vm.cuts(v)
    fat = [q for q, b in enumerate(bk) if b[2]]
    assert len(fat) == 1 and nb[10] == 27
    q = at[10] + fat[0]                                                      # the fat bucket inside a run:
    assert rm.run_ids(at[10], nb[10], CH)[fat[0]] == rm.run_ids(at[10], nb[10], CH)[fat[0] - 1]
    assert rm.run_ids(at[10], nb[10], CH)[fat[0]] == rm.run_ids(at[10], nb[10], CH)[fat[0] + 1]
    assert q % CH not in (0, CH - 1)


def test_runs_against_buckets_and_first_call(eng, data, monkeypatch):
    _, ds, first = data
    _same(_both(eng, ds, _code(K0), K0, monkeypatch), first)
    assert np.any(first.rows.ties > 0)


def test_against_oracle(eng, data):
    import oracle as O
    X, ds, _ = data
    code = _code(K0)
    r = _run(eng, ds, code, K0, 1).rows
    o = O.de_fast(X, code, K0, min_per_cent=1.0, log_fc_thrs=0.0)
    np.testing.assert_array_equal(r.pair_tested, o.pair_tested)
    np.testing.assert_array_equal(r.gene, o.row_gene)
    np.testing.assert_array_equal(r.u2, np.round(2 * o.row_W).astype(np.int64))
    np.testing.assert_array_equal(r.ties, np.round(o.row_ties).astype(np.int64))
    np.testing.assert_allclose(r.p, o.row_p, rtol=1e-6, atol=0)
    assert {5, 9, 10} <= set(r.gene.tolist())  # the dense, the two-run and the tie gene are among the rows


def test_unkept_cluster(eng, data, monkeypatch):
    """Unkept cells (code 255 lanes) inside the buckets of every run."""
    _, ds, _ = data
    code = _code(K0, unkept=True)
    assert np.sum(code < 0) > 250 and len(np.unique(code[code >= 0])) == K0
    _both(eng, ds, code, K0, monkeypatch)


@pytest.mark.parametrize("K", [2, 16])
def test_cluster_counts(eng, data, K, monkeypatch):
    _, ds, _ = data
    _both(eng, ds, _code(K), K, monkeypatch)


@pytest.mark.parametrize("bound", [1, 50_000, 200_000])
def test_forced_flush_inside_runs(eng, data, bound, monkeypatch):
    """SCC_RANK_RUN_BOUND lowers what the 32-bit accumulators may hold.  A run
    of 16 full buckets bounds an entry by sum 2 * 64 * (64 + 64 q) = 278,528,
    the run of the dense tie gene that holds the group of 200 by more: 50,000
    flushes inside every long run and takes the 64-bit path for the buckets
    late in a run (2 * 64 * npre > 50,000 from npre = 391), 200,000 flushes
    once late in a full run and never leaves 32 bits, 1 flushes before every
    bucket."""
    _, ds, first = data
    H = np.full((16, 1), 64, np.int64)
    _, flushes, _ = rm.bounded_local(H, H[:, 0], np.zeros(16, int), bound)
    assert flushes > 0
    monkeypatch.setenv("SCC_RANK_RUN_BOUND", str(bound))
    _same(_both(eng, ds, _code(K0), K0, monkeypatch), first)
