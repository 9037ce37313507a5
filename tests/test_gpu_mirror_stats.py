"""The per-cluster gene statistics taken from the gene-major mirror
(scc_ingest.hip: k_mir_stats) against the regroup and k_gene_stats they
replace on the value-order route, bit for bit on the fields
tests/test_gpu_rank_vorder.py compares.  The reference computes them per pair
(R/reclusterDEConsensusFast.R: the expm1 row means and detection rates of
ComputePairWiseDE); here they are one pass over a gene's cell-ordered entries,
whose additions are ordered as k_gene_stats orders them.  Every comparison
asserts which route ran (scc_diag_mirror_last_uses bit 0, the rank route, the
ingest path): a silent fallback would pass every equality."""
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

FAST_FIELDS = ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top")
FULL, LEAN, MIRROR = 1, 2, 3  # scc_diag_ingest_last_path
BUCKETS, VORDER = 1, 2        # scc_diag_rank_last_route
STATS = 1                     # scc_diag_mirror_last_uses: the last DE run's statistics came from the mirror
CH = 1024                     # k_mir_stats: entries a chunk
MAX_K = 36                    # k_mir_stats: scc_mirror_stats_max_k()
ST_W = 4                      # k_gene_stats: waves (its pieces)
# nearly every gene tested, so that its avg_logfc, pct1 and pct2 are compared
LOOSE = dict(min_per_cent=0.0, log_fc_thrs=0.0, test_all=True)


@pytest.fixture(scope="module")
def eng():
    e = nat.Engine(0)
    yield e
    e.close()


def _same(a, b):
    np.testing.assert_array_equal(a.union, b.union)
    np.testing.assert_array_equal(a.nodg, b.nodg)
    for f in FAST_FIELDS:
        np.testing.assert_array_equal(getattr(a.rows, f), getattr(b.rows, f), err_msg=f)


def _run(eng, ds, code, K, **kw):
    """The result and (ingest path, rank route, statistics from the mirror)."""
    r = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows", **kw)
    return r, (int(eng.lib.scc_diag_ingest_last_path()), int(eng.lib.scc_diag_rank_last_route()),
               int(eng.lib.scc_diag_mirror_last_uses()) & STATS)


def _three_calls(eng, d, code, K, stats=STATS, **kw):
    """The validating call, the call that builds the mirror and the order, a
    third that reuses them: equal results; the dataset and the first result."""
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    first, w1 = _run(eng, ds, code, K, **kw)
    built, w2 = _run(eng, ds, code, K, **kw)
    again, w3 = _run(eng, ds, code, K, **kw)
    assert (w1, w2, w3) == ((FULL, BUCKETS, 0), (MIRROR, VORDER, stats), (MIRROR, VORDER, stats))
    _same(built, first)
    _same(again, first)
    return ds, first


def _on_off(eng, ds, code, K, monkeypatch, stats=STATS, **kw):
    """The same run with the statistics from the mirror and with SCC_STATS_MIRROR=0; the former's result."""
    on, w_on = _run(eng, ds, code, K, **kw)
    monkeypatch.setenv("SCC_STATS_MIRROR", "0")
    off, w_off = _run(eng, ds, code, K, **kw)
    monkeypatch.delenv("SCC_STATS_MIRROR")
    assert (w_on, w_off) == ((MIRROR, VORDER, stats), (MIRROR, VORDER, 0))
    _same(on, off)
    return on


def _piece(n):
    per_wave = -(-n // ST_W)
    return max(64, -(-per_wave // 64) * 64)  # Lp of a gene of n kept entries


def _hand_matrix():
    """60 genes x 5,000 cells, K = 5, cells alternating between the clusters,
    the last 40 cells unkept.  The sizes are those at which k_mir_stats takes
    another path: around a row of 64, a piece, a chunk."""
    rng = np.random.default_rng(17)
    G, N, K = 60, 5000, 5
    i = np.arange(N)
    code = (i % K).astype(np.int32)
    code[N - 40:] = -1
    kept = np.flatnonzero(code >= 0)
    X = np.zeros((G, N))

    def vals(n):
        return 0.01 + rng.gamma(2.0, 1.0, n)

    def put(g, n, cells=kept):
        X[g, np.sort(rng.choice(cells, n, replace=False))] = vals(n)

    sizes = [1, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 1, len(kept)]
    for g, n in enumerate(sizes):
        put(g, n)
    g = len(sizes)
    put(g, 600, kept[code[kept] == 2])                      # one cluster alone: four pieces of it
    assert -(-600 // _piece(600)) == 4
    put(g + 1, 900, kept[code[kept] != 3])                  # an empty cluster
    for a in range(4):                                      # per-cluster counts that are whole pieces
        put(g + 2, 320, kept[code[kept] == a])
    assert _piece(1280) == 320
    X[g + 3, N - 40:] = vals(40)                            # no kept entry
    put(g + 4, 700)
    X[g + 4, rng.choice(np.flatnonzero(X[g + 4]), 300, replace=False)] *= -1.0  # negative values
    X[g + 5] = vals(N)                                      # every cell, the unkept ones too
    put(g + 6, 3000, np.arange(N))                          # kept and unkept entries over three chunks
    for h in range(g + 7, G):
        lam = np.full(N, 0.6)
        lam[code == h % K] = 3.0
        X[h] = np.log1p(rng.poisson(lam))
    assert [int(np.sum(X[q, kept] != 0)) for q in range(len(sizes))] == sizes
    assert np.sum(X[g + 4] < 0) == 300 and not np.any(X[g + 3, kept])
    return synth.from_dense(X, code.astype(str)), code, K


def test_hand_built_sizes(eng, monkeypatch):
    d, code, K = _hand_matrix()
    ds, first = _three_calls(eng, d, code, K, **LOOSE)
    r = _on_off(eng, ds, code, K, monkeypatch, **LOOSE)
    _same(r, first)
    assert len(np.unique(r.rows.gene)) >= d.G - 2 and np.any(r.rows.pct2 > 0)


@pytest.mark.parametrize("K", [2, 12, 16, 17, 33, 70])
def test_cluster_counts(eng, K, monkeypatch):
    """K <= 16: the lane sums in registers; above, in LDS; 70 is past the
    kernel's limit and keeps regroup + k_gene_stats (clusters past 64 there)."""
    d = synth.generate("A", G=400, N=3000, K=K, seed=9)
    names, code = api.select_clusters(d.labels, 10)
    assert len(names) == K
    stats = STATS if K <= MAX_K else 0
    ds, first = _three_calls(eng, d, code, K, stats=stats, **LOOSE)
    r = _on_off(eng, ds, code, K, monkeypatch, stats=stats, **LOOSE)
    _same(r, first)
    assert len(r.rows.gene) > 0


def test_second_labelling(eng, monkeypatch):
    d = synth.generate("A", G=400, N=3000, K=6, seed=43)
    names, code = api.select_clusters(d.labels, 10)
    ds, _ = _three_calls(eng, d, code, len(names), **LOOSE)
    # another labelling: K = 4, every cluster spread over the whole cell range, 10 % of the cells unkept
    i = np.arange(d.N)
    code2 = np.where(i % 10 == 9, -1, (i % 10) % 4).astype(np.int32)
    r = _on_off(eng, ds, code2, 4, monkeypatch, **LOOSE)
    assert len(r.rows.gene) > 0
    # a fresh dataset under the second labelling gives the same
    _, first2 = _three_calls(eng, d, code2, 4, **LOOSE)
    _same(r, first2)


def test_no_mirror_keeps_the_old_route(eng, monkeypatch):
    d = synth.generate("A", G=400, N=3000, K=6, seed=43)
    names, code = api.select_clusters(d.labels, 10)
    K = len(names)
    _, first = _three_calls(eng, d, code, K, **LOOSE)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    monkeypatch.setenv("SCC_INGEST_MIRROR_MAX_BYTES", "1")
    a, w1 = _run(eng, ds, code, K, **LOOSE)
    b, w2 = _run(eng, ds, code, K, **LOOSE)
    assert (w1, w2) == ((FULL, BUCKETS, 0), (LEAN, BUCKETS, 0))
    _same(a, first)
    _same(b, first)
    monkeypatch.delenv("SCC_INGEST_MIRROR_MAX_BYTES")
    c, w3 = _run(eng, ds, code, K, **LOOSE)  # the limit gone: the mirror and the order are built
    assert w3 == (MIRROR, VORDER, STATS)
    _same(c, first)
