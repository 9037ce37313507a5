"""The dataset's gene-major mirror (scc_ingest.hip: k_mir_regroup) against the
per-call sparse transpose it replaces, bit for bit: a validated sparse
dataset's FAST runs regroup a cell-ordered gene-major copy of the kept entries
by cluster instead of counting, scanning and scattering the CSC again
(reference: R/reclusterDEConsensusFast.R:361-368, the per-pair column subsets
of as.matrix(dataMatrix) that the ingest stands for).  Every comparison also
asserts which ingest ran (scc_diag_ingest_last_path): a silent fallback would
pass every equality."""
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

FAST_FIELDS = ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top")
FULL, LEAN, MIRROR = 1, 2, 3  # scc_diag_ingest_last_path
CHUNK = 2048                  # MR_CH, the regroup's staging chunk (entries of one gene per round)


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
    return r, int(eng.lib.scc_diag_ingest_last_path())


def _mirrored(eng, d):
    """A dataset after its validating call and the call that builds the mirror."""
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    code = np.arange(d.N, dtype=np.int32) % 2
    assert _run(eng, ds, code, 2)[1] == FULL
    assert _run(eng, ds, code, 2)[1] == MIRROR
    return ds


def _on_off(eng, ds, code, K, monkeypatch, **kw):
    """The same run through the mirror and through the transpose; the mirror's result."""
    on, p_on = _run(eng, ds, code, K, **kw)
    monkeypatch.setenv("SCC_INGEST_MIRROR", "0")
    off, p_off = _run(eng, ds, code, K, **kw)
    monkeypatch.delenv("SCC_INGEST_MIRROR")
    assert p_on == MIRROR and p_off in (FULL, LEAN)
    _same(on, off)
    return on


def test_same_results_on_every_path(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    first, p1 = _run(eng, ds, code, K)   # validating read
    built, p2 = _run(eng, ds, code, K)   # builds the mirror and regroups it
    again, p3 = _run(eng, ds, code, K)   # regroups it
    monkeypatch.setenv("SCC_INGEST_MIRROR", "0")
    lean, p4 = _run(eng, ds, code, K)
    monkeypatch.delenv("SCC_INGEST_MIRROR")
    monkeypatch.setenv("SCC_INGEST_FULL", "1")
    full, p5 = _run(eng, ds, code, K)
    assert (p1, p2, p3, p4, p5) == (FULL, MIRROR, MIRROR, LEAN, FULL)
    for r in (built, again, lean, full):
        _same(r, first)
    assert len(first.union) > 20


def test_labels_change_mirror_stays(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    assert _run(eng, ds, code, K)[1] == FULL
    assert _run(eng, ds, code, K)[1] == MIRROR
    # another labelling: K = 4, every cluster spread over the whole cell range, 10 % of the cells unkept
    i = np.arange(d.N)
    code2 = np.where(i % 10 == 9, -1, (i % 10) % 4).astype(np.int32)
    assert K != 4 and abs(np.mean(code2 < 0) - 0.1) < 0.01
    r = _on_off(eng, ds, code2, 4, monkeypatch, min_per_cent=5.0, log_fc_thrs=0.0)
    assert len(r.rows.gene) > 0


def _edge_matrix():
    """G = 70, N = 2 * CHUNK + 35: an empty gene, a gene with one entry, a gene
    nonzero in every cell (three chunks), a gene nonzero in unkept cells only, a
    gene of one cluster only, stored explicit zeros; clusters of 3, 33, 65 and
    131 cells among six, 150 cells unkept, cells in random order."""
    rng = np.random.default_rng(5)
    G, N = 70, 2 * CHUNK + 35
    assert N >= 2 * CHUNK + 1 and N % 64 != 0
    sizes = [3, 33, 65, 131, 1800]
    unkept = 150
    sizes.append(N - sum(sizes) - unkept)
    code = np.concatenate([np.full(s, a) for a, s in enumerate(sizes)] + [np.full(unkept, -1)]).astype(np.int32)
    rng.shuffle(code)
    K = len(sizes)
    lam = np.full((G, N), 0.4)
    for a in range(K):
        lam[10 + 8 * a: 18 + 8 * a, code == a] *= 8.0
    X = np.log1p(rng.poisson(lam).astype(np.float64))
    X[0] = 0.0
    X[1] = 0.0
    X[1, np.flatnonzero(code == 4)[7]] = 1.5
    X[2] = np.log1p(1.0 + rng.poisson(2.0, N))
    X[3] = np.where(code < 0, 1.25, 0.0)
    X[4] = np.where(code == 2, X[2], 0.0)
    d = synth.from_dense(X, code.astype(str))
    assert np.all(np.diff(d.indptr) > 0)
    zero = np.flatnonzero(d.indices >= 10)[:: 997]  # stored explicit zeros
    d.data[zero] = 0.0
    assert len(zero) > 20
    return d, code, K


def test_edge_rows(eng, monkeypatch):
    d, code, K = _edge_matrix()
    ds = _mirrored(eng, d)
    r = _on_off(eng, ds, code, K, monkeypatch, min_per_cent=1.0, log_fc_thrs=0.0)
    assert len(r.rows.gene) > 0


@pytest.mark.parametrize("K,G,N", [(2, 300, 600), (100, 300, 6000)])
def test_cluster_count_limits(eng, K, G, N, monkeypatch):
    d = synth.generate("A", G=G, N=N, K=K, seed=9, sizes="dirichlet")
    names, code = api.select_clusters(d.labels, 10)
    assert len(names) == K and np.all(code >= 0)
    ds = _mirrored(eng, d)
    _on_off(eng, ds, code, K, monkeypatch)


def _shards(eng, ds, code, K, bounds, want):
    nbytes = eng.de_shard_bytes(K, ds.G)
    total = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda:0")
    for lo, hi in bounds:
        buf = torch.full((nbytes // 8,), -1, dtype=torch.int64, device="cuda:0")
        eng.de_run_shard(ds, code, K, lo, hi, buf.data_ptr())
        eng.synchronize()
        path = int(eng.lib.scc_diag_ingest_last_path())
        assert (path == MIRROR) if want else (path in (FULL, LEAN))
        total += buf
    torch.cuda.synchronize()
    return eng.de_finish(ds, code, K, total.data_ptr(), fetch="rows")


def test_gene_shards(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    whole, p = _run(eng, ds, code, K)
    assert p == FULL
    bounds = [(0, 333), (333, 1000)]  # not aligned to the transpose's gene tiles
    on = _shards(eng, ds, code, K, bounds, True)
    monkeypatch.setenv("SCC_INGEST_MIRROR", "0")
    off = _shards(eng, ds, code, K, bounds, False)
    _same(on, off)
    _same(on, whole)


def test_other_modes_and_tests(eng, cfg, monkeypatch):
    d, code, K = cfg
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    assert _run(eng, ds, code, K)[1] == FULL
    assert _run(eng, ds, code, K)[1] == MIRROR
    for test in ("t", "bimod"):  # the same keys feed both: they follow the mirror
        _on_off(eng, ds, code, K, monkeypatch, test=test)
    # SLOW reads every entry (its expm1 mean): the mirror is not taken
    sub = synth.from_dense(d.dense()[:200], d.labels)
    dss = eng.dataset_csc(sub.indptr, sub.indices, sub.data, sub.G, sub.N)
    assert _run(eng, dss, code, K)[1] == FULL
    assert _run(eng, dss, code, K)[1] == MIRROR
    kw = dict(q_val_thrs=0.05, fc_thrs=1.5, mean_scaling_factor=5.0)
    s1 = eng.de_run(dss, code, K, nat.SCC_DE_SLOW, fetch="all", **kw)
    assert int(eng.lib.scc_diag_ingest_last_path()) == FULL
    monkeypatch.setenv("SCC_INGEST_MIRROR", "0")
    s2 = eng.de_run(dss, code, K, nat.SCC_DE_SLOW, fetch="all", **kw)
    assert int(eng.lib.scc_diag_ingest_last_path()) == FULL
    for f in ("union", "p", "q", "logfc", "u2", "de"):
        np.testing.assert_array_equal(getattr(s2, f), getattr(s1, f), err_msg=f)


def test_fallback_and_fresh_mirror(eng, cfg, monkeypatch):
    d, code, K = cfg
    mirror_bytes = 12 * d.nnz  # cells and keys; the gene starts and order on top
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    first, p1 = _run(eng, ds, code, K)
    monkeypatch.setenv("SCC_INGEST_MIRROR_MAX_BYTES", str(mirror_bytes // 2))
    lean, p2 = _run(eng, ds, code, K)
    assert (p1, p2) == (FULL, LEAN)
    _same(lean, first)
    monkeypatch.delenv("SCC_INGEST_MIRROR_MAX_BYTES")
    ds.close()
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)  # a new dataset: validated and mirrored afresh
    again, p3 = _run(eng, ds, code, K)
    built, p4 = _run(eng, ds, code, K)
    assert (p3, p4) == (FULL, MIRROR)
    _same(again, first)
    _same(built, first)
