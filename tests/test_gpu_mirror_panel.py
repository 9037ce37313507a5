"""The PCA panel and its column means from the dataset's gene-major mirror
(scc_dist.hip: k_mir_panel, k_mir_colsum) against the CSC gather and k_colsum
they replace, bit for bit (reference: R/reclusterDEConsensusFast.R:398-400,
prcomp_irlba(t(X[U, ]), center = TRUE) and dist of its scores; :403, the
Pearson alternative).  The panel holds the same values in the same places and
the column sums keep k_colsum's partition and order, so the PCA scores, the
packed Euclidean distance and the Pearson distance must not change in any
bit.  Every comparison also asserts which gather ran
(scc_diag_mirror_last_uses, bit 1): a silent fallback would pass every
equality.  No matrix here stores a negative zero (the one value the mirror
does not keep)."""
import numpy as np
import pytest
import torch  # before the engine loads (torch's HIP runtime first)

from scconsensus_amd import _native as nat
from scconsensus_amd import synth

pytestmark = pytest.mark.gpu

FULL, LEAN, MIRROR = 1, 2, 3  # scc_diag_ingest_last_path
PANEL = 2                     # scc_diag_mirror_last_uses: the last PCA gather read the mirror
SEG = 128                     # SCC_MIRROR_SEG, the cells of one segment of the mirror's table


@pytest.fixture(scope="module")
def eng():
    e = nat.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cfg():
    return synth.generate("A", G=1000, N=1500, K=6, seed=43)


def _mirrored(eng, d):
    """A dataset after its validating call and the call that builds the mirror."""
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    code = np.arange(d.N, dtype=np.int32) % 2
    for want in (FULL, MIRROR):
        eng.de_run(ds, code, 2, nat.SCC_DE_FAST, fetch="rows")
        assert int(eng.lib.scc_diag_ingest_last_path()) == want
    return ds


def _outputs(eng, ds, genes, want_mirror):
    """(PCA scores, packed Euclidean distance, Pearson distance) of one route."""
    want = PANEL if want_mirror else 0
    dist = eng.distance(ds, genes, nat.SCC_DIST_PCA_EUCLID)
    assert int(eng.lib.scc_diag_mirror_last_uses()) & PANEL == want
    scores = eng.last_pca_scores(ds.N).copy()
    eng.pca_scores(ds, genes)
    assert int(eng.lib.scc_diag_mirror_last_uses()) & PANEL == want
    np.testing.assert_array_equal(eng.last_pca_scores(ds.N), scores)
    pear = eng.distance(ds, genes, nat.SCC_DIST_PEARSON)
    assert int(eng.lib.scc_diag_mirror_last_uses()) & PANEL == want
    return scores, dist, pear


def _equal(a, b):
    for x, y, name in zip(a, b, ("pca_scores", "distance", "pearson")):
        np.testing.assert_array_equal(x, y, err_msg=name)


def _on_off(eng, ds, genes, monkeypatch):
    on = _outputs(eng, ds, genes, True)
    monkeypatch.setenv("SCC_GATHER_MIRROR", "0")
    off = _outputs(eng, ds, genes, False)
    monkeypatch.delenv("SCC_GATHER_MIRROR")
    _equal(on, off)
    assert np.all(np.isfinite(on[0])) and np.all(np.isfinite(on[1]))
    return on


def _union(G, nu, seed):
    """nu distinct genes, not in ascending order."""
    u = np.random.default_rng(seed).permutation(G)[:nu].astype(np.int32)
    assert np.any(np.diff(u) < 0)
    return u


@pytest.mark.parametrize("nu", [130, 16, 70])
def test_panel_same_as_csc_gather(eng, cfg, nu, monkeypatch):
    ds = _mirrored(eng, cfg)
    s, d, p = _on_off(eng, ds, _union(cfg.G, nu, nu), monkeypatch)
    assert s.shape == (cfg.N, min(nu, 15)) and np.ptp(d) > 0


def _edge_matrix(seed=5):
    """G = 70, N = 2 * 2048 + 35 (no multiple of 16, 64 or the segment): an empty
    gene, a gene whose single entry is in the last cell, a gene nonzero in every
    cell, a gene nonzero in the first cell only, stored explicit (positive)
    zeros in the union's genes."""
    rng = np.random.default_rng(seed)
    G, N = 70, 2 * 2048 + 35
    assert N % 16 != 0 and N % 64 != 0 and N % SEG != 0
    lam = np.full((G, N), 0.4)
    lam[10:40, : N // 3] *= 6.0
    X = np.log1p(rng.poisson(lam).astype(np.float64))
    X[0] = 0.0
    X[1] = 0.0
    X[1, N - 1] = 1.5
    X[2] = np.log1p(1.0 + rng.poisson(2.0, N))
    X[3] = 0.0
    X[3, 0] = 2.25
    d = synth.from_dense(X, (np.arange(N) % 3).astype(str))
    zero = np.flatnonzero(d.indices >= 10)[::97]  # stored explicit zeros
    d.data[zero] = 0.0
    assert len(zero) > 200 and not np.any(np.signbit(d.data))
    union = np.array([12, 0, 33, 1, 2, 3, 5] + list(range(14, 32)) + [69, 10], np.int32)
    assert np.isin(d.indices[zero], union).sum() > 50
    return d, union


def test_edge_matrix(eng, monkeypatch):
    d, union = _edge_matrix()
    ds = _mirrored(eng, d)
    _on_off(eng, ds, union, monkeypatch)


def test_fewer_cells_than_a_segment(eng, monkeypatch):
    d = synth.generate("A", G=300, N=100, K=3, seed=11)   # N < SEG and < 512 mean chunks: one cell a chunk
    assert d.N < SEG
    ds = _mirrored(eng, d)
    _on_off(eng, ds, _union(d.G, 40, 3), monkeypatch)


def test_without_a_mirror_the_csc_gather(eng, cfg):
    genes = _union(cfg.G, 70, 70)
    want = _outputs(eng, _mirrored(eng, cfg), genes, True)
    # no DE run before the distance: no mirror, and the distance builds none
    ds = eng.dataset_csc(cfg.indptr, cfg.indices, cfg.data, cfg.G, cfg.N)
    _equal(_outputs(eng, ds, genes, False), want)
    _equal(_outputs(eng, ds, genes, False), want)
    # a dense dataset never has one
    dd = eng.dataset_dense(cfg.dense())
    _equal(_outputs(eng, dd, genes, False), want)


def test_recreated_dataset_gets_a_fresh_table(eng, monkeypatch):
    d1, union = _edge_matrix(5)
    d2, _ = _edge_matrix(6)   # the same shape, other entries: a stale table would misplace them
    assert d1.nnz != d2.nnz
    ds = _mirrored(eng, d1)
    a = _on_off(eng, ds, union, monkeypatch)
    ds.close()
    ds = _mirrored(eng, d2)
    b = _on_off(eng, ds, union, monkeypatch)
    assert not np.array_equal(a[0], b[0])
