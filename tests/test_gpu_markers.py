"""GPU parity: one-vs-rest marker genes (scc_de_markers) against the oracle.

The reference is the binary-code oracle loop of tests/markers_reference.py
(cluster a -> 0, the other kept cells -> 1, "pair" 0 of O.de_fast).  Bar, as in
tests/test_gpu_de.py: tested sets and their order, u2, ties, pct, the flags and
the union bit-equal; p and q within 1e-6 relative; avg_logFC within 1e-12
relative or 5e-14 absolute.  Every parity fixture must keep the oracle's filter
quantities more than 1e-9 away from the thresholds (asserted)."""
import numpy as np
import pytest

import markers_reference as MR
import oracle as O
from scconsensus_amd import api, synth
from test_gpu_de import _dense_stretch_matrix, _near_tie_dataset

pytestmark = pytest.mark.gpu

PARAMS = {
    "default": dict(),
    "loose": dict(q_val_thrs=0.05, log_fc_thrs=0.25, min_per_cent=10.0, top_n=5),
    "only_pos": dict(only_pos=True),
}


@pytest.fixture(scope="module")
def nat():
    from scconsensus_amd import _native
    return _native


@pytest.fixture(scope="module")
def eng(nat):
    return nat.Engine(0)


@pytest.fixture(scope="module")
def cfg_a():
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    return d, d.dense(), names, code, {}


def _thresholds(kw):
    return kw.get("log_fc_thrs", 0.5), kw.get("min_per_cent", 20.0)


def _reference(X, code, K, kw, cache=None, key=None):
    if cache is not None and key in cache:
        return cache[key]
    ref = MR.reference(X, code, K, **kw)
    MR.check_margins(ref, X, code, K, *_thresholds(kw))
    if cache is not None:
        cache[key] = ref
    return ref


def _pair_index(K):
    return {(i, j): p for p, (i, j) in enumerate((i, j) for i in range(K - 1) for j in range(i + 1, K))}


def _check_all_cells(g, X, code, K, p_rel=1e-6):
    """Every (cluster, gene) u2 and ties (bit-equal) and p (the project's 1e-6
    bar) of a test_all run against R's wilcox.test on (cluster a, the other
    kept cells)."""
    sel = code >= 0
    for a in range(K):
        for gene in range(X.shape[0]):
            po, W, T, _ = O.wilcox_test(X[gene, code == a], X[gene, sel & (code != a)])
            assert g.u2[a, gene] == int(round(2 * W)), (a, gene)
            assert g.ties[a, gene] == int(round(T)), (a, gene)
            if np.isnan(po):
                assert np.isnan(g.p[a, gene]), (a, gene)
            else:
                assert g.p[a, gene] == pytest.approx(po, rel=p_rel), (a, gene)


# ---------------------------------------------------------------- full parity
@pytest.mark.parametrize("layout", ["csc", "dense"])
@pytest.mark.parametrize("which", list(PARAMS))
def test_parity_config_a(eng, cfg_a, which, layout):
    d, X, names, code, cache = cfg_a
    K = len(names)
    assert K == 8
    ref = _reference(X, code, K, PARAMS[which], cache, which)
    assert ref.tested.min() > 1 and len(ref.union) > 20
    ds = eng.dataset_dense(X) if layout == "dense" else eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    g = eng.de_markers(ds, code, K, fetch="rows", **PARAMS[which])
    assert g.n_pairs == K
    MR.compare(g, ref)
    np.testing.assert_array_equal(g.nodg, O.nodg(X))
    ds.close()


def test_parity_edge_fixture(eng):
    """grey / grey60 / tiny are excluded: -1 codes, explicit ties, negatives."""
    d = synth.edge_fixture()
    names, code = api.select_clusters(d.labels, 10)
    assert (code < 0).any() and "grey" not in names and "tiny" not in names
    X = d.dense()
    kw = dict(log_fc_thrs=0.1, min_per_cent=17.0)
    ref = _reference(X, code, len(names), kw)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    MR.compare(eng.de_markers(ds, code, len(names), fetch="rows", **kw), ref)


def test_exact_branch(eng):
    """n_a = 40 and n_rest = 45: R's exact pwilcox for the 40-cell cluster on
    tie-free, zero-free genes; the 25- and 20-cell clusters have a rest of 60
    and 65 cells and take the normal approximation."""
    rng = np.random.default_rng(17)
    sizes = [40, 25, 20]
    code = np.concatenate([np.repeat(np.arange(3), sizes), -np.ones(15, int)]).astype(np.int32)
    rng.shuffle(code)
    N = len(code)
    X = np.zeros((8, N))
    for g in range(6):  # tie-free, zero-free
        X[g] = rng.permutation(N) / 7.0 + 0.5 + g + np.where(code == g % 3, (3.0 + 1.0 / 14.0) * (g % 2), 0.0)
    X[6] = np.round(rng.gamma(2.0, 1.0, N), 1)                       # ties: normal everywhere
    X[7] = np.where(rng.random(N) < 0.5, rng.gamma(2.0, 1.0, N), 0)  # zeros: tied
    ds = eng.dataset_dense(X)
    g = eng.de_markers(ds, code, 3, fetch="all")
    sel = code >= 0
    for a in range(3):
        for gene in range(8):
            po, W, T, meth = O.wilcox_test(X[gene, code == a], X[gene, sel & (code != a)])
            assert meth == ("exact" if a == 0 and gene < 6 else "normal"), (a, gene)
            assert g.u2[a, gene] == int(round(2 * W))
            assert g.p[a, gene] == pytest.approx(po, rel=1e-13), (a, gene)


# ---------------------------------------------------------------- rank paths
@pytest.mark.parametrize("which", ["near_tie", "stretch_0.9", "stretch_0.07", "nested_0.02", "nested_0.07"])
def test_rank_paths_value_structure(eng, which):
    """The all-pairs route's hard value layouts (last-bit neighbours, a crowded
    stretch of the value axis, a stretch inside the stretch), every
    (cluster, gene) cell."""
    if which == "near_tie":
        d, X = _near_tie_dataset()
    elif which.startswith("stretch"):
        d, X = _dense_stretch_matrix(frac=float(which.split("_")[1]))
    else:
        d, X = _dense_stretch_matrix(frac=float(which.split("_")[1]), nested=150)
    names, code = api.select_clusters(d.labels, 10)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    g = eng.de_markers(ds, code, len(names), fetch="all")
    _check_all_cells(g, X, code, len(names))


def test_rank_paths_special_genes(eng):
    """One value repeated in 100 cells across clusters; exactly 63, 64 and 65
    nonzeros; every selected cell equal (p is NaN); with excluded cells."""
    rng = np.random.default_rng(23)
    K, N = 4, 400
    code = rng.integers(-1, K, N).astype(np.int32)
    X = np.zeros((7, N))
    X[0, rng.choice(N, 100, replace=False)] = 2.5
    for g, n in ((1, 63), (2, 64), (3, 65)):
        X[g, rng.choice(N, n, replace=False)] = np.round(rng.gamma(2.0, 1.0, n), 1) + 0.1
    X[4] = 1.25
    X[5, rng.choice(N, 100, replace=False)] = 2.5
    X[5, rng.choice(N, 30, replace=False)] = -1.0
    X[6] = rng.normal(0.0, 1.0, N)
    ds = eng.dataset_dense(X)
    g = eng.de_markers(ds, code, K, fetch="all")
    _check_all_cells(g, X, code, K)
    assert np.isnan(g.p[:, 4]).all()
    n_sel = int((code >= 0).sum())
    assert (g.ties[:, 4] == n_sel ** 3 - n_sel).all()


def test_rank_paths_size_classes(eng):
    """Genes at the edges of the kernel's size classes: 2047 / 2048 / 2049
    nonzeros (the 256-thread class ends at 2048), 8192 / 8193 (one LDS chunk
    ends at 8192) and 17000 (three chunks, more than the 8,192 values of the
    all-pairs split's large-gene path), ties across chunks included."""
    rng = np.random.default_rng(29)
    K, N = 3, 17000
    code = rng.integers(0, K, N).astype(np.int32)
    sizes = [2047, 2048, 2049, 8192, 8193, 17000, 9000, 9000]
    X = np.zeros((len(sizes), N))
    for g, n in enumerate(sizes):
        idx = rng.choice(N, n, replace=False)
        v = rng.gamma(2.0, 1.0, n) + 0.01
        X[g, idx] = np.round(v, 2) if g % 2 else v  # odd genes: heavy ties
    X[7] = np.where(X[7] != 0, 3.0, 0.0)            # 9000 copies of one value
    ds = eng.dataset_dense(X)
    g = eng.de_markers(ds, code, K, fetch="all")
    _check_all_cells(g, X, code, K)


def test_rank_paths_bucket_limit(eng):
    """900,000 nonzeros: more than the kernel's 256 value-range buckets hold at
    their expected size, so its buckets grow past the splitter spacing; one
    continuous gene, one rounded to a grid (ties across bucket borders' values)."""
    rng = np.random.default_rng(31)
    K, N = 3, 900000
    code = rng.integers(0, K, N).astype(np.int32)
    v = rng.gamma(2.0, 1.0, N) + 0.01
    X = np.stack([v, np.round(v, 3)])
    ds = eng.dataset_dense(X)
    g = eng.de_markers(ds, code, K, fetch="all")
    _check_all_cells(g, X, code, K)
    ds.close()


# ---------------------------------------------------------------- K sweep
@pytest.mark.parametrize("k", [2, 3, 16, 17, 64, 65, 128])
def test_k_sweep_against_all_pairs_route(eng, nat, k):
    """2U_a = sum over b != a of the all-pairs route's 2U_ab, bit for bit
    (orientation: 2 n_a n_b - u2(b, a) for b < a); ties identical across the
    clusters of a gene; k = 2: cluster 0's row is the pair route's pair (0, 1);
    k <= 17: full parity with the binary-code oracle too."""
    # (the generator gives every cluster >= 30 cells: 128 clusters need more than 2500)
    d = synth.generate("A", G=200, N=2500 if k <= 65 else 4608, K=k, seed=100 + k)
    names, code = api.select_clusters(d.labels, 2)
    assert len(names) == k
    kw = dict(min_per_cent=5.0, log_fc_thrs=0.1)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    m = eng.de_markers(ds, code, k, fetch="all", **kw)
    pr = eng.de_run(ds, code, k, nat.SCC_DE_FAST, fetch="all", **kw)
    n = np.bincount(code[code >= 0], minlength=k).astype(np.int64)
    pidx = _pair_index(k)
    want = np.zeros((k, d.G), np.int64)
    for (i, j), p in pidx.items():
        want[i] += pr.u2[p]
        want[j] += 2 * n[i] * n[j] - pr.u2[p]
    np.testing.assert_array_equal(m.u2, want)
    assert (m.ties == m.ties[0]).all()
    if k == 2:
        # (one pair: the filters see the same two groups, so even the tested rows coincide)
        np.testing.assert_array_equal(m.u2[0], pr.u2[0])
        np.testing.assert_array_equal(m.p[0], pr.p[0])
        s = slice(0, int(m.rows.pair_tested[0]))
        np.testing.assert_array_equal(m.rows.gene[s], pr.rows.gene)
        np.testing.assert_array_equal(m.rows.ties[s], pr.rows.ties)
        np.testing.assert_array_equal(m.rows.u2[s], pr.rows.u2)
        np.testing.assert_array_equal(m.rows.p[s], pr.rows.p)
    if k <= 17:
        MR.compare(m, _reference(d.dense(), code, k, kw))


# ---------------------------------------------------------------- determinism and refusals
def test_determinism_and_layouts(eng, cfg_a):
    d, X, names, code, _ = cfg_a
    K = len(names)
    csc = d.scipy_csc()
    csr = csc.tocsr()
    sets = [eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N),
            eng.dataset_csr(csr.indptr, csr.indices, csr.data, d.G, d.N), eng.dataset_dense(X)]
    runs = [eng.de_markers(sets[0], code, K, fetch="all") for _ in range(2)]
    runs += [eng.de_markers(s, code, K, fetch="all") for s in sets[1:]]
    a = runs[0]
    for b in runs[1:]:
        for f in ("p", "logfc", "u2", "ties", "union", "nodg"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
        for f in ("pair_tested", "gene", "p", "q", "avg_logfc", "pct1", "pct2", "u2", "ties", "de", "top"):
            assert getattr(a.rows, f).tobytes() == getattr(b.rows, f).tobytes(), f


def test_refusals_leave_the_context_usable(eng, nat, cfg_a):
    d, X, names, code, _ = cfg_a
    K = len(names)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    before = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows")

    def refused(code_, K_, **kw):
        with pytest.raises(nat.SccError) as e:
            eng.de_markers(ds, code_, K_, **kw)
        return e.value.code

    assert refused(np.where(code == 0, 0, -1).astype(np.int32), 1) == nat.SCC_ERR_INVALID
    two = code.copy()
    two[np.flatnonzero(code == 1)[2:]] = -1  # cluster 1 keeps 2 cells
    assert refused(two, K) == nat.SCC_ERR_RSTOP
    assert refused(code, 129) == nat.SCC_ERR_UNSUPPORTED
    assert refused(code, K, test="t") == nat.SCC_ERR_UNSUPPORTED
    assert refused(code, K, test="bimod") == nat.SCC_ERR_UNSUPPORTED
    import ctypes
    prm = nat.MarkersParams(30, 0, nat.SCC_TEST_WILCOX, 0, 0.1, 0.5, 20.0)
    prm.reserved[2] = 7  # reserved fields must be zero
    r = ctypes.c_void_p()
    assert eng.lib.scc_de_markers(eng.ctx, ds.handle, code.ctypes.data_as(ctypes.c_void_p), K, ctypes.byref(prm),
                                  ctypes.byref(r)) == nat.SCC_ERR_INVALID
    assert not r.value
    after = eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="rows")
    for f in ("pair_tested", "gene", "p", "q", "avg_logfc", "u2", "ties", "de", "top"):
        assert getattr(before.rows, f).tobytes() == getattr(after.rows, f).tobytes(), f
    np.testing.assert_array_equal(before.union, after.union)
    # and the markers call itself still runs
    assert eng.de_markers(ds, code, K, fetch="union").n_pairs == K


# ---------------------------------------------------------------- the public function
def test_find_all_markers_end_to_end(cfg_a, nat):
    d, X, names, code, cache = cfg_a
    K = len(names)
    ref = _reference(X, code, K, {}, cache, "default")
    e = api._engine(0)
    ds = e.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    e.distance(ds, ref.union, nat.SCC_DIST_PCA_EUCLID)  # the engine keeps its device copy
    groups = (np.arange(d.N) % 5 + 1).astype(np.int32)
    w0, avg0 = e.silhouette(d.N, groups)  # (reads the kept distance)
    out = api.findAllMarkers(d.scipy_csc(), d.labels, gene_names=d.gene_names)
    assert out["clusters"] == names
    np.testing.assert_array_equal(out["union_idx"], ref.union)
    assert out["union"] == [d.gene_names[g] for g in ref.union]
    starts = np.concatenate([[0], np.cumsum(ref.tested)])
    for a, name in enumerate(names):
        t = out["markers"][name]
        s = slice(int(starts[a]), int(starts[a + 1]))
        np.testing.assert_array_equal(t["gene_idx"], ref.gene[s])
        assert list(t["gene"]) == [d.gene_names[g] for g in ref.gene[s]]
        np.testing.assert_allclose(t["p_val"], ref.p[s], rtol=1e-6, atol=0)
        np.testing.assert_allclose(t["p_val_adj"], ref.q[s], rtol=1e-6, atol=0)
        np.testing.assert_allclose(t["avg_logFC"], ref.lfc[s], rtol=1e-12, atol=5e-14)
        np.testing.assert_array_equal(t["pct.1"], ref.pct1[s])
        np.testing.assert_array_equal(t["pct.2"], ref.pct2[s])
        np.testing.assert_array_equal(t["kept"], ref.de[s])
        np.testing.assert_array_equal(t["top"], ref.top[s])
    # the distance an earlier scc_distance left in the engine survives the call
    w1, avg1 = e.silhouette(d.N, groups)
    np.testing.assert_array_equal(w0, w1)
    np.testing.assert_array_equal(avg0, avg1)
