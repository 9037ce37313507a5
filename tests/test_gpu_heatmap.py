"""The heatmap's inputs on the device (include/scc.h "heatmap inputs";
cellTypeDEPlot.R:168-253): scc_gene_distance and scc_heatmap_raster against
the long-double restatement of tests/heatmap_reference.py, and the ``heatmap``
keyword of the Python mirror end to end.

Shapes: nu in {2, 63, 64, 65, 130} = a partial 64-gene tile, an exact one, one
past it, and three tiles (a tile pair off the diagonal); N in {17, 1000, 4099}
= fewer cells than one 512-cell slab, two slabs with a padding tail (N is no
multiple of 16), and nine slabs (a slab holds at least 512 cells and there are
ceil(Npad / 512) of them at these widths, so 4099 cells are more than one).

Bounds (derived, not measured; u = 2^-53):
  dist      each term fl(x_a - x_b)^2 carries <= 2u, a sum of N non-negative
            terms in any order <= (N - 1) u more, the sqrt halves that and
            adds u: within 2 N u relative of the exact value
  row_mean  a double-double sum rounded once: within 1 ulp
  raster    a sequential sum of n_bin values and one division: within
            n_bin u mean|x| absolute (mean|x| over the bin)
  range     elements of the input: bitwise"""
import numpy as np
import pytest

import heatmap_reference as H
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

LD = np.longdouble
G = 160
NUS = [2, 63, 64, 65, 130]
NS = [17, 1000, 4099]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


def _matrix(N):
    """G x N, ~30 % stored values of both signs; row 1 repeats row 0 exactly."""
    rng = np.random.default_rng(N)
    X = rng.standard_normal((G, N)) * rng.uniform(0.3, 4.0, (G, 1))
    X[rng.random((G, N)) > 0.3] = 0.0
    X[1] = X[0]
    return X


def _genes(nu):
    """nu distinct genes in no particular order; the first two are the identical rows 0 and 1."""
    rest = np.random.default_rng(nu).permutation(np.arange(2, G))[: nu - 2]
    return np.concatenate([[0, 1], rest]).astype(np.int32)


_CACHE = {}


def _case(eng, N):
    """(X, csc dataset) per N, built once and never modified."""
    if N not in _CACHE:
        import scipy.sparse as sp
        X = _matrix(N)
        m = sp.csc_matrix(X)
        m.sort_indices()
        _CACHE[N] = (X, eng.dataset_csc(m.indptr, m.indices, m.data, G, N))
    return _CACHE[N]


_REF = {}


def _ref(X, N, nu):
    if (N, nu) not in _REF:
        B = X[_genes(nu)]
        _REF[(N, nu)] = (H.gene_dist(B), H.row_means(B), H.value_range(B))
    return _REF[(N, nu)]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nu", NUS)
def test_gene_distance(eng, nu, N):
    X, ds = _case(eng, N)
    genes = _genes(nu)
    d, mean, rng = eng.gene_distance(ds, genes)
    dref, mref, rref = _ref(X, N, nu)
    assert d.shape == (nu * (nu - 1) // 2,) and np.isfinite(d).all()
    err = np.abs(d.astype(LD) - dref)
    worst = float(np.max(err / np.maximum(dref, LD(1e-300))))
    print(f"nu={nu} N={N}: worst relative distance error {worst:.3e} (bound {2 * N * U:.3e})")
    assert np.all(err <= 2 * N * U * dref)
    assert d[H.packed_index(nu, 0, 1)] == 0.0  # identical genes: exactly zero
    assert np.all(np.abs(mean.astype(LD) - mref) <= np.spacing(np.abs(mref.astype(np.float64))))
    assert rng.tobytes() == rref.tobytes()
    d2, mean2, rng2 = eng.gene_distance(ds, genes)  # a second call: the same bits
    assert d2.tobytes() == d.tobytes() and mean2.tobytes() == mean.tobytes() and rng2.tobytes() == rng.tobytes()


@pytest.mark.parametrize("N", NS)
def test_csc_csr_dense_give_the_same_bits(eng, N):
    import scipy.sparse as sp
    X, ds = _case(eng, N)
    r = sp.csr_matrix(X)
    r.sort_indices()
    ds_r = eng.dataset_csr(r.indptr, r.indices, r.data, G, N)
    ds_d = eng.dataset_dense(X)
    for nu in (65, 130):
        genes = _genes(nu)
        a = eng.gene_distance(ds, genes)
        for other in (ds_r, ds_d):
            b = eng.gene_distance(other, genes)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    order = np.random.default_rng(5).permutation(N).astype(np.int32) + 1
    genes = _genes(65)
    rows = np.arange(65, 0, -1, dtype=np.int32)
    a = eng.heatmap_raster(ds, genes, rows, order, min(N, 7))
    for other in (ds_r, ds_d):
        assert eng.heatmap_raster(other, genes, rows, order, min(N, 7)).tobytes() == a.tobytes()
    ds_r.close()
    ds_d.close()


def test_range_counts_the_implicit_zeros(eng):
    # two sparse genes whose stored values are all negative: the zeros nobody stored decide max x and min |x|
    import scipy.sparse as sp
    N = 300
    X = np.zeros((5, N))
    X[1, [3, 77, 250]] = [-2.5, -0.125, -7.0]
    X[3, [0, 299]] = [-1.0, -3.0]
    X[2, 10] = 99.0  # not in the union
    m = sp.csc_matrix(X)
    ds = eng.dataset_csc(m.indptr, m.indices, m.data, 5, N)
    _, mean, rng = eng.gene_distance(ds, [3, 1])
    assert rng.tolist() == [-7.0, 0.0, 0.0, 7.0]
    assert rng.tobytes() == H.value_range(X[[3, 1]]).tobytes()
    assert np.all(np.abs(mean.astype(LD) - H.row_means(X[[3, 1]])) <= np.spacing(np.abs(mean)))
    # a dense gene without a zero: min |x| is its smallest magnitude
    Xd = np.full((2, 40), -4.0)
    Xd[1, 7] = -0.5
    dd = eng.dataset_dense(Xd)
    assert eng.gene_distance(dd, [0, 1])[2].tolist() == [-4.0, -0.5, 0.5, 4.0]
    ds.close()
    dd.close()


@pytest.mark.parametrize("N", NS)
def test_raster(eng, N):
    X, ds = _case(eng, N)
    nu = 65
    genes = _genes(nu)
    rng = np.random.default_rng(N + 1)
    rows = rng.permutation(nu).astype(np.int32) + 1
    cells = rng.permutation(N).astype(np.int32) + 1
    B = X[genes]
    full = eng.heatmap_raster(ds, genes, rows, cells, N)
    assert full.tobytes() == np.ascontiguousarray(B[rows - 1][:, cells - 1]).tobytes()  # the reordered matrix itself
    for width in (1, 7, N - 1):
        got = eng.heatmap_raster(ds, genes, rows, cells, width)
        ref, bound = H.raster(B, rows, cells, width)
        assert got.shape == (nu, width)
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        print(f"N={N} width={width}: worst raster error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound)


def test_raster_rejects_a_non_permutation(eng):
    X, ds = _case(eng, 17)
    genes = _genes(63)
    rows = np.arange(1, 64, dtype=np.int32)
    cells = np.arange(1, 18, dtype=np.int32)
    bad_cells = cells.copy()
    bad_cells[4] = bad_cells[5]
    bad_rows = rows.copy()
    bad_rows[0] = 64
    for r, c, w in ((rows, bad_cells, 5), (bad_rows, cells, 5), (rows, cells, 0), (rows, cells, 18)):
        with pytest.raises(nat.SccError) as e:
            eng.heatmap_raster(ds, genes, r, c, w)
        assert e.value.code == nat.SCC_ERR_INVALID
    assert eng.heatmap_raster(ds, genes, rows, cells, 17).shape == (63, 17)


def test_errors(eng):
    import scipy.sparse as sp
    X, ds = _case(eng, 1000)
    for genes in ([5, 9, 5], [7], [3, G], [-1, 3]):
        with pytest.raises(nat.SccError) as e:
            eng.gene_distance(ds, genes)
        assert e.value.code == nat.SCC_ERR_INVALID
    other = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        other.gene_distance(ds, [1, 2])
    assert e.value.code == nat.SCC_ERR_INVALID
    other.close()
    Xn = X[:8, :100].copy()
    Xn[4, 50] = np.nan
    Xn[6, 3] = np.inf
    m = sp.csc_matrix(Xn)
    dn = eng.dataset_csc(m.indptr, m.indices, m.data, 8, 100)
    for genes in ([2, 4, 5], [6, 0]):
        with pytest.raises(nat.SccError) as e:
            eng.gene_distance(dn, genes)
        assert e.value.code == nat.SCC_ERR_NONFINITE
    d, _, _ = eng.gene_distance(dn, [0, 2, 3, 5, 7])  # the rows without one are fine
    assert np.isfinite(d).all()
    dn.close()


def test_kept_distance_survives_the_heatmap_calls(eng):
    X, ds = _case(eng, 1000)
    genes = _genes(65)
    eng.distance(ds, genes, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0)  # kept in the engine
    groups = (np.arange(1000) % 3).astype(np.int32)
    w0, c0 = eng.silhouette(1000, groups)
    s0 = eng.last_pca_scores(1000)
    eng.gene_distance(ds, _genes(130))
    eng.heatmap_raster(ds, _genes(130), np.arange(1, 131), np.arange(1, 1001), 100)
    w1, c1 = eng.silhouette(1000, groups)
    assert w1.tobytes() == w0.tobytes() and c1.tobytes() == c0.tobytes()
    assert eng.last_pca_scores(1000).tobytes() == s0.tobytes()


def test_api_heatmap_keyword(tmp_path):
    d = synth.generate("A")
    kw = dict(deepSplitValues=(1,), minClusterSize=10)
    plain = api.reclusterDEConsensusFast(d, d.labels, **kw)
    assert set(plain) == {"deGeneUnion", "cellTree", "dynamicColors"}
    plot = str(tmp_path / "DE_Heatmap")
    ret = api.reclusterDEConsensusFast(d, d.labels, heatmap=64, return_details=True, save=True,
                                       filename=str(tmp_path / "obj"), plotName=plot, **kw)
    assert set(ret) == {"deGeneUnion", "cellTree", "dynamicColors", "heatmap", "_details"}
    assert ret["deGeneUnion"] == plain["deGeneUnion"] and ret["dynamicColors"] == plain["dynamicColors"]
    hm, uni = ret["heatmap"], ret["_details"]["union_idx"]
    nu = len(uni)
    assert set(hm) == {"rowTree", "rowOrder", "colOrder", "rowMeans", "range", "raster"}
    B = d.dense()[uni]
    dref = H.gene_dist(B)
    merge, height, _ = H.hclust_complete(dref.astype(np.float64), nu)
    merge, order = H.dendro_reorder(merge, -H.row_means(B).astype(np.float64))
    tree = hm["rowTree"]
    assert tree["method"] == "complete"
    assert np.array_equal(tree["merge"], merge)
    assert np.array_equal(tree["order"], order) and np.array_equal(hm["rowOrder"], order)
    np.testing.assert_allclose(tree["height"], height, rtol=2 * d.N * U, atol=0)
    assert np.array_equal(hm["colOrder"], ret["cellTree"]["order"])
    assert hm["range"].tobytes() == H.value_range(B).tobytes()
    assert hm["raster"].shape == (nu, 64)
    ref, bound = H.raster(B, order, hm["colOrder"], 64)
    assert np.all(np.abs(hm["raster"].astype(LD) - ref).astype(np.float64) <= bound)
    z = np.load(plot + ".npz")
    assert z["raster"].tobytes() == hm["raster"].tobytes() and np.array_equal(z["merge"], merge)
    # the stand-alone entry gives the same thing
    hd = api.heatmap_data(d, uni, ret["cellTree"], width=64)
    assert hd["raster"].tobytes() == hm["raster"].tobytes() and np.array_equal(hd["rowTree"]["merge"], merge)
    raw = api.heatmap_data(d, uni, ret["cellTree"], width=5, row_reorder=None)
    assert np.array_equal(raw["rowTree"]["merge"], H.hclust_complete(dref.astype(np.float64), nu)[0])


def test_api_slow_heatmap_keyword():
    d = synth.generate("A")
    kw = dict(qValThrs=0.05, fcThrs=1.5, deepSplitValues=(1,), minClusterSize=10)
    plain = api.reclusterDEConsensus(d, d.labels, **kw)
    assert set(plain) == {"deGeneUnion", "cellTree", "dynamicColors"}
    ret = api.reclusterDEConsensus(d, d.labels, heatmap=True, return_details=True, **kw)
    assert ret["deGeneUnion"] == plain["deGeneUnion"]
    hm, uni = ret["heatmap"], ret["_details"]["union_idx"]
    assert hm["raster"].shape == (len(uni), min(d.N, 4096))  # True: the default width
    B = d.dense()[uni]
    # width == N here: the raster is the matrix in (rowOrder, colOrder) order, bit for bit
    assert hm["raster"].tobytes() == np.ascontiguousarray(B[hm["rowOrder"] - 1][:, hm["colOrder"] - 1]).tobytes()
    assert hm["range"].tobytes() == H.value_range(B).tobytes()
    assert H.is_valid_tree(hm["rowTree"]["merge"], len(uni)) and np.all(np.diff(hm["rowTree"]["height"]) >= 0)
