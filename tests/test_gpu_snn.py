"""GPU: the SNN graph and the modularity clustering on the engine
(scc_snn_graph, scc_modularity_cluster, scc_snn_clusters_scores;
api.find_clusters), against the NumPy restatement in snn_reference.

Graph.  indptr, cols and the shared counts exactly the reference's, vals bit
for bit (a value is one f64 division of two small integers), on the engine's
own k-NN tables, a hub table, duplicate points and prune = 0 and 1.

Clustering.  The weights are integers and the gain and Q are evaluated in one
written order, so labels, cluster, level and sweep counts and the bits of the
modularity equal the reference's.

Agreement with Seurat, igraph or leidenalg is not tested: none is installed."""
import ctypes

import numpy as np
import pytest
import torch

import snn_reference as sr
import umap_reference as ur
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth
from test_gpu_hclust_scores import _device_scores
from test_snn_reference import _csr, cliques, ring_of_cliques

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 16, 17, 63, 64, 65, 257, 1025, 3000]
KS = [1, 2, 15, 19, 32, 64]
CASES = [(n, k) for n in SIZES for k in KS if k <= n - 1]
assert {n for n, _ in CASES} == set(SIZES) and {k for _, k in CASES} == set(KS)
GAMMAS = [0.2, 1.0, 2.0]
PRUNE = 1.0 / 15.0


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


_POINTS = {}


def _points(n):
    """Eight unit-spread blobs in 8 dimensions around centres of scale 1.5 (they touch: several levels and sweeps)."""
    if n not in _POINTS:
        x, _ = sr.blobs(n, 1.5, seed=1)
        x.setflags(write=False)
        _POINTS[n] = {"x": x, "t": _device_scores(x)}
    return _POINTS[n]


_TABLES = {}


def _table(eng, n, k):
    """The engine's own k-NN table of the blob scores and the reference SNN graph of it, once."""
    if (n, k) not in _TABLES:
        idx, _ = eng.knn_scores(n, k, 0, _points(n)["t"].data_ptr())
        ref = sr.snn_graph(idx, PRUNE)
        for a in (idx,) + ref:
            a.setflags(write=False)
        _TABLES[(n, k)] = (idx, ref)
    return _TABLES[(n, k)]


def _assert_graph(got, ref):
    indptr, cols, vals, shared = got
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64 and shared.dtype == np.int32
    assert np.array_equal(indptr, ref[0]) and np.array_equal(cols, ref[1]) and np.array_equal(shared, ref[3])
    assert np.array_equal(_bits(vals), _bits(ref[2]))


def _assert_symmetric(indptr, cols, vals):
    n = len(indptr) - 1
    row = np.repeat(np.arange(n), np.diff(indptr))
    fwd = dict(zip(zip(row.tolist(), cols.tolist()), _bits(vals).tolist()))
    assert len(fwd) == len(cols) and all(fwd.get((j, i)) == v for (i, j), v in fwd.items())


# ------------------------------------------------------------------ 1. graph
@pytest.mark.parametrize("n,k", CASES)
def test_graph_of_the_engine_table(eng, n, k):
    idx, ref = _table(eng, n, k)
    got = eng.snn_graph(idx, PRUNE, return_shared=True)
    print(f"n={n} k={k}: nnz {got[0][-1]}, longest row {int(np.diff(got[0]).max())}")
    _assert_graph(got, ref)
    if n <= 257:
        _assert_symmetric(*got[:3])
    assert all(np.all(np.diff(got[1][got[0][r]:got[0][r + 1]]) > 0) for r in range(0, n, max(1, n // 50)))


def _hub_table(n=300):
    """Every row lists cell 0 (row 0: cells 1 and 2): every pair shares it."""
    return np.array([[1, 2]] + [[0, 1 + i % (n - 1)] for i in range(1, n)], np.int32)


def test_hub_table_keeps_every_pair(eng):
    idx = _hub_table()
    got = eng.snn_graph(idx, PRUNE, return_shared=True)
    _assert_graph(got, sr.snn_graph(idx, PRUNE))
    assert np.all(np.diff(got[0]) == 299) and got[0][-1] == 300 * 299
    assert np.array_equal(got[1][:299], np.arange(1, 300))
    _assert_symmetric(*got[:3])


def test_duplicate_points(eng):
    x = np.array(_points(257)["x"])
    x[40:80] = x[40]
    x[200:] = x[5]
    t = _device_scores(x)
    for k in (3, 19, 64):
        idx, _ = eng.knn_scores(257, k, 0, t.data_ptr())
        _assert_graph(eng.snn_graph(idx, PRUNE, return_shared=True), sr.snn_graph(idx, PRUNE))


@pytest.mark.parametrize("prune", [0.0, 1.0])
@pytest.mark.parametrize("n,k", [(2, 1), (65, 19), (1025, 15)])
def test_prune_at_its_ends(eng, n, k, prune):
    idx, _ = _table(eng, n, k)
    got = eng.snn_graph(idx, prune, return_shared=True)
    _assert_graph(got, sr.snn_graph(idx, prune))
    if prune == 1.0:
        assert np.all(got[3] == k + 1)
    if n == 2:
        assert got[1].tolist() == [1, 0] and got[2].tolist() == [1.0, 1.0]


def test_prune_boundary_is_kept(eng):
    n, k = 16, 7  # K = 8, s = 1: w = 1 / 15 is the default prune itself
    idx = np.array([[(i + t) % n for t in range(1, k + 1)] for i in range(n)], np.int32)
    got = eng.snn_graph(idx, PRUNE, return_shared=True)
    _assert_graph(got, sr.snn_graph(idx, PRUNE))
    assert (got[3] == 1).any()


def test_cap_too_small_then_the_second_call(eng):
    idx, ref = _table(eng, 257, 19)
    need = int(ref[0][-1])
    with pytest.raises(nat.SccError) as e:
        eng.snn_graph(idx, PRUNE, cap=need - 1)
    assert e.value.code == nat.SCC_ERR_INVALID
    indptr, cols, vals = np.zeros(258, np.int64), np.empty(8, np.int32), np.empty(8)
    nnz = ctypes.c_int64()
    rc = eng.lib.scc_snn_graph(eng.ctx, 257, 19, nat._ptr(np.ascontiguousarray(idx)), PRUNE, nat._ptr(indptr),
                               nat._ptr(cols), nat._ptr(vals), None, 8, ctypes.byref(nnz))
    assert rc == nat.SCC_ERR_INVALID and nnz.value == need
    _assert_graph(eng.snn_graph(idx, PRUNE, return_shared=True, cap=nnz.value), ref)


def _bad_tables():
    idx = _hub_table()
    out = {}

    def case(name, code, i=None, prune=PRUNE):
        out[name] = (np.array(idx) if i is None else i, prune, code)
    i = np.array(idx); i[3, 1] = -1
    case("index -1", nat.SCC_ERR_INVALID, i=i)
    i = np.array(idx); i[3, 1] = 300
    case("index n", nat.SCC_ERR_INVALID, i=i)
    i = np.array(idx); i[3, 1] = i[3, 0]
    case("index twice", nat.SCC_ERR_INVALID, i=i)
    i = np.array(idx); i[7, 1] = 7
    case("row lists itself", nat.SCC_ERR_INVALID, i=i)
    case("n = 1", nat.SCC_ERR_INVALID, i=np.zeros((1, 1), np.int32))
    case("k = 0", nat.SCC_ERR_INVALID, i=idx[:, :0])
    case("k = n", nat.SCC_ERR_INVALID, i=np.zeros((5, 5), np.int32))
    case("k = 65", nat.SCC_ERR_UNSUPPORTED, i=np.tile(np.arange(1, 66, dtype=np.int32), (300, 1)))
    case("prune -0.1", nat.SCC_ERR_INVALID, prune=-0.1)
    case("prune 1.5", nat.SCC_ERR_INVALID, prune=1.5)
    case("prune nan", nat.SCC_ERR_NONFINITE, prune=np.nan)
    case("prune inf", nat.SCC_ERR_NONFINITE, prune=np.inf)
    return out


BAD_TABLES = _bad_tables()


def _knn_baseline(eng):
    return eng.knn_scores(257, 15, 8, _points(257)["t"].data_ptr())


def _assert_knn_unchanged(eng, before):
    idx, dist = _knn_baseline(eng)
    assert np.array_equal(idx, before[0]) and np.array_equal(_bits(dist), _bits(before[1]))


@pytest.mark.parametrize("what", list(BAD_TABLES))
def test_graph_refusals(eng, what):
    before = _knn_baseline(eng)
    idx, prune, code = BAD_TABLES[what]
    with pytest.raises(nat.SccError) as e:
        eng.snn_graph(idx, prune)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


# ------------------------------------------------------------- 2. clustering
def _assert_clustering(got, ref, tag=""):
    print(f"{tag}: clusters {got['n_clusters']}, levels {got['n_levels']}, sweeps {got['sweeps']}, "
          f"Q {got['modularity']:.6f}")
    assert got["labels"].dtype == np.int32
    assert got["n_levels"] == ref["n_levels"] and got["sweeps"] == ref["sweeps"]
    assert got["n_clusters"] == ref["n_clusters"] and np.array_equal(got["labels"], ref["labels"])
    assert _bits(got["modularity"]).item() == _bits(ref["modularity"]).item()


_REFS = {}


def _reference(key, graph, gamma):
    if (key, gamma) not in _REFS:
        _REFS[(key, gamma)] = sr.modularity_cluster(*graph[:3], gamma)
    return _REFS[(key, gamma)]


@pytest.mark.parametrize("n,gamma", [(n, g) for n in (17, 65, 257, 1025) for g in GAMMAS] + [(3000, 1.0)])
def test_clustering_of_the_snn_graph(eng, n, gamma):
    k = min(19, n - 1)
    _, g = _table(eng, n, k)
    keep = [np.array(a) for a in g[:3]]
    got = eng.modularity_cluster(*g[:3], gamma)
    _assert_clustering(got, _reference(("snn", n), g, gamma), f"n={n} gamma={gamma}")
    again = eng.modularity_cluster(*g[:3], gamma)  # two calls return the same bits
    _assert_clustering(again, got)
    assert all(np.array_equal(a, b) for a, b in zip(keep, g[:3]))  # the inputs are untouched
    if n >= 257:
        assert got["n_levels"] >= 2 and got["n_clusters"] <= n // 8  # (gamma = 0.2 may leave one cluster)


def test_clustering_of_a_umap_graph(eng):
    n = 1025
    idx, dist = eng.knn_scores(n, 14, 0, _points(n)["t"].data_ptr())
    g = eng.umap_graph(idx, dist)
    for gamma in (1.0, 0.2):
        _assert_clustering(eng.modularity_cluster(*g, gamma), sr.modularity_cluster(*g, gamma), f"umap gamma={gamma}")


def test_cliques_and_ring(eng):
    two = eng.modularity_cluster(*cliques([7, 5]), 1.0)
    _assert_clustering(two, sr.modularity_cluster(*cliques([7, 5]), 1.0), "two cliques")
    assert two["labels"].tolist() == [0] * 7 + [1] * 5
    ring = eng.modularity_cluster(*ring_of_cliques(), 1.0)
    _assert_clustering(ring, sr.modularity_cluster(*ring_of_cliques(), 1.0), "ring")
    assert ring["labels"].tolist() == [c for c in range(8) for _ in range(6)]
    pair = eng.modularity_cluster(*_csr(2, [(0, 1, 0.5)]), 1.0)
    assert pair["labels"].tolist() == [0, 0] and pair["sweeps"] == [2, 1] and pair["modularity"] == 0.0


def test_rows_longer_than_the_lds_table(eng):
    g = eng.snn_graph(_hub_table(), PRUNE)  # every row holds 299 entries
    for gamma in GAMMAS:
        _assert_clustering(eng.modularity_cluster(*g, gamma), sr.modularity_cluster(*g, gamma), f"hub gamma={gamma}")
    # a coarse level with a long row: a star of 400 cliques of 3 around one clique
    sizes = [3] * 401
    star = cliques(sizes, [(0, 3 * c, 0.25) for c in range(1, 401)])
    _assert_clustering(eng.modularity_cluster(*star, 1.0), sr.modularity_cluster(*star, 1.0), "star")


def test_isolated_vertices_and_vanishing_weights(eng):
    g = cliques([5, 1, 4, 1, 1])
    got = eng.modularity_cluster(*g, 1.0)
    _assert_clustering(got, sr.modularity_cluster(*g, 1.0), "isolated")
    assert got["n_clusters"] == 5 and got["labels"].tolist() == [0] * 5 + [2] + [1] * 4 + [3, 4]
    tiny = 2.0 ** -34  # rint(2^-34 2^32) = 0: the bridges are absent
    g = cliques([4, 4, 3], [(3, 4, tiny), (7, 8, tiny), (0, 10, 2.0 ** -33)])
    got = eng.modularity_cluster(*g, 1.0)
    _assert_clustering(got, sr.modularity_cluster(*g, 1.0), "vanishing")
    assert got["n_clusters"] == 3
    nothing = eng.modularity_cluster(*_csr(3, [(0, 1, 1e-12)]), 1.0)
    assert nothing["labels"].tolist() == [0, 1, 2] and nothing["n_levels"] == 0 and nothing["modularity"] == 0.0
    empty = eng.modularity_cluster(np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0), 1.0)
    assert empty["labels"].tolist() == [0, 1, 2, 3] and empty["n_clusters"] == 4


def _bad_graphs():
    ip, cl, vl = ring_of_cliques()
    out = {}

    def case(name, code, indptr=ip, cols=cl, vals=vl, gamma=1.0):
        out[name] = (np.array(indptr), np.array(cols), np.array(vals), gamma, code)
    c = np.array(cl); c[0] = 0
    case("diagonal entry", nat.SCC_ERR_INVALID, cols=c)
    v = np.array(vl); v[0] = v[ip[1]] = -1.0
    case("negative weight", nat.SCC_ERR_INVALID, vals=v)
    v = np.array(vl); v[0] = np.nextafter(1.0, 2.0)
    case("transpose differs", nat.SCC_ERR_INVALID, vals=v)
    i2 = np.array(ip); i2[1:] -= 1
    case("transpose missing", nat.SCC_ERR_INVALID, indptr=i2, cols=cl[1:], vals=vl[1:])
    i2 = np.array(ip); i2[0] = 1
    case("indptr from 1", nat.SCC_ERR_INVALID, indptr=i2)
    i2 = np.array(ip); i2[3] = i2[2] - 1
    case("indptr descends", nat.SCC_ERR_INVALID, indptr=i2)
    c = np.array(cl); c[4] = 48
    case("column n", nat.SCC_ERR_INVALID, cols=c)
    c = np.array(cl); c[1], c[2] = c[2], c[1]
    case("columns not ascending", nat.SCC_ERR_INVALID, cols=c)
    case("gamma 0", nat.SCC_ERR_INVALID, gamma=0.0)
    case("gamma -1", nat.SCC_ERR_INVALID, gamma=-1.0)
    case("gamma nan", nat.SCC_ERR_NONFINITE, gamma=np.nan)
    case("gamma inf", nat.SCC_ERR_NONFINITE, gamma=np.inf)
    for name, x in (("nan", np.nan), ("inf", np.inf)):
        v = np.array(vl); v[0] = v[ip[1]] = x
        case("weight " + name, nat.SCC_ERR_NONFINITE, vals=v)
    v = np.array(vl); v[0] = v[ip[1]] = 2.0 ** 20 + 1.0
    case("weight above 2^20", nat.SCC_ERR_UNSUPPORTED, vals=v)
    big = cliques([33])  # 1056 entries of 2^52: m2 >= 2^62
    case("m2 2^62", nat.SCC_ERR_UNSUPPORTED, indptr=big[0], cols=big[1], vals=big[2] * 2.0 ** 20)
    return out


BAD_GRAPHS = _bad_graphs()


@pytest.mark.parametrize("what", list(BAD_GRAPHS))
def test_clustering_refusals(eng, what):
    before = _knn_baseline(eng)
    ip, cl, vl, gamma, code = BAD_GRAPHS[what]
    with pytest.raises(nat.SccError) as e:
        eng.modularity_cluster(ip, cl, vl, gamma)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


def test_the_largest_weight_is_taken(eng):
    g = cliques([4, 3])
    g = (g[0], g[1], g[2] * 2.0 ** 20)
    _assert_clustering(eng.modularity_cluster(*g, 1.0), sr.modularity_cluster(*g, 1.0), "2^20")


# ------------------------------------------------------- 3. the fused call
@pytest.mark.parametrize("n,kp,dims,gamma", [(65, 20, 0, 1.0), (1025, 20, 8, 0.8), (3000, 33, 0, 0.2)])
def test_fused_call_equals_the_three_calls(eng, n, kp, dims, gamma):
    p = _points(n)
    out = eng.snn_clusters_scores(n, kp, dims, PRUNE, gamma, p["t"].data_ptr(), return_graph=True)
    idx, _ = eng.knn_scores(n, kp - 1, dims, p["t"].data_ptr())
    g = eng.snn_graph(idx, PRUNE)
    assert np.array_equal(out["graph"][0], g[0]) and np.array_equal(out["graph"][1], g[1])
    assert np.array_equal(_bits(out["graph"][2]), _bits(g[2])) and out["nnz"] == g[0][-1]
    _assert_clustering(out, eng.modularity_cluster(*g, gamma), f"fused n={n}")
    alone = eng.snn_clusters_scores(n, kp, dims, PRUNE, gamma, p["t"].data_ptr())
    _assert_clustering(alone, out)
    assert "graph" not in alone and alone["nnz"] == out["nnz"]


def test_fused_dims_equals_a_zeroed_copy(eng):
    n = 1025
    p = _points(n)
    z = np.array(p["x"])
    z[:, 5:] = 0.0
    tz = _device_scores(z)
    before = p["t"].clone()
    a = eng.snn_clusters_scores(n, 20, 5, PRUNE, 0.8, p["t"].data_ptr())
    b = eng.snn_clusters_scores(n, 20, 0, PRUNE, 0.8, tz.data_ptr())
    torch.cuda.synchronize()
    _assert_clustering(a, b)
    assert torch.equal(p["t"], before)


FUSED_BAD = {
    "k_param = 1": (dict(k_param=1), nat.SCC_ERR_INVALID),
    "k_param = n + 1": (dict(k_param=258), nat.SCC_ERR_INVALID),
    "k_param = 66": (dict(k_param=66), nat.SCC_ERR_UNSUPPORTED),
    "dims = 16": (dict(dims=16), nat.SCC_ERR_INVALID),
    "prune = 2": (dict(prune=2.0), nat.SCC_ERR_INVALID),
    "resolution = 0": (dict(resolution=0.0), nat.SCC_ERR_INVALID),
    "resolution nan": (dict(resolution=np.nan), nat.SCC_ERR_NONFINITE),
    "nan score": (dict(), nat.SCC_ERR_NONFINITE),
}


@pytest.mark.parametrize("what", list(FUSED_BAD))
def test_fused_refusals(eng, what):
    n = 257
    before = _knn_baseline(eng)
    kw, code = FUSED_BAD[what]
    t = _points(n)["t"]
    if what == "nan score":
        y = np.array(_points(n)["x"])
        y[n // 3, 4] = np.nan
        t = _device_scores(y)
    with pytest.raises(nat.SccError) as e:
        eng.snn_clusters_scores(n, scores_device_ptr=t.data_ptr(), **kw)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


def test_no_kept_scores_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.snn_clusters_scores(65, 20)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


def test_profiled_call_fills_the_three_timer_families():
    n = 1025
    prof = nat.Engine(0, profile=True)
    prof.reset_timers()
    prof.snn_clusters_scores(n, 20, 8, PRUNE, 0.8, _points(n)["t"].data_ptr())
    for family in ("knn_scores", "snn_graph", "modularity_cluster"):
        ms, calls = prof.kernel_time(family)
        assert calls == 1 and ms > 0.0, family
    prof.close()


# -------------------------------------------------------------------- 4. API
def test_api_find_clusters_feeds_recluster():
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    e0 = api._engine(0)
    ds = e0.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = e0.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    ds.close()
    N = d.N
    out = api.find_clusters(d, union, k_param=20, dims=8, resolution=0.8, return_graph=True)
    lab, (indptr, cols, vals) = out["labels"], out["graph"]
    assert lab.shape == (N,) and lab.dtype == np.int32 and out["n_clusters"] == lab.max() + 1 >= 2
    sizes = np.bincount(lab)
    assert np.all(np.diff(sizes) <= 0)  # 0 is the largest
    assert len(indptr) == N + 1 and indptr[-1] == len(cols) == len(vals)
    again = e0.snn_clusters_scores(N, 20, 8, PRUNE, 0.8)  # on the scores that call kept
    _assert_clustering(again, out)
    _assert_clustering(out, sr.modularity_cluster(indptr, cols, vals, 0.8), "api")
    assert api.find_clusters(d, union)["graph"] is None
    with pytest.raises(ValueError):
        api.find_clusters(d, union, k_param=1)
    with pytest.raises(ValueError):
        api.find_clusters(d, union, dims=16)
    res = api.reclusterDEConsensusFast(d, lab, deepSplitValues=(1,), minClusterSize=10)
    assert set(res) == {"deGeneUnion", "cellTree", "dynamicColors"} and len(res["dynamicColors"]["deepsplit: 1"]) == N
