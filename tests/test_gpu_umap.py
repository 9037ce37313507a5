"""GPU: UMAP of the cells on the engine (scc_umap_graph, scc_umap_layout,
scc_umap_scores; api.umap), against the NumPy restatement in umap_reference.

Graph.  rho bit for bit; every row's sigma satisfies the bisection's defining
property (the host-evaluated psum at the device's sigma within 1e-5 + 1e-12 of
log2(n_neighbors): at most 64 terms <= 1, each with a few ulp of exp) or equals
its floor (rtol 1e-12), and the rows that end at the floor are the reference's:
none on the blob inputs, except at n_neighbors = 3, where psum = 1 + exp(-(d2 -
d1) / mid) and a row whose two distances nearly tie has a sigma below a
thousandth of their mean (test_umap_reference counts them); sigma bit-equal to
the reference's in all but 0.1 % of rows (a compare against the target flips
only where psum lies within rounding of a threshold); directed weights within
rtol 1e-12 of exp(-(d - rho) / sigma) from the device's own rho and sigma (the
argument's rounding contributes at most 745 * 2^-53); indptr and cols exactly
the reference's, vals within rtol 1e-14.

Layout.  The device and the float64 reference run the same steps on the same
graph; they differ in pow's last bits and in the shape of a vertex's sum.  The
bound is measured, not fixed: 100 times the largest deviation between the
float64 reference and the same reference in np.longdouble on that graph, init
and epoch count, and no less than 1e-12 of the layout's extent
(profiles/umap_layout.md lists the values this gave).  The 200-epoch run is
compared by quality: trustworthiness and 2-D label purity no worse than the
reference's on the same graph and seed, minus the reference's spread over five
seeds (0.0014 and 0, measured on the host, same file).

Agreement with the umap, uwot or umap-learn packages is not tested: none is
installed."""
import numpy as np
import pytest
import torch

import umap_reference as ur
import ward_vector_reference as wv
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth
from test_gpu_hclust_scores import _device_scores

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 16, 17, 63, 64, 65, 257, 1025, 3000]
NNS = [2, 3, 15, 16, 17, 33, 65]
CASES = [(n, nn) for n in SIZES for nn in NNS if nn <= n]
assert {n for n, _ in CASES} == set(SIZES) and {nn for _, nn in CASES} == set(NNS)
assert all(sum(1 for m, _ in CASES if m == n) == len(NNS) for n in SIZES if n >= 65)

TRUST_MARGIN = 0.0014  # the reference's spread over seeds 0..4 at n = 3000 (0.96207 .. 0.96339)
PURITY_MARGIN = 0.0    # (its purity is 1.0 at every seed)


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


_POINTS = {}


def _points(n):
    if n not in _POINTS:
        x = wv.blobs(n)
        x.setflags(write=False)
        _POINTS[n] = {"x": x, "t": _device_scores(x)}
    return _POINTS[n]


_TABLES = {}


def _table(eng, n, nn):
    """The engine's own k-NN table of the blob scores, and the reference graph of it, once."""
    if (n, nn) not in _TABLES:
        idx, dist = eng.knn_scores(n, nn - 1, 0, _points(n)["t"].data_ptr())
        ref = ur.fuzzy_graph(idx, dist)
        for a in (idx, dist) + ref:
            a.setflags(write=False)
        _TABLES[(n, nn)] = (idx, dist, ref)
    return _TABLES[(n, nn)]


def _check_rows(dist, nn, rho, sigma, tag):
    """rho, and the defining property of sigma; returns the rows that sit at the floor without reaching the target."""
    k = dist.shape[1]
    pos = np.where(dist > 0.0, dist, np.inf).min(axis=1)
    assert np.array_equal(_bits(rho), _bits(np.where(np.isfinite(pos), pos, 0.0)))
    ps = ur.psum_at(dist, rho, sigma)
    off = np.abs(ps - np.log2(float(nn)))
    hit = off <= 1e-5 + 1e-12
    rs = np.zeros(len(dist))
    for j in range(k):
        rs = rs + dist[:, j]
    floor = ur.FLOOR * np.where(rho > 0.0, rs / float(k), ur.fixed_total(rs) / (float(len(dist)) * float(k)))
    floored = np.abs(sigma - floor) <= 1e-12 * floor
    print(f"{tag}: worst |psum - target| among the rows at the target {off[hit].max() if hit.any() else 0.0:.3g}, "
          f"rows at the floor only {int((~hit).sum())}")
    assert np.all(hit | floored)
    return np.nonzero(~hit)[0]


# ------------------------------------------------------------------ 1. graph
@pytest.mark.parametrize("n,nn", CASES)
def test_graph_of_the_engine_table(eng, n, nn):
    idx, dist, (r_indptr, r_cols, r_vals, r_rho, r_sigma) = _table(eng, n, nn)
    indptr, cols, vals, rho, sigma, w = eng.umap_graph(idx, dist, return_rho_sigma=True)
    ref_floored = _check_rows(dist, nn, r_rho, r_sigma, "reference")
    if nn != 3:
        assert len(ref_floored) == 0  # checked first: the blob inputs do not reach the floor
    dev_floored = _check_rows(dist, nn, rho, sigma, "device")
    assert np.array_equal(dev_floored, ref_floored)
    differ = int(np.sum(_bits(sigma) != _bits(r_sigma)))
    print(f"n={n} n_neighbors={nn}: sigma differs from the reference in {differ} rows, nnz {indptr[-1]}, "
          f"longest row {int(np.diff(indptr).max())}")
    assert differ <= n / 1000.0
    np.testing.assert_allclose(w, ur.directed_weights(dist, rho, sigma), rtol=1e-12, atol=0)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    assert np.array_equal(indptr, r_indptr) and np.array_equal(cols, r_cols)
    np.testing.assert_allclose(vals, r_vals, rtol=1e-14, atol=0)


def _graph_equals_reference(eng, idx, dist, mix=1.0):
    got = eng.umap_graph(idx, dist, set_op_mix_ratio=mix, return_rho_sigma=True)
    ref = ur.fuzzy_graph(idx, dist, mix)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-14, atol=0)
    assert np.array_equal(_bits(got[3]), _bits(ref[3]))
    np.testing.assert_allclose(got[4], ref[4], rtol=1e-12, atol=0)
    return got, ref


def test_hub_row_holds_every_other_vertex(eng):
    idx, dist = ur.hub_table(300, 4)
    (indptr, cols, vals, rho, sigma, w), _ = _graph_equals_reference(eng, idx, dist)
    assert indptr[1] - indptr[0] == 299 and np.array_equal(cols[:299], np.arange(1, 300))
    assert all(np.all(np.diff(cols[indptr[r]:indptr[r + 1]]) > 0) for r in range(300))


def test_duplicate_points_have_weight_one(eng):
    n, k = 40, 5
    x = np.array(wv.blobs(n))
    x[5] = x[30]
    x[6] = x[30]
    idx, dist = eng.knn_scores(n, k, 0, _device_scores(x).data_ptr())
    assert np.all(dist[[5, 6, 30], :2] == 0.0) and np.all(dist[[5, 6, 30], 2] > 0.0)
    (indptr, cols, vals, rho, sigma, w), _ = _graph_equals_reference(eng, idx, dist)
    assert np.array_equal(rho[[5, 6, 30]], dist[[5, 6, 30], 2])  # the first positive distance
    assert np.all(w[[5, 6, 30], :3] == 1.0)
    for a, b in ((5, 6), (5, 30), (6, 30)):
        row = slice(indptr[a], indptr[a + 1])
        assert vals[row][cols[row] == b] == 1.0


def test_rows_of_zeros_and_of_equal_distances_take_the_floor(eng):
    idx, dist = (np.array(a) for a in ur.hub_table(50, 4))
    dist[7] = 0.0   # no positive distance: rho 0, the floor from the global mean
    dist[9] = 2.5   # all equal: psum stays k, the bisection runs out, the floor from the row
    (indptr, cols, vals, rho, sigma, w), ref = _graph_equals_reference(eng, idx, dist)
    rs = dist.sum(axis=1)
    assert rho[7] == 0.0 and rho[9] == 2.5
    np.testing.assert_allclose(sigma[7], ur.FLOOR * ur.fixed_total(rs) / dist.size, rtol=1e-12)
    np.testing.assert_allclose(sigma[9], ur.FLOOR * 2.5, rtol=1e-12)
    assert np.all(w[7] == 1.0) and np.all(w[9] == 1.0)
    _check_rows(dist, 5, rho, sigma, "hand-made")


@pytest.mark.parametrize("mix", [0.0, 0.5])
@pytest.mark.parametrize("n,nn", [(65, 15), (1025, 16)])
def test_set_op_mix_ratio(eng, n, nn, mix):
    idx, dist, _ = _table(eng, n, nn)
    (indptr, cols, vals, _, _, _), _ = _graph_equals_reference(eng, idx, dist, mix)
    union = eng.umap_graph(idx, dist)
    if mix == 0.0:  # the intersection: fewer entries, on both sides of the diagonal
        assert 0 < indptr[-1] < union[0][-1]
        pairs = set(zip(np.repeat(np.arange(n), np.diff(indptr)).tolist(), cols.tolist()))
        assert all((c, r) in pairs for r, c in pairs)
    else:
        assert np.array_equal(indptr, union[0]) and np.array_equal(cols, union[1])


def test_self_entries_are_dropped(eng):
    idx, dist = (np.array(a) for a in ur.hub_table(50, 4))
    idx[11, 2] = 11
    (indptr, cols, _, _, _, _), _ = _graph_equals_reference(eng, idx, dist)
    assert 11 not in cols[indptr[11]:indptr[12]]


def _bad_tables():
    idx, dist = ur.hub_table(300, 4)
    out = {}

    def case(name, code, i=None, d=None, **kw):
        out[name] = (np.array(idx) if i is None else i, np.array(dist) if d is None else d, kw, code)
    i = np.array(idx); i[3, 1] = -1
    case("index -1", nat.SCC_ERR_INVALID, i=i)
    i = np.array(idx); i[3, 1] = 300
    case("index n", nat.SCC_ERR_INVALID, i=i)
    i = np.array(idx); i[3, 1] = i[3, 2]
    case("index twice", nat.SCC_ERR_INVALID, i=i)
    d = np.array(dist); d[8, 0] = -1.0
    case("negative distance", nat.SCC_ERR_INVALID, d=d)
    d = np.array(dist); d[8, 1], d[8, 2] = d[8, 2], d[8, 1]
    case("descending distance", nat.SCC_ERR_INVALID, d=d)
    for name, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        d = np.array(dist); d[299, 3] = v
        case(name, nat.SCC_ERR_NONFINITE, d=d)
    case("k = 0", nat.SCC_ERR_INVALID, i=idx[:, :0], d=dist[:, :0])
    case("k = n", nat.SCC_ERR_INVALID, i=np.zeros((5, 5), np.int32), d=np.ones((5, 5)))
    case("k = 65", nat.SCC_ERR_UNSUPPORTED, i=np.tile(np.arange(1, 66, dtype=np.int32), (300, 1)),
         d=np.tile(np.arange(1.0, 66.0), (300, 1)))
    case("local_connectivity = 2", nat.SCC_ERR_UNSUPPORTED, local_connectivity=2.0)
    case("bandwidth = 2", nat.SCC_ERR_UNSUPPORTED, bandwidth=2.0)
    case("mix = 1.5", nat.SCC_ERR_INVALID, set_op_mix_ratio=1.5)
    return out


BAD_TABLES = _bad_tables()


def _knn_baseline(eng):
    p = _points(257)
    return eng.knn_scores(257, 15, 8, p["t"].data_ptr())


def _assert_knn_unchanged(eng, before):
    idx, dist = _knn_baseline(eng)
    assert np.array_equal(idx, before[0]) and np.array_equal(_bits(dist), _bits(before[1]))


@pytest.mark.parametrize("what", list(BAD_TABLES))
def test_graph_refusals(eng, what):
    before = _knn_baseline(eng)
    idx, dist, kw, code = BAD_TABLES[what]
    with pytest.raises(nat.SccError) as e:
        eng.umap_graph(idx, dist, **kw)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


# ----------------------------------------------------------------- 2. layout
def _layout_inputs(eng, which):
    if which == "hub":
        idx, dist = ur.hub_table(300, 4)
        init = np.random.default_rng(300).normal(scale=5.0, size=(300, 2))
    else:
        idx, dist, _ = _table(eng, which, 15)
        init = ur.pca_init(_points(which)["x"])
    return eng.umap_graph(idx, dist), init


@pytest.mark.parametrize("epochs", [1, 2, 10])
@pytest.mark.parametrize("which", [17, 65, 1025, "hub"])
def test_layout_follows_the_reference(eng, which, epochs):
    (indptr, cols, vals), init = _layout_inputs(eng, which)
    y = eng.umap_layout(indptr, cols, vals, init, n_epochs=epochs, seed=7)
    r64 = ur.layout(indptr, cols, vals, init, n_epochs=epochs, seed=7)
    rld = ur.layout(indptr, cols, vals, init, n_epochs=epochs, seed=7, dtype=np.longdouble)
    rounding = float(np.max(np.abs(r64.astype(np.longdouble) - rld)))
    extent = float(np.max(np.ptp(r64, axis=0)))
    bound = max(100.0 * rounding, 1e-12 * extent)
    err = float(np.max(np.abs(y - r64)))
    print(f"{which} epochs={epochs}: device - reference {err:.3g}, float64 - longdouble {rounding:.3g}, "
          f"extent {extent:.3g}, bound {bound:.3g}")
    assert y.shape == init.shape and y.dtype == np.float64
    assert err <= bound
    assert not np.array_equal(y, init)


def test_layout_is_deterministic_seeded_and_leaves_its_inputs(eng):
    (indptr, cols, vals), init = _layout_inputs(eng, 1025)
    keep = [a.copy() for a in (indptr, cols, vals, init)]
    a = eng.umap_layout(indptr, cols, vals, init, n_epochs=30, seed=5)
    b = eng.umap_layout(indptr, cols, vals, init, n_epochs=30, seed=5)
    c = eng.umap_layout(indptr, cols, vals, init, n_epochs=30, seed=6)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(a, c)
    assert all(np.array_equal(x, y) for x, y in zip(keep, (indptr, cols, vals, init)))


def test_vertices_without_an_active_edge_stay(eng):
    (indptr, cols, vals), init = _layout_inputs(eng, 65)
    indptr = np.concatenate([indptr, [indptr[-1]] * 3])  # three vertices without edges
    init = np.concatenate([init, [[1.0, 2.0], [-3.0, 0.5], [0.0, 0.0]]])
    y = eng.umap_layout(indptr, cols, vals, init, n_epochs=10)
    assert np.array_equal(_bits(y[65:]), _bits(init[65:])) and not np.array_equal(y[:65], init[:65])
    # a graph whose only edge is too light ever to act (w < w_max / n_epochs), and one without entries
    ip = np.array([0, 1, 2, 3, 4], np.int64)
    cl = np.array([1, 0, 3, 2], np.int32)
    vl = np.array([1.0, 1.0, 0.01, 0.01])
    i4 = np.array([[0.0, 0.0], [1.0, 0.0], [5.0, 5.0], [6.0, 5.0]])
    y = eng.umap_layout(ip, cl, vl, i4, n_epochs=10)
    assert np.array_equal(y[2:], i4[2:]) and not np.array_equal(y[:2], i4[:2])
    # two vertices, at most 10 attractions and 50 draws each, every move at most 4 with a few ulp of error
    np.testing.assert_allclose(y, ur.layout(ip, cl, vl, i4, n_epochs=10), rtol=0, atol=1e-11)
    none = eng.umap_layout(np.zeros(5, np.int64), cl[:0], vl[:0], i4, n_epochs=3)
    assert np.array_equal(none, i4)


@pytest.fixture(scope="module")
def blob3000(eng):
    n = 3000
    x, lab = ur.blobs(n, dim=8, n_blobs=6, seed=3000)
    t = _device_scores(x)
    idx, dist = eng.knn_scores(n, 14, 0, t.data_ptr())
    return x, lab, t, eng.umap_graph(idx, dist), ur.pca_init(x)


def test_200_epochs_at_3000_cells_match_the_reference_quality(eng, blob3000):
    from sklearn.manifold import trustworthiness
    x, lab, _, (indptr, cols, vals), init = blob3000
    assert ur.label_purity(x, lab) == 1.0
    y = eng.umap_layout(indptr, cols, vals, init, n_epochs=200, seed=0)
    assert np.all(np.isfinite(y))
    ref = ur.layout(indptr, cols, vals, init, n_epochs=200, seed=0)
    t_dev, t_ref = trustworthiness(x, y, n_neighbors=15), trustworthiness(x, ref, n_neighbors=15)
    p_dev, p_ref = ur.label_purity(y, lab), ur.label_purity(ref, lab)
    print(f"trustworthiness device {t_dev:.5f} reference {t_ref:.5f} (init {trustworthiness(x, init, n_neighbors=15):.5f}), "
          f"purity device {p_dev:.5f} reference {p_ref:.5f}, extent {np.ptp(y, axis=0)}")
    assert t_dev >= t_ref - TRUST_MARGIN
    assert p_dev >= p_ref - PURITY_MARGIN


def _bad_layouts():
    ip = np.array([0, 1, 2, 3, 4], np.int64)
    cl = np.array([1, 0, 3, 2], np.int32)
    vl = np.array([1.0, 1.0, 0.5, 0.5])
    i4 = np.array([[0.0, 0.0], [1.0, 0.0], [5.0, 5.0], [6.0, 5.0]])
    out = {}

    def case(name, code, ip=ip, cl=cl, vl=vl, i4=i4, **kw):
        out[name] = (ip, cl, vl, i4, kw, code)
    for name, v in (("nan init", np.nan), ("inf init", np.inf)):
        bad = i4.copy(); bad[2, 1] = v
        case(name, nat.SCC_ERR_NONFINITE, i4=bad)
    for name, v in (("nan weight", np.nan), ("inf weight", np.inf)):
        bad = vl.copy(); bad[3] = v
        case(name, nat.SCC_ERR_NONFINITE, vl=bad)
    case("negative weight", nat.SCC_ERR_INVALID, vl=np.array([1.0, 1.0, -0.5, 0.5]))
    case("indptr descending", nat.SCC_ERR_INVALID, ip=np.array([0, 2, 1, 3, 4], np.int64))
    case("indptr from 1", nat.SCC_ERR_INVALID, ip=np.array([1, 1, 2, 3, 4], np.int64))
    case("column n", nat.SCC_ERR_INVALID, cl=np.array([1, 0, 4, 2], np.int32))
    case("column -1", nat.SCC_ERR_INVALID, cl=np.array([1, 0, -1, 2], np.int32))
    case("n_epochs = 0", nat.SCC_ERR_INVALID, n_epochs=0)
    case("negative a", nat.SCC_ERR_INVALID, a=-1.0, b=1.0)
    case("negative b", nat.SCC_ERR_INVALID, a=1.0, b=-1.0)
    case("negative_sample_rate = -1", nat.SCC_ERR_INVALID, negative_sample_rate=-1)
    return out


BAD_LAYOUTS = _bad_layouts()


@pytest.mark.parametrize("what", list(BAD_LAYOUTS))
def test_layout_refusals(eng, what):
    before = _knn_baseline(eng)
    ip, cl, vl, i4, kw, code = BAD_LAYOUTS[what]
    with pytest.raises(nat.SccError) as e:
        eng.umap_layout(ip, cl, vl, i4, **kw)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


# ------------------------------------------------------- 3. the fused call
def _default_init(x16):
    y = x16[:, :2]
    return y * (10.0 / np.abs(y).max())


@pytest.mark.parametrize("n,nn,dims,epochs", [(65, 15, 0, 11), (1025, 15, 8, 20), (3000, 33, 0, 4)])
def test_fused_call_equals_the_three_calls(eng, n, nn, dims, epochs):
    p = _points(n)
    x16 = p["t"].cpu().numpy()
    y, g = eng.umap_scores(n, nn, dims, p["t"].data_ptr(), n_epochs=epochs, seed=9, return_graph=True)
    idx, dist = eng.knn_scores(n, nn - 1, dims, p["t"].data_ptr())
    indptr, cols, vals = eng.umap_graph(idx, dist)
    assert np.array_equal(g[0], indptr) and np.array_equal(g[1], cols) and np.array_equal(_bits(g[2]), _bits(vals))
    init = _default_init(x16)  # the default initialisation, as specified
    assert abs(np.abs(init).max() - 10.0) <= 1e-14
    sep = eng.umap_layout(indptr, cols, vals, init, n_epochs=epochs, seed=9)
    assert np.array_equal(_bits(y), _bits(sep))
    alone = eng.umap_scores(n, nn, dims, p["t"].data_ptr(), n_epochs=epochs, seed=9)
    assert np.array_equal(_bits(alone), _bits(y))
    mine = np.random.default_rng(n).normal(size=(n, 2))
    given = eng.umap_scores(n, nn, dims, p["t"].data_ptr(), init=mine, n_epochs=epochs, seed=9)
    assert np.array_equal(_bits(given), _bits(eng.umap_layout(indptr, cols, vals, mine, n_epochs=epochs, seed=9)))


def test_fused_dims_equals_a_zeroed_copy(eng):
    n = 1025
    p = _points(n)
    z = np.array(p["x"])
    z[:, 8:] = 0.0
    tz = _device_scores(z)
    before = p["t"].clone()
    a = eng.umap_scores(n, 15, 8, p["t"].data_ptr(), n_epochs=12, seed=3)
    b = eng.umap_scores(n, 15, 0, tz.data_ptr(), n_epochs=12, seed=3)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a), _bits(b))
    assert torch.equal(p["t"], before)


FUSED_BAD = {
    "n_neighbors = 1": (dict(n_neighbors=1), nat.SCC_ERR_INVALID),
    "n_neighbors = n + 1": (dict(n_neighbors=258), nat.SCC_ERR_INVALID),
    "n_neighbors = 66": (dict(n_neighbors=66), nat.SCC_ERR_UNSUPPORTED),
    "dims = 16": (dict(dims=16), nat.SCC_ERR_INVALID),
    "n_epochs = 0": (dict(n_epochs=0), nat.SCC_ERR_INVALID),
    "local_connectivity = 2": (dict(local_connectivity=2.0), nat.SCC_ERR_UNSUPPORTED),
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
        eng.umap_scores(n, scores_device_ptr=t.data_ptr(), **kw)
    assert e.value.code == code
    _assert_knn_unchanged(eng, before)


def test_no_kept_scores_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.umap_scores(65, 15)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


def test_profiled_call_fills_the_three_timer_families():
    n = 1025
    prof = nat.Engine(0, profile=True)
    prof.reset_timers()
    prof.umap_scores(n, 15, 8, _points(n)["t"].data_ptr(), n_epochs=20)
    for family in ("knn_scores", "umap_graph", "umap_layout"):
        ms, calls = prof.kernel_time(family)
        assert calls == 1 and ms > 0.0, family
    prof.close()


# -------------------------------------------------------------------- 4. API
def test_api_umap():
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    e0 = api._engine(0)
    ds = e0.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = e0.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    ds.close()
    N = d.N
    out = api.umap(d, union, n_neighbors=15, dims=8, n_epochs=50, seed=4, return_graph=True)
    y, (indptr, cols, vals) = out["layout"], out["graph"]
    assert y.shape == (N, 2) and y.dtype == np.float64 and np.all(np.isfinite(y))
    assert len(indptr) == N + 1 and indptr[-1] == len(cols) == len(vals) and 14 * N <= len(cols) <= 28 * N
    a, b = ur.find_ab_params(1.0, 0.1)  # the recipe api.umap fits with
    assert abs(a - nat.UMAP_A) <= 1e-6 * a and abs(b - nat.UMAP_B) <= 1e-6 * b
    again = e0.umap_scores(N, 15, 8, n_epochs=50, seed=4, a=a, b=b)  # on the scores that call kept
    assert np.array_equal(_bits(y), _bits(again))
    assert api.umap(d, union, n_epochs=5)["graph"] is None
    mine = np.random.default_rng(1).normal(size=(N, 2))
    other = api.umap(d, union, n_epochs=5, init=mine)["layout"]
    assert other.shape == (N, 2) and not np.array_equal(other, mine)
    with pytest.raises(ValueError):
        api.umap(d, union, n_neighbors=1)
    with pytest.raises(ValueError):
        api.umap(d, union, dims=16)
    with pytest.raises(ValueError):
        api.umap(d, union, min_dist=2.0, spread=1.0)
