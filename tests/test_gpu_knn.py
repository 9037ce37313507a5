"""GPU: the exact k nearest neighbours of every cell from the PCA scores,
without the N x N matrix (scc_knn_scores; the search the reference README's
umap::umap(d = pca.data) starts with).

The kernel computes each d(i, j) from two score rows with the dist kernel's
arithmetic and keeps, per row, the k smallest keys (distance, index).  Checked:
index equality and distance bit equality with the reference order
(knn_reference) on the engine's own distance of the same scores; the tie rule
on a lattice and on duplicate rows; scipy's pdist as an independent distance
(rtol 1e-9, test_gpu_sil's); `dims` against a zeroed copy; sampled rows at a
size whose matrix is never formed.  Sizes sit on the edges of a 64-lane wave, of
the 128- and 256-row workgroups, of the 128-column LDS tile and of the 16-chunk
cap (16 x 128 columns); k on the edges of the 16-, 32- and 64-slot lists."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import pdist, squareform

import knn_reference as kr
import ward_vector_reference as wv
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth
from test_gpu_hclust_scores import _device_scores

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # test_gpu_sil's
SIZES = [2, 3, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025, 2047, 2048, 2049, 3000]
KS = [1, 2, 15, 16, 17, 32, 33, 63, 64]
CASES = [(n, k) for n in SIZES for k in KS if k <= n - 1]

# Nothing is dropped silently: every size and every k runs, a size above 64
# runs every k, and a smaller one every k it admits.
assert {n for n, _ in CASES} == set(SIZES) and {k for _, k in CASES} == set(KS)
assert all(sum(1 for m, _ in CASES if m == n) == sum(1 for k in KS if k <= n - 1) for n in SIZES)
assert all(sum(1 for m, _ in CASES if m == n) == len(KS) for n in SIZES if n > 64)


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


@pytest.fixture(scope="module")
def cfg_a(eng):
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    return d, ds, union, np.asarray(code, np.int32)


_POINTS = {}


def _points(n):
    if n not in _POINTS:
        x = wv.blobs(n)
        x.setflags(write=False)
        _POINTS[n] = {"x": x, "t": _device_scores(x)}
    return _POINTS[n]


def _ref(p, key, square, k):
    """The reference neighbours of a square matrix at the largest k the tests
    use, computed once per input; a smaller k is its prefix."""
    if key not in p:
        n = square.shape[0]
        idx, dist = kr.knn_from_square(square, min(64, n - 1))
        idx.setflags(write=False)
        dist.setflags(write=False)
        p[key] = (idx, dist)
    return p[key][0][:, :k], p[key][1][:, :k]


def _engine_square(eng, p, n):
    if "engine" not in p:
        m = squareform(eng.distance_scores(p["t"].data_ptr(), n, 0, n))
        m.setflags(write=False)
        p["engine"] = m
    return p["engine"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _assert_same(got, ref, tag):
    (gi, gd), (ri, rd) = got, ref
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == ri.shape and gd.shape == rd.shape
    bad = int(np.sum(gi != ri)) + int(np.sum(_bits(gd) != _bits(rd)))
    print(f"{tag}: n={gi.shape[0]} k={gi.shape[1]} differing entries {bad}")
    assert np.array_equal(gi, ri)
    assert np.array_equal(_bits(gd), _bits(rd))


# ---------------------------------------------- 1. the engine's own distance
@pytest.mark.parametrize("n,k", CASES)
def test_neighbours_equal_reference_on_engine_distance(eng, n, k):
    p = _points(n)
    ref = _ref(p, "ref_engine", _engine_square(eng, p, n), k)
    _assert_same(eng.knn_scores(n, k, 0, p["t"].data_ptr()), ref, "engine")


# --------------------------------------------------------------- 2. ties
@pytest.fixture(scope="module")
def lattice(eng):
    n = 1025
    p = {"x": kr.lattice(n)}
    p["t"] = _device_scores(p["x"])
    _engine_square(eng, p, n)
    return n, p


@pytest.fixture(scope="module")
def shifted(eng):
    n = 1025
    x = wv.blobs(n) + 1e3
    x[5] = x[900]
    x[6] = x[900]
    p = {"x": x, "t": _device_scores(x)}
    sq = _engine_square(eng, p, n)
    assert sq[5, 6] == 0.0 and sq[5, 900] == 0.0 and sq[6, 900] == 0.0
    return n, p


@pytest.mark.parametrize("k", KS)
def test_lattice_ties_resolve_by_index(eng, lattice, k):
    n, p = lattice
    ref = _ref(p, "ref_engine", p["engine"], k)
    idx, dist = eng.knn_scores(n, k, 0, p["t"].data_ptr())
    _assert_same((idx, dist), ref, "lattice")
    same = np.diff(dist, axis=1) == 0
    assert np.all(np.diff(idx, axis=1)[same] > 0)
    if k >= 15:
        assert same.sum() > n * (k - 1) // 2  # the ties are massive: the rule, not the values, decides


@pytest.mark.parametrize("k", KS)
def test_offset_and_duplicate_rows(eng, shifted, k):
    n, p = shifted
    ref = _ref(p, "ref_engine", p["engine"], k)
    idx, dist = eng.knn_scores(n, k, 0, p["t"].data_ptr())
    _assert_same((idx, dist), ref, "offset")
    if k >= 2:  # the three duplicates: each other's first neighbours at exactly 0, in index order
        assert list(idx[5, :2]) == [6, 900] and list(idx[6, :2]) == [5, 900] and list(idx[900, :2]) == [5, 6]
        assert np.all(dist[[5, 6, 900], :2] == 0.0)
    else:
        assert list(idx[[5, 6, 900], 0]) == [6, 5, 5] and np.all(dist[[5, 6, 900], 0] == 0.0)


# ------------------------------------------------ 3. an independent distance
def _check_independent(got, square, k, tag):
    """Distances within RTOL of the reference's, indices equal on every row
    whose first k + 1 reference distances have no relative gap <= RTOL;
    returns the number of rows that condition excludes."""
    idx, dist = got
    n = square.shape[0]
    ri, rd = kr.knn_from_square(square, min(k + 1, n - 1))
    gap = kr.min_relative_gap(rd) if rd.shape[1] > 1 else np.full(n, np.inf)
    keep = gap > RTOL
    err = float(np.max(np.abs(dist - rd[:, :k]) / rd[:, :k]))
    print(f"{tag}: n={n} k={k} worst relative distance error {err:.3g} (rtol {RTOL:g}), smallest relative gap "
          f"{gap.min():.3g}, rows excluded {int((~keep).sum())}")
    np.testing.assert_allclose(dist, rd[:, :k], rtol=RTOL, atol=0)
    assert np.array_equal(idx[keep], ri[keep, :k])
    return int((~keep).sum())


@pytest.mark.parametrize("n,k", [(n, k) for n in (65, 1025, 3000) for k in (15, 64)])
def test_neighbours_match_pdist(eng, n, k):
    p = _points(n)
    if "pdist" not in p:
        p["pdist"] = squareform(pdist(p["x"]))
    excluded = _check_independent(eng.knn_scores(n, k, 0, p["t"].data_ptr()), p["pdist"], k, "pdist")
    assert excluded == 0  # the smallest relative gap on these inputs is 2.1e-8 (n = 3000, k = 64)


# ------------------------------------------------------------------ 4. dims
@pytest.mark.parametrize("dims", [1, 8, 14])
@pytest.mark.parametrize("n,k", [(257, 17), (1025, 15)])
def test_dims_equals_zeroed_copy_and_leading_pdist(eng, dims, n, k):
    p = _points(n)
    z = np.array(p["x"])
    z[:, dims:] = 0.0
    tz = _device_scores(z)
    got = eng.knn_scores(n, k, dims, p["t"].data_ptr())
    zero = eng.knn_scores(n, k, 0, tz.data_ptr())
    _assert_same(got, zero, f"dims={dims}")
    _assert_same(eng.knn_scores(n, k, dims, tz.data_ptr()), zero, f"dims={dims} on the zeroed copy")
    excluded = _check_independent(got, squareform(pdist(p["x"][:, :dims])), k, f"pdist dims={dims}")
    assert excluded <= n // 10  # (1-D points may tie within RTOL; the comparison must not become empty)


# ----------------------------------------------- 5. large n, no matrix at all
def test_sampled_rows_at_50000_cells(eng):
    n, k = 50000, 15
    x = wv.blobs(n)
    t = _device_scores(x)
    idx, dist = eng.knn_scores(n, k, 0, t.data_ptr())
    assert idx.shape == (n, k) and dist.shape == (n, k)
    assert idx.min() >= 0 and idx.max() < n
    assert np.all(idx != np.arange(n)[:, None])
    dd, di = np.diff(dist, axis=1), np.diff(idx, axis=1)
    assert np.all((dd > 0) | ((dd == 0) & (di > 0)))  # strictly ordered by (distance, index)
    rng = np.random.default_rng(50000)
    rows = np.r_[0, n - 1, 1 + rng.choice(n - 2, 254, replace=False)]
    assert len(np.unique(rows)) == 256
    excluded = 0
    worst = 0.0
    for i in rows:  # the difference form
        d = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
        order = np.lexsort((np.arange(n), d))
        order = order[order != i][:k + 1]
        rd = d[order]
        worst = max(worst, float(np.max(np.abs(dist[i] - rd[:k]) / rd[:k])))
        np.testing.assert_allclose(dist[i], rd[:k], rtol=RTOL, atol=0)
        if np.min(np.diff(rd) / rd[1:]) > RTOL:
            assert np.array_equal(idx[i], order[:k])
        else:
            excluded += 1
    print(f"n={n}: {len(rows)} rows, worst relative distance error {worst:.3g}, rows excluded {excluded}")
    assert excluded <= 2  # 256 x 15 gaps between distances of order 1: a gap <= 1e-9 has odds around 1e-5


# ------------------------------------------------------------ 6. kept scores
def test_kept_scores_answer_the_null_call(eng, cfg_a):
    d, ds, union, code = cfg_a
    eng.pca_scores(ds, union)
    kept = eng.knn_scores(d.N, 15, 8)
    again = _device_scores(eng.last_pca_scores(d.N))
    _assert_same(kept, eng.knn_scores(d.N, 15, 8, again.data_ptr()), "kept")
    w0, c0 = eng.silhouette_scores(d.N, code)
    with pytest.raises(nat.SccError) as e:  # a wrong n
        eng.knn_scores(d.N - 1, 15, 8)
    assert e.value.code == nat.SCC_ERR_INVALID
    w1, c1 = eng.silhouette_scores(d.N, code)
    assert np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(c0), _bits(c1))
    _assert_same(eng.knn_scores(d.N, 15, 8), kept, "kept after a refusal")


def test_no_kept_scores_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.knn_scores(65, 15)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


# ------------------------------------------------------------- 7. refusals
BAD = {  # (k, dims, a value planted in the scores, the code); k = None: n
    "k = 0": (0, 0, None, nat.SCC_ERR_INVALID), "k = n": (None, 0, None, nat.SCC_ERR_INVALID),
    "k = 65": (65, 0, None, nat.SCC_ERR_UNSUPPORTED), "dims = 16": (15, 16, None, nat.SCC_ERR_INVALID),
    "dims = -1": (15, -1, None, nat.SCC_ERR_INVALID), "nan": (15, 0, np.nan, nat.SCC_ERR_NONFINITE),
    "inf": (15, 0, np.inf, nat.SCC_ERR_NONFINITE), "-inf": (15, 8, -np.inf, nat.SCC_ERR_NONFINITE),
}


@pytest.mark.parametrize("what", list(BAD))
def test_refusals_leave_the_engine_as_it_was(eng, what):
    n = 257
    p = _points(n)
    g = (np.arange(n) % 5).astype(np.int32)
    w0, c0 = eng.silhouette_scores(n, g, p["t"].data_ptr())
    k, dims, v, code = BAD[what]
    t = p["t"]
    if v is not None:
        y = np.array(p["x"])
        y[n // 3, 4] = v
        t = _device_scores(y)
    with pytest.raises(nat.SccError) as e:
        eng.knn_scores(n, n if k is None else k, dims, t.data_ptr())
    assert e.value.code == code
    w1, c1 = eng.silhouette_scores(n, g, p["t"].data_ptr())
    assert np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(c0), _bits(c1))


# ---------------------------------------------------------- 8. determinism
def test_two_calls_same_bits_and_scores_untouched(eng):
    n = 3000
    t = _device_scores(_points(n)["x"])
    before = t.clone()
    a = eng.knn_scores(n, 33, 8, t.data_ptr())
    b = eng.knn_scores(n, 33, 8, t.data_ptr())
    torch.cuda.synchronize()
    _assert_same(a, b, "second call")
    assert torch.equal(t, before)


@pytest.mark.parametrize("k", [15, 64])
def test_row_blocks_per_launch_change_no_bit(eng, monkeypatch, k):
    n = 1025
    p = _points(n)
    whole = eng.knn_scores(n, k, 0, p["t"].data_ptr())
    monkeypatch.setenv("SCC_KNN_ROWS_PER_LAUNCH", "256")  # five launches, another chunk count
    split = eng.knn_scores(n, k, 0, p["t"].data_ptr())
    monkeypatch.delenv("SCC_KNN_ROWS_PER_LAUNCH")
    _assert_same(split, whole, "row blocks")


# --------------------------------------------------------------- 9. timers
def test_profiled_call_is_timed_as_knn_scores():
    n = 1025
    prof = nat.Engine(0, profile=True)
    prof.reset_timers()
    prof.knn_scores(n, 15, 8, _points(n)["t"].data_ptr())
    ms, calls = prof.kernel_time("knn_scores")
    assert calls == 1 and ms > 0.0
    prof.close()


# ------------------------------------------------------------------ 10. API
def test_api_nearest_neighbors(cfg_a):
    d, _, union, _ = cfg_a
    N, k = d.N, 16
    nn = api.nearest_neighbors(d, union, k=k, dims=8)
    idx, dist = nn["indexes"], nn["distances"]
    assert idx.shape == (N, k) and dist.shape == (N, k) and nn["scores"].shape == (N, 15)
    assert idx.dtype == np.int32 and np.array_equal(idx[:, 0], np.arange(N)) and np.all(dist[:, 0] == 0.0)
    ei, ed = api._engine(0).knn_scores(N, k - 1, 8)  # the scores that call kept
    _assert_same((idx[:, 1:], dist[:, 1:]), (ei, ed), "api dims=8")
    others = api.nearest_neighbors(d, union, k=k - 1, dims=8, include_self=False)
    _assert_same((others["indexes"], others["distances"]), (ei, ed), "api include_self=False")
    assert np.array_equal(_bits(others["scores"]), _bits(nn["scores"]))
    with pytest.raises(ValueError):
        api.nearest_neighbors(d, union, k=1)
    with pytest.raises(ValueError):
        api.nearest_neighbors(d, union, k=5, dims=16)
