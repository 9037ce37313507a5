"""GPU: silhouette widths from the PCA scores, without the N x N matrix
(scc_silhouette_scores; reference line R/reclusterDEConsensusFast.R:433,
SI = mean(summary(cluster::silhouette(groups, dmatrix = as.matrix(d)))$clus.avg.widths)
with d = dist(scores)).

The kernel computes each d(i, j) from two score rows with the dist kernel's
arithmetic where scc_silhouette loads it, and sums in the same order, so three
things are checked: the widths against sklearn's silhouette_samples on the
engine's own distance of the same scores and on scipy's pdist (the tolerances
of test_gpu_sil: rtol 1e-9, atol 1e-12), bit equality with scc_silhouette on
the kept distance, and, at a size whose matrix is never formed, sampled rows
against a numpy restatement of cluster's rule.  Sizes sit on the edges of a
16-row wave, a 64-row workgroup, a column chunk that is no multiple of 16 and
the 256-column LDS tile; group counts on the edges of a 16-cluster tile and of
the 64-cluster pass."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import pdist, squareform
from sklearn.metrics import silhouette_samples

import ward_vector_reference as wv
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth
from test_gpu_hclust_scores import _device_scores

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12  # test_gpu_sil's
SIZES = [3, 15, 16, 17, 63, 64, 65, 1025, 3000]
KINDS = ["k2", "k16", "k17", "k64", "k65", "ids", "singletons", "001"]


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


def _groups(kind, n):
    """The labelling `kind` for n cells, or None where it has no 2 <= k < n form."""
    rng = np.random.default_rng(7919 * n + KINDS.index(kind))
    if kind == "001":
        return np.array([0, 0, 1], np.int32) if n == 3 else None
    if kind == "singletons":  # three singletons plus 4 groups
        if n < 15:
            return None
        return np.r_[np.arange(3) + 50, rng.permutation(np.arange(n - 3) % 4)].astype(np.int32)
    if kind == "ids":  # ids in -3..96, as many of them as n allows
        k = min(100, n - 1)
        ids = np.sort(rng.choice(np.arange(-3, 97), k, replace=False))
        return ids[rng.permutation(np.arange(n) % k)].astype(np.int32)
    k = int(kind[1:])
    if not 2 <= k < n:
        return None
    return rng.permutation(np.arange(n) % k).astype(np.int32)  # exactly k groups


CASES = [(n, kind) for n in SIZES for kind in KINDS if _groups(kind, n) is not None]


# Nothing is dropped silently: each size runs at least two labellings, each
# labelling runs at some size, the large sizes run all but [0, 0, 1], and
# every case has 2 <= k < n.
assert {n for n, _ in CASES} == set(SIZES) and {kind for _, kind in CASES} == set(KINDS)
assert all(sum(1 for m, _ in CASES if m == n) >= 2 for n in SIZES)
assert all(sum(1 for m, _ in CASES if m == n) == len(KINDS) - 1 for n in (1025, 3000))
assert all(2 <= len(np.unique(_groups(kind, n))) < n for n, kind in CASES)


_POINTS = {}


def _points(n):
    """Blob points, their device scores, and both square distance matrices
    (the engine's own dist of the scores; scipy's pdist), computed once."""
    if n not in _POINTS:
        x = wv.blobs(n)
        x.setflags(write=False)
        _POINTS[n] = {"x": x, "t": _device_scores(x)}
    return _POINTS[n]


def _square(eng, n, which):
    p = _points(n)
    if which not in p:
        v = eng.distance_scores(p["t"].data_ptr(), n, 0, n) if which == "engine" else pdist(p["x"])
        m = squareform(v)
        m.setflags(write=False)
        p[which] = m
    return p[which]


def _ref(square, groups):
    w = silhouette_samples(square, groups, metric="precomputed")
    return w, np.array([w[groups == k].mean() for k in np.unique(groups)])


def _check(eng, n, t, square, groups, tag):
    w, ca = eng.silhouette_scores(n, groups, t.data_ptr())
    rw, rca = _ref(square, groups)
    err = float(np.max(np.abs(w - rw) - RTOL * np.abs(rw)))
    print(f"{tag}: n={n} k={len(ca)} worst |w - ref| - rtol |ref| = {err:.3g} (atol {ATOL:g})")
    np.testing.assert_allclose(w, rw, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(ca, rca, rtol=RTOL, atol=ATOL)
    cnt = {k: c for k, c in zip(*np.unique(groups, return_counts=True))}
    single = np.array([cnt[g] == 1 for g in groups])
    assert np.all(w[single] == 0.0)
    return w, ca


# ---------------------------------------------- 1. the engine's own distance
@pytest.mark.parametrize("n,kind", CASES)
def test_widths_match_sklearn_on_engine_distance(eng, n, kind):
    g = _groups(kind, n)
    w, _ = _check(eng, n, _points(n)["t"], _square(eng, n, "engine"), g, kind)
    if kind == "singletons":
        assert (w[:3] == 0.0).all()


# ------------------------------------------------ 2. an independent distance
@pytest.mark.parametrize("n,kind", [c for c in CASES if c[0] in (65, 1025, 3000)])
def test_widths_match_sklearn_on_pdist(eng, n, kind):
    _check(eng, n, _points(n)["t"], _square(eng, n, "pdist"), _groups(kind, n), "pdist " + kind)


# ------------------------------------- 3. bit for bit with the distance route
def test_bits_equal_the_distance_route(eng, cfg_a):
    d, ds, union, code = cfg_a
    eng.distance(ds, union, device_out_ptr=0)  # keeps the f64 distance and the scores it was formed from
    rng = np.random.default_rng(3)
    for g in (code, rng.integers(-3, 97, d.N).astype(np.int32)):
        wd, cd = eng.silhouette(d.N, g)
        ws, cs = eng.silhouette_scores(d.N, g)
        assert np.array_equal(ws, wd)
        assert np.array_equal(cs, cd)


# --------------------------------------------- 4. cancellation and duplicates
@pytest.fixture(scope="module")
def shifted(eng):
    n = 1025
    x = wv.blobs(n) + 1e3
    x[5] = x[900]
    x[6] = x[900]
    t = _device_scores(x)
    sq = squareform(eng.distance_scores(t.data_ptr(), n, 0, n))
    assert sq[5, 6] == 0.0 and sq[5, 900] == 0.0 and sq[6, 900] == 0.0
    return n, t, sq


@pytest.mark.parametrize("kind", ["k2", "k17", "k65", "singletons"])
def test_offset_and_duplicate_rows(eng, shifted, kind):
    n, t, sq = shifted
    _check(eng, n, t, sq, _groups(kind, n), "offset " + kind)


def test_duplicates_alone_in_a_group_have_width_one(eng, shifted):
    n, t, sq = shifted
    g = (np.arange(n) % 4).astype(np.int32)
    g[[5, 6, 900]] = 9
    w, _ = _check(eng, n, t, sq, g, "duplicates")
    assert (w[[5, 6, 900]] == 1.0).all()  # a = 0, b > 0: 1 - 0 / b


# ----------------------------------------------- 5. large n, no matrix at all
def test_sampled_rows_at_50000_cells(eng):
    n, k = 50000, 40
    x = wv.blobs(n)
    t = _device_scores(x)
    rng = np.random.default_rng(50000)
    g = rng.integers(0, k, n).astype(np.int32)
    cnt = np.bincount(g, minlength=k)
    assert cnt.min() > 1
    w, ca = eng.silhouette_scores(n, g, t.data_ptr())
    rows = np.r_[0, n - 1, 1 + rng.choice(n - 2, 254, replace=False)]  # 256 distinct rows
    assert len(np.unique(rows)) == 256
    ref = np.empty(len(rows))
    for q, i in enumerate(rows):  # the difference form, then cluster's sildist rule
        dist = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
        s = np.bincount(g, weights=dist, minlength=k)
        a = s[g[i]] / (cnt[g[i]] - 1)
        b = np.min(np.delete(s / cnt, g[i]))
        ref[q] = 1.0 - a / b if a < b else (b / a - 1.0 if a > b else 0.0)
    err = float(np.max(np.abs(w[rows] - ref) - RTOL * np.abs(ref)))
    print(f"n={n}: {len(rows)} rows, worst |w - ref| - rtol |ref| = {err:.3g} (atol {ATOL:g})")
    np.testing.assert_allclose(w[rows], ref, rtol=RTOL, atol=ATOL)
    assert np.all(np.isfinite(w)) and np.all(np.abs(w) <= 1.0)
    means = np.array([w[g == c].mean() for c in range(k)])
    # the long-double means against numpy's pairwise sums of ~1250 widths below 1 in magnitude:
    # ~log2(1250) roundings of 1.1e-16 each on the mean
    np.testing.assert_allclose(ca, means, rtol=0, atol=1e-14)


# ------------------------------------- 6. determinism and read-only scores
def test_two_calls_same_bits_and_scores_untouched(eng):
    n = 3000
    t = _device_scores(_points(n)["x"])
    before = t.clone()
    g = _groups("k65", n)
    w0, c0 = eng.silhouette_scores(n, g, t.data_ptr())
    w1, c1 = eng.silhouette_scores(n, g, t.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(w0, w1) and np.array_equal(c0, c1)
    assert torch.equal(t, before)


# ------------------------------------------------------------- 7. refusals
def test_no_kept_scores_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.silhouette_scores(65, np.arange(65, dtype=np.int32) % 3)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


def test_kept_scores_answer_where_the_distance_is_gone(eng, cfg_a):
    d, ds, union, code = cfg_a
    eng.pca_scores(ds, union)
    with pytest.raises(nat.SccError) as e:
        eng.silhouette_scores(d.N - 1, code[:-1])
    assert e.value.code == nat.SCC_ERR_INVALID
    w, ca = eng.silhouette_scores(d.N, code)
    assert w.shape == (d.N,) and len(ca) == len(np.unique(code))
    assert np.all(np.isfinite(w)) and np.all(np.abs(w) <= 1.0)
    with pytest.raises(nat.SccError) as e:
        eng.silhouette(d.N, code)
    assert e.value.code == nat.SCC_ERR_INVALID


@pytest.mark.parametrize("kind", ["one group", "n groups"])
def test_bad_group_count_is_invalid(eng, kind):
    n = 65
    g = np.zeros(n, np.int32) if kind == "one group" else np.arange(n, dtype=np.int32)
    with pytest.raises(nat.SccError) as e:
        eng.silhouette_scores(n, g, _points(n)["t"].data_ptr())
    assert e.value.code == nat.SCC_ERR_INVALID


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_nonfinite_score_is_refused(eng, value):
    n = 65
    x = _points(n)["x"].copy()
    x[n // 3, 4] = value
    t = _device_scores(x)
    with pytest.raises(nat.SccError) as e:
        eng.silhouette_scores(n, _groups("k2", n), t.data_ptr())
    assert e.value.code == nat.SCC_ERR_NONFINITE


# ------------------------------------------------------------------ 8. API
def test_api_scores_si_equals_host_si(cfg_a):
    d = cfg_a[0]
    kw = dict(deepSplitValues=(1, 2, 3, 4), minClusterSize=10, return_details=True)
    host = api.reclusterDEConsensusFast(d, d.labels, tree="host", **kw)
    wv.assert_tie_free(host["cellTree"]["height"])
    sc = api.reclusterDEConsensusFast(d, d.labels, tree="scores", scores_si=True, **kw)
    assert sc["dynamicColors"] == host["dynamicColors"]
    assert sc["_details"]["dist"] is None
    rows, href = sc["_details"]["deepSplitInfo"], host["_details"]["deepSplitInfo"]
    assert len(rows) == len(href) == 4
    for r, h in zip(rows, href):
        assert r["DeepSplit"] == h["DeepSplit"]
        assert r["NumbersOfClusters"] == h["NumbersOfClusters"]
        assert isinstance(r["SI"], float) and r["SI"] == h["SI"]
    with pytest.raises(ValueError):
        api.reclusterDEConsensusFast(d, d.labels, tree="host", scores_si=True, **kw)


# ------------------------------------------------------ 9. launch accounting
def test_profiled_call_is_timed_as_silhouette_scores(eng):
    n = 1025
    t = _points(n)["t"]
    g = _groups("k17", n)
    packed = torch.tensor(eng.distance_scores(t.data_ptr(), n, 0, n), device="cuda")
    torch.cuda.synchronize()
    prof = nat.Engine(0, profile=True)
    prof.reset_timers()
    wd, cd = prof.silhouette(n, g, dist_device_ptr=packed.data_ptr())
    ws, cs = prof.silhouette_scores(n, g, t.data_ptr())
    ms_d, n_d = prof.kernel_time("silhouette")
    ms_s, n_s = prof.kernel_time("silhouette_scores")
    assert n_d > 0 and n_s == n_d
    assert ms_s > 0.0
    assert np.array_equal(ws, wd) and np.array_equal(cs, cd)
    prof.close()
