"""GPU: hclust(ward.D2) and the dynamic tree cut from the PCA scores, without
the N x N matrix (scc_pca_scores, scc_hclust_ward_d2_scores,
scc_cutree_hybrid_scores; reference lines R/reclusterDEConsensusFast.R:398-431,
R/reclusterDEConsensus.R:234-266).

The tree is compared with the host function on tie-free inputs: ``merge`` and
``order`` equal, heights within a relative 1e-12 (the derivation of the bound
is in test_ward_vector_reference), and the condition on the input (smallest
relative gap between consecutive host heights >= 1e-9) asserted first.  On
inputs with exact ties only the validity of the tree is checked.  The cut's
distance entries are the dist kernel's bit for bit, so its labels are compared
with ``array_equal``.  The loop caps, a corrupt state and memory exhaustion are
not provoked here (as in test_gpu_hclust_dev)."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial.distance import pdist

import ward_vector_reference as wv
from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth
from test_gpu_hclust_dev import CUTS, SIZES

pytestmark = pytest.mark.gpu

S = nat.HCLUST_VEC_SCAN_NODES
# test_gpu_hclust_dev's sizes; the edges of one and two scan workgroups; 3000
# needs several launch batches (asserted below)
TREE_SIZES = sorted(set(SIZES + [S - 1, S, S + 1, 2 * S + 1]))
MULTI_BATCH_N = 3000


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


_HOST = {}


def _host_tree(n):
    """Blob points and the host tree of their distances, computed once."""
    if n not in _HOST:
        x = wv.blobs(n)
        m, h, o = nat.hclust_ward_d2(pdist(x), n)
        for a in (x, m, h, o):
            a.setflags(write=False)
        _HOST[n] = (x, m, h, o)
    return _HOST[n]


def _device_scores(x):
    """[n][16] device scores from points of up to 16 dimensions, zero-padded."""
    p = np.zeros((x.shape[0], 16))
    p[:, :x.shape[1]] = x
    t = torch.tensor(p, device="cuda")
    torch.cuda.synchronize()
    return t


def _assert_same_tree(got, host):
    (mg, hg, og), (m, h, o) = got, host
    wv.assert_tie_free(h)
    assert np.array_equal(mg, m)
    assert np.array_equal(og, o)
    rel = float(np.max(np.abs(hg - h) / h))
    print(f"n={len(o)}: worst relative height error {rel:.3g}, smallest gap {wv.min_relative_gap(h):.3g}")
    assert rel <= 1e-12


# ------------------------------------------------------------------ 1. tree
@pytest.mark.parametrize("n", TREE_SIZES)
def test_tree_equals_host_on_tie_free_blobs(eng, n):
    x, m, h, o = _host_tree(n)
    t = _device_scores(x)
    got = eng.hclust_ward_d2_scores(n, t.data_ptr())
    _assert_same_tree(got, (m, h, o))
    scans = eng.hclust_last_scans()
    assert n - 1 <= scans < 3 * n
    if n == MULTI_BATCH_N:
        assert scans > nat.HCLUST_VEC_SCANS_PER_BATCH  # more than one launch batch


def test_scores_are_read_only(eng):
    n = 1025
    x = _host_tree(n)[0]
    t = _device_scores(x)
    before = t.clone()
    eng.hclust_ward_d2_scores(n, t.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(t, before)


# ---------------------------------------------------------------- config A
@pytest.fixture(scope="module")
def cfg_a(eng):
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    return d, ds, union


# ------------------------------------------------------------------- 2. cut
def test_cut_distances_are_the_dist_kernels(eng, cfg_a):
    d, ds, union = cfg_a
    dist = eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID)  # to the host; the scores are kept
    m, h, _ = nat.hclust_ward_d2(dist, d.N)
    for dsv, mcs in CUTS:
        lh, ch = nat.cutree_hybrid(m, h, dist, dsv, mcs)
        ls, cs = eng.cutree_hybrid_scores(m, h, dsv, mcs)
        assert np.array_equal(ls, lh), (dsv, mcs)
        assert cs == ch, (dsv, mcs)


# ------------------------------------------------------------ 3. pca_scores
def test_pca_scores_leaves_the_scores_of_distance(eng, cfg_a):
    d, ds, union = cfg_a
    eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0)
    eng.synchronize()
    after_distance = eng.last_pca_scores(d.N)
    eng.pca_scores(ds, union)
    after_scores = eng.last_pca_scores(d.N)
    assert after_scores.shape == after_distance.shape == (d.N, 15)
    assert np.array_equal(after_scores, after_distance)
    # the kept distance of the earlier call is dropped, not read
    with pytest.raises(nat.SccError) as e:
        eng.hclust_ward_d2_dev(d.N)
    assert e.value.code == nat.SCC_ERR_INVALID
    with pytest.raises(nat.SccError) as e:
        eng.silhouette(d.N, np.arange(d.N, dtype=np.int32) % 3)
    assert e.value.code == nat.SCC_ERR_INVALID


# ------------------------------------------------------------------ 4. ties
def _tied_points(kind, n):
    rng = np.random.default_rng(1000 * n + 7)
    if kind == "lattice":  # 2-D integer lattice with duplicates
        side = max(2, int(math.sqrt(n) / 2))
        return rng.integers(0, side, size=(n, 2)).astype(np.float64)
    return rng.permutation(n).astype(np.float64)[:, None]  # shuffled collinear points


@pytest.mark.parametrize("kind", ["lattice", "collinear"])
@pytest.mark.parametrize("n", [65, 1025])
def test_ties_give_a_valid_tree(eng, n, kind):
    x = _tied_points(kind, n)
    t = _device_scores(x)
    m, h, o = eng.hclust_ward_d2_scores(n, t.data_ptr())
    # a valid R merge matrix: every observation and every earlier row used exactly once
    used = m.reshape(-1)
    assert sorted((-used[used < 0]).tolist()) == list(range(1, n + 1))
    pos = used[used > 0]
    assert sorted(pos.tolist()) == list(range(1, n - 1))
    for k in range(n - 1):
        assert m[k, 0] != 0 and m[k, 1] != 0
        assert max(m[k, 0], m[k, 1]) <= k  # a row names only earlier rows (1-based: row k is k + 1)
    assert sorted(o.tolist()) == list(range(1, n + 1))
    assert np.all(np.isfinite(h))
    assert np.all(np.diff(h) >= 0)
    # duplicates merge at height 0: one zero-height merge per redundant point
    n_dup = n - len(np.unique(x, axis=0))
    assert np.count_nonzero(h == 0.0) == n_dup


# -------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_nonfinite_score_is_refused(eng, value):
    n = 65
    x = _host_tree(n)[0].copy()
    x[n // 3, 4] = value
    t = _device_scores(x)
    with pytest.raises(nat.SccError) as e:
        eng.hclust_ward_d2_scores(n, t.data_ptr())
    assert e.value.code == nat.SCC_ERR_NONFINITE


def test_no_kept_scores_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.hclust_ward_d2_scores(65)
    assert e.value.code == nat.SCC_ERR_INVALID
    with pytest.raises(nat.SccError) as e:
        fresh.cutree_hybrid_scores(np.array([[-1, -2]], np.int32), np.array([1.0]), 1, 10)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


def test_wrong_n_against_kept_scores_is_invalid(eng, cfg_a):
    d, ds, union = cfg_a
    eng.pca_scores(ds, union)
    with pytest.raises(nat.SccError) as e:
        eng.hclust_ward_d2_scores(d.N - 1)
    assert e.value.code == nat.SCC_ERR_INVALID


# ------------------------------------------------------------------- 6. API
def _same_result(sc, host):
    h = host["cellTree"]["height"]
    wv.assert_tie_free(h)
    assert sc["deGeneUnion"] == host["deGeneUnion"]
    assert np.array_equal(sc["cellTree"]["merge"], host["cellTree"]["merge"])
    assert np.array_equal(sc["cellTree"]["order"], host["cellTree"]["order"])
    rel = float(np.max(np.abs(sc["cellTree"]["height"] - h) / h))
    print(f"worst relative height error {rel:.3g}, smallest gap {wv.min_relative_gap(h):.3g}")
    assert rel <= 1e-12
    assert sc["dynamicColors"] == host["dynamicColors"]
    assert sc["_details"]["dist"] is None
    assert host["_details"]["dist"] is not None


def test_api_fast_scores_tree_equals_host_tree(cfg_a):
    d = cfg_a[0]
    kw = dict(deepSplitValues=(1, 2, 3, 4), minClusterSize=10, return_details=True)
    host = api.reclusterDEConsensusFast(d, d.labels, tree="host", **kw)
    sc = api.reclusterDEConsensusFast(d, d.labels, tree="scores", **kw)
    _same_result(sc, host)
    rows, href = sc["_details"]["deepSplitInfo"], host["_details"]["deepSplitInfo"]
    assert [(r["DeepSplit"], r["NumbersOfClusters"]) for r in rows] == \
        [(r["DeepSplit"], r["NumbersOfClusters"]) for r in href]
    assert all(r["SI"] is None for r in rows)
    with pytest.raises(ValueError):
        api.reclusterDEConsensusFast(d, d.labels, tree="score", **kw)


def test_api_slow_scores_tree_equals_host_tree(cfg_a):
    d = cfg_a[0]
    kw = dict(qValThrs=0.05, fcThrs=1.5, deepSplitValues=(1, 2, 3, 4), minClusterSize=10, return_details=True)
    host = api.reclusterDEConsensus(d, d.labels, tree="host", **kw)
    sc = api.reclusterDEConsensus(d, d.labels, tree="scores", **kw)
    _same_result(sc, host)


# ------------------------------------------------------ 7. launch accounting
def test_scan_launches_come_in_whole_batches():
    """profile=1: every launch of the chain is timed under hclust_vec, two
    launches per scan, a whole number of batches per call."""
    n = MULTI_BATCH_N
    x = _host_tree(n)[0]
    prof = nat.Engine(0, profile=True)
    t = _device_scores(x)
    prof.reset_timers()
    prof.hclust_ward_d2_scores(n, t.data_ptr())
    ms, launches = prof.kernel_time("hclust_vec")
    scans = prof.hclust_last_scans()
    per_batch = 2 * nat.HCLUST_VEC_SCANS_PER_BATCH
    assert launches > 0 and launches % per_batch == 0
    assert launches // per_batch == math.ceil(scans / nat.HCLUST_VEC_SCANS_PER_BATCH)
    assert ms > 0.0
    assert n - 1 <= scans < 3 * n
    prof.close()
