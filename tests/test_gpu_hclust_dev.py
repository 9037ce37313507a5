"""GPU: hclust(ward.D2) and the dynamic tree cut on the HBM-resident distance
(scc_hclust_ward_d2_dev, scc_cutree_hybrid_dev; reference lines
R/reclusterDEConsensusFast.R:406-431, R/reclusterDEConsensus.R:242-266).

The contract is equality with the host functions on the same distance values:
every comparison is ``array_equal`` against ``nat.hclust_ward_d2`` /
``nat.cutree_hybrid``, no tolerance.  The kernel's loop caps and the
half-of-free-memory rule are not tested here: reaching them means provoking a
corrupt matrix or exhausting a shared device."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial.distance import pdist

from scconsensus_amd import _native as nat
from scconsensus_amd import api, synth

pytestmark = pytest.mark.gpu

# single merge and the tip <= 3 restart; the wave edge; one and two elements
# per thread of the 1024-thread chain kernel; several chain launches
SIZES = [2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049, 3000]
KINDS = ["blobs", "lattice", "ones", "collinear"]


def _packed(kind, n):
    """A packed R `dist` vector (row-major upper triangle) of n points."""
    rng = np.random.default_rng(1000 * n + KINDS.index(kind))
    if kind == "blobs":  # seeded Gaussian blobs in 15 dimensions
        k = max(1, min(8, n // 8))
        centers = rng.normal(scale=6.0, size=(k, 15))
        x = centers[rng.integers(0, k, n)] + rng.normal(size=(n, 15))
        return pdist(x)
    if kind == "lattice":  # integer lattice with duplicates: exact ties and zero distances
        side = max(2, int(math.sqrt(n) / 2))
        return pdist(rng.integers(0, side, size=(n, 2)).astype(np.float64))
    if kind == "ones":
        return np.ones(n * (n - 1) // 2)
    # collinear points 0 .. n-1, shuffled: long chains and restarts
    return pdist(rng.permutation(n).astype(np.float64)[:, None])


@pytest.fixture(scope="module")
def eng():
    return nat.Engine(0)


_HOST = {}


def _host_tree(kind, n, f32):
    key = (kind, n, f32)
    if key not in _HOST:
        d = _packed(kind, n)
        if f32:
            d = d.astype(np.float32)
        m, h, o = nat.hclust_ward_d2(d.astype(np.float64), n)
        for a in (d, m, h, o):
            a.setflags(write=False)
        _HOST[key] = (d, m, h, o)
    return _HOST[key]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_tree_equals_host(eng, n, kind, f32):
    d, m, h, o = _host_tree(kind, n, f32)
    t = torch.tensor(d, device="cuda")
    torch.cuda.synchronize()
    md, hd, od = eng.hclust_ward_d2_dev(n, t.data_ptr(), f32=f32)
    assert np.array_equal(md, m)
    assert np.array_equal(hd, h)
    assert np.array_equal(od, o)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_nonfinite_entry_is_refused(eng, value):
    n = 65
    d = _packed("blobs", n).copy()
    d[len(d) // 3] = value
    t = torch.tensor(d, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(nat.SccError) as e:
        eng.hclust_ward_d2_dev(n, t.data_ptr())
    assert e.value.code == nat.SCC_ERR_NONFINITE


def test_no_kept_distance_is_invalid():
    fresh = nat.Engine(0)
    with pytest.raises(nat.SccError) as e:
        fresh.hclust_ward_d2_dev(65)
    assert e.value.code == nat.SCC_ERR_INVALID
    with pytest.raises(nat.SccError) as e:
        fresh.cutree_hybrid_dev(np.array([[-1, -2]], np.int32), np.array([1.0]), 1, 10)
    assert e.value.code == nat.SCC_ERR_INVALID
    fresh.close()


# ---------------------------------------------------------------- config A
@pytest.fixture(scope="module")
def cfg_a(eng):
    d = synth.generate("A")
    names, code = api.select_clusters(d.labels, 10)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    host = {}
    for f32 in (False, True):
        dist = eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID, f32=f32)
        d64 = dist.astype(np.float64)
        m, h, o = nat.hclust_ward_d2(d64, d.N)
        host[f32] = (d64, m, h, o)
    return d, ds, union, host


CUTS = [(dsv, mcs) for dsv in range(5) for mcs in (10, 30)]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_config_a_tree_and_cuts_from_kept_distance(eng, cfg_a, f32):
    d, ds, union, host = cfg_a
    d64, m, h, o = host[f32]
    got = eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID, f32=f32)  # the engine keeps its device copy
    assert np.array_equal(got.astype(np.float64), d64)
    lab2, _ = nat.cutree_hybrid(m, h, d64, 2, 10)
    w0, _ = eng.silhouette(d.N, lab2)
    md, hd, od = eng.hclust_ward_d2_dev(d.N)
    assert np.array_equal(md, m)
    assert np.array_equal(hd, h)
    assert np.array_equal(od, o)
    for dsv, mcs in CUTS:
        lh, ch = nat.cutree_hybrid(m, h, d64, dsv, mcs)
        ld, cd = eng.cutree_hybrid_dev(md, hd, dsv, mcs)
        assert np.array_equal(ld, lh), (dsv, mcs)
        assert cd == ch, (dsv, mcs)
    # the kept distance is read, never written
    w1, _ = eng.silhouette(d.N, lab2)
    assert np.array_equal(w0, w1)


def test_wrong_n_against_kept_distance_is_invalid(eng, cfg_a):
    d, ds, union, _ = cfg_a
    eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0)
    with pytest.raises(nat.SccError) as e:
        eng.hclust_ward_d2_dev(d.N - 1)
    assert e.value.code == nat.SCC_ERR_INVALID


def _same_result(dev, host):
    for k in ("merge", "height", "order"):
        assert np.array_equal(dev["cellTree"][k], host["cellTree"][k]), k
    assert dev["deGeneUnion"] == host["deGeneUnion"]
    assert dev["dynamicColors"] == host["dynamicColors"]
    assert dev["_details"]["dist"] is None
    assert host["_details"]["dist"] is not None


def test_api_fast_device_tree_equals_host_tree(cfg_a):
    d = cfg_a[0]
    kw = dict(deepSplitValues=(1, 2, 3, 4), minClusterSize=10, return_details=True)
    host = api.reclusterDEConsensusFast(d, d.labels, tree="host", **kw)
    dev = api.reclusterDEConsensusFast(d, d.labels, tree="device", **kw)
    _same_result(dev, host)
    assert dev["_details"]["deepSplitInfo"] == host["_details"]["deepSplitInfo"]
    with pytest.raises(ValueError):
        api.reclusterDEConsensusFast(d, d.labels, tree="gpu", **kw)


def test_api_slow_device_tree_equals_host_tree(cfg_a):
    d = cfg_a[0]
    kw = dict(qValThrs=0.05, fcThrs=1.5, deepSplitValues=(1, 2, 3, 4), minClusterSize=10, return_details=True)
    host = api.reclusterDEConsensus(d, d.labels, tree="host", **kw)
    dev = api.reclusterDEConsensus(d, d.labels, tree="device", **kw)
    _same_result(dev, host)


def test_chain_launches_are_bounded_and_timed():
    """profile=1: the chain runs as ceil((n - 1) / M) launches under the
    timer family hclust_dev, the expansion under hclust_expand."""
    n = 3000
    d = _host_tree("blobs", n, False)[0]
    prof = nat.Engine(0, profile=True)
    t = torch.tensor(d, device="cuda")
    torch.cuda.synchronize()
    prof.reset_timers()
    prof.hclust_ward_d2_dev(n, t.data_ptr())
    ms, launches = prof.kernel_time("hclust_dev")
    assert launches == math.ceil((n - 1) / nat.HCLUST_MERGES_PER_LAUNCH) == 3
    assert ms > 0.0
    assert prof.kernel_time("hclust_expand")[1] == 1
    assert n - 1 <= prof.hclust_last_scans() < 3 * n
    prof.close()
