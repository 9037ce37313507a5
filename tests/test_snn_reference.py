"""CPU: the NumPy restatement of the SNN graph and the modularity clustering
(snn_reference) against brute force, hand cases and networkx.

Quality.  Q of the reference's labels (networkx.community.modularity on the
float64 graph) may fall short of the best of networkx's Louvain over seeds 0..4
by at most MARGIN = twice the largest shortfall measured over the four inputs
below (profiles/snn_cluster.md lists them: 0, 0.000813, 0 and -0.002874: at
gamma = 2 the reference is ahead)."""
import networkx as nx
import numpy as np
import pytest

import snn_reference as sr

MARGIN = 2 * 0.000813
# Blob centres are drawn at `scale` times a standard normal; the points have unit spread.  Seed 1: at scale 3.0 the
# closest two centres lie 7.1 apart, beyond both blobs' 3-sigma radii.  (At seed 0 two centres lie 3.8 apart, the
# blobs overlap, and the planted partition's Q, 0.8586, is below what networkx itself finds, 0.8613: no modularity
# method returns it.)
SEED = 1
QUALITY = [(1500, 3.0, 1.0), (1500, 1.0, 1.0), (1500, 1.5, 0.2), (1500, 1.0, 2.0)]


def _random_table(n, k, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)


@pytest.mark.parametrize("n,k", [(2, 1), (3, 2), (17, 4), (40, 7), (65, 19), (65, 64)])
def test_graph_equals_brute_force(n, k):
    idx = _random_table(n, k, 100 * n + k)
    for prune in (0.0, 1.0 / 15.0, 0.5, 1.0):
        got, ref = sr.snn_graph(idx, prune), sr.snn_brute(idx, prune)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert np.array_equal(got[2].view(np.int64), ref[2].view(np.int64))


def test_two_cells_share_everything():
    indptr, cols, vals, shared = sr.snn_graph(np.array([[1], [0]], np.int32))
    assert indptr.tolist() == [0, 1, 2] and cols.tolist() == [1, 0] and shared.tolist() == [2, 2]
    assert vals.tolist() == [1.0, 1.0]


def test_prune_boundary_is_kept():
    # K = 8, s = 1: w = 1 / 15, the same f64 as the default prune, so the pair stays
    n, k = 16, 7
    idx = np.array([[(i + t) % n for t in range(1, k + 1)] for i in range(n)], np.int32)
    indptr, cols, vals, shared = sr.snn_graph(idx, 1.0 / 15.0)
    assert (shared == 1).any() and np.all(vals[shared == 1] == 1.0 / 15.0)
    off = sr.snn_graph(idx, np.nextafter(1.0 / 15.0, 1.0))
    assert not (off[3] == 1).any() and len(off[1]) == len(cols) - int((shared == 1).sum())


def _csr(n, edges):
    """Symmetric CSR of weighted edges (i, j, w), i != j."""
    both = sorted({(i, j): w for i, j, w in edges} | {(j, i): w for i, j, w in edges})
    w = {(i, j): v for i, j, v in edges}
    w.update({(j, i): v for i, j, v in edges})
    indptr = np.zeros(n + 1, np.int64)
    for i, _ in both:
        indptr[i + 1] += 1
    return np.cumsum(indptr), np.array([j for _, j in both], np.int32), np.array([w[e] for e in both], np.float64)


def cliques(sizes, bridges=()):
    edges, start = [], 0
    for s in sizes:
        edges += [(start + a, start + b, 1.0) for a in range(s) for b in range(a + 1, s)]
        start += s
    return _csr(start, edges + list(bridges))


def ring_of_cliques(m=8, s=6):
    return cliques([s] * m, [(c * s + s - 1, ((c + 1) % m) * s, 1.0) for c in range(m)])


def test_two_disjoint_cliques():
    out = sr.modularity_cluster(*cliques([7, 5]), 1.0)
    assert out["n_clusters"] == 2 and out["labels"].tolist() == [0] * 7 + [1] * 5


def test_ring_of_cliques():
    out = sr.modularity_cluster(*ring_of_cliques(), 1.0)
    assert out["n_clusters"] == 8 and out["labels"].tolist() == [c for c in range(8) for _ in range(6)]


def test_one_edge_vertex_1_joins_community_0():
    g = _csr(2, [(0, 1, 0.5)])
    row, col, q = np.array([0, 1]), np.array([1, 0]), sr.quantise(g[2])
    comm, sweeps, qs = sr.one_level(2, row, col, q, 1.0, int(q.sum()))
    assert comm.tolist() == [0, 0] and sweeps == 2 and len(qs) == 2
    out = sr.modularity_cluster(*g, 1.0)
    assert out["labels"].tolist() == [0, 0] and out["n_clusters"] == 1 and out["modularity"] == 0.0


def test_no_weight_leaves_every_vertex_alone():
    g = _csr(3, [(0, 1, 1e-12)])
    out = sr.modularity_cluster(*g, 1.0)
    assert out["labels"].tolist() == [0, 1, 2] and out["n_levels"] == 0 and out["sweeps"] == []


def test_labels_are_numbered_by_size_then_smallest_member():
    lab, nc = sr.number_labels([5, 9, 9, 5, 9, 2, 7, 7])
    assert nc == 4 and lab.tolist() == [1, 0, 0, 1, 0, 3, 2, 2]
    out = sr.modularity_cluster(*cliques([3, 6, 4, 6]), 1.0)
    assert out["labels"].tolist() == [3] * 3 + [0] * 6 + [2] * 4 + [1] * 6


_SNN = {}


def blob_graph(n, scale):
    if (n, scale) not in _SNN:
        x, lab = sr.blobs(n, scale, seed=SEED)
        g = sr.snn_graph(sr.knn_table(x, 19))
        for a in g:
            a.setflags(write=False)
        _SNN[(n, scale)] = (g, lab)
    return _SNN[(n, scale)]


def test_modularity_never_decreases_over_accepted_sweeps():
    (indptr, cols, vals, _), _ = blob_graph(1500, 1.0)
    trace = []
    out = sr.modularity_cluster(indptr, cols, vals, 1.0, trace=trace)
    assert len(trace) == out["n_levels"] >= 2
    for qs in trace:
        assert all(b > a for a, b in zip(qs, qs[1:]))
    best = [qs[-1] for qs in trace]
    assert all(b >= a - 1e-12 for a, b in zip(best, best[1:]))  # (a level's sum has another shape: a few ulp)
    assert out["modularity"] == max(qs[-1] for qs in trace if len(qs) > 1)


def _nx_graph(indptr, cols, vals):
    G = nx.Graph()
    G.add_nodes_from(range(len(indptr) - 1))
    row = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    up = cols > row
    G.add_weighted_edges_from(zip(row[up].tolist(), cols[up].tolist(), vals[up].tolist()))
    return G


@pytest.mark.parametrize("n,scale,gamma", QUALITY)
def test_quality_against_networkx_louvain(n, scale, gamma):
    (indptr, cols, vals, _), lab = blob_graph(n, scale)
    out = sr.modularity_cluster(indptr, cols, vals, gamma)
    G = _nx_graph(indptr, cols, vals)
    mine = [set(np.flatnonzero(out["labels"] == c).tolist()) for c in range(out["n_clusters"])]
    q_mine = nx.community.modularity(G, mine, weight="weight", resolution=gamma)
    q_nx = max(nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=s),
                                       weight="weight", resolution=gamma) for s in range(5))
    print(f"n={n} scale={scale} gamma={gamma}: Q {q_mine:.6f} (fixed-point {out['modularity']:.6f}), networkx best "
          f"{q_nx:.6f}, shortfall {q_nx - q_mine:.6f}, clusters {out['n_clusters']}, sweeps {out['sweeps']}")
    assert abs(q_mine - out["modularity"]) <= 1e-8  # (the weights' quantisation: 2^-33 relative each)
    assert q_mine >= q_nx - MARGIN
    if scale == 3.0:
        assert out["n_clusters"] == 8
        pairs = {(int(a), int(b)) for a, b in zip(lab, out["labels"])}
        assert len(pairs) == 8  # the planted blobs, up to renaming
