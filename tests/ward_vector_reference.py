"""A numpy restatement of the NN-chain on centroids behind
``scc_hclust_ward_d2_scores`` (scconsensus_amd/csrc/scc_hclust_vec.hip).

Ward linkage on Euclidean points needs no distance matrix: the squared
dissimilarity the Lance-Williams update carries between clusters A and B is
``2 |A| |B| / (|A| + |B|) * ||cA - cB||^2`` and a merge is a weighted mean of
two centroids.  The control flow is the host chain's (scc_cluster.cpp:
nn_chain_ward): the ``tip <= 3`` restart from the lowest active index,
``tip -= 3`` after a merge, an ascending scan with strict ``<`` from the
carried minimum (the lowest index wins a tie), the larger index survives.
"""
import numpy as np


def _ward_row(cent, size, r, idx):
    """2 s_i s_r / (s_i + s_r) * sum_q (c_i[q] - c_r[q])^2 for the nodes idx,
    the difference form, components summed in ascending order."""
    d = cent[idx] - cent[r]
    ss = np.zeros(len(idx))
    for q in range(cent.shape[1]):
        ss = ss + d[:, q] * d[:, q]
    return 2.0 * size[idx] * size[r] / (size[idx] + size[r]) * ss


def _nearest(cent, size, act, r):
    """(value, lowest index) of the minimum over the active nodes i != r."""
    idx = np.flatnonzero(act)
    idx = idx[idx != r]
    v = _ward_row(cent, size, r, idx)
    k = int(np.argmin(v))  # the first occurrence: the lowest index on a tie
    return float(v[k]), int(idx[k])


def ward_vector_chain(x):
    """The chain's n - 1 steps (a, b, squared height) and its scan count."""
    cent = np.array(x, np.float64)
    n = cent.shape[0]
    size = np.ones(n)
    act = np.ones(n, bool)
    chain = np.zeros(n, np.int64)
    a, b, h2 = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), np.zeros(n - 1)
    start, tip, scans = 0, 0, 0
    for step in range(n - 1):
        if tip <= 3:
            i1 = start
            chain[0] = i1
            tip = 1
            mn, i2 = _nearest(cent, size, act, i1)
            scans += 1
        else:
            tip -= 3
            i1, i2 = int(chain[tip - 1]), int(chain[tip])
            mn = float(_ward_row(cent, size, i1, np.array([i2]))[0])
        while True:
            chain[tip] = i2
            v, i = _nearest(cent, size, act, i2)
            scans += 1
            before = i1
            if v < mn:
                mn, i1 = v, i
            i1, i2 = i2, i1
            tip += 1
            if i2 == before:
                break
        a[step], b[step], h2[step] = i1, i2, mn
        lo, hi = min(i1, i2), max(i1, i2)
        s, t = size[lo], size[hi]
        cent[hi] = (s * cent[lo] + t * cent[hi]) / (s + t)
        size[hi] = s + t
        act[lo] = False
        if lo == start:
            start = int(np.flatnonzero(act)[0])
    return a, b, h2, scans


def hclust_finish(n, a, b, h2):
    """The steps -> R's hclust fields (scc_cluster.cpp: ward_finish): sqrt,
    stable sort by height, union-find relabelling, left-to-right leaf order."""
    h = np.sqrt(h2)
    perm = np.argsort(h, kind="stable")
    parent = np.zeros(2 * n - 1, np.int64)

    def find(x):
        while parent[x]:
            x = parent[x]
        return x

    merge = np.zeros((n - 1, 2), np.int32)
    nsize = np.zeros(n - 1, np.int64)
    for k, p in enumerate(perm):
        u, v = find(int(a[p])), find(int(b[p]))
        parent[u] = parent[v] = n + k
        if u > v:
            u, v = v, u
        merge[k, 0] = -u - 1 if u < n else u - n + 1
        merge[k, 1] = -v - 1 if v < n else v - n + 1
        nsize[k] = (1 if u < n else nsize[u - n]) + (1 if v < n else nsize[v - n])
    order = np.zeros(n, np.int32)
    stack = [(0, n - 2)]
    while stack:
        pos, node = stack.pop()
        c1, c2 = int(merge[node, 0]), int(merge[node, 1])
        if c1 < 0:
            order[pos] = -c1
            pos += 1
        else:
            stack.append((pos, c1 - 1))
            pos += int(nsize[c1 - 1])
        if c2 < 0:
            order[pos] = -c2
        else:
            stack.append((pos, c2 - 1))
    return merge, h[perm], order


def ward_vector_tree(x):
    """(merge, height, order, scans) of hclust(dist(x), "ward.D2") from the points."""
    a, b, h2, scans = ward_vector_chain(x)
    merge, height, order = hclust_finish(len(a) + 1, a, b, h2)
    return merge, height, order, scans


def blobs(n, seed=None):
    """Seeded Gaussian blobs in 15 dimensions (the points behind
    test_gpu_hclust_dev._packed("blobs", n))."""
    rng = np.random.default_rng(1000 * n if seed is None else seed)
    k = max(1, min(8, n // 8))
    centers = rng.normal(scale=6.0, size=(k, 15))
    return centers[rng.integers(0, k, n)] + rng.normal(size=(n, 15))


def min_relative_gap(height):
    """The smallest relative gap between consecutive heights of a tree."""
    h = np.asarray(height, np.float64)
    if len(h) < 2:
        return np.inf
    return float(np.min(np.diff(h) / h[1:]))


def assert_tie_free(height, bound=1e-9):
    """The input condition of every tie-free comparison, from the host tree."""
    gap = min_relative_gap(height)
    assert gap >= bound, f"smallest relative gap between host heights {gap:.3g} < {bound:g}: choose another seed"
