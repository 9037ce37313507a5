"""numpy/scipy restatement of the heatmap inputs (include/scc.h: "heatmap
inputs", cellTypeDEPlot.R:168-253): what ComplexHeatmap::Heatmap(cluster_rows
= TRUE, use_raster = TRUE) computes from dataMatrix[deGeneUnion, ] before it
draws.  Independent of the engine's code: long-double direct differences,
scipy's complete linkage, a recursive reorder, a long-double block mean.
Pinned by tests/test_heatmap_reference.py."""
import numpy as np
from scipy.cluster.hierarchy import linkage

LD = np.longdouble


def packed_index(n, i, j):
    """Position of (i, j), i != j, in R's packed `dist` vector of n observations."""
    i, j = (i, j) if i < j else (j, i)
    return n * i - i * (i + 1) // 2 + (j - i - 1)


def gene_dist(X):
    """dist(X, "euclidean") of the rows of X (genes x cells), packed in R order:
    sqrt(sum (x_a - x_b)^2) in long double (returned as long double)."""
    X = np.asarray(X, np.float64).astype(LD)
    n = X.shape[0]
    out = np.empty(n * (n - 1) // 2, LD)
    k = 0
    for b in range(n - 1):  # column b of the lower triangle: rows b + 1 .. n - 1
        d = X[b + 1:] - X[b]
        out[k:k + n - 1 - b] = np.sqrt((d * d).sum(axis=1))
        k += n - 1 - b
    return out


def row_means(X):
    X = np.asarray(X, np.float64).astype(LD)
    return X.sum(axis=1) / LD(X.shape[1])


def value_range(X):
    """{min x, max x, min |x|, max |x|} (the colour ramp's inputs, cellTypeDEPlot.R:174-222)."""
    X = np.asarray(X, np.float64)
    A = np.abs(X)
    return np.array([X.min(), X.max(), A.min(), A.max()])


def linkage_to_r(Z, n):
    """scipy linkage matrix -> R's hclust (merge (n-1, 2), height, order):
    -i = observation i, +k = the k-th merge (1-based); in a row singletons come
    before clusters, two singletons and two clusters in increasing index; the
    order is the left-to-right leaf order of merge."""
    merge = np.zeros((n - 1, 2), np.int32)
    for k in range(n - 1):
        a, b = sorted((int(Z[k, 0]), int(Z[k, 1])))  # leaves (< n) sort before clusters (>= n)
        merge[k] = [-(a + 1) if a < n else a - n + 1, -(b + 1) if b < n else b - n + 1]
    return merge, Z[:, 2].copy(), merge_order(merge)


def merge_order(merge):
    """Left-to-right 1-based leaf order of an R merge matrix."""
    merge = np.asarray(merge)
    out, stack = [], [merge.shape[0]]
    while stack:
        c = stack.pop()
        if c < 0:
            out.append(-c)
        else:
            stack.append(int(merge[c - 1, 1]))
            stack.append(int(merge[c - 1, 0]))
    return np.array(out, np.int32)


def hclust_complete(d, n):
    """stats::hclust(d, "complete") through scipy (unique when d has no ties)."""
    return linkage_to_r(linkage(np.asarray(d, np.float64), "complete"), n)


def hclust_complete_brute(d, n):
    """The textbook algorithm, O(n^3): merge the closest pair of clusters under
    max linkage (the first such pair on a tie); R conventions."""
    d = np.asarray(d, np.float64)
    members = {-(i + 1): [i] for i in range(n)}  # R id -> leaves
    merge, height = np.zeros((n - 1, 2), np.int32), np.zeros(n - 1)

    def key(c):  # singletons first, then increasing index
        return (0, -c) if c < 0 else (1, c)

    for k in range(n - 1):
        ids = sorted(members, key=key)
        best = None
        for x in range(len(ids)):
            for y in range(x + 1, len(ids)):
                h = max(d[packed_index(n, i, j)] for i in members[ids[x]] for j in members[ids[y]])
                if best is None or h < best[0]:
                    best = (h, ids[x], ids[y])
        h, a, b = best
        merge[k], height[k] = [a, b], h
        members[k + 1] = members.pop(a) + members.pop(b)
    return merge, height, merge_order(merge)


def r_mean2(a, b):
    """R's mean(c(a, b)): a long-double sum, one correction pass."""
    a, b = LD(a), LD(b)
    s = (a + b) / LD(2)
    s += ((a - s) + (b - s)) / LD(2)
    return float(s)


def dendro_reorder(merge, wts):
    """stats::reorder.dendrogram(as.dendrogram(tree), wts, agglo.FUN = mean):
    a leaf's value is its weight, an inner node's the mean of its children's;
    children in increasing value, an equal pair keeps its order.  Returns
    (merge with the swapped rows, the 1-based leaf order)."""
    merge = np.array(merge, np.int32)
    val = np.zeros(merge.shape[0])
    for k in range(merge.shape[0]):  # rows refer to earlier rows only
        v = [wts[-c - 1] if c < 0 else val[c - 1] for c in merge[k]]
        if v[1] < v[0]:
            merge[k] = merge[k, ::-1]
            v = v[::-1]
        val[k] = r_mean2(v[0], v[1])
    return merge, merge_order(merge)


def leaf_sets(merge):
    """The set of leaves under every row of a merge matrix (as frozensets)."""
    sets = []
    for a, b in np.asarray(merge):
        s = set()
        for c in (int(a), int(b)):
            s |= {-c} if c < 0 else sets[c - 1]
        sets.append(frozenset(s))
    return sets


def is_valid_tree(merge, n):
    """Every leaf and every row but the last is a child exactly once, rows refer to earlier rows."""
    used = []
    for k, (a, b) in enumerate(np.asarray(merge)):
        for c in (int(a), int(b)):
            if c == 0 or c < -n or c > k:
                return False
            used.append(c)
    return sorted(used) == sorted(list(range(-n, 0)) + list(range(1, n - 1)))


def bin_edges(N, width):
    return [(b * N) // width for b in range(width + 1)]


def raster(X, row_order, cell_order, width):
    """|U| x width long-double bin means of X[row_order - 1][:, cell_order - 1]
    over the bins [floor(b N / width), floor((b + 1) N / width)); also the
    per-entry bound n_bin 2^-53 mean|x| the device sum is held to."""
    X = np.asarray(X, np.float64)
    M = X[np.asarray(row_order) - 1][:, np.asarray(cell_order) - 1].astype(LD)
    N = M.shape[1]
    e = bin_edges(N, width)
    out = np.empty((M.shape[0], width), LD)
    bound = np.empty((M.shape[0], width))
    for b in range(width):
        blk = M[:, e[b]:e[b + 1]]
        nb = e[b + 1] - e[b]
        out[:, b] = blk.sum(axis=1) / LD(nb)
        bound[:, b] = (nb * 2.0 ** -53 * np.abs(blk).sum(axis=1) / LD(nb)).astype(np.float64)
    return out, bound
