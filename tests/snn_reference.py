"""The shared-nearest-neighbour graph and the multilevel modularity clustering
as the engine defines them (include/scc.h: scc_snn_graph,
scc_modularity_cluster), in plain NumPy.

Graph: Seurat's ComputeSNN rule on a k-NN table that leaves the cell itself
out (k.param = K = k + 1): with N_i = {i} + idx[i] and s = |N_i & N_j|, the
pair i != j is an edge of weight s / (K + (K - s)) when that weight is not
below `prune`.  The diagonal is not stored.  The counts come from the sparse
product M M^T of the membership matrix.

Clustering: synchronous local-move sweeps on integer weights
q = rint(w 2^32), every sum of weights an exact integer, the gain and the
modularity evaluated in float64 in one written order; communities are
aggregated level after level.  No random order, no refinement.

Agreement with Seurat, igraph or leidenalg is not claimed: none was available
to compare with."""
import numpy as np

from umap_reference import fixed_total

MAX_SWEEPS = 256
MAX_LEVELS = 32
SCALE = 2.0 ** 32


# ---------------------------------------------------------------------- graph
def snn_graph(idx, prune=1.0 / 15.0):
    """(indptr int64 [n + 1], cols int32, vals float64, shared int32) of a table idx [n, k]."""
    import scipy.sparse as sp
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    K = k + 1
    rows = np.repeat(np.arange(n), K)
    members = np.concatenate([np.arange(n)[:, None], idx], axis=1).ravel()
    M = sp.csr_matrix((np.ones(n * K, np.int32), (rows, members)), shape=(n, n))
    S = (M @ M.T).tocoo()
    off = S.row != S.col
    r, c, s = S.row[off].astype(np.int64), S.col[off].astype(np.int64), S.data[off].astype(np.int64)
    w = s.astype(np.float64) / (K + (K - s)).astype(np.float64)
    keep = (s >= 1) & (w >= float(prune))
    r, c, s, w = r[keep], c[keep], s[keep], w[keep]
    order = np.lexsort((c, r))
    r, c, s, w = r[order], c[order], s[order], w[order]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    return indptr, c.astype(np.int32), w, s.astype(np.int32)


def snn_brute(idx, prune=1.0 / 15.0):
    """The same rule by set intersection, pair by pair (small n only)."""
    idx = np.asarray(idx)
    n, k = idx.shape
    K = k + 1
    sets = [set([i]) | set(int(v) for v in idx[i]) for i in range(n)]
    indptr, cols, vals, shared = [0], [], [], []
    for i in range(n):
        for j in range(n):
            s = len(sets[i] & sets[j])
            if j != i and s >= 1 and float(s) / float(K + (K - s)) >= prune:
                cols.append(j)
                vals.append(float(s) / float(K + (K - s)))
                shared.append(s)
        indptr.append(len(cols))
    return np.array(indptr, np.int64), np.array(cols, np.int32), np.array(vals, np.float64), np.array(shared, np.int32)


# ----------------------------------------------------------------- clustering
def quantise(vals):
    return np.rint(np.asarray(vals, np.float64) * SCALE).astype(np.int64)


def _isum(where, what, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, where, what)
    return out


def level_modularity(row, col, q, comm, tot, gamma, m2):
    """Q of a state: term c = in_c / m2 - gamma (tot_c / m2)(tot_c / m2) for every community id
    0..n-1 of the level (an empty one gives 0), summed in fixed_total's shape."""
    n = len(comm)
    inside = comm[row] == comm[col]
    inc = _isum(comm[row[inside]], q[inside], n)
    fm = float(m2)
    a = tot.astype(np.float64) / fm
    return fixed_total(inc.astype(np.float64) / fm - (float(gamma) * a) * a)


def one_level(n, row, col, q, gamma, m2):
    """The local-move sweeps of one level: (communities, sweeps run, Q of every accepted state)."""
    gamma = float(gamma)
    ar = np.arange(n, dtype=np.int64)
    k = _isum(row, q, n)
    comm, tot, size = ar.copy(), k.copy(), np.ones(n, np.int64)
    qs = [level_modularity(row, col, q, comm, tot, gamma, m2)]
    nb = (col != row) & (q > 0)
    r_, c_, q_ = row[nb], col[nb], q[nb]
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        key = np.concatenate([r_ * n + comm[c_], ar * n + comm])
        uk, inv = np.unique(key, return_inverse=True)
        kin = _isum(inv.ravel(), np.concatenate([q_, np.zeros(n, np.int64)]), len(uk))
        ui, uc = uk // n, uk % n
        own = uc == comm[ui]
        t = tot[uc] - np.where(own, k[ui], 0)
        g = kin.astype(np.float64) - ((gamma * k[ui].astype(np.float64)) * t.astype(np.float64)) / float(m2)
        order = np.lexsort((uc, -g, ui))
        first = order[np.r_[True, ui[order][1:] != ui[order][:-1]]]
        best_c, best_g, g_own = uc[first], g[first], g[own]
        move = (best_c != comm) & (best_g > g_own) & ~((size[best_c] == 1) & (size[comm] == 1) & (best_c > comm))
        if not move.any():
            break
        new = np.where(move, best_c, comm)
        tot2 = _isum(new, k, n)
        q2 = level_modularity(row, col, q, new, tot2, gamma, m2)
        if q2 <= qs[-1]:
            break
        comm, tot, size = new, tot2, np.bincount(new, minlength=n).astype(np.int64)
        qs.append(q2)
    return comm, sweeps, qs


def number_labels(member):
    """Communities numbered by (size descending, smallest member ascending)."""
    member = np.asarray(member, np.int64)
    ids, first, counts = np.unique(member, return_index=True, return_counts=True)
    order = np.lexsort((first, -counts))
    new = np.empty(len(ids), np.int64)
    new[order] = np.arange(len(ids))
    return new[np.searchsorted(ids, member)].astype(np.int32), len(ids)


def modularity_cluster(indptr, cols, vals, resolution=1.0, trace=None):
    """{"labels", "n_clusters", "modularity", "n_levels", "sweeps"} of a symmetric CSR graph."""
    indptr = np.asarray(indptr, np.int64)
    n0 = len(indptr) - 1
    row = np.repeat(np.arange(n0, dtype=np.int64), np.diff(indptr))
    col = np.asarray(cols, np.int64)[:indptr[-1]]
    q = quantise(np.asarray(vals)[:indptr[-1]])
    m2 = int(q.sum())
    member = np.arange(n0, dtype=np.int64)
    out = {"labels": member.astype(np.int32), "n_clusters": n0, "modularity": 0.0, "n_levels": 0, "sweeps": []}
    if m2 == 0:
        return out
    n = n0
    while out["n_levels"] < MAX_LEVELS:
        comm, sweeps, qs = one_level(n, row, col, q, resolution, m2)
        if out["n_levels"] == 0 or len(qs) > 1:
            out["modularity"] = qs[-1]
        if trace is not None:
            trace.append(qs)
        out["n_levels"] += 1
        out["sweeps"].append(sweeps)
        ids = np.unique(comm)
        if len(ids) == n:
            break
        newid = np.searchsorted(ids, comm)
        member = newid[member]
        nc = len(ids)
        uk, inv = np.unique(newid[row] * nc + newid[col], return_inverse=True)
        q = _isum(inv.ravel(), q, len(uk))
        row, col, n = uk // nc, uk % nc, nc
    out["labels"], out["n_clusters"] = number_labels(member)
    return out


# --------------------------------------------------------------------- inputs
def blobs(n, scale, seed=0, centres=8, dim=8):
    """n points around `centres` Gaussian centres of spread `scale` in `dim` dimensions, and their blob."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((centres, dim)) * scale
    lab = np.arange(n) % centres
    return mu[lab] + rng.standard_normal((n, dim)), lab


def knn_table(X, k):
    """Exact k-NN table [n, k] by (distance, index), the point itself left out (small n: dense)."""
    X = np.asarray(X, np.float64)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) if len(X) <= 400 else \
        (X * X).sum(1)[:, None] + (X * X).sum(1)[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(d2, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(len(X)), d2.shape), d2), axis=1)
    return order[:, :k].astype(np.int32)
