"""UMAP's fuzzy simplicial set and stochastic-gradient layout as the engine
defines them (include/scc.h: scc_umap_graph, scc_umap_layout), in plain NumPy.

Graph: umap-learn's smooth_knn_dist, compute_membership_strengths and
fuzzy_simplicial_set at local_connectivity = 1, bandwidth = 1, on a k-NN table
that leaves the cell itself out (n_neighbors = k + 1).  The rows advance
together, but every row's sums run over its entries in order, one at a time,
as a loop over the row would: a row's result depends on that row alone.

Layout: one vectorised step per epoch on double-buffered positions; every
vertex adds its moves in slot order, the attraction of a slot before its
negative samples s = 0, 1, ...; every draw is a pure function of (seed, epoch,
slot, s) in uint64 arithmetic (mod 2^64).  `dtype` chooses the arithmetic of
the positions and moves (np.longdouble measures the float64 rounding); the
schedule stays float64 in either case, so both runs take the same steps.

Agreement with the umap, uwot or umap-learn packages is not claimed: none was
available to compare with."""
import numpy as np

A_DEFAULT = 1.5769434602697652  # find_ab_params(spread = 1, min_dist = 0.1)
B_DEFAULT = 0.8950608778515733
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TOL = 1e-5
FLOOR = 1e-3
TOTAL_LANES = 1024  # the fixed shape of the global sum: lane t adds x[t], x[t + 1024], ..., then a halving tree


def find_ab_params(spread=1.0, min_dist=0.1):
    """umap-learn's recipe: fit 1 / (1 + a x^(2b)) to the target curve at 300 points of [0, 3 spread]."""
    from scipy.optimize import curve_fit
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


# ---------------------------------------------------------------------- graph
def _row_sums(x):
    s = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        s = s + x[:, j]
    return s


def fixed_total(x):
    """The sum of a vector in the engine's one shape."""
    x = np.asarray(x, np.float64)
    pad = (-len(x)) % TOTAL_LANES
    m = np.concatenate([x, np.zeros(pad)]).reshape(-1, TOTAL_LANES)
    sh = np.zeros(TOTAL_LANES)
    for r in range(m.shape[0]):
        sh = sh + m[r]
    h = TOTAL_LANES // 2
    while h >= 1:
        sh[:h] = sh[:h] + sh[h:2 * h]
        h //= 2
    return float(sh[0])


def psum_at(dist, rho, mid):
    """Per row: sum_j (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / mid_i) : 1), entry after entry."""
    dist = np.asarray(dist, np.float64)
    s = np.zeros(dist.shape[0])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(dist.shape[1]):
            x = dist[:, j] - rho
            s = s + np.where(x > 0.0, np.exp(-x / mid), 1.0)
    return s


def smooth_knn(dist):
    """(rho, sigma, sigma before its floor, the floor) of a table dist [n, k]."""
    dist = np.asarray(dist, np.float64)
    n, k = dist.shape
    target = np.log2(k + 1.0)
    pos = np.where(dist > 0.0, dist, np.inf)
    rho = pos.min(axis=1)
    rho[~np.isfinite(rho)] = 0.0
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    run = np.ones(n, bool)
    for _ in range(64):
        ps = psum_at(dist, rho, mid)
        run &= ~(np.abs(ps - target) < TOL)
        if not run.any():
            break
        up = run & (ps > target)
        dn = run & ~(ps > target)
        hi[up] = mid[up]
        mid[up] = (lo[up] + hi[up]) / 2.0
        lo[dn] = mid[dn]
        grow = dn & np.isinf(hi)
        half = dn & ~np.isinf(hi)
        mid[grow] = mid[grow] * 2.0
        mid[half] = (lo[half] + hi[half]) / 2.0
    rs = _row_sums(dist)
    mean = np.where(rho > 0.0, rs / float(k), fixed_total(rs) / (float(n) * float(k)))
    floor = FLOOR * mean
    return rho, np.maximum(mid, floor), mid, floor


def directed_weights(dist, rho, sigma):
    dist = np.asarray(dist, np.float64)
    x = dist - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where((x <= 0.0) | (sigma[:, None] == 0.0), 1.0, np.exp(-x / sigma[:, None]))


def union_csr(idx, w, mix=1.0):
    """The symmetric CSR of the directed weights w [n, k] on the table idx."""
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.reshape(-1)
    a = np.asarray(w, np.float64).reshape(-1)
    keep = j != i
    i, j, a = i[keep], j[keep], a[keep]
    key = i * n + j
    order = np.argsort(key, kind="stable")
    skey, sw = key[order], a[order]
    assert np.all(np.diff(skey) > 0), "an index is listed twice in a row"
    pos = np.minimum(np.searchsorted(skey, j * n + i), max(len(skey) - 1, 0))
    has = skey[pos] == j * n + i if len(skey) else np.zeros(0, bool)
    b = np.where(has, sw[pos], 0.0) if len(skey) else np.zeros(0)
    prod = a * b
    val = mix * ((a + b) - prod) + (1.0 - mix) * prod
    if mix == 0.0:
        r, c, v = i[has], j[has], val[has]
    else:
        r = np.concatenate([i, j[~has]])
        c = np.concatenate([j, i[~has]])
        v = np.concatenate([val, val[~has]])
    o = np.lexsort((c, r))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    return indptr, c[o].astype(np.int32), v[o]


def fuzzy_graph(idx, dist, mix=1.0):
    """(indptr, cols, vals, rho, sigma) of a k-NN table."""
    rho, sigma, _, _ = smooth_knn(dist)
    indptr, cols, vals = union_csr(idx, directed_weights(dist, rho, sigma), mix)
    return indptr, cols, vals, rho, sigma


# --------------------------------------------------------------------- layout
def draw(seed, ctr, n):
    """The vertex a draw picks: ((mix64(seed + C ctr) >> 32) n) >> 32 on uint64 arrays."""
    ctr = np.asarray(ctr, np.uint64)
    with np.errstate(over="ignore"):
        z = np.full(ctr.shape, int(seed) & 0xFFFFFFFFFFFFFFFF, np.uint64) + GOLDEN * ctr
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def counters(e, nnz, slot, s):
    """ctr = ((e nnz + slot) << 16) + s (mod 2^64)."""
    with np.errstate(over="ignore"):
        base = np.full(np.shape(slot), e, np.uint64) * np.uint64(nnz) + np.asarray(slot, np.uint64)
        return (base << np.uint64(16)) + np.asarray(s, np.uint64)


def _sq(d):
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def layout(indptr, cols, vals, init, n_epochs=200, a=0.0, b=0.0, gamma=1.0, nsr=5, lr=1.0, seed=0,
           dtype=np.float64, stats=None):
    """Y [n, 2] after n_epochs epochs.  stats: a dict that receives the counted
    attractions and draws."""
    if a == 0.0 and b == 0.0:
        a, b = A_DEFAULT, B_DEFAULT
    indptr = np.asarray(indptr, np.int64)
    n, nnz = len(indptr) - 1, int(indptr[-1])
    cols = np.asarray(cols, np.int64)[:nnz]
    w = np.asarray(vals, np.float64)[:nnz]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    T = dtype
    a_, b_, g_ = T(a), T(b), T(gamma)
    wmax = float(w.max()) if nnz else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        act = (w > 0.0) & ~(w < wmax / float(n_epochs))
        per = wmax / w
        epn = per / float(nsr)
    nxt = np.where(act, per, np.inf)
    nneg = np.where(act, epn, np.inf)
    Y = np.array(init, dtype=T)
    n_att = n_draw = 0
    for e in range(1, n_epochs + 1):
        alpha = lr * (1.0 - float(e - 1) / float(n_epochs))
        ed = float(e)
        on = np.nonzero(nxt <= ed)[0]
        S = np.zeros((n, 2), T)
        if len(on):
            i, j = rows[on], cols[on]
            d = Y[i] - Y[j]
            d2 = _sq(d)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                c = np.where(d2 > 0, (T(-2.0) * a_ * b_ * np.power(d2, b_ - T(1.0))) / (a_ * np.power(d2, b_) + T(1.0)),
                             T(0.0))
                mv_att = np.clip(c[:, None] * d, -4.0, 4.0)
            if nsr > 0:
                mf = np.floor((ed - nneg[on]) / epn[on])
                mf = np.where(mf > 0.0, np.minimum(mf, 65535.0), 0.0)
            else:
                mf = np.zeros(len(on))
            m = mf.astype(np.int64)
            tot = int(m.sum())
            which = np.repeat(np.arange(len(on)), m)  # position in `on` of each draw
            s = np.arange(tot) - np.repeat(np.cumsum(m) - m, m)
            v = draw(seed, counters(e, nnz, on[which], s), n)
            iv = i[which]
            d = Y[iv] - Y[v]
            d2 = _sq(d)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                c = (T(2.0) * g_ * b_) / ((T(0.001) + d2) * (a_ * np.power(d2, b_) + T(1.0)))
                mv_neg = np.clip(c[:, None] * d, -4.0, 4.0)
            mv_neg[d2 == 0] = 4.0
            mv_neg[v == iv] = 0.0  # a draw of the vertex itself is skipped (x + 0 is x)
            # slot order; inside a slot the attraction, then s = 0, 1, ...
            major = np.concatenate([np.arange(len(on)), which])
            minor = np.concatenate([np.zeros(len(on), np.int64), 1 + s])
            order = np.lexsort((minor, major))
            tgt = np.concatenate([i, iv])[order]
            mv = np.concatenate([mv_att, mv_neg])[order]
            if T is np.float64:  # (bincount adds in input order, as add.at does, and is quicker)
                S[:, 0] = np.bincount(tgt, weights=mv[:, 0], minlength=n)
                S[:, 1] = np.bincount(tgt, weights=mv[:, 1], minlength=n)
            else:
                np.add.at(S[:, 0], tgt, mv[:, 0])
                np.add.at(S[:, 1], tgt, mv[:, 1])
            if nsr > 0:
                nneg[on] = nneg[on] + mf * epn[on]
            nxt[on] = nxt[on] + per[on]
            n_att += len(on)
            n_draw += tot
        Y = Y + T(alpha) * S
    if stats is not None:
        stats["attractions"], stats["draws"] = n_att, n_draw
    return Y


def schedule_counts(indptr, vals, n_epochs=200, nsr=5):
    """(attractions, draws) of a layout run: the schedule alone, no positions (it does not depend on them)."""
    nnz = int(np.asarray(indptr)[-1])
    w = np.asarray(vals, np.float64)[:nnz]
    wmax = float(w.max()) if nnz else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        act = (w > 0.0) & ~(w < wmax / float(n_epochs))
        per = (wmax / w)[act]
        epn = per / float(nsr)
    nxt, nneg = per.copy(), epn.copy()
    n_att = n_draw = 0
    for e in range(1, n_epochs + 1):
        on = nxt <= float(e)
        if nsr > 0:
            mf = np.floor((float(e) - nneg[on]) / epn[on])
            mf = np.where(mf > 0.0, np.minimum(mf, 65535.0), 0.0)
            nneg[on] = nneg[on] + mf * epn[on]
            n_draw += int(mf.sum())
        nxt[on] = nxt[on] + per[on]
        n_att += int(on.sum())
    return n_att, n_draw


# ------------------------------------------------------------ data and scores
def blobs(n, dim=8, n_blobs=6, seed=0, scale=10.0):
    """(points [n, dim], labels) of well separated Gaussian blobs."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=scale, size=(n_blobs, dim))
    lab = np.arange(n) % n_blobs
    return centers[lab] + rng.normal(size=(n, dim)), lab


def knn_table(x, k):
    """The exact table of points x in the engine's order (distance, index), the point itself left out."""
    x = np.asarray(x, np.float64)
    g = (x * x).sum(axis=1)
    D = np.sqrt(np.maximum(g[:, None] + g[None, :] - 2.0 * (x @ x.T), 0.0))
    n = len(x)
    np.fill_diagonal(D, -1.0)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), D), axis=1)[:, 1:k + 1]
    return order.astype(np.int32), np.take_along_axis(D, order, axis=1)


def hub_table(n=300, k=4):
    """A hand-made table in which every row lists vertex 0 first: row 0 of the union holds n - 1 entries."""
    idx = np.empty((n, k), np.int32)
    dist = np.empty((n, k))
    for i in range(n):
        idx[i] = [0] + [1 + (i + t) % (n - 1) for t in range(k - 1)] if i else np.arange(1, k + 1)
        dist[i] = 1.0 + np.arange(k) + 0.001 * i
    return idx, dist


def pca_init(x):
    """The first two principal components, the largest absolute coordinate scaled to 10."""
    xc = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    y = u[:, :2] * s[:2]
    return y * (10.0 / np.abs(y).max())


def label_purity(y, lab, k=15):
    """The share of every point's k nearest neighbours in y that carry its label."""
    idx, _ = knn_table(y, k)
    return float(np.mean(lab[idx] == lab[:, None]))
