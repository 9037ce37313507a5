"""Numpy statement of the value order's bucket cuts (scconsensus_amd/csrc/
scc_vorder.hip, k_vord_cuts) and of the sums the rank stage takes over them
(k_rank_mfma16<1, true> in scc_rank_waves.hip and k_rank_cross in
scc_rank_cross.hip).  Test code only.

A gene's stored values are in ascending order (equal values in cell order).
From a bucket's start s the candidates for its end are the positions e in
(s, s + 64] that start a group of equal values, or the segment's end; the last
one is taken.  Where there is none the group at s is longer than 64 entries,
and the bucket is that whole group (a "fat" bucket)."""
import numpy as np

WIDTH = 64


def f(c):
    c = np.asarray(c, dtype=np.int64)
    return c * c * c - c


def cuts(v):
    """[(start, end, fat)] over the sorted values v."""
    v = np.asarray(v)
    n = len(v)
    start = np.ones(n + 1, bool)  # position n: the segment's end
    start[1:n] = v[1:] != v[:-1]
    out = []
    s = 0
    while s < n:
        cand = np.flatnonzero(start[s + 1:min(s + WIDTH, n) + 1])
        if len(cand):
            e, fat = s + 1 + int(cand[-1]), False
        else:
            e, fat = s + 1 + WIDTH + int(np.flatnonzero(start[s + 1 + WIDTH:])[0]), True
        out.append((s, e, fat))
        s = e
    return out


def bucket_sums(v, c, K, bk):
    """S, E, X [K][K] and F [K] as the rank stage forms them: per bucket the
    pairs inside it (codes in order inside a tie group, unkept entries, code
    < 0, dropped), then the cross term from the buckets' cluster histograms."""
    v, c = np.asarray(v), np.asarray(c, np.int64)
    S = np.zeros((K, K), np.int64)
    E = np.zeros((K, K), np.int64)
    X = np.zeros((K, K), np.int64)
    F = np.zeros(K, np.int64)
    hb = np.zeros((len(bk), K), np.int64)
    for q, (s, e, fat) in enumerate(bk):
        keep = c[s:e] >= 0
        vv, cc = v[s:e][keep], c[s:e][keep]
        hb[q] = np.bincount(cc, minlength=K)
        if fat:  # one repeated value: the closed form over the histogram
            assert len(np.unique(v[s:e])) == 1
            h = hb[q]
            F += np.where(h >= 2, f(h), 0)
            E += np.outer(h, h)
            X += np.outer(h, h) * (h[:, None] + h[None, :])
            continue
        o = np.lexsort((cc, vv))
        vv, cc = vv[o], cc[o]
        seen = np.zeros(K, np.int64)
        i = 0
        while i < len(vv):
            j = i
            while j < len(vv) and vv[j] == vv[i]:
                j += 1
            h = np.bincount(cc[i:j], minlength=K)
            S += np.outer(h, seen)  # x in a above every earlier y in b
            seen += h
            if j - i >= 2:
                F += np.where(h >= 2, f(h), 0)
                E += np.outer(h, h)
                X += np.outer(h, h) * (h[:, None] + h[None, :])
            i = j
    below = np.cumsum(hb, axis=0) - hb  # elements of each cluster in earlier buckets
    S += hb.T @ below
    for M in (E, X):
        np.fill_diagonal(M, 0)
    np.fill_diagonal(S, 0)
    return S, E, X, F


def brute_sums(v, c, K):
    """The same sums over all pairs of kept entries."""
    v, c = np.asarray(v), np.asarray(c, np.int64)
    keep = c >= 0
    v, c = v[keep], c[keep]
    gt = (v[:, None] > v[None, :]).astype(np.int64)
    eq = (v[:, None] == v[None, :]).astype(np.int64)
    oh = (c[:, None] == np.arange(K)[None, :]).astype(np.int64)
    S = oh.T @ gt @ oh
    E = oh.T @ eq @ oh
    X = np.zeros((K, K), np.int64)
    F = np.zeros(K, np.int64)
    for x in np.unique(v):
        h = np.bincount(c[v == x], minlength=K)
        X += np.outer(h, h) * (h[:, None] + h[None, :])
        F += np.where(h >= 2, f(h), 0)
    for M in (S, E, X):
        np.fill_diagonal(M, 0)
    return S, E, X, F
