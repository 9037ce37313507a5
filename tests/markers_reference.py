"""One-vs-rest marker reference for the scc_de_markers tests (test
infrastructure only; imports the oracle).

* ``reference`` -- the reference result: for every cluster a one binary-code
  oracle run ``O.de_fast(X, where(code < 0, -1, where(code == a, 0, 1)), 2)``,
  whose "pair" 0 is ComputePairWiseDE(cells.1 = a, cells.2 = the rest) with
  the caller's rules.  ``only_pos`` keeps the rows with avg_logFC > 0 (the
  tested set of avg_logFC > thr, thr >= 0) and restates BH, the kept / top
  flags and the union over the surviving rows, in the manner of
  ``parity_helpers.check_selection``.
* ``check_margins`` -- a fixture is valid only if no oracle filter decision
  sits within 1e-9 of its threshold.
* ``model_gene`` -- a numpy model of the engine's integer statistics (the
  issue's S_a, E_a, T and the zero group, and the rank-sum form the kernel
  accumulates), and ``brute_gene``, the O(n^2) count they are checked against.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import oracle as O


@dataclass
class MarkerRows:
    tested: np.ndarray   # [K] rows per cluster
    gene: np.ndarray
    p: np.ndarray
    q: np.ndarray
    lfc: np.ndarray
    pct1: np.ndarray
    pct2: np.ndarray
    u2: np.ndarray       # int64 2W
    ties: np.ndarray     # int64
    de: np.ndarray
    top: np.ndarray
    union: np.ndarray
    margin: float        # the smallest |quantity - threshold| over the oracle's filter decisions seen


def binary_code(code, a):
    code = np.asarray(code)
    return np.where(code < 0, -1, np.where(code == a, 0, 1)).astype(np.int32)


def reference(X, code, K, q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, only_pos=False):
    parts = []
    margin = np.inf
    for a in range(K):
        o = O.de_fast(X, binary_code(code, a), 2, q_val_thrs=q_val_thrs, log_fc_thrs=log_fc_thrs,
                      min_per_cent=min_per_cent, top_n=top_n)
        assert o.status == 0, f"cluster {a}: oracle status {o.status}"
        g, p, q, lfc = o.row_gene, o.row_p, o.row_q, o.row_lfc
        pct1, pct2, W, T, de, top = o.row_pct1, o.row_pct2, o.row_W, o.row_ties, o.row_de, o.row_top
        if len(g):
            margin = min(margin, float(np.min(np.abs(np.abs(lfc) - log_fc_thrs))),
                         float(np.min(np.abs(np.maximum(pct1, pct2) - min_per_cent))))
        if only_pos:
            keep = lfc > 0
            g, p, lfc, pct1, pct2, W, T = g[keep], p[keep], lfc[keep], pct1[keep], pct2[keep], W[keep], T[keep]
            q = O.p_adjust_bh(p) if len(p) else p.copy()
            de = (len(g) > 1) & (q < q_val_thrs)
            w = np.abs(lfc)
            above = (w[de][None, :] > w[:, None]).sum(axis=1)
            top = de & (above + 1 <= top_n)
        parts.append((g, p, q, lfc, pct1, pct2, np.round(2 * W).astype(np.int64), np.round(T).astype(np.int64),
                      np.asarray(de, bool), np.asarray(top, bool)))
    cat = [np.concatenate([pt[k] for pt in parts]) for k in range(10)]
    tested = np.array([len(pt[0]) for pt in parts], np.int32)
    top_genes = cat[0][cat[9]]
    _, first = np.unique(top_genes, return_index=True)
    union = top_genes[np.sort(first)].astype(np.int32)
    return MarkerRows(tested, *cat, union, margin)


def all_cells_margin(X, code, K, log_fc_thrs):
    """The smallest distance of ANY (cluster, gene) cell's |avg_logFC| from its
    threshold, dropped cells included (numpy restatement of Fast:259-286; its
    rounding, ~1e-15, is far below the 1e-9 the margin is compared with).  The
    pct filter needs no such margin for dropped cells: 100 * count / n is the
    same expression of the same integers on both sides (pct is compared bit for
    bit), so a cell at exactly min_per_cent is dropped by both."""
    X = np.asarray(X, np.float64)
    code = np.asarray(code)
    sel = code >= 0
    margin = np.inf
    for a in range(K):
        A, R = X[:, code == a], X[:, sel & (code != a)]
        lfc = np.log(np.expm1(A).mean(1) + 1.0) - np.log(np.expm1(R).mean(1) + 1.0)
        margin = min(margin, float(np.min(np.abs(np.abs(lfc) - log_fc_thrs))))
    return margin


def check_margins(ref, X, code, K, log_fc_thrs=0.5, min_per_cent=20.0):
    """A fixture is valid only if the oracle's own |avg_logFC| - threshold and
    pct - min_per_cent margins exceed 1e-9 (``ref.margin``: the oracle's tested
    rows), and no dropped cell's avg_logFC sits that close either."""
    assert ref.margin > 1e-9, f"a tested row sits {ref.margin:.3g} from a filter threshold: pick another seed"
    m = all_cells_margin(X, code, K, log_fc_thrs)
    assert m > 1e-9, f"a (cluster, gene) cell sits {m:.3g} from the avg_logFC threshold: pick another seed"
    return min(m, ref.margin)


def compare(g, ref, p_rtol=1e-6, lfc_rtol=1e-12, lfc_atol=5e-14):
    """Engine result (``Engine.de_markers``) against ``reference``: the project's bar."""
    r = g.rows
    np.testing.assert_array_equal(r.pair_tested, ref.tested)
    np.testing.assert_array_equal(r.gene, ref.gene)
    np.testing.assert_array_equal(r.u2, ref.u2)
    np.testing.assert_array_equal(r.ties, ref.ties)
    np.testing.assert_array_equal(r.pct1, ref.pct1)
    np.testing.assert_array_equal(r.pct2, ref.pct2)
    np.testing.assert_allclose(r.p, ref.p, rtol=p_rtol, atol=0)
    np.testing.assert_allclose(r.q, ref.q, rtol=p_rtol, atol=0)
    np.testing.assert_allclose(r.avg_logfc, ref.lfc, rtol=lfc_rtol, atol=lfc_atol)
    np.testing.assert_array_equal(r.de, ref.de)
    np.testing.assert_array_equal(r.top, ref.top)
    np.testing.assert_array_equal(g.union, ref.union)


# ------------------------------------------------------------------ the integer statistics
def brute_gene(x, code, K):
    """O(n^2): 2U_a = 2 #{i in a, j in rest: x_j < x_i} + #{x_j == x_i} over all
    selected cells (zeros included), and T = sum(NTIES^3 - NTIES)."""
    x = np.asarray(x, np.float64)
    code = np.asarray(code)
    sel = code >= 0
    xs, cs = x[sel], code[sel]
    u2 = np.zeros(K, np.int64)
    for a in range(K):
        xa, xr = xs[cs == a], xs[cs != a]
        u2[a] = 2 * int((xa[:, None] > xr[None, :]).sum()) + int((xa[:, None] == xr[None, :]).sum())
    _, cnt = np.unique(xs, return_counts=True)
    cnt = cnt.astype(np.int64)
    return u2, int((cnt ** 3 - cnt).sum())


def model_gene(x, code, K, chunk=None):
    """The engine's bucketed formulas on one gene.  Returns (u2_issue, u2_kernel, T):
    u2_issue from S_a, E_a and the zero group as the issue states them;
    u2_kernel from the rank-sum accumulator R2_a = sum_{i in a}(2 below(i) + n_t(i))
    the kernel keeps (2 S_a + E_a = R2_a - nz_a^2), with below / n_t found the
    kernel's way for a bucket beyond its LDS capacity: binary searches over
    sorted chunks of ``chunk`` elements."""
    x = np.asarray(x, np.float64)
    code = np.asarray(code)
    sel = code >= 0
    xs, cs = x[sel], code[sel].astype(np.int64)
    n_clu = np.bincount(cs, minlength=K).astype(np.int64)
    nzm = xs != 0
    v, c = xs[nzm], cs[nzm]
    pos = np.bincount(cs[xs > 0], minlength=K).astype(np.int64)
    neg = np.bincount(cs[xs < 0], minlength=K).astype(np.int64)
    z = n_clu - pos - neg
    Z = int(z.sum())
    # --- the issue's statistics from tie groups of the sorted nonzeros
    order = np.argsort(v, kind="stable")
    sv, sc = v[order], c[order]
    S = np.zeros(K, np.int64)
    E = np.zeros(K, np.int64)
    T = 0
    below_own = np.zeros(K, np.int64)
    i = 0
    while i < len(sv):
        e = i
        while e < len(sv) and sv[e] == sv[i]:
            e += 1
        ct = np.bincount(sc[i:e], minlength=K).astype(np.int64)
        nt = int(ct.sum())
        S += ct * (i - below_own)        # all elements below minus own-cluster elements below
        E += ct * (nt - ct)
        T += nt ** 3 - nt
        below_own += ct
        i = e
    T += Z ** 3 - Z
    neg_rest, z_rest = neg.sum() - neg, Z - z
    u2_issue = 2 * (S + z * neg_rest + pos * z_rest) + z * z_rest + E
    # --- the kernel's accumulator, by searches over sorted chunks
    n = len(v)
    chunk = chunk or max(n, 1)
    chunks = [np.sort(v[s:s + chunk]) for s in range(0, n, chunk)]
    lo = sum(np.searchsorted(ch, v, side="left") for ch in chunks) if chunks else np.zeros(0, np.int64)
    hi = sum(np.searchsorted(ch, v, side="right") for ch in chunks) if chunks else np.zeros(0, np.int64)
    nt = (hi - lo).astype(np.int64)
    R2 = np.zeros(K, np.int64)
    np.add.at(R2, c, 2 * lo.astype(np.int64) + nt)
    Tk = int((nt * nt - 1).sum()) + Z ** 3 - Z
    assert Tk == T
    nz = pos + neg
    u2_kernel = R2 - nz * nz + 2 * (z * neg_rest + pos * z_rest) + z * z_rest
    return u2_issue, u2_kernel, T
