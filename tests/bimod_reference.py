"""TEST INFRASTRUCTURE ONLY -- the FAST "bimod" test restated from the cells.

``test.use = "bimod"`` is McDavid's zero-inflated likelihood-ratio test as the
reference runs it (bimodLikData / DifferentialLRT / DiffExpTest,
R/reclusterDEConsensusFast.R:93-133).  This module restates it per (pair, gene)
directly from the cell values, the way the R code does: numpy ``longdouble``,
R's two-pass ``mean`` and ``sd``, a literal per-value ``dnorm(..., log = TRUE)``
sum, and ``scipy.stats.chi2.sf`` for the tail.  It uses neither moments nor the
closed form of the sum nor a closed-form tail, so it shares no structure with
the engine (which works from per-(gene, cluster) moments).

The feature filters (which cells a pair tests), avg_logFC and pct.1 / pct.2 do
not depend on the test: they come from the oracle run as ``wilcox``.  The
selection (R's ``order(p, -avg_logFC)``, BH, the ``> 1 row`` rule, ``top_n``,
``unique``; Fast:346-392) is restated here on the reference p.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.stats import chi2

import oracle as O

LD = np.longdouble
_LOG_SQRT_2PI = np.log(np.sqrt(2 * LD(np.pi)))


def r_mean(x) -> float:
    """R's mean(): long-double sum / n, then one refinement pass; a double."""
    x = np.asarray(x, LD)
    n = LD(len(x))
    s = x.sum() / n
    s = s + (x - s).sum() / n
    return float(s)


def r_sd(x) -> float:
    """R's sd(): two-pass, divisor n - 1, long-double accumulation; a double."""
    x = np.asarray(x, LD)
    m = LD(r_mean(x))
    return float(np.sqrt(((x - m) ** 2).sum() / LD(len(x) - 1)))


def dnorm_log(x, mu, sd):
    """R's dnorm(x, mu, sd, log = TRUE) per value (nmath/dnorm.c): sd = 0 gives
    +Inf at x == mu and -Inf elsewhere."""
    x = np.asarray(x, LD)
    if sd == 0.0:
        return np.where(x == LD(mu), LD(np.inf), LD(-np.inf))
    z = (x - LD(mu)) / LD(sd)
    return -(_LOG_SQRT_2PI + LD(0.5) * z * z + np.log(LD(sd)))


def lik(x) -> np.longdouble:
    """bimodLikData(x) (Fast:93-111)."""
    x = np.asarray(x, np.float64)
    x2 = x[x > 0]
    n, n2 = len(x), len(x2)
    xal = min(max(n2 / n, 1e-5), 1 - 1e-5)  # MinMax(), doubles as in R
    lik_a = LD(n - n2) * np.log(LD(1 - xal))
    sd = 1.0 if n2 < 2 else r_sd(x2)
    gauss = dnorm_log(x2, r_mean(x2), sd).sum() if n2 else LD(0)
    with np.errstate(invalid="ignore"):
        return lik_a + (LD(n2) * np.log(LD(xal)) + gauss)


def lrt(x, y) -> float:
    """DifferentialLRT's statistic (Fast:113-116); Inf - Inf is NaN as in R."""
    with np.errstate(invalid="ignore"):
        return float(2 * (lik(x) + lik(y) - lik(np.concatenate([x, y]))))


def p_value(x, y) -> float:
    """pchisq(lrt, df = 3, lower.tail = FALSE) (Fast:117)."""
    return float(chi2.sf(lrt(x, y), 3))


def pair_list(K):
    return [(i, j) for i in range(K - 1) for j in range(i + 1, K)]


@dataclass
class BimodResult:
    pair_tested: np.ndarray  # [P]
    gene: list               # per pair: tested genes, ascending gene row
    p: list                  # per pair: reference p of those genes
    lfc: list
    pct1: list
    pct2: list
    q: list                  # per pair: BH q (of the rows in gene order)
    de: list                 # per pair: kept rows
    top: list
    union: np.ndarray


def de_bimod(X, code, K, q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, sample=None) -> BimodResult:
    """The FAST DE stage with test.use = "bimod", per pair in gene order.
    ``sample`` (a boolean mask over the oracle's rows, pair-major in the
    oracle's order) limits the p computation to those rows (others NaN; the
    selection fields are then meaningless and left empty)."""
    X = np.asarray(X, np.float64)
    code = np.asarray(code)
    o = O.de_fast(X, code, K, q_val_thrs=q_val_thrs, log_fc_thrs=log_fc_thrs, min_per_cent=min_per_cent,
                  top_n=top_n)
    cells = [np.flatnonzero(code == a) for a in range(K)]
    starts = np.concatenate([[0], np.cumsum(o.pair_tested)]).astype(np.int64)
    res = BimodResult(o.pair_tested.copy(), [], [], [], [], [], [], [], [], np.zeros(0, np.int32))
    top_rows = []
    for k, (i, j) in enumerate(pair_list(K)):
        a, b = int(starts[k]), int(starts[k + 1])
        sel = np.arange(a, b)
        order = np.argsort(o.row_gene[sel], kind="stable")
        sel = sel[order]
        g = o.row_gene[sel]
        p = np.full(len(g), np.nan)
        for r, (row, gene) in enumerate(zip(sel, g)):
            if sample is None or sample[row]:
                p[r] = p_value(X[gene, cells[i]], X[gene, cells[j]])
        res.gene.append(g)
        res.p.append(p)
        res.lfc.append(o.row_lfc[sel])
        res.pct1.append(o.row_pct1[sel])
        res.pct2.append(o.row_pct2[sel])
        if sample is not None:
            continue
        q = O.p_adjust_bh(p) if len(p) else p.copy()
        de = (len(p) > 1) & (q < q_val_thrs)
        w = np.abs(res.lfc[-1])
        above = (w[de][None, :] > w[:, None]).sum(axis=1)
        top = de & (above + 1 <= top_n)
        res.q.append(q)
        res.de.append(de)
        res.top.append(top)
        # the pair's top list in R's row order: order(p, -avg_logFC), then gene row
        ro = np.lexsort((g, -res.lfc[-1], p))
        top_rows.append(g[ro][top[ro]])
    if sample is None:
        tg = np.concatenate(top_rows) if top_rows else np.zeros(0, np.int32)
        _, first = np.unique(tg, return_index=True)
        res.union = tg[np.sort(first)].astype(np.int32)
    return res


def degenerate_fixture(with_nan_gene=False, seed=11):
    """The degenerate-case matrix: clusters of 20, 30 and 25 cells
    (cluster-major), one gene per IEEE case of the test.  "Spread" values are
    log1p(gamma(2, 2)) + 0.1.  Returns (X [G][75], code)."""
    rng = np.random.default_rng(seed)
    n = (20, 30, 25)
    code = np.repeat(np.arange(3), n).astype(np.int32)
    lo = np.concatenate([[0], np.cumsum(n)])

    def spread(k):
        return np.log1p(rng.gamma(2.0, 2.0, k)) + 0.1

    X = np.zeros((7 if with_nan_gene else 6, 75))

    def put(g, c, vals):
        vals = np.atleast_1d(np.asarray(vals, np.float64))
        X[g, lo[c]:lo[c] + len(vals)] = vals

    put(0, 0, np.full(10, 2.0)); put(0, 1, spread(12)); put(0, 2, spread(3))      # lrt = +Inf: p = 0
    put(1, 0, spread(1)); put(1, 1, spread(9)); put(1, 2, X[1, lo[0]] + 0.25)     # sd := 1; (0, 2): lrt < 0
    put(2, 1, spread(15)); put(2, 2, spread(2))                                    # n2 = 0 in cluster 0
    put(3, 0, np.full(10, 1.0)); put(3, 1, np.full(10, 3.0)); put(3, 2, spread(10))  # every pair p = 0
    put(4, 0, 2.0); put(4, 1, 2.0); put(4, 2, spread(8))                           # (0, 1): lrt = -Inf, p = 1
    X[5] = rng.normal(0.0, 1.0, 75)                                                # negatives: not expressed
    if with_nan_gene:
        put(6, 0, np.full(10, 1.0)); put(6, 1, np.full(10, 1.0))                   # every pair Inf - Inf
    return X, code


# the cells of the degenerate fixture with a known sign: (gene, pair (i, j)) -> p
DEGENERATE_EXACT = {
    (0, (0, 1)): 0.0, (0, (0, 2)): 0.0,
    (1, (0, 2)): 1.0,
    (3, (0, 1)): 0.0, (3, (0, 2)): 0.0, (3, (1, 2)): 0.0,
    (4, (0, 1)): 1.0,
}
