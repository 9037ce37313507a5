"""The bimod reference helper (tests/bimod_reference.py) pinned on the CPU:
its likelihood against scipy.stats.norm.logpdf sums, its tail against
chi2.sf, and R's IEEE cases on the degenerate fixture the GPU test uses."""
import math
import os
import re

import numpy as np
import pytest
from scipy.stats import chi2, norm

import bimod_reference as B
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _zero_inflated(rng, n, frac):
    return np.where(rng.random(n) < frac, np.log1p(rng.gamma(2.0, 2.0, n)) + 0.1, 0.0)


def _lik_scipy(x):
    x2 = x[x > 0]
    n, n2 = len(x), len(x2)
    xal = min(max(n2 / n, 1e-5), 1 - 1e-5)
    sd = 1.0 if n2 < 2 else np.std(x2, ddof=1)
    g = norm.logpdf(x2, np.mean(x2), sd).sum() if n2 else 0.0
    return (n - n2) * math.log(1 - xal) + n2 * math.log(xal) + g


def test_likelihood_and_tail_against_scipy():
    rng = np.random.default_rng(2)
    for _ in range(200):
        nx, ny = rng.integers(3, 60, 2)
        x = _zero_inflated(rng, nx, rng.uniform(0.05, 1.0))
        y = _zero_inflated(rng, ny, rng.uniform(0.05, 1.0))
        if rng.random() < 0.2:
            x[rng.integers(nx)] = -0.5  # a negative value is "not expressed"
        for v in (x, y, np.concatenate([x, y])):
            np.testing.assert_allclose(float(B.lik(v)), _lik_scipy(v), rtol=1e-12, atol=1e-12)
        stat = B.lrt(x, y)
        assert B.p_value(x, y) == chi2.sf(stat, 3)
        want = 2 * (_lik_scipy(x) + _lik_scipy(y) - _lik_scipy(np.concatenate([x, y])))
        np.testing.assert_allclose(stat, want, rtol=0, atol=1e-12 * (1 + abs(_lik_scipy(x)) + abs(_lik_scipy(y))))


def test_r_mean_and_sd():
    rng = np.random.default_rng(3)
    x = rng.gamma(2.0, 2.0, 500)
    np.testing.assert_allclose(B.r_mean(x), O.r_mean(x), rtol=0, atol=0)
    np.testing.assert_allclose(B.r_sd(x), np.std(x, ddof=1), rtol=1e-14)
    assert B.r_sd(np.full(10, 2.0)) == 0.0 and B.r_sd(np.full(3000, 0.1)) == 0.0


def test_ieee_cases_of_the_tail():
    # what pchisq(q, 3, lower.tail = FALSE) gives in R for these q
    assert chi2.sf(np.inf, 3) == 0.0
    assert chi2.sf(-np.inf, 3) == 1.0
    assert chi2.sf(-3.0, 3) == 1.0 and chi2.sf(0.0, 3) == 1.0
    assert np.isnan(chi2.sf(np.nan, 3))
    assert B.dnorm_log([2.0], 2.0, 0.0)[0] == np.inf and B.dnorm_log([2.0], 1.0, 0.0)[0] == -np.inf


def _tested(o, K, gene, pair):
    starts = np.concatenate([[0], np.cumsum(o.pair_tested)])
    k = B.pair_list(K).index(pair)
    return gene in o.row_gene[starts[k]:starts[k + 1]]


def test_degenerate_table():
    """Case (c) of the GPU test: every listed cell is tested, its reference p
    has the stated exact value, the other tested cells are finite."""
    X, code = B.degenerate_fixture()
    kw = dict(min_per_cent=1.0, log_fc_thrs=0.0)
    o = O.de_fast(X, code, 3, **kw)
    r = B.de_bimod(X, code, 3, **kw)
    for (gene, pair), want in B.DEGENERATE_EXACT.items():
        assert _tested(o, 3, gene, pair), (gene, pair)
        k = B.pair_list(3).index(pair)
        assert r.p[k][list(r.gene[k]).index(gene)] == want, (gene, pair)
    allp = np.concatenate(r.p)
    assert len(allp) == 18 and not np.isnan(allp).any()  # 6 genes x 3 pairs, all tested
    assert ((allp > 0) & (allp < 1)).sum() >= 8
    c = [X[:, code == a] for a in range(3)]
    assert B.lrt(c[0][0], c[1][0]) == np.inf and B.lrt(c[0][4], c[1][4]) == -np.inf
    assert B.lrt(c[0][1], c[2][1]) < 0  # the sd := 1 branch on both sides, finite
    # negatives are "not expressed": gene 5's p is the p of its values clipped at 0
    assert (c[0][5] < 0).any() and (c[1][5] < 0).any()
    assert B.p_value(c[0][5], c[1][5]) == B.p_value(np.maximum(c[0][5], 0), np.maximum(c[1][5], 0))


def test_nan_gene_of_the_stop_fixture():
    """Case (d): every pair of g6 is Inf - Inf in the reference and tested at
    log_fc_thrs = 0; at log_fc_thrs = 5 no cell of the matrix is tested."""
    X, code = B.degenerate_fixture(with_nan_gene=True)
    o = O.de_fast(X, code, 3, min_per_cent=1.0, log_fc_thrs=0.0)
    c = [X[6, code == a] for a in range(3)]
    for i, j in B.pair_list(3):
        assert np.isnan(B.lrt(c[i], c[j])) and np.isnan(B.p_value(c[i], c[j]))
        assert _tested(o, 3, 6, (i, j))
    assert O.de_fast(X, code, 3, min_per_cent=1.0, log_fc_thrs=5.0).pair_tested.sum() == 0
    np.testing.assert_array_equal(X[:6], B.degenerate_fixture()[0])


def test_bindings_accept_bimod():
    """The Python layers take "bimod" (SCC_TEST_BIMOD = 2 as in scc.h) and
    still refuse "roc"; no device is touched."""
    from scconsensus_amd import _native as nat
    from scconsensus_amd import api
    hdr = open(os.path.join(ROOT, "include", "scc.h")).read()
    codes = {m[0]: int(m[1]) for m in re.findall(r"#define SCC_TEST_(\w+) (\d+)", hdr)}
    assert codes == {"WILCOX": 0, "T": 1, "BIMOD": 2}
    assert (nat.SCC_TEST_WILCOX, nat.SCC_TEST_T, nat.SCC_TEST_BIMOD) == (0, 1, 2)
    for name, val in (("wilcox", 0), ("t", 1), ("bimod", 2)):
        assert nat.Engine._de_params(nat.SCC_DE_FAST, 0.1, 0.5, 20.0, 30, 1.5, 5.0, False, name).test == val
    with pytest.raises(ValueError):
        nat.Engine._de_params(nat.SCC_DE_FAST, 0.1, 0.5, 20.0, 30, 1.5, 5.0, False, "roc")
    with pytest.raises(NotImplementedError, match="'wilcox', 't' and 'bimod'"):
        api.reclusterDEConsensusFast(np.zeros((2, 4)), ["a", "a", "b", "b"], method="roc")
    r_glue = open(os.path.join(ROOT, "integration", "R", "scConsensusAMD.R")).read()
    assert 'c("wilcox", "t", "bimod")' in r_glue and "match(method, tests) - 1L" in r_glue
