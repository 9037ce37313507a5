"""CPU: the one-vs-rest statistics (scc_de_markers) in numpy against the oracle.

The model (tests/markers_reference.py) states the integer statistics twice: as
the issue's S_a, E_a, T with the zero group in closed form, and as the rank-sum
accumulator the kernel keeps, found by binary searches over sorted chunks.
Both are checked against the binary-code oracle (R's wilcox.test on cluster a
vs the rest) and a brute-force O(n^2) count."""
import numpy as np
import pytest

import markers_reference as MR
import oracle as O


def _genes(seed=3, N=260, K=5):
    """Genes with negatives, exact ties, implicit zeros and excluded cells."""
    rng = np.random.default_rng(seed)
    code = rng.integers(-1, K, N).astype(np.int32)  # -1: excluded cells
    X = np.zeros((8, N))
    X[0] = np.where(rng.random(N) < 0.5, rng.gamma(2.0, 1.0, N), 0.0)                      # sparse, tie-free
    X[1] = np.where(rng.random(N) < 0.8, np.round(rng.gamma(2.0, 1.0, N), 1), 0.0)         # heavy ties
    X[2] = rng.choice([-2.0, -1.0, 0.0, 0.0, 1.0, 1.0, 3.5], N)                            # negatives, few levels
    X[3] = rng.normal(0.0, 1.0, N)                                                         # no zeros at all
    X[4] = np.where(code == 2, 0.0, rng.gamma(1.0, 1.0, N))                                # one cluster all zero
    X[5] = 1.25                                                                            # every cell equal
    X[6] = 0.0                                                                             # every cell zero
    X[7] = np.where(rng.random(N) < 0.3, -rng.gamma(2.0, 1.0, N), np.round(rng.random(N), 2))
    return X, code, K


@pytest.mark.parametrize("chunk", [None, 64, 7])
def test_model_matches_oracle_and_brute_force(chunk):
    X, code, K = _genes()
    sel = code >= 0
    for g in range(X.shape[0]):
        u2_issue, u2_kernel, T = MR.model_gene(X[g], code, K, chunk=chunk)
        u2_brute, T_brute = MR.brute_gene(X[g], code, K)
        np.testing.assert_array_equal(u2_issue, u2_brute, err_msg=f"gene {g}: S_a / E_a form")
        np.testing.assert_array_equal(u2_kernel, u2_brute, err_msg=f"gene {g}: rank-sum form")
        assert T == T_brute, g
        for a in range(K):
            _, W, To, _ = O.wilcox_test(X[g, code == a], X[g, sel & (code != a)])
            assert u2_kernel[a] == int(round(2 * W)), (g, a)
            assert T == int(round(To)), (g, a)


def test_additivity_over_pairs():
    """2U_a = sum over b != a of 2U_ab (R's W of a vs b), exactly."""
    X, code, K = _genes(seed=8)
    sel = code >= 0
    for g in range(X.shape[0]):
        for a in range(K):
            tot = 0
            for b in range(K):
                if b != a:
                    tot += int(round(2 * O.wilcox_test(X[g, code == a], X[g, code == b])[1]))
            W = O.wilcox_test(X[g, code == a], X[g, sel & (code != a)])[1]
            assert tot == int(round(2 * W)), (g, a)


def test_tie_term_is_not_a_sum_of_pair_terms():
    """T of 'a vs rest' holds triple products of cluster counts: three clusters
    sharing one value give 3^3 - 3 = 24, the three pair terms 6 each."""
    x = np.array([1.0, 1.0, 1.0])
    code = np.array([0, 1, 2], np.int32)
    _, _, T = MR.model_gene(x, code, 3)
    assert T == 24
    assert sum(int(O.wilcox_test(x[code == a], x[code == b])[2]) for a in range(3) for b in range(a + 1, 3)) == 18


def test_only_pos_bh_restatement_hand_checked():
    """BH over the surviving rows in order: p = (0.01, 0.02, 0.03, 0.5) with
    n = 4 gives q = (0.04, 0.04, 0.04, 0.5); dropping the second row (negative
    avg_logFC) gives n = 3 and q = (0.03, 0.045, 0.5)."""
    p = np.array([0.01, 0.02, 0.03, 0.5])
    np.testing.assert_allclose(O.p_adjust_bh(p), [0.04, 0.04, 0.04, 0.5], rtol=1e-15)
    lfc = np.array([1.0, -2.0, 0.7, 0.6])
    np.testing.assert_allclose(O.p_adjust_bh(p[lfc > 0]), [0.03, 0.045, 0.5], rtol=1e-15)


def test_reference_loop_only_pos_is_a_row_subset():
    """reference(only_pos=True) keeps exactly the default rows with avg_logFC > 0,
    in their order, with BH restated over them."""
    from scconsensus_amd import api, synth
    d = synth.generate("A", G=300, N=600, K=4, seed=2)
    names, code = api.select_clusters(d.labels, 10)
    X = d.dense()
    K = len(names)
    full = MR.reference(X, code, K, log_fc_thrs=0.25, min_per_cent=10.0)
    pos = MR.reference(X, code, K, log_fc_thrs=0.25, min_per_cent=10.0, only_pos=True)
    keep = full.lfc > 0
    np.testing.assert_array_equal(pos.gene, full.gene[keep])
    np.testing.assert_array_equal(pos.u2, full.u2[keep])
    assert pos.tested.sum() == keep.sum() and 0 < keep.sum() < len(keep)
    starts = np.concatenate([[0], np.cumsum(pos.tested)])
    for a in range(K):
        s, e = starts[a], starts[a + 1]
        np.testing.assert_allclose(pos.q[s:e], O.p_adjust_bh(pos.p[s:e]), rtol=1e-15)
    assert set(pos.union) <= set(pos.gene[pos.top])
