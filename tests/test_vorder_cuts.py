"""The bucket cuts of the dataset's value order (tests/vorder_model.py states
the rule of scc_vorder.hip's k_vord_cuts): on sorted arrays with ties every
bucket holds at most 64 entries unless it is one tie group, no group is
divided, the buckets tile the segment, and S, E, X and F summed over the
buckets plus the cross term equal brute force over all pairs."""
import numpy as np
import pytest

import vorder_model as vm


def _arrays():
    rng = np.random.default_rng(11)
    out = []
    for n, nval in [(1, 1), (2, 1), (63, 5), (64, 1), (64, 64), (65, 1), (65, 3), (128, 2), (129, 40), (300, 1),
                    (500, 7), (700, 200), (1000, 30)]:
        out.append(np.sort(rng.integers(0, nval, n)).astype(np.float64))
    # a group that would straddle position 64; groups of exactly 64 and 65; singles around them
    out.append(np.repeat([1.0, 2.0, 3.0], [60, 10, 5]))
    out.append(np.repeat([1.0, 2.0, 3.0, 4.0], [1, 64, 1, 65]))
    out.append(np.repeat([-2.0, -1.0, 0.5, 7.0, 9.0], [64, 64, 65, 63, 2]))
    out.append(np.repeat(np.arange(40.0), rng.integers(1, 90, 40)))
    return out


@pytest.mark.parametrize("v", _arrays(), ids=lambda v: f"n{len(v)}u{len(np.unique(v))}")
def test_cut_rule(v):
    bk = vm.cuts(v)
    assert bk[0][0] == 0 and bk[-1][1] == len(v)
    for (s, e, fat), nxt in zip(bk, bk[1:] + [None]):
        assert e > s
        if nxt is not None:
            assert nxt[0] == e                      # the buckets tile the segment
            assert v[e] != v[e - 1]                 # no tie group is divided
        one_group = v[s] == v[e - 1]
        assert (e - s <= vm.WIDTH) or one_group     # at most 64 entries unless one group
        assert fat == (e - s > vm.WIDTH)
        if fat:
            assert one_group
        # greedy: the bucket could not have taken the next group too
        if nxt is not None and not fat:
            e2 = nxt[0] + int(np.searchsorted(v[nxt[0]:], v[nxt[0]], side="right"))
            assert e2 - s > vm.WIDTH


@pytest.mark.parametrize("K,unkept", [(2, False), (6, False), (12, True), (16, True)])
def test_sums_equal_brute_force(K, unkept):
    rng = np.random.default_rng(100 + K)
    for v in _arrays():
        c = rng.integers(0, K, len(v))
        if unkept:
            c[rng.random(len(v)) < 0.2] = -1
        if len(v) > 70:
            c[64:70] = np.arange(6) % 2  # a stretch whose cells alternate between two clusters
        got = vm.bucket_sums(v, c, K, vm.cuts(v))
        want = vm.brute_sums(v, c, K)
        for name, g, w in zip("SEXF", got, want):
            np.testing.assert_array_equal(g, w, err_msg=name)
