"""The identity behind the rank stage's run rows (tests/rank_runs_model.py): the
cross term over a gene's buckets equals the part inside the runs plus the part
between the runs, for any cut of the buckets into runs; the run rows sit where
k_rank_cross_runs looks for them; and the bounded 32-bit accumulation gives the
same sums whatever the bound."""
import numpy as np
import pytest

import rank_runs_model as rm


def _hist(rng, nb, K, fat=0.0):
    """nb bucket rows: up to 64 elements each, a share of fat tie groups of up to 5000."""
    n = rng.integers(1, 65, nb)
    big = rng.random(nb) < fat
    n[big] = rng.integers(65, 5000, int(big.sum()))
    H = np.array([rng.multinomial(m, rng.dirichlet(np.ones(K))) for m in n], np.int64)
    drop = rng.random(nb) < 0.3  # unkept elements: the row sums to less than the bucket holds
    H[drop, 0] //= 2
    return H, n


@pytest.mark.parametrize("K", [2, 12, 16])
def test_random_cuts(K):
    rng = np.random.default_rng(K)
    for nb in [1, 2, 3, 16, 17, 40, 200]:
        H, _ = _hist(rng, nb, K, fat=0.1)
        want = rm.bucket_cross(H)
        for trial in range(6):
            if trial == 0:
                run = np.zeros(nb, np.int64)          # one run
            elif trial == 1:
                run = np.arange(nb)                   # every run one bucket
            else:
                run = np.cumsum(rng.random(nb) < rng.random()) # random cuts, runs of one bucket among them
            local, between, rows = rm.split_cross(H, run)
            np.testing.assert_array_equal(local + between, want)
            np.testing.assert_array_equal(rows.sum(axis=0), H.sum(axis=0))
            if trial == 0:
                assert not between.any()
            if trial == 1:
                assert not local.any()


@pytest.mark.parametrize("CH", [16, 64, 512])
def test_chunk_runs_and_rows(CH):
    rng = np.random.default_rng(CH)
    K = 12
    cases = [(0, 1), (5, 40), (0, CH), (3, CH), (CH - 1, 2), (CH, CH), (2 * CH - 3, 3), (7, 3 * CH - 7), (CH + 1, 5 * CH)]
    cases += [(int(rng.integers(0, 4 * CH)), int(rng.integers(1, 6 * CH))) for _ in range(20)]
    for bk0, nb in cases:
        H, _ = _hist(rng, nb, K)
        run = rm.run_ids(bk0, nb, CH)
        rows_at = rm.run_rows(bk0, nb, CH)
        # a run per chunk the gene touches, its row at its first slot; rows of different runs never meet
        assert len(rows_at) == run[-1] + 1 == (bk0 + nb - 1) // CH - bk0 // CH + 1
        first = np.array([bk0 + int(np.flatnonzero(run == r)[0]) for r in range(run[-1] + 1)])
        np.testing.assert_array_equal(rows_at, first)
        assert np.all(np.bincount(run) <= CH) and np.all(np.bincount(run)[1:-1] == CH)
        local, between, rows = rm.split_cross(H, run)
        np.testing.assert_array_equal(local + between, rm.bucket_cross(H))
        assert len(rows) == len(rows_at)


def test_chunk_rule():
    assert rm.chunk(0, 2048) == 16 and rm.chunk(200, 2048) == 16
    assert rm.chunk(236_000, 2048) == 16                 # config B: 7 by the division
    assert rm.chunk(16 * 2048 * 100 + 5, 2048) == 100
    assert rm.chunk(1 << 30, 2048) == 512


@pytest.mark.parametrize("blim", [1, 8192, 50_000, 1 << 20, (1 << 31) - 1])
def test_bounded_accumulators(blim):
    rng = np.random.default_rng(5)
    K = 12
    nb, bk0, CH = 70, 9, 16
    H, n = _hist(rng, nb, K)
    H[30], n[30] = rng.multinomial(3000, np.ones(K) / K), 3000  # a fat tie group inside a run
    run = rm.run_ids(bk0, nb, CH)
    got, flushes, peak = rm.bounded_local(H, n, run, blim)
    local, _, _ = rm.split_cross(H, run)
    np.testing.assert_array_equal(got, 2 * local)
    assert peak <= max(blim, 0) or blim < 8192
    if blim <= 50_000:
        assert flushes > 0     # the bound was passed inside a run
    if blim == (1 << 31) - 1:
        assert flushes == 0
