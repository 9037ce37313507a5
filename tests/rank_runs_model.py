"""Numpy statement of the run rows of the rank stage (scconsensus_amd/csrc/
scc_rank_dev.hpp: rk_chunk; scc_rank_waves.hip: k_rank_mfma16<1, true, true>;
scc_rank_cross.hip: k_rank_cross_runs).  Test code only.

A gene's buckets sit at consecutive slots [bk0, bk0 + nb) of the bucket list,
in value order.  The bucket kernel takes the list in chunks of CH slots; a
gene's buckets inside one chunk are a run.  With h_q the cluster histogram of
bucket q and pre_q[b] the b-elements of the run's earlier buckets, the cross
term over buckets splits into a part inside the runs and a part between them:

    sum_q h_q[a] * (b-elements of buckets < q)
      = sum_q h_q[a] * pre_q[b]  +  sum_r H_r[a] * (b-elements of runs < r)

H_r the run's totals, kept in the row of the run's first slot, max(bk0, c CH)."""
import numpy as np


def chunk(cnt, grid):
    """rk_chunk: the slots a wave takes at a time (cnt: list length, grid: workgroups of four waves)."""
    return max(16, min(512, cnt // (4 * (grid * 4))))


def bucket_cross(H):
    """[K][K] cross term over the buckets' rows H [nb][K]."""
    H = np.asarray(H, np.int64)
    return H.T @ (np.cumsum(H, axis=0) - H)


def run_ids(bk0, nb, CH):
    """The run (chunk number, from the gene's first) of each of the gene's buckets."""
    return (bk0 + np.arange(nb)) // CH - bk0 // CH


def run_rows(bk0, nb, CH):
    """The list slots that hold the gene's run rows: max(bk0, c CH) for the chunks c it touches."""
    c0, c1 = bk0 // CH, (bk0 + nb - 1) // CH
    return np.maximum(bk0, np.arange(c0, c1 + 1) * CH)


def split_cross(H, run):
    """(inside the runs, between the runs, the runs' rows) for buckets H [nb][K]
    with run numbers run [nb] (non-decreasing)."""
    H = np.asarray(H, np.int64)
    run = np.asarray(run)
    K = H.shape[1]
    local = np.zeros((K, K), np.int64)
    rows = []
    for r in np.unique(run):
        Hr = H[run == r]
        local += bucket_cross(Hr)
        rows.append(Hr.sum(axis=0))
    rows = np.array(rows, np.int64)
    return local, bucket_cross(rows), rows


def bounded_local(H, n, run, blim):
    """The part inside the runs as the bucket kernel forms it: doubled, in
    32-bit accumulators that are flushed when the bound of what an entry may
    hold (2 n^2 for the bucket itself, 2 n npre for the run's prefix) would pass
    blim; a bucket whose own term would pass it adds the prefix part in 64
    bits.  Returns (twice the sum, flushes inside runs, the largest value an
    accumulator held)."""
    H = np.asarray(H, np.int64)
    K = H.shape[1]
    total = np.zeros((K, K), np.int64)
    acc = np.zeros((K, K), np.int64)
    pre = np.zeros(K, np.int64)
    npre = bnd = 0
    flushes = peak = 0
    last = None
    for q in range(len(H)):
        if run[q] != last:
            pre[:] = 0
            npre = 0
            last = run[q]
        own = 2 * n[q] * n[q]
        add = own + 2 * n[q] * npre
        wide = add > blim or npre >= 1 << 24  # (the prefix stays within the 24-bit multiplier)
        if wide:
            add = own
        if bnd + add > blim and bnd:
            total += acc
            acc[:] = 0
            bnd = 0
            flushes += npre > 0
        bnd += add
        if wide:
            total += 2 * np.outer(H[q], pre)
        else:
            acc += 2 * np.outer(H[q], pre)
        peak = max(peak, int(acc.max()))
        pre += H[q]
        npre += n[q]
    return total + acc, flushes, peak
