// scc_rank_dev.hpp — what two or more of the rank stage's translation units share.
//
// The rank stage is the all-pairs Wilcoxon rank-sum engine.  It replaces the
// reference's per-(pair, gene) `wilcox.test(data.use[x, ] ~ group)` calls
// (R/reclusterDEConsensusFast.R:78-91; R/reclusterDEConsensus.R:99-103) with
// exact integer arithmetic: R's statistic W = 2U/2 and its tie term
// sum(NTIES^3 - NTIES) are reproduced bit for bit.  All of it works on the
// nonzeros the ingest grouped by (gene, cluster); zeros are never
// materialised.  For every tested pair (a, b) of a gene the units below leave,
// added with integer atomics (order-free) into per-(pair, gene) accumulators,
//   S_ab = #{x in a, y in b: x > y}            (accS)
//   E_ab = sum over tie groups of c_a c_b      (accE)
//   X_ab = sum c_a c_b (c_a + c_b)             (accX)
//   F_a  = sum (c_a^3 - c_a)                   (accF, per cluster)
// and the pair-test kernel (scc_select.hip) adds the implicit zero group in
// closed form:  2U = 2 (S + z_a neg_b + pos_a z_b) + z_a z_b + E,
//               T  = F_a + F_b + f(z_a) + f(z_b) + 3 z_a z_b (z_a + z_b) + 3 X.
//
// The units, in launch order ("Rank stage files"):
//   scc_rank_split.hip    classify the genes any pair tests, cut each into value
//                         buckets (or, on the value-order route, list the
//                         dataset's precomputed cuts)
//   scc_rank_resplit.hip  cut buckets of > 64 distinct values again, two levels
//   scc_rank_waves.hip    one wave per bucket of <= 64 values: slot kernels and
//                         the matrix-core kernel
//   scc_rank_item.hip     one workgroup per bucket too large for a wave
//   scc_rank_cross.hip    what the buckets of one gene owe each other
// Everything here is inline or a template; a helper with one user stays beside
// that user.
#pragma once
#include "scc_common.hpp"
#include "scc_kernels.hpp"

#include <algorithm>

// ---- constants on which two units must agree
// (the split decides each bucket's kind by what the kernels after it can hold)
#define RW_SLOTS_MAX 16  // tested pairs per gene the wave kernel holds: 64 * slots (2, 4, 8 or 16)
#define RW_PAIRS_MAX (8 * 64 * RW_SLOTS_MAX)  // genes past 1024 tested pairs: one 16-slot pass per 1024
#define RS_T 256          // re-split: threads per workgroup
#define RS_KPT 8          // keys per thread (held in registers: the scatter is in place)
#define RS_CAP (RS_T * RS_KPT)  // the largest bucket the split hands to the re-split

// ---- the work counters (names: ScRankCounter, scc_kernels.hpp)
__device__ inline int& rk_cnt(const ScRankLaunch& A, int which) { return A.counts[SCC_CNT_STRIDE * which]; }

// ---- lane helpers
__device__ inline u64 f_tie(u64 c) { return c * c * c - c; }

__device__ inline u32 lanes_below(u64 m)  // popcount of m over lanes < this lane
{
    return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
}

__device__ inline u64 shfl_xor_u64(u64 v, int m)
{
    const u32 lo = __shfl_xor((u32)v, m, 64), hi = __shfl_xor((u32)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

__device__ inline void pair_decode(int p, int K, int& a, int& b)
{
    a = 0;
    int rem = p;
    while (rem >= K - 1 - a) {
        rem -= K - 1 - a;
        ++a;
    }
    b = a + 1 + rem;
}

// lanes whose value of the low `bits` bits of d equals this lane's (among `act`)
template <int BITS>
__device__ inline u64 match_bits(u32 d, u64 act)
{
    u64 peers = act;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 bb = __ballot(bit);
        peers &= bit ? bb : ~bb;
    }
    return peers;
}

// orders one wave's LDS accesses (the wave-level kernels use no workgroup barrier)
__device__ inline void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- the list of ranked genes (k_rank_classify fills it)
// split gene i of split_count(A) (the large ones first)
__device__ inline int split_count(const ScRankLaunch& A) { return rk_cnt(A, RK_CNT_SPLIT_GENES) + rk_cnt(A, RK_CNT_BIG_GENES); }
// (nbig = rk_cnt(A, RK_CNT_BIG_GENES), read once by the caller)
__device__ inline int split_gene_at(const ScRankLaunch& A, int nbig, int i)
{
    return i < nbig ? A.split_genes[A.G - 1 - i] : A.split_genes[i - nbig];
}

// The chunk of the bucket list a wave of k_rank_mfma16 takes at a time: chunk c
// is the list slots [c CH, (c + 1) CH).  cnt: the list's length (RK_CNT_WAVE_SLOTS,
// capped), grid: that kernel's workgroups.  k_rank_cross_runs finds the
// run rows with the same two numbers (ScRankLaunch::rk_grid).
__device__ inline int rk_chunk(int cnt, int grid) { return max(16, min(512, cnt / (4 * (grid * 4)))); }

// ---- host: streams for launches that may overlap
// Launches that may run concurrently taken round st0, side[0], side[1], ...:
// a side stream waits on the fork event (recorded on st0 before the first
// launch: a record costs no wait) when it first gets a launch, and st0 waits on
// its join event at the end.  nside 0: everything on st0.
struct SideStreams {
    hipStream_t st0;
    const hipStream_t* side;
    int nside;
    hipEvent_t fork;
    const hipEvent_t* join;
    bool used[4] = {false, false, false, false};
    int turn = 0;
    SideStreams(hipStream_t s, const hipStream_t* sd, int n, hipEvent_t f, const hipEvent_t* j)
        : st0(s), side(sd), nside((f && j && sd) ? std::min(n, 4) : 0), fork(f), join(j)
    {
        if (nside > 0) hipEventRecord(fork, st0);
    }
    hipStream_t next()
    {
        const int t = turn++;
        if (nside <= 0 || t % (nside + 1) == 0) return st0;
        return pick(t % (nside + 1) - 1);
    }
    hipStream_t pick(int i)  // -1: st0; i: side[i] (st0 when there are fewer sides)
    {
        if (i < 0 || i >= nside) return st0;
        if (!used[i]) hipStreamWaitEvent(side[i], fork, 0);
        used[i] = true;
        return side[i];
    }
    void end()
    {
        for (int i = 0; i < nside; ++i)
            if (used[i]) {
                hipEventRecord(join[i], side[i]);
                hipStreamWaitEvent(st0, join[i], 0);
                used[i] = false;
            }
    }
};
