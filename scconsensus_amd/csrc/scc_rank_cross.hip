// scc_rank_cross.hip — rank stage: what the buckets of one gene owe each other.
//
// Buckets are value ranges in ascending order, so for tested pair (a, b) every
// a-element of a bucket lies above every b-element of the buckets before it:
//   S_ab += sum over buckets q of h_q[a] * #(b-elements in buckets < q)
// from the per-bucket cluster histogram rows (hbg) that whoever ranked a bucket
// wrote.  Three forms of the same sum:
//   k_rank_cross       one wave per (gene, pair), lanes over buckets
//                      (P <= 128, or SCC_CROSS_WAVE=1).
//   k_rank_cross_gene  one workgroup per gene, its rows read once into LDS
//                      (P > 128).
//   k_rank_cross_runs  run rows (value-order route, K <= 16): the matrix-core
//                      kernel has added the term inside each run and left one
//                      row per run; this adds what the runs owe each other.
// The SEG instances of the first two run the sum over the sub-buckets of each
// re-split parent that left a segment (rsseg): scc_launch_rank_cross_seg.
#include "scc_rank_dev.hpp"

// ===================================================================== cross
// Cross-bucket rank sums: for tested pair (a, b) of gene g,
//   S_ab += sum over buckets beta of h_beta[a] * #(b-elements in buckets < beta)
// one wave per (gene, pair), lanes over buckets (inclusive scan per 64).
// SEG: the same over the sub-buckets of each re-split parent (k_rank_resplit).
template <bool SEG>
__global__ void __launch_bounds__(256) k_rank_cross(ScRankLaunch A)
{
    const int lane = threadIdx.x & 63;
    const int W = blockIdx.x * 4 + scc_wave_id(), NW = gridDim.x * 4;
    const int ng = SEG ? rk_cnt(A, RK_CNT_SEGMENTS) : split_count(A), P = A.P, nbig = rk_cnt(A, RK_CNT_BIG_GENES);
    for (int f = W; f < ng * P; f += NW) {
        const int gi = f / P, p = f - gi * P;
        int g, bk0, nb;
        if (SEG) {
            const int4 sg = A.rsseg[gi];
            g = sg.x;
            bk0 = sg.y;
            nb = sg.z;
        } else {
            g = split_gene_at(A, nbig, gi);
            bk0 = A.gene_bk[2 * g];
            nb = A.gene_bk[2 * g + 1];
        }
        if (!A.all_pairs && !(A.flags[(size_t)p * A.G + g] & 1)) continue;
        int a, b;
        pair_decode(p, A.K, a, b);
        const unsigned int* h = A.hbg + (size_t)bk0 * A.K;
        u64 s = 0, carry = 0;
        for (int q0 = 0; q0 < nb; q0 += 64) {
            const int q = q0 + lane;
            const u32 ha = (q < nb) ? h[(size_t)q * A.K + a] : 0u;
            const u32 hb = (q < nb) ? h[(size_t)q * A.K + b] : 0u;
            u32 inc = hb;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            s += (u64)ha * (carry + inc - hb);
            carry += (u32)__shfl((int)inc, 63, 64);
        }
        s = u64_wave_sum(s);
        if (lane == 0 && s) atomicAdd((unsigned long long*)&A.accS[(size_t)p * A.G + g], (unsigned long long)s);
    }
}

// The same over run rows (k_rank_mfma16<NC, true, true>): within a run the
// bucket kernel has added the term itself, so what is left is
//   S_ab += sum over runs r of H_r[a] * #(b-elements in the gene's earlier runs)
// H_r the run's totals, in the hbg row of the run's first list slot.  A gene
// with buckets [bk0, bk0 + nb) has a run in every chunk it touches, chunk c at
// row max(bk0, c CH), CH from rk_chunk as in the bucket kernel.  A gene has few
// runs (config B: four of 16 buckets) and up to 120 tested pairs, so a wave
// takes a gene, a lane a tested pair of its list, and walks the runs in order
// with the b-count so far in a register, four rows' loads in flight together
// (a wave per (gene, pair) with the lanes over runs was a chain of four
// dependent loads per pair, 19 pairs a wave in turn: 54 us at B).  A gene of
// one run owes nothing.
__global__ void __launch_bounds__(256) k_rank_cross_runs(ScRankLaunch A)
{
    const int lane = threadIdx.x & 63;
    const int W = blockIdx.x * 4 + scc_wave_id(), NW = gridDim.x * 4;
    const int ng = split_count(A), P = A.P, K = A.K, nbig = rk_cnt(A, RK_CNT_BIG_GENES);
    const int CH = rk_chunk(min(rk_cnt(A, RK_CNT_WAVE_SLOTS), A.bucket_cap), A.rk_grid);
    for (int gi = W; gi < ng; gi += NW) {
        const int g = split_gene_at(A, nbig, gi);
        const int bk0 = A.gene_bk[2 * g], nb = A.gene_bk[2 * g + 1];
        if (nb < 1) continue;
        const int ch0 = bk0 / CH, nr = (bk0 + nb - 1) / CH - ch0 + 1;
        if (nr < 2) continue;
        const int ntp = min(A.gene_nt[g], P);
        const u32* tl = A.gene_tp + (size_t)g * P;
        for (int j0 = 0; j0 < ntp; j0 += 64) {
            const int j = j0 + lane;
            const u32 v = tl[min(j, ntp - 1)];
            const int a = (int)((v >> 16) & 0xffu), b = (int)(v >> 24);
            u64 s = 0, below = 0;
            for (int r0 = 0; r0 < nr; r0 += 4) {
                u32 ha[4], hb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {  // (rows past the gene's last run: the last run's again, zeroed)
                    const int r = min(r0 + u, nr - 1);
                    const unsigned int* h = A.hbg + (size_t)max(bk0, (ch0 + r) * CH) * K;
                    ha[u] = h[a];
                    hb[u] = h[b];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (r0 + u < nr) {
                        s += (u64)ha[u] * below;
                        below += hb[u];
                    }
                }
            }
            if (j < ntp && s) atomicAdd((unsigned long long*)&A.accS[(size_t)(v & 0xffffu) * A.G + g], (unsigned long long)s);
        }
    }
}

// Gene-level cross terms, one workgroup per split gene:
//   S_ab += sum_q H[q][a] * C[q][b],  C[q][b] = #(b-elements in buckets < q)
// over the gene's buckets q in value order.  The gene's histogram rows are
// read once, 64 buckets at a time, into LDS (coalesced: rows are [bucket][K]),
// C comes from a column scan with a carry, and each thread accumulates its
// tested pairs (<= XC_J per thread) in registers: one atomic per (gene, pair).
// (The per-(gene, pair) wave version re-read the rows once per pair.)
#define XC_T 256
#define XC_Q 64                 // buckets per LDS round
#define XC_KC SCC_MAX_K         // cluster columns held
#define XC_J 8                  // tested pairs per thread per pass over the rows (2048)
#define XC_PF ((XC_Q * XC_KC + XC_T - 1) / XC_T)  // histogram words a thread prefetches per round
// SEG: the same sum over the sub-buckets of each re-split parent (the
// in-parent cross term; segments from k_rank_resplit*, rsseg).
// Each round's rows are loaded into registers while the previous round is
// summed (its latency off the per-gene chain), and every pair's sum over a
// round runs as four independent partial sums (the LDS reads in flight
// together): one workgroup walks a gene's buckets in order, so the per-round
// chain is what its time was (config D: 2.5 ms, D SLOW 7.8 ms before).
template <bool SEG>
__global__ void __launch_bounds__(XC_T) k_rank_cross_gene(ScRankLaunch A)
{
    // cluster-major: a pair's rows of one round are contiguous, read 4 at a time
    // (16-B LDS reads; the row stride XC_Q + 4 words spreads the clusters over banks)
    __shared__ __attribute__((aligned(16))) u32 Hs[XC_KC][XC_Q + 4];
    __shared__ __attribute__((aligned(16))) u32 Cs[XC_KC][XC_Q + 4];
    __shared__ u32 seg[XC_T / XC_KC][XC_KC];
    __shared__ u32 carry[XC_KC];
    constexpr int NPART = XC_T / XC_KC, RPP = XC_Q / NPART;  // column-scan parts, rows per part
    const int tid = threadIdx.x, K = A.K, G = A.G, P = A.P;
    const int ng = SEG ? rk_cnt(A, RK_CNT_SEGMENTS) : split_count(A), nbig = rk_cnt(A, RK_CNT_BIG_GENES);
    for (int gi = blockIdx.x; gi < ng; gi += gridDim.x) {
        int g, bk0, nb;
        if (SEG) {
            const int4 sg = A.rsseg[gi];
            g = sg.x;
            bk0 = sg.y;
            nb = sg.z;
        } else {
            g = split_gene_at(A, nbig, gi);
            bk0 = A.gene_bk[2 * g];
            nb = A.gene_bk[2 * g + 1];
        }
        const int ntp = min(A.gene_nt[g], P);
        const u32* tl = A.gene_tp + (size_t)g * P;
        const int nw = XC_Q * K;  // histogram words of a full round
        // one round's rows into registers (clamped loads, masked past the gene)
        u32 hv[XC_PF];
        auto prefetch = [&](int q0) {
            const unsigned int* h = A.hbg + (size_t)(bk0 + q0) * K;
            const int lim = (min(XC_Q, nb - q0)) * K;
#pragma unroll
            for (int r = 0; r < XC_PF; ++r) {
                const int e = r * XC_T + tid;
                hv[r] = h[min(e, max(lim - 1, 0))];
                if (e >= lim) hv[r] = 0u;
            }
        };
        for (int j0 = 0; j0 < ntp; j0 += XC_J * XC_T) {  // windows of 2048 tested pairs
            u32 pv[XC_J];
            u64 acc[XC_J];
#pragma unroll
            for (int u = 0; u < XC_J; ++u) {
                const int j = j0 + u * XC_T + tid;
                pv[u] = j < ntp ? tl[j] : 0u;
                acc[u] = 0;
            }
            if (nb > 0) prefetch(0);
            __syncthreads();
            if (tid < XC_KC) carry[tid] = 0;
            for (int q0 = 0; q0 < nb; q0 += XC_Q) {
                const int nq = min(XC_Q, nb - q0);
                __syncthreads();
#pragma unroll
                for (int r = 0; r < XC_PF; ++r) {
                    const int e = r * XC_T + tid;
                    if (e < nw) {
                        const int q = e / K, c = e - q * K;
                        Hs[c][q] = hv[r];
                    }
                }
                if (q0 + XC_Q < nb) prefetch(q0 + XC_Q);  // the next round's rows, in flight meanwhile
                __syncthreads();
                // column scan: thread (c, part) sums RPP rows, parts combined through LDS
                const int c = tid % XC_KC, part = tid / XC_KC;
                u32 ssum = 0;
                if (c < K)
                    for (int q = part * RPP; q < part * RPP + RPP; ++q) ssum += Hs[c][q];
                seg[part][c] = ssum;
                __syncthreads();
                if (c < K) {
                    u32 run = carry[c];
                    for (int v = 0; v < part; ++v) run += seg[v][c];
                    for (int q = part * RPP; q < part * RPP + RPP; ++q) {
                        Cs[c][q] = run;
                        run += Hs[c][q];
                    }
                }
                __syncthreads();
                if (tid < K)
                    for (int v = 0; v < NPART; ++v) carry[tid] += seg[v][tid];
#pragma unroll
                for (int u = 0; u < XC_J; ++u) {
                    if (j0 + u * XC_T + tid < ntp) {
                        const int a = (int)((pv[u] >> 16) & 0xffu), b = (int)(pv[u] >> 24);
                        u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;  // (rows past nq are zero)
                        const uint4* ha = (const uint4*)Hs[a];
                        const uint4* cb = (const uint4*)Cs[b];
#pragma unroll 4
                        for (int q4 = 0; q4 < XC_Q / 4; ++q4) {
                            const uint4 hx = ha[q4], cx = cb[q4];
                            s0 += (u64)hx.x * cx.x;
                            s1 += (u64)hx.y * cx.y;
                            s2 += (u64)hx.z * cx.z;
                            s3 += (u64)hx.w * cx.w;
                        }
                        acc[u] += (s0 + s1) + (s2 + s3);
                    }
                }
                (void)nq;
            }
#pragma unroll
            for (int u = 0; u < XC_J; ++u) {
                if (j0 + u * XC_T + tid < ntp && acc[u])
                    atomicAdd((unsigned long long*)&A.accS[(size_t)(pv[u] & 0xffffu) * G + g], (unsigned long long)acc[u]);
            }
        }
        __syncthreads();
    }
}

extern "C" hipError_t scc_launch_rank_cross(const ScRankLaunch* L, int grid, hipStream_t st)
{
    // per-gene workgroups pay off once genes have many tested pairs (at P = 66 the
    // per-(gene, pair) waves are 12 us faster; at P >= 435 the gene kernel wins)
    if (L->rank_runs)  // the bucket kernel left run rows (K <= 16: P <= 120)
        hipLaunchKernelGGL(k_rank_cross_runs, dim3(grid), dim3(256), 0, st, *L);
    else if (L->P > 128 && !L->cross_wave)
        hipLaunchKernelGGL(k_rank_cross_gene<false>, dim3(grid), dim3(XC_T), 0, st, *L);
    else  // one wave per (gene, pair) (SCC_CROSS_WAVE=1 selects it for comparisons)
        hipLaunchKernelGGL(k_rank_cross<false>, dim3(grid), dim3(256), 0, st, *L);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_rank_cross_seg(const ScRankLaunch* L, int grid, hipStream_t st)
{
    if (!L->fatbk) return hipSuccess;
    if (L->P > 128 && !L->cross_wave)  // one workgroup per segment, its rows read once (as the gene level)
        hipLaunchKernelGGL(k_rank_cross_gene<true>, dim3(grid), dim3(XC_T), 0, st, *L);
    else
        hipLaunchKernelGGL(k_rank_cross<true>, dim3(grid), dim3(256), 0, st, *L);
    return hipGetLastError();
}
