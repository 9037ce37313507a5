// scc_rank_resplit.hip — rank stage: buckets of > 64 distinct values, cut again.
//
// The split's 2048-bin window spans a gene's whole value range; at 100k+ cells
// a dense stretch puts hundreds of values in one bin.  Such a bucket (a
// "parent", fatbk) is cut again on its own key window, in place, into
// sub-buckets for the wave kernels.  The parent keeps its hbg row for the
// gene-level cross term; what its sub-buckets owe each other is added here from
// LDS histograms, or left as a segment (rsseg, RK_CNT_SEGMENTS) for
// scc_launch_rank_cross_seg when they do not fit.
//   k_rank_resplit     workgroup form: parents of more than RSW_CAP values,
//                      512 bins, a gene's parents dealt to RS_SLICES
//                      workgroups from a queue (RK_CNT_RESPLIT_CURSOR).
//   k_rank_resplit_w   wave form: one wave per parent of <= RSW_CAP values
//                      (most of them), 256 bins, no workgroup barrier.  Two
//                      instances by the gene's tested pairs (TS slots of 64 in
//                      registers).
// Levels: level 0 reads fatbk; a sub-bucket that still holds > 64 distinct
// values is pushed to fat2 (push_fat2, RK_CNT_FAT2) and a second launch of the
// wave form (rs_level 1) cuts it once more.  What fits nowhere (bucket ids or a
// list exhausted) becomes an item (scc_rank_item.hip).  SCC_RESPLIT=0 leaves
// fatbk null and the split sends such buckets to the items.
#include "scc_rank_dev.hpp"

#include <algorithm>
#include <cstddef>

#define RS_SLICES 8       // re-split: workgroups sharing one gene's large parents
#define RS_LOG2B 9
#define RS_BINS (1 << RS_LOG2B)
#define RS_BMAX (2 * RS_BINS + 1)
#define RS_HCAP 2048      // sub-bucket x cluster histogram entries held in LDS
#define RSW_LOG2B 8       // wave re-split: parents of <= RSW_CAP elements, 256 bins
#define RSW_BINS (1 << RSW_LOG2B)
#define RSW_CAP 256
#define RSW_HCAP 512
#define RSW_PACC 1280     // genes with <= this many tested pairs keep them (and their sums) in registers
#define RSW_TS_SMALL 8    // the wave re-split's launch for genes with <= 512 tested pairs

// ===================================================================== re-split
// A bucket the split left with > 64 distinct values (a dense stretch of the
// value axis: at 100k+ cells a 2048-bin window over the gene's whole range
// puts hundreds of values in one bin) is split again on its own key window:
// 512 bins, the same packing rule, elements scattered in place (all of them
// are in registers first).  The sub-buckets go to the wave kernel; the
// parent keeps its cluster histogram row (the gene-level cross term of
// k_rank_cross) and records its sub-bucket range, whose in-parent cross term
// k_rank_cross_seg adds from the sub-buckets' rows.
struct ResplitLds {
    u32 hist[RS_BINS];
    u32 excl[RS_BINS];
    u32 bid[RS_BINS];
    u64 rep[RS_BINS];
    u32 bcur[RS_BMAX];
    u32 boff[RS_BMAX + 1];
    u8 bdiff[RS_BMAX + 3];
    u32 m[SCC_MAX_K];
    u32 wsum[RS_T / 64 + 1];
    u32 wsum2[RS_T / 64 + 1];
    u64 rmn[RS_T / 64], rmx[RS_T / 64];
    u32 hs[RS_HCAP];  // [sub-bucket][cluster] counts (in-parent cross term), when nb * K fits
    u32 bs[RS_HCAP];  // [sub-bucket][cluster] elements of the cluster in lower sub-buckets
    int nb, bk0, next, ovf, nw, w0;
};

// A sub-bucket that still holds > 64 distinct values goes to the second
// re-split level (k_rank_resplit_w with rs_level 1) while its list has room.
__device__ inline bool push_fat2(const ScRankLaunch& A, const ScRankItem& itm)
{
    const int f = atomicAdd(&rk_cnt(A, RK_CNT_FAT2), 1);
    if (f >= A.fat2_cap) return false;
    A.fat2[f] = itm;
    return true;
}

__device__ void resplit_one(const ScRankLaunch& A, const ScRankItem it, ResplitLds& L, u64* __restrict__ acc)
{
    constexpr int W = RS_T / 64, BPT = RS_BINS / RS_T;
    const int K = A.K, g = it.gene, n = it.n;
    const int tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    u64 t_prev = A.stamps ? __builtin_amdgcn_s_memtime() : 0;
#define RSTAMP(ph)                                                                         \
    do {                                                                                   \
        if (A.stamps && tid == 0) {                                                        \
            const u64 t_now = __builtin_amdgcn_s_memtime();                               \
            atomicAdd((unsigned long long*)&A.stamps[ph], (unsigned long long)(t_now - t_prev)); \
            t_prev = t_now;                                                                \
        }                                                                                  \
    } while (0)
    u64 kr[RS_KPT];
    u8 cd[RS_KPT];
#pragma unroll
    for (int q = 0; q < RS_KPT; ++q) {
        const int i = q * RS_T + tid;
        kr[q] = i < n ? A.keys2[it.base + i] : 0ull;
        cd[q] = i < n ? A.codes2[it.base + i] : (u8)0;
    }
    for (int d = tid; d < RS_BINS; d += RS_T) L.hist[d] = 0;
    if (tid < SCC_MAX_K) L.m[tid] = 0;
    u64 kmn = ~0ull, kmx = 0;
#pragma unroll
    for (int q = 0; q < RS_KPT; ++q) {
        if (q * RS_T + tid < n) {
            kmn = kr[q] < kmn ? kr[q] : kmn;
            kmx = kr[q] > kmx ? kr[q] : kmx;
        }
    }
    for (int m2 = 32; m2 >= 1; m2 >>= 1) {
        const u64 o1 = shfl_xor_u64(kmn, m2), o2 = shfl_xor_u64(kmx, m2);
        kmn = o1 < kmn ? o1 : kmn;
        kmx = o2 > kmx ? o2 : kmx;
    }
    if (lane == 0) {
        L.rmn[w] = kmn;
        L.rmx[w] = kmx;
    }
    __syncthreads();
    kmn = L.rmn[0];
    kmx = L.rmx[0];
    for (int v = 1; v < W; ++v) {
        kmn = L.rmn[v] < kmn ? L.rmn[v] : kmn;
        kmx = L.rmx[v] > kmx ? L.rmx[v] : kmx;
    }
    RSTAMP(0);
    const u64 range = kmx - kmn;
    const int bits = range ? 64 - __clzll((long long)range) : 0;
    const int sh = bits > RS_LOG2B ? bits - RS_LOG2B : 0;
#pragma unroll
    for (int q = 0; q < RS_KPT; ++q) {
        if (q * RS_T + tid < n) {
            const u32 d = (u32)((kr[q] - kmn) >> sh);
            atomicAdd(&L.hist[d], 1u);
            L.rep[d] = kr[q];
            atomicAdd(&L.m[cd[q]], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the bins (BPT consecutive bins per thread)
    {
        u32 h[BPT], v = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            h[q] = L.hist[BPT * tid + q];
            v += h[q];
        }
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum[w] = incl;
        __syncthreads();
        u32 b = incl - v;
        for (int q = 0; q < w; ++q) b += L.wsum[q];
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            L.excl[BPT * tid + q] = b;
            b += h[q];
        }
    }
    __syncthreads();
    // buckets: runs of bins with equal floor(excl / target); a bin of more
    // than `target` elements is a bucket of its own (the split's rule)
    const u32 target = (u32)A.wave_target;
    {
        u32 st[BPT], v = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const int d = BPT * tid + q;
            const bool fat = L.hist[d] > target;
            const bool pfat = d > 0 && L.hist[d - 1] > target;
            st[q] = (d == 0) || fat || pfat || (L.excl[d] / target != L.excl[d - 1] / target);
            v += st[q];
        }
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum2[w] = incl;
        __syncthreads();
        u32 b = incl - v;
        for (int q = 0; q < w; ++q) b += L.wsum2[q];
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const int d = BPT * tid + q;
            if (st[q]) L.boff[b] = L.excl[d];
            b += st[q];
            L.bid[d] = b - 1;
        }
        if (tid == RS_T - 1) {
            L.nb = (int)b;
            L.boff[b] = (u32)n;
            const int bk0 = atomicAdd(&rk_cnt(A, RK_CNT_BUCKET_IDS), (int)b);
            L.ovf = bk0 + (int)b > A.bucket_cap;
            L.bk0 = bk0;
        }
    }
    __syncthreads();
    const int nb = L.nb, bk0 = L.bk0;
    RSTAMP(1);
    if (L.ovf) {  // out of bucket ids: rank the parent as one LDS item
        if (tid == 0) {
            const int cls = (n <= A.cap_s) ? 0 : ((n <= A.cap_m) ? 1 : 2);
            A.items[(size_t)cls * A.item_cap + atomicAdd(&rk_cnt(A, RK_CNT_ITEMS0 + cls), 1)] = it;
        }
        return;
    }
    const bool hist_lds = nb * K <= RS_HCAP;
    for (int q = tid; q < nb; q += RS_T) {
        L.bcur[q] = L.boff[q];
        L.bdiff[q] = 0;
    }
    if (hist_lds)
        for (int e = tid; e < nb * K; e += RS_T) L.hs[e] = 0;
    __syncthreads();
    // in-place scatter into sub-bucket order (every element is in registers)
#pragma unroll
    for (int q = 0; q < RS_KPT; ++q) {
        if (q * RS_T + tid < n) {
            const u32 d = (u32)((kr[q] - kmn) >> sh);
            const u32 bk = L.bid[d];
            const u32 pos = atomicAdd(&L.bcur[bk], 1u);
            A.keys2[it.base + pos] = kr[q];
            A.codes2[it.base + pos] = cd[q];
            if (kr[q] != L.rep[d]) L.bdiff[bk] = 1;
            if (hist_lds) atomicAdd(&L.hs[bk * K + cd[q]], 1u);
        }
    }
    __syncthreads();
    RSTAMP(2);
    if (tid < K) A.hbg[(size_t)it.bucket * K + tid] = L.m[tid];  // the parent's row (gene-level cross)
    // sub-buckets for the wave kernel: one list reservation per parent
    {
        u32 wv[(RS_BMAX + RS_T - 1) / RS_T];
        u32 cntw = 0;
        for (int q0 = 0, r = 0; q0 < nb; q0 += RS_T, ++r) {
            const int q = q0 + tid;
            const int c = q < nb ? (int)(L.boff[q + 1] - L.boff[q]) : 0;
            const bool tw = c > 0 && (c <= 64 || !L.bdiff[q]);
            wv[r] = tw;
            cntw += tw;
        }
        cntw = u32_wave_sum(cntw);
        if (lane == 0) L.wsum[w] = cntw;
        __syncthreads();
        if (tid == 0) {
            u32 t = 0;
            for (int v = 0; v < W; ++v) t += L.wsum[v];
            L.nw = (int)t;
            L.w0 = t ? atomicAdd(&rk_cnt(A, RK_CNT_WAVE_SLOTS), (int)t) : 0;
        }
        __syncthreads();
        u32 o = (u32)L.w0;
        for (int q0 = 0, r = 0; q0 < nb; q0 += RS_T, ++r) {  // ordered slots: wave prefix per round
            const int q = q0 + tid;
            const u64 bal = __ballot(wv[r] != 0);
            if (lane == 0) L.wsum2[w] = (u32)__popcll(bal);
            __syncthreads();
            u32 ow = o;
            for (int v = 0; v < w; ++v) ow += L.wsum2[v];
            if (q < nb) {
                const int c = (int)(L.boff[q + 1] - L.boff[q]);
                const int bid = bk0 + q;
                if (c <= 0) {
                    for (int k2 = 0; k2 < K; ++k2) A.hbg[(size_t)bid * K + k2] = 0;
                } else {
                    const bool ties_only = c > 64 && !L.bdiff[q];
                    const ScRankItem itm{it.base + L.boff[q], c, g, ties_only ? 2 : 1, bid};
                    if (wv[r]) {
                        A.sbuckets[ow + lanes_below(bal)] = itm;
                    } else if (A.fat2 && c <= RSW_CAP && push_fat2(A, itm)) {
                        // still > 64 distinct values: a second re-split level
                    } else {
                        const int cls = (c <= A.cap_s) ? 0 : ((c <= A.cap_m) ? 1 : 2);
                        A.items[(size_t)cls * A.item_cap + atomicAdd(&rk_cnt(A, RK_CNT_ITEMS0 + cls), 1)] = itm;
                    }
                }
            }
            for (int v = 0; v < W; ++v) o += L.wsum2[v];
            __syncthreads();
        }
    }
    RSTAMP(3);
    if (!hist_lds) {  // many sub-buckets: k_rank_cross_seg adds the in-parent cross term
        if (tid == 0) A.rsseg[atomicAdd(&rk_cnt(A, RK_CNT_SEGMENTS), 1)] = int4{g, bk0, nb, 0};
        return;
    }
    // in-parent cross term: S_ab += sum_s hs[s][a] * bs[s][b], bs = #(b in
    // sub-buckets < s) (a column scan per cluster first: the pair sums are
    // then independent loads, not a dependent chain)
    for (int c = tid; c < K; c += RS_T) {
        u32 run = 0;
        for (int q = 0; q < nb; ++q) {
            L.bs[q * K + c] = run;
            run += L.hs[q * K + c];
        }
    }
    __syncthreads();
    const int ntp = A.gene_nt[g];
    const bool lds_acc = ntp <= A.P;  // always: the dynamic LDS array holds P entries
    for (int j = tid; j < ntp; j += RS_T) {
        const u32 v = A.gene_tp[(size_t)g * A.P + j];
        const int a = (int)((v >> 16) & 0xffu), b = (int)(v >> 24);
        if (!L.m[a] || !L.m[b]) continue;
        u64 sacc = 0;
#pragma unroll 4
        for (int q = 0; q < nb; ++q) sacc += (u64)L.hs[q * K + a] * L.bs[q * K + b];
        if (lds_acc)
            acc[j] += sacc;  // thread j owns tested pair j for the whole gene
        else if (sacc)
            atomicAdd((unsigned long long*)&A.accS[(size_t)(v & 0xffffu) * A.G + g], (unsigned long long)sacc);
    }
    RSTAMP(4);
    if (A.stamps && tid == 0) atomicAdd((unsigned long long*)&A.stamps[7], 1ull);
#undef RSTAMP
}

__global__ void __launch_bounds__(RS_T) k_rank_resplit(ScRankLaunch A)
{
    __shared__ ResplitLds L;
    // the gene's in-parent cross terms per tested pair: P entries of dynamic LDS
    // (8 B x 66 at config B, x 4950 at E), so no gene falls back to one global
    // atomic per (parent, pair)
    extern __shared__ __attribute__((aligned(16))) u64 racc[];
    const int ng = rk_cnt(A, RK_CNT_FAT_GENES);
    // work items from a queue: slice sl of gene i takes the gene's parents
    // ge.y + sl, ge.y + sl + RS_SLICES, ... (a contiguous run of fatbk), so the
    // large parents of one heavy gene spread over RS_SLICES workgroups (one
    // workgroup per gene left the kernel waiting on its heaviest gene: ~1.5 ms
    // for 1/8 of config D's genes as for all of them).  Every slice adds its
    // in-parent cross terms with integer atomics: order-free.
    for (;;) {
        if (threadIdx.x == 0) L.next = atomicAdd(&rk_cnt(A, RK_CNT_RESPLIT_CURSOR), 1);
        __syncthreads();
        const int wi = L.next;
        if (wi >= ng * RS_SLICES) break;
        const int i = wi / RS_SLICES, sl = wi - i * RS_SLICES;
        const int4 ge = A.fatg[i];
        const int g = ge.x;
        const int ntp = A.gene_nt[g];
        for (int j = threadIdx.x; j < ntp; j += RS_T) racc[j] = 0;
        __syncthreads();
        for (int f = ge.y + sl; f < ge.y + ge.z; f += RS_SLICES) {
            const ScRankItem it = A.fatbk[f];
            if (it.n <= RSW_CAP) continue;  // k_rank_resplit_w (one wave per parent)
            resplit_one(A, it, L, racc);
            __syncthreads();
        }
        for (int j = threadIdx.x; j < ntp; j += RS_T) {
            if (racc[j]) {
                const u32 v = A.gene_tp[(size_t)g * A.P + j];
                atomicAdd((unsigned long long*)&A.accS[(size_t)(v & 0xffffu) * A.G + g], (unsigned long long)racc[j]);
            }
        }
        __syncthreads();
    }
}

// One wave per re-split parent of <= RSW_CAP elements (most of them): the
// same binning, packing, in-place scatter and in-parent cross term as
// resplit_one, with wave-level ordering only (no workgroup barriers) and four
// parents per workgroup in flight.
struct ResplitWLds {  // (offsets and running counts <= RSW_CAP: 16 bits; 12.3 KB a wave, three workgroups per CU)
    u32 hist[RSW_BINS];
    u32 excl[RSW_BINS];
    u32 bid[RSW_BINS];
    u64 rep[RSW_BINS];
    u32 bcur[2 * RSW_BINS + 1];
    uint16_t boff[2 * RSW_BINS + 2];
    u8 bdiff[2 * RSW_BINS + 4];
    u32 m[SCC_MAX_K];
    u32 hs[RSW_HCAP];
    uint16_t bs[RSW_HCAP];
};
static_assert(4 * sizeof(ResplitWLds) <= 160 * 1024 / 3, "wave re-split: three workgroups per CU");

// TS: tested-pair slots held in registers (64 pairs each).  Two launches
// split the genes: TS = RSW_TS_SMALL takes those with <= 64 * RSW_TS_SMALL
// tested pairs (config D FAST: all of them; 3 waves per SIMD instead of 2),
// RSW_PACC / 64 the others (SLOW at K = 50: 1225 pairs).
template <int TS>
__global__ void __launch_bounds__(256) k_rank_resplit_w(ScRankLaunch A)
{
    __shared__ ResplitWLds Ls[4];
    const int lane = threadIdx.x & 63, wv = scc_wave_id();
    ResplitWLds& L = Ls[wv];
    const int K = A.K;
    const ScRankItem* list = A.rs_level ? A.fat2 : A.fatbk;
    const int cnt = A.rs_level ? min(rk_cnt(A, RK_CNT_FAT2), A.fat2_cap) : min(rk_cnt(A, RK_CNT_FAT), A.fat_cap);
    constexpr int EPL = RSW_CAP / 64, BPL = RSW_BINS / 64;
    // Bucket ids and wave-list slots come from wave-private chunks: one global
    // atomic per chunk, not per parent (same-address atomics serialise in L2:
    // two per parent cost 48 of this kernel's 54 ms at config D).  Unused
    // list slots are filled with empty descriptors the wave kernel skips.
    const ScRankItem nullit{0, 0, 0, 1, -1};
    const int chunk = A.rsw_chunk;
    int id_cur = 0, id_end = 0, sl_cur = 0, sl_end = 0;
    auto fill_null = [&](int a, int b) {
        for (int q = a + lane; q < b; q += 64) A.sbuckets[q] = nullit;
    };
    // Each wave takes a contiguous run of the parent list.  The list holds a
    // gene's parents together, so the gene's tested pairs are loaded into
    // registers once per run (lane l: pairs l, l + 64, ...) and the in-parent
    // cross terms of consecutive parents add up there, reaching accS with one
    // atomic per (run of one gene, pair) instead of one per (parent, pair).
    // The consecutive sub-buckets also keep the wave kernel's register
    // accumulation on one gene.
    constexpr int PACC = 64 * TS;  // genes past it: per-(parent, pair) atomics (as past RSW_PACC before)
    constexpr bool SMALL = TS < RSW_PACC / 64;
    const int nw = gridDim.x * 4, w = blockIdx.x * 4 + wv;
    const int f0 = (int)((long long)cnt * w / nw), f1 = (int)((long long)cnt * (w + 1) / nw);
    u32 tpr[TS], par[TS];
#pragma unroll
    for (int s = 0; s < TS; ++s) tpr[s] = par[s] = 0;
    int pg = -1, pnt = 0, pn = 0;
    auto flush_par = [&]() {
        if (pg >= 0 && pn > 0 && pnt <= PACC) {
#pragma unroll
            for (int s = 0; s < TS; ++s) {
                if (s * 64 >= pnt) break;
                if (par[s])
                    atomicAdd((unsigned long long*)&A.accS[(size_t)(tpr[s] & 0xffffu) * A.G + pg], (unsigned long long)par[s]);
                par[s] = 0;
            }
        }
        pn = 0;
    };
    for (int f = f0; f < f1; ++f) {
        const ScRankItem it = list[f];
        const int n = it.n, g = it.gene;
        if (!A.rsw_all) {  // this launch's genes (a gene's parents are together in the list)
            const int nt_g = A.gene_nt[g];
            if (SMALL ? nt_g > PACC : nt_g <= 64 * RSW_TS_SMALL) continue;
        }
        // a parent adds at most 128 * 128 to one pair: flush before u32 could wrap
        if (g != pg || pn >= 65536) {
            flush_par();
            if (g != pg) {
                pg = g;
                pnt = A.gene_nt[g];
                if (pnt > 0 && pnt <= PACC) {
                    const u32* tl = A.gene_tp + (size_t)g * A.P;
#pragma unroll
                    for (int s = 0; s < TS; ++s) tpr[s] = tl[min(s * 64 + lane, pnt - 1)];
                }
            }
        }
        if (n > RSW_CAP) continue;  // k_rank_resplit (a workgroup per parent)
        u64 kr[EPL];
        u32 cd[EPL];
        u64 kmn = ~0ull, kmx = 0;
#pragma unroll
        for (int q = 0; q < EPL; ++q) {
            const int i = q * 64 + lane;
            kr[q] = i < n ? A.keys2[it.base + i] : 0ull;
            cd[q] = i < n ? (u32)A.codes2[it.base + i] : 0u;
            if (i < n) {
                kmn = kr[q] < kmn ? kr[q] : kmn;
                kmx = kr[q] > kmx ? kr[q] : kmx;
            }
        }
        for (int m2 = 32; m2 >= 1; m2 >>= 1) {
            const u64 o1 = shfl_xor_u64(kmn, m2), o2 = shfl_xor_u64(kmx, m2);
            kmn = o1 < kmn ? o1 : kmn;
            kmx = o2 > kmx ? o2 : kmx;
        }
        const u64 range = kmx - kmn;
        const int bits = range ? 64 - __clzll((long long)range) : 0;
        const int sh = bits > RSW_LOG2B ? bits - RSW_LOG2B : 0;
#pragma unroll
        for (int q = 0; q < BPL; ++q) L.hist[q * 64 + lane] = 0;
        for (int c = lane; c < SCC_MAX_K; c += 64) L.m[c] = 0;
        wsync();
#pragma unroll
        for (int q = 0; q < EPL; ++q) {
            if (q * 64 + lane < n) {
                const u32 d = (u32)((kr[q] - kmn) >> sh);
                atomicAdd(&L.hist[d], 1u);
                L.rep[d] = kr[q];
                atomicAdd(&L.m[cd[q]], 1u);
            }
        }
        wsync();
        // exclusive scan of the bins, BPL consecutive bins per lane
        {
            u32 h[BPL], v = 0;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                h[q] = L.hist[BPL * lane + q];
                v += h[q];
            }
            u32 incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            u32 b = incl - v;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                L.excl[BPL * lane + q] = b;
                b += h[q];
            }
        }
        wsync();
        const u32 target = (u32)A.wave_target;
        int nb;
        {
            u32 st[BPL], v = 0;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                const int d = BPL * lane + q;
                const bool fat = L.hist[d] > target;
                const bool pfat = d > 0 && L.hist[d - 1] > target;
                st[q] = (d == 0) || fat || pfat || (L.excl[d] / target != L.excl[d - 1] / target);
                v += st[q];
            }
            u32 incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            u32 b = incl - v;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                const int d = BPL * lane + q;
                if (st[q]) L.boff[b] = L.excl[d];
                b += st[q];
                L.bid[d] = b - 1;
            }
            nb = __shfl((int)incl, 63, 64);
            if (lane == 0) L.boff[nb] = (u32)n;
        }
        bool ovf = false;
        if (nb > id_end - id_cur) {
            const int grab = max(nb, 2 * chunk);
            int b0 = 0;
            if (lane == 0) b0 = atomicAdd(&rk_cnt(A, RK_CNT_BUCKET_IDS), grab);
            b0 = __shfl(b0, 0, 64);
            ovf = b0 + grab > A.bucket_cap;
            id_cur = b0;
            id_end = ovf ? b0 : b0 + grab;
        }
        const int bk0 = id_cur;
        if (!ovf) id_cur += nb;
        if (ovf) {  // out of bucket ids: rank the parent as one LDS item
            if (lane == 0) {
                const int cls = (n <= A.cap_s) ? 0 : ((n <= A.cap_m) ? 1 : 2);
                A.items[(size_t)cls * A.item_cap + atomicAdd(&rk_cnt(A, RK_CNT_ITEMS0 + cls), 1)] = it;
            }
            continue;
        }
        const bool hist_lds = nb * K <= RSW_HCAP;
        wsync();
        for (int q = lane; q < nb; q += 64) {
            L.bcur[q] = L.boff[q];
            L.bdiff[q] = 0;
        }
        if (hist_lds)
            for (int e = lane; e < nb * K; e += 64) L.hs[e] = 0;
        wsync();
#pragma unroll
        for (int q = 0; q < EPL; ++q) {
            if (q * 64 + lane < n) {
                const u32 d = (u32)((kr[q] - kmn) >> sh);
                const u32 bk = L.bid[d];
                const u32 pos = atomicAdd(&L.bcur[bk], 1u);
                A.keys2[it.base + pos] = kr[q];
                A.codes2[it.base + pos] = (u8)cd[q];
                if (kr[q] != L.rep[d]) L.bdiff[bk] = 1;
                if (hist_lds) atomicAdd(&L.hs[bk * K + cd[q]], 1u);
            }
        }
        wsync();
        for (int c = lane; c < K; c += 64) A.hbg[(size_t)it.bucket * K + c] = L.m[c];  // the parent's row (gene-level cross)
        // sub-buckets: one list reservation per parent, slots in sub-bucket order
        {
            u32 cw = 0;
            for (int q = lane; q < nb; q += 64) {
                const int c = (int)(L.boff[q + 1] - L.boff[q]);
                cw += (c > 0 && (c <= 64 || !L.bdiff[q])) ? 1u : 0u;
            }
            cw = u32_wave_sum(cw);
            bool to_items = false;
            if ((int)cw > sl_end - sl_cur) {
                fill_null(sl_cur, sl_end);
                const int grab = max((int)cw, chunk);
                int s0 = 0;
                if (lane == 0) s0 = atomicAdd(&rk_cnt(A, RK_CNT_WAVE_SLOTS), grab);
                s0 = __shfl(s0, 0, 64);
                if (s0 + grab > A.bucket_cap) {  // list full: these sub-buckets go to the LDS items
                    fill_null(min(s0, A.bucket_cap), A.bucket_cap);
                    to_items = true;
                    sl_cur = sl_end = 0;
                } else {
                    sl_cur = s0;
                    sl_end = s0 + grab;
                }
            }
            u32 o = (u32)sl_cur;
            if (!to_items) sl_cur += (int)cw;
            for (int q0 = 0; q0 < nb; q0 += 64) {
                const int q = q0 + lane;
                int c = 0;
                bool tw = false;
                if (q < nb) {
                    c = (int)(L.boff[q + 1] - L.boff[q]);
                    tw = c > 0 && (c <= 64 || !L.bdiff[q]);
                }
                if (to_items) tw = false;
                const u64 bal = __ballot(tw);
                if (q < nb) {
                    const int bid = bk0 + q;
                    if (c <= 0) {
                        for (int k2 = 0; k2 < K; ++k2) A.hbg[(size_t)bid * K + k2] = 0;
                    } else {
                        const bool ties_only = c > 64 && !L.bdiff[q];
                        const ScRankItem itm{it.base + L.boff[q], c, g, ties_only ? 2 : 1, bid};
                        if (tw) {
                            A.sbuckets[o + lanes_below(bal)] = itm;
                        } else if (A.rs_level == 0 && A.fat2 && push_fat2(A, itm)) {
                            // still > 64 distinct values: a second re-split level
                        } else {
                            const int cls = (c <= A.cap_s) ? 0 : ((c <= A.cap_m) ? 1 : 2);
                            A.items[(size_t)cls * A.item_cap + atomicAdd(&rk_cnt(A, RK_CNT_ITEMS0 + cls), 1)] = itm;
                        }
                    }
                }
                o += (u32)__popcll(bal);
            }
        }
        if (!hist_lds) {  // many sub-buckets: k_rank_cross_seg adds the in-parent cross term
            if (lane == 0) A.rsseg[atomicAdd(&rk_cnt(A, RK_CNT_SEGMENTS), 1)] = int4{g, bk0, nb, 0};
            continue;
        }
        for (int c = lane; c < K; c += 64) {
            u32 run = 0;
            for (int q = 0; q < nb; ++q) {
                L.bs[q * K + c] = run;
                run += L.hs[q * K + c];
            }
        }
        wsync();
        const int ntp = pnt;
        if (ntp <= PACC) {
            // m[a] = 0 or m[b] = 0 makes every product zero: no test needed
            ++pn;
#pragma unroll
            for (int s = 0; s < TS; ++s) {
                if (s * 64 >= ntp) break;
                const u32 v = tpr[s];
                const int a = (int)((v >> 16) & 0xffu), b = (int)(v >> 24);
                u32 sacc = 0;  // <= m[a] * m[b] <= 128 * 128
                for (int q = 0; q < nb; ++q) sacc += L.hs[q * K + a] * L.bs[q * K + b];
                par[s] += (s * 64 + lane < ntp) ? sacc : 0u;
            }
        } else {
            const u32* tl = A.gene_tp + (size_t)g * A.P;
            for (int j = lane; j < ntp; j += 64) {
                const u32 v = tl[j];
                const int a = (int)((v >> 16) & 0xffu), b = (int)(v >> 24);
                if (!L.m[a] || !L.m[b]) continue;
                u64 sacc = 0;
                for (int q = 0; q < nb; ++q) sacc += (u64)L.hs[q * K + a] * L.bs[q * K + b];
                if (sacc) atomicAdd((unsigned long long*)&A.accS[(size_t)(v & 0xffffu) * A.G + g], (unsigned long long)sacc);
            }
        }
        wsync();
    }
    flush_par();
    fill_null(sl_cur, sl_end);
}

extern "C" hipError_t scc_launch_rank_resplit(const ScRankLaunch* L, int grid, hipStream_t st0, const hipStream_t* side,
                                              int nside, hipEvent_t fork, const hipEvent_t* join)
{
    if (!L->fatbk || grid <= 0) return hipSuccess;
    // the first level's three launches take disjoint parents (<= RSW_CAP
    // elements by tested-pair class, larger ones) and meet only in atomic
    // allocation counters: concurrent; the second level reads the first's fat2
    SideStreams ss(st0, side, nside, fork, join);
    hipStream_t st = st0;
    // wave-private allocation chunks sized so that the unused tails of all
    // waves stay a small part of the bucket capacity
    ScRankLaunch W = *L;
    const long long waves = 2LL * grid * 4;
    W.rsw_chunk = (int)std::max(8LL, std::min(128LL, (long long)L->bucket_cap / (16 * waves)));
    W.rs_level = 0;
    // K > 64 (config E): most genes hold more than 512 tested pairs, one launch
    // of the wide variant takes every parent (a second pass over the list cost more)
    W.rsw_all = L->K > 64 ? 1 : 0;
    if (!W.rsw_all) hipLaunchKernelGGL(k_rank_resplit_w<RSW_TS_SMALL>, dim3(2 * grid), dim3(256), 0, ss.next(), W);
    if (L->P > 64 * RSW_TS_SMALL)
        hipLaunchKernelGGL(k_rank_resplit_w<RSW_PACC / 64>, dim3(2 * grid), dim3(256), 0, ss.next(), W);
    const size_t acc_lds = sizeof(u64) * (size_t)std::max(L->P, 1);
    scc_set_lds((const void*)k_rank_resplit, (int)acc_lds);
    hipLaunchKernelGGL(k_rank_resplit, dim3(grid), dim3(RS_T), acc_lds, ss.next(), *L);
    ss.end();
    if (L->fat2) {  // sub-buckets the first level left with > 64 distinct values
        W.rs_level = 1;
        if (!W.rsw_all) hipLaunchKernelGGL(k_rank_resplit_w<RSW_TS_SMALL>, dim3(2 * grid), dim3(256), 0, st, W);
        if (L->P > 64 * RSW_TS_SMALL)
            hipLaunchKernelGGL(k_rank_resplit_w<RSW_PACC / 64>, dim3(2 * grid), dim3(256), 0, st, W);
    }
    return hipGetLastError();
}
