// scc_rank_split.hip — rank stage: which genes are ranked, and their value buckets.
//
//   k_rank_classify  per gene: does any cluster pair test it (FAST filters
//                  ran before the rank stage, exactly as ComputePairWiseDE
//                  only tests the features that pass, Fast:242-291)?  Every
//                  tested gene joins split_genes: genes of >= SPLIT_BIG values
//                  from the far end (RK_CNT_BIG_GENES), the others from the
//                  front (RK_CNT_SPLIT_GENES); split_gene_at hands the large
//                  ones out first.
//   k_rank_split   workgroups take genes from a queue (RK_CNT_SPLIT_CURSOR):
//                  the gene's tested pairs compacted into gene_tp, a 2048-bin
//                  histogram of the value key, bins packed into value-range
//                  buckets, the values scattered to bucket order (keys2 /
//                  codes2).  Equal values never straddle buckets, so ties
//                  stay inside one unit of work.  Each bucket gets a global id
//                  (its hbg row) and a kind: <= 64 values, or one repeated
//                  value, to the wave-bucket list (scc_rank_waves.hip); up to
//                  RS_CAP values to the re-split (scc_rank_resplit.hip);
//                  anything else is an item (scc_rank_item.hip).
//   k_rank_vorder_list  the split's stand-in on the value-order route
//                  (SCC_RANK_VORDER, scc_vorder.hip): the dataset keeps each
//                  gene's cells in value order with precomputed cuts, so the
//                  list is one wave bucket per cut and nothing is scattered.
// scc_rank_split_diag prints the per-gene clocks k_rank_split keeps under
// SCC_RW_DEBUG >= 9 (g_split_diag).
#include "scc_rank_dev.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <vector>

// ===================================================================== classify
#define SPLIT_BIG 32768

__global__ void k_rank_classify(ScRankLaunch A)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.G) return;
    const i64 base = A.gstart[g];
    const i64 n = A.gstart[g + 1] - base;
    if (n <= 0) return;
    if (!A.all_pairs) {
        // 16 pairs' flags per round (clamped loads in flight together): an untested
        // gene costs P / 16 dependent rounds instead of P
        bool any = false;
        for (int p0 = 0; p0 < A.P && !any; p0 += 16) {
            u8 f[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) f[u] = A.flags[(size_t)min(p0 + u, A.P - 1) * A.G + g];
#pragma unroll
            for (int u = 0; u < 16; ++u) any |= (f[u] & 1) != 0;
        }
        if (!any) return;
    }
    // every ranked gene is split into value buckets; genes of >= SPLIT_BIG
    // values fill the list from its end (split_gene_at hands them out first:
    // the split's queue runs longest first, so a gene shard's largest genes
    // are not its tail)
    if (n >= SPLIT_BIG)
        A.split_genes[A.G - 1 - atomicAdd(&rk_cnt(A, RK_CNT_BIG_GENES), 1)] = g;
    else
        A.split_genes[atomicAdd(&rk_cnt(A, RK_CNT_SPLIT_GENES), 1)] = g;
}

extern "C" hipError_t scc_launch_rank_classify(const ScRankLaunch* L, hipStream_t st)
{
    hipLaunchKernelGGL(k_rank_classify, dim3((L->G + 255) / 256), dim3(256), 0, st, *L);
    return hipGetLastError();
}

// ===================================================================== split
#define SP_T 1024
#define SP_W (SP_T / 64)
#define SP_BINS 2048
#define SP_BMAX (2 * SP_BINS + 1)  // a bucket starts at a bin, or right after a fat bin
#define SP_KPT 8                    // keys per thread held in registers across the passes
#define SP_CHUNK (SP_T * SP_KPT)
#define SP_SUP 4096  // two-level scatter: group width (a group holds < 2 * SP_SUP = SP_CHUNK values)
#define SP_NSUP 1022 // groups a gene may have (three [SP_NSUP + 1] u32 tables fit the excl table)

struct SplitLds {
    u32 hist[SP_BINS];
    u32 excl[SP_BINS];
    u32 bid[SP_BINS];   // bucket of each bin
    u32 bcur[SP_BMAX];  // bucket cursors
    u32 boff[SP_BMAX + 1];
    u64 rep[SP_BINS];      // one key of each bin (any: the last leader's store wins)
    u8 bdiff[SP_BMAX + 3]; // bucket holds two different keys
    u32 wsum[SP_W + 1];
    u32 wsum2[SP_W + 1];
    u64 rmn[SP_W], rmx[SP_W];
    u32 cdf[SP_BINS + 1];  // the linear window's counts, scanned: the equalized bins' map
    int off[SCC_MAX_K + 1];
    int nb, bk0, next;
    int nfat, fat0, nwav, wav0;
    int nsup;
};
// the split's LDS: its tables, then the bucket-order staging of a gene that
// fits one register chunk (SP_CHUNK keys + codes)
static constexpr size_t kSplitStageOff = (sizeof(SplitLds) + 15) & ~(size_t)15;
static_assert(kSplitStageOff + (size_t)SP_CHUNK * 9 <= 160 * 1024, "split LDS");


// The tested pairs of gene g, compacted in pair order into gene_tp[g] as
// p | a << 16 | b << 24, and their number (also gene_nt[g]).  A workgroup of
// T threads; wsum: [T / 64] in LDS.
template <int T>
__device__ inline u32 gene_tested_pairs(const ScRankLaunch& A, int g, u32* wsum)
{
    const int K = A.K, G = A.G;
    const int tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    u32 ntested = 0;
    if constexpr (T == 64) {  // one wave (any wave of a workgroup, on a gene of its own): ballots alone
        for (int p0 = 0; p0 < A.P; p0 += 64) {
            const int p = p0 + lane;
            const bool t = p < A.P && (A.all_pairs || (A.flags[(size_t)p * G + g] & 1));
            const u64 bal = __ballot(t);
            if (t) {
                int a2, b2;
                pair_decode(p, K, a2, b2);
                A.gene_tp[(size_t)g * A.P + ntested + lanes_below(bal)] = (u32)p | ((u32)a2 << 16) | ((u32)b2 << 24);
            }
            ntested += (u32)__popcll(bal);
        }
        if (lane == 0) A.gene_nt[g] = (int)ntested;
        return ntested;
    }
    for (int p0 = 0; p0 < A.P; p0 += T) {
        const int p = p0 + tid;
        const bool t = p < A.P && (A.all_pairs || (A.flags[(size_t)p * G + g] & 1));
        const u64 bal = __ballot(t);
        if (lane == 0) wsum[w] = (u32)__popcll(bal);
        __syncthreads();
        u32 o = ntested;
        for (int v = 0; v < w; ++v) o += wsum[v];
        if (t) {
            int a2, b2;
            pair_decode(p, K, a2, b2);
            A.gene_tp[(size_t)g * A.P + o + lanes_below(bal)] = (u32)p | ((u32)a2 << 16) | ((u32)b2 << 24);
        }
        for (int v = 0; v < T / 64; ++v) ntested += wsum[v];
        __syncthreads();
    }
    if (tid == 0) A.gene_nt[g] = (int)ntested;
    return ntested;
}

// One ranked gene: 2048-bin histogram of its key window, bins packed into
// value buckets of < 2 * target elements (a bin of more than `target` is a
// bucket of its own), elements scattered into bucket order (keys2 / codes2
// over the gene's own range).  Buckets of <= 64 elements go to the wave
// kernel, larger ones (fat bins) to the LDS item kernel.  Every bucket gets a
// global id: its cluster histogram row in hbg, written by whoever ranks it.
__device__ void split_one_gene(const ScRankLaunch& A, int g, SplitLds& L)
{
    const int K = A.K, G = A.G;
    const int tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    const i64 base = A.gstart[g];
    const int n = (int)(A.gstart[g + 1] - base);
    const u64* key = A.keys + base;
    if (tid <= K) L.off[tid] = (int)A.coff[(size_t)A.cl_cc[tid] * G + g];
    for (int i = tid; i < SP_BINS; i += SP_T) L.hist[i] = 0;
    // tested pairs of the gene (the wave kernel holds at most 64 * A.rw_slots)
    const u32 ntested = gene_tested_pairs<SP_T>(A, g, L.wsum2);
    const bool waves_ok = ntested <= (A.rw_slots >= RW_SLOTS_MAX ? (u32)RW_PAIRS_MAX : 64u * (u32)A.rw_slots);
    // the gene's keys stay in registers when they fit (SP_KPT per thread);
    // larger genes re-read each chunk in every pass (from L2)
    u64 kr[SP_KPT];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int q = 0; q < SP_KPT; ++q) {
            const int i = c0 + q * SP_T + tid;
            kr[q] = i < n ? key[i] : 0ull;
        }
    };
    load_chunk(0);
    // key range of the gene (min / max over its nonzeros)
    u64 kmn = ~0ull, kmx = 0;
    for (int c0 = 0; c0 < n; c0 += SP_CHUNK) {
        if (c0) load_chunk(c0);
#pragma unroll
        for (int q = 0; q < SP_KPT; ++q) {
            if (c0 + q * SP_T + tid < n) {
                kmn = kr[q] < kmn ? kr[q] : kmn;
                kmx = kr[q] > kmx ? kr[q] : kmx;
            }
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
    for (int v = 1; v < SP_W; ++v) {
        kmn = L.rmn[v] < kmn ? L.rmn[v] : kmn;
        kmx = L.rmx[v] > kmx ? L.rmx[v] : kmx;
    }
    const u64 range = kmx - kmn;
    const int bits = range ? 64 - __clzll((long long)range) : 0;
    const int sh = bits > 11 ? bits - 11 : 0;
    if (tid == 0) A.gkmin[g] = bits <= 64 - SCC_CODE_BITS ? kmn : ~0ull;  // wave kernel: (key - kmin) << 7 | cluster
    // ---- 1. equalized bins.  A linear 2048-bin window over the gene's whole
    // key range puts hundreds of distinct values into one bin where the values
    // crowd (at 200k cells: the count-1 band of a dense gene), and every such
    // bin cost a re-split (k_rank_resplit*: 8 ms of config D's rank stage).
    // So the linear histogram is a first look: where a bin holds more than 64
    // elements, its scan (cdf) maps a key
    // to  floor(2048 (cdf[j] + f h_j) / n)  (j its linear bin, f its place in
    // it, h_j the bin's count) -- the gene's empirical CDF, interpolated --
    // and the buckets are cut on those bins.  The map is non-decreasing in the
    // key (every operation is a correctly rounded monotone one), so a bin is a
    // key interval: equal values never straddle bins and order is kept.
    // A gene whose linear bins all hold <= 64 elements keeps them (no second pass).
    for (int c0 = 0; c0 < n; c0 += SP_CHUNK) {
        if (n > SP_CHUNK) load_chunk(c0);
#pragma unroll
        for (int q = 0; q < SP_KPT; ++q) {
            if (c0 + q * SP_T + tid < n) {
                const u32 d = (u32)((kr[q] - kmn) >> sh);
                atomicAdd(&L.hist[d], 1u);
                L.rep[d] = kr[q];
            }
        }
    }
    __syncthreads();
    const bool equalize = __syncthreads_or(L.hist[2 * tid] > 64u || L.hist[2 * tid + 1] > 64u) != 0;
    if (equalize) {
        const u32 h0 = L.hist[2 * tid], h1 = L.hist[2 * tid + 1];
        const u32 v = h0 + h1;
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum[w] = incl;
        __syncthreads();
        u32 b = incl - v;
        for (int q = 0; q < w; ++q) b += L.wsum[q];
        L.cdf[2 * tid] = b;
        L.cdf[2 * tid + 1] = b + h0;
        if (tid == SP_T - 1) L.cdf[SP_BINS] = (u32)n;
        L.hist[2 * tid] = 0;
        L.hist[2 * tid + 1] = 0;
    }
    __syncthreads();
    const double inv_w = ldexp(1.0, -sh), bin_scale = (double)SP_BINS / (double)max(n, 1);
    auto binof = [&](u64 k) -> u32 {
        const u64 x = k - kmn;
        const u32 j = (u32)(x >> sh);
        if (!equalize) return j;
        const u32 lo = L.cdf[j], h = L.cdf[j + 1] - lo;
        const double f = (double)(x - ((u64)j << sh)) * inv_w;
        const u32 d = (u32)(((double)lo + f * (double)h) * bin_scale);
        return d < SP_BINS ? d : SP_BINS - 1;
    };
    // histogram of the equalized bins (one LDS atomic per element; any key of
    // a bin is kept as its representative)
    for (int c0 = 0; c0 < n && equalize; c0 += SP_CHUNK) {
        if (n > SP_CHUNK) load_chunk(c0);
#pragma unroll
        for (int q = 0; q < SP_KPT; ++q) {
            if (c0 + q * SP_T + tid < n) {
                const u32 d = binof(kr[q]);
                atomicAdd(&L.hist[d], 1u);
                L.rep[d] = kr[q];
            }
        }
    }
    __syncthreads();
    // ---- 2. exclusive scan of the bins (2 per thread)
    {
        const u32 h0 = L.hist[2 * tid], h1 = L.hist[2 * tid + 1];
        const u32 v = h0 + h1;
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum[w] = incl;
        __syncthreads();
        u32 b = incl - v;
        for (int q = 0; q < w; ++q) b += L.wsum[q];
        L.excl[2 * tid] = b;
        L.excl[2 * tid + 1] = b + h0;
    }
    __syncthreads();
    // ---- 3. buckets: runs of bins with equal floor(excl / target); a bin of
    // more than `target` elements is a bucket of its own
    const u32 target = (u32)A.wave_target;
    {
        u32 st[2];
        for (int q = 0; q < 2; ++q) {
            const int d = 2 * tid + q;
            const bool fat = L.hist[d] > target;
            const bool pfat = d > 0 && L.hist[d - 1] > target;
            st[q] = (d == 0) || fat || pfat || (L.excl[d] / target != L.excl[d - 1] / target);
        }
        const u32 v = st[0] + st[1];
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum2[w] = incl;
        __syncthreads();
        u32 b = incl - v;
        for (int q = 0; q < w; ++q) b += L.wsum2[q];
        L.bid[2 * tid] = b + st[0] - 1;
        L.bid[2 * tid + 1] = b + st[0] + st[1] - 1;
        if (st[0]) L.boff[b] = L.excl[2 * tid];
        if (st[1]) L.boff[b + st[0]] = L.excl[2 * tid + 1];
        if (tid == SP_T - 1) {
            L.nb = (int)(b + v);
            L.boff[b + v] = (u32)n;
            L.bk0 = atomicAdd(&rk_cnt(A, RK_CNT_BUCKET_IDS), (int)(b + v));
            A.gene_bk[2 * g] = L.bk0;
            A.gene_bk[2 * g + 1] = (int)(b + v);
        }
    }
    __syncthreads();
    const int nb = L.nb, bk0 = L.bk0;
    for (int q = tid; q < nb; q += SP_T) {
        L.bcur[q] = L.boff[q];
        L.bdiff[q] = 0;
    }
    __syncthreads();
    // ---- 4. scatter into bucket order (keys2 / codes2 over the gene's own range);
    // the order inside a bucket is arbitrary (its ranker sorts by key and cluster).
    // A gene of one register chunk is ordered in LDS and leaves as whole lines
    // (scattered 8-byte / 1-byte stores wrote each line several times over:
    // 3.8x the keys2 + codes2 bytes at config D).  A larger gene goes in two
    // levels: its buckets grouped into super-buckets (runs of buckets whose
    // starts share floor(offset / SP_SUP); a bucket of more than SP_SUP values
    // alone, so a group holds < SP_CHUNK), the values scattered into group
    // order (a chunk's values land in a few dozen runs: whole lines), then each
    // group of two or more buckets reloaded, ordered in LDS and written back.
    // The one-level scatter's scattered stores were ~2/3 of a large gene's
    // split time (8.4 -> 3.0 cycles per value without them at config D).
    // A gene past SP_NSUP groups: the one-level scatter.
    const bool staged = n <= SP_CHUNK;
    u64* stk = (u64*)((char*)&L + kSplitStageOff);
    u8* stc = (u8*)(stk + SP_CHUNK);
    // group tables over the bin tables the layout no longer needs (hist and
    // excl, adjacent: 4096 words): the bins' group ids in the first 1024, then
    // three [SP_NSUP + 1] tables
    static_assert(offsetof(SplitLds, excl) == offsetof(SplitLds, hist) + sizeof(u32) * SP_BINS, "hist | excl");
    static_assert(SP_BINS / 2 + 3 * (SP_NSUP + 1) <= 2 * SP_BINS, "group tables");
    unsigned short* supbin = (unsigned short*)L.hist;  // [SP_BINS] group of each bin
    u32* sbeg = L.hist + SP_BINS / 2;                  // [SP_NSUP + 1] group starts (offsets)
    u32* sbk = sbeg + (SP_NSUP + 1);                   // [SP_NSUP + 1] first bucket of each group
    u32* scur = sbk + (SP_NSUP + 1);                   // [SP_NSUP] group cursors
    bool two = !staged;
    if (two) {
        // group starts over the bins, 2 per thread (the bucket rule's scan)
        auto big = [&](u32 b) { return L.boff[b + 1] - L.boff[b] > (u32)SP_SUP; };
        u32 st[2], bq[2];
        for (int q = 0; q < 2; ++q) {
            const int d = 2 * tid + q;
            const u32 b = L.bid[d];
            bq[q] = b;
            const u32 bp = d > 0 ? L.bid[d - 1] : b;
            st[q] = (d == 0) || (bp != b && (big(b) || big(bp) || L.boff[b] / SP_SUP != L.boff[bp] / SP_SUP));
        }
        const u32 v = st[0] + st[1];
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.wsum2[w] = incl;
        __syncthreads();
        u32 sb = incl - v;
        for (int q = 0; q < w; ++q) sb += L.wsum2[q];
        const u32 ns = [&] {
            u32 t = 0;
            for (int q = 0; q < SP_W; ++q) t += L.wsum2[q];
            return t;
        }();
        if (ns <= SP_NSUP) {
            for (int q = 0; q < 2; ++q) {
                sb += st[q];
                if (st[q]) {
                    sbeg[sb - 1] = L.boff[bq[q]];
                    sbk[sb - 1] = bq[q];
                    scur[sb - 1] = L.boff[bq[q]];
                }
            }
            // (the writes above use the per-thread running index; store the bin's group after)
        }
        __syncthreads();  // every thread has read the bin tables' old contents (hist / excl no longer read)
        if (ns <= SP_NSUP) {
            u32 sb2 = incl - v;
            for (int q = 0; q < w; ++q) sb2 += L.wsum2[q];
            for (int q = 0; q < 2; ++q) {
                sb2 += st[q];
                supbin[2 * tid + q] = (unsigned short)(sb2 - 1);
            }
            if (tid == 0) {
                sbeg[ns] = (u32)n;
                sbk[ns] = (u32)nb;
            }
        }
        two = ns <= SP_NSUP;  // (block-uniform)
        if (tid == 0) L.nsup = (int)ns;
        __syncthreads();
    }
    if (two) {  // first level: straight to the group cursors
        // (staging each chunk in LDS by group first, for whole-line stores,
        // measured no faster at config D for genes from 32k, 64k or 128k values)
        for (int c0 = 0; c0 < n; c0 += SP_CHUNK) {
            load_chunk(c0);
            int a = 0;
#pragma unroll
            for (int q = 0; q < SP_KPT; ++q) {
                const int i = c0 + q * SP_T + tid;
                if (i < n) {
                    while (a + 1 < K && L.off[a + 1] <= i) ++a;
                    const u64 k = kr[q];
                    const u32 d = binof(k);
                    const u32 pos = atomicAdd(&scur[supbin[d]], 1u);
                    A.keys2[base + pos] = k;
                    A.codes2[base + pos] = (u8)a;
                    if (k != L.rep[d]) L.bdiff[L.bid[d]] = 1;
                }
            }
        }
    }
    for (int c0 = 0; c0 < n && !two; c0 += SP_CHUNK) {
        if (n > SP_CHUNK) load_chunk(c0);
        int a = 0;
#pragma unroll
        for (int q = 0; q < SP_KPT; ++q) {
            const int i = c0 + q * SP_T + tid;
            if (i < n) {
                while (a + 1 < K && L.off[a + 1] <= i) ++a;
                const u64 k = kr[q];
                const u32 d = binof(k);
                const u32 bk = L.bid[d];
                const u32 pos = atomicAdd(&L.bcur[bk], 1u);
                if (staged) {
                    stk[pos] = k;
                    stc[pos] = (u8)a;
                } else if (A.dbg != 10) {  // (SCC_RW_DEBUG=10: timing cut, no unstaged stores; results invalid)
                    A.keys2[base + pos] = k;
                    A.codes2[base + pos] = (u8)a;
                }
                if (k != L.rep[d]) L.bdiff[bk] = 1;
            }
        }
    }
    __syncthreads();
    if (staged) {
        for (int i = tid; i < n; i += SP_T) {
            A.keys2[base + i] = stk[i];
            A.codes2[base + i] = stc[i];
        }
    }
    if (two) {  // second level: each group of >= 2 buckets ordered in LDS, in place
        const int ns = L.nsup;
        for (int sg = 0; sg < ns; ++sg) {
            if (sbk[sg + 1] - sbk[sg] < 2) continue;  // one bucket: in place already (block-uniform)
            const u32 o0 = sbeg[sg], m = sbeg[sg + 1] - o0;  // m < SP_CHUNK
            if (m == 0) continue;
            u64 kv[SP_KPT];
            u8 cv[SP_KPT];
#pragma unroll
            for (int q = 0; q < SP_KPT; ++q) {  // clamped unconditional loads (all in flight)
                const u32 j = (u32)(q * SP_T + tid);
                const u32 jc = j < m ? j : m - 1;
                kv[q] = A.keys2[base + o0 + jc];
                cv[q] = A.codes2[base + o0 + jc];
            }
#pragma unroll
            for (int q = 0; q < SP_KPT; ++q) {
                if ((u32)(q * SP_T + tid) < m) {
                    const u32 d = binof(kv[q]);
                    const u32 p = atomicAdd(&L.bcur[L.bid[d]], 1u) - o0;
                    stk[p] = kv[q];
                    stc[p] = cv[q];
                }
            }
            __syncthreads();
            for (u32 j = tid; j < m; j += SP_T) {
                A.keys2[base + o0 + j] = stk[j];
                A.codes2[base + o0 + j] = stc[j];
            }
            __syncthreads();
        }
    }
    // ---- 5. one work unit per bucket (empty buckets: a zero histogram row).
    // Wave buckets and re-split parents are reserved once per gene (one global
    // atomic each, not one per bucket) and placed with LDS cursors.
    auto kind = [&](int q) {  // 0 none, 1 wave bucket, 2 re-split parent, 3 LDS item
        const int c = (int)(L.boff[q + 1] - L.boff[q]);
        if (c <= 0) return 0;
        const bool ties_only = c > 64 && !L.bdiff[q];
        if ((c <= 64 || ties_only) && waves_ok) return 1;
        if (waves_ok && c <= RS_CAP && A.fatbk) return 2;
        return 3;
    };
    if (tid == 0) {
        L.nfat = 0;
        L.nwav = 0;
    }
    __syncthreads();
    for (int q = tid; q < nb; q += SP_T) {
        const int k = kind(q);
        if (k == 1) atomicAdd(&L.nwav, 1);
        if (k == 2) atomicAdd(&L.nfat, 1);
    }
    __syncthreads();
    if (tid == 0) {
        L.wav0 = L.nwav ? atomicAdd(&rk_cnt(A, RK_CNT_WAVE_SLOTS), L.nwav) : 0;
        L.fat0 = -1;
        if (L.nfat) {
            const int f0 = atomicAdd(&rk_cnt(A, RK_CNT_FAT), L.nfat);
            if (f0 + L.nfat <= A.fat_cap) {
                L.fat0 = f0;
                A.fatg[atomicAdd(&rk_cnt(A, RK_CNT_FAT_GENES), 1)] = int4{g, f0, L.nfat, 0};
            }
        }
        L.nfat = 0;
        L.nwav = 0;
    }
    __syncthreads();
    for (int q = tid; q < nb; q += SP_T) {
        const int c = (int)(L.boff[q + 1] - L.boff[q]);
        const int bid = bk0 + q;
        const int k = kind(q);
        if (k == 0) {
            for (int k2 = 0; k2 < K; ++k2) A.hbg[(size_t)bid * K + k2] = 0;
            continue;
        }
        // a bucket of one repeated key (a fat bin of ties): closed form in the wave kernel
        const bool ties_only = c > 64 && !L.bdiff[q];
        const ScRankItem itm{base + L.boff[q], c, g, ties_only ? 2 : 1, bid};
        if (k == 1) {
            A.sbuckets[L.wav0 + atomicAdd(&L.nwav, 1)] = itm;
        } else if (k == 2 && L.fat0 >= 0) {
            // > 64 distinct values in one bin: re-split on a finer window (k_rank_resplit)
            A.fatbk[L.fat0 + atomicAdd(&L.nfat, 1)] = itm;
        } else {
            const int cls = (c <= A.cap_s) ? 0 : ((c <= A.cap_m) ? 1 : 2);
            A.items[(size_t)cls * A.item_cap + atomicAdd(&rk_cnt(A, RK_CNT_ITEMS0 + cls), 1)] = itm;
        }
    }
    __syncthreads();
}

// SCC_RW_DEBUG=9: per split gene (stored values, cycles) of the first
// SPLIT_DIAG_MAX genes, printed as a distribution (scc_rank_split_diag)
#define SPLIT_DIAG_MAX 65536
__device__ unsigned long long g_split_diag[SPLIT_DIAG_MAX][2];

__global__ void __launch_bounds__(SP_T) k_rank_split(ScRankLaunch A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SplitLds& L = *(SplitLds*)smem;
    const int cnt = split_count(A), nbig = rk_cnt(A, RK_CNT_BIG_GENES);
    for (;;) {  // genes from a queue (their sizes vary by orders of magnitude)
        if (threadIdx.x == 0) L.next = atomicAdd(&rk_cnt(A, RK_CNT_SPLIT_CURSOR), 1);
        __syncthreads();
        const int i = L.next;
        if (i >= cnt) break;
        const u64 t0 = A.dbg >= 9 ? __builtin_amdgcn_s_memtime() : 0;
        split_one_gene(A, split_gene_at(A, nbig, i), L);
        if (A.dbg >= 9 && threadIdx.x == 0 && i < SPLIT_DIAG_MAX) {
            const int g = split_gene_at(A, nbig, i);
            g_split_diag[i][0] = (unsigned long long)(A.gstart[g + 1] - A.gstart[g]);
            g_split_diag[i][1] = __builtin_amdgcn_s_memtime() - t0;
        }
    }
}

extern "C" void scc_rank_split_diag(hipStream_t st, int ngenes)
{
    static unsigned long long h[SPLIT_DIAG_MAX][2];
    const int n = ngenes < SPLIT_DIAG_MAX ? ngenes : SPLIT_DIAG_MAX;
    if (n <= 0 || hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpyFromSymbol(h, HIP_SYMBOL(g_split_diag), sizeof(unsigned long long) * 2 * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return;
    std::vector<int> ix(n);
    for (int i = 0; i < n; ++i) ix[i] = i;
    std::sort(ix.begin(), ix.end(), [&](int a, int b) { return h[a][1] > h[b][1]; });
    unsigned long long tot = 0, totn = 0;
    for (int i = 0; i < n; ++i) {
        tot += h[i][1];
        totn += h[i][0];
    }
    fprintf(stderr, "[scc split diag] genes %d values %llu cycles %llu (mean %.0f per gene, %.1f per value); slowest:", n,
            totn, tot, (double)tot / n, (double)tot / std::max(1ull, totn));
    for (int q = 0; q < std::min(n, 12); ++q) fprintf(stderr, " %llu/%llu", h[ix[q]][0], h[ix[q]][1]);
    fprintf(stderr, "\n");
}

extern "C" size_t scc_rank_split_lds(int K)
{
    (void)K;
    return kSplitStageOff + (size_t)SP_CHUNK * (sizeof(u64) + 1);
}

// The value-order route's bucket list, in place of the split: each classified
// gene's tested pairs, then one wave bucket per precomputed cut of its sorted
// segment (base: an offset into vcell; src 2: one tie group of more than 64),
// contiguous and in value order in sbuckets and hbg as k_rank_cross expects.
// A workgroup takes VL_G consecutive classified genes: one global atomic
// reserves their buckets' ids and list slots together (an atomic per gene, all
// on one counter, queued behind each other: 46 us at config B), then each
// wave takes genes of its own.
#define VL_G 8
__global__ void __launch_bounds__(256) k_rank_vorder_list(ScRankLaunch A)
{
    __shared__ int sg[VL_G], sq0[VL_G], snb[VL_G], sat[VL_G];
    const int tid = threadIdx.x, lane = tid & 63, wv = scc_wave_id();
    const int cnt = split_count(A), nbig = rk_cnt(A, RK_CNT_BIG_GENES);
    for (int i0 = blockIdx.x * VL_G; i0 < cnt; i0 += gridDim.x * VL_G) {
        const int ng = min(VL_G, cnt - i0);
        if (tid < ng) {
            const int g = split_gene_at(A, nbig, i0 + tid);
            const u32 q0 = A.vbk_ptr[g];
            sg[tid] = g;
            sq0[tid] = (int)q0;
            snb[tid] = (int)(A.vbk_ptr[g + 1] - q0);
        }
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int j = 0; j < ng; ++j) {
                sat[j] = tot;
                tot += snb[j];
            }
            // (bucket ids and list slots run together on this route: one bucket, one slot)
            const int at = atomicAdd(&rk_cnt(A, RK_CNT_WAVE_SLOTS), tot);
            atomicAdd(&rk_cnt(A, RK_CNT_BUCKET_IDS), tot);
            for (int j = 0; j < ng; ++j) sat[j] += at;
        }
        __syncthreads();
        for (int j = wv; j < ng; j += 4) {
            const int g = sg[j], nb = snb[j], bk0 = sat[j];
            const u32 q0 = (u32)sq0[j];
            const i64 base = A.vgptr[g];
            const int n = (int)(A.vgptr[g + 1] - base);
            gene_tested_pairs<64>(A, g, nullptr);
            if (lane == 0) {
                A.gene_bk[2 * g] = bk0;
                A.gene_bk[2 * g + 1] = nb;
            }
            for (int q = lane; q < nb; q += 64) {
                const u32 w0 = A.vbk[q0 + q];
                const int s = (int)(w0 & 0x7fffffffu);
                const int e = q + 1 < nb ? (int)(A.vbk[q0 + q + 1] & 0x7fffffffu) : n;
                if (bk0 + q < A.bucket_cap)
                    A.sbuckets[bk0 + q] = ScRankItem{base + s, e - s, g, (w0 >> 31) ? 2 : 1, bk0 + q};
            }
        }
        __syncthreads();
    }
}

extern "C" hipError_t scc_launch_rank_vorder_list(const ScRankLaunch* L, int grid, hipStream_t st)
{
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rank_vorder_list, dim3(grid), dim3(256), 0, st, *L);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_rank_split(const ScRankLaunch* L, int grid, hipStream_t st)
{
    if (grid <= 0) return hipSuccess;
    const size_t lds = scc_rank_split_lds(L->K);
    scc_set_lds((const void*)k_rank_split, (int)lds);
    hipLaunchKernelGGL(k_rank_split, dim3(grid), dim3(SP_T), lds, st, *L);
    return hipGetLastError();
}
