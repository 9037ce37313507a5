// scc_rank_rest.hip — the one-vs-rest Wilcoxon rank kernel (scc_de_markers).
//
// For every cluster a the test is "cluster a against every other kept cell"
// (the reference's ComputePairWiseDE with cells.2 = the rest, Fast:73-355).
// a and the rest always make up the whole selection, so one sort of a gene's
// kept nonzeros serves all K tests: with below(i) the nonzeros strictly below
// x_i (of any cluster) and n_t(i) the size of i's tie group,
//
//   R2[a] = sum_{i in a} (2 below(i) + n_t(i))       (twice the midrank sum - nz_a)
//   T     = sum_i (n_t(i)^2 - 1) = sum_t (n_t^3 - n_t)
//
// and, because the same sum inside cluster a alone is nz_a^2,
//
//   2 S_a + E_a = R2[a] - nz_a^2
//
// (S_a = #{i in a, j in rest: x_j < x_i}, E_a = sum_t c_a(t) (n_t - c_a(t)):
// include/scc.h).  One integer accumulator per (cluster, gene) and one per gene
// (K statistics per gene, not K (K - 1) / 2), every sum an exact integer
// whatever the order.  k_rest_test (scc_select.hip) adds the implicit zero group
// in closed form.
//
// k_rank_rest: one workgroup per gene (the ingest leaves a gene's nonzeros
// grouped by cluster).
//   n <= CAP: the gene is sorted by a bitonic network in LDS, the cluster code
//     as payload; below / n_t of an element are the bounds of its key's run,
//     two binary searches of the sorted LDS copy.
//   n > CAP: the gene is first cut into value-range buckets.  CAP keys sampled
//     at even strides are sorted in LDS; every (CAP / nb)-th of them is a
//     splitter (nb buckets of ~0.4 CAP expected elements, at most RR_MAXB); a
//     count pass and a scatter pass move the keys and codes to keys2 / codes2
//     in bucket order.  Bucket b holds the keys in (splitter b - 1, splitter b],
//     so equal keys never straddle buckets and below(i) = the bucket's start +
//     the position inside the sorted bucket: each bucket is sorted and searched
//     in LDS like a short gene, no search crosses buckets.  A bucket that still
//     exceeds CAP (one value repeated more than CAP times, or a sample that
//     missed a crowded stretch) is sorted in chunks of CAP written back in place,
//     and each of its elements searches every chunk of the bucket in global
//     memory.
// Cost per element: log^2 of the sorted size compare-exchanges in LDS, two
// binary searches in LDS, and for n > CAP two more reads of the key with a
// search of the <= 255 splitters.  A gene is one workgroup's work however long
// it is.  The K sums live in LDS and are flushed once per gene with plain
// stores, [cluster][gene]: the layout k_rest_test and the selection read
// coalesced over genes.
#include "scc_common.hpp"
#include "scc_kernels.hpp"

#define RR_ACC (SCC_MAX_K + 1)  // K cluster sums and the gene's tie term
#define RR_MAXB 256             // value-range buckets of a long gene

template <int CAP>
constexpr size_t rr_lds_bytes()
{
    return sizeof(u64) * CAP + sizeof(u64) * RR_ACC + sizeof(int) * (RR_ACC + 1) + sizeof(int) * (2 * RR_MAXB + 2) +
           CAP;
}

// first index in [0, n) with a[idx] >= k (UPPER: > k)
template <bool UPPER>
__device__ inline int rr_bound(const u64* a, int n, u64 k)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u64 v = a[mid];
        const bool right = UPPER ? (v <= k) : (v < k);
        lo = right ? mid + 1 : lo;
        hi = right ? hi : mid;
    }
    return lo;
}

// [lo, hi): the run of k in the sorted a[0, n) (empty at lo when k is absent)
__device__ inline void rr_range(const u64* a, int n, u64 k, int& lo, int& hi)
{
    lo = rr_bound<false>(a, n, k);
    hi = (lo < n && a[lo] == k) ? rr_bound<true>(a, n, k) : lo;
}

// bitonic sort of sk[0, M) ascending, sc the payload (M a power of two; ends with a barrier)
template <int T>
__device__ inline void rr_sort(u64* sk, u8* sc, int M, int tid)
{
    for (int kk = 2; kk <= M; kk <<= 1)
        for (int j = kk >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < (M >> 1); i += T) {
                const int l = 2 * i - (i & (j - 1)), r = l + j;
                const u64 a = sk[l], b = sk[r];
                const bool up = (l & kk) == 0;
                if ((a > b) == up && a != b) {
                    sk[l] = b, sk[r] = a;
                    const u8 t = sc[l];
                    sc[l] = sc[r], sc[r] = t;
                }
            }
            __syncthreads();
        }
}

// the network's size for m elements: a power of two >= max(m, 64)
__device__ inline int rr_pow2(int m)
{
    int M = 64;
    while (M < m) M <<= 1;
    return M;
}

// the sorted sk[0, m) / sc[0, m) hold the elements at ranks [base, base + m) of the gene
template <int T>
__device__ inline void rr_accum_lds(const u64* sk, const u8* sc, int m, u64 base, u64* acc, int K, u64& tsum, int tid)
{
    for (int i = tid; i < m; i += T) {
        int l0, h0;
        rr_range(sk, m, sk[i], l0, h0);
        const u64 nt = (u64)(h0 - l0);
        atomicAdd(&acc[min((int)sc[i], K)], 2 * (base + (u64)l0) + nt);  // (a padding code: non-finite input, the run fails)
        tsum += nt * nt - 1;
    }
}

template <int CAP, int T>
__global__ void __launch_bounds__(T) k_rank_rest(ScRestRankLaunch A, int n_lo, int n_hi)
{
    extern __shared__ __align__(16) unsigned char rr_smem[];
    u64* sk = (u64*)rr_smem;              // [CAP] keys being sorted
    u64* acc = sk + CAP;                  // [RR_ACC]
    int* off = (int*)(acc + RR_ACC);      // [K + 1] cluster starts inside the gene's segment
    int* boff = off + RR_ACC + 1;         // [RR_MAXB + 1] bucket starts of a long gene
    int* bcur = boff + RR_MAXB + 1;       // [RR_MAXB + 1] bucket counts, then scatter cursors
    u8* sc = (u8*)(bcur + RR_MAXB + 1);   // [CAP] cluster codes
    const int g = blockIdx.x, K = A.K, G = A.G, tid = threadIdx.x;
    const i64 base = A.gstart[g];
    const int n = (int)(A.gstart[g + 1] - base);
    if (n < n_lo || n > n_hi) return;  // another launch's size class
    if (!A.all) {  // ranked iff at least one cluster tests the gene
        int t = 0;
        for (int a = tid; a < K; a += T) t |= A.flags[(size_t)a * G + g] & 1;
        if (!__syncthreads_or(t)) return;
    }
    for (int a = tid; a <= K; a += T) {
        off[a] = min((int)A.coff[(size_t)A.cl_cc[a] * G + g], n);
        acc[a] = 0;
    }
    __syncthreads();
    const u64* key = A.keys + base;
    auto code_at = [&](int pos) {  // the cluster whose range holds position pos of the segment
        int lo = 0, hi = K;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= pos) lo = mid; else hi = mid;
        }
        return (u8)lo;
    };
    u64 tsum = 0;  // this thread's part of the tie term: one LDS add per wave, not per element
    if (n <= CAP) {
        const int M = rr_pow2(n);
        for (int i = tid; i < M; i += T) {
            const bool in = i < n;
            sk[i] = in ? key[i] : ~0ull;  // padding sorts last (no finite value has this key)
            sc[i] = in ? code_at(i) : (u8)0xff;
        }
        __syncthreads();
        rr_sort<T>(sk, sc, M, tid);
        rr_accum_lds<T>(sk, sc, n, 0, acc, K, tsum, tid);
    } else {
        u64* gk = A.keys2 + base;  // the gene in bucket order
        u8* gc = A.codes2 + base;
        // splitters: CAP keys at even strides, sorted; splitter b = sk[(b + 1) CAP / nb]
        const int nb = min(RR_MAXB, (int)(((i64)n * 5 + 2 * CAP - 1) / (2 * CAP)));  // ~0.4 CAP per bucket
        for (int i = tid; i < CAP; i += T) {
            sk[i] = key[(int)(((i64)i * n) / CAP)];
            sc[i] = 0;
        }
        for (int b = tid; b <= RR_MAXB; b += T) bcur[b] = 0;
        __syncthreads();
        rr_sort<T>(sk, sc, CAP, tid);
        auto bucket_of = [&](u64 k) {  // the first b with splitter b >= k (nb - 1: above every splitter)
            int lo = 0, hi = nb - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sk[(int)(((i64)(mid + 1) * CAP) / nb)] < k) lo = mid + 1; else hi = mid;
            }
            return lo;
        };
        for (int i = tid; i < n; i += T) atomicAdd(&bcur[bucket_of(key[i])], 1);
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int b = 0; b < nb; ++b) {
                const int c = bcur[b];
                boff[b] = run;
                bcur[b] = run;
                run += c;
            }
            boff[nb] = run;  // == n
        }
        __syncthreads();
        for (int i = tid; i < n; i += T) {
            const u64 k = key[i];
            const int pos = atomicAdd(&bcur[bucket_of(k)], 1);
            gk[pos] = k;
            gc[pos] = code_at(i);
        }
        __syncthreads();  // (orders the workgroup's global stores before its loads below)
        for (int b = 0; b < nb; ++b) {
            const int b0 = boff[b], m = boff[b + 1] - b0;
            if (m <= 0) continue;  // (uniform: boff is shared)
            if (m <= CAP) {
                const int M = rr_pow2(m);
                for (int i = tid; i < M; i += T) {
                    const bool in = i < m;
                    sk[i] = in ? gk[b0 + i] : ~0ull;
                    sc[i] = in ? gc[b0 + i] : (u8)0xff;
                }
                __syncthreads();
                rr_sort<T>(sk, sc, M, tid);
                rr_accum_lds<T>(sk, sc, m, (u64)b0, acc, K, tsum, tid);
                __syncthreads();  // the next bucket overwrites sk / sc
                continue;
            }
            // a bucket beyond CAP: chunks of CAP sorted in place, every chunk searched
            const int nchunk = (m + CAP - 1) / CAP;
            for (int c = 0; c < nchunk; ++c) {
                const int c0 = b0 + c * CAP, mc = min(CAP, b0 + m - c0);
                const int M = rr_pow2(mc);
                for (int i = tid; i < M; i += T) {
                    const bool in = i < mc;
                    sk[i] = in ? gk[c0 + i] : ~0ull;
                    sc[i] = in ? gc[c0 + i] : (u8)0xff;
                }
                __syncthreads();
                rr_sort<T>(sk, sc, M, tid);
                for (int i = tid; i < mc; i += T) {
                    gk[c0 + i] = sk[i];
                    gc[c0 + i] = sc[i];
                }
                __syncthreads();  // the next chunk overwrites sk / sc; orders the stores before the loads below
            }
            for (int i = tid; i < m; i += T) {
                const u64 k = gk[b0 + i];
                u64 lo = (u64)b0, hi = (u64)b0;
                for (int c = 0; c < nchunk; ++c) {
                    const int c0 = b0 + c * CAP, mc = min(CAP, b0 + m - c0);
                    int l0, h0;
                    rr_range(gk + c0, mc, k, l0, h0);
                    lo += (u64)l0;
                    hi += (u64)h0;
                }
                const u64 nt = hi - lo;
                atomicAdd(&acc[min((int)gc[b0 + i], K)], 2 * lo + nt);
                tsum += nt * nt - 1;
            }
        }
    }
    tsum = u64_wave_sum(tsum);
    if ((tid & 63) == 0) atomicAdd(&acc[K], tsum);
    __syncthreads();
    for (int a = tid; a < K; a += T) A.accR[(size_t)a * G + g] = acc[a];
    if (tid == 0) A.accT[g] = acc[K];
}

#define RR_CAP_S 2048
#define RR_CAP_L 8192

extern "C" hipError_t scc_launch_rank_rest(const ScRestRankLaunch* L, hipStream_t st)
{
    if (L->G <= 0) return hipSuccess;
    if (L->K < 1 || L->K > SCC_MAX_K) return hipErrorInvalidValue;
    auto ks = k_rank_rest<RR_CAP_S, 256>;
    auto kl = k_rank_rest<RR_CAP_L, 1024>;
    hipError_t e = scc_set_lds((const void*)ks, rr_lds_bytes<RR_CAP_S>());
    if (e != hipSuccess) return e;
    e = scc_set_lds((const void*)kl, rr_lds_bytes<RR_CAP_L>());
    if (e != hipSuccess) return e;
    // the long genes first: they run longest
    hipLaunchKernelGGL(kl, dim3(L->G), dim3(1024), rr_lds_bytes<RR_CAP_L>(), st, *L, RR_CAP_S + 1, 0x7fffffff);
    hipLaunchKernelGGL(ks, dim3(L->G), dim3(256), rr_lds_bytes<RR_CAP_S>(), st, *L, 0, RR_CAP_S);
    return hipGetLastError();
}
