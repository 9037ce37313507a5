// scc_rank_item.hip — rank stage: one workgroup per work item.
//
// An item is a value bucket too large for a wave that the re-split did not
// take: more than RS_CAP values, a gene whose tested pairs pass what the wave
// kernels hold, or a parent met when a re-split list was full (shared
// definitions and the stage's arithmetic: scc_rank_dev.hpp).
//   k_rank_item    stable LSD radix sort (8-bit digits, wave match-ranking, no
//                  atomic conflicts) on a 32-bit window of the orderable key
//                  with an exact fix-up of windows that merged distinct
//                  doubles; the sorted positions partitioned by cluster; for
//                  every tested pair (a, b) the within-item count
//                  #{x in a, y in b: x > y} by binary searches of the smaller
//                  cluster's positions in the larger's; tie groups (runs of
//                  equal values) give E_ab, X_ab and F_a.  It also writes the
//                  item's cluster histogram row (hbg) for the cross terms.
// Three instances by item size (RK_CNT_ITEMS0 + class): class 0 (256 threads)
// and class 1 (512) keep the window, indices and codes in LDS, class 2 (1024)
// keeps every per-element array in HBM scratch.  An item's tested-pair tables
// follow the fixed state in LDS, or live in HBM when they pass 24 KB
// (scc_rank_tables_global: many tested pairs per gene, K > ~40).
// Host side: the LDS sizing the runtime plans capacities with
// (scc_rank_item_lds, scc_rank_item_cap) and scc_launch_rank_items.
#include "scc_rank_dev.hpp"

#include <cstddef>
#include <type_traits>

// ===================================================================== radix
// LDS block state of the radix passes (W waves)
template <int W>
struct RadixLds {
    u32 hist[W * 256];
    u32 dtot[256 + W];
};

// One stable LSD pass of the digit dig(id) (< 2^BITS, BITS <= 8): in -> out.
// Each wave owns a contiguous range and per-(wave, digit) counters; inside a
// 64-element tile equal digits are ranked by lane (match by ballots), so one
// leader lane per distinct digit touches the counter: no LDS atomic ever
// conflicts.  Two tiles are in flight per wave; the returning adds of the
// scatter execute in tile order, which keeps the pass stable.
template <int W, int BITS, class IX, class DIG>
__device__ void radix_pass(DIG dig, const IX* in, IX* out, int n, RadixLds<W>& L)
{
    constexpr int U = 2;
    const int tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    const int R = (((n + W - 1) / W) + 63) & ~63;
    const int lo = min(n, w * R), hi = min(n, lo + R);
    u32* hw = L.hist + w * 256;
    for (int d = lane; d < 256; d += 64) hw[d] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int i0 = lo; i0 < hi; i0 += 64 * U) {
        u32 d[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 64 * u + lane;
            ok[u] = i < hi;
            d[u] = ok[u] ? dig(in[i]) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 peers = match_bits<BITS>(d[u], __ballot(ok[u]));
            if (ok[u] && lanes_below(peers) == 0)
                __hip_atomic_fetch_add(&hw[d[u]], (u32)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
    __syncthreads();
    u32 tot = 0, incl = 0;
    if (tid < 256) {
        u32 c[W];
#pragma unroll
        for (int v = 0; v < W; ++v) c[v] = L.hist[v * 256 + tid];
        u32 s = 0;
#pragma unroll
        for (int v = 0; v < W; ++v) {
            L.hist[v * 256 + tid] = s;
            s += c[v];
        }
        tot = s;
        incl = s;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.dtot[256 + (tid >> 6)] = incl;
    }
    __syncthreads();
    if (tid < 256) {
        u32 base = incl - tot;
        for (int v = 0; v < (tid >> 6); ++v) base += L.dtot[256 + v];
#pragma unroll
        for (int v = 0; v < W; ++v) L.hist[v * 256 + tid] += base;
    }
    __syncthreads();
    for (int i0 = lo; i0 < hi; i0 += 64 * U) {
        u32 d[U];
        IX id[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 64 * u + lane;
            ok[u] = i < hi;
            id[u] = ok[u] ? in[i] : (IX)0;
            d[u] = ok[u] ? dig(id[u]) : 0u;
        }
        u32 b[U], rank[U];
        int leader[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 peers = match_bits<BITS>(d[u], __ballot(ok[u]));
            rank[u] = lanes_below(peers);
            leader[u] = __builtin_ctzll(peers ? peers : 1ull);
            b[u] = 0;
            if (ok[u] && rank[u] == 0)
                b[u] = __hip_atomic_fetch_add(&hw[d[u]], (u32)__popcll(peers), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32 bb = (u32)__shfl((int)b[u], leader[u], 64);
            if (ok[u]) out[bb + rank[u]] = id[u];
        }
    }
    __syncthreads();
}

// exact order of one mixed run (length <= 64) by (key, cluster, index): one wave
template <class KP, class IX>
__device__ void wave_sort_run(KP key, const u8* code, IX* ix, int s, int len)
{
    const int lane = threadIdx.x & 63;
    u64 k = ~0ull;
    u32 id = 0xffffffffu;
    if (lane < len) {
        id = (u32)ix[s + lane];
        k = key[id];
    }
    // secondary key: cluster code above the index (ties of equal doubles keep cluster order)
    u64 k2 = (lane < len) ? (((u64)code[id] << 32) | id) : ~0ull;
    for (int size = 2; size <= 64; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const u64 ok = shfl_xor_u64(k, stride);
            const u64 ok2 = shfl_xor_u64(k2, stride);
            const bool up = (lane & size) == 0 || size == 64;
            const bool lower = (lane & stride) == 0;
            const bool other_less = (ok < k) || (ok == k && ok2 < k2);
            const bool take = (lower == up) ? other_less : !other_less;
            if (take) {
                k = ok;
                k2 = ok2;
            }
        }
    }
    if (lane < len) ix[s + lane] = (IX)(u32)k2;
}

// ===================================================================== item
#define RK_RUNS 256

template <int W>
struct ItemLds {
    RadixLds<W> rx;
    u32 m[SCC_MAX_K];       // nonzeros per cluster in this item
    u32 po[SCC_MAX_K + 1];  // position-list offsets
    u64 F[SCC_MAX_K];       // per-cluster tie term
    u64 red64[2 * W];  // min / max keys
    u32 redu[W + 1];
    int run_s[RK_RUNS], run_l[RK_RUNS];
    int nruns, flag, redo, anytie;
    int ntp, nchunk;
    u64 kmin, kmax;
    // tested pairs: packed (p | a << 16 | b << 23 | small-is-b << 30), chunk prefix
    u32 tp[1];  // dynamic tail: tp[ntp_max], cp[ntp_max + 1], eacc[ntp_max], xacc[ntp_max] (u64),
                // pmap[K * K] (u16: tested-pair slot + 1, 0 = untested)
};

__device__ inline int tp_p(u32 v) { return (int)(v & 0xffffu); }
__device__ inline int tp_a(u32 v) { return (int)((v >> 16) & 127u); }
__device__ inline int tp_b(u32 v) { return (int)((v >> 23) & 127u); }
__device__ inline bool tp_sb(u32 v) { return ((v >> 30) & 1u) != 0; }

// lower_bound of x in the ascending array s[0..len)
template <class IX>
__device__ inline u32 lower_bound_ix(const IX* s, u32 len, u32 x)
{
    u32 lo = 0;
    while (len > 0) {
        const u32 half = len >> 1;
        const bool lt = (u32)s[lo + half] < x;
        lo = lt ? lo + half + 1 : lo;
        len = lt ? len - half - 1 : half;
    }
    return lo;
}

// GLOBALMEM: every per-element array lives in HBM scratch (items too large
// for LDS); otherwise the key window, indices, codes and sorted codes are in
// LDS and the 64-bit keys stay in registers / L2.  KPT: keys per thread held
// in registers during the setup (LDS items: cap <= KPT * T).
template <int T, bool GLOBALMEM, int KPT>
__device__ void rank_one_item(const ScRankLaunch& A, const ScRankItem it, int item_no, char* smem)
{
    constexpr int W = T / 64;
    using IX = typename std::conditional<GLOBALMEM, u32, unsigned short>::type;
    const int K = A.K, P = A.P, G = A.G, g = it.gene, n = it.n;
    const int tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    ItemLds<W>& L = *(ItemLds<W>*)smem;
    // tested-pair tables: in LDS after the fixed state, or (many tested pairs,
    // e.g. K > 64) in this workgroup's slice of an HBM scratch
    char* tab = A.tp_global ? (A.tp_scr + (size_t)blockIdx.x * A.tp_scr_stride) : (char*)L.tp;
    u32* tp = (u32*)tab;
    u32* cp = tp + A.ntp_max;
    u64* eacc = (u64*)(((uintptr_t)(cp + A.ntp_max + 1) + 7) & ~(uintptr_t)7);
    u64* xacc = eacc + A.ntp_max;
    unsigned short* pmap = (unsigned short*)(xacc + A.ntp_max);
    char* big = A.tp_global ? (char*)L.tp : (char*)(pmap + K * K);
    big = (char*)(((uintptr_t)big + 15) & ~(uintptr_t)15);
    u64* const stamps = A.stamps ? A.stamps + (size_t)item_no * 8 : nullptr;
#define ISTAMP(ph)                                                                   \
    do {                                                                             \
        if (stamps && threadIdx.x == 0) stamps[ph] = __builtin_amdgcn_s_memtime(); \
    } while (0)
    ISTAMP(0);
    // ---- per-element arrays
    const u64* key = (it.src ? A.keys2 : A.keys) + it.base;  // HBM / L2
    u32* win;
    u8 *code, *sc;
    IX *ix0, *ix1;
    if (GLOBALMEM) {
        win = A.gwin + it.base;
        code = it.src ? (A.codes2 + it.base) : (A.gcode + it.base);
        sc = A.gsc + it.base;
        ix0 = (IX*)(A.gix + it.base);
        ix1 = (IX*)(A.gix + A.nnz + it.base);
    } else {
        win = (u32*)big;
        ix0 = (IX*)(win + A.cap_lds);
        ix1 = ix0 + A.cap_lds;
        code = (u8*)(ix1 + A.cap_lds);
        sc = code + A.cap_lds;
    }
    // ---- setup: every global read issued before the first barrier
    int off_r = 0;
    if (it.src == 0 && tid <= K) off_r = (int)A.coff[(size_t)A.cl_cc[tid] * G + g];
    u64 kr[KPT];
    u64 kmn = ~0ull, kmx = 0;
    if (!GLOBALMEM) {
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const int i = u * T + tid;
            kr[u] = (i < n) ? key[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            if (u * T + tid < n) {
                kmn = kr[u] < kmn ? kr[u] : kmn;
                kmx = kr[u] > kmx ? kr[u] : kmx;
            }
        }
    } else {
        for (int i = tid; i < n; i += T) {
            const u64 k = key[i];
            kmn = k < kmn ? k : kmn;
            kmx = k > kmx ? k : kmx;
        }
    }
    for (int m2 = 32; m2 >= 1; m2 >>= 1) {
        const u64 o1 = shfl_xor_u64(kmn, m2), o2 = shfl_xor_u64(kmx, m2);
        kmn = o1 < kmn ? o1 : kmn;
        kmx = o2 > kmx ? o2 : kmx;
    }
    if (tid < SCC_MAX_K) {
        L.m[tid] = 0;
        L.F[tid] = 0;
    }
    for (int i = tid; i < K * K; i += T) pmap[i] = 0;
    if (lane == 0) {
        L.red64[w] = kmn;
        L.red64[W + w] = kmx;
    }
    if (tid == 0) {
        L.nruns = 0;
        L.flag = 0;
        L.redo = 0;
        L.anytie = 0;
    }
    int* off = (int*)L.po;  // cluster offsets of a gene segment, until the position offsets exist
    if (it.src == 0 && tid <= K) off[tid] = off_r;
    // tested pairs of this gene, compacted in pair order (all of them in SLOW / test-all)
    {
        u32 basep = 0;
        for (int p0 = 0; p0 < P; p0 += T) {
            const int p = p0 + tid;
            const bool t = p < P && (A.all_pairs || (A.flags[(size_t)p * G + g] & 1));
            const u64 bal = __ballot(t);
            if (lane == 0) L.redu[w] = (u32)__popcll(bal);
            __syncthreads();
            u32 o = basep;
            for (int v = 0; v < w; ++v) o += L.redu[v];
            if (t) tp[o + lanes_below(bal)] = (u32)p;
            for (int v = 0; v < W; ++v) basep += L.redu[v];
            __syncthreads();
        }
        if (tid == 0) L.ntp = (int)basep;
    }
    // key range -> 32-bit window of (key - kmin)
    kmn = L.red64[0];
    kmx = L.red64[W];
    for (int v = 1; v < W; ++v) {
        kmn = L.red64[v] < kmn ? L.red64[v] : kmn;
        kmx = L.red64[W + v] > kmx ? L.red64[W + v] : kmx;
    }
    const u64 kmin = kmn, kmax = kmx;
    const u64 range = kmax - kmin;
    const int bits = range ? 64 - __clzll((long long)range) : 0;
    const int sh = bits > 32 ? bits - 32 : 0;
    if (!GLOBALMEM) {
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const int i = u * T + tid;
            if (i < n) win[i] = (u32)((kr[u] - kmin) >> sh);
        }
    } else {
        for (int i = tid; i < n; i += T) win[i] = (u32)((key[i] - kmin) >> sh);
    }
    if (it.src == 0) {  // the ingest's cluster-grouped gene segment: codes from the offsets
        for (int a = 0; a < K; ++a) {
            const int s0 = off[a], s1 = off[a + 1];
            if (tid == 0) L.m[a] = (u32)(s1 - s0);
            for (int i = s0 + tid; i < s1; i += T) code[i] = (u8)a;
        }
    } else {
        for (int i0 = 0; i0 < n; i0 += T) {  // bucket: codes and cluster counts
            const int i = i0 + tid;
            const bool ok = i < n;
            const u32 c = ok ? A.codes2[it.base + i] : 0u;
            if (ok && !GLOBALMEM) code[i] = (u8)c;
            const u64 peers = match_bits<SCC_CODE_BITS>(c, __ballot(ok));
            if (ok && lanes_below(peers) == 0) atomicAdd(&L.m[c], (u32)__popcll(peers));
        }
    }
    __syncthreads();
    {
        // pack (pair, a, b, smaller side), one tested pair per thread, and chunk
        // the smaller side by 64 (chunk offsets: a workgroup exclusive scan)
        const int ntp0 = L.ntp;
        u32 basec = 0;
        for (int j0 = 0; j0 < ntp0; j0 += T) {
            const int j = j0 + tid;
            u32 nchk = 0;
            if (j < ntp0) {
                int a2, b2;
                pair_decode((int)tp[j], K, a2, b2);
                const u32 ma = L.m[a2], mb = L.m[b2];
                const bool sb = mb < ma;
                tp[j] = tp[j] | ((u32)a2 << 16) | ((u32)b2 << 23) | ((u32)sb << 30);
                pmap[a2 * K + b2] = (unsigned short)(j + 1);
                eacc[j] = 0;
                xacc[j] = 0;
                nchk = ((sb ? mb : ma) + 63) / 64;
            }
            u32 inc = nchk;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            if (lane == 63) L.redu[w] = inc;
            __syncthreads();
            u32 pre = basec;
            for (int v = 0; v < w; ++v) pre += L.redu[v];
            if (j < ntp0) cp[j] = pre + inc - nchk;
            for (int v = 0; v < W; ++v) basec += L.redu[v];
            __syncthreads();
        }
        if (tid == 0) {
        cp[ntp0] = basec;
        L.nchunk = (int)basec;
        u32 s2 = 0;
        for (int a3 = 0; a3 < K; ++a3) {
            L.po[a3] = s2;
            s2 += L.m[a3];
        }
        L.po[K] = s2;
        }
    }
    __syncthreads();
    const int ntp = L.ntp;
    if (it.bucket >= 0 && tid < K) A.hbg[(size_t)it.bucket * K + tid] = L.m[tid];
    ISTAMP(1);
    if (kmin == kmax) {
        // one distinct value: every pair is a tie, no order needed
        if (tid < K) {
            const u64 c = L.m[tid];
            if (c >= 2) atomicAdd((unsigned long long*)&A.accF[(size_t)tid * G + g], (unsigned long long)f_tie(c));
        }
        for (int j = tid; j < ntp; j += T) {
            const u32 v = tp[j];
            const u64 ca = L.m[tp_a(v)], cb = L.m[tp_b(v)];
            if (ca && cb) {
                atomicAdd((unsigned long long*)&A.accE[(size_t)tp_p(v) * G + g], (unsigned long long)(ca * cb));
                atomicAdd((unsigned long long*)&A.accX[(size_t)tp_p(v) * G + g],
                          (unsigned long long)(ca * cb * (ca + cb)));
            }
        }
        return;
    }
    // ---- stable sort by (value, cluster) on the 32-bit window
    for (int i = tid; i < n; i += T) ix0[i] = (IX)i;
    __syncthreads();
    IX* in = ix0;
    IX* out = ix1;
    if (it.src != 0) {  // bucket input is not cluster-grouped: stable pass on the cluster first
        radix_pass<W, SCC_CODE_BITS>([&](IX id) { return (u32)code[id]; }, in, out, n, L.rx);
        IX* t = in;
        in = out;
        out = t;
    }
    const int wbits = bits - sh;
    for (int p = 0; 8 * p < wbits; ++p) {
        const int s = 8 * p;
        radix_pass<W, 8>([&](IX id) { return (win[id] >> s) & 255u; }, in, out, n, L.rx);
        IX* t = in;
        in = out;
        out = t;
    }
    ISTAMP(2);
    if (sh > 0) {  // exact fix-up of windows that merged distinct doubles
        for (int i = tid; i + 1 < n; i += T) {
            const IX i0 = in[i], i1 = in[i + 1];
            if (win[i0] == win[i1] && key[i0] != key[i1]) L.flag = 1;
        }
        __syncthreads();
        if (L.flag) {
            for (int i = tid; i < n; i += T) {
                const u32 w0 = win[in[i]];
                const bool start = (i == 0 || win[in[i - 1]] != w0) && i + 1 < n && win[in[i + 1]] == w0;
                if (!start) continue;
                const u64 k0 = key[in[i]];
                int e = i + 1;
                bool mixed = false;
                while (e < n && win[in[e]] == w0) {
                    mixed |= key[in[e]] != k0;
                    ++e;
                }
                if (!mixed) continue;
                if (e - i <= 64) {
                    const int slot = atomicAdd(&L.nruns, 1);
                    if (slot < RK_RUNS) {
                        L.run_s[slot] = i;
                        L.run_l[slot] = e - i;
                    } else {
                        L.redo = 1;
                    }
                } else {
                    L.redo = 1;
                }
            }
            __syncthreads();
            if (L.redo) {  // pathological: exact LSD sort on every key bit (equal keys keep their order)
                for (int p = 0; 8 * p < bits; ++p) {
                    const int s = 8 * p;
                    radix_pass<W, 8>([&](IX id) { return (u32)((key[id] - kmin) >> s) & 255u; }, in, out, n, L.rx);
                    IX* t = in;
                    in = out;
                    out = t;
                }
            } else {
                // a mixed run holds one window: sort it exactly on (key, cluster, index)
                for (int r = w; r < L.nruns; r += W) wave_sort_run(key, code, in, L.run_s[r], L.run_l[r]);
                __syncthreads();
            }
        }
    }
    // sorted codes; bit 7: equal to the next element (a tie group continues)
    bool tie = false;
    for (int i = tid; i < n; i += T) {
        const IX id = in[i];
        bool eqn = false;
        if (i + 1 < n) {
            const IX id1 = in[i + 1];
            eqn = win[id1] == win[id] && (sh == 0 || key[id1] == key[id]);
        }
        tie |= eqn;
        sc[i] = (u8)(code[id] | (eqn ? 128 : 0));
    }
    if (__ballot(tie) && lane == 0) L.anytie = 1;
    __syncthreads();
    ISTAMP(3);
    // ---- positions partitioned by cluster (stable: ascending inside a cluster)
    IX* pl = out;  // the free index buffer
    {
        const int R = (((n + W - 1) / W) + 63) & ~63;
        const int lo = min(n, w * R), hi = min(n, lo + R);
        u32* hw = L.rx.hist + w * 256;
        for (int d = lane; d < SCC_MAX_K; d += 64) hw[d] = 0;
        __builtin_amdgcn_wave_barrier();
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int i = i0 + lane;
            const bool ok = i < hi;
            const u32 d = ok ? (sc[i] & SCC_CODE_MASK) : 0u;
            const u64 peers = match_bits<SCC_CODE_BITS>(d, __ballot(ok));
            if (ok && lanes_below(peers) == 0) hw[d] += (u32)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        if (tid < SCC_MAX_K) {  // per-(wave, cluster) start offsets
            u32 s = (tid < K) ? L.po[tid] : 0u;
            for (int v = 0; v < W; ++v) {
                const u32 c = L.rx.hist[v * 256 + tid];
                L.rx.hist[v * 256 + tid] = s;
                s += c;
            }
        }
        __syncthreads();
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int i = i0 + lane;
            const bool ok = i < hi;
            const u32 d = ok ? (sc[i] & SCC_CODE_MASK) : 0u;
            const u64 peers = match_bits<SCC_CODE_BITS>(d, __ballot(ok));
            if (ok) {
                const u32 rank = lanes_below(peers);
                const u32 b = hw[d];
                pl[b + rank] = (IX)i;
                if (rank == 0) hw[d] = b + (u32)__popcll(peers);
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }
    ISTAMP(4);
    // ---- within-item S_ab for every tested pair: the smaller cluster's
    // positions binary-searched in the larger one's (positions are distinct)
    {
        const int nch = L.nchunk;
        int cur = -1;
        u64 acc = 0;
        for (int c = w; c < nch; c += W) {
            int lo = 0, hi = ntp;  // last j with cp[j] <= c (wave-uniform)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int)cp[mid] <= c) lo = mid;
                else hi = mid;
            }
            const int j = lo;
            if (j != cur) {
                if (cur >= 0) {
                    const u64 s = u64_wave_sum(acc);
                    if (lane == 0 && s)
                        atomicAdd((unsigned long long*)&A.accS[(size_t)tp_p(tp[cur]) * G + g], (unsigned long long)s);
                }
                cur = j;
                acc = 0;
            }
            const u32 v = tp[j];
            const int a = tp_a(v), b = tp_b(v);
            const bool sb = tp_sb(v);
            const int s = sb ? b : a, lg = sb ? a : b;
            const u32 ms = L.m[s];
            const u32 e = (u32)(c - (int)cp[j]) * 64u + (u32)lane;
            const u32 mlg = L.m[lg];
            const IX* lst = pl + L.po[lg];
            u32 x = 0;
            if (e < ms) x = (u32)pl[L.po[s] + e];
            const u32 lb = lower_bound_ix(lst, mlg, x);
            if (e < ms) acc += sb ? (u64)(mlg - lb) : (u64)lb;
        }
        if (cur >= 0) {
            const u64 s = u64_wave_sum(acc);
            if (lane == 0 && s)
                atomicAdd((unsigned long long*)&A.accS[(size_t)tp_p(tp[cur]) * G + g], (unsigned long long)s);
        }
    }
    ISTAMP(5);
    // ---- tie groups: runs of equal (value, cluster) inside groups of equal value
    if (L.anytie) {
        IX* rs = in;  // sorted order no longer needed: run starts
        // run start flags -> exclusive scan (per-thread contiguous chunks)
        const int chunk = (n + T - 1) / T;
        const int c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
        u32 cnt = 0;
        for (int i = c0; i < c1; ++i) {
            const bool st = (i == 0) || !(sc[i - 1] & 128) || ((sc[i - 1] & SCC_CODE_MASK) != (sc[i] & SCC_CODE_MASK));
            cnt += st;
        }
        u32 incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) L.redu[w] = incl;
        __syncthreads();
        u32 basev = incl - cnt;
        for (int v = 0; v < w; ++v) basev += L.redu[v];
        if (tid == T - 1) L.redu[W] = basev + cnt;  // number of runs
        __syncthreads();
        const u32 nr = L.redu[W];
        // rs aliases the sorted-order buffer that is no longer read; the
        // starts are written after every thread finished reading it above
        for (int i = c0; i < c1; ++i) {
            const bool st = (i == 0) || !(sc[i - 1] & 128) || ((sc[i - 1] & SCC_CODE_MASK) != (sc[i] & SCC_CODE_MASK));
            if (st) rs[basev++] = (IX)i;
        }
        if (tid == 0) rs[nr] = (IX)n;
        __syncthreads();
        for (u32 r = tid; r < nr; r += T) {
            const u32 s0 = rs[r], len = (u32)rs[r + 1] - s0;
            const int a = sc[s0] & SCC_CODE_MASK;
            if (len >= 2) atomicAdd((unsigned long long*)&L.F[a], (unsigned long long)f_tie(len));
            // earlier runs of the same value: their clusters are smaller (codes
            // increase inside a group), each gives a cross-cluster tie block
            u32 q = r;
            while (q > 0 && (sc[(u32)rs[q] - 1] & 128)) {
                --q;
                const u32 ps = rs[q];
                const u64 lb = (u32)rs[q + 1] - ps, la = len;
                const int b = sc[ps] & SCC_CODE_MASK;  // b < a
                const int slot = pmap[b * K + a];
                if (slot) {
                    atomicAdd((unsigned long long*)&eacc[slot - 1], (unsigned long long)(la * lb));
                    atomicAdd((unsigned long long*)&xacc[slot - 1], (unsigned long long)(la * lb * (la + lb)));
                }
            }
        }
        __syncthreads();
        if (tid < K && L.F[tid])
            atomicAdd((unsigned long long*)&A.accF[(size_t)tid * G + g], (unsigned long long)L.F[tid]);
        for (int j = tid; j < ntp; j += T) {
            const int pp = tp_p(tp[j]);
            if (eacc[j]) atomicAdd((unsigned long long*)&A.accE[(size_t)pp * G + g], (unsigned long long)eacc[j]);
            if (xacc[j]) atomicAdd((unsigned long long*)&A.accX[(size_t)pp * G + g], (unsigned long long)xacc[j]);
        }
    }
    ISTAMP(6);
#undef ISTAMP
}

template <int T, bool GLOBALMEM, int KPT>
__global__ void __launch_bounds__(T, 4) k_rank_item(ScRankLaunch A, int cls)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cnt = rk_cnt(A, RK_CNT_ITEMS0 + cls);
    for (int i = blockIdx.x; i < cnt; i += gridDim.x) {
        const ScRankItem it = A.items[(size_t)cls * A.item_cap + i];
        rank_one_item<T, GLOBALMEM, KPT>(A, it, i + A.stamp_base[cls], smem);
        __syncthreads();
    }
}

// ===================================================================== host
// bytes of an item's tested-pair tables (tp, cp, eacc, xacc, pmap)
static size_t item_tables_bytes(int ntp_max, int K)
{
    const size_t s = sizeof(u32) * (2 * (size_t)ntp_max + 1) + 8 + 16 * (size_t)ntp_max + 2 * (size_t)K * K;
    return (s + 31) & ~(size_t)15;
}

// tables past 24 KB (many tested pairs per gene, K > ~40) live in HBM scratch
extern "C" int scc_rank_tables_global(int ntp_max, int K) { return item_tables_bytes(ntp_max, K) > 24 * 1024; }
extern "C" size_t scc_rank_tables_stride(int ntp_max, int K) { return (item_tables_bytes(ntp_max, K) + 255) & ~(size_t)255; }

template <int W>
static size_t item_lds_fixed(int ntp_max, int K)
{
    const size_t s = sizeof(ItemLds<W>) + (scc_rank_tables_global(ntp_max, K) ? 16 : item_tables_bytes(ntp_max, K));
    return (s + 31) & ~(size_t)15;
}

#define RK_T0 256   // small items
#define RK_T1 512   // medium items (two workgroups per CU)
#define RK_T2 1024  // HBM-resident items

extern "C" size_t scc_rank_item_lds(int cls, int cap, int ntp_max, int K)
{
    if (cls == 0) return item_lds_fixed<RK_T0 / 64>(ntp_max, K) + (size_t)cap * (4 + 2 + 2 + 1 + 1);
    if (cls == 1) return item_lds_fixed<RK_T1 / 64>(ntp_max, K) + (size_t)cap * (4 + 2 + 2 + 1 + 1);
    return item_lds_fixed<RK_T2 / 64>(ntp_max, K);
}

// largest LDS-resident item capacity (multiple of 64) of class cls within lim bytes
#define RK_KPT0 8   // cap_s <= 8 * 256
#define RK_KPT1 8  // cap_m <= 8 * 512

extern "C" int scc_rank_item_cap(int cls, int want, int ntp_max, int K, int lim)
{
    int cap = want & ~63;
    if (cls == 0 && cap > RK_KPT0 * RK_T0) cap = RK_KPT0 * RK_T0;
    if (cls == 1 && cap > RK_KPT1 * RK_T1) cap = RK_KPT1 * RK_T1;
    while (cap > 64 && scc_rank_item_lds(cls, cap, ntp_max, K) > (size_t)lim) cap -= 64;
    if (cap > 65535) cap = 65535 & ~63;
    return cap;
}

extern "C" hipError_t scc_launch_rank_items(const ScRankLaunch* L, int cls, int grid, hipStream_t st)
{
    if (grid <= 0) return hipSuccess;
    ScRankLaunch A = *L;
    if (cls == 0) {
        A.cap_lds = L->cap_s;
        const size_t lds = scc_rank_item_lds(0, L->cap_s, L->ntp_max, L->K);
        scc_set_lds((const void*)k_rank_item<RK_T0, false, RK_KPT0>, (int)lds);
        hipLaunchKernelGGL((k_rank_item<RK_T0, false, RK_KPT0>), dim3(grid), dim3(RK_T0), lds, st, A, 0);
    } else if (cls == 1) {
        A.cap_lds = L->cap_m;
        const size_t lds = scc_rank_item_lds(1, L->cap_m, L->ntp_max, L->K);
        scc_set_lds((const void*)k_rank_item<RK_T1, false, RK_KPT1>, (int)lds);
        hipLaunchKernelGGL((k_rank_item<RK_T1, false, RK_KPT1>), dim3(grid), dim3(RK_T1), lds, st, A, 1);
    } else {
        A.cap_lds = 0;
        const size_t lds = scc_rank_item_lds(2, 0, L->ntp_max, L->K);
        scc_set_lds((const void*)k_rank_item<RK_T2, true, 1>, (int)lds);
        hipLaunchKernelGGL((k_rank_item<RK_T2, true, 1>), dim3(grid), dim3(RK_T2), lds, st, A, 2);
    }
    return hipGetLastError();
}
