// scc_rank_waves.hip — rank stage: one wave per bucket of <= 64 values.
//
// Both kernel families walk the wave-bucket list (sbuckets, RK_CNT_WAVE_SLOTS
// entries: the split's, the re-split's, or on the value-order route
// k_rank_vorder_list's), sort a bucket across the lanes, count every tested
// pair inside it, write its cluster histogram row (hbg) and keep a gene's sums
// in registers until the gene changes.
//   k_rank_waves   the slot kernels: lane j of slot s holds tested pair
//                  64 s + j.  Four slot classes by the gene's tested pairs
//                  (<= 128 on 2 slots, <= 256 on 4, <= 512 on 8, <= 1024 on
//                  RW_SLOTS_MAX = 16), each a launch of its own that skips the
//                  other classes' genes; past 1024 pairs (up to RW_PAIRS_MAX)
//                  one 16-slot pass per window of 1024.
//   k_rank_mfma16  the matrix-core kernel (K <= 16 NC, NC = 1..4): every pair of
//                  the K x K matrix from int8 MFMAs at a fixed cost per bucket.
//                  By default it takes the genes past 512 tested pairs, and at
//                  K <= 16 every gene (SCC_RANK_MFMA, SCC_RANK_MFMA16).
// VORD instances of both read the dataset's value order (scc_vorder.hip)
// through the call's cell codes instead of scattered keys.  RUNS (with VORD,
// K <= 16, SCC_RANK_RUNS) makes the matrix-core kernel add the cross term
// inside each run of a gene's buckets and leave one hbg row per run for
// k_rank_cross_runs (scc_rank_cross.hip).
// rank_waves_launches_t places the launches of both families on the main and
// side streams, which is why they share this unit.
#include "scc_rank_dev.hpp"

#include <algorithm>
#include <cstdio>

// ===================================================================== waves
// One wave per bucket of <= 64 elements: bitonic sort of (key, cluster) across
// the lanes (DPP / permlane swaps, no LDS), one ballot mask per cluster over
// the sorted lanes, then every lane computes its own tested pair's S (and the
// tie terms E, X) from the two masks (pair_counts).  Buckets of one repeated
// key (fat bins of ties) need only their cluster histogram.  Consecutive
// buckets of one gene accumulate in registers (lane j: tested pair j) and are
// flushed with one integer atomic per pair when the gene changes.

// The same merge on one combined key (key - gene minimum) << 7 | cluster.
// The lanes that keep the minimum at stride ST of a merge whose direction
// bit is UPBIT (0: ascending everywhere) form a compile-time lane mask KM, so
// a compare-exchange is two lane moves, one 64-bit compare into a lane mask,
// one scalar XNOR with KM and two selects (the min / max / direction selects
// the compiler made of `keep_min ? min : max` took 14 instructions a step,
// the per-lane direction masks spilled to SGPR lanes).  take = lt XNOR KM:
// a keep-min lane takes the partner's key when it is smaller, a keep-max lane
// when it is not smaller (equal keys: either is the same key).
__host__ __device__ constexpr u64 bitonic_km(int ST, int UPBIT)
{
    u64 m = 0;
    for (int l = 0; l < 64; ++l)
        if (((l & ST) == 0) == (UPBIT == 0 || (l & UPBIT) == 0)) m |= 1ull << l;
    return m;
}

// per-lane select by a lane mask held in scalar registers (bit set: b)
__device__ inline u32 lane_select(u64 mask, u32 a, u32 b)
{
    u32 r;
    asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}

template <int ST, int UPBIT>
__device__ inline void bitonic_merge_ck(u64& ck)
{
    const u32 olo = scc_xor_lane<ST>((u32)ck), ohi = scc_xor_lane<ST>((u32)(ck >> 32));
    const u64 o = ((u64)ohi << 32) | olo;
    constexpr u64 KM = bitonic_km(ST, UPBIT);
    const u64 lt = __ballot(o < ck);
    const u64 take = ~(lt ^ KM);
    ck = ((u64)lane_select(take, (u32)(ck >> 32), ohi) << 32) | lane_select(take, (u32)ck, olo);
    if constexpr (ST > 1) bitonic_merge_ck<ST / 2, UPBIT>(ck);
}

// The same merge on 32-bit keys (the value-order route's (group, code) keys fit
// 15 bits, unkept lanes ~0): a lane keeps the smaller (KM bit set) or the larger
// of its own key and its partner's, which is what the compare, ballot and two
// selects of the 64-bit form decide; about half its VALU instructions.
template <int ST, int UPBIT>
__device__ inline void bitonic_merge_ck32(u32& ck)
{
    const u32 o = scc_xor_lane<ST>(ck);
    constexpr u64 KM = bitonic_km(ST, UPBIT);
    ck = lane_select(KM, max(ck, o), min(ck, o));
    if constexpr (ST > 1) bitonic_merge_ck32<ST / 2, UPBIT>(ck);
}

__device__ inline u64 shfl_u64(u64 v, int src)
{
    const u32 lo = (u32)__shfl((int)(u32)v, src, 64), hi = (u32)__shfl((int)(u32)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// One pair's counts over a sorted bucket from its cluster masks, walking the
// set bits of the smaller one: S_ab = sum_{i in a} #b below i = sum_{j in b}
// #a above j; with ties (gst: lanes starting a group of equal keys, n: valid
// lanes) E_ab = sum over groups c_a c_b and X_ab = sum c_a c_b (c_a + c_b).
__device__ inline void pair_counts(u64 ma, u64 mb, bool ties, u64 gst, int n, u32& S, u32& E, u32& X)
{
    const bool walk_a = __popcll(ma) <= __popcll(mb);
    u64 m = walk_a ? ma : mb;
    const u64 self = m, other = walk_a ? mb : ma;
    S = E = X = 0;
    while (m) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        const u64 le = (2ull << i) - 1;  // lanes <= i (all of them for i = 63)
        S += (u32)__popcll(other & (walk_a ? (le >> 1) : ~le));
        if (ties) {
            const int gsl = 63 - __clzll((long long)(gst & le));
            const u64 aft = gst & ~le;
            const int ge = aft ? __builtin_ctzll(aft) : n;
            const u64 grp = ((ge >= 64) ? ~0ull : ((1ull << ge) - 1)) & ~((1ull << gsl) - 1);
            const u32 co = (u32)__popcll(other & grp), cs = (u32)__popcll(self & grp);
            E += co;
            X += co * (co + cs);
        }
    }
}

// One bitonic merge level of (key, code) across the lanes, strides ST .. 1.
template <int ST>
__device__ inline void bitonic_merge(u64& key, u32& code, bool up, int lane)
{
    const u64 ok = ((u64)scc_xor_lane<ST>((u32)(key >> 32)) << 32) | (u64)scc_xor_lane<ST>((u32)key);
    const u32 oc = scc_xor_lane<ST>(code);
    const bool lower = (lane & ST) == 0;
    const bool other_less = (ok < key) || (ok == key && oc < code);
    if ((lower == up) ? other_less : !other_less) {
        key = ok;
        code = oc;
    }
    if constexpr (ST > 1) bitonic_merge<ST / 2>(key, code, up, lane);
}

// VORD: the buckets are the dataset's precomputed cuts of each gene's value
// order, read through the call's cell codes (see k_rank_mfma16: unkept lanes
// carry code 255 and are in no cluster mask; a bucket without a tie bit is
// not sorted, one with a tie bit sorts (tie group, code) with the unkept last).
template <int RW_SLOTS, bool VORD = false>
__global__ void __launch_bounds__(256) k_rank_waves(ScRankLaunch A)
{
    __shared__ u64 cms[4][SCC_MAX_K];  // per-wave cluster masks (K > 16)
    const int lane = threadIdx.x & 63, wv = scc_wave_id();
    const int W = blockIdx.x * 4 + wv, NW = gridDim.x * 4;
    const int cnt = min(rk_cnt(A, RK_CNT_WAVE_SLOTS), A.bucket_cap);
    const int K = A.K, G = A.G, P = A.P;
    constexpr int CH = 16;  // consecutive buckets per wave visit (gene locality; 8 / 32 / 64 measured no better)
    int cur = -1, ntp = 0;
    u64 xbud = 0;  // a bound on the largest slot sum of the current run
    u64 gk = ~0ull;
    // per slot: the tested pair as the split packed it (p | a << 16 | b << 24)
    // and its sums over the buckets of the current run of one gene, in 32 bits
    // (a wave bucket adds S <= 32 * 32, E <= 32 * 32, X <= 32 * 32 * 64 to one
    // pair, a ties-only bucket of n values E <= n^2 / 4, X <= n^3 / 4: a run is
    // cut before the bound passes 2^32; a ties-only bucket past 2048 values
    // goes straight out in 64 bits):
    // half the registers of u64 sums and three pair words, so the 16-slot
    // variant fits two waves per SIMD
    u32 tp[RW_SLOTS];
    u32 aS[RW_SLOTS], aE[RW_SLOTS], aX[RW_SLOTS];
#pragma unroll
    for (int q = 0; q < RW_SLOTS; ++q) {
        tp[q] = 0;
        aS[q] = aE[q] = aX[q] = 0;
    }
    for (int c0 = W * CH; c0 < cnt; c0 += NW * CH) {
        const int c1 = min(cnt, c0 + CH);
        // the chunk's descriptors, one per lane, and the first bucket's elements:
        // every bucket's loads are issued one bucket ahead
        ScRankItem D{0, 0, 0, 0, 0};
        if (lane < c1 - c0) D = A.sbuckets[c0 + lane];
        // this launch ranks the buckets of genes with wv_lo < tested pairs <= wv_hi
        // (the slot count of each launch fits its genes: fewer registers, more waves)
        // (one class launched: no filter, and no dependent load before the first bucket)
        u64 rem;
        if (A.wv_filter) {
            const int ntg = (lane < c1 - c0 && D.n > 0) ? A.gene_nt[D.gene] : -1;  // n = 0: an unused re-split slot
            rem = __ballot(ntg > A.wv_lo && ntg <= A.wv_hi);
        } else {
            rem = __ballot(lane < c1 - c0 && D.n > 0);
        }
        if (!rem) continue;
        const u32 dlo = (u32)(u64)D.base, dhi = (u32)((u64)D.base >> 32);
        auto dbase = [&](int li) {
            return (i64)(((u64)(u32)__builtin_amdgcn_readlane((int)dhi, li) << 32) |
                         (u32)__builtin_amdgcn_readlane((int)dlo, li));
        };
        // a bucket's first 64 elements (VORD: key = the vcell word, its tie bit in bit 31)
        auto load = [&](i64 b, int nl, u64& k, u32& cd) {
            if constexpr (VORD) {
                const u32 w = lane < nl ? A.vcell[b + lane] : 0u;
                const int c8 = lane < nl ? (int)A.code8[w & 0x7fffffffu] : -1;
                k = (u64)w;
                cd = c8 < 0 ? 255u : (u32)c8;
            } else {
                k = lane < nl ? A.keys2[b + lane] : ~0ull;
                cd = lane < nl ? (u32)A.codes2[b + lane] : 255u;
            }
        };
        u64 nkey;
        u32 ncode;
        {
            const int l0 = __builtin_ctzll(rem);
            load(dbase(l0), __builtin_amdgcn_readlane(D.n, l0), nkey, ncode);
        }
        while (rem) {
            const int li = __builtin_ctzll(rem);
            rem &= rem - 1;
            const int g = __builtin_amdgcn_readlane(D.gene, li);
            int n = __builtin_amdgcn_readlane(D.n, li);
            const int bucket = __builtin_amdgcn_readlane(D.bucket, li);
            const int src = __builtin_amdgcn_readlane(D.src, li);
            const i64 bbase = dbase(li);
            u64 key = nkey;
            u32 code = ncode;
            if (rem) {
                const int l1 = __builtin_ctzll(rem);
                load(dbase(l1), __builtin_amdgcn_readlane(D.n, l1), nkey, ncode);
            }
            const bool big_ties = src == 2 && n > 2048;
            const u64 xadd = src == 2 ? (big_ties ? 0ull : (u64)n * n * n / 4 + 1) : 65536ull;
            if (g != cur || xbud + xadd > 0xffffffffull) {
                // flush the previous run's sums: one integer atomic per pair
                if (cur >= 0) {
#pragma unroll
                    for (int q = 0; q < RW_SLOTS; ++q) {
                        if (q * 64 + lane < ntp) {
                            const size_t o = (size_t)(tp[q] & 0xffffu) * G + cur;
                            if (aS[q]) atomicAdd((unsigned long long*)&A.accS[o], (unsigned long long)aS[q]);
                            if (aE[q]) atomicAdd((unsigned long long*)&A.accE[o], (unsigned long long)aE[q]);
                            if (aX[q]) atomicAdd((unsigned long long*)&A.accX[o], (unsigned long long)aX[q]);
                        }
                        aS[q] = aE[q] = aX[q] = 0;
                    }
                }
                xbud = 0;
            }
            xbud += xadd;
            if (g != cur) {
                cur = g;
                if constexpr (!VORD) gk = A.gkmin[g];
                // tested pairs of g in pair order (compacted by the split)
                // this launch's window of the gene's tested pairs (wv_base > 0: the
                // second pass over a gene with more than 64 * RW_SLOTS of them)
                ntp = max(0, min(A.gene_nt[g] - A.wv_base, 64 * RW_SLOTS));
                const u32* tl = A.gene_tp + (size_t)g * P + A.wv_base;
#pragma unroll
                for (int q = 0; q < RW_SLOTS; ++q) {
                    const int j = q * 64 + lane;
                    const u32 v = tl[j < ntp ? j : 0];
                    if (j < ntp) tp[q] = v;
                }
            }
            if (src == 2) {
                // one repeated key: only the cluster histogram matters.  Inside
                // the bucket S_ab = 0 (a < b: ties ordered by cluster),
                // E_ab = c_a c_b, X_ab = c_a c_b (c_a + c_b), F_a = f(c_a).
                u32 myc = 0, myc1 = 0;  // lane c: cluster c's count, and cluster c + 64's
                for (int i0 = 0; i0 < n; i0 += 256) {
                    u32 cd[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = i0 + u * 64 + lane;
                        if constexpr (VORD) {
                            const int c8 = i < n ? (int)A.code8[A.vcell[bbase + i] & 0x7fffffffu] : -1;
                            cd[u] = c8 < 0 ? 255u : (u32)c8;
                        } else {
                            cd[u] = i < n ? (u32)A.codes2[bbase + i] : 255u;
                        }
                    }
                    for (int c = 0; c < K; ++c) {
                        u32 t = 0;
#pragma unroll
                        for (int u = 0; u < 4; ++u) t += (u32)__popcll(__ballot(cd[u] == (u32)c));
                        if (lane == c) myc += t;
                        if (lane + 64 == c) myc1 += t;
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int c = lane + 64 * h;
                    const u32 mc = h ? myc1 : myc;
                    if (c < K) {
                        A.hbg[(size_t)bucket * K + c] = mc;
                        if (mc >= 2 && A.wv_base == 0)  // per cluster: once, not per pair window
                            atomicAdd((unsigned long long*)&A.accF[(size_t)c * G + g], (unsigned long long)f_tie(mc));
                    }
                }
                // (past 2048 values its counts can pass 32 bits: straight out in 64)
#pragma unroll
                for (int q = 0; q < RW_SLOTS; ++q) {
                    const u32 pa = (tp[q] >> 16) & 0xffu, pb = tp[q] >> 24;
                    u64 ca = (u32)__shfl((int)myc, (int)(pa & 63u), 64);
                    u64 cb = (u32)__shfl((int)myc, (int)(pb & 63u), 64);
                    if (K > 64) {
                        const u64 ca1 = (u32)__shfl((int)myc1, (int)(pa & 63u), 64);
                        const u64 cb1 = (u32)__shfl((int)myc1, (int)(pb & 63u), 64);
                        ca = pa >= 64 ? ca1 : ca;
                        cb = pb >= 64 ? cb1 : cb;
                    }
                    if (q * 64 + lane < ntp && ca && cb) {
                        if (big_ties) {
                            const size_t o = (size_t)(tp[q] & 0xffffu) * G + g;
                            atomicAdd((unsigned long long*)&A.accE[o], (unsigned long long)(ca * cb));
                            atomicAdd((unsigned long long*)&A.accX[o], (unsigned long long)(ca * cb * (ca + cb)));
                        } else {
                            aE[q] += (u32)(ca * cb);
                            aX[q] += (u32)(ca * cb * (ca + cb));
                        }
                    }
                }
                continue;
            }
            // ---- load and bitonic sort by (key, code) across the lanes (invalid lanes last)
            bool vl = lane < n;
            if constexpr (VORD) {
                const u64 tb = __ballot(vl && ((key >> 31) & 1ull));
                if (tb) {
                    // (lane 0 of a bucket starts a group: its bit is clear, so a group number is >= 1)
                    const u64 vm = (n >= 64) ? ~0ull : ((1ull << n) - 1);
                    const u64 le = (lane == 63) ? ~0ull : ((2ull << lane) - 1);
                    const u64 grp = (u64)__popcll(~tb & vm & le);
                    const bool kept = vl && code != 255u;
                    const int nk = __popcll(__ballot(kept));
                    u32 ck = kept ? (((u32)grp << SCC_CODE_BITS) | code) : ~0u;  // (grp <= 64: a 32-bit key)
                    if (n > 1) bitonic_merge_ck32<1, 2>(ck);
                    if (n > 2) bitonic_merge_ck32<2, 4>(ck);
                    if (n > 4) bitonic_merge_ck32<4, 8>(ck);
                    if (n > 8) bitonic_merge_ck32<8, 16>(ck);
                    if (n > 16) bitonic_merge_ck32<16, 32>(ck);
                    if (n > 32) bitonic_merge_ck32<32, 0>(ck);
                    n = nk;  // the kept elements, in (group, code) order in the first lanes
                    vl = lane < n;
                    key = (u64)(ck >> SCC_CODE_BITS);
                    code = vl ? (ck & (u32)SCC_CODE_MASK) : 255u;
                } else {
                    key = (u64)lane;  // every value its own group
                }
            } else if (A.dbg == 2) {
            } else if (gk != ~0ull) {  // one 64-bit sort key: (key - gene minimum) << 7 | cluster
                u64 ck = vl ? (((key - gk) << SCC_CODE_BITS) | code) : ~0ull;
                // levels up to the next power of two >= n (lanes past it hold only ~0)
                if (n > 1) bitonic_merge_ck<1, 2>(ck);
                if (n > 2) bitonic_merge_ck<2, 4>(ck);
                if (n > 4) bitonic_merge_ck<4, 8>(ck);
                if (n > 8) bitonic_merge_ck<8, 16>(ck);
                if (n > 16) bitonic_merge_ck<16, 32>(ck);
                if (n > 32) bitonic_merge_ck<32, 0>(ck);
                key = ck >> SCC_CODE_BITS;  // order-equivalent for the tie tests below
                code = vl ? (u32)(ck & SCC_CODE_MASK) : 255u;
            } else {
                if (n > 1) bitonic_merge<1>(key, code, (lane & 2) == 0, lane);
                if (n > 2) bitonic_merge<2>(key, code, (lane & 4) == 0, lane);
                if (n > 4) bitonic_merge<4>(key, code, (lane & 8) == 0, lane);
                if (n > 8) bitonic_merge<8>(key, code, (lane & 16) == 0, lane);
                if (n > 16) bitonic_merge<16>(key, code, (lane & 32) == 0, lane);
                if (n > 32) bitonic_merge<32>(key, code, true, lane);
            }
            // ---- cluster masks over the sorted lanes (lane c holds cluster c's, cm1
            // cluster c + 64's) and the hbg row
            u64 cm = 0, cm1 = 0;
            if (K <= 16) {  // one ballot per cluster
                for (int c = 0; c < K; ++c) {
                    const u64 m = __ballot(code == (u32)c);
                    if (lane == c) cm = m;
                }
            } else {  // many clusters: 7 ballots match equal codes, each cluster's leader posts its mask
                const bool in_clu = vl && code != 255u;  // (VORD: an unkept lane inside the bucket)
                const u64 peers = match_bits<SCC_CODE_BITS>(code & SCC_CODE_MASK, __ballot(in_clu));
                cms[wv][lane] = 0;
                if (K > 64) cms[wv][lane + 64] = 0;
                wsync();
                if (in_clu && lanes_below(peers) == 0) cms[wv][code] = peers;
                wsync();
                cm = cms[wv][lane];
                if (K > 64) cm1 = cms[wv][lane + 64];
            }
            if (lane < K) A.hbg[(size_t)bucket * K + lane] = (u32)__popcll(cm);
            if (lane + 64 < K) A.hbg[(size_t)bucket * K + lane + 64] = (u32)__popcll(cm1);
            // ---- tie groups (equal keys) and runs (equal key and cluster)
            const u64 kp = ((u64)(u32)__shfl_up((int)(u32)(key >> 32), 1, 64) << 32) |
                           (u64)(u32)__shfl_up((int)(u32)key, 1, 64);
            const u32 cpv = (u32)__shfl_up((int)code, 1, 64);
            const u64 vmask = (n >= 64) ? ~0ull : ((1ull << n) - 1);
            const bool gs_me = (lane == 0) || (kp != key);
            const u64 gst = __ballot(gs_me && vl);
            const bool anytie = ((~gst) & vmask & ~1ull) != 0;
            if (anytie) {
                // within-cluster runs: F_a += len^3 - len per run of >= 2
                const u64 le = (lane == 63) ? ~0ull : ((2ull << lane) - 1);  // lanes <= me
                const bool rs_me = (lane == 0) || (kp != key) || (cpv != code);
                const u64 rst = __ballot(rs_me && vl);
                if (rs_me && vl) {
                    const u64 raft = rst & ~le;
                    const int re = raft ? __builtin_ctzll(raft) : n;
                    const u64 len = (u64)(re - lane);
                    if (len >= 2 && A.wv_base == 0)
                        atomicAdd((unsigned long long*)&A.accF[(size_t)code * G + g], (unsigned long long)f_tie(len));
                }
            }
            // ---- tested pairs: lane l of slot q owns pair q * 64 + l
#pragma unroll
            for (int q = 0; q < RW_SLOTS; ++q) {
                if (q * 64 >= ntp || A.dbg == 1) break;
                u64 ma, mb;
                const u32 pa = (tp[q] >> 16) & 0xffu, pb = tp[q] >> 24;
                if (K > 16) {  // the pair's masks straight from the leaders' LDS posts (two reads, no lane moves;
                               // clusters 64..127 too: 8 lane moves a slot before at K > 64)
                    ma = cms[wv][pa];
                    mb = cms[wv][pb];
                } else {
                    ma = shfl_u64(cm, (int)(pa & 63u));
                    mb = shfl_u64(cm, (int)(pb & 63u));
                }
                if (q * 64 + lane < ntp && ma && mb) {
                    u32 S, E, X;
                    pair_counts(ma, mb, anytie, gst, n, S, E, X);
                    aS[q] += S;
                    aE[q] += E;
                    aX[q] += X;
                }
            }
            if (K > 16) wsync();  // the masks are reposted by the next bucket
        }
    }
    if (cur >= 0) {
#pragma unroll
        for (int q = 0; q < RW_SLOTS; ++q) {
            if (q * 64 + lane < ntp) {
                const size_t o = (size_t)(tp[q] & 0xffffu) * G + cur;
                if (aS[q]) atomicAdd((unsigned long long*)&A.accS[o], (unsigned long long)aS[q]);
                if (aE[q]) atomicAdd((unsigned long long*)&A.accE[o], (unsigned long long)aE[q]);
                if (aX[q]) atomicAdd((unsigned long long*)&A.accX[o], (unsigned long long)aX[q]);
            }
        }
    }
}

// ===================================================================== waves on MFMA
// The bucket walk of k_rank_waves with the pair counting on the int8 matrix
// cores (K <= 64).  After the bitonic sort, with O the bucket's one-hot
// (element x cluster) matrix and L the strict lower triangle of positions,
//   M = L O        M[i][b]: b-elements sorted below element i
//   S += O^T M     S[a][b] = sum over i in a of #b below i (for a < b the
//                  positional count is the strict one: equal keys sort by cluster)
// and, in a bucket with ties, with Eq[i][j] = [j in i's tie group],
// Q = Eq O (Q[i][b] = t_b of i's group) and D_i = t_{c_i} of i's group:
//   E += O^T Q                     sum over groups t_a t_b
//   X += (D O)^T Q + Q^T (D O)     sum over groups t_a^2 t_b + t_a t_b^2
// Every operand is 0/1 or a count <= 64 (int8) and one bucket's products fit
// int32.  A gene's sums stay in the accumulator tiles (the upper 16 x 16 tiles
// of the K x K matrices hold every pair a < b) and leave with one integer
// atomic per tested pair when the gene changes: at K <= 64 (NC = 4 cluster
// tiles) 26 MFMAs 16x16x64 per bucket without ties, 72 with, whatever the
// number of tested pairs (the per-pair walk of k_rank_waves ran 16 slots of 64
// pairs per bucket at config D).  Same bucket list, same hbg rows and F terms,
// same integers.
typedef int rk_v4i __attribute__((ext_vector_type(4)));
// bytes [base + q < x], q = 0..3 (0 / 1 each)
__device__ inline u32 rk_lt_bytes(int x, int base)
{
    int v = x - base;
    v = v < 0 ? 0 : (v > 4 ? 4 : v);
    return (u32)((0x01010101ull << (8 * v)) >> 32);
}

// bytes of w equal to c (0 / 1 each)
__device__ inline u32 rk_eq_bytes(u32 w, u32 c)
{
    const u32 x = w ^ (c * 0x01010101u);
    const u32 nz = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;  // bit 7 of a byte: the byte is not zero
    return (~nz >> 7) & 0x01010101u;
}

__device__ unsigned long long g_rk_stamps[8];  // SCC_RK_STAMPS diagnostics: summed phase cycles
extern "C" void scc_rank_mfma_stamps(hipStream_t st, int print)
{
    unsigned long long h[8];
    if (print) {
        hipStreamSynchronize(st);
        hipMemcpyFromSymbol(h, HIP_SYMBOL(g_rk_stamps), sizeof(h), 0, hipMemcpyDeviceToHost);
        fprintf(stderr, "[scc rk stamps] buckets %llu flush %llu: per bucket sort %.0f operands %.0f products %.0f ties %.0f "
                "flush %.0f fat %.0f\n", h[6], h[7], h[0] / (double)(h[6] + 1), h[1] / (double)(h[6] + 1),
                h[2] / (double)(h[6] + 1), h[3] / (double)(h[6] + 1), h[4] / (double)(h[6] + 1), h[5] / (double)(h[6] + 1));
    }
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rk_stamps), z, sizeof(z), 0, hipMemcpyHostToDevice, st);
    hipStreamSynchronize(st);
}

struct RkWaveLds {
    u8 code[64];  // sorted codes at their operand slots
    u8 dcnt[64];  // D_i at their operand slots
    u32 cnt[64];  // a fat bin's cluster counts
    u64 F[64];    // within-cluster tie terms of the current gene, per cluster
    u32 pre[64];  // RUNS: the run's prefix counts per cluster, for the 64-bit cross sums
};

// The products on 16 x 16 x 64 tiles (K <= 16 * NC): one MFMA covers a
// bucket's 64 elements, a cluster tile is 4 accumulator registers, so the
// kernel keeps two waves per SIMD even at K = 64 (a 32 x 32 x 32 form of the
// same products held 1 wave at 422 registers: D SLOW rank 60.8 ms against
// 42.3 ms for this one, round 6).  Slots: lane l holds
// row / column l & 15 and, in byte t of its 16-byte fragment (lane group
// g = l >> 4), element e(g, t) = 16 (t >> 2) + 4 g + (t & 3): the row the
// accumulator layout puts in register t & 3 of lane group g of row tile
// t >> 2, so four packed accumulator tiles are the next product's operand.
// Lane shuffles of the bucket loop with their addresses formed once (a
// __shfl* forms its source lane and clamps it at every call: four VALU
// instructions a shuffle in a kernel bound by VALU issue).
// the value of the lane below (lane 0: 0), one DPP move
__device__ inline u32 rk_lane_up1(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }
// the value of lane addr4 / 4
__device__ inline u32 rk_lane_at(int addr4, u32 v) { return (u32)__builtin_amdgcn_ds_bpermute(addr4, (int)v); }

__device__ inline rk_v4i rk_mfma16(rk_v4i a, rk_v4i b, rk_v4i c)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

template <int NC>
__device__ constexpr int rk_tile16(int ma, int nb)  // upper tiles (ma <= nb) in row order
{
    return ma * NC - ma * (ma - 1) / 2 + (nb - ma);
}

// VORD: the buckets are the dataset's precomputed cuts of each gene's value
// order (scc_vorder.hip): an element is a cell of A.vcell, its code the call's
// code of that cell (unkept: 255, an all-zero one-hot row that adds nothing to
// L O, O^T (2 M) or the histogram row, so unkept lanes stay where they are).
// A bucket without a tie bit is in order as loaded: nothing is sorted.  With
// one, the lanes' tie-group numbers stand for the keys: (group, code) is
// sorted as the combined key is, unkept lanes last, because the tie terms
// assume the codes in order inside a group.
// RUNS (with VORD, this launch the call's only bucket kernel): a wave walks
// consecutive buckets of a gene in value order, so inside its run (the gene's
// buckets within the chunk) it adds the cross-bucket term itself: pre[b], the
// b-elements of the run's earlier buckets, is kept per lane for column
// r16 (+ 16 t), and each bucket adds 2 h[a] pre[b] to a tile that joins R at
// the flush (u2 = 2 S + E, so the doubled cross sum belongs where the doubled
// in-bucket sum is).  The run's
// totals go to the hbg row of the run's first list slot, max(bk0, c CH), the
// only rows written: k_rank_cross_runs adds what the runs owe each other.
// A wave-uniform bound of what a tile entry may have received since the last
// flush keeps the 32-bit accumulators below A.run_bound: the accumulators are
// flushed when it would pass, pre runs on.  A bucket whose own term would pass
// it (a run that holds a tie group of millions) adds it in 64 bits instead.
template <int NC, bool VORD = false, bool RUNS = false>
__global__ void __launch_bounds__(256, NC >= 3 ? 2 : 1) k_rank_mfma16(ScRankLaunch A)  // NC >= 3: 2 waves / SIMD (NC = 4: 23 VGPRs spill)
{
    constexpr int NTL = NC * (NC + 1) / 2;
    constexpr int TL = NC == 1 ? 2 : NC == 2 ? 8 : 32;  // tested-pair list entries per lane (P <= 120 / 496 / 2016)
    __shared__ __attribute__((aligned(16))) RkWaveLds Ls[4];
    __shared__ u32 Lbuf[4][NTL * 256];   // one accumulator matrix of a flush, [tile][a & 15][b & 15]
    const int lane = threadIdx.x & 63, wv = scc_wave_id();
    RkWaveLds& Lw = Ls[wv];
    u32* buf = Lbuf[wv];
    const int NW = gridDim.x * 4, W = blockIdx.x * 4 + wv;
    const int cnt = min(rk_cnt(A, RK_CNT_WAVE_SLOTS), A.bucket_cap);
    const int K = A.K, G = A.G, P = A.P;
    const int CH = rk_chunk(cnt, (int)gridDim.x);
    const int g4 = lane >> 4, r16 = lane & 15;
    const int at16 = (lane ^ 16) << 2, at32 = (lane ^ 32) << 2, atrow = g4 << 4, atcol = r16 << 2;  // rk_lane_at addresses
    const rk_v4i zero = {0, 0, 0, 0};
    // L rows 16 mt + r16: bytes [e(g4, t) < i] (formed where used: held for the
    // whole kernel they were 16 registers of the 2-waves-per-SIMD budget at NC = 4)
    auto Lrow = [&](int mt) {
        rk_v4i l;
#pragma unroll
        for (int d = 0; d < 4; ++d) l[d] = (int)rk_lt_bytes(16 * mt + r16, 16 * d + 4 * g4);
        return l;
    };
    rk_v4i R[NTL], X[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) R[t] = X[t] = zero;
    Lw.F[lane] = 0;
    int cur = -1, ntp = 0, nrun = 0;
    bool rtie = false;
    u64 gk = ~0ull;
    // RUNS: the open run's prefix, its row, its chunk, its elements so far; the bound
    u32 pre[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) pre[t] = 0;
    // the cross term's own tiles, added to R at a flush (R lives in the matrix
    // cores' accumulator registers: adding there each bucket read and wrote them
    // back around every product, 264 us against 250 at config B)
    rk_v4i Cx[RUNS ? NTL : 1];
#pragma unroll
    for (int t = 0; t < (RUNS ? NTL : 1); ++t) Cx[t] = zero;
    int rrow = -1, rc0 = -1;
    u32 npre = 0, bnd = 0;  // (a gene holds fewer than 2^31 entries; bnd <= blim < 2^31)
    const u32 blim = min(A.run_bound, 0x7fffffffu);
    auto end_run = [&]() {
        if (rrow >= 0) {
#pragma unroll
            for (int t = 0; t < NC; ++t)
                if (g4 == 0 && r16 + 16 * t < K) A.hbg[(size_t)rrow * K + r16 + 16 * t] = pre[t];
        }
#pragma unroll
        for (int t = 0; t < NC; ++t) pre[t] = 0;
        npre = 0;
        rrow = -1;
    };
    const bool stm = A.dbg == 7;  // SCC_RW_DEBUG=7: phase clocks into g_rk_stamps
    u64 tph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = stm ? __builtin_amdgcn_s_memtime() : 0;
    auto stamp = [&](int ph) {
        if (stm) {
            const u64 t = __builtin_amdgcn_s_memtime();
            tph[ph] += t - tprev;
            tprev = t;
        }
    };
    auto flush = [&]() {
        ++tph[7];
        const u32* tl = A.gene_tp + (size_t)cur * P;
        // the tested-pair list in register chunks of <= 8 entries a lane (a
        // whole 2016-pair list in registers would cost the kernel its occupancy)
        constexpr int TLC = TL < 8 ? TL : 8;
        auto out = [&](rk_v4i* Mx, unsigned long long* acc) {
#pragma unroll
            for (int ma = 0; ma < NC; ++ma)
#pragma unroll
                for (int nb = ma; nb < NC; ++nb) {
                    const int t = rk_tile16<NC>(ma, nb);
#pragma unroll
                    for (int r = 0; r < 4; ++r) buf[t * 256 + (4 * g4 + r) * 16 + r16] = (u32)Mx[t][r];
                    Mx[t] = zero;
                }
            wsync();
            for (int q0 = 0; q0 < TL; q0 += TLC) {
                if (q0 * 64 >= ntp) break;
                u32 tv[TLC];
#pragma unroll
                for (int q = 0; q < TLC; ++q) tv[q] = tl[min((q0 + q) * 64 + lane, max(ntp - 1, 0))];
#pragma unroll
                for (int q = 0; q < TLC; ++q) {
                    if ((q0 + q) * 64 >= ntp) break;
                    const u32 v = tv[q];
                    const int a = (int)((v >> 16) & 0xffu), b = (int)(v >> 24);
                    const u32 x = buf[rk_tile16<NC>(a >> 4, b >> 4) * 256 + (a & 15) * 16 + (b & 15)];
                    if ((q0 + q) * 64 + lane < ntp && x)
                        atomicAdd(&acc[(size_t)(v & 0xffffu) * G + cur], (unsigned long long)x);
                }
            }
            wsync();
        };
        if constexpr (RUNS) {
#pragma unroll
            for (int t = 0; t < NTL; ++t) {
                R[t] += Cx[t];
                Cx[t] = zero;
            }
        }
        out(R, (unsigned long long*)A.accE);
        if (rtie) {
            out(X, (unsigned long long*)A.accX);
            const u64 f = Lw.F[lane];
            if (lane < K && f) atomicAdd((unsigned long long*)&A.accF[(size_t)lane * G + cur], (unsigned long long)f);
            Lw.F[lane] = 0;
            wsync();
        }
        nrun = 0;
        rtie = false;
        bnd = 0;
    };
    for (int c0 = W * CH; c0 < cnt; c0 += NW * CH) {
        const int c1 = min(cnt, c0 + CH);
        for (int s0 = c0; s0 < c1; s0 += 64) {
            const int s1 = min(c1, s0 + 64);
            ScRankItem D{0, 0, 0, 0, 0};
            if (lane < s1 - s0) D = A.sbuckets[s0 + lane];
            u64 rem;
            if constexpr (RUNS) {  // (every slot, so that each run's row is written)
                rem = __ballot(lane < s1 - s0);
            } else if (A.wv_filter) {
                const int ntg = (lane < s1 - s0 && D.n > 0) ? A.gene_nt[D.gene] : -1;
                rem = __ballot(ntg > A.wv_lo && ntg <= A.wv_hi);
            } else {
                rem = __ballot(lane < s1 - s0 && D.n > 0);
            }
            if (!rem) continue;
            const u32 dlo = (u32)(u64)D.base, dhi = (u32)((u64)D.base >> 32);
            auto dbase = [&](int li) {
                return (i64)(((u64)(u32)__builtin_amdgcn_readlane((int)dhi, li) << 32) |
                             (u32)__builtin_amdgcn_readlane((int)dlo, li));
            };
            // a bucket's first 64 elements (VORD: key = the vcell word, its tie bit in bit 31)
            auto load = [&](i64 b, int nl, u64& k, u32& cd) {
                if constexpr (VORD) {
                    const u32 w = lane < nl ? A.vcell[b + lane] : 0u;
                    const int c8 = lane < nl ? (int)A.code8[w & 0x7fffffffu] : -1;
                    k = (u64)w;
                    cd = c8 < 0 ? 255u : (u32)c8;
                } else {
                    k = lane < nl ? A.keys2[b + lane] : ~0ull;
                    cd = lane < nl ? (u32)A.codes2[b + lane] : 255u;
                }
            };
            u64 nkey;
            u32 ncode;
            {
                const int l0 = __builtin_ctzll(rem);
                load(dbase(l0), __builtin_amdgcn_readlane(D.n, l0), nkey, ncode);
            }
            while (rem) {
                const int li = __builtin_ctzll(rem);
                rem &= rem - 1;
                const int g = __builtin_amdgcn_readlane(D.gene, li);
                int n = __builtin_amdgcn_readlane(D.n, li);
                const int bucket = __builtin_amdgcn_readlane(D.bucket, li);
                const int src = __builtin_amdgcn_readlane(D.src, li);
                const i64 bbase = dbase(li);
                u64 key = nkey;
                u32 code = ncode;
                if (rem) {
                    const int l1 = __builtin_ctzll(rem);
                    load(dbase(l1), __builtin_amdgcn_readlane(D.n, l1), nkey, ncode);
                }
                const bool newrun = RUNS && (g != cur || c0 != rc0);
                if (newrun) end_run();
                if (g != cur || nrun >= 16384) {
                    if (cur >= 0) flush();
                    if (g != cur) {
                        cur = g;
                        if constexpr (!VORD) gk = A.gkmin[g];
                        ntp = A.gene_nt[g];
                    }
                }
                bool wide = false;  // RUNS: this bucket's cross term in 64 bits
                if constexpr (RUNS) {
                    if (newrun) {
                        // every slot is walked and a bucket's id is its slot: the run's
                        // first bucket is at max(bk0, c0), where k_rank_cross_runs looks
                        // (no load of gene_bk on the gene-change path)
                        rrow = bucket;
                        rc0 = c0;
                    }
                    if (src != 2) {
                        // a tile entry gets at most 2 n^2 from the bucket itself and 2 n npre from the run
                        // (n <= 64; the prefix below 2^24 keeps the products in the 24-bit multiplier)
                        const u32 own = 2u * (u32)n * (u32)n;
                        const u64 add64 = own + 2ull * (u64)n * npre;
                        wide = add64 > blim || npre >= (1u << 24);
                        const u32 add = wide ? own : (u32)add64;
                        if (bnd + add > blim && bnd) flush();
                        bnd += add;
                    }
                }
                ++nrun;
                ++tph[6];
                stamp(4);
                if (src == 2) {  // one repeated key: only the cluster histogram matters (as in k_rank_waves)
                    u32 myc = 0;
                    for (int i00 = 0; i00 < n; i00 += 256) {
                        u32 cd[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int i = i00 + u * 64 + lane;
                            if constexpr (VORD) {
                                const int c8 = i < n ? (int)A.code8[A.vcell[bbase + i] & 0x7fffffffu] : -1;
                                cd[u] = c8 < 0 ? 255u : (u32)c8;
                            } else {
                                cd[u] = i < n ? (u32)A.codes2[bbase + i] : 255u;
                            }
                        }
                        for (int c = 0; c < K; ++c) {
                            u32 t = 0;
#pragma unroll
                            for (int u = 0; u < 4; ++u) t += (u32)__popcll(__ballot(cd[u] == (u32)c));
                            if (lane == c) myc += t;
                        }
                    }
                    if (lane < K) {
                        if constexpr (!RUNS) A.hbg[(size_t)bucket * K + lane] = myc;
                        if (myc >= 2) Lw.F[lane] += f_tie(myc);
                    }
                    rtie = true;
                    Lw.cnt[lane] = myc;
                    if constexpr (RUNS) {
#pragma unroll
                        for (int t = 0; t < NC; ++t)
                            if (g4 == 0) Lw.pre[r16 + 16 * t] = pre[t];
                    }
                    wsync();
                    const u32* tl = A.gene_tp + (size_t)g * P;
                    for (int j = lane; j < ntp; j += 64) {
                        const u32 v = tl[j];
                        const u64 ca = Lw.cnt[(v >> 16) & 0xffu], cb = Lw.cnt[v >> 24];
                        const size_t o = (size_t)(v & 0xffffu) * G + g;
                        if (ca && cb) {
                            atomicAdd((unsigned long long*)&A.accE[o], (unsigned long long)(ca * cb));
                            atomicAdd((unsigned long long*)&A.accX[o], (unsigned long long)(ca * cb * (ca + cb)));
                        }
                        if constexpr (RUNS) {  // the group's a-elements above the run's earlier b-elements
                            const u64 pb = Lw.pre[v >> 24];
                            if (ca && pb) atomicAdd((unsigned long long*)&A.accS[o], (unsigned long long)(ca * pb));
                        }
                    }
                    if constexpr (RUNS) {
#pragma unroll
                        for (int t = 0; t < NC; ++t) pre[t] += Lw.cnt[r16 + 16 * t];
                        npre += (u32)n;
                    }
                    wsync();
                    stamp(5);
                    continue;
                }
                bool vl = lane < n;
                if constexpr (VORD) {
                    const u64 tb = __ballot(vl && ((key >> 31) & 1ull));
                    if (tb) {
                        // (lane 0 of a bucket starts a group: its bit is clear, so a group number is >= 1)
                        const u64 vm = (n >= 64) ? ~0ull : ((1ull << n) - 1);
                        const u64 le = (lane == 63) ? ~0ull : ((2ull << lane) - 1);
                        const u64 grp = (u64)__popcll(~tb & vm & le);
                        const bool kept = vl && code != 255u;
                        const int nk = __popcll(__ballot(kept));
                        static_assert(SCC_CODE_BITS <= 16, "the (group, code) sort key: 32 bits");
                        u32 ck = kept ? (((u32)grp << SCC_CODE_BITS) | code) : ~0u;  // (grp <= 64)
                        if (n > 1) bitonic_merge_ck32<1, 2>(ck);
                        if (n > 2) bitonic_merge_ck32<2, 4>(ck);
                        if (n > 4) bitonic_merge_ck32<4, 8>(ck);
                        if (n > 8) bitonic_merge_ck32<8, 16>(ck);
                        if (n > 16) bitonic_merge_ck32<16, 32>(ck);
                        if (n > 32) bitonic_merge_ck32<32, 0>(ck);
                        n = nk;  // the kept elements, in (group, code) order in the first lanes
                        vl = lane < n;
                        key = (u64)(ck >> SCC_CODE_BITS);
                        code = vl ? (ck & (u32)SCC_CODE_MASK) : 255u;
                    } else {
                        key = (u64)lane;  // every value its own group
                    }
                } else if (gk != ~0ull) {
                    u64 ck = vl ? (((key - gk) << SCC_CODE_BITS) | code) : ~0ull;
                    if (n > 1) bitonic_merge_ck<1, 2>(ck);
                    if (n > 2) bitonic_merge_ck<2, 4>(ck);
                    if (n > 4) bitonic_merge_ck<4, 8>(ck);
                    if (n > 8) bitonic_merge_ck<8, 16>(ck);
                    if (n > 16) bitonic_merge_ck<16, 32>(ck);
                    if (n > 32) bitonic_merge_ck<32, 0>(ck);
                    key = ck >> SCC_CODE_BITS;
                    code = vl ? (u32)(ck & SCC_CODE_MASK) : 255u;
                } else {
                    if (n > 1) bitonic_merge<1>(key, code, (lane & 2) == 0, lane);
                    if (n > 2) bitonic_merge<2>(key, code, (lane & 4) == 0, lane);
                    if (n > 4) bitonic_merge<4>(key, code, (lane & 8) == 0, lane);
                    if (n > 8) bitonic_merge<8>(key, code, (lane & 16) == 0, lane);
                    if (n > 16) bitonic_merge<16>(key, code, (lane & 32) == 0, lane);
                    if (n > 32) bitonic_merge<32>(key, code, true, lane);
                }
                stamp(0);
                // ---- one-hot operand: sorted codes at their slots, element i at
                // byte 16 ((i >> 2) & 3) + 4 (i >> 4) + (i & 3)
                const int sg = (((lane >> 2) & 3) << 4) | ((lane >> 4) << 2) | (lane & 3);
                Lw.code[sg] = (u8)code;
                wsync();
                const rk_v4i cw = *(const rk_v4i*)(Lw.code + 16 * g4);
                rk_v4i ob[NC];
#pragma unroll
                for (int t = 0; t < NC; ++t)
#pragma unroll
                    for (int d = 0; d < 4; ++d) ob[t][d] = (int)rk_eq_bytes((u32)cw[d], (u32)(r16 + 16 * t));
                u32 hc[NC];  // (RUNS) the bucket's count of cluster r16 + 16 t, in every lane group
#pragma unroll
                for (int t = 0; t < NC; ++t) {  // the bucket's cluster histogram row
                    u32 c = 0;  // the sum of the sixteen 0 / 1 bytes
#pragma unroll
                    for (int d = 0; d < 4; ++d) c = __builtin_amdgcn_sad_u8((u32)ob[t][d], 0u, c);
                    c += rk_lane_at(at16, c);
                    c += rk_lane_at(at32, c);
                    hc[t] = c;
                    if constexpr (!RUNS)
                        if (g4 == 0 && r16 + 16 * t < K) A.hbg[(size_t)bucket * K + r16 + 16 * t] = c;
                }
                stamp(1);
                // ---- M = L O (row tiles of 16 elements), R += O^T (2 M)
                const int nmt = (n + 15) >> 4;
                rk_v4i mb[NC];
#pragma unroll
                for (int t = 0; t < NC; ++t) mb[t] = zero;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    if (mt >= nmt) break;
                    const rk_v4i Lmt = Lrow(mt);
#pragma unroll
                    for (int t = 0; t < NC; ++t) {
                        const rk_v4i m = rk_mfma16(Lmt, ob[t], zero);
                        mb[t][mt] = (int)((u32)(2 * m[0]) | ((u32)(2 * m[1]) << 8) | ((u32)(2 * m[2]) << 16) |
                                          ((u32)(2 * m[3]) << 24));
                    }
                }
#pragma unroll
                for (int ma = 0; ma < NC; ++ma)
#pragma unroll
                    for (int nb = ma; nb < NC; ++nb) {
                        const int t = rk_tile16<NC>(ma, nb);
                        R[t] = rk_mfma16(ob[ma], mb[nb], R[t]);
                    }
                if constexpr (RUNS) {
                    // ---- the run's cross term: rows 16 ma + 4 g4 + r of this bucket's
                    // histogram against the prefix of column 16 nb + r16, then pre += h
                    if (!wide) {
#pragma unroll
                        for (int ma = 0; ma < NC; ++ma) {
                            u32 hr[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) hr[r] = rk_lane_at(atrow + 4 * r, 2u * hc[ma]);
#pragma unroll
                            for (int nb = ma; nb < NC; ++nb) {
                                const int t = rk_tile16<NC>(ma, nb);
#pragma unroll
                                for (int r = 0; r < 4; ++r) Cx[t][r] += (int)__umul24(hr[r], pre[nb]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int t = 0; t < NC; ++t)
                            if (g4 == 0) {
                                Lw.cnt[r16 + 16 * t] = hc[t];
                                Lw.pre[r16 + 16 * t] = pre[t];
                            }
                        wsync();
                        const u32* tl = A.gene_tp + (size_t)g * P;
                        for (int j = lane; j < ntp; j += 64) {
                            const u32 v = tl[j];
                            const u64 ca = Lw.cnt[(v >> 16) & 0xffu], pb = Lw.pre[v >> 24];
                            if (ca && pb)
                                atomicAdd((unsigned long long*)&A.accS[(size_t)(v & 0xffffu) * G + g],
                                          (unsigned long long)(ca * pb));
                        }
                        wsync();
                    }
#pragma unroll
                    for (int t = 0; t < NC; ++t) pre[t] += hc[t];
                    npre += (u32)n;
                }
                stamp(2);
                // ---- tie groups and runs
                const u64 kp = ((u64)rk_lane_up1((u32)(key >> 32)) << 32) | (u64)rk_lane_up1((u32)key);
                const u32 cpv = rk_lane_up1(code);
                const u64 vmask = (n >= 64) ? ~0ull : ((1ull << n) - 1);
                const bool gs_me = (lane == 0) || (kp != key);
                const u64 gst = __ballot(gs_me && vl);
                const bool anytie = ((~gst) & vmask & ~1ull) != 0;
                if (anytie) {
                    rtie = true;
                    const u64 le = (lane == 63) ? ~0ull : ((2ull << lane) - 1);
                    const bool rs_me = (lane == 0) || (kp != key) || (cpv != code);
                    const u64 rst = __ballot(rs_me && vl);
                    const u64 raft = rst & ~le;
                    const int re = raft ? __builtin_ctzll(raft) : n;
                    const int rs = 63 - __clzll((long long)((rst & le) | 1ull));
                    if (rs_me && vl && re - lane >= 2)
                        atomicAdd((unsigned long long*)&Lw.F[code], (unsigned long long)f_tie((u64)(re - lane)));
                    const int gs = 63 - __clzll((long long)((gst & le) | 1ull));
                    const u64 gaft = gst & ~le;
                    const int ge = gaft ? __builtin_ctzll(gaft) : n;
                    Lw.dcnt[sg] = (u8)(vl ? re - rs : 0);
                    wsync();
                    const rk_v4i dw = *(const rk_v4i*)(Lw.dcnt + 16 * g4);
                    rk_v4i odb[NC], qb[NC];
#pragma unroll
                    for (int t = 0; t < NC; ++t) {
                        qb[t] = zero;
#pragma unroll
                        for (int d = 0; d < 4; ++d) odb[t][d] = (int)(((u32)ob[t][d] * 0xffu) & (u32)dw[d]);
                    }
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        if (mt >= nmt) break;
                        const int gsr = (int)rk_lane_at(atcol + 64 * mt, (u32)gs), ger = (int)rk_lane_at(atcol + 64 * mt, (u32)ge);
                        rk_v4i eq;
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            eq[d] = (int)(rk_lt_bytes(ger, 16 * d + 4 * g4) - rk_lt_bytes(gsr, 16 * d + 4 * g4));
#pragma unroll
                        for (int t = 0; t < NC; ++t) {
                            const rk_v4i q = rk_mfma16(eq, ob[t], zero);
                            qb[t][mt] = (int)((u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24));
                        }
                    }
#pragma unroll
                    for (int ma = 0; ma < NC; ++ma)
#pragma unroll
                        for (int nb = ma; nb < NC; ++nb) {
                            const int t = rk_tile16<NC>(ma, nb);
                            R[t] = rk_mfma16(ob[ma], qb[nb], R[t]);
                            X[t] = rk_mfma16(odb[ma], qb[nb], X[t]);
                            X[t] = rk_mfma16(qb[ma], odb[nb], X[t]);
                        }
                    wsync();
                }
                wsync();
                stamp(3);
            }
        }
    }
    if constexpr (RUNS) end_run();
    if (cur >= 0) flush();
    stamp(4);
    if (stm && lane == 0)
        for (int q = 0; q < 8; ++q) atomicAdd(&g_rk_stamps[q], (unsigned long long)tph[q]);
}

static hipError_t rank_waves_launches(const ScRankLaunch* L, int grid, SideStreams& ss);

extern "C" hipError_t scc_launch_rank_waves(const ScRankLaunch* L, int grid, hipStream_t st0, const hipStream_t* side,
                                            int nside, hipEvent_t fork, const hipEvent_t* join)
{
    SideStreams ss(st0, side, nside, fork, join);
    const hipError_t e = rank_waves_launches(L, grid, ss);
    ss.end();
    return e != hipSuccess ? e : hipGetLastError();
}

template <bool VORD>
static hipError_t rank_waves_launches_t(const ScRankLaunch* L, int grid, SideStreams& ss)
{
    // the launches below touch disjoint genes' accumulator cells (each gene is
    // in one class) or, for the windows of one gene, disjoint pair rows, and
    // read only what the split wrote: they may run concurrently, so each takes
    // the next stream in turn and their tails overlap (a gene shard's grid is
    // an eighth of the whole job's and each launch ended on a long tail)
    // With two sides (the runtime passes {a side stream, the LDS items'
    // stream}: three hardware queues) the launches take fixed places, longest
    // chains apart (config D timeline, profiles/r06_timeline_rank_d_*.txt):
    // matrix-core genes on side 1 ahead of the items, <= 128 tested pairs on
    // side 0 (the largest class), <= 256 then <= 512 on st0.  Otherwise round robin.
    auto next_stream = [&]() { return ss.next(); };
    auto place = [&](int role) {  // 0..3: slot class, 4: matrix cores, 5: windows
        if (ss.nside < 2) return ss.next();
        static const int where[6] = {0, -1, -1, 1, 1, -1};
        return ss.pick(where[role]);
    };
    hipStream_t st = ss.st0;
    // one launch per slot class present: genes with <= 128 tested pairs on the
    // 2-slot kernel, <= 256 on 4, <= 512 on 8, <= 1024 on 16
    // the matrix-core kernel (K <= 64) counts all K^2 pairs of a bucket at a
    // fixed cost: it takes the genes with more than 512 tested pairs (SLOW at
    // config D: every gene, 1225 pairs), the slot kernels the others
    // (SCC_RANK_MFMA=2: every gene on the matrix cores, 0: none)
    // (from 256 or 128 tested pairs, or every gene, measured slower at config D: rank
    // 22.6 / 29.0 / 31.9 vs 20.2 ms, round 6)
    constexpr int mfma_min = 512;  // the tested-pair count past which a gene goes there
    const int hi[4] = {128, 256, 512, 1024};
    const bool mfma = L->rw_mfma && L->K <= 64 && (L->rw_mfma == 2 || 64 * L->rw_slots > mfma_min);
    if (mfma) {
        ScRankLaunch M = *L;
        M.wv_filter = L->rw_mfma == 2 ? 0 : 1;
        M.wv_lo = mfma_min;
        st = place(4);
        M.wv_hi = 1 << 30;
        if (L->K <= 16 && VORD && L->rank_runs && !M.wv_filter)
            hipLaunchKernelGGL((k_rank_mfma16<1, VORD, VORD>), dim3(grid), dim3(256), 0, st, M);
        else if (L->K <= 16)
            hipLaunchKernelGGL((k_rank_mfma16<1, VORD>), dim3(grid), dim3(256), 0, st, M);
        else if (L->K <= 32)
            hipLaunchKernelGGL((k_rank_mfma16<2, VORD>), dim3(grid), dim3(256), 0, st, M);
        else if (L->K <= 48)
            hipLaunchKernelGGL((k_rank_mfma16<3, VORD>), dim3(grid), dim3(256), 0, st, M);
        else
            hipLaunchKernelGGL((k_rank_mfma16<4, VORD>), dim3(grid), dim3(256), 0, st, M);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || L->rw_mfma == 2) return e;
    }
    ScRankLaunch A = *L;
    // the 16-wide matrix-core kernel for the genes the slot kernels would take:
    // by default at K <= 16 (four waves per SIMD; config B rank 0.785 -> 0.744
    // ms), SCC_RANK_MFMA16=1 also at K <= 32 (two waves: config C 8.6 -> 10.2 ms)
    if (L->rw_mfma16 > 0 ? L->K <= 32 : (L->rw_mfma16 < 0 && L->K <= 16)) {
        ScRankLaunch M = *L;
        M.wv_filter = mfma ? 1 : 0;
        M.wv_lo = -1;
        M.wv_hi = mfma ? mfma_min : (1 << 30);
        if (L->K <= 16 && VORD && L->rank_runs && !M.wv_filter)
            hipLaunchKernelGGL((k_rank_mfma16<1, VORD, VORD>), dim3(grid), dim3(256), 0, st, M);
        else if (L->K <= 16)
            hipLaunchKernelGGL((k_rank_mfma16<1, VORD>), dim3(grid), dim3(256), 0, st, M);
        else
            hipLaunchKernelGGL((k_rank_mfma16<2, VORD>), dim3(grid), dim3(256), 0, st, M);
        return hipGetLastError();
    }
    if (L->rank_runs) return hipErrorInvalidValue;  // (run rows come from the matrix-core kernel alone)
    for (int c = 0; c < 4; ++c) {
        if (c > 0 && 64 * L->rw_slots < hi[c]) break;
        if (mfma && hi[c] > mfma_min) return hipSuccess;  // the genes past mfma_min: done on the matrix cores
        A.wv_lo = c ? hi[c - 1] : -1;
        A.wv_hi = hi[c];
        A.wv_base = 0;
        A.wv_filter = L->rw_slots > 2 ? 1 : 0;  // rw_slots 2: class 0 is the only launch and holds every gene
        st = place(c);
        if (c == 0)
            hipLaunchKernelGGL((k_rank_waves<2, VORD>), dim3(grid), dim3(256), 0, st, A);
        else if (c == 1)
            hipLaunchKernelGGL((k_rank_waves<4, VORD>), dim3(grid), dim3(256), 0, st, A);
        else if (c == 2)
            hipLaunchKernelGGL((k_rank_waves<8, VORD>), dim3(grid), dim3(256), 0, st, A);
        else
            hipLaunchKernelGGL((k_rank_waves<RW_SLOTS_MAX, VORD>), dim3(grid), dim3(256), 0, st, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // genes with more than 1024 tested pairs (SLOW at K > 45, K > 64 runs): one
    // 16-slot pass per window of 1024 pairs, window k over the genes that reach it
    if (L->rw_slots >= RW_SLOTS_MAX) {
        const int per = 64 * RW_SLOTS_MAX;
        const int npass = (std::min(L->ntp_max, RW_PAIRS_MAX) + per - 1) / per;
        st = place(5);  // (the windows in one stream)
        for (int k = 0; k < npass; ++k) {
            A.wv_lo = std::max(per, k * per);
            A.wv_hi = RW_PAIRS_MAX;
            A.wv_base = k * per;
            A.wv_filter = 1;
            hipLaunchKernelGGL((k_rank_waves<RW_SLOTS_MAX, VORD>), dim3(grid), dim3(256), 0, st, A);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// (a launch that carries the dataset's value order: the VORD kernels)
static hipError_t rank_waves_launches(const ScRankLaunch* L, int grid, SideStreams& ss)
{
    return L->vcell ? rank_waves_launches_t<true>(L, grid, ss) : rank_waves_launches_t<false>(L, grid, ss);
}
