// scc_vorder.hip — the value order of the dataset's gene-major mirror.
//
// Inside a gene the ascending order of its stored values depends on the matrix
// alone (only the cluster code attached to a value depends on a call's
// labels), so a dataset that keeps the mirror keeps that order too:
//   vcell[nnz]   each gene's entries in ascending key order, equal keys in
//                ascending cell order (a stable sort of the mirror's segment,
//                which is in cell order): the cell index in the low 31 bits,
//                bit 31 set when the entry's key equals the previous entry's
//                key of the same gene
//   vbk_ptr[G+1] / vbk[]  each gene's bucket cuts, positions inside its sorted
//                segment, made greedily from the segment's start: a bucket ends
//                at the last group start within the next 64 entries, so it holds
//                at most 64 entries and never divides a tie group; a tie group
//                of more than 64 entries is a bucket of its own (bit 31)
// The rank stage of a FAST Wilcoxon run over the whole gene range walks these
// buckets and sorts only inside tie groups (scc_rank_split.hip: k_rank_vorder_list,
// then the VORD variants of k_rank_mfma16 and k_rank_waves, scc_rank_waves.hip).
//
// The sort is rocPRIM's segmented radix sort of (key, cell) pairs, run over
// blocks of whole genes so that its scratch fits what the caller lends it (two
// of the run's workspace buffers, idle before the ingest).  A radix sort is
// stable and the cuts are a sequential rule, so the arrays do not depend on
// launch geometry.
#include "scc_common.hpp"
#include <algorithm>
#include <vector>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include "scc_kernels.hpp"

#define VO_TIE 0x80000000u
// stored values sorted per rocPRIM call (a longer gene goes alone): as many as
// the lent scratch holds at about 12.5 B a value, so a large dataset goes in two
// calls whose long segments share the device (8 M a call left D's 350 genes a
// call alone on it)
static i64 vo_block(i64 nnz, i64 ks_n, size_t tmp_bytes)
{
    const i64 fit = std::min<i64>(ks_n, (i64)(tmp_bytes / 25) * 2);
    return std::max<i64>(1ll << 20, std::min<i64>({fit, nnz, 1ll << 30}));
}

// segment offsets of the genes [g0, g0 + ng] relative to the block's first entry
__global__ void k_vord_offsets(const i64* __restrict__ gptr, int g0, int ng, u32* __restrict__ off)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= ng) off[i] = (u32)(gptr[g0 + i] - gptr[g0]);
}

// ks: the block's sorted keys (relative to the block's first entry)
__global__ void __launch_bounds__(256) k_vord_mark(const i64* __restrict__ gptr, int g0, const u64* __restrict__ ks,
                                                   u32* __restrict__ vcell)
{
    const int g = g0 + blockIdx.x;
    const i64 b = gptr[g], off0 = gptr[g0];
    const i64 n = gptr[g + 1] - b;
    const u64* k = ks + (b - off0);
    for (i64 i = threadIdx.x; i < n; i += 256)
        if (i > 0 && k[i] == k[i - 1]) vcell[b + i] |= VO_TIE;
}

// One wave per gene, buckets in order.  From a bucket's start s the
// candidates for its end are e in (s, s + 64]: a group start (tie bit clear)
// or the segment's end; the last one is taken.  None: the group at s is
// longer than 64, and the bucket is that group.
// FILL false: nbk[g] = the gene's buckets; true: vbk_ptr (from the scan) and vbk.
template <bool FILL>
__global__ void __launch_bounds__(256) k_vord_cuts(const i64* __restrict__ gptr, const u32* __restrict__ vcell, int G,
                                                   u32* __restrict__ nbk, const i64* __restrict__ bptr,
                                                   u32* __restrict__ vbk_ptr, u32* __restrict__ vbk)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const i64 base = gptr[g];
    const int n = (int)(gptr[g + 1] - base);
    const u32* v = vcell + base;
    const i64 o = FILL ? bptr[g] : 0;
    if (FILL && lane == 0) {
        vbk_ptr[g] = (u32)o;
        if (g == G - 1) vbk_ptr[G] = (u32)bptr[G];
    }
    auto starts = [&](int q) {  // of the positions q + lane: group starts, or the segment's end
        const int e = q + lane;
        return __ballot(e <= n && (e == n || !(v[e] & VO_TIE)));
    };
    u32 nb = 0;
    int s = 0;
    while (s < n) {
        int end;
        u32 fat = 0;
        const u64 m = starts(s + 1);
        if (m) {
            end = s + 1 + (63 - __clzll((long long)m));
        } else {  // (n > s + 64: a later window holds the segment's end)
            fat = VO_TIE;
            for (int q = s + 65;; q += 64) {
                const u64 m2 = starts(q);
                if (m2) {
                    end = q + __builtin_ctzll(m2);
                    break;
                }
            }
        }
        if (FILL && lane == 0) vbk[o + nb] = (u32)s | fat;
        ++nb;
        s = end;
    }
    if (!FILL && lane == 0) nbk[g] = nb;
}

// vcell: [max(1, nnz)], vbk_ptr: [G + 1]; *vbk_out is allocated here (hipMalloc;
// the caller frees it) unless it would pass vbk_max_bytes: then *vbk_out stays
// nullptr and hipSuccess is returned.  cnt: [G] u32, bptr: [G + 1], scan_scratch:
// the scan's block sums (scc_scan_scratch_blocks(G) + 1).
// ks_lent [ks_n] and tmp_lent [tmp_lent_bytes]: the sort's scratch (its sorted
// keys and rocPRIM's temporary storage); what they cannot hold is allocated here.
extern "C" hipError_t scc_launch_vorder_build(const i64* gptr, int G, const u32* mcell, const u64* mkey, u32* vcell,
                                              u32* vbk_ptr, u32** vbk_out, i64* nbk_out, u32* cnt, i64* bptr,
                                              i64* scan_scratch, size_t vbk_max_bytes, u64* ks_lent, i64 ks_n,
                                              void* tmp_lent, size_t tmp_lent_bytes, hipStream_t st)
{
    *vbk_out = nullptr;
    *nbk_out = 0;
    std::vector<i64> gp((size_t)G + 1);
    hipError_t e = hipMemcpyAsync(gp.data(), gptr, sizeof(i64) * gp.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    // ---- the sort, over blocks of whole genes
    const i64 VO_BLOCK = vo_block(gp[G], ks_lent ? ks_n : 0, tmp_lent ? tmp_lent_bytes : 0);
    i64 cap = 1;
    int seg_cap = 1;
    for (int g0 = 0; g0 < G;) {
        int g1 = g0 + 1;
        while (g1 < G && gp[g1 + 1] - gp[g0] <= VO_BLOCK) ++g1;
        cap = std::max(cap, gp[g1] - gp[g0]);
        seg_cap = std::max(seg_cap, g1 - g0);
        g0 = g1;
    }
    if (cap >= (1ll << 31)) return hipErrorInvalidValue;
    u64 *ks = nullptr, *ks_own = nullptr;
    u32* off = nullptr;
    void *tmp = tmp_lent, *tmp_own = nullptr;
    size_t tmp_n = tmp_lent ? tmp_lent_bytes : 0;
    auto done = [&](hipError_t r) {
        hipFree(ks_own);
        hipFree(off);
        hipFree(tmp_own);
        return r;
    };
    if (ks_lent && ks_n >= cap)
        ks = ks_lent;
    else if ((e = hipMalloc((void**)&ks_own, sizeof(u64) * (size_t)cap)) != hipSuccess)
        return done(e);
    else
        ks = ks_own;
    if ((e = hipMalloc((void**)&off, sizeof(u32) * ((size_t)seg_cap + 1))) != hipSuccess) return done(e);
    for (int g0 = 0; g0 < G;) {
        int g1 = g0 + 1;
        while (g1 < G && gp[g1 + 1] - gp[g0] <= VO_BLOCK) ++g1;
        const i64 b0 = gp[g0], m = gp[g1] - b0;
        const int ng = g1 - g0;
        if (m > 0) {
            hipLaunchKernelGGL(k_vord_offsets, dim3(ng / 256 + 1), dim3(256), 0, st, gptr, g0, ng, off);
            size_t need = 0;
            e = rocprim::segmented_radix_sort_pairs(nullptr, need, mkey + b0, ks, mcell + b0, vcell + b0, (unsigned)m,
                                                    (unsigned)ng, off, off + 1, 0, 64, st);
            if (e != hipSuccess) return done(e);
            if (need > tmp_n) {
                if ((e = hipStreamSynchronize(st)) != hipSuccess) return done(e);
                hipFree(tmp_own);
                tmp_own = nullptr;
                tmp_n = 0;
                if ((e = hipMalloc(&tmp_own, need)) != hipSuccess) return done(e);
                tmp = tmp_own;
                tmp_n = need;
            }
            e = rocprim::segmented_radix_sort_pairs(tmp, need, mkey + b0, ks, mcell + b0, vcell + b0, (unsigned)m,
                                                    (unsigned)ng, off, off + 1, 0, 64, st);
            if (e != hipSuccess) return done(e);
            hipLaunchKernelGGL(k_vord_mark, dim3(ng), dim3(256), 0, st, gptr, g0, ks, vcell);
        }
        g0 = g1;
    }
    if ((e = hipGetLastError()) != hipSuccess) return done(e);
    // ---- the cuts: count, scan, fill
    const dim3 grid((G + 3) / 4);
    hipLaunchKernelGGL(k_vord_cuts<false>, grid, dim3(256), 0, st, gptr, vcell, G, cnt, nullptr, nullptr, nullptr);
    if ((e = scc_launch_scan(cnt, G, bptr, scan_scratch, bptr + G, st)) != hipSuccess) return done(e);
    i64 nbk = 0;
    e = hipMemcpyAsync(&nbk, bptr + G, sizeof(i64), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the sort's scratch is no longer read)
    if (e != hipSuccess) return done(e);
    done(hipSuccess);
    if (nbk >= (1ll << 31)) return hipErrorInvalidValue;
    const size_t vbk_bytes = sizeof(u32) * (size_t)std::max<i64>(1, nbk);
    if (vbk_bytes > vbk_max_bytes) return hipSuccess;
    u32* vbk = nullptr;
    if ((e = hipMalloc((void**)&vbk, vbk_bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vord_cuts<true>, grid, dim3(256), 0, st, gptr, vcell, G, nullptr, bptr, vbk_ptr, vbk);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        hipFree(vbk);
        return e;
    }
    *vbk_out = vbk;
    *nbk_out = nbk;
    return hipSuccess;
}
