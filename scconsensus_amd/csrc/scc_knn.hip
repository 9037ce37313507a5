// scc_knn.hip — exact k nearest neighbours of every cell from the PCA scores.
//
// Reference: the neighbour search umap::umap(d = pca.data) starts with (the
// README's worked example, pca.data = pca.obj$x[, 1:8]).  The distance is
// dist() of the [N][16] scores: each entry d(i, j) is computed from two score
// rows with the dist kernel's arithmetic (scc_dist_entry.hpp), so a returned
// distance is bit for bit the entry of the packed f64 vector of the same
// scores, and nothing N x N exists.
//
// The order is total: (distance ascending, index ascending).  The k smallest
// keys of a row are one set and one sequence whatever the tiling, the chunking
// or the merge, so two calls give the same bits.
//
// k_knn_partial  a lane owns a row: its leading `dims` scores (the others taken
//                as zero) and its norm in registers.  The workgroup shares a
//                column chunk (blockIdx.y), staged through LDS a tile of
//                KNN_TILE columns at a time with the norm in the 16th slot;
//                every lane of a wave reads the same staged column (one
//                address: a broadcast).  The row's k best so far sit unsorted
//                in LDS, slot s of row r at [s][r] (conflict-free), with the
//                largest key and its slot in registers: an entry is compared
//                with that key, and only a smaller one replaces the slot and
//                rescans the k slots for the new largest.  At the end of the
//                chunk the list leaves in key order, padded with (inf, INT_MAX)
//                where the chunk had fewer than k columns.
// k_knn_merge    a thread per row merges the chunks' sorted lists by their
//                heads under the same key.
//
// Template: D components enter the fma chains (8 or 15; a chain over zeros is
// an exact no-op, so D > dims changes no bit), R rows per workgroup and KCAP
// list slots per row (LDS: 12 KCAP R bytes of lists beside the 18 KiB tile).
#include "scc_common.hpp"
#include "scc_dist_entry.hpp"

#include <climits>

#define KNN_TILE 128   // columns staged per LDS tile
#define KNN_LD 18      // doubles per staged column: 15 scores, |p|^2, 2 of padding (conflict-free 16-byte stores)
#define KNN_MAX_CH 16  // column chunks (grid.y) at most
#define KNN_U 4        // columns whose entries are formed before their compares
#define KNN_WGS 512    // workgroups a launch aims for when it picks the chunk count (two per CU are resident)

typedef double knn_dv2 __attribute__((ext_vector_type(2)));

__device__ inline bool knn_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

template <int D, int R, int KCAP>
__global__ void __launch_bounds__(R) k_knn_partial(const double* __restrict__ P, int N, int dims, int k, int row0,
                                                   int row1, int nch, int ldp, double* __restrict__ part_d,
                                                   int* __restrict__ part_i)
{
    static_assert(KNN_TILE % KNN_U == 0 && KNN_LD % 2 == 0 && D <= 15, "whole compare groups, 16-byte staged rows");
    __shared__ __attribute__((aligned(16))) double tile[KNN_TILE * KNN_LD];
    __shared__ double best_d[KCAP * R];
    __shared__ int best_i[KCAP * R];
    const int tid = threadIdx.x;
    const int i = row0 + blockIdx.x * R + tid;  // a lane past row1 computes on row N - 1 and writes nothing
    const int ch = blockIdx.y;
    const int per = (N + nch - 1) / nch;
    const int J0 = (int)min((long long)N, (long long)ch * per), J1 = min(N, J0 + per);
    double pi[D];
    {
        const int ic = min(i, N - 1);
#pragma unroll
        for (int q = 0; q < D; ++q) pi[q] = q < dims ? P[(size_t)ic * 16 + q] : 0.0;
    }
    const double ni = scc_dist_norm_lead<D>(pi);
    double kd = INFINITY;  // the largest key kept, once k are kept
    int ki = INT_MAX, kpos = 0, cnt = 0;
    for (int T0 = J0; T0 < J1; T0 += KNN_TILE) {
        __syncthreads();  // the previous tile is read
        for (int c = tid; c < KNN_TILE; c += R) {
            const int jc = T0 + c;
            double pj[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) pj[q] = (jc < J1 && q < dims) ? P[(size_t)jc * 16 + q] : 0.0;
            pj[15] = scc_dist_norm_lead<D>(pj);
#pragma unroll
            for (int q = 0; q < 16; q += 2) *(knn_dv2*)&tile[c * KNN_LD + q] = knn_dv2{pj[q], pj[q + 1]};
        }
        __syncthreads();
        const int nt = min(J1 - T0, KNN_TILE);
        for (int c0 = 0; c0 < nt; c0 += KNN_U) {  // c0 + u < KNN_TILE; a column past nt is staged as zeros and skipped
            double e[KNN_U];
#pragma unroll
            for (int u = 0; u < KNN_U; ++u) {
                double pj[16];
#pragma unroll
                for (int q = 0; q < 16; q += 2) {
                    const knn_dv2 v = *(const knn_dv2*)&tile[(c0 + u) * KNN_LD + q];
                    pj[q] = v.x;
                    pj[q + 1] = v.y;
                }
                e[u] = scc_dist_entry_lead<D>(pi, ni, pj, pj[15]);
            }
#pragma unroll
            for (int u = 0; u < KNN_U; ++u) {
                const int j = T0 + c0 + u;
                if (j < J1 && j != i && knn_less(e[u], j, kd, ki)) {  // rare once the list has settled
                    const int slot = cnt < k ? cnt++ : kpos;           // slot < k <= KCAP
                    best_d[slot * R + tid] = e[u];
                    best_i[slot * R + tid] = j;
                    if (cnt == k) {  // the largest key kept, again
                        kd = best_d[tid];
                        ki = best_i[tid];
                        kpos = 0;
#pragma unroll 8
                        for (int s = 1; s < k; ++s) {  // (unrolled: the reads of a group are in flight together)
                            const double d = best_d[s * R + tid];
                            const int x = best_i[s * R + tid];
                            if (knn_less(kd, ki, d, x)) {
                                kd = d;
                                ki = x;
                                kpos = s;
                            }
                        }
                    }
                }
            }
        }
    }
    if (i >= row1) return;
    // the list in key order: k passes, each taking the smallest key after the last one written
    double last_d = -1.0;  // every entry is >= 0
    int last_i = -1;
    for (int s = 0; s < k; ++s) {
        double bd = INFINITY;
        int bi = INT_MAX;
        if (s < cnt)
            for (int t = 0; t < cnt; ++t) {
                const double d = best_d[t * R + tid];
                const int x = best_i[t * R + tid];
                if (knn_less(last_d, last_i, d, x) && knn_less(d, x, bd, bi)) {
                    bd = d;
                    bi = x;
                }
            }
        last_d = bd;
        last_i = bi;
        const size_t o = ((size_t)ch * k + s) * ldp + (i - row0);
        part_d[o] = bd;
        part_i[o] = bi;
    }
}

// rows [row0, row1): the nch sorted lists of a row -> its k neighbours
__global__ void __launch_bounds__(256) k_knn_merge(const double* __restrict__ part_d, const int* __restrict__ part_i,
                                                   int k, int row0, int row1, int nch, int ldp,
                                                   int* __restrict__ idx, double* __restrict__ dist)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (row0 + r >= row1) return;
    double hd[KNN_MAX_CH];
    int hi[KNN_MAX_CH], hp[KNN_MAX_CH];
#pragma unroll
    for (int c = 0; c < KNN_MAX_CH; ++c) {
        hp[c] = 0;
        hd[c] = c < nch ? part_d[((size_t)c * k) * ldp + r] : INFINITY;
        hi[c] = c < nch ? part_i[((size_t)c * k) * ldp + r] : INT_MAX;
    }
    for (int s = 0; s < k; ++s) {
        double bd = hd[0];
        int bi = hi[0], bc = 0;
#pragma unroll
        for (int c = 1; c < KNN_MAX_CH; ++c)
            if (knn_less(hd[c], hi[c], bd, bi)) {
                bd = hd[c];
                bi = hi[c];
                bc = c;
            }
        idx[(size_t)(row0 + r) * k + s] = bi;
        dist[(size_t)(row0 + r) * k + s] = bd;
#pragma unroll
        for (int c = 0; c < KNN_MAX_CH; ++c)
            if (c == bc) {
                const bool more = ++hp[c] < k;  // (c < nch: a chunk past nch never wins against the k valid keys)
                hd[c] = more ? part_d[((size_t)c * k + hp[c]) * ldp + r] : INFINITY;
                hi[c] = more ? part_i[((size_t)c * k + hp[c]) * ldp + r] : INT_MAX;
            }
    }
}

// rows per workgroup for k neighbours
static int knn_wg_rows(int k) { return k <= 32 ? 256 : 128; }

// Rows per launch and column chunks.  A launch forms about 2^36 entries at most
// (a few tenths of a second), in whole workgroups; rows_forced > 0 sets the
// rows instead.  The chunks fill the device when the rows alone do not, and no
// further: every chunk fills a list of its own, and filling is the slow part.
extern "C" void scc_knn_plan(int N, int k, int rows_forced, int* rows_per_launch, int* nch)
{
    const int R = knn_wg_rows(k);
    long long rows = rows_forced > 0 ? rows_forced : (1LL << 36) / N;
    rows = (std::min<long long>(rows, N) + R - 1) / R * R;
    const int blocks = (int)(rows / R);
    *rows_per_launch = (int)rows;
    *nch = std::max(1, std::min(std::min(KNN_MAX_CH, (N + KNN_TILE - 1) / KNN_TILE), KNN_WGS / blocks));
}

extern "C" size_t scc_knn_scratch_entries(int N, int k, int rows_forced)
{
    int rows, nch;
    scc_knn_plan(N, k, rows_forced, &rows, &nch);
    return (size_t)nch * k * rows;
}

template <int D, int R, int KCAP>
static void knn_launch_partial(const double* P, int N, int dims, int k, int row0, int row1, int nch, int ldp,
                               double* part_d, int* part_i, hipStream_t st)
{
    const dim3 grid((row1 - row0 + R - 1) / R, nch);
    hipLaunchKernelGGL((k_knn_partial<D, R, KCAP>), grid, dim3(R), 0, st, P, N, dims, k, row0, row1, nch, ldp, part_d,
                       part_i);
}

// idx, dist: device [N][k].  dims in 1..15, 1 <= k <= min(N - 1, 64); part_d and
// part_i hold scc_knn_scratch_entries(N, k, rows_forced) entries each.
extern "C" hipError_t scc_launch_knn_scores(const double* P, int N, int dims, int k, int rows_forced, double* part_d,
                                            int* part_i, int* idx, double* dist, hipStream_t st)
{
    int rows, nch;
    scc_knn_plan(N, k, rows_forced, &rows, &nch);
    for (int row0 = 0; row0 < N; row0 += rows) {
        const int row1 = std::min(N, row0 + rows);
        if (dims <= 8) {
            if (k <= 16)
                knn_launch_partial<8, 256, 16>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
            else if (k <= 32)
                knn_launch_partial<8, 256, 32>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
            else
                knn_launch_partial<8, 128, 64>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
        } else {
            if (k <= 16)
                knn_launch_partial<15, 256, 16>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
            else if (k <= 32)
                knn_launch_partial<15, 256, 32>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
            else
                knn_launch_partial<15, 128, 64>(P, N, dims, k, row0, row1, nch, rows, part_d, part_i, st);
        }
        hipLaunchKernelGGL(k_knn_merge, dim3((row1 - row0 + 255) / 256), dim3(256), 0, st, part_d, part_i, k, row0,
                           row1, nch, rows, idx, dist);
    }
    return hipGetLastError();
}
