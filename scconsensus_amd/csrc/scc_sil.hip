// scc_sil.hip — silhouette widths on the HBM-resident distance vector, or
// from the PCA scores whose dist() it would be.
//
// Reference: cluster::silhouette(dynamicGroups, dmatrix = as.matrix(d)) and
// mean(summary(.)$clus.avg.widths) per deepSplit value
// (R/reclusterDEConsensusFast.R:433), SURVEY §8(f)-2.  R materialises the
// N x N matrix (as.matrix) and sums per cluster on the host; here the packed
// R `dist` vector stays in HBM and is read once per (row, column) pair.
//
// k_sil_sums   S[i][c] = sum_{j in cluster c} d(i, j) as the product of the
//              full symmetric matrix (read from the packed lower triangle,
//              mirrored) and the one-hot cluster matrix, on fp64 MFMA
//              16x16x4: a wave owns 16 rows x one of SIL_JCH column chunks,
//              up to 4 cluster tiles of 16 in its accumulators.  Partial sums
//              per chunk go to a scratch and are added in chunk order
//              (deterministic).  The entry source is a template parameter:
//              the packed f64 or f32 vector, or the [N][16] PCA scores, from
//              which each entry is computed with the dist kernel's arithmetic
//              (scc_silhouette_scores: no N x N object; the widths are bit for
//              bit those read from the packed f64 vector of the same scores).
// k_sil_widths cluster's sildist rule: a = S[own] / (n_own - 1),
//              b = min_{c != own} S[c] / n_c, s = 1 - a/b (a < b), b/a - 1
//              (a > b), 0 (a == b or a singleton cluster).
#include "scc_common.hpp"
#include "scc_dist_entry.hpp"

typedef double d4 __attribute__((ext_vector_type(4)));

#define SIL_JCH 8    // column chunks per 16-row block (waves in flight)
#define SIL_CT 4     // cluster tiles of 16 per pass (64 clusters)

template <class T>
__device__ inline double sil_d(const T* __restrict__ D, long long N, long long i, long long j)
{
    if (i == j || i >= N || j >= N) return 0.0;
    const long long c = i < j ? i : j, r = i < j ? j : i;  // column c < row r in the packed lower triangle
    return (double)D[c * (2 * N - c - 1) / 2 + (r - c - 1)];
}

// Where an entry d(i, j) comes from.  Packed: a load from the lower triangle
// (T = double or float).  Scores: computed from rows i and j of the [N][16]
// scores with the dist kernel's arithmetic (scc_dist_entry.hpp), so the value
// is the one the packed f64 vector would hold and nothing N x N exists.
template <class T>
struct SilPacked {
    typedef T elem;
    static constexpr bool scores = false;
};
struct SilScores {
    typedef double elem;
    static constexpr bool scores = true;
};

#define SIL_TILE 256                 // columns staged per LDS tile (scores source)
#define SIL_LD 18                    // doubles per staged row: 15 scores, |p|^2, 2 of padding
typedef double dv2 __attribute__((ext_vector_type(2)));

// grid: (row blocks of 64 = 4 waves x 16 rows, SIL_JCH, cluster passes)
//
// The summation (column chunks, the 16-column steps, the 4 k-steps, the
// one-hot MFMA, the partial per chunk) is the same for every source; only the
// origin of the A operand dv[u] differs.  With the scores source the four
// waves of a workgroup share the column chunk, so its score rows go through
// LDS a tile of SIL_TILE columns at a time, each with its squared norm in the
// unused 16th slot; a lane keeps its own row's 15 scores and norm in
// registers.  A row of SIL_LD doubles puts the 4 rows of one wave read (16
// lanes per address) on distinct banks.  More than 64 clusters are further
// passes (blockIdx.z) that compute the entries again.
template <class Src>
__global__ void __launch_bounds__(256) k_sil_sums(const typename Src::elem* __restrict__ D, int N,
                                                  const int* __restrict__ lab, int C, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, w = scc_wave_id();
    const int I0 = (blockIdx.x * 4 + w) * 16;
    if (!Src::scores && I0 >= N) return;  // (the scores source keeps every wave for the tile barriers)
    const int ch = blockIdx.y, c0 = blockIdx.z * 16 * SIL_CT;
    const int per = ((N + SIL_JCH - 1) / SIL_JCH + 3) & ~3;
    const int J0 = ch * per, J1 = min(N, J0 + per);
    const int i = I0 + (lane & 15), kq = lane >> 4, cl = lane & 15;
    d4 acc[SIL_CT];
#pragma unroll
    for (int t = 0; t < SIL_CT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    if constexpr (Src::scores) {
        static_assert(SIL_TILE == 256 && SIL_TILE % 16 == 0, "one staged column per thread, whole 16-column steps");
        __shared__ __attribute__((aligned(16))) double tile[SIL_TILE * SIL_LD];
        double pi[15];
        const int ic = min(i, N - 1);
#pragma unroll
        for (int q = 0; q < 15; ++q) pi[q] = D[(size_t)ic * 16 + q];
        const double ni = scc_dist_norm15(pi);
        for (int T0 = J0; T0 < J1; T0 += SIL_TILE) {
            __syncthreads();  // the previous tile is read
            {
                const int jc = T0 + (int)threadIdx.x;  // SIL_TILE == the workgroup's threads: one column each
                double pj[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) pj[q] = jc < J1 ? D[(size_t)jc * 16 + q] : 0.0;
                pj[15] = scc_dist_norm15(pj);
#pragma unroll
                for (int q = 0; q < 16; q += 2) *(dv2*)&tile[threadIdx.x * SIL_LD + q] = dv2{pj[q], pj[q + 1]};
            }
            __syncthreads();
            if (I0 >= N) continue;  // wave-uniform
            const int T1 = min(J1, T0 + SIL_TILE);
            for (int j0 = T0; j0 < T1; j0 += 16) {
                double dv[4];
                int lj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + 4 * u + kq;  // j - T0 < SIL_TILE: T0 and SIL_TILE are multiples of 16
                    const bool ok = j < J1;
                    double pj[16];
#pragma unroll
                    for (int q = 0; q < 16; q += 2) {
                        const dv2 v = *(const dv2*)&tile[(j - T0) * SIL_LD + q];
                        pj[q] = v.x;
                        pj[q + 1] = v.y;
                    }
                    const double e = scc_dist_entry15(pi, ni, pj, pj[15]);
                    dv[u] = (ok && i != j && i < N) ? e : 0.0;  // as sil_d: 0 on the diagonal and past the end
                    lj[u] = ok ? lab[j] : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int t = 0; t < SIL_CT; ++t) {
                        const double b = (lj[u] == c0 + 16 * t + cl) ? 1.0 : 0.0;
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[u], b, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        if (I0 >= N) return;
    } else {  // (kept as it was, not folded into the loop above: the packed kernels compile as before)
        for (int j0 = J0; j0 < J1; j0 += 16) {
            double dv[4];
            int lj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // 4 k-steps: loads first
                const int j = j0 + 4 * u + kq;
                const bool ok = j < J1;
                dv[u] = ok ? sil_d(D, N, i, j) : 0.0;
                lj[u] = ok ? lab[j] : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int t = 0; t < SIL_CT; ++t) {
                    const double b = (lj[u] == c0 + 16 * t + cl) ? 1.0 : 0.0;
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(dv[u], b, acc[t], 0, 0, 0);
                }
            }
        }
    }
    // accumulator register r of tile t: S[row = I0 + kq + 4 r][cluster c0 + 16 t + cl]
#pragma unroll
    for (int t = 0; t < SIL_CT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I0 + kq + 4 * r, c = c0 + 16 * t + cl;
            if (row < N && c < C) part[((size_t)ch * N + row) * C + c] = acc[t][r];
        }
}

// how many of the N x 16 scores are not finite (the counter starts at zero)
__global__ void k_sil_clear(unsigned int* nonfinite) { *nonfinite = 0; }
__global__ void __launch_bounds__(256) k_sil_nonfinite(const double* __restrict__ P, size_t n,
                                                       unsigned int* nonfinite)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && !isfinite(P[e])) atomicAdd(nonfinite, 1u);
}

__global__ void __launch_bounds__(256) k_sil_widths(const double* __restrict__ part, int N, int C,
                                                    const int* __restrict__ lab, const int* __restrict__ cnt,
                                                    double* __restrict__ width)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int own = lab[i];
    double a = 0.0, b = INFINITY;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int ch = 0; ch < SIL_JCH; ++ch) s += part[((size_t)ch * N + i) * C + c];  // chunk order
        if (c == own)
            a = s;
        else if (cnt[c] > 0)
            b = fmin(b, s / cnt[c]);
    }
    double w = 0.0;
    if (cnt[own] > 1) {
        a /= (cnt[own] - 1);
        w = (a < b) ? 1.0 - a / b : ((a > b) ? b / a - 1.0 : 0.0);
    }
    width[i] = w;
}

extern "C" size_t scc_sil_scratch_doubles(int N, int C) { return (size_t)SIL_JCH * N * C; }

extern "C" hipError_t scc_launch_silhouette(const void* D, int f32, int N, const int* lab, const int* cnt, int C,
                                            double* part, double* width, hipStream_t st)
{
    const dim3 grid((N + 63) / 64, SIL_JCH, (C + 16 * SIL_CT - 1) / (16 * SIL_CT));
    if (f32)
        hipLaunchKernelGGL(k_sil_sums<SilPacked<float>>, grid, dim3(256), 0, st, (const float*)D, N, lab, C, part);
    else
        hipLaunchKernelGGL(k_sil_sums<SilPacked<double>>, grid, dim3(256), 0, st, (const double*)D, N, lab, C, part);
    hipLaunchKernelGGL(k_sil_widths, dim3((N + 255) / 256), dim3(256), 0, st, part, N, C, lab, cnt, width);
    return hipGetLastError();
}

// *nonfinite = how many of the [N][16] scores P are not finite (also scc_knn_scores' check)
extern "C" hipError_t scc_launch_scores_nonfinite(const double* P, int N, unsigned int* nonfinite, hipStream_t st)
{
    const size_t n = (size_t)N * 16;
    hipLaunchKernelGGL(k_sil_clear, dim3(1), dim3(1), 0, st, nonfinite);
    hipLaunchKernelGGL(k_sil_nonfinite, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, n, nonfinite);
    return hipGetLastError();
}

// the widths of dist(P) for the [N][16] scores P; *nonfinite counts the scores
// that are not finite (the caller refuses the widths then)
extern "C" hipError_t scc_launch_silhouette_scores(const double* P, int N, const int* lab, const int* cnt, int C,
                                                   double* part, double* width, unsigned int* nonfinite,
                                                   hipStream_t st)
{
    scc_launch_scores_nonfinite(P, N, nonfinite, st);
    const dim3 grid((N + 63) / 64, SIL_JCH, (C + 16 * SIL_CT - 1) / (16 * SIL_CT));
    hipLaunchKernelGGL(k_sil_sums<SilScores>, grid, dim3(256), 0, st, P, N, lab, C, part);
    hipLaunchKernelGGL(k_sil_widths, dim3((N + 255) / 256), dim3(256), 0, st, part, N, C, lab, cnt, width);
    return hipGetLastError();
}
