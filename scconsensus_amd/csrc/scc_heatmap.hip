// scc_heatmap.hip — the heatmap's inputs on the device (include/scc.h:
// scc_gene_distance, scc_heatmap_raster).
//
// Reference: cellTypeDEPlot(dataMatrix[deGeneUnion, ], ...) (Fast:456-464,
// slow:288-296) ends in ComplexHeatmap::Heatmap(cluster_rows = TRUE,
// use_raster = TRUE) (cellTypeDEPlot.R:225-253): dist() of the |U| gene rows
// over all N cells, hclust "complete", a reorder by -rowMeans, a raster of
// every cell, and a colour ramp from the extrema of x and |x| (:174-222).
//
// All kernels read the gathered panel Xc [Npad][ld] of scc_launch_gather (one
// row per cell, the union's genes contiguous, ld a multiple of 64, zero in the
// padding columns [nu, ld) and the padding rows [N, Npad)).
//
// Kernels
//   k_gene_dist         sum_c (x_ac - x_bc)^2 for a 64 x 64 tile of gene pairs
//                       over one slab of cells, from LDS-staged rows
//   k_gene_dist_finish  the slabs added in slab order, sqrt, R's packed order
//   k_hm_range(_fold)   min x, max x, min |x|, max |x| and the non-finite count
//   k_heatmap_raster    one workgroup per output bin: the bin's cells in
//                       cell_order order, lanes over genes, one division
#include "scc_common.hpp"
#include <algorithm>

// ------------------------------------------------------------------ gene x gene distance
// The direct difference, not g_aa + g_bb - 2 g_ab: every term is >= 0, so the
// sum has no cancellation (relative error <= (N + 2) 2^-53 before the sqrt,
// whatever the order) and two identical rows give exactly 0.  That rules the
// matrix cores out (they multiply, they do not subtract first): per term one
// v_add_f64 and one v_fma_f64 on the vector pipe, which issues a wave64 FP64
// instruction in 4 cycles per SIMD.
//
// Workgroup = 256 threads = a 64 x 64 tile of pairs, 4 x 4 per thread, over
// GD_KC cells per LDS stage.  Per cell a wave issues 32 FP64 instructions (128
// cycles) and reads 8 doubles per lane from LDS:
//   - the `a` genes tx + 16 i as four ds_read_b64: the 16 lanes of a tx row
//     read 16 consecutive doubles (banks 2 tx .. 2 tx + 1 of 64: conflict-free,
//     lanes with the same tx broadcast), 2 LDS cycles each;
//   - the `b` genes 4 ty + j as two ds_read_b128 of four distinct addresses
//     per wave (broadcast), 4 LDS cycles each.
// 16 LDS cycles per wave and cell against 128 on the vector pipe: with the
// four SIMDs issuing side by side the LDS port is busy half the time, so the
// layout needs no padding or swizzle, and a wider register tile would only
// cost occupancy.  The next stage's rows are in flight in registers while the
// current one is computed (two LDS buffers, one barrier per stage).
//
// The tile leaves as T[b][a] (a over the lanes: whole 128-byte runs), one tile
// per (slab, lower-triangle tile); k_gene_dist_finish reads them with a over
// the lanes as well.
#define GD_T 64   // genes per tile side
#define GD_KC 16  // cells per LDS stage (Npad is a multiple of 16)

__global__ void __launch_bounds__(256) k_gene_dist(const double* __restrict__ Xc, int Npad, int ld, int ntl,
                                                   int rows_per_slab, double* __restrict__ slabs)
{
    __shared__ __attribute__((aligned(16))) double sA[2][GD_KC][GD_T];
    __shared__ __attribute__((aligned(16))) double sB[2][GD_KC][GD_T];
    const int tile = (int)(blockIdx.x % (unsigned)ntl), slab = (int)(blockIdx.x / (unsigned)ntl);
    int ta = 0, tb = tile;  // lower triangle, row-major: tile = ta (ta + 1) / 2 + tb, tb <= ta
    while (tb > ta) {
        ++ta;
        tb -= ta;
    }
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c0 = slab * rows_per_slab, c1 = min(Npad, c0 + rows_per_slab);
    const int nst = c1 > c0 ? (c1 - c0) / GD_KC : 0;
    // staging: thread -> rows lr and lr + 8 of the stage, doubles 2 lc, 2 lc + 1 of each operand
    const int lr = tid >> 5, lc = tid & 31;
    const double* gA = Xc + (size_t)c0 * ld + (size_t)ta * GD_T + 2 * lc;
    const double* gB = Xc + (size_t)c0 * ld + (size_t)tb * GD_T + 2 * lc;
    double acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.0;
    double2 pa[2], pb[2];
    auto gload = [&](int s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const size_t off = (size_t)(s * GD_KC + lr + 8 * h) * ld;
            pa[h] = *(const double2*)(gA + off);
            pb[h] = *(const double2*)(gB + off);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(double2*)&sA[buf][lr + 8 * h][2 * lc] = pa[h];
            *(double2*)&sB[buf][lr + 8 * h][2 * lc] = pb[h];
        }
    };
    if (nst > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        if (s + 1 < nst) gload(s + 1);
#pragma unroll 4
        for (int k = 0; k < GD_KC; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = sA[buf][k][tx + 16 * i];
            const double2 b01 = *(const double2*)&sB[buf][k][4 * ty], b23 = *(const double2*)&sB[buf][k][4 * ty + 2];
            b[0] = b01.x, b[1] = b01.y, b[2] = b23.x, b[3] = b23.y;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double d = a[i] - b[j];
                    acc[j][i] = fma(d, d, acc[j][i]);
                }
        }
        if (s + 1 < nst) lstore(buf ^ 1);
        __syncthreads();
    }
    double* T = slabs + ((size_t)slab * ntl + tile) * (GD_T * GD_T);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) T[(4 * ty + j) * GD_T + tx + 16 * i] = acc[j][i];
}

// One thread per (a, b), b = blockIdx.y the smaller gene (R's column), a over
// the lanes: the slabs' partial sums in slab order (a fixed order: two runs
// give the same bits), the sqrt, and the packed entry b n - b (b + 1) / 2 +
// a - b - 1.  Gene a is the tile's `a` side (ta >= tb since a > b).
__global__ void __launch_bounds__(256) k_gene_dist_finish(const double* __restrict__ slabs, int nslab, int ntl, int nu,
                                                          double* __restrict__ out)
{
    const int a = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (a >= nu || a <= b) return;
    const int ta = a / GD_T, tb = b / GD_T;
    const size_t tile = (size_t)ta * (ta + 1) / 2 + tb;
    const size_t e = (size_t)(b % GD_T) * GD_T + (a % GD_T);
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += slabs[((size_t)k * ntl + tile) * (GD_T * GD_T) + e];
    out[(size_t)b * nu - (size_t)b * (b + 1) / 2 + (a - b - 1)] = sqrt(s);
}

extern "C" int scc_gene_dist_slabs(int Npad, int ld)
{
    // cells split over workgroups until the grid holds ~4 workgroups per CU;
    // a slab is at least 512 cells (32 LDS stages) and there are at most 64
    const int nt = ld / GD_T, ntl = nt * (nt + 1) / 2;
    const int want = (4 * scc_device_cus(256) + ntl - 1) / ntl;
    return std::max(1, std::min(std::min(want, 64), (Npad + 511) / 512));
}

extern "C" size_t scc_gene_dist_slab_doubles(int Npad, int ld)
{
    const int nt = ld / GD_T, ntl = nt * (nt + 1) / 2;
    return (size_t)scc_gene_dist_slabs(Npad, ld) * ntl * (GD_T * GD_T);
}

extern "C" hipError_t scc_launch_gene_dist(const double* Xc, int Npad, int nu, int ld, double* slabs, double* out,
                                           hipStream_t st)
{
    if (ld % GD_T || Npad % GD_KC || nu < 2 || nu > ld) return hipErrorInvalidValue;
    const int nt = ld / GD_T, ntl = nt * (nt + 1) / 2;
    const int nslab = scc_gene_dist_slabs(Npad, ld);
    const int rps = (((Npad + nslab - 1) / nslab) + GD_KC - 1) / GD_KC * GD_KC;
    hipLaunchKernelGGL(k_gene_dist, dim3((unsigned)(ntl * nslab)), dim3(256), 0, st, Xc, Npad, ld, ntl, rps, slabs);
    hipLaunchKernelGGL(k_gene_dist_finish, dim3((nu + 255) / 256, nu - 1), dim3(256), 0, st, slabs, nslab, ntl, nu,
                       out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ range
// One wave per cell row, lanes over the union's genes (the padding columns are
// zeros of the panel, not of the data: left out).  Non-finite values are
// counted and kept out of the extrema.  Minima and maxima do not depend on the
// order, so the partials need no fixed shape.
#define HR_WG 1024  // partials (workgroups) of the range pass, at most

__global__ void __launch_bounds__(256) k_hm_range(const double* __restrict__ Xc, int N, int nu, int ld,
                                                  double* __restrict__ part, unsigned int* __restrict__ pbad)
{
    __shared__ double sm[4][4];
    __shared__ unsigned int sb[4];
    const int lane = threadIdx.x & 63, wv = scc_wave_id();
    double mn = INFINITY, mx = -INFINITY, amn = INFINITY, amx = -INFINITY;
    unsigned int bad = 0;
    for (int c = blockIdx.x * 4 + wv; c < N; c += gridDim.x * 4) {
        const double* row = Xc + (size_t)c * ld;
        for (int u = lane; u < nu; u += 64) {
            const double x = row[u], ax = fabs(x);
            if (ax < INFINITY) {  // false for NaN and both infinities
                mn = fmin(mn, x);
                mx = fmax(mx, x);
                amn = fmin(amn, ax);
                amx = fmax(amx, ax);
            } else
                ++bad;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, m));
        mx = fmax(mx, __shfl_xor(mx, m));
        amn = fmin(amn, __shfl_xor(amn, m));
        amx = fmax(amx, __shfl_xor(amx, m));
        bad += __shfl_xor(bad, m);
    }
    if (lane == 0) {
        sm[wv][0] = mn, sm[wv][1] = mx, sm[wv][2] = amn, sm[wv][3] = amx;
        sb[wv] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = fmin(mn, sm[w][0]);
            mx = fmax(mx, sm[w][1]);
            amn = fmin(amn, sm[w][2]);
            amx = fmax(amx, sm[w][3]);
            bad += sb[w];
        }
        part[4 * blockIdx.x + 0] = mn, part[4 * blockIdx.x + 1] = mx;
        part[4 * blockIdx.x + 2] = amn, part[4 * blockIdx.x + 3] = amx;
        pbad[blockIdx.x] = bad;
    }
}

// one wave folds the partials: out = {min x, max x, min |x|, max |x|}, *nbad the count (saturating)
__global__ void __launch_bounds__(64) k_hm_range_fold(const double* __restrict__ part, const unsigned int* __restrict__ pbad,
                                                      int nparts, double* __restrict__ out, unsigned int* __restrict__ nbad)
{
    const int lane = threadIdx.x;
    double mn = INFINITY, mx = -INFINITY, amn = INFINITY, amx = -INFINITY;
    unsigned long long bad = 0;
    for (int k = lane; k < nparts; k += 64) {
        mn = fmin(mn, part[4 * k + 0]);
        mx = fmax(mx, part[4 * k + 1]);
        amn = fmin(amn, part[4 * k + 2]);
        amx = fmax(amx, part[4 * k + 3]);
        bad += pbad[k];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, m));
        mx = fmax(mx, __shfl_xor(mx, m));
        amn = fmin(amn, __shfl_xor(amn, m));
        amx = fmax(amx, __shfl_xor(amx, m));
        bad += __shfl_xor(bad, m);
    }
    if (lane == 0) {
        out[0] = mn, out[1] = mx, out[2] = amn, out[3] = amx;
        *nbad = bad > 0xffffffffull ? 0xffffffffu : (unsigned int)bad;
    }
}

extern "C" size_t scc_hm_range_scratch_bytes(void) { return (size_t)HR_WG * (4 * sizeof(double) + sizeof(unsigned int)); }

// scratch: scc_hm_range_scratch_bytes(); out: 4 doubles; nbad: one counter
extern "C" hipError_t scc_launch_hm_range(const double* Xc, int N, int nu, int ld, void* scratch, double* out,
                                          unsigned int* nbad, hipStream_t st)
{
    if (N < 1 || nu < 1) return hipErrorInvalidValue;
    const int grid = std::max(1, std::min(HR_WG, (N + 3) / 4));
    double* part = (double*)scratch;
    unsigned int* pbad = (unsigned int*)(part + 4 * (size_t)HR_WG);
    hipLaunchKernelGGL(k_hm_range, dim3(grid), dim3(256), 0, st, Xc, N, nu, ld, part, pbad);
    hipLaunchKernelGGL(k_hm_range_fold, dim3(1), dim3(64), 0, st, part, pbad, grid, out, nbad);
    return hipGetLastError();
}

// ------------------------------------------------------------------ raster
// Bin b holds the cells cell[floor(b N / width) .. floor((b + 1) N / width))
// (0-based ids in the caller's order).  Lanes over genes: every panel row read
// is one coalesced run; a lane adds its bin's cells one after the other,
// starting from the first (so a one-cell bin is that cell's value, bit for
// bit), and divides once.  R [width][nu]; no atomics.
__global__ void __launch_bounds__(256) k_heatmap_raster(const double* __restrict__ Xc, int N, int nu, int ld,
                                                        const int* __restrict__ cell, int width,
                                                        double* __restrict__ R)
{
    const long long b = blockIdx.x;
    const int lo = (int)(b * N / width), hi = (int)((b + 1) * N / width);  // width <= N: hi > lo
    for (int u = threadIdx.x; u < nu; u += 256) {
        double s = Xc[(size_t)cell[lo] * ld + u];
        for (int c = lo + 1; c < hi; ++c) s += Xc[(size_t)cell[c] * ld + u];
        R[(size_t)b * nu + u] = hi - lo > 1 ? s / (double)(hi - lo) : s;
    }
}

// cell: device [N], every id in [0, N) (checked by the caller)
extern "C" hipError_t scc_launch_heatmap_raster(const double* Xc, int N, int nu, int ld, const int* cell, int width,
                                                double* R, hipStream_t st)
{
    if (width < 1 || width > N || nu < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_heatmap_raster, dim3((unsigned)width), dim3(256), 0, st, Xc, N, nu, ld, cell, width, R);
    return hipGetLastError();
}
