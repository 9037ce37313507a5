// scc_umap.hip — UMAP of the cells on the device: the fuzzy simplicial set of a
// k-NN table and the stochastic-gradient layout of a symmetric weighted graph
// (include/scc.h: scc_umap_graph, scc_umap_layout, scc_umap_scores; host driver:
// scc_umap.cpp; the rules restated in NumPy: tests/umap_reference.py).
//
// Everything is f64 and no floating-point atomic is used: every sum has one
// fixed shape, so two calls return the same bits.  The integer atomics (row
// counts, fill cursors, the maxima taken on the bit patterns of non-negative
// doubles) decide no output bit: the fill order is undone by the row sort, and
// a maximum does not depend on its order.
//
// Graph (umap-learn's smooth_knn_dist, compute_membership_strengths and
// fuzzy_simplicial_set at local_connectivity = 1, bandwidth = 1):
//   k_umap_rowsum   a thread per row: the row's distances summed in order
//   k_umap_total    one workgroup: the row sums in one fixed-shape reduction
//   k_umap_sigma    a lane per row, 64 rows of the table staged in LDS (odd row
//                   stride: conflict-free): rho, the bisection for sigma, its
//                   floor, the k directed weights
//   k_umap_count    a thread per directed entry i -> j: looks for i in row j
//                   (k <= 64 compares) and counts the entry for row i, and for
//                   row j when j does not list i (the transpose's entry)
//   k_umap_scan     one workgroup: exclusive scan of the counts (int64)
//   k_umap_fill     as k_umap_count, writing (column, value) at a cursor
//   k_umap_sort     a thread per filled entry: its rank among its row's columns
//                   (they are distinct) is its place; rows of any length
//
// Layout (one plain launch per epoch, positions double-buffered):
//   k_umap_epoch    head-centred: UMAP_LANES lanes own a vertex and split its
//                   row by slot (lane l takes slots l, l + 16, ...: a coalesced
//                   read of the schedule state), each lane adds its moves in
//                   slot order (attraction, then the slot's negative samples
//                   s = 0, 1, ...), and the 16 partial sums meet in one xor
//                   butterfly.  Every position read comes from the old buffer;
//                   the vertex's group is the only writer of its new position
//                   and of its row's schedule state.  A long (hub) row is the
//                   same loop with more rounds.
#include "scc_common.hpp"

#include <algorithm>
#include <climits>

#define UMAP_LANES 16     // lanes that share a vertex in k_umap_epoch
#define UMAP_ROWS 64       // table rows per k_umap_sigma workgroup
#define UMAP_BISECT 64     // bisection steps at most
#define UMAP_SCAN_T 1024   // threads of the scan and total workgroups

__global__ void __launch_bounds__(256) k_umap_rowsum(const double* __restrict__ dist, int n, int k,
                                                     double* __restrict__ rowsum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < k; ++j) s += dist[(size_t)i * k + j];
    rowsum[i] = s;
}

// total[0] = the sum of x[0..n) in one shape: thread t adds x[t], x[t + T], ... in order, then a halving tree
__global__ void __launch_bounds__(UMAP_SCAN_T) k_umap_total(const double* __restrict__ x, int n,
                                                            double* __restrict__ total)
{
    __shared__ double sh[UMAP_SCAN_T];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += UMAP_SCAN_T) s += x[i];
    sh[t] = s;
    __syncthreads();
    for (int m = UMAP_SCAN_T / 2; m >= 1; m >>= 1) {
        if (t < m) sh[t] += sh[t + m];
        __syncthreads();
    }
    if (t == 0) total[0] = sh[0];
}

// rho, sigma and the directed weights of rows [64 b, 64 b + 64); dynamic LDS: 64 (k | 1) doubles
__global__ void __launch_bounds__(UMAP_ROWS) k_umap_sigma(const double* __restrict__ dist, int n, int k, double target,
                                                          const double* __restrict__ rowsum,
                                                          const double* __restrict__ total, double* __restrict__ rho,
                                                          double* __restrict__ sigma, double* __restrict__ w)
{
    extern __shared__ double um_rows[];
    const int ld = k | 1, tid = threadIdx.x;
    const int r0 = blockIdx.x * UMAP_ROWS, nr = min(UMAP_ROWS, n - r0);
    for (int e = tid; e < nr * k; e += UMAP_ROWS) um_rows[(e / k) * ld + e % k] = dist[(size_t)r0 * k + e];
    __syncthreads();
    if (tid >= nr) return;
    const int i = r0 + tid;
    const double* d = um_rows + tid * ld;
    double rh = 0.0;  // the smallest strictly positive distance
    for (int j = 0; j < k; ++j)
        if (d[j] > 0.0 && (rh == 0.0 || d[j] < rh)) rh = d[j];
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < UMAP_BISECT; ++it) {
        double psum = 0.0;
        for (int j = 0; j < k; ++j) {
            const double x = d[j] - rh;
            psum += x > 0.0 ? exp(-x / mid) : 1.0;
        }
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            if (hi == INFINITY)
                mid *= 2.0;
            else
                mid = (lo + hi) / 2.0;
        }
    }
    const double mean = rh > 0.0 ? rowsum[i] / (double)k : total[0] / ((double)n * (double)k);
    const double sg = fmax(mid, 1e-3 * mean);
    rho[i] = rh;
    sigma[i] = sg;
    for (int j = 0; j < k; ++j) {
        const double x = d[j] - rh;
        w[(size_t)i * k + j] = (x <= 0.0 || sg == 0.0) ? 1.0 : exp(-x / sg);
    }
}

// where row j lists i: its slot, or -1
__device__ inline int umap_find(const int* __restrict__ idx, int k, int j, int i)
{
    int at = -1;
    for (int q = 0; q < k; ++q)
        if (idx[(size_t)j * k + q] == i) at = q;
    return at;
}

// inter: the intersection (set_op_mix_ratio == 0) instead of the union
__global__ void __launch_bounds__(256) k_umap_count(const int* __restrict__ idx, int n, int k, int inter,
                                                    int* __restrict__ cnt)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const int i = (int)(t / k), j = idx[t];
    if (j == i) return;
    const bool back = umap_find(idx, k, j, i) >= 0;
    if (inter) {
        if (back) atomicAdd(&cnt[i], 1);
    } else {
        atomicAdd(&cnt[i], 1);
        if (!back) atomicAdd(&cnt[j], 1);
    }
}

// indptr[0..n] = exclusive scan of cnt[0..n), by one workgroup chunk after chunk
__global__ void __launch_bounds__(UMAP_SCAN_T) k_umap_scan(const int* __restrict__ cnt, int n, i64* __restrict__ indptr)
{
    __shared__ i64 sh[UMAP_SCAN_T];
    const int t = threadIdx.x;
    i64 carry = 0;
    for (int c0 = 0; c0 < n; c0 += UMAP_SCAN_T) {
        const i64 v = c0 + t < n ? (i64)cnt[c0 + t] : 0;
        sh[t] = v;
        __syncthreads();
        for (int m = 1; m < UMAP_SCAN_T; m <<= 1) {  // Hillis-Steele, inclusive
            const i64 a = t >= m ? sh[t - m] : 0;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (c0 + t < n) indptr[c0 + t] = carry + sh[t] - v;
        carry += sh[UMAP_SCAN_T - 1];
        __syncthreads();
    }
    if (t == 0) indptr[n] = carry;
}

__global__ void __launch_bounds__(256) k_umap_fill(const int* __restrict__ idx, const double* __restrict__ w, int n,
                                                   int k, int inter, double mix, const i64* __restrict__ indptr,
                                                   int* __restrict__ cur, int* __restrict__ cols_u,
                                                   double* __restrict__ vals_u, int* __restrict__ rowid)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const int i = (int)(t / k), j = idx[t];
    if (j == i) return;
    const int at = umap_find(idx, k, j, i);
    if (inter && at < 0) return;
    const double a = w[t], b = at >= 0 ? w[(size_t)j * k + at] : 0.0;
    const double prod = a * b;  // (a + b and a * b commute: entry (j, i) gets the same bits)
    const double val = mix * ((a + b) - prod) + (1.0 - mix) * prod;
    i64 pos = indptr[i] + atomicAdd(&cur[i], 1);  // < indptr[i + 1]: k_umap_count counted this entry
    cols_u[pos] = j;
    vals_u[pos] = val;
    rowid[pos] = i;
    if (at < 0) {
        pos = indptr[j] + atomicAdd(&cur[j], 1);
        cols_u[pos] = i;
        vals_u[pos] = val;
        rowid[pos] = j;
    }
}

__global__ void __launch_bounds__(256) k_umap_sort(const i64* __restrict__ indptr, const int* __restrict__ rowid,
                                                   const int* __restrict__ cols_u, const double* __restrict__ vals_u,
                                                   i64 nnz, int* __restrict__ cols, double* __restrict__ vals)
{
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const int r = rowid[p], c = cols_u[p];
    const i64 p0 = indptr[r], p1 = indptr[r + 1];
    i64 rank = 0;
    for (i64 q = p0; q < p1; ++q) rank += cols_u[q] < c;
    cols[p0 + rank] = c;  // the columns of a row are distinct: rank < p1 - p0, one entry per place
    vals[p0 + rank] = vals_u[p];
}

// ------------------------------------------------------------------ layout

// out = max(out, max |x[i * stride + off]|) over i < n, on the bit patterns (non-negative doubles order as integers)
__global__ void __launch_bounds__(256) k_umap_absmax(const double* __restrict__ x, i64 n, int stride, int off0,
                                                     int off1, u64* __restrict__ out)
{
    __shared__ u64 sh[256];
    u64 m = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        m = max(m, (u64)__double_as_longlong(fabs(x[i * stride + off0])));
        m = max(m, (u64)__double_as_longlong(fabs(x[i * stride + off1])));
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax((unsigned long long*)out, (unsigned long long)sh[0]);
}

// the default initialisation: the first two score columns, the largest absolute coordinate scaled to 10
__global__ void __launch_bounds__(256) k_umap_init_scores(const double* __restrict__ P, int n,
                                                          const u64* __restrict__ amax, double* __restrict__ Y)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double mx = __longlong_as_double((long long)amax[0]);
    const double sc = mx > 0.0 ? 10.0 / mx : 0.0;
    Y[2 * (size_t)i] = P[(size_t)i * 16] * sc;
    Y[2 * (size_t)i + 1] = P[(size_t)i * 16 + 1] * sc;
}

// an edge acts when its weight is positive and not below w_max / n_epochs; its period is w_max / w
__global__ void __launch_bounds__(256) k_umap_sched(const double* __restrict__ vals, i64 nnz, const u64* __restrict__ wmax,
                                                    int n_epochs, double nsr, double* __restrict__ next,
                                                    double* __restrict__ nneg)
{
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const double wm = __longlong_as_double((long long)wmax[0]), w = vals[p];
    const bool act = w > 0.0 && !(w < wm / (double)n_epochs);
    const double per = wm / w;
    next[p] = act ? per : INFINITY;
    nneg[p] = act ? per / nsr : INFINITY;
}

__device__ inline double umap_clip(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

// the vertex draw s of slot p in epoch e picks: a pure function of (seed, e, p, s)
__device__ inline int umap_draw(u64 seed, u64 ctr, int n)
{
    u64 z = seed + 0x9E3779B97F4A7C15ull * ctr;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int)(((z >> 32) * (u64)n) >> 32);  // < n
}

__global__ void __launch_bounds__(256) k_umap_epoch(const i64* __restrict__ indptr, const int* __restrict__ cols,
                                                    const double* __restrict__ vals, double* __restrict__ next,
                                                    double* __restrict__ nneg, const double2* __restrict__ Yold,
                                                    double2* __restrict__ Ynew, int n, i64 nnz, int e, double alpha,
                                                    double a, double b, double gamma, double nsr,
                                                    const u64* __restrict__ wmax, u64 seed)
{
    const i64 gt = (i64)blockIdx.x * 256 + threadIdx.x;
    const int l = (int)(gt & (UMAP_LANES - 1));
    const i64 g = gt / UMAP_LANES;
    const bool live = g < n;  // a group past n adds nothing and stays for the butterfly
    const double wm = __longlong_as_double((long long)wmax[0]);
    const double ed = (double)e;
    double sx = 0.0, sy = 0.0;
    double2 yi = {0.0, 0.0};
    if (live) {
        yi = Yold[g];
        const i64 p1 = indptr[g + 1];
        for (i64 p = indptr[g] + l; p < p1; p += UMAP_LANES) {
            const double nx = next[p];
            if (!(nx <= ed)) continue;
            const double per = wm / vals[p], epn = per / nsr;
            {
                const double2 yj = Yold[cols[p]];
                const double dx = yi.x - yj.x, dy = yi.y - yj.y;
                const double d2 = dx * dx + dy * dy;
                const double c = d2 > 0.0 ? (-2.0 * a * b * pow(d2, b - 1.0)) / (a * pow(d2, b) + 1.0) : 0.0;
                sx += umap_clip(c * dx);
                sy += umap_clip(c * dy);
            }
            const double nn = nneg[p];
            double mf = nsr > 0.0 ? floor((ed - nn) / epn) : 0.0;
            mf = mf > 0.0 ? fmin(mf, 65535.0) : 0.0;  // (a draw index has 16 bits of the counter)
            const int m = (int)mf;
            const u64 base = ((u64)e * (u64)nnz + (u64)p) << 16;
            for (int s = 0; s < m; ++s) {
                const int v = umap_draw(seed, base + (u64)s, n);
                if (v == (int)g) continue;
                const double2 yv = Yold[v];
                const double dx = yi.x - yv.x, dy = yi.y - yv.y;
                const double d2 = dx * dx + dy * dy;
                if (d2 > 0.0) {
                    const double c = (2.0 * gamma * b) / ((0.001 + d2) * (a * pow(d2, b) + 1.0));
                    sx += umap_clip(c * dx);
                    sy += umap_clip(c * dy);
                } else {
                    sx += 4.0;
                    sy += 4.0;
                }
            }
            nneg[p] = nn + mf * epn;
            next[p] = nx + per;
        }
    }
#pragma unroll
    for (int m = UMAP_LANES / 2; m >= 1; m >>= 1) {  // a + b on both lanes of a pair: every lane ends with the same bits
        sx += __shfl_xor(sx, m, UMAP_LANES);
        sy += __shfl_xor(sy, m, UMAP_LANES);
    }
    if (live && l == 0) Ynew[g] = double2{yi.x + alpha * sx, yi.y + alpha * sy};
}

// ------------------------------------------------------------------ launchers

extern "C" hipError_t scc_launch_umap_graph_weights(const double* dist, int n, int k, double target, double* rowsum,
                                                    double* total, double* rho, double* sigma, double* w,
                                                    hipStream_t st)
{
    hipLaunchKernelGGL(k_umap_rowsum, dim3((n + 255) / 256), dim3(256), 0, st, dist, n, k, rowsum);
    hipLaunchKernelGGL(k_umap_total, dim3(1), dim3(UMAP_SCAN_T), 0, st, rowsum, n, total);
    const size_t lds = sizeof(double) * UMAP_ROWS * (size_t)(k | 1);  // k <= 64: at most 33,280 bytes
    hipLaunchKernelGGL(k_umap_sigma, dim3((n + UMAP_ROWS - 1) / UMAP_ROWS), dim3(UMAP_ROWS), lds, st, dist, n, k, target,
                       rowsum, total, rho, sigma, w);
    return hipGetLastError();
}

// cnt [n] is zeroed here; indptr [n + 1] holds the row starts afterwards
extern "C" hipError_t scc_launch_umap_graph_count(const int* idx, int n, int k, int inter, int* cnt, i64* indptr,
                                                  hipStream_t st)
{
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    const size_t nk = (size_t)n * k;
    hipLaunchKernelGGL(k_umap_count, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, idx, n, k, inter, cnt);
    hipLaunchKernelGGL(k_umap_scan, dim3(1), dim3(UMAP_SCAN_T), 0, st, cnt, n, indptr);
    return hipGetLastError();
}

// cols_u, vals_u, rowid, cols, vals: nnz entries each (nnz = indptr[n] > 0)
extern "C" hipError_t scc_launch_umap_graph_fill(const int* idx, const double* w, int n, int k, int inter, double mix,
                                                 const i64* indptr, i64 nnz, int* cur, int* cols_u, double* vals_u,
                                                 int* rowid, int* cols, double* vals, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(cur, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    const size_t nk = (size_t)n * k;
    hipLaunchKernelGGL(k_umap_fill, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, idx, w, n, k, inter, mix,
                       indptr, cur, cols_u, vals_u, rowid);
    hipLaunchKernelGGL(k_umap_sort, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, indptr, rowid, cols_u, vals_u,
                       nnz, cols, vals);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_umap_init_scores(const double* P, int n, u64* amax, double* Y, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(amax, 0, sizeof(u64), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_umap_absmax, dim3(std::min(1024, (n + 255) / 256)), dim3(256), 0, st, P, (i64)n, 16, 0, 1, amax);
    hipLaunchKernelGGL(k_umap_init_scores, dim3((n + 255) / 256), dim3(256), 0, st, P, n, amax, Y);
    return hipGetLastError();
}

// Ya holds the initialisation; the result is in Ya after an even number of epochs, in Yb after an odd one
extern "C" hipError_t scc_launch_umap_layout(const i64* indptr, const int* cols, const double* vals, int n, i64 nnz,
                                             int n_epochs, double a, double b, double gamma, double nsr, double lr,
                                             u64 seed, u64* wmax, double* next, double* nneg, double* Ya, double* Yb,
                                             hipStream_t st)
{
    hipError_t e = hipMemsetAsync(wmax, 0, sizeof(u64), st);
    if (e != hipSuccess) return e;
    if (nnz > 0) {
        const unsigned gb = (unsigned)std::min<i64>(1024, (nnz + 255) / 256);
        hipLaunchKernelGGL(k_umap_absmax, dim3(gb), dim3(256), 0, st, vals, nnz, 1, 0, 0, wmax);
        hipLaunchKernelGGL(k_umap_sched, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, vals, nnz, wmax, n_epochs,
                           nsr, next, nneg);
    }
    const unsigned grid = (unsigned)(((i64)n * UMAP_LANES + 255) / 256);
    for (int ep = 1; ep <= n_epochs; ++ep) {
        const double alpha = lr * (1.0 - (double)(ep - 1) / (double)n_epochs);
        hipLaunchKernelGGL(k_umap_epoch, dim3(grid), dim3(256), 0, st, indptr, cols, vals, next, nneg,
                           (const double2*)Ya, (double2*)Yb, n, nnz, ep, alpha, a, b, gamma, nsr, wmax, seed);
        std::swap(Ya, Yb);
    }
    return hipGetLastError();
}
