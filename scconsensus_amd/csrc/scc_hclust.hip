// scc_hclust.hip — hclust(ward.D2) and the tree cut's distance reads on the
// HBM-resident distance vector (include/scc.h: scc_hclust_ward_d2_dev,
// scc_cutree_hybrid_dev).
//
// Reference: cellTree = fastcluster::hclust(d, method = "ward.D2")
// (R/reclusterDEConsensusFast.R:406-411, R/reclusterDEConsensus.R:242-247) and
// cutreeDynamic(dendro, distM = as.matrix(d), ...) (Fast:421-427).  The host
// restatement (scc_cluster.cpp: nn_chain_ward, cutree_hybrid) is the yardstick:
// the kernels here return the same merges, heights and distance values bit
// for bit, so the tree and the labels are the host's.
//
// k_hc_expand       packed f64 / f32 triangle -> the full symmetric N x N
//                   matrix of squared distances (the host's FULL layout: both
//                   triangles, zero diagonal; every later row scan is
//                   contiguous), counting non-finite entries in the same pass.
//                   A tile above the diagonal is read once (contiguous in the
//                   packed vector) and written twice, the mirror through LDS.
// k_hc_chain        the NN-chain, ONE workgroup of 1024 threads (the merges
//                   are a serial dependency chain; one workgroup's barriers
//                   give the host's sequential semantics, nothing waits on
//                   another workgroup).  A launch does at most `max_merges`
//                   merges and leaves its state (chain, sizes, active flags,
//                   start, tip, step) in device memory for the next launch.
//                     scan     row i2 over the active i != i2: block-wide min
//                              over (value, index), the lower index on a tie.
//                              The host's ascending strict-< scan from the
//                              carried mn is "the lowest index attaining the
//                              row minimum if that minimum is < mn, else the
//                              carried i1"; its restart scan is "the lowest
//                              index attaining the minimum of row start".
//                     update   ((v+s)*a - v*mn + (v+t)*b) / (s+t+v) in that
//                              operand order (no contraction: -ffp-contract=
//                              off; IEEE division), rows i1 and i2 read and
//                              row i2 written contiguously, column i2 strided.
//                   Every data-dependent loop is capped (one chain extension:
//                   n scans; one call: 3 n scans; chain positions < n): past
//                   a cap the kernel sets the state's error flag and returns,
//                   and every later launch of the call returns at once.
// k_hc_gather_core  the cs x cs block distM[core, core] of the packed vector
//                   (diagonal 0, f32 widened) for the tree cut's core scatter.
#include "scc_common.hpp"
#include "scc_kernels.hpp"

#define HC_THREADS 1024
#define HC_WAVES (HC_THREADS / SCC_WAVE)
#define HC_TILE 32
#define HC_SCAN_U 8  // row entries a thread loads before it compares them
#define HC_UPD_U 4   // entries a thread loads before it updates them

// packed R `dist` index of (i, j), i < j: row-major upper triangle
__device__ inline size_t hc_pidx(size_t n, size_t i, size_t j) { return i * (2 * n - i - 1) / 2 + (j - i - 1); }

// grid (nt, nt), tiles with blockIdx.y > blockIdx.x idle; block (HC_TILE, 8)
template <class T>
__global__ void __launch_bounds__(HC_TILE * 8) k_hc_expand(const T* __restrict__ P, int N, double* __restrict__ D,
                                                           unsigned int* __restrict__ nonfinite)
{
    __shared__ double tile[HC_TILE][HC_TILE + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const size_t n = (size_t)N;
    unsigned int bad = 0;
    for (int r = ty; r < HC_TILE; r += 8) {
        const int i = bi * HC_TILE + r, j = bj * HC_TILE + tx;
        double v = 0.0;
        if (i < N && j < N && i != j) {
            // a diagonal tile holds both triangles: its lower entries read (j, i)
            const double x = (double)(i < j ? P[hc_pidx(n, i, j)] : P[hc_pidx(n, j, i)]);
            if (i < j && !isfinite(x)) bad++;
            v = x * x;
        }
        tile[r][tx] = v;
        if (i < N && j < N) D[(size_t)i * n + j] = v;
    }
    if (bad) atomicAdd(nonfinite, bad);
    if (bi == bj) return;
    __syncthreads();
    for (int r = ty; r < HC_TILE; r += 8) {
        const int j = bj * HC_TILE + r, i = bi * HC_TILE + tx;  // D[j][i] = tile[i - I0][j - J0]
        if (i < N && j < N) D[(size_t)j * n + i] = tile[tx][r];
    }
}

struct HcBest {
    double v;
    int i;
};

// the earlier of two candidates in the host's scan: the smaller value, the
// lower index on a tie (i == INT_MAX: no candidate)
__device__ inline HcBest hc_min(HcBest a, HcBest b)
{
    const bool take = b.v < a.v || (b.v == a.v && b.i < a.i) || (a.i == INT_MAX && b.i != INT_MAX);
    return take ? b : a;
}

// min over the active i != r of row r, the same value in every thread.
// Two barriers; the first also orders the previous update's stores before
// the next phase's loads (one workgroup: its waves share the CU's L1).
__device__ inline HcBest hc_row_min(const double* D, int N, int r, const uint8_t* act, double* s_v, int* s_i)
{
    const double* row = D + (size_t)r * (size_t)N;
    HcBest b{INFINITY, INT_MAX};
    // HC_SCAN_U independent loads per thread in flight (the row entry is read
    // whether or not its node is active: a removed node's entries are stale,
    // never out of bounds)
    for (int i0 = threadIdx.x; i0 < N; i0 += HC_THREADS * HC_SCAN_U) {
        double v[HC_SCAN_U];
        uint8_t a[HC_SCAN_U];
#pragma unroll
        for (int u = 0; u < HC_SCAN_U; ++u) {
            const int i = i0 + u * HC_THREADS;
            v[u] = i < N ? row[i] : 0.0;
            a[u] = i < N ? act[i] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < HC_SCAN_U; ++u) {
            const int i = i0 + u * HC_THREADS;
            if (a[u] && i != r && (b.i == INT_MAX || v[u] < b.v))
                b = HcBest{v[u], i};  // ascending i: strict < keeps the lowest index
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        HcBest o{__shfl_xor(b.v, m, SCC_WAVE), __shfl_xor(b.i, m, SCC_WAVE)};
        b = hc_min(b, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_v[w] = b.v;
        s_i[w] = b.i;
    }
    __syncthreads();
    b = HcBest{s_v[0], s_i[0]};
#pragma unroll
    for (int k = 1; k < HC_WAVES; ++k) b = hc_min(b, HcBest{s_v[k], s_i[k]});
    __syncthreads();
    return b;
}

// (no __restrict__: the matrix, chain, sizes and flags are written by one
// thread and read by the others behind a barrier)
__global__ void __launch_bounds__(HC_THREADS) k_hc_chain(double* D, int N, scc_hc_state* S, int* chain, double* size,
                                                         uint8_t* act, int* out_a, int* out_b, double* out_h,
                                                         int max_merges)
{
    __shared__ double s_v[HC_WAVES];
    __shared__ int s_i[HC_WAVES];
    const int tid = threadIdx.x;
    int start = S->start, tip = S->tip, step = S->step, err = S->err;
    long long scans = S->scans;
    if (err || step >= N - 1 || start < 0 || start >= N || tip < 0 || tip >= N) {
        if (!err && step < N - 1 && tid == 0) S->err = SCC_HC_ERR_STATE;
        return;
    }
    const long long scan_cap = 3ll * N;
    const size_t n = (size_t)N;
    for (int m = 0; m < max_merges && step < N - 1 && !err; ++m) {
        int i1, i2;
        double mn;
        if (tip <= 3) {
            i1 = start;
            const HcBest b = hc_row_min(D, N, i1, act, s_v, s_i);
            ++scans;
            if (b.i == INT_MAX) {
                err = SCC_HC_ERR_STATE;  // fewer than two active nodes before the last merge
                break;
            }
            i2 = b.i;
            mn = b.v;
            if (tid == 0) chain[0] = i1;
            tip = 1;
        } else {
            tip -= 3;
            i1 = chain[tip - 1];
            i2 = chain[tip];
            if (i1 < 0 || i1 >= N || i2 < 0 || i2 >= N || i1 == i2) {
                err = SCC_HC_ERR_STATE;
                break;
            }
            mn = D[(size_t)i1 * n + i2];
        }
        // grow the chain until the nearest neighbour of its tip is the node
        // before the tip (chain[tip - 1] == i1 at every entry)
        for (int ext = 0;; ++ext) {
            if (ext >= N || scans >= scan_cap || tip >= N) {
                err = SCC_HC_ERR_CAP;
                break;
            }
            if (tid == 0) chain[tip] = i2;
            const HcBest b = hc_row_min(D, N, i2, act, s_v, s_i);
            ++scans;
            const int before = i1;
            if (b.i != INT_MAX && b.v < mn) {
                mn = b.v;
                i1 = b.i;
            }
            const int nn = i1;
            i1 = i2;
            i2 = nn;
            ++tip;
            if (i2 == before) break;
        }
        if (err) break;

        // merge (i1, i2): the larger index survives
        const int lo = i1 < i2 ? i1 : i2, hi = i1 < i2 ? i2 : i1;
        const double s = size[lo], t = size[hi];
        double* rlo = D + (size_t)lo * n;
        double* rhi = D + (size_t)hi * n;
        int first = INT_MAX;  // the lowest active index other than lo (the next start)
        for (int i0 = tid; i0 < N; i0 += HC_THREADS * HC_UPD_U) {
            double v[HC_UPD_U], a[HC_UPD_U], b[HC_UPD_U];
            uint8_t on[HC_UPD_U];
#pragma unroll
            for (int u = 0; u < HC_UPD_U; ++u) {  // loads first
                const int i = i0 + u * HC_THREADS;
                const bool in = i < N;
                on[u] = in ? act[i] : (uint8_t)0;
                v[u] = in ? size[i] : 1.0;
                a[u] = in ? rlo[i] : 0.0;
                b[u] = in ? rhi[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HC_UPD_U; ++u) {
                const int i = i0 + u * HC_THREADS;
                if (!on[u] || i == lo) continue;
                if (first == INT_MAX) first = i;
                if (i == hi) continue;
                const double nv = ((v[u] + s) * a[u] - v[u] * mn + (v[u] + t) * b[u]) / (s + t + v[u]);
                rhi[i] = nv;
                D[(size_t)i * n + hi] = nv;
            }
        }
        if (lo == start) {
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) first = min(first, __shfl_xor(first, k, SCC_WAVE));
            if ((tid & 63) == 0) s_i[tid >> 6] = first;
            __syncthreads();
            first = s_i[0];
#pragma unroll
            for (int k = 1; k < HC_WAVES; ++k) first = min(first, s_i[k]);
            start = first;  // hi is active, so there is one
        }
        __syncthreads();  // s, t and the rows are read: the state may change
        if (tid == 0) {
            size[hi] = t + s;  // host: size[i2] += size[i1]
            act[lo] = 0;
            out_a[step] = i1;
            out_b[step] = i2;
            out_h[step] = mn;
        }
        ++step;
        __syncthreads();
    }
    if (tid == 0) {
        S->start = start;
        S->tip = tip;
        S->step = step;
        S->scans = scans;
        if (err) S->err = err;
    }
}

// chain / sizes / flags / state of a fresh call
__global__ void k_hc_init(int N, scc_hc_state* S, double* size, uint8_t* act, unsigned int* nonfinite)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        size[i] = 1.0;
        act[i] = 1;
    }
    if (i == 0) {
        S->start = 0;
        S->tip = 0;
        S->step = 0;
        S->err = 0;
        S->scans = 0;
        *nonfinite = 0;
    }
}

// block[j * cs + i] = distM[core[i], core[j]] (core: 1-based ids; 0 on the diagonal)
template <class T>
__global__ void __launch_bounds__(256) k_hc_gather_core(const T* __restrict__ P, int N, const int* __restrict__ core,
                                                        int cs, double* __restrict__ block)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cs * cs) return;
    const int ci = core[k % cs] - 1, cj = core[k / cs] - 1;
    double v = 0.0;
    if (ci != cj && ci >= 0 && cj >= 0 && ci < N && cj < N)
        v = (double)(ci < cj ? P[hc_pidx((size_t)N, ci, cj)] : P[hc_pidx((size_t)N, cj, ci)]);
    block[k] = v;
}

extern "C" hipError_t scc_launch_hc_init(int N, scc_hc_state* S, double* size, uint8_t* act, unsigned int* nonfinite,
                                         hipStream_t st)
{
    hipLaunchKernelGGL(k_hc_init, dim3((N + 255) / 256), dim3(256), 0, st, N, S, size, act, nonfinite);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_hc_expand(const void* P, int f32, int N, double* D, unsigned int* nonfinite,
                                           hipStream_t st)
{
    const int nt = (N + HC_TILE - 1) / HC_TILE;
    const dim3 grid(nt, nt), block(HC_TILE, 8);
    if (f32)
        hipLaunchKernelGGL(k_hc_expand<float>, grid, block, 0, st, (const float*)P, N, D, nonfinite);
    else
        hipLaunchKernelGGL(k_hc_expand<double>, grid, block, 0, st, (const double*)P, N, D, nonfinite);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_hc_chain(double* D, int N, scc_hc_state* S, int* chain, double* size, uint8_t* act,
                                          int* out_a, int* out_b, double* out_h, int max_merges, hipStream_t st)
{
    hipLaunchKernelGGL(k_hc_chain, dim3(1), dim3(HC_THREADS), 0, st, D, N, S, chain, size, act, out_a, out_b, out_h,
                       max_merges);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_hc_gather_core(const void* P, int f32, int N, const int* core, int cs, double* block,
                                                hipStream_t st)
{
    const dim3 grid((cs * cs + 255) / 256);
    if (f32)
        hipLaunchKernelGGL(k_hc_gather_core<float>, grid, dim3(256), 0, st, (const float*)P, N, core, cs, block);
    else
        hipLaunchKernelGGL(k_hc_gather_core<double>, grid, dim3(256), 0, st, (const double*)P, N, core, cs, block);
    return hipGetLastError();
}
