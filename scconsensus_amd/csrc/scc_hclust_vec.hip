// scc_hclust_vec.hip — hclust(ward.D2) and the tree cut's distance reads from
// the PCA scores, without the N x N matrix (include/scc.h:
// scc_hclust_ward_d2_scores, scc_cutree_hybrid_scores).
//
// Reference: cellTree = fastcluster::hclust(dist(scores), method = "ward.D2")
// (R/reclusterDEConsensusFast.R:398-411, R/reclusterDEConsensus.R:234-247) and
// cutreeDynamic(dendro, distM = as.matrix(d), ...) (Fast:421-427).  The
// distance is dist() of N points in 16 dimensions, and Ward linkage on
// Euclidean points is a function of centroids and sizes: the squared
// dissimilarity the Lance-Williams update carries between clusters A and B is
//   2 |A| |B| / (|A| + |B|) * |cA - cB|^2
// and a merge is the weighted mean of two centroids.  The state is 128 bytes
// of centroid per node instead of 8 N bytes of matrix row.
//
// The control flow is nn_chain_ward's (scc_cluster.cpp), as k_hc_chain
// (scc_hclust.hip) restates it: the tip <= 3 restart from the lowest active
// index, tip -= 3 after a merge, the ascending strict-< scan from the carried
// minimum (the lowest index wins a tie), the larger index survives a merge.
// The rounding differs from the matrix routes (a mean of centroids against an
// update of squared distances), so the tree is theirs whenever no two
// candidate dissimilarities lie within rounding of each other; on exact ties
// it is a valid Ward tree that may resolve the tie differently.
//
// One nearest-neighbour scan is two launches; the kernel boundary is the only
// communication between workgroups (no in-launch hand-off, no spin):
// k_wv_scan     grid over the nodes, SCC_HCLUST_VEC_SCAN_NODES per workgroup: the minimum of
//               wv_ward(i, r) over the workgroup's active nodes i != r, r the
//               node the state names; one (value, lowest index) partial per
//               workgroup.  wv_ward is bitwise symmetric in its two nodes
//               (the chain's reciprocity test relies on that): the difference
//               form, components in ascending order.
// k_wv_advance  one workgroup: the minimum of the partials under the total
//               order (value, index), which no arrival order can change; the
//               chain step; when the step closes a reciprocal pair, the merge
//               (centroid (s c_lo + t c_hi) / (s + t), size, flag, outputs,
//               the next start) and, after tip -= 3, the carried minimum
//               recomputed from the two centroids.  It leaves the node of the
//               next scan in the state.
// Launches after the last merge or after an error return at once.  Every
// data-dependent loop is capped as in k_hc_chain (one chain extension: n
// scans; one call: 3 n scans; chain positions < n): past a cap the state's
// error flag is set.
// The centroids are component-major ([16][n]: a scan's loads are contiguous
// across the lanes), a working copy made by k_wv_init from the caller's
// row-major scores, which are never written.
//
// k_wv_gather_core  the cs x cs block distM[core, core] from the scores with
//               the per-entry arithmetic of k_dist_aligned (scc_dist.hip): the
//               values the packed vector would hold, bit for bit.
#include "scc.h"
#include "scc_common.hpp"
#include "scc_dist_entry.hpp"
#include "scc_kernels.hpp"

#define WV_THREADS 256
#define WV_WAVES (WV_THREADS / SCC_WAVE)
#define WV_PER_THREAD (SCC_HCLUST_VEC_SCAN_NODES / WV_THREADS)
static_assert(SCC_HCLUST_VEC_SCAN_NODES % WV_THREADS == 0, "a scan workgroup owns whole rounds of its threads");

#define WV_RESTART 0  // the scan of row `start` that begins a chain
#define WV_EXTEND 1   // the scan of the chain's tip

struct WvBest {
    double v;
    int i;
};

// the earlier of two candidates in the host's scan: the smaller value, the
// lower index on a tie (i == INT_MAX: no candidate)
__device__ inline WvBest wv_min(WvBest a, WvBest b)
{
    const bool take = b.i != INT_MAX && (a.i == INT_MAX || b.v < a.v || (b.v == a.v && b.i < a.i));
    return take ? b : a;
}

// sum_q d[q]^2, q ascending; d = c_i - c_r or c_r - c_i: the squares are equal
__device__ inline double wv_sumsq(const double* d)
{
    double ss = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) ss = fma(d[q], d[q], ss);
    return ss;
}

// 2 s_i s_r / (s_i + s_r) * ss: every operation commutes in (i, r)
__device__ inline double wv_ward(double si, double sr, double ss) { return 2.0 * si * sr / (si + sr) * ss; }

// the same value in every thread; two barriers
__device__ inline WvBest wv_block_min(WvBest b, double* s_v, int* s_i)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        WvBest o{__shfl_xor(b.v, m, SCC_WAVE), __shfl_xor(b.i, m, SCC_WAVE)};
        b = wv_min(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6] = b.v;
        s_i[threadIdx.x >> 6] = b.i;
    }
    __syncthreads();
    b = WvBest{s_v[0], s_i[0]};
#pragma unroll
    for (int k = 1; k < WV_WAVES; ++k) b = wv_min(b, WvBest{s_v[k], s_i[k]});
    __syncthreads();
    return b;
}

// whether this launch has a scan to do, the same answer in k_wv_scan and in
// k_wv_advance (which alone reports a bad state)
__device__ inline bool wv_live(const scc_wv_state* S, int N)
{
    return !S->err && S->step < N - 1 && S->node >= 0 && S->node < N;
}

// scores [N][16] row-major -> centroids [16][N]; sizes, flags, the state
__global__ void __launch_bounds__(256) k_wv_init(const double* __restrict__ P, int N, double* __restrict__ C,
                                                 scc_wv_state* S, double* __restrict__ size,
                                                 uint8_t* __restrict__ act, unsigned int* nonfinite)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        unsigned int bad = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const double x = P[(size_t)i * 16 + q];
            if (!isfinite(x)) bad++;
            C[(size_t)q * (size_t)N + i] = x;
        }
        size[i] = 1.0;
        act[i] = 1;
        if (bad) atomicAdd(nonfinite, bad);
    }
    if (i == 0) {
        S->start = 0;
        S->tip = 0;
        S->step = 0;
        S->err = 0;
        S->scans = 0;
        S->node = 0;
        S->mode = WV_RESTART;
        S->i1 = 0;
        S->ext = 0;
        S->mn = 0.0;
    }
}

// k_wv_init's counter starts at zero
__global__ void k_wv_clear(unsigned int* nonfinite) { *nonfinite = 0; }

// grid ceil(N / SCC_HCLUST_VEC_SCAN_NODES); everything it reads is constant during the launch
__global__ void __launch_bounds__(WV_THREADS) k_wv_scan(const double* __restrict__ C, int N,
                                                        const scc_wv_state* __restrict__ S,
                                                        const double* __restrict__ size,
                                                        const uint8_t* __restrict__ act, double* __restrict__ part_v,
                                                        int* __restrict__ part_i)
{
    __shared__ double s_v[WV_WAVES];
    __shared__ int s_i[WV_WAVES];
    if (!wv_live(S, N)) return;
    const int r = S->node;
    const size_t n = (size_t)N;
    double cr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) cr[q] = C[(size_t)q * n + r];
    const double sr = size[r];
    WvBest b{INFINITY, INT_MAX};
#pragma unroll
    for (int u = 0; u < WV_PER_THREAD; ++u) {  // ascending i within a thread
        const int i = blockIdx.x * SCC_HCLUST_VEC_SCAN_NODES + u * WV_THREADS + threadIdx.x;
        if (i < N && i != r && act[i]) {
            double d[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) d[q] = C[(size_t)q * n + i] - cr[q];
            b = wv_min(b, WvBest{wv_ward(size[i], sr, wv_sumsq(d)), i});
        }
    }
    b = wv_block_min(b, s_v, s_i);
    if (threadIdx.x == 0) {
        part_v[blockIdx.x] = b.v;
        part_i[blockIdx.x] = b.i;
    }
}

// one workgroup.  (no __restrict__: centroids, chain, sizes and flags are
// written by some threads and read by others behind a barrier.)  Every thread
// follows the chain step with the same values; thread 0 stores them.
__global__ void __launch_bounds__(WV_THREADS) k_wv_advance(double* C, int N, scc_wv_state* S, int* chain, double* size,
                                                           uint8_t* act, const double* part_v, const int* part_i,
                                                           int nparts, int* out_a, int* out_b, double* out_h)
{
    __shared__ double s_v[WV_WAVES];
    __shared__ int s_i[WV_WAVES];
    __shared__ double s_d[16];
    const int tid = threadIdx.x;
    int start = S->start, tip = S->tip, step = S->step, err = S->err;
    int r = S->node, mode = S->mode, i1 = S->i1, ext = S->ext;
    long long scans = S->scans;
    double mn = S->mn;
    if (err || step >= N - 1) return;
    if (r < 0 || r >= N || start < 0 || start >= N || tip < 0 ||
        (mode == WV_EXTEND && (tip >= N || i1 < 0 || i1 >= N))) {  // (a restart sets tip itself)
        if (tid == 0) S->err = SCC_HC_ERR_STATE;
        return;
    }
    const size_t n = (size_t)N;
    const long long scan_cap = 3ll * N;

    // the scan's result: (value, index) is a total order, so the workgroups'
    // partials reduce to the same pair in any order
    WvBest b{INFINITY, INT_MAX};
    for (int p = tid; p < nparts; p += WV_THREADS) b = wv_min(b, WvBest{part_v[p], part_i[p]});
    b = wv_block_min(b, s_v, s_i);
    ++scans;
    if (b.i != INT_MAX && (b.i < 0 || b.i >= N)) err = SCC_HC_ERR_STATE;

    int i2 = r;
    bool merge = false;
    if (err) {
    } else if (mode == WV_RESTART) {
        if (b.i == INT_MAX) {
            err = SCC_HC_ERR_STATE;  // fewer than two active nodes before the last merge
        } else {
            i1 = r;
            i2 = b.i;
            mn = b.v;
            if (tid == 0) chain[0] = i1;
            tip = 1;
            ext = 0;
        }
    } else {
        if (tid == 0) chain[tip] = i2;  // tip < N: checked before this scan was scheduled
        const int before = i1;
        if (b.i != INT_MAX && b.v < mn) {
            mn = b.v;
            i1 = b.i;
        }
        const int nn = i1;
        i1 = i2;
        i2 = nn;
        ++tip;
        ++ext;
        merge = i2 == before;
    }

    if (!err && merge) {
        // merge (i1, i2): the larger index survives
        const int lo = i1 < i2 ? i1 : i2, hi = i1 < i2 ? i2 : i1;
        const double s = size[lo], t = size[hi];
        if (tid < 16) {
            const double cl = C[(size_t)tid * n + lo], ch = C[(size_t)tid * n + hi];
            C[(size_t)tid * n + hi] = (s * cl + t * ch) / (s + t);
        }
        if (lo == start) {  // the next start: the lowest active index above lo (hi is one)
            int first = INT_MAX;
            for (int base = lo + 1; base < N && first == INT_MAX; base += WV_THREADS) {
                const int i = base + tid;
                const WvBest f = wv_block_min(WvBest{0.0, (i < N && act[i]) ? i : INT_MAX}, s_v, s_i);
                first = f.i;
            }
            if (first == INT_MAX)
                err = SCC_HC_ERR_STATE;
            else
                start = first;
        }
        __syncthreads();  // s and t are read, the centroid of hi is stored
        if (tid == 0) {
            size[hi] = t + s;  // host: size[i2] += size[i1]
            act[lo] = 0;
            out_a[step] = i1;
            out_b[step] = i2;
            out_h[step] = mn;
        }
        ++step;
        if (!err && step < N - 1) {
            if (tip <= 3) {
                mode = WV_RESTART;
                r = start;
            } else {
                tip -= 3;
                i1 = chain[tip - 1];  // (stored by earlier launches: this one wrote chain[tip + 2])
                i2 = chain[tip];
                if (i1 < 0 || i1 >= N || i2 < 0 || i2 >= N || i1 == i2) {
                    err = SCC_HC_ERR_STATE;
                } else {
                    // the carried minimum, from the two centroids (neither is
                    // the one just stored: both nodes lie below the merged
                    // pair in the chain); per-lane loads, summed as wv_sumsq
                    if (tid < 16) s_d[tid] = C[(size_t)tid * n + i1] - C[(size_t)tid * n + i2];
                    __syncthreads();
                    double d[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) d[q] = s_d[q];
                    mn = wv_ward(size[i1], size[i2], wv_sumsq(d));
                    mode = WV_EXTEND;
                    r = i2;
                    ext = 0;
                }
            }
        }
    } else if (!err) {
        mode = WV_EXTEND;
        r = i2;
    }
    // the caps of the extension scan just scheduled
    if (!err && step < N - 1 && mode == WV_EXTEND && (ext >= N || scans >= scan_cap || tip >= N)) err = SCC_HC_ERR_CAP;
    if (!err && step < N - 1 && scans >= scan_cap) err = SCC_HC_ERR_CAP;
    if (tid == 0) {
        S->start = start;
        S->tip = tip;
        S->step = step;
        S->scans = scans;
        S->node = r;
        S->mode = mode;
        S->i1 = i1;
        S->ext = ext;
        S->mn = mn;
        if (err) S->err = err;
    }
}

// One entry of the packed vector as k_dist_aligned forms it (row i > column
// j), from the two score rows (scc_dist_entry.hpp).
__device__ inline double wv_dist_entry(const double* __restrict__ P, int i, int j)
{
    double pi[15], pj[15];
#pragma unroll
    for (int q = 0; q < 15; ++q) {
        pi[q] = P[(size_t)i * 16 + q];
        pj[q] = P[(size_t)j * 16 + q];
    }
    return scc_dist_entry15(pi, scc_dist_norm15(pi), pj, scc_dist_norm15(pj));
}

// block[j * cs + i] = distM[core[i], core[j]] (core: 1-based ids; 0 on the diagonal)
__global__ void __launch_bounds__(256) k_wv_gather_core(const double* __restrict__ P, int N,
                                                        const int* __restrict__ core, int cs,
                                                        double* __restrict__ block)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cs * cs) return;
    const int ci = core[k % cs] - 1, cj = core[k / cs] - 1;
    double v = 0.0;
    if (ci != cj && ci >= 0 && cj >= 0 && ci < N && cj < N) v = wv_dist_entry(P, max(ci, cj), min(ci, cj));
    block[k] = v;
}

extern "C" int scc_wv_scan_workgroups(int N) { return (N + SCC_HCLUST_VEC_SCAN_NODES - 1) / SCC_HCLUST_VEC_SCAN_NODES; }

extern "C" hipError_t scc_launch_wv_init(const double* P, int N, double* C, scc_wv_state* S, double* size, uint8_t* act,
                                         unsigned int* nonfinite, hipStream_t st)
{
    hipLaunchKernelGGL(k_wv_clear, dim3(1), dim3(1), 0, st, nonfinite);
    hipLaunchKernelGGL(k_wv_init, dim3((N + 255) / 256), dim3(256), 0, st, P, N, C, S, size, act, nonfinite);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_wv_scan(const double* C, int N, const scc_wv_state* S, const double* size,
                                         const uint8_t* act, double* part_v, int* part_i, hipStream_t st)
{
    hipLaunchKernelGGL(k_wv_scan, dim3(scc_wv_scan_workgroups(N)), dim3(WV_THREADS), 0, st, C, N, S, size, act, part_v,
                       part_i);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_wv_advance(double* C, int N, scc_wv_state* S, int* chain, double* size, uint8_t* act,
                                            const double* part_v, const int* part_i, int* out_a, int* out_b,
                                            double* out_h, hipStream_t st)
{
    hipLaunchKernelGGL(k_wv_advance, dim3(1), dim3(WV_THREADS), 0, st, C, N, S, chain, size, act, part_v, part_i,
                       scc_wv_scan_workgroups(N), out_a, out_b, out_h);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_wv_gather_core(const double* P, int N, const int* core, int cs, double* block,
                                                hipStream_t st)
{
    hipLaunchKernelGGL(k_wv_gather_core, dim3((cs * cs + 255) / 256), dim3(256), 0, st, P, N, core, cs, block);
    return hipGetLastError();
}
