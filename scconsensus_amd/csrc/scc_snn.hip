// scc_snn.hip — the shared-nearest-neighbour graph of a k-NN table and the
// multilevel modularity clustering of a symmetric weighted graph on the device
// (include/scc.h: scc_snn_graph, scc_modularity_cluster, scc_snn_clusters_scores;
// host driver: scc_snn.cpp; the rules restated in NumPy: tests/snn_reference.py).
//
// No floating-point atomic is used.  The graph's values are a function of the
// integer shared count alone; the clustering's weights are the integers
// q = rint(w 2^32), so every sum of weights is an exact int64 and integer
// atomics in any order give the same value.  The integer atomics that order
// anything (fill cursors, hash slots) decide no output bit: the fill order is
// undone by the row sort, a hash slot's place is never read, and the best
// community is the maximum of the total order (gain, smaller id).
//
// Graph (Seurat's ComputeSNN rule, K = k + 1, N_i = {i} + idx[i]):
//   k_snn_sets     a thread per member: its rank among the row's K members is
//                  its place (S [n][K], ascending)
//   k_snn_rcount   a thread per member m of N_i: counts row i for R(m), the rows
//   k_snn_rfill    that hold m; R(m) stays in fill order (nothing reads its order)
//   k_snn_pairs    SNN_LANES lanes own row i (S_i staged in LDS); for m in S_i in
//                  order the lanes split R(m); a candidate j is merged with S_i
//                  (2K steps: the shared count s and the smallest shared member);
//                  the pair is taken only where that member is m, so once.  The
//                  first pass counts (one butterfly per row), the second writes
//                  at a cursor.  A hub's R(m) is the same loop with more rounds.
//   k_snn_sort     a thread per entry: its rank among its row's columns is its
//                  place; the value s / (K + (K - s)) is formed here
//
// Clustering (one level: synchronous sweeps on double-buffered communities):
//   k_mc_degree    MC_LANES lanes per row: k_i, the longest row, m2
//   k_mc_move      a wave per vertex with at most MC_SHORT entries: the row's
//                  (community -> kin) table in LDS (MC_SLOTS slots, open
//                  addressing, atomicCAS on the key, atomicAdd on the int64
//                  sum), then the lanes split the slots and one butterfly on
//                  (gain, id) picks the best
//   k_mc_move_long a workgroup per longer row, the same table in global memory
//                  (2 len slots at 2 indptr[i]), read back through atomics
//   k_mc_state     MC_LANES lanes per row: tot, size and the inside weight of
//                  the new communities
//   k_mc_terms, k_mc_total   Q in one fixed shape (thread t adds terms t,
//                  t + 1024, ..., then a halving tree)
//   aggregation    the coarse key (new row << 32 | new column) of every entry,
//                  rocprim radix sort and reduce-by-key (integer sums), then the
//                  coarse CSR by count and scan
#include "scc_common.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>

#include <climits>

#define SNN_LANES 16     // lanes that share a row in k_snn_pairs
#define SNN_MAXK 65      // K = k + 1 at most (SCC_KNN_MAX_K + 1)
#define SNN_SCAN_T 1024  // threads of the scan and total workgroups
#define MC_LANES 16      // lanes that share a row in k_mc_degree, k_mc_state, k_mc_keys
#define MC_SHORT 256     // entries of a row the LDS table takes
#define MC_SLOTS 512     // its slots (load at most 1/2)

// ------------------------------------------------------------------ graph

__global__ void __launch_bounds__(256) k_snn_sets(const int* __restrict__ idx, int n, int k, int* __restrict__ S)
{
    const int K = k + 1;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * K) return;
    const int i = (int)(t / K), s = (int)(t % K);
    const int* r = idx + (size_t)i * k;
    const int v = s ? r[s - 1] : i;
    int rank = v > i;
    for (int q = 0; q < k; ++q) rank += r[q] < v;
    S[(size_t)i * K + rank] = v;  // the members of a row are distinct: rank < K, one member per place
}

__global__ void __launch_bounds__(256) k_snn_rcount(const int* __restrict__ S, size_t nK, int* __restrict__ cnt)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < nK) atomicAdd(&cnt[S[t]], 1);
}

// out[0..n] = exclusive scan of cnt[0..n), by one workgroup chunk after chunk
__global__ void __launch_bounds__(SNN_SCAN_T) k_snn_scan(const int* __restrict__ cnt, int n, i64* __restrict__ out)
{
    __shared__ i64 sh[SNN_SCAN_T];
    const int t = threadIdx.x;
    i64 carry = 0;
    for (int c0 = 0; c0 < n; c0 += SNN_SCAN_T) {
        const i64 v = c0 + t < n ? (i64)cnt[c0 + t] : 0;
        sh[t] = v;
        __syncthreads();
        for (int m = 1; m < SNN_SCAN_T; m <<= 1) {  // Hillis-Steele, inclusive
            const i64 a = t >= m ? sh[t - m] : 0;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (c0 + t < n) out[c0 + t] = carry + sh[t] - v;
        carry += sh[SNN_SCAN_T - 1];
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

__global__ void __launch_bounds__(256) k_snn_rfill(const int* __restrict__ S, size_t nK, int K,
                                                   const i64* __restrict__ rptr, int* __restrict__ cur,
                                                   int* __restrict__ R)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nK) return;
    const int m = S[t];
    R[rptr[m] + atomicAdd(&cur[m], 1)] = (int)(t / K);  // < rptr[m + 1]: k_snn_rcount counted this member
}

template <bool FILL>
__global__ void __launch_bounds__(256) k_snn_pairs(const int* __restrict__ S, int n, int K, const i64* __restrict__ rptr,
                                                   const int* __restrict__ R, double prune, int* __restrict__ cnt,
                                                   const i64* __restrict__ indptr, int* __restrict__ cur,
                                                   int* __restrict__ cols_u, int* __restrict__ s_u,
                                                   int* __restrict__ rowid)
{
    __shared__ int sh[256 / SNN_LANES][SNN_MAXK];
    const int grp = threadIdx.x / SNN_LANES, l = threadIdx.x % SNN_LANES;
    const i64 row = (i64)blockIdx.x * (256 / SNN_LANES) + grp;
    const bool live = row < n;  // a group past n finds nothing and stays for the barrier and the butterfly
    const int i = live ? (int)row : 0;
    int* Si = sh[grp];
    if (live)
        for (int a = l; a < K; a += SNN_LANES) Si[a] = S[(size_t)i * K + a];
    __syncthreads();
    int found = 0;
    if (live) {
        for (int mi = 0; mi < K; ++mi) {
            const int m = Si[mi];
            const i64 p1 = rptr[m + 1];
            for (i64 p = rptr[m] + l; p < p1; p += SNN_LANES) {
                const int j = R[p];
                if (j == i) continue;
                const int* Sj = S + (size_t)j * K;
                int a = 0, b = 0, s = 0, first = -1;
                int x = Si[0], y = Sj[0];
                while (true) {  // at most 2K - 1 steps
                    if (x == y) {
                        if (first < 0) first = x;
                        ++s;
                        ++a;
                        ++b;
                        if (a >= K || b >= K) break;
                        x = Si[a];
                        y = Sj[b];
                    } else if (x < y) {
                        if (++a >= K) break;
                        x = Si[a];
                    } else {
                        if (++b >= K) break;
                        y = Sj[b];
                    }
                }
                if (first != m) continue;  // the pair belongs to its smallest shared member
                const double w = (double)s / (double)(K + (K - s));
                if (!(w >= prune)) continue;
                if (FILL) {
                    const i64 pos = indptr[i] + atomicAdd(&cur[i], 1);  // < indptr[i + 1]: the count pass counted it
                    cols_u[pos] = j;
                    s_u[pos] = s;
                    rowid[pos] = i;
                } else {
                    ++found;
                }
            }
        }
    }
    if (!FILL) {
#pragma unroll
        for (int m = SNN_LANES / 2; m >= 1; m >>= 1) found += __shfl_xor(found, m, SNN_LANES);
        if (live && l == 0) cnt[i] = found;
    }
}

__global__ void __launch_bounds__(256) k_snn_sort(const i64* __restrict__ indptr, const int* __restrict__ rowid,
                                                  const int* __restrict__ cols_u, const int* __restrict__ s_u, i64 nnz,
                                                  int K, int* __restrict__ cols, int* __restrict__ shared,
                                                  double* __restrict__ vals)
{
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnz) return;
    const int r = rowid[p], c = cols_u[p], s = s_u[p];
    const i64 p0 = indptr[r], p1 = indptr[r + 1];
    i64 rank = 0;
    for (i64 q = p0; q < p1; ++q) rank += cols_u[q] < c;
    cols[p0 + rank] = c;  // the columns of a row are distinct: rank < p1 - p0, one entry per place
    shared[p0 + rank] = s;
    vals[p0 + rank] = (double)s / (double)(K + (K - s));
}

// ------------------------------------------------------------------ clustering

__global__ void __launch_bounds__(256) k_mc_quant(const double* __restrict__ vals, i64 nnz, i64* __restrict__ q)
{
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p < nnz) q[p] = (i64)rint(vals[p] * 4294967296.0);
}

// head[0] = m2 (added to), head[1] = the longest row (a maximum)
__global__ void __launch_bounds__(256) k_mc_degree(const i64* __restrict__ indptr, const i64* __restrict__ q, int n,
                                                   i64* __restrict__ deg, u64* __restrict__ head)
{
    const i64 gt = (i64)blockIdx.x * 256 + threadIdx.x;
    const int l = (int)(gt % MC_LANES);
    const i64 i = gt / MC_LANES;
    i64 s = 0, len = 0;
    if (i < n) {
        const i64 p0 = indptr[i], p1 = indptr[i + 1];
        len = p1 - p0;
        for (i64 p = p0 + l; p < p1; p += MC_LANES) s += q[p];
    }
#pragma unroll
    for (int m = MC_LANES / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, MC_LANES);
    if (i < n && l == 0) {
        deg[i] = s;
        if (s) atomicAdd((unsigned long long*)&head[0], (unsigned long long)s);
        atomicMax((unsigned long long*)&head[1], (unsigned long long)len);
    }
}

__global__ void __launch_bounds__(256) k_mc_init(const i64* __restrict__ deg, int n, int* __restrict__ comm,
                                                 i64* __restrict__ tot, int* __restrict__ size)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    comm[i] = i;
    tot[i] = deg[i];
    size[i] = 1;
}

__device__ inline bool mc_better(double g, int c, double bg, int bc) { return g > bg || (g == bg && c < bc); }

__device__ inline void mc_decide(int i, int ci, double g_own, double best_g, int best_c, const int* __restrict__ size,
                                 int* __restrict__ comm_new, int* __restrict__ moved)
{
    const bool move = best_c != ci && best_g > g_own && !(size[best_c] == 1 && size[ci] == 1 && best_c > ci);
    comm_new[i] = move ? best_c : ci;
    if (move) atomicAdd(moved, 1);
}

__global__ void __launch_bounds__(256) k_mc_move(const i64* __restrict__ indptr, const int* __restrict__ cols,
                                                 const i64* __restrict__ q, const i64* __restrict__ deg, int n,
                                                 const int* __restrict__ comm, const i64* __restrict__ tot,
                                                 const int* __restrict__ size, double gamma, double m2,
                                                 int* __restrict__ comm_new, int* __restrict__ moved)
{
    __shared__ int keys[4][MC_SLOTS];
    __shared__ u64 sums[4][MC_SLOTS];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const i64 row = (i64)blockIdx.x * 4 + wv;
    const int i = row < n ? (int)row : 0;
    i64 p0 = 0, p1 = 0;
    if (row < n) {
        p0 = indptr[i];
        p1 = indptr[i + 1];
    }
    const bool mine = row < n && p1 - p0 <= MC_SHORT;  // a longer row is k_mc_move_long's
    int* Kt = keys[wv];
    u64* Vt = sums[wv];
    for (int s = l; s < MC_SLOTS; s += 64) {
        Kt[s] = -1;
        Vt[s] = 0;
    }
    __syncthreads();
    if (mine)
        for (i64 p = p0 + l; p < p1; p += 64) {
            const int j = cols[p];
            const i64 w = q[p];
            if (j == i || w == 0) continue;
            const int c = comm[j];
            unsigned h = ((unsigned)c * 2654435761u) >> 23;  // 9 bits
            for (int it = 0; it < MC_SLOTS; ++it) {          // at most MC_SHORT keys: a free slot is met
                const int prev = atomicCAS(&Kt[h], -1, c);
                if (prev == -1 || prev == c) {
                    atomicAdd((unsigned long long*)&Vt[h], (unsigned long long)w);
                    break;
                }
                h = (h + 1) & (MC_SLOTS - 1);
            }
        }
    __syncthreads();
    int ci = 0, best_c = INT_MAX;
    double g_own = 0.0, best_g = -INFINITY;
    if (mine) {
        ci = comm[i];
        const i64 ki = deg[i];
        const double gk = gamma * (double)ki;
        i64 kin_own = 0;
        unsigned h = ((unsigned)ci * 2654435761u) >> 23;
        for (int it = 0; it < MC_SLOTS; ++it) {
            const int key = Kt[h];
            if (key == ci) kin_own = (i64)Vt[h];
            if (key == ci || key == -1) break;
            h = (h + 1) & (MC_SLOTS - 1);
        }
        g_own = (double)kin_own - (gk * (double)(tot[ci] - ki)) / m2;
        best_g = g_own;
        best_c = ci;
        for (int s = l; s < MC_SLOTS; s += 64) {
            const int c = Kt[s];
            if (c < 0 || c == ci) continue;
            const double g = (double)(i64)Vt[s] - (gk * (double)tot[c]) / m2;
            if (mc_better(g, c, best_g, best_c)) {
                best_g = g;
                best_c = c;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double og = __shfl_xor(best_g, m);
        const int oc = __shfl_xor(best_c, m);
        if (mc_better(og, oc, best_g, best_c)) {
            best_g = og;
            best_c = oc;
        }
    }
    if (mine && l == 0) mc_decide(i, ci, g_own, best_g, best_c, size, comm_new, moved);
}

// a workgroup per row of more than MC_SHORT entries; gkeys, gsums: 2 nnz slots, row i's 2 len at 2 indptr[i]
__global__ void __launch_bounds__(256) k_mc_move_long(const i64* __restrict__ indptr, const int* __restrict__ cols,
                                                      const i64* __restrict__ q, const i64* __restrict__ deg, int n,
                                                      const int* __restrict__ comm, const i64* __restrict__ tot,
                                                      const int* __restrict__ size, double gamma, double m2,
                                                      int* __restrict__ gkeys, u64* __restrict__ gsums,
                                                      int* __restrict__ comm_new, int* __restrict__ moved)
{
    __shared__ double sh_g[256];
    __shared__ int sh_c[256];
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= n) return;
    const i64 p0 = indptr[i], p1 = indptr[i + 1];
    if (p1 - p0 <= MC_SHORT) return;  // (the whole workgroup: before any barrier)
    const u64 slots = 2 * (u64)(p1 - p0);
    int* Kt = gkeys + 2 * p0;
    u64* Vt = gsums + 2 * p0;
    for (u64 s = t; s < slots; s += 256) {
        Kt[s] = -1;
        Vt[s] = 0;
    }
    __syncthreads();
    for (i64 p = p0 + t; p < p1; p += 256) {
        const int j = cols[p];
        const i64 w = q[p];
        if (j == i || w == 0) continue;
        const int c = comm[j];
        u64 h = (u64)((unsigned)c * 2654435761u) % slots;
        for (u64 it = 0; it < slots; ++it) {  // at most len keys in 2 len slots: a free slot is met
            const int prev = atomicCAS(&Kt[h], -1, c);
            if (prev == -1 || prev == c) {
                atomicAdd((unsigned long long*)&Vt[h], (unsigned long long)w);
                break;
            }
            if (++h == slots) h = 0;
        }
    }
    __syncthreads();
    const int ci = comm[i];
    const i64 ki = deg[i];
    const double gk = gamma * (double)ki;
    i64 kin_own = 0;
    {
        u64 h = (u64)((unsigned)ci * 2654435761u) % slots;
        for (u64 it = 0; it < slots; ++it) {
            const int key = atomicOr(&Kt[h], 0);  // (read where the atomics wrote)
            if (key == ci) kin_own = (i64)atomicAdd((unsigned long long*)&Vt[h], 0ull);
            if (key == ci || key == -1) break;
            if (++h == slots) h = 0;
        }
    }
    const double g_own = (double)kin_own - (gk * (double)(tot[ci] - ki)) / m2;
    double best_g = g_own;
    int best_c = ci;
    for (u64 s = t; s < slots; s += 256) {
        const int c = atomicOr(&Kt[s], 0);
        if (c < 0 || c == ci) continue;
        const double g = (double)(i64)atomicAdd((unsigned long long*)&Vt[s], 0ull) - (gk * (double)tot[c]) / m2;
        if (mc_better(g, c, best_g, best_c)) {
            best_g = g;
            best_c = c;
        }
    }
    sh_g[t] = best_g;
    sh_c[t] = best_c;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (t < m && mc_better(sh_g[t + m], sh_c[t + m], sh_g[t], sh_c[t])) {
            sh_g[t] = sh_g[t + m];
            sh_c[t] = sh_c[t + m];
        }
        __syncthreads();
    }
    if (t == 0) mc_decide(i, ci, g_own, sh_g[0], sh_c[0], size, comm_new, moved);
}

// tot, size, inc (zeroed by the launcher): the totals, sizes and inside weights of the communities in comm
__global__ void __launch_bounds__(256) k_mc_state(const i64* __restrict__ indptr, const int* __restrict__ cols,
                                                  const i64* __restrict__ q, const i64* __restrict__ deg, int n,
                                                  const int* __restrict__ comm, i64* __restrict__ tot,
                                                  int* __restrict__ size, i64* __restrict__ inc)
{
    const i64 gt = (i64)blockIdx.x * 256 + threadIdx.x;
    const int l = (int)(gt % MC_LANES);
    const i64 i = gt / MC_LANES;
    i64 s = 0;
    int c = 0;
    if (i < n) {
        c = comm[i];
        const i64 p1 = indptr[i + 1];
        for (i64 p = indptr[i] + l; p < p1; p += MC_LANES)
            if (comm[cols[p]] == c) s += q[p];
    }
#pragma unroll
    for (int m = MC_LANES / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, MC_LANES);
    if (i < n && l == 0) {
        if (deg[i]) atomicAdd((unsigned long long*)&tot[c], (unsigned long long)deg[i]);
        atomicAdd(&size[c], 1);
        if (s) atomicAdd((unsigned long long*)&inc[c], (unsigned long long)s);
    }
}

__global__ void __launch_bounds__(256) k_mc_terms(const i64* __restrict__ inc, const i64* __restrict__ tot, int n,
                                                  double gamma, double m2, double* __restrict__ term)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const double a = (double)tot[c] / m2;
    term[c] = (double)inc[c] / m2 - (gamma * a) * a;
}

// out[0] = the sum of x[0..n) in one shape: thread t adds x[t], x[t + T], ... in order, then a halving tree
__global__ void __launch_bounds__(SNN_SCAN_T) k_mc_total(const double* __restrict__ x, int n, double* __restrict__ out)
{
    __shared__ double sh[SNN_SCAN_T];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += SNN_SCAN_T) s += x[i];
    sh[t] = s;
    __syncthreads();
    for (int m = SNN_SCAN_T / 2; m >= 1; m >>= 1) {
        if (t < m) sh[t] += sh[t + m];
        __syncthreads();
    }
    if (t == 0) out[0] = sh[0];
}

__global__ void __launch_bounds__(256) k_mc_flags(const int* __restrict__ size, int n, int* __restrict__ flag)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n) flag[c] = size[c] > 0;
}

// member[v] = the coarse vertex of v: newid[comm[member[v]]]
__global__ void __launch_bounds__(256) k_mc_member(const int* __restrict__ comm, const i64* __restrict__ newid, int n0,
                                                   int* __restrict__ member)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < n0) member[v] = (int)newid[comm[member[v]]];
}

__global__ void __launch_bounds__(256) k_mc_keys(const i64* __restrict__ indptr, const int* __restrict__ cols, int n,
                                                 const int* __restrict__ comm, const i64* __restrict__ newid,
                                                 u64* __restrict__ key)
{
    const i64 gt = (i64)blockIdx.x * 256 + threadIdx.x;
    const int l = (int)(gt % MC_LANES);
    const i64 i = gt / MC_LANES;
    if (i >= n) return;
    const u64 hi = (u64)newid[comm[i]] << 32;
    const i64 p1 = indptr[i + 1];
    for (i64 p = indptr[i] + l; p < p1; p += MC_LANES) key[p] = hi | (u64)newid[comm[cols[p]]];
}

// the coarse entries (sorted unique keys): columns and the entries of every row
__global__ void __launch_bounds__(256) k_mc_coarse(const u64* __restrict__ ukey, i64 ne, int* __restrict__ cols,
                                                   int* __restrict__ cnt)
{
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    cols[e] = (int)(ukey[e] & 0xffffffffull);
    atomicAdd(&cnt[(int)(ukey[e] >> 32)], 1);
}

// ------------------------------------------------------------------ launchers

static inline unsigned blocks(i64 items, int per = 256) { return (unsigned)((items + per - 1) / per); }

// S [n][K]; rcnt [n] (zeroed here); rptr [n + 1]
extern "C" hipError_t scc_launch_snn_sets(const int* idx, int n, int k, int* S, int* rcnt, i64* rptr, hipStream_t st)
{
    const size_t nK = (size_t)n * (k + 1);
    hipError_t e = hipMemsetAsync(rcnt, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_snn_sets, dim3(blocks((i64)nK)), dim3(256), 0, st, idx, n, k, S);
    hipLaunchKernelGGL(k_snn_rcount, dim3(blocks((i64)nK)), dim3(256), 0, st, S, nK, rcnt);
    hipLaunchKernelGGL(k_snn_scan, dim3(1), dim3(SNN_SCAN_T), 0, st, rcnt, n, rptr);
    return hipGetLastError();
}

// R [n K]; cur [n] (zeroed here); then the count pass: cnt [n], indptr [n + 1]
extern "C" hipError_t scc_launch_snn_count(const int* S, int n, int k, const i64* rptr, int* cur, int* R, double prune,
                                           int* cnt, i64* indptr, hipStream_t st)
{
    const int K = k + 1;
    const size_t nK = (size_t)n * K;
    hipError_t e = hipMemsetAsync(cur, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_snn_rfill, dim3(blocks((i64)nK)), dim3(256), 0, st, S, nK, K, rptr, cur, R);
    hipLaunchKernelGGL(k_snn_pairs<false>, dim3(blocks(n, 256 / SNN_LANES)), dim3(256), 0, st, S, n, K, rptr, R, prune,
                       cnt, (const i64*)nullptr, (int*)nullptr, (int*)nullptr, (int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_snn_scan, dim3(1), dim3(SNN_SCAN_T), 0, st, cnt, n, indptr);
    return hipGetLastError();
}

// cols_u, s_u, rowid, cols, shared, vals: nnz entries each (nnz = indptr[n] > 0); cur [n] (zeroed here)
extern "C" hipError_t scc_launch_snn_fill(const int* S, int n, int k, const i64* rptr, const int* R, double prune,
                                          const i64* indptr, i64 nnz, int* cur, int* cols_u, int* s_u, int* rowid,
                                          int* cols, int* shared, double* vals, hipStream_t st)
{
    const int K = k + 1;
    hipError_t e = hipMemsetAsync(cur, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_snn_pairs<true>, dim3(blocks(n, 256 / SNN_LANES)), dim3(256), 0, st, S, n, K, rptr, R, prune,
                       (int*)nullptr, indptr, cur, cols_u, s_u, rowid);
    hipLaunchKernelGGL(k_snn_sort, dim3(blocks(nnz)), dim3(256), 0, st, indptr, rowid, cols_u, s_u, nnz, K, cols, shared,
                       vals);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_mc_quant(const double* vals, i64 nnz, i64* q, hipStream_t st)
{
    if (nnz > 0) hipLaunchKernelGGL(k_mc_quant, dim3(blocks(nnz)), dim3(256), 0, st, vals, nnz, q);
    return hipGetLastError();
}

// deg [n]; head [2] (zeroed here): m2 and the longest row
extern "C" hipError_t scc_launch_mc_degree(const i64* indptr, const i64* q, int n, i64* deg, u64* head, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(head, 0, 2 * sizeof(u64), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mc_degree, dim3(blocks((i64)n * MC_LANES)), dim3(256), 0, st, indptr, q, n, deg, head);
    return hipGetLastError();
}

extern "C" hipError_t scc_launch_mc_init(const i64* deg, int n, int* comm, i64* tot, int* size, hipStream_t st)
{
    hipLaunchKernelGGL(k_mc_init, dim3(blocks(n)), dim3(256), 0, st, deg, n, comm, tot, size);
    return hipGetLastError();
}

// one sweep's moves: comm -> comm_new, out_moved[0] counted (zeroed here); gkeys, gsums only when longest > MC_SHORT
extern "C" hipError_t scc_launch_mc_move(const i64* indptr, const int* cols, const i64* q, const i64* deg, int n,
                                         i64 longest, const int* comm, const i64* tot, const int* size, double gamma,
                                         double m2, int* gkeys, u64* gsums, int* comm_new, int* moved, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(moved, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mc_move, dim3(blocks(n, 4)), dim3(256), 0, st, indptr, cols, q, deg, n, comm, tot, size, gamma,
                       m2, comm_new, moved);
    if (longest > MC_SHORT)
        hipLaunchKernelGGL(k_mc_move_long, dim3((unsigned)n), dim3(256), 0, st, indptr, cols, q, deg, n, comm, tot, size,
                           gamma, m2, gkeys, gsums, comm_new, moved);
    return hipGetLastError();
}

extern "C" int scc_mc_short_row(void) { return MC_SHORT; }

// the state of comm: tot, size, inc [n] (zeroed here), then Q into out_q[0] (term [n] scratch)
extern "C" hipError_t scc_launch_mc_state(const i64* indptr, const int* cols, const i64* q, const i64* deg, int n,
                                          const int* comm, double gamma, double m2, i64* tot, int* size, i64* inc,
                                          double* term, double* out_q, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(tot, 0, sizeof(i64) * (size_t)n, st);
    if (e == hipSuccess) e = hipMemsetAsync(size, 0, sizeof(int) * (size_t)n, st);
    if (e == hipSuccess) e = hipMemsetAsync(inc, 0, sizeof(i64) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mc_state, dim3(blocks((i64)n * MC_LANES)), dim3(256), 0, st, indptr, cols, q, deg, n, comm, tot,
                       size, inc);
    hipLaunchKernelGGL(k_mc_terms, dim3(blocks(n)), dim3(256), 0, st, inc, tot, n, gamma, m2, term);
    hipLaunchKernelGGL(k_mc_total, dim3(1), dim3(SNN_SCAN_T), 0, st, term, n, out_q);
    return hipGetLastError();
}

// newid [n + 1] = exclusive scan of (size > 0) (flag [n] scratch); member [n0] follows; key [nnz] = the coarse keys
extern "C" hipError_t scc_launch_mc_renumber(const i64* indptr, const int* cols, int n, i64 nnz, const int* comm,
                                             const int* size, int* flag, i64* newid, int n0, int* member, u64* key,
                                             hipStream_t st)
{
    hipLaunchKernelGGL(k_mc_flags, dim3(blocks(n)), dim3(256), 0, st, size, n, flag);
    hipLaunchKernelGGL(k_snn_scan, dim3(1), dim3(SNN_SCAN_T), 0, st, flag, n, newid);
    hipLaunchKernelGGL(k_mc_member, dim3(blocks(n0)), dim3(256), 0, st, comm, newid, n0, member);
    if (nnz > 0)
        hipLaunchKernelGGL(k_mc_keys, dim3(blocks((i64)n * MC_LANES)), dim3(256), 0, st, indptr, cols, n, comm, newid,
                           key);
    return hipGetLastError();
}

// bytes of rocprim scratch the sort and the reduce-by-key of nnz entries need (the larger of the two)
extern "C" hipError_t scc_mc_aggregate_bytes(i64 nnz, size_t* bytes)
{
    size_t a = 0, b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, a, (u64*)nullptr, (u64*)nullptr, (i64*)nullptr, (i64*)nullptr,
                                             (size_t)nnz, 0, 64, (hipStream_t)0);
    if (e != hipSuccess) return e;
    e = rocprim::reduce_by_key(nullptr, b, (u64*)nullptr, (i64*)nullptr, (size_t)nnz, (u64*)nullptr, (i64*)nullptr,
                               (i64*)nullptr, rocprim::plus<i64>(), rocprim::equal_to<u64>(), (hipStream_t)0);
    *bytes = a > b ? a : b;
    return e;
}

// key, q [nnz] -> sorted (key_s, q_s) -> unique keys ukey and their sums uq, the count in ne[0] (device)
extern "C" hipError_t scc_launch_mc_aggregate(void* tmp, size_t tmp_bytes, const u64* key, const i64* q, i64 nnz,
                                              int bits, u64* key_s, i64* q_s, u64* ukey, i64* uq, i64* ne,
                                              hipStream_t st)
{
    size_t bytes = tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, key, key_s, q, q_s, (size_t)nnz, 0, (unsigned)bits, st);
    if (e != hipSuccess) return e;
    bytes = tmp_bytes;
    return rocprim::reduce_by_key(tmp, bytes, key_s, q_s, (size_t)nnz, ukey, uq, ne, rocprim::plus<i64>(),
                                  rocprim::equal_to<u64>(), st);
}

// the coarse CSR of ne sorted unique keys: cols [ne], indptr [nc + 1] (cnt [nc] zeroed here)
extern "C" hipError_t scc_launch_mc_coarse(const u64* ukey, i64 ne, int nc, int* cols, int* cnt, i64* indptr,
                                           hipStream_t st)
{
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)nc, st);
    if (e != hipSuccess) return e;
    if (ne > 0) hipLaunchKernelGGL(k_mc_coarse, dim3(blocks(ne)), dim3(256), 0, st, ukey, ne, cols, cnt);
    hipLaunchKernelGGL(k_snn_scan, dim3(1), dim3(SNN_SCAN_T), 0, st, cnt, nc, indptr);
    return hipGetLastError();
}
