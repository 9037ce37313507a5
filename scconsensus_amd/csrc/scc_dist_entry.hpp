// scc_dist_entry.hpp — one entry of dist(scores) outside the dist kernel.
//
// k_dist_aligned (scc_dist.hip) forms an entry of the packed vector from two
// score rows as: the ascending fma chains over the 15 components for the two
// squared norms and the dot product, fma(-2, dot, ni + nj), the difference
// form where that cancels (below 2^-20 of the norm sum), scc_sqrt_nr.  The
// kernels that need single entries without the vector (the tree cut's core
// blocks, scc_hclust_vec.hip; the silhouette from the scores, scc_sil.hip)
// share this restatement, so they see the bits the vector would hold.  Every
// step commutes in its two rows: the entry is bitwise symmetric.
#pragma once
#include "scc_common.hpp"

// |p|^2 over the 15 components, ascending
__device__ inline double scc_dist_norm15(const double* p)
{
    double n = 0.0;
#pragma unroll
    for (int q = 0; q < 15; ++q) n = fma(p[q], p[q], n);
    return n;
}

// the entry from two rows (15 components each, in registers) and their norms
// as scc_dist_norm15 gives them: a caller hoists a row and its norm out of a
// pair loop without changing a bit
__device__ inline double scc_dist_entry15(const double* pi, double ni, const double* pj, double nj)
{
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < 15; ++q) dot = fma(pi[q], pj[q], dot);
    const double nsum = ni + nj;
    double s = fma(-2.0, dot, nsum);
    if (s < 0x1p-20 * nsum) {  // near-identical cells: the difference form
        s = 0.0;
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            const double dv = pi[q] - pj[q];
            s = fma(dv, dv, s);
        }
    }
    return scc_sqrt_nr(s);
}

// The same two over the leading D components only, for rows whose other
// components are zero (scc_knn.hip's `dims`): fma(0, 0, s) is s exactly and
// 0 - 0 is 0, so the steps left out change no bit of the norm or the entry.
template <int D>
__device__ inline double scc_dist_norm_lead(const double* p)
{
    double n = 0.0;
#pragma unroll
    for (int q = 0; q < D; ++q) n = fma(p[q], p[q], n);
    return n;
}

template <int D>
__device__ inline double scc_dist_entry_lead(const double* pi, double ni, const double* pj, double nj)
{
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < D; ++q) dot = fma(pi[q], pj[q], dot);
    const double nsum = ni + nj;
    double s = fma(-2.0, dot, nsum);
    if (s < 0x1p-20 * nsum) {
        s = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const double dv = pi[q] - pj[q];
            s = fma(dv, dv, s);
        }
    }
    return scc_sqrt_nr(s);
}
