// scc_stats.hip — per-gene, per-cluster statistics of the cluster-grouped nonzeros.
//
// Replaces the reference's per-cluster log-mean / detection statistics
// (R/reclusterDEConsensusFast.R:229-271, R/reclusterDEConsensus.R:104-113).
//   k_gene_stats   one workgroup per gene: per-cluster double-double sums of
//                  x and expm1(x), counts of x > 0 and x < 0, fixed reduction
//                  order (bitwise deterministic).  Seven instances: FAST,
//                  SLOW, the t test's two passes, the bimod test's two passes
//                  over the values x > 0, and one-vs-rest's undivided sums.
//   scc_launch_gene_stats picks the instances by mode and test.
// k_mir_stats (scc_ingest.hip) computes the same numbers straight from the
// gene-major mirror and repeats this kernel's pieces: the static_assert below
// keeps their wave counts equal.
#include "scc_common.hpp"
#include "scc_kernels.hpp"

#define ST_T 256
#define ST_W (ST_T / 64)
static_assert(ST_W == SCC_STATS_WAVES, "k_mir_stats (scc_ingest.hip) repeats k_gene_stats' pieces");
#ifndef ST_U
#define ST_U 4
#endif

struct StatItem {
    double sx_hi, sx_lo, se_hi, se_lo;
    u32 pos, neg;
};

// FAST needs the per-cluster mean of expm1(x) (Fast:259-272), SLOW the mean
// of x (slow:105), the FAST t test (DiffTTest, Fast:185-196) both plus, in a
// second pass (VAR), R's two-pass variance sum((x - mean)^2) / (n - 1) over
// the cluster, zeros included.  Each pass accumulates only its own
// double-double sums.
//
// The FAST bimod test (DifferentialLRT, Fast:93-133) models the values x > 0 of
// a cluster alone (POS): its first pass sums them instead of every x and keeps
// their minimum and maximum (bitwise equal when they are all the same value:
// R's sd is 0 there, which no computed variance decides reliably); its second
// pass (POS && VAR) sums (x - mean_pos)^2 over them, zeros and negatives left
// out, undivided.
struct StatMinMax {
    double mn, mx;
};

// minimum / maximum over the wave, every lane the same value (whole wave only)
template <bool MAX>
__device__ inline double f64_wave_ext_dpp(double x)
{
    auto ext = [](double a, double b) { return MAX ? fmax(a, b) : fmin(a, b); };
    x = ext(x, scc_xor_lane_f64<32>(x));
    x = ext(x, scc_xor_lane_f64<16>(x));
    x = ext(x, scc_xor_lane_f64<8>(x));
    x = ext(x, scc_xor_lane_f64<4>(x));
    x = ext(x, scc_xor_lane_f64<2>(x));
    return ext(x, scc_xor_lane_f64<1>(x));
}

#define ST_NITEM (SCC_MAX_K + ST_W + 4)
static_assert(sizeof(int) * (SCC_MAX_K + 1) + (sizeof(StatItem) + sizeof(StatMinMax)) * ST_NITEM <= 16 * 1024,
              "k_gene_stats: static LDS (off[], item[], mm[]) beyond 16 KiB a workgroup");

template <bool EXPM1, bool SUMX, bool VAR, bool POS = false, bool SUME = false>
__global__ void __launch_bounds__(ST_T) k_gene_stats(ScStatsLaunch A)
{
    __shared__ int off[SCC_MAX_K + 1];
    __shared__ StatItem item[ST_NITEM];
    __shared__ StatMinMax mm[POS && !VAR ? ST_NITEM : 1];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const int g = A.glo + blockIdx.x, K = A.K, tid = threadIdx.x, lane = tid & 63, w = scc_wave_id();
    const i64 base = A.gstart[g];
    const int n = (int)(A.gstart[g + 1] - base);
    const u64* key = A.keys + base;
    if (tid <= K) off[tid] = (int)A.coff[(size_t)A.cl_cc[tid] * A.G + g];
    __syncthreads();
    // balanced pieces that never straddle clusters, combined in a fixed order
    const int Lp = max(64, (((n + ST_W - 1) / ST_W) + 63) & ~63);
    for (int it = w;; it += ST_W) {
        int a = 0, acc = 0, ni = 0;
        for (; a < K; ++a) {
            ni = (off[a + 1] - off[a] + Lp - 1) / Lp;
            if (it < acc + ni) break;
            acc += ni;
        }
        if (a == K) break;
        const int s0 = off[a] + (it - acc) * Lp, s1 = min(off[a + 1], s0 + Lp);
        const double ma = VAR ? (POS ? A.mean_pos : A.mean_x)[(size_t)a * A.G + g] : 0.0;
        dd sx{0.0, 0.0}, se{0.0, 0.0};
        u32 pos = 0, neg = 0;
        double mn = inf, mx = -inf;  // POS: over the values > 0
        // ST_U loads in flight per lane (16 measured slower: B 0.18 -> 0.28 ms,
        // D 2.06 -> 2.75: the stage is VALU-bound on fp64 expm1 + double-double
        // adds, and the wider unroll cost occupancy); the per-lane summation
        // order (i, i + 64, i + 128, ...) does not depend on ST_U
        for (int i = s0 + lane; i < s1; i += 64 * ST_U) {
            double x[ST_U];  // past the end adds +0 (exact no-op)
#pragma unroll
            for (int q = 0; q < ST_U; ++q) {  // clamped unconditional load + select (i < s1)
                const double v = scc_val_of(key[min(i + 64 * q, s1 - 1)]);
                x[q] = (i + 64 * q < s1) ? v : 0.0;
            }
#pragma unroll
            for (int q = 0; q < ST_U; ++q) {
                if (EXPM1) se = dd_add_d(se, expm1(x[q]));
                if (SUMX) sx = dd_add_d(sx, x[q]);
                if (VAR && !POS && i + 64 * q < s1) sx = dd_add(sx, dd_two_prod(x[q] - ma, x[q] - ma));
                if (POS && !VAR) {  // (past the end x is 0: not a positive value)
                    sx = dd_add_d(sx, x[q] > 0.0 ? x[q] : 0.0);
                    mn = x[q] > 0.0 ? fmin(mn, x[q]) : mn;
                    mx = x[q] > 0.0 ? fmax(mx, x[q]) : mx;
                }
                if (POS && VAR && x[q] > 0.0) sx = dd_add(sx, dd_two_prod(x[q] - ma, x[q] - ma));
                pos += (x[q] > 0.0);
                neg += (x[q] < 0.0);
            }
        }
        if (EXPM1) se = dd_wave_sum_dpp(se);
        if (SUMX || VAR || POS) sx = dd_wave_sum_dpp(sx);
        pos = u32_wave_sum_dpp(pos);
        neg = u32_wave_sum_dpp(neg);
        if (POS && !VAR) {
            mn = f64_wave_ext_dpp<false>(mn);
            mx = f64_wave_ext_dpp<true>(mx);
            if (lane == 0) mm[it] = StatMinMax{mn, mx};
        }
        if (lane == 0) item[it] = StatItem{sx.hi, sx.lo, se.hi, se.lo, pos, neg};
    }
    __syncthreads();
    if (tid < K) {
        const int a = tid;
        int first = 0;
        for (int b = 0; b < a; ++b) first += (off[b + 1] - off[b] + Lp - 1) / Lp;
        const int ni = (off[a + 1] - off[a] + Lp - 1) / Lp;
        dd sx{0.0, 0.0}, se{0.0, 0.0};
        u32 pos = 0, neg = 0;
        double mn = inf, mx = -inf;
        for (int q = first; q < first + ni; ++q) {
            sx = dd_add(sx, dd{item[q].sx_hi, item[q].sx_lo});
            se = dd_add(se, dd{item[q].se_hi, item[q].se_lo});
            pos += item[q].pos;
            neg += item[q].neg;
            if (POS && !VAR) {
                mn = fmin(mn, mm[q].mn);
                mx = fmax(mx, mm[q].mx);
            }
        }
        const double na = (double)A.n_clu[a];
        if (POS && VAR) {  // the positive part's sum of squared deviations (undivided)
            A.m2_pos[(size_t)a * A.G + g] = sx.hi + sx.lo;
            return;
        }
        if (POS) {
            A.mean_pos[(size_t)a * A.G + g] = pos ? dd_div_n(sx, (double)pos) : 0.0;
            A.min_pos[(size_t)a * A.G + g] = mn;
            A.max_pos[(size_t)a * A.G + g] = mx;
        }
        if (VAR) {  // + the zeros' (0 - mean)^2, then / (n - 1)
            const double m = A.mean_x[(size_t)a * A.G + g];
            const double z = na - (double)A.cnt_pos[(size_t)a * A.G + g] - (double)A.cnt_neg[(size_t)a * A.G + g];
            sx = dd_add(sx, dd_mul_d(dd_two_prod(m, m), z));
            A.var_x[(size_t)a * A.G + g] = dd_div_n(sx, na - 1.0);
            return;
        }
        if (EXPM1) A.mean_e[(size_t)a * A.G + g] = dd_div_n(se, na);
        if (SUME) A.sum_e[(size_t)a * A.G + g] = se;  // one-vs-rest (an instance of its own): the rest's mean divides a sum of these
        if (SUMX) A.mean_x[(size_t)a * A.G + g] = dd_div_n(sx, na);
        A.cnt_pos[(size_t)a * A.G + g] = pos;
        A.cnt_neg[(size_t)a * A.G + g] = neg;
    }
}

extern "C" hipError_t scc_launch_gene_stats(const ScStatsLaunch* L, hipStream_t st)
{
    if (L->G <= 0 || L->gn <= 0 || L->glo < 0 || L->glo + L->gn > L->G) return hipSuccess;
    const dim3 grid(L->gn);
    if (L->mode == SCC_DE_FAST && L->test == SCC_TEST_BIMOD) {
        hipLaunchKernelGGL((k_gene_stats<true, false, false, true>), grid, dim3(ST_T), 0, st, *L);
        hipLaunchKernelGGL((k_gene_stats<false, false, true, true>), grid, dim3(ST_T), 0, st, *L);
    } else if (L->mode == SCC_DE_FAST && L->test == SCC_TEST_T) {
        hipLaunchKernelGGL((k_gene_stats<true, true, false>), grid, dim3(ST_T), 0, st, *L);
        hipLaunchKernelGGL((k_gene_stats<false, false, true>), grid, dim3(ST_T), 0, st, *L);
    } else if (L->mode == SCC_DE_FAST && L->sum_e) {
        hipLaunchKernelGGL((k_gene_stats<true, false, false, false, true>), grid, dim3(ST_T), 0, st, *L);
    } else if (L->mode == SCC_DE_FAST) {
        hipLaunchKernelGGL((k_gene_stats<true, false, false>), grid, dim3(ST_T), 0, st, *L);
    } else {
        hipLaunchKernelGGL((k_gene_stats<false, true, false>), grid, dim3(ST_T), 0, st, *L);
    }
    return hipGetLastError();
}
