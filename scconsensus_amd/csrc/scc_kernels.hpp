// scc_kernels.hpp — internal launcher interface between the runtime
// (scc_runtime.cpp, scc_de.cpp) and the HIP kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#ifndef SCC_DE_FAST  // (same values as include/scc.h)
#define SCC_DE_FAST 0
#define SCC_DE_SLOW 1
#endif
#ifndef SCC_TEST_T
#define SCC_TEST_WILCOX 0
#define SCC_TEST_T 1
#endif
#ifndef SCC_TEST_BIMOD
#define SCC_TEST_BIMOD 2
#endif

#define SCC_ING_HIST_WAVES 16  // waves per ingest histogram workgroup (one partial expm1 sum each)

struct dd;

// The rank stage's work counters (ScRankLaunch::counts, 16 of them) sit
// SCC_CNT_STRIDE ints apart, one 128-B line each: every split workgroup adds
// to several of them per gene, and on one shared line the atomics (and any
// load of a neighbour) queued behind each other in L2.
#define SCC_NCOUNTS 16
#define SCC_CNT_STRIDE 32

// What each counter counts.  Kernels reach them through rk_cnt (scc_rank_dev.hpp),
// the host through read_counts (scc_de.cpp); both index by these names.
enum ScRankCounter {
    RK_CNT_ITEMS0 = 0,          // items of class 0 (small, LDS), + 1: class 1 (medium, LDS), + 2: class 2 (HBM-resident)
    RK_CNT_SPLIT_GENES = 3,     // ranked genes below SPLIT_BIG values: split_genes, filled from the front
    RK_CNT_WAVE_SLOTS = 4,      // slots taken in the wave-bucket list (sbuckets)
    RK_CNT_BUCKET_IDS = 5,      // global bucket ids handed out (rows of hbg)
    RK_CNT_SPLIT_CURSOR = 6,    // the split's work-queue cursor over the ranked genes
    RK_CNT_FAT = 8,             // re-split parents: entries taken in fatbk
    RK_CNT_RESPLIT_CURSOR = 9,  // the workgroup re-split's work-queue cursor over (gene, slice)
    RK_CNT_SEGMENTS = 10,       // re-split segments written to rsseg (in-parent cross terms)
    RK_CNT_FAT_GENES = 11,      // genes with re-split parents: entries of fatg
    RK_CNT_FAT2 = 12,           // second-level re-split parents pushed to fat2 (may pass fat2_cap)
    RK_CNT_BIG_GENES = 13,      // ranked genes of >= SPLIT_BIG values: split_genes, filled from the far end
    RK_CNT_END                  // one past the largest slot in use
};
static_assert(RK_CNT_END <= SCC_NCOUNTS, "a rank work counter past the counts array");

struct ScStatsLaunch {
    const long long* gstart;
    const unsigned long long* keys;
    int G, K;
    const int* n_clu;
    const uint32_t* coff;
    const int* cl_cc;
    double* mean_x;     // [K][G] (slow mode only)
    double* mean_e;     // [K][G] (fast mode only)
    double* var_x;      // [K][G] (fast t test only)
    int mode;           // SCC_DE_FAST: mean of expm1(x); SCC_DE_SLOW: mean of x
    int test;           // SCC_TEST_WILCOX | SCC_TEST_T | SCC_TEST_BIMOD (FAST)
    uint32_t* cnt_pos;  // [K][G]
    uint32_t* cnt_neg;  // [K][G]
    int glo, gn;        // the genes [glo, glo + gn) (a gene shard; nothing else is read downstream)
    // FAST bimod test only, over the values x > 0 of each (cluster, gene): [K][G]
    double* mean_pos;   // their mean (0 when there is none)
    double* m2_pos;     // sum((x - mean_pos)^2), second pass
    double* min_pos;    // their minimum (+Inf when there is none)
    double* max_pos;    // their maximum (-Inf when there is none)
    dd* sum_e;          // [K][G] the undivided double-double sums of expm1(x) (one-vs-rest only; else nullptr)
};

// one unit of rank work: a whole gene (src 0: the ingest's cluster-grouped
// segment) or one value bucket of a split gene (src 1: keys2 / codes2)
struct ScRankItem {
    long long base;
    int n, gene, src, bucket;  // bucket: global bucket id (its cluster histogram row), -1 none
};

struct ScRankLaunch {
    const long long* gstart;
    const unsigned long long* keys;
    int G, K, P, all_pairs;
    const uint32_t* coff;
    const int* cl_cc;
    const uint8_t* flags;  // [P][G] bit0: the pair tests the gene
    int cap_s, cap_m, cap_lds, bucket_target, ntp_max, item_cap;
    int wave_target;       // split: bins are packed into buckets of < 2 * wave_target elements
    int rw_slots;          // wave kernel: tested pairs per gene held in registers, 64 * rw_slots (2, 4, 8 or 16)
    int dbg;               // SCC_RW_DEBUG timing experiments (1: no pair counts, 2: no sort); results invalid
    int bucket_cap;        // capacity of sbuckets / hbg rows
    ScRankItem* sbuckets;  // [bucket_cap] buckets of <= 64 elements (one wave each)
    unsigned int* hbg;     // [bucket_cap][K] per-bucket cluster counts
    int* gene_bk;          // [2 G] first bucket id and bucket count of each split gene
    unsigned long long* gkmin;  // [G] key minimum of a split gene when its range fits 58 bits, else ~0
    ScRankItem* items;     // [3][item_cap]
    int* counts;           // the work counters, one per ScRankCounter name, SCC_CNT_STRIDE ints apart
    uint32_t* gene_tp;     // [G][P] tested pairs of each split gene, p | a << 16 | b << 24 (pair order)
    int* gene_nt;          // [G] their number
    int wv_lo, wv_hi;      // wave kernel launch: genes with wv_lo < tested pairs <= wv_hi
    int wv_base;           // ... and their tested pairs [wv_base, wv_base + 64 * slots)
    int wv_filter;         // 0: one launch holds every gene (no per-bucket class test)
    int rw_mfma;           // K <= 64: the wave buckets' pair counts on the int8 matrix cores (k_rank_mfma16)
    int rw_mfma16;         // the 16 x 16 x 64 form for the genes the slot kernels take (k_rank_mfma16): -1 at K <= 16, 1 at K <= 32, 0 off
    ScRankItem* fatbk;     // [fat_cap] buckets of > 64 distinct values (re-split into sub-buckets)
    int4* fatg;            // [G] {gene, first fatbk entry, parents}: the re-split work units
    int4* rsseg;           // [fat_cap] {gene, first sub-bucket id, sub-buckets}: in-parent cross terms
    int fat_cap;
    int rsw_chunk;         // wave re-split: bucket ids / list slots taken per global atomic
    ScRankItem* fat2;      // [fat2_cap] second re-split level (RK_CNT_FAT2 of them)
    int fat2_cap;
    int rs_level;          // wave re-split launch: 0 reads fatbk, 1 reads fat2
    int rsw_all;           // wave re-split: one launch takes every gene (no split by tested pairs)
    int cross_wave;        // 1: gene-level cross terms by the per-(gene, pair) wave kernel
    int* split_genes;      // [G]
    unsigned long long* keys2;  // [nnz] bucket-ordered keys of split genes
    uint8_t* codes2;            // [nnz]
    uint32_t* gix;              // [2][nnz] index ping-pong of HBM-resident items
    uint32_t* gwin;             // [nnz] key windows of HBM-resident items
    uint8_t* gcode;             // [nnz]
    uint8_t* gsc;               // [nnz]
    long long nnz;
    unsigned long long* accS;   // [P][G] #{x > y}, nonzeros
    unsigned long long* accE;   // [P][G] cross-cluster equal pairs
    unsigned long long* accX;   // [P][G] sum c_a c_b (c_a + c_b) over tie groups
    unsigned long long* accF;   // [K][G] sum c^3 - c over within-cluster runs
    unsigned long long* stamps; // diagnostic phase clocks [item][8] (nullptr normally)
    int stamp_base[3];
    int tp_global;              // items' tested-pair tables in HBM (scc_rank_tables_global)
    char* tp_scr;               // [item workgroups][tp_scr_stride] when tp_global
    size_t tp_scr_stride;
    // the value-order route (nullptr: today's buckets): the dataset's sorted cells
    // and bucket cuts (scc_vorder.hip), the mirror's gene starts and the call's codes
    const uint32_t* vcell;      // [nnz] cell | tie bit << 31
    const uint32_t* vbk_ptr;    // [G + 1]
    const uint32_t* vbk;        // bucket starts inside the gene's segment | fat bit << 31
    const long long* vgptr;     // [G + 1] the mirror's gene starts
    const signed char* code8;   // [N] cluster code of each cell, -1 unkept
    // run rows (value-order route, one k_rank_mfma16<1, true> launch): the bucket
    // kernel adds the cross term inside each run (a gene's buckets within one
    // chunk of the list) and leaves one hbg row per run, at the run's first
    // list slot; k_rank_cross_runs sums over those rows
    int rank_runs;              // 1: run rows, 0: a row per bucket and k_rank_cross
    int rk_grid;                // the bucket kernel's grid: both kernels derive the chunk from it (rk_chunk)
    unsigned int run_bound;     // what a 32-bit accumulator may hold between flushes (tests lower it)
};


struct ScTestLaunch {
    int K, G, P, mode;
    int glo, ghi;          // genes [glo, ghi): a run's gene shard (all genes: 0, G)
    double min_pct, lfc_thr, log_thr;
    const int* n_clu;
    const double* mean_x;
    const double* mean_e;
    const uint32_t* cnt_pos;
    const uint32_t* cnt_neg;
    const unsigned long long* accS;
    const unsigned long long* accE;
    const unsigned long long* accX;
    const unsigned long long* accF;
    int all_pairs;
    int test;              // SCC_TEST_WILCOX | SCC_TEST_T | SCC_TEST_BIMOD
    const double* var_x;   // [K][G] (t test)
    const double* mean_pos;  // [K][G] moments of the values x > 0 (bimod test, ScStatsLaunch)
    const double* m2_pos;
    const double* min_pos;
    const double* max_pos;
    int* err;              // bit 8: t.test would stop ("data are essentially constant");
                           // bit 0x20: the bimod p of a tested cell is NaN (R stops downstream)
    const double* wtab;
    const int* woff;
    double* out_p;
    double* out_lfc;
    double* out_pct1;
    double* out_pct2;
    long long* out_u2;
    long long* out_t;
    uint8_t* out_flags;
};

// ---- one-vs-rest (scc_de_markers): cluster a against every other kept cell ----
// The rank kernel (scc_rank_rest.hip) sorts a gene's nonzeros once and leaves
//   R2[a][g] = sum over the nonzeros i of cluster a of (2 below(i) + n_t(i)),
//   T[g]     = sum over the tie groups of the nonzeros of (n_t^3 - n_t),
// below(i) the nonzeros of ANY cluster strictly below x_i, n_t(i) the size of
// i's tie group.  Twice the midrank sum of cluster a among the nonzeros is
// R2 + nz_a, so 2 (S_a) + E_a = R2 - nz_a^2 (k_rest_test adds the zero group).
struct ScRestRankLaunch {
    const long long* gstart;
    const unsigned long long* keys;
    int G, K, all;              // all: every gene is ranked (test_all)
    const uint32_t* coff;
    const int* cl_cc;
    const uint8_t* flags;       // [K][G] bit0: cluster a tests the gene
    unsigned long long* keys2;  // [nnz] sorted chunks of genes longer than one LDS chunk
    uint8_t* codes2;            // [nnz]
    unsigned long long* accR;   // [K][G]
    unsigned long long* accT;   // [G]
};

struct ScRestTestLaunch {
    int K, G, only_pos, all;
    double min_pct, lfc_thr;
    const int* n_clu;
    const dd* sum_e;            // [K][G] (ScStatsLaunch::sum_e)
    const uint32_t* cnt_pos;
    const uint32_t* cnt_neg;
    const unsigned long long* accR;
    const unsigned long long* accT;
    const double* wtab;
    const int* woff;
    double* out_p;              // all [K][G]
    double* out_lfc;
    double* out_pct1;
    double* out_pct2;
    long long* out_u2;
    long long* out_t;
    uint8_t* out_flags;
};

struct ScSelectLaunch {
    int K, G, P, mode, top_n, cap;
    int plo, phi;          // pairs [plo, phi) (all: 0, P)
    double q_thr, lfc_cut;
    const double* p;
    const double* lfc;
    const double* pct1;
    const double* pct2;
    const long long* u2;
    const long long* t;
    const uint8_t* flags;
    const long long* row_off;
    void* rec_scratch;
    void* key_scratch;
    int* row_gene;
    double* row_p;
    double* row_q;
    double* row_lfc;
    double* row_pct1;
    double* row_pct2;
    long long* row_u2;
    long long* row_t;
    uint8_t* row_flags;
    double* slow_q;
    uint8_t* slow_de;
    unsigned long long* first_occ;
    int* err;
};

extern "C" {
int scc_ingest_gene_tile(void);
hipError_t scc_launch_de_clear(int* err, int* counts, unsigned long long* acc, long long acc_n,
                               unsigned long long* first, int G, int glo, int ghi, hipStream_t st);
int scc_ingest_hist_window(int G);
hipError_t scc_launch_ingest_hist(const long long* indptr, const int* rows, const double* vals, const double* dense,
                                  int G, const int* perm, const int* cc_p0, const int* cc_code, int nc, int ntile,
                                  uint32_t* cnt, long long* bnd, int* nodg, dd* wave_expm1, int want_expm1, int glo,
                                  int ghi, int rng, const long long* tbnd, int* err, hipStream_t st);
hipError_t scc_launch_tile_bounds(const long long* indptr, const int* rows, int N, int gt, int ntile, long long* tbnd,
                                  hipStream_t st);
int scc_ingest_colscan_scratch(int nc, int G);
hipError_t scc_launch_ingest_colscan(uint32_t* cnt, int nc, int nc_kept, int G, int g0, int g1, uint32_t* scratch,
                                     hipStream_t st);
void scc_ingest_count_range(int G, int glo, int ghi, int* g0, int* g1);
hipError_t scc_launch_ingest_scatter(const long long* indptr, const int* rows, const double* vals,
                                     const double* dense, int G, const int* perm, const int* cc_p0, const int* sc_cc0,
                                     int ns, const uint32_t* cnt, const long long* gstart, const long long* bnd,
                                     const long long* tbnd, int ntile, int glo, int ghi, unsigned long long* keys,
                                     hipStream_t st);
// the counting pass of a validated zero-free dataset over all genes (FAST; the
// tile starts come from the dataset's cache, nodg from its cache)
// (a gene shard [glo, ghi) of a validated dataset too: its tiles' entries from tbnd)
hipError_t scc_launch_ingest_count_ro(const long long* indptr, const int* rows, int G, const int* perm,
                                      const int* cc_p0, const int* cc_code, int nc, int glo, int ghi,
                                      const long long* tbnd, uint32_t* cnt, hipStream_t st);
hipError_t scc_launch_scan(const uint32_t* in, long long n, long long* out, long long* bsum_scratch,
                           long long* total, hipStream_t st);
int scc_scan_scratch_blocks(long long n);
// the dataset's gene-major mirror (scc_ingest.hip): built once from the
// validated CSC (cnt: ceil(N / 32) + 1 count rows of G; the
// column scan's and the scan's scratch as for a run of that many chunks),
// then regrouped by cluster at every call (code: int8 per cell, -1 unkept;
// total: kept entries per gene of [glo, ghi) for the scan behind gstart)
// mseg [G][ceil(N / SCC_MIRROR_SEG) + 1] (or nullptr: none): a gene's entries
// before each segment of SCC_MIRROR_SEG cells (the last column: all of them)
#define SCC_MIRROR_SEG 128
hipError_t scc_launch_mirror_build(const long long* indptr, const int* rows, const double* vals, long long nnz, int N,
                                   int G, uint32_t* cnt, uint32_t* colscan_scratch, long long* scan_scratch,
                                   long long* gptr, uint32_t* mcell, unsigned long long* mkey, uint32_t* mseg,
                                   hipStream_t st);
// the PCA panel and its column sums from the mirror (scc_dist.hip): what
// scc_launch_gather and scc_launch_center give for the whole cell range of a
// sparse dataset, read from the union genes' entries alone
hipError_t scc_launch_gather_mirror(const long long* gptr, const uint32_t* mcell, const unsigned long long* mkey,
                                    const uint32_t* mseg, int N, int Npad, const int* genes, int nu, int ld,
                                    double* Xc, hipStream_t st);
hipError_t scc_launch_center_mirror(const long long* gptr, const uint32_t* mcell, const unsigned long long* mkey,
                                    const uint32_t* mseg, double* Xc, int N, int nu, int ld, const int* genes,
                                    dd* part, int nchunk, double* mean, int apply, hipStream_t st);
hipError_t scc_launch_mirror_total(const long long* gptr, const uint32_t* mcell, const signed char* code, int glo,
                                   int ghi, uint32_t* total, hipStream_t st);
hipError_t scc_launch_mirror_regroup(const long long* gptr, const uint32_t* mcell, const unsigned long long* mkey,
                                     const signed char* code, const int* order, int glo, int ghi, int K, int G,
                                     const int* cl_cc, const long long* gstart, uint32_t* cnt,
                                     unsigned long long* keys, hipStream_t st);
// FAST Wilcoxon statistics straight from the mirror (k_mir_stats): mean_e,
// cnt_pos and cnt_neg [K][G] as k_gene_stats<true, false, false> gives them
// after the regroup, bit for bit, for every gene in `order` [G]; K at most
// scc_mirror_stats_max_k().  gstart [G + 1]: the genes' kept entries.
#define SCC_STATS_WAVES 4  // waves of k_gene_stats: they set its piece length, which fixes the summation order
int scc_mirror_stats_max_k(void);
hipError_t scc_launch_mirror_stats(const long long* gptr, const uint32_t* mcell, const unsigned long long* mkey,
                                   const signed char* code, const int* order, int G, int K, const long long* gstart,
                                   const int* n_clu, double* mean_e, uint32_t* cnt_pos, uint32_t* cnt_neg,
                                   hipStream_t st);
// the mirror's value order (scc_vorder.hip): vcell [nnz] each gene's cells in
// ascending key order (bit 31: the key equals the previous entry's), vbk_ptr
// [G + 1] / vbk the genes' bucket cuts (positions in the sorted segment; bit
// 31: one tie group of more than 64 entries).  cnt: [G], bptr: [G + 1], the
// scan's scratch as for G.  *vbk_out is allocated with hipMalloc (the caller
// frees it); left nullptr when the table would pass vbk_max_bytes.  ks_lent
// [ks_n] and tmp_lent: scratch lent to the sort (nullptr: it allocates its own).
hipError_t scc_launch_vorder_build(const long long* gptr, int G, const uint32_t* mcell, const unsigned long long* mkey,
                                   uint32_t* vcell, uint32_t* vbk_ptr, uint32_t** vbk_out, long long* nbk_out,
                                   uint32_t* cnt, long long* bptr, long long* scan_scratch, size_t vbk_max_bytes,
                                   unsigned long long* ks_lent, long long ks_n, void* tmp_lent, size_t tmp_lent_bytes,
                                   hipStream_t st);
// CSR -> CSC transpose (scc_csr.hip): a plan sized on the host from (G, N,
// nnz), one scratch blob, a validating pass, then the two-pass transpose
struct ScCsrPlan {
    long long G, N, nnz;
    int SB, NS;      // cells per superblock, superblocks
    int T;           // gene tiles of 256
    int CG, NG;      // cells per output group, groups
    size_t off_bnd, off_rs, off_tt, off_ts, off_off, off_gm, off_gb, off_scan, off_meta, off_ival, bytes;
};
int scc_csr_plan(long long G, long long N, long long nnz, ScCsrPlan* P);
// validation (columns in [0, N), strictly ascending per gene) + superblock bounds
hipError_t scc_launch_csr_check(const ScCsrPlan* P, const long long* indptr, const int* cols, void* scratch,
                                int* err, hipStream_t st);
hipError_t scc_launch_csr_to_csc(const ScCsrPlan* P, const long long* indptr, const int* cols, const double* vals,
                                 void* scratch, long long* csc_indptr, int* csc_rows, double* csc_vals,
                                 hipStream_t st);
hipError_t scc_launch_reduce_dd(const dd* parts, int n, dd* out, hipStream_t st);

hipError_t scc_launch_gene_stats(const ScStatsLaunch* L, hipStream_t st);
hipError_t scc_launch_rank_classify(const ScRankLaunch* L, hipStream_t st);
size_t scc_rank_item_lds(int cls, int cap, int ntp_max, int K);
int scc_rank_item_cap(int cls, int want, int ntp_max, int K, int lim);
size_t scc_rank_split_lds(int K);
int scc_rank_tables_global(int ntp_max, int K);
size_t scc_rank_tables_stride(int ntp_max, int K);
hipError_t scc_launch_rank_split(const ScRankLaunch* L, int grid, hipStream_t st);
hipError_t scc_launch_rank_items(const ScRankLaunch* L, int cls, int grid, hipStream_t st);
// the value-order route (L->vcell set): the classified genes' precomputed buckets
// into the wave list; scc_launch_rank_waves then runs the VORD kernels over them
hipError_t scc_launch_rank_vorder_list(const ScRankLaunch* L, int grid, hipStream_t st);
// the slot classes' launches go round st, side[0], side[1], ... (nside 0: all
// on st); a side stream is forked from st (event fork) when it first gets a
// launch and joined back (its event in join[]) at the end
hipError_t scc_launch_rank_waves(const ScRankLaunch* L, int grid, hipStream_t st, const hipStream_t* side = nullptr,
                                 int nside = 0, hipEvent_t fork = nullptr, const hipEvent_t* join = nullptr);
void scc_rank_mfma_stamps(hipStream_t st, int print);
hipError_t scc_launch_rank_cross(const ScRankLaunch* L, int grid_genes, hipStream_t st);
hipError_t scc_launch_rank_resplit(const ScRankLaunch* L, int grid, hipStream_t st, const hipStream_t* side = nullptr,
                                   int nside = 0, hipEvent_t fork = nullptr, const hipEvent_t* join = nullptr);
hipError_t scc_launch_rank_cross_seg(const ScRankLaunch* L, int grid, hipStream_t st);
hipError_t scc_launch_pair_filter(const ScTestLaunch* L, hipStream_t st);
hipError_t scc_launch_rest_filter(const ScRestTestLaunch* L, hipStream_t st);
hipError_t scc_launch_rest_test(const ScRestTestLaunch* L, hipStream_t st);
hipError_t scc_launch_rank_rest(const ScRestRankLaunch* L, hipStream_t st);
size_t scc_eigen_scratch_doubles(int n, int lda, int k);
hipError_t scc_launch_eigen_topk(const double* A, int n, int lda, int k, double* scratch, double* Z, double* W,
                                 unsigned int** err_dev, int* nwg_out, hipEvent_t* marks,
                                 unsigned long long* stamps, unsigned long long key, hipStream_t st);

hipError_t scc_launch_wilcox_table(double* W, const int* woff, int mmax, hipStream_t st);
int scc_wilcox_table_layout(int* woff);
hipError_t scc_launch_pair_test(const ScTestLaunch* L, hipStream_t st);
hipError_t scc_launch_count_tested(const uint8_t* flags, int G, int P, int* tested, long long* row_off,
                                   hipStream_t st);
size_t scc_select_lds_bytes(int cap);
size_t scc_select_rec_bytes(void);
size_t scc_select_key_bytes(void);
hipError_t scc_launch_pair_select(const ScSelectLaunch* L, hipStream_t st);
hipError_t scc_launch_union(const unsigned long long* first_occ, int G, void* scratch, int cap, int* out,
                            int* n_out, hipStream_t st);
hipError_t scc_launch_flag_copy(const unsigned int* src, unsigned int* dst_dev, hipStream_t st);
hipError_t scc_launch_stage_pack(const int* nu, const int* err, const long long* nrows, const int* tested, int P,
                                 const int* uni, int G, int* out_dev, hipStream_t st);
hipError_t scc_launch_seg_copy(const void* src, void* dst, int elem_bytes, const long long* seg, long long nseg,
                               hipStream_t st);
hipError_t scc_launch_row_hist(const int* rows, long long nnz, int G, unsigned int* cnt, hipStream_t st);
hipError_t scc_launch_first_remap(const unsigned long long* local, int G, const long long* lp2gp,
                                  unsigned long long* global, hipStream_t st);
}

// ---- device hclust (scc_hclust.hip) -----------------------------------------
// The NN-chain's state between two launches of one call (device memory).
#define SCC_HC_ERR_CAP 1    // a loop cap was passed (one extension: n scans; one call: 3 n scans)
#define SCC_HC_ERR_STATE 2  // the state or the chain holds an index out of range
struct scc_hc_state {
    int start;  // lowest active node
    int tip;    // chain length
    int step;   // merges done
    int err;    // SCC_HC_ERR_*: every later launch returns at once
    long long scans;  // nearest-neighbour scans so far
};
extern "C" {
hipError_t scc_launch_hc_init(int N, scc_hc_state* S, double* size, uint8_t* act, unsigned int* nonfinite,
                              hipStream_t st);
hipError_t scc_launch_hc_expand(const void* P, int f32, int N, double* D, unsigned int* nonfinite, hipStream_t st);
hipError_t scc_launch_hc_chain(double* D, int N, scc_hc_state* S, int* chain, double* size, uint8_t* act, int* out_a,
                               int* out_b, double* out_h, int max_merges, hipStream_t st);
hipError_t scc_launch_hc_gather_core(const void* P, int f32, int N, const int* core, int cs, double* block,
                                     hipStream_t st);
}

// ---- hclust from the scores (scc_hclust_vec.hip) -----------------------------
// The centroid NN-chain's state between two launches (device memory): the
// scalars of scc_hc_state, then what one scan hands to the next.
struct scc_wv_state {
    int start;  // lowest active node
    int tip;    // chain length
    int step;   // merges done
    int err;    // SCC_HC_ERR_*: every later launch returns at once
    long long scans;  // nearest-neighbour scans so far
    int node;   // the node the next scan reads
    int mode;   // 0: that scan restarts the chain from `start`; 1: it extends the chain
    int i1;     // the node before the tip (the carried nearest neighbour)
    int ext;    // scans of this chain extension
    double mn;  // the carried minimum
};
extern "C" {
int scc_wv_scan_workgroups(int N);  // partials of one scan
hipError_t scc_launch_wv_init(const double* P, int N, double* C, scc_wv_state* S, double* size, uint8_t* act,
                              unsigned int* nonfinite, hipStream_t st);
hipError_t scc_launch_wv_scan(const double* C, int N, const scc_wv_state* S, const double* size, const uint8_t* act,
                              double* part_v, int* part_i, hipStream_t st);
hipError_t scc_launch_wv_advance(double* C, int N, scc_wv_state* S, int* chain, double* size, uint8_t* act,
                                 const double* part_v, const int* part_i, int* out_a, int* out_b, double* out_h,
                                 hipStream_t st);
hipError_t scc_launch_wv_gather_core(const double* P, int N, const int* core, int cs, double* block, hipStream_t st);
}

// ---- heatmap inputs (scc_heatmap.hip) -----------------------------------------
// All read the gathered panel Xc [Npad][ld] of scc_launch_gather.
extern "C" {
int scc_gene_dist_slabs(int Npad, int ld);             // cell slabs of one call
size_t scc_gene_dist_slab_doubles(int Npad, int ld);   // their scratch
// out: device, packed R `dist` order, nu (nu - 1) / 2 doubles
hipError_t scc_launch_gene_dist(const double* Xc, int Npad, int nu, int ld, double* slabs, double* out,
                                hipStream_t st);
size_t scc_hm_range_scratch_bytes(void);
// out: {min x, max x, min |x|, max |x|} over rows [0, N), columns [0, nu); nbad: non-finite values
hipError_t scc_launch_hm_range(const double* Xc, int N, int nu, int ld, void* scratch, double* out,
                               unsigned int* nbad, hipStream_t st);
// R [width][nu]: bin means over cell[floor(b N / width) .. floor((b + 1) N / width)) (0-based ids)
hipError_t scc_launch_heatmap_raster(const double* Xc, int N, int nu, int ld, const int* cell, int width, double* R,
                                     hipStream_t st);
}
