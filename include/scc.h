/*
 * scc.h — C ABI of the MI355X scConsensus engine (libscc.so).
 *
 * Drop-in boundary for the data-parallel core of the reference R package
 * (bbbranjan/scConsensus).  The reference has no native code and no FFI
 * (NAMESPACE:3-6 has no useDynLib); these entry points are what its R
 * functions bind through `.Call` (see INTEGRATION.md for the R glue):
 *
 *   reclusterDEConsensusFast()  R/reclusterDEConsensusFast.R:22-33
 *       pair loop + ComputePairWiseDE + union      :57-392  -> scc_de_run(SCC_DE_FAST)
 *       prcomp_irlba + dist                         :398-400 -> scc_distance(SCC_DIST_PCA_EUCLID)
 *       `1 - cor(...)` (commented alternative)      :403     -> scc_distance(SCC_DIST_PEARSON)
 *       nodg loop                                   :440-443 -> scc_de_result_nodg
 *       cellTypeDEPlot's Heatmap inputs             :456-464 -> scc_gene_distance, scc_hclust_complete,
 *                                                               scc_dendro_reorder, scc_heatmap_raster
 *   reclusterDEConsensus()      R/reclusterDEConsensus.R:20-29
 *       global threshold + pair loop + union        :32-227  -> scc_de_run(SCC_DE_SLOW)
 *       prcomp_irlba + dist                         :234-236 -> scc_distance(SCC_DIST_PCA_EUCLID)
 *
 * Conventions: plain pointers and sizes, no C++ types, int status returns
 * (SCC_OK == 0), no exceptions or longjmp across the ABI.  Inputs are borrowed
 * read-only; the caller owns every output buffer.  Cluster selection (R's
 * table()/grepl("grey")/locale order, Fast:40-53) stays in the caller, which
 * passes integer codes: code[c] in [0, K) in the reference's cluster order,
 * or -1 for cells whose cluster is not compared.  Pairs are (i<j) in the
 * reference's nested-loop order: p = i*K - i*(i+1)/2 + (j-i-1).
 */
#ifndef SCC_H
#define SCC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define SCC_API __attribute__((visibility("default")))
#else
#define SCC_API
#endif

#define SCC_OK 0
#define SCC_ERR_INVALID 1     /* bad argument / shape */
#define SCC_ERR_HIP 2         /* HIP runtime error (no device, launch failure) */
#define SCC_ERR_OOM 3         /* device allocation failed */
#define SCC_ERR_NONFINITE 4   /* input holds NaN/Inf or out-of-range row index */
#define SCC_ERR_RSTOP 5       /* the reference R code would stop() on this input */
#define SCC_ERR_UNSUPPORTED 6 /* valid input outside this build's limits (e.g. ncomp > 16) */

#define SCC_DE_FAST 0 /* reclusterDEConsensusFast(method = "wilcox") */
#define SCC_DE_SLOW 1 /* reclusterDEConsensus(method = "Wilcoxon") */
#define SCC_TEST_WILCOX 0 /* FAST test.use = "wilcox" (WilcoxDETest, Fast:78-91) */
#define SCC_TEST_T 1      /* FAST test.use = "t" (DiffTTest: Welch t.test, Fast:185-196) */
#define SCC_TEST_BIMOD 2  /* FAST test.use = "bimod" (DiffExpTest: McDavid's zero-inflated LRT, Fast:93-133) */
/* test.use = "roc" has no defined result (the caller filters on p_val_adj, which
 * the roc branch never produces, Fast:343-351,377) and is not offered.
 *
 * SCC_TEST_BIMOD, per tested (pair, gene): for a group of n cells with the
 * n2 values x2 = x[x > 0] (zeros and negative values are the other part, n1),
 *   xal = min(max(n2 / n, 1e-5), 1 - 1e-5)
 *   sd  = 1 if n2 < 2, else sd(x2) (two-pass, divisor n2 - 1)
 *   lik = n1 log(1 - xal) + n2 log(xal) + sum(dnorm(x2, mean(x2), sd, log = TRUE))
 *   lrt = 2 (lik(x) + lik(y) - lik(c(x, y)));  p = pchisq(lrt, df = 3, lower.tail = FALSE)
 * from per-(gene, cluster) moments of the values > 0 (count, mean, two-pass sum
 * of squared deviations, minimum, maximum); the pooled group's by Chan's merge.
 * R's IEEE cases are decided explicitly, not left to rounding:
 *   - n2 >= 2 values that are all equal (minimum == maximum bitwise): sd = 0,
 *     dnorm(x, x, 0, log = TRUE) = +Inf, lik = +Inf;
 *   - lrt <= 0 (-Inf included): p = 1;  lrt = +Inf: p = 0;
 *   - lrt = Inf - Inf = NaN: p = NaN.  R turns it into an NA p_val_adj, an
 *     all-NA marker row, an NA in deGeneUnion, and stops at
 *     dataMatrix[deGeneUnion, ]: the run fails with SCC_ERR_RSTOP, for cells
 *     the pair tests only (cells computed because test_all is set never fail
 *     a run).  One deviation: R does not stop when the affected pair has that
 *     single tested row (a pair with <= 1 row contributes nothing, Fast:376);
 *     the engine stops there as well.
 * u2 and ties are 0, as for SCC_TEST_T; the feature filters, BH, top_n and the
 * union do not depend on the test. */

#define SCC_DIST_PCA_EUCLID 0 /* dist(prcomp_irlba(t(X[U,]), n=min(|U|,15))$x) */
#define SCC_DIST_PEARSON 1    /* as.dist(1 - cor(X[U,], method = "pearson")) */

#define SCC_PTR_HOST 0   /* pointers are host memory (copied H2D by the engine) */
#define SCC_PTR_DEVICE 1 /* pointers are device memory of the context's device */

typedef struct scc_ctx scc_ctx;
typedef struct scc_dataset scc_dataset;
typedef struct scc_de_result scc_de_result;

typedef struct {
    int32_t device;      /* HIP device ordinal (the context's only device when n_devices <= 1) */
    int32_t profile;     /* 1: time the dominant kernels with HIP events */
    int32_t n_devices;   /* > 1: ONE job over the devices devices[0 .. n_devices) (SURVEY 8b's device
                            list; replaces the reference's nCores PSOCK workers, Fast:61-65,384) */
    int32_t reserved[5];
    const int32_t* devices; /* n_devices HIP ordinals, devices[0] the primary (a repeated ordinal runs
                               several engines on one device: the sharded path on one GPU) */
} scc_opts;

typedef struct {
    int32_t mode;               /* SCC_DE_FAST | SCC_DE_SLOW */
    int32_t top_n;              /* FAST: NumbertopDEGenes (Fast:32); SLOW: 30 (slow:218) */
    double q_val_thrs;          /* qValThrs */
    double log_fc_thrs;         /* FAST: logFCThrs, natural log (Fast:26) */
    double min_per_cent;        /* FAST: minPerCent (Fast:29) */
    double fc_thrs;             /* SLOW: fcThrs, compared as log(fcThrs) (slow:167) */
    double mean_scaling_factor; /* SLOW: meanScalingFactor (slow:23) */
    int32_t test_all;           /* FAST: 1 = also compute U / p for the (pair, gene) cells the
                                   feature filters drop (diagnostics; R never tests them) */
    int32_t test;               /* FAST: SCC_TEST_WILCOX (default) | SCC_TEST_T | SCC_TEST_BIMOD; u2 / ties
                                   are 0 for t and bimod.  SLOW takes SCC_TEST_WILCOX only */
} scc_de_params;

/* ---- context ---------------------------------------------------------- */
/* With a device list (opts.n_devices > 1) the context drives every device of
 * the list from this one host process (one host thread per device inside
 * each call; peer copies over xGMI between them):
 *   scc_dataset_create_*  uploads to devices[0] and replicates the matrix on
 *                         the others (peer copies; a repeated ordinal shares it)
 *   scc_de_run            gene row-blocks balanced by stored values, one per
 *                         device, their tested-cell records gathered on
 *                         devices[0], which runs the per-pair selection: the
 *                         result equals the one-device run bit for bit
 *                         (K > 128: every group-pair run is sharded this way)
 *   scc_distance(_cols)   the PCA on devices[0], its N x 16 scores copied to
 *                         every device, each device the packed columns of an
 *                         equal share of the entries, streamed straight to
 *                         the caller's host buffer or copied into its device
 *                         buffer (bit for bit the one-device output; the
 *                         Pearson metric runs on devices[0] only)
 * Every other entry point works on devices[0].  Results and outputs live on
 * devices[0]. */
SCC_API int scc_ctx_create(const scc_opts* opts, scc_ctx** out);
/* number of visible HIP devices (0 when none) */
SCC_API int scc_device_count(int32_t* n);
SCC_API void scc_ctx_destroy(scc_ctx* ctx);
SCC_API const char* scc_ctx_last_error(const scc_ctx* ctx);
SCC_API int scc_ctx_synchronize(scc_ctx* ctx);
/* Launch the engine's work on the caller's stream (a hipStream_t of the
 * context's device; external = 1, the legacy default stream NULL included)
 * instead of its own non-blocking one (external = 0: back to its own).  A
 * caller whose buffers come from a framework stream (torch) then needs no host
 * synchronisation between its own work, its collectives and the engine. */
SCC_API int scc_ctx_set_stream(scc_ctx* ctx, void* stream, int32_t external);
/* Kernel timing (opts.profile = 1): total ms and launch count of a named
 * kernel family since the last reset ("gene_rank", "dist", "gram", ...). */
SCC_API int scc_ctx_kernel_time(const scc_ctx* ctx, const char* name, double* total_ms, int64_t* launches);
SCC_API void scc_ctx_reset_timers(scc_ctx* ctx);

/* ---- dataset: the genes x cells matrix as R holds it ------------------- */
/* dgCMatrix (CSC over cells): indptr[N+1] (R @p), rows[nnz] (R @i, 0-based
 * gene rows), vals[nnz] (R @x).  Replaces as.matrix(dataMatrix) (Fast:368).
 * SCC_PTR_HOST copies the arrays; SCC_PTR_DEVICE borrows them, and their
 * contents must not change while the dataset lives: the first error-free DE
 * run that reads every entry marks the dataset validated (rows in range and
 * sorted) and caches nodg, and later gene-shard runs read only their genes.
 * The first FAST run after that (the dataset's second DE call) also builds a
 * gene-major mirror of the kept entries on the device, 12 bytes per stored
 * value, held until scc_dataset_destroy: later FAST runs regroup it by the
 * call's clusters instead of transposing the matrix again (same results).
 * It is built only while it needs at most a quarter of the free device
 * memory; otherwise, and with SCC_INGEST_MIRROR=0, the per-call transpose
 * stays. */
SCC_API int scc_dataset_create_csc(scc_ctx* ctx, const int64_t* indptr, const int32_t* rows, const double* vals,
                           int64_t n_genes, int64_t n_cells, int64_t nnz, int32_t ptr_kind,
                           scc_dataset** out);
/* Gene-major CSR (genes x cells; per gene ascending cell columns, e.g. a
 * scipy csr_matrix or an AnnData .X transposed; BASELINE config E's CSR
 * input): indptr[G+1], cols[nnz] (0-based cells), vals[nnz].  Transposed once
 * on the device into the resident CSC over cells above (the dgCMatrix R
 * would hold for the same matrix), so every result equals the CSC path's.
 * Column indices outside [0, N), or not strictly ascending within a gene
 * (unsorted, or a repeated (gene, cell)), fail with SCC_ERR_INVALID here;
 * more than 262,144 genes with SCC_ERR_UNSUPPORTED.  No
 * reference interface: the reference takes dataMatrix as an R matrix
 * (Fast:22, :368); this is the R-free caller's equivalent. */
SCC_API int scc_dataset_create_csr(scc_ctx* ctx, const int64_t* indptr, const int32_t* cols, const double* vals,
                           int64_t n_genes, int64_t n_cells, int64_t nnz, int32_t ptr_kind,
                           scc_dataset** out);
/* base R matrix: G x N column-major doubles (slow:32 as.matrix). */
SCC_API int scc_dataset_create_dense(scc_ctx* ctx, const double* x_colmajor, int64_t n_genes, int64_t n_cells,
                             int32_t ptr_kind, scc_dataset** out);
/* Destroy every dataset before the context it was created on. */
SCC_API void scc_dataset_destroy(scc_dataset* ds);
/* Copy a sparse dataset's resident dgCMatrix (indptr[N+1], rows[nnz],
 * vals[nnz]) to host arrays: what the CSR transpose built, for checks and
 * for callers that want the CSC back (rows = vals = NULL: indptr only).  No
 * reference interface (the R side already holds its matrix). */
SCC_API int scc_dataset_read_csc(scc_dataset* ds, int64_t* indptr, int32_t* rows, double* vals);

/* ---- stage 1+2: per-cluster statistics, all-pairs Wilcoxon, BH, union --- */
SCC_API int scc_de_run(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */, int32_t K,
               const scc_de_params* params, scc_de_result** out);

/* ---- the same DE sharded over gene row-blocks (one process per GPU) -------
 * Replaces the reference's per-cluster foreach workers (Fast:61-65,359,384):
 * every rank holds the whole dataset and runs scc_de_run_shard on its genes
 * [gene_lo, gene_hi); `shard` (device, scc_de_shard_bytes) receives the
 * per-(pair, gene) cells p, avg_logFC, pct1, pct2 (f64), 2U, ties (i64) and
 * flags (u8), each [n_pairs][G], zero outside the shard.  The caller sums the
 * shards of all ranks as int64 words (one all-reduce: the shards are
 * disjoint, so the sum is the exact union) and calls scc_de_finish on the
 * same context with the sum: per-pair BH, filters, top-N and the union, the
 * same result scc_de_run gives. */
SCC_API int64_t scc_de_shard_bytes(int32_t K, int64_t n_genes);
SCC_API int scc_de_run_shard(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */, int32_t K,
                     const scc_de_params* params, int64_t gene_lo, int64_t gene_hi, void* shard /* device */);
SCC_API int scc_de_finish(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */, int32_t K,
                  const scc_de_params* params, const void* shards_sum /* device */, scc_de_result** out);
/* The compact exchange (gather of per-(pair, tested gene)
 * records): scc_de_run_shard_records runs the shard's per-(pair, gene) stage
 * like scc_de_run_shard and packs, in (pair, gene) order, one scc_de_record per
 * cell the pair tests (FAST: the cells that pass the feature filters; SLOW:
 * every cell) into `records` (device, capacity `cap` records; cap >=
 * n_pairs * (gene_hi - gene_lo) always suffices), *n_records = the count.
 * The caller gathers every rank's records (block r = rank r's, stride
 * `stride` records apart, counts[r] valid) and calls scc_de_finish_records on
 * the same context: the result equals scc_de_run's. */
typedef struct {
    int32_t pair, gene;
    double p, avg_logfc, pct1, pct2;
    int64_t u2, ties;
    uint32_t flags, reserved;
} scc_de_record; /* 64 bytes */
SCC_API int scc_de_run_shard_records(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */,
                                     int32_t K, const scc_de_params* params, int64_t gene_lo, int64_t gene_hi,
                                     void* records /* device */, int64_t cap, int64_t* n_records);
SCC_API int scc_de_finish_records(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */, int32_t K,
                                  const scc_de_params* params, const void* records /* device */,
                                  const int64_t* counts /* host [n_blocks] */, int32_t n_blocks, int64_t stride,
                                  scc_de_result** out);
/* The per-pair selection of a FAST job split over the ranks by PAIRS (each
 * rank the pairs [pair_lo, pair_hi); the pairs are independent until the
 * union, Fast:359-392): scatters the gathered records like
 * scc_de_finish_records, runs BH / filters / top_n for its pairs only and
 * writes the first-occurrence key of every gene (u64 [G], device: pair-major
 * order key, all ones = not selected; ordered by (pair, rank in the pair)).
 * The caller combines the ranks' arrays by an element-wise MIN (all-reduce)
 * and scc_de_union_first_occ turns the combined array into deGeneUnion in
 * the reference's order (unique() over the pairs' top lists, Fast:392): the
 * same union scc_de_finish_records returns.  No result object. */
SCC_API int scc_de_finish_records_pairs(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */,
                                        int32_t K, const scc_de_params* params, const void* records /* device */,
                                        const int64_t* counts /* host [n_blocks] */, int32_t n_blocks, int64_t stride,
                                        int32_t pair_lo, int32_t pair_hi, void* first_occ /* device u64 [G] */);
SCC_API int scc_de_union_first_occ(scc_ctx* ctx, const void* first_occ /* device u64 [G] */, int64_t n_genes,
                                   int32_t* genes /* host [G] */, int32_t* n_union);

/* n_pairs = K(K-1)/2; n_rows = FAST tested rows over all pairs (0 for SLOW);
 * n_union = |deGeneUnion|. */
SCC_API int scc_de_result_counts(const scc_de_result* r, int32_t* n_pairs, int64_t* n_rows, int32_t* n_union);
/* deGeneUnion as 0-based gene rows, in the reference's order (Fast:392 / slow:224). */
SCC_API int scc_de_result_union(const scc_de_result* r, int32_t* genes);
/* FAST rows, pair-major, inside a pair in R's order(p, -avg_logFC) (Fast:346):
 * every tested feature of every pair.  flags bit0 = kept DE row
 * (pair has > 1 row and q < qValThrs, Fast:376-377), bit1 = survives
 * top_n (Fast:391).  u2 = 2 * W (W = wilcox STATISTIC); ties = sum(t^3 - t).
 * Any pointer may be NULL. */
SCC_API int scc_de_result_rows(const scc_de_result* r, int32_t* pair_rows /* [n_pairs] */, int32_t* gene,
                       double* p, double* q, double* avg_logfc, double* pct1, double* pct2, int64_t* u2,
                       int64_t* ties, uint8_t* flags);
/* SLOW per-pair full vectors [n_pairs][G] (the qValueList/logFCList RDS dumps,
 * slow:181-184,200-202) plus p, u2 and de (0/1).  Any pointer may be NULL. */
SCC_API int scc_de_result_pair_vectors(const scc_de_result* r, double* p, double* q, double* logfc, int64_t* u2,
                               uint8_t* de);
/* log(meanScalingFactor * mean(expm1(X))) used by SLOW (slow:36,111). */
SCC_API int scc_de_result_log_threshold(const scc_de_result* r, double* log_thr);
/* nodg: number of genes with x > 0 per cell, all cells (Fast:440-443). */
SCC_API int scc_de_result_nodg(const scc_de_result* r, int32_t* nodg /* [N] */);
SCC_API void scc_de_result_destroy(scc_de_result* r);

/* ---- one-vs-rest marker genes: every cluster against the rest, one pass ----
 * The reference README's FindAllMarkers step (README.md:143-153) on the
 * engine.  Kept clusters are the codes 0..K-1; cells with code -1 take part
 * in nothing.  For each cluster a, cells.1 = {code == a}, cells.2 = {code >= 0
 * and code != a}, and the result for a is what ComputePairWiseDE(cells.1,
 * cells.2, test.use = "wilcox") returns (Fast:73-355) followed by the caller's
 * rules (Fast:376-392):
 *   pct1 = 100 cnt_a / n_a, pct2 = 100 (cnt_sel - cnt_a) / n_rest (exact);
 *   avg_logFC = log(mean_a(expm1 x) + 1) - log(mean_rest(expm1 x) + 1), the
 *     rest's mean from the double-double sums of the other clusters added in
 *     cluster order and divided once by n_rest;
 *   filters max(pct1, pct2) > min_per_cent, expm1(m1) > 0 || expm1(m2) > 0,
 *     |avg_logFC| > log_fc_thrs (only_pos: avg_logFC > log_fc_thrs), strict;
 *   wilcox.test's rule: exact iff n_a < 50, n_rest < 50 and no ties, else the
 *     continuity-corrected normal p;
 *   rows in order(p, -avg_logFC), BH with n = the cluster's tested rows, a
 *     cluster with <= 1 tested row contributes nothing, flags as in
 *     scc_de_result_rows, the union unique() over a = 0..K-1 in row order.
 * One sort of a gene's nonzeros serves all K tests: the statistics are exact
 * integers (2U_a equals the sum over b != a of the all-pairs 2U_ab).
 * The result is an ordinary scc_de_result with the K clusters in the place of
 * pairs: scc_de_result_counts reports n_pairs = K; scc_de_result_rows gives
 * cluster-major rows (pct1: cluster a, pct2: the rest, u2 = 2W of cluster a,
 * ties = the selection's tie term, the same for every cluster of a gene);
 * scc_de_result_union and scc_de_result_nodg as for scc_de_run;
 * scc_de_result_pair_vectors (p, logfc, u2; q and de NULL) and
 * scc_de_result_ties give the dense [K][G] arrays -- with test_all = 1 also
 * for the (cluster, gene) cells the filters drop, else p = NaN, u2 = ties = -1
 * there.
 * Limits: test = SCC_TEST_WILCOX only (SCC_TEST_T and SCC_TEST_BIMOD return
 * SCC_ERR_UNSUPPORTED); K <= 128 (more: SCC_ERR_UNSUPPORTED); every cluster
 * needs >= 3 cells (min.cells.group; else SCC_ERR_RSTOP, as scc_de_run);
 * there is no SLOW form; no subsampling, no min.diff.pct; the call runs on the
 * context's first device only. */
typedef struct {
    int32_t top_n, only_pos, test /* SCC_TEST_WILCOX only */, test_all;
    double q_val_thrs, log_fc_thrs, min_per_cent;
    int32_t reserved[4]; /* must be zero (else SCC_ERR_INVALID) */
} scc_markers_params;
SCC_API int scc_de_markers(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host [N] */, int32_t K,
                           const scc_markers_params* params, scc_de_result** out);
/* The dense tie terms [n_pairs][G] of an scc_de_markers result (every row of a
 * tested gene holds the same value). */
SCC_API int scc_de_result_ties(const scc_de_result* r, int64_t* ties);

/* ---- stage 3: cell x cell distance on the DE-gene union ---------------- */
/* Packed lower triangle in R `dist` order (column-major: (1,0),(2,0),...,
 * (N-1,0),(2,1),...), length N(N-1)/2.  out_kind SCC_PTR_HOST copies to the
 * caller's host buffer; SCC_PTR_DEVICE writes a device buffer of the ctx
 * device (dist_out == NULL: the engine keeps it HBM-resident in its own
 * workspace, valid until the next call; that call returns as soon as its work
 * is queued, and a failure of its eigensolver's cross-workgroup hand-off is
 * reported by the next synchronising call: scc_ctx_synchronize, scc_de_run,
 * or an scc_distance into a host or caller buffer).  ncomp <= 0 means min(n_union, 15) (Fast:398).  out_f32 != 0 writes
 * float instead of double. */
SCC_API int scc_distance(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host */, int32_t n_union,
                 int32_t metric, int32_t ncomp, void* dist_out, int32_t out_kind, int32_t out_f32);
/* reclusterDEConsensusFast's compute path in one call (Fast:57-400): the DE
 * of scc_de_run, then scc_distance over its gene union, without returning to
 * the caller in between (one host round trip fewer per job).  *out receives
 * the DE result as from scc_de_run (the union: scc_de_result_union); the
 * distance goes to dist_out as in scc_distance.  An empty union fails with
 * SCC_ERR_INVALID after *out is set. */
SCC_API int scc_de_distance(scc_ctx* ctx, const scc_dataset* ds, const int32_t* code /* host, [N] */, int32_t K,
                    const scc_de_params* params, int32_t metric, int32_t ncomp, void* dist_out, int32_t out_kind,
                    int32_t out_f32, scc_de_result** out);
/* The same for the columns [col_lo, col_hi) only: entries
 * [col_lo(2N-col_lo-1)/2, col_hi(2N-col_hi-1)/2) of the packed R `dist`
 * vector, a contiguous slice.  Ranks that split [0, N) into column ranges of
 * equal entry counts each compute and keep their slice (the
 * distance tiles stay HBM-resident per GPU); the PCA is recomputed on every
 * rank.  The eigensolver's reductions have a fixed shape (no dependence on how
 * many workgroups joined a hand-off), so every rank gets the same scores bit
 * for bit on the same device type. */
SCC_API int scc_distance_cols(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host */,
                      int32_t n_union, int32_t metric, int32_t ncomp, int64_t col_lo, int64_t col_hi,
                      void* dist_out, int32_t out_kind, int32_t out_f32);
/* ---- stage 3 sharded over ranks (one process per GPU) --------
 * prcomp_irlba + dist (Fast:398-400) of ONE job over the ranks of a process
 * group: every rank holds the dataset and owns the cells [cell_lo, cell_hi)
 * (ranks in order, covering [0, N)).  Each rank calls, with the same genes:
 *   scc_pca_shard_colsum(.., part)      part: device, 2 * n_union doubles =
 *       this rank's double-double column sums of X[U, cell_lo:cell_hi)
 *   -> the caller all-gathers the parts in rank order: parts [world][2 n_union]
 *   scc_pca_shard_gram(.., parts, world, gram)   gram: device, n_union^2
 *       doubles = this rank's partial Gram of the centred rows
 *   -> the caller all-reduces (sums) gram
 *   scc_pca_shard_scores(.., gram_sum, ncomp, scores)   scores: device
 *       [N][16] doubles; rows [cell_lo, cell_hi) written, others untouched
 *   -> the caller combines the score rows of all ranks (disjoint)
 *   scc_distance_scores(.., scores, ..)  the packed `dist` columns
 *       [col_lo, col_hi) from the full score matrix.
 * The mean is the same double-double sum as the unsharded path's, combined in
 * rank order, so every rank sees identical bits; the eigensolve of the summed
 * Gram runs once (scc_pca_shard_eigen on rank 0, vectors broadcast) or on every
 * rank (scc_pca_shard_scores = eigen + project, single-rank use).
 * Order: colsum, then gram, then eigen / project / scores; a call before its
 * predecessor on the same context fails with SCC_ERR_INVALID.  An empty shard
 * (cell_lo == cell_hi, a rank with no cells) is valid: SCC_OK with zero sums,
 * a zero partial Gram and no score rows written. */
SCC_API int scc_pca_shard_colsum(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host */,
                                 int32_t n_union, int64_t cell_lo, int64_t cell_hi, void* part /* device */);
SCC_API int scc_pca_shard_gram(scc_ctx* ctx, const void* parts /* device [world][2 n_union] */, int32_t world,
                               void* gram /* device [n_union][n_union] */);
SCC_API int scc_pca_shard_scores(scc_ctx* ctx, const void* gram_sum /* device */, int32_t ncomp,
                                 void* scores /* device [N][16] */);
/* scc_pca_shard_scores in two halves, so the eigenvectors can come from ONE
 * rank: scc_pca_shard_eigen writes the top-ncomp eigenvectors of gram_sum as
 * vecs [n_union][16] doubles (device; columns >= ncomp zero); the caller
 * broadcasts rank 0's vecs; scc_pca_shard_project scores this rank's cells
 * with them (rows [cell_lo, cell_hi) of scores).  The eigensolver's hand-off
 * kernel sums per-workgroup partials and how many workgroups join depends on
 * arrival order, so separate eigensolves may differ in the last bits; one
 * broadcast set of vectors makes every rank's block a block of one embedding. */
SCC_API int scc_pca_shard_eigen(scc_ctx* ctx, const void* gram_sum /* device */, int32_t ncomp,
                                void* vecs /* device [n_union][16] */);
SCC_API int scc_pca_shard_project(scc_ctx* ctx, const void* vecs /* device [n_union][16] */, int32_t ncomp,
                                  void* scores /* device [N][16] */);
/* Packed `dist` columns [col_lo, col_hi) from a device score matrix [N][16]
 * (components >= ncomp zero); output as in scc_distance_cols. */
SCC_API int scc_distance_scores(scc_ctx* ctx, const void* scores /* device */, int64_t n_cells, int64_t col_lo,
                                int64_t col_hi, void* dist_out, int32_t out_kind, int32_t out_f32);

/* ---- silhouette on the distance vector (Fast:433) ---------
 * cluster::silhouette(groups, dmatrix = as.matrix(d)) without the N x N
 * matrix: widths[i] = s(i) (0 for a singleton cluster), clus_avg[k] = mean
 * width of the k-th cluster in increasing group-id order (summary(.)$
 * clus.avg.widths; the reference averages them into "SI").  dist: device
 * pointer to the full packed vector (f64, or f32 if dist_f32), or NULL for
 * the engine-kept output of the last full scc_distance call.  Needs
 * 2 <= n_groups < n_cells (R returns NA otherwise).  Any output may be NULL. */
SCC_API int scc_silhouette(scc_ctx* ctx, int64_t n_cells, const int32_t* groups /* host [N] */, const void* dist,
                   int32_t dist_f32, double* widths /* host [N] */, double* clus_avg /* host [n_groups] */,
                   int32_t* n_groups);
/* PCA scores (N x ncomp, row-major) of the last PCA distance call. */
SCC_API int scc_last_pca_scores(const scc_ctx* ctx, double* scores, int32_t* ncomp);

/* ---- host clustering on the packed distance --------------
 * Host code (no device needed), restating the packages the reference calls:
 *   fastcluster::hclust(d, method = "ward.D2")            Fast:406-411
 *     merge: [2 (n-1)] int32, R's column-major (n-1) x 2 merge matrix
 *     (-i = observation i, +k = merge k, 1-based); height [n-1]; order [n]
 *     (1-based leaf order, may be NULL).  dist: host packed R `dist` vector.
 *   dynamicTreeCut::cutreeDynamic(dendro, distM = as.matrix(d), deepSplit,
 *     pamStage = FALSE, minClusterSize) (method "hybrid", default cut height)
 *                                                         Fast:421-427
 *     labels [n]: 0 = unassigned, 1.. by decreasing cluster size; cut_height
 *     (may be NULL) receives the default cut height used. */
SCC_API int scc_hclust_ward_d2(const double* dist, int64_t n, int32_t* merge, double* height, int32_t* order);
SCC_API int scc_cutree_hybrid(const int32_t* merge, const double* height, int64_t n, const double* dist,
                              int32_t deep_split, int32_t min_cluster_size, int32_t* labels, double* cut_height);

/* ---- the same two on the device-resident distance -----------------------
 * The tree and the cut without the packed vector ever crossing PCIe (opt-in;
 * Fast:406-431, slow:242-266).  For the same distance values both return
 * exactly what the host functions return (merge, height, order, labels and
 * cut height bit for bit): the NN-chain runs in one workgroup with the host's
 * scan order and update arithmetic (scc_hclust.hip), the tree cut reads its
 * core x core blocks through a gather kernel and sums them on the host.
 *
 * fastcluster::hclust(d, "ward.D2") on a device-resident packed dist.  dist: device pointer
 * (f64, or f32 if dist_f32), or NULL = the engine-kept output of the last full scc_distance
 * call (as scc_silhouette).  merge/height/order: host, as scc_hclust_ward_d2.
 * SCC_ERR_NONFINITE: a non-finite entry; SCC_ERR_INVALID: no kept distance, or one of another
 * size; SCC_ERR_OOM: the full symmetric working copy (8 n^2 bytes, freed before returning)
 * does not fit in half of the free device memory; SCC_ERR_HIP: the chain passed a loop cap.
 * The chain runs as ceil((n - 1) / SCC_HCLUST_MERGES_PER_LAUNCH) launches (timer family
 * "hclust_dev"; the expansion: "hclust_expand"). */
#define SCC_HCLUST_MERGES_PER_LAUNCH 1024
SCC_API int scc_hclust_ward_d2_dev(scc_ctx* ctx, int64_t n, const void* dist, int32_t dist_f32, int32_t* merge,
                                   double* height, int32_t* order);
/* scc_cutree_hybrid with distM read from the device-resident dist (same NULL rule). */
SCC_API int scc_cutree_hybrid_dev(scc_ctx* ctx, const int32_t* merge, const double* height, int64_t n,
                                  const void* dist, int32_t dist_f32, int32_t deep_split, int32_t min_cluster_size,
                                  int32_t* labels, double* cut_height);

/* ---- the same two from the PCA scores, no N x N matrix -------------------
 * The third route (opt-in) to cellTree and dynamicColors, for cell counts whose
 * packed distance (4 n^2 bytes) or its working copy (8 n^2 bytes) fit nowhere.
 * The distance is dist() of the [n][16] scores, and Ward linkage on Euclidean
 * points needs only centroids and sizes: 2 |A| |B| / (|A| + |B|) |cA - cB|^2 is
 * the squared dissimilarity the Lance-Williams update carries, a merge is a
 * weighted mean.  Device memory: 128 bytes of centroid per cell plus ~40 bytes
 * of chain state (scc_hclust_vec.hip).
 *
 * Where it differs from the host and the device route: the chain is the same
 * (restart, scan order, lowest index on a tie, the larger index survives), the
 * rounding is not.  It returns their tree (merge and order equal, heights
 * within a few ulp) whenever no two candidate dissimilarities lie within
 * rounding of each other; on exact ties (duplicate cells, lattices) it returns
 * a valid Ward tree that may resolve the tie differently.
 *
 * scc_pca_scores: the PCA half of scc_distance(SCC_DIST_PCA_EUCLID), stopping
 * before the dist kernel: it never allocates the n (n - 1) / 2 outputs.  The
 * [n][16] scores are kept where scc_distance keeps them (scc_last_pca_scores
 * returns the same bits after either call on the same input); any engine-kept
 * distance is dropped, so a later NULL-distance call (scc_silhouette,
 * scc_hclust_ward_d2_dev, scc_cutree_hybrid_dev) fails with SCC_ERR_INVALID.
 * Runs on devices[0] only. */
SCC_API int scc_pca_scores(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host */, int32_t n_union,
                           int32_t ncomp);
/* hclust(dist(scores), "ward.D2").  scores: device pointer to [n][16] doubles, unused
 * components zero (as scc_distance_scores takes them), read only; NULL = the kept scores
 * of the last scc_pca_scores / PCA scc_distance.  merge/height/order: host, as
 * scc_hclust_ward_d2.  SCC_ERR_NONFINITE: a non-finite score; SCC_ERR_INVALID: no kept
 * scores, or scores of another size; SCC_ERR_HIP: the chain passed a loop cap.
 * One nearest-neighbour scan is two launches (a grid over the nodes,
 * SCC_HCLUST_VEC_SCAN_NODES per workgroup, then one workgroup that steps the chain); the
 * host queues SCC_HCLUST_VEC_SCANS_PER_BATCH scans, reads the state and queues the next
 * batch until the last merge (timer family "hclust_vec", one entry per launch). */
#define SCC_HCLUST_VEC_SCAN_NODES 512
#define SCC_HCLUST_VEC_SCANS_PER_BATCH 1024
SCC_API int scc_hclust_ward_d2_scores(scc_ctx* ctx, int64_t n, const void* scores, int32_t* merge, double* height,
                                      int32_t* order);
/* scc_cutree_hybrid_dev with distM[core, core] computed from the scores (same NULL rule as
 * scc_hclust_ward_d2_scores) with the dist kernel's arithmetic: the values the packed f64
 * vector would hold, so the labels are those of the other routes for the same tree. */
SCC_API int scc_cutree_hybrid_scores(scc_ctx* ctx, const int32_t* merge, const double* height, int64_t n,
                                     const void* scores, int32_t deep_split, int32_t min_cluster_size,
                                     int32_t* labels, double* cut_height);
/* scc_silhouette of dist(scores) without the packed vector: deepSplitInfo's SI (Fast:433)
 * on this route.  Each d(i, j) is computed from score rows i and j with the dist kernel's
 * arithmetic where scc_silhouette loads it, and summed in the same order, so widths and
 * clus_avg are bit for bit those of scc_silhouette on the f64 scc_distance_scores output of
 * the same scores.  Device memory: the scores, 8 n n_groups doubles of partial sums, O(n)
 * besides.  groups, widths, clus_avg, n_groups: as scc_silhouette (sorted group ids,
 * 2 <= n_groups < n_cells, singleton width 0, any output may be NULL).  scores: as
 * scc_hclust_ward_d2_scores (read only; NULL = the kept scores).  SCC_ERR_NONFINITE: a
 * non-finite score (counted on the device before the widths are read, never returned as NaN
 * widths); SCC_ERR_INVALID: a bad group count, no kept scores, or scores of another size.
 * More than 64 groups run as further passes that compute the entries again.  Runs on
 * devices[0] only (timer family "silhouette_scores", one entry per call). */
SCC_API int scc_silhouette_scores(scc_ctx* ctx, int64_t n_cells, const int32_t* groups /* host [N] */,
                                  const void* scores /* device [n][16], NULL = kept */, double* widths,
                                  double* clus_avg, int32_t* n_groups);
/* The exact k nearest neighbours of every cell under dist(scores), the search
 * umap::umap(d = pca.data) and every other graph method on the scores starts with,
 * without the packed vector or an n x n matrix.  For cell i: the k cells j != i with the
 * smallest d(i, j), ordered by (distance ascending, index ascending); the same key decides
 * which cell holds the k-th place, so the result does not depend on how the columns are
 * tiled, chunked or merged, and two calls return the same bits.  d(i, j) is computed from
 * score rows i and j with the dist kernel's arithmetic: dist[i][.] are bit for bit entries of
 * the f64 scc_distance_scores output of the same scores.  dims: only the first dims
 * components enter and the others are taken as zero (the README's pca.obj$x[, 1:8]), bit
 * for bit the dims = 0 call on a copy whose other components are zeroed; the caller makes
 * no copy.  scores: as scc_hclust_ward_d2_scores (read only; NULL = the kept scores).
 * Device memory: the scores, 12 n k bytes of result, 12 k bytes per row of a launch and
 * column chunk (at most 16 chunks) of partial lists, O(n) besides.  Launches are split by
 * row blocks of about 2^36 entries (SCC_KNN_ROWS_PER_LAUNCH overrides the rows).
 *   SCC_ERR_INVALID      no kept scores or scores of another size, k < 1 or k > n - 1,
 *                        dims outside 0..15
 *   SCC_ERR_UNSUPPORTED  k > SCC_KNN_MAX_K
 *   SCC_ERR_NONFINITE    a non-finite score (counted on the device before any output is
 *                        copied; no NaN distance is returned)
 * A refused call leaves the context, the kept scores and any kept distance as they were.
 * Runs on devices[0] only (timer family "knn_scores", one entry per call). */
#define SCC_KNN_MAX_K 64
SCC_API int scc_knn_scores(scc_ctx* ctx, int64_t n, const void* scores /* device [n][16], NULL = kept */,
                           int32_t dims /* 1..15, 0 = all */, int32_t k,
                           int32_t* idx /* host [n][k], 0-based */, double* dist /* host [n][k], may be NULL */);

/* ---- UMAP of the cells (README.md:143-160: umap::umap(d = pca.data)) -------
 * The last step of the README's example on the device: the fuzzy simplicial set
 * of a k-NN table (umap-learn's smooth_knn_dist, compute_membership_strengths
 * and fuzzy_simplicial_set), the stochastic-gradient layout of a symmetric
 * weighted graph, and both behind scc_knn_scores in one call.  Everything is
 * f64, no floating-point atomic is used, every random draw is a pure function
 * of (seed, epoch, edge, draw): two calls return the same bits.  Agreement with
 * the umap, uwot or umap-learn packages has not been measured (none was
 * available); the rules are restated in NumPy in tests/umap_reference.py.
 * All three run on devices[0] only, in workspace buffers of their own ("um_*";
 * scc_umap_scores also in scc_knn_scores'): a refused call leaves the context,
 * the kept scores and any kept distance as they were. */
typedef struct {
    double local_connectivity; /* 1.0 only (else SCC_ERR_UNSUPPORTED) */
    double bandwidth;          /* 1.0 only (else SCC_ERR_UNSUPPORTED) */
    double set_op_mix_ratio;   /* in [0, 1]; 1 = the fuzzy union, 0 = the intersection */
    int32_t n_epochs;          /* >= 1 (the R package's default: 200) */
    int32_t negative_sample_rate; /* 0..64 (default 5) */
    double a, b;               /* the curve 1 / (1 + a d^(2b)); 0, 0 = SCC_UMAP_A, SCC_UMAP_B */
    double gamma;              /* repulsion strength (default 1) */
    double learning_rate;      /* initial alpha (default 1) */
    uint64_t seed;
    int32_t reserved[4];
} scc_umap_params;
/* find_ab_params(spread = 1, min_dist = 0.1): scipy.optimize.curve_fit of 1 / (1 + a x^(2b)) to
 * umap-learn's target curve at 300 points of [0, 3] */
#define SCC_UMAP_A 1.5769434602697652
#define SCC_UMAP_B 0.8950608778515733

/* The fuzzy simplicial set of a k-NN table in scc_knn_scores' output form (0-based, the cell
 * itself left out, each row ascending in distance), n_neighbors = k + 1 (the cell counts as
 * its own first neighbour).  Per row i over its k entries d_ij:
 *   rho_i    the smallest strictly positive d_ij (0 if none)
 *   sigma_i  bisection lo = 0, hi = inf, mid = 1, at most 64 steps, on
 *            psum = sum_j (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / mid) : 1) against
 *            target = log2(k + 1): stop at |psum - target| < 1e-5; psum > target: hi = mid,
 *            mid = (lo + hi) / 2; else lo = mid and mid *= 2 while hi is infinite, else
 *            mid = (lo + hi) / 2.  Then sigma_i = max(mid, 1e-3 mean(row i)) if rho_i > 0, else
 *            max(mid, 1e-3 mean(all distances)) (row sums in entry order, the global sum one
 *            fixed-shape reduction of the row sums)
 *   w_ij     (d_ij - rho_i <= 0 || sigma_i == 0) ? 1 : exp(-(d_ij - rho_i) / sigma_i)
 * An entry whose index is its own row is dropped.  With a = w_ij, b = w_ji (a missing entry
 * counts as 0) and mix = set_op_mix_ratio the edge value is mix (a + b - a b) + (1 - mix) a b,
 * bit for bit the same on (i, j) and (j, i); the edge set is the union of the table and its
 * transpose (mix > 0) or their intersection (mix == 0).  Output: host CSR, columns ascending
 * within a row, rows of any length up to n - 1; cap: the entries cols and vals hold (2 n k
 * always suffices); *nnz the entries written.  rho, sigma: host [n], weights: host [n][k] (the
 * directed w_ij, a dropped entry's included); each may be NULL.
 *   SCC_ERR_INVALID      n < 2, k < 1 or k > n - 1, an index outside 0..n-1 or listed twice in
 *                        a row, a negative distance, a row not ascending in distance,
 *                        set_op_mix_ratio outside [0, 1], cap below the entries needed
 *   SCC_ERR_NONFINITE    a non-finite distance
 *   SCC_ERR_UNSUPPORTED  k > SCC_KNN_MAX_K, local_connectivity or bandwidth other than 1
 * Timer family "umap_graph", one entry per call. */
SCC_API int scc_umap_graph(scc_ctx* ctx, int64_t n, int32_t k, const int32_t* idx /* host [n][k] */,
                           const double* dist /* host [n][k] */, const scc_umap_params* prm,
                           int64_t* indptr /* host [n + 1] */, int32_t* cols /* host [cap] */,
                           double* vals /* host [cap] */, int64_t cap, int64_t* nnz, double* rho, double* sigma,
                           double* weights);
/* The layout of a symmetric weighted graph (host CSR as scc_umap_graph returns it) from
 * init [n][2] to Y [n][2], n_epochs epochs of one launch each on double-buffered positions:
 * vertex i owns row i, reads every position from the previous epoch's buffer and is the only
 * writer of its new position and of its row's schedule, so an edge is seen from both ends, each
 * on its own schedule.  With w_max the largest weight, an edge of weight w acts when w > 0 and
 * w >= w_max / n_epochs: period p = w_max / w, next = p and next_neg = p / nsr initially
 * (nsr = negative_sample_rate).  Epoch e = 1 .. n_epochs, alpha = learning_rate (1 - (e - 1) /
 * n_epochs); an edge (i, j) at place `slot` of cols acts iff next <= e:
 *   attraction   d2 = |y_i - y_j|^2, c = d2 > 0 ? -2 a b d2^(b-1) / (a d2^b + 1) : 0,
 *                move clip(c (y_i - y_j), -4, 4) per coordinate
 *   m = floor((e - next_neg) / (p / nsr)) draws (0 <= m <= 65535; nsr = 0: none), then
 *                next_neg += m p / nsr, next += p; draw s picks
 *                v = ((mix64(seed + C ctr) >> 32) n) >> 32, C = 0x9E3779B97F4A7C15,
 *                ctr = ((e nnz + slot) << 16) + s (mod 2^64), mix64 splitmix64's output
 *                function (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *                z *= 0x94D049BB133111EB, z ^= z >> 31); v == i is skipped, else
 *                c = d2 > 0 ? 2 gamma b / ((0.001 + d2)(a d2^b + 1)) : 0 and the move is
 *                clip(c (y_i - y_v), -4, 4), or +4 in both coordinates when d2 == 0
 *   y_i += alpha (the sum of i's moves: 16 lanes take the row's slots l, l + 16, ..., each adds
 *                in slot order, attraction before the slot's draws, then one xor butterfly)
 *   SCC_ERR_INVALID    n < 1, indptr not ascending from 0, a column outside 0..n-1, a negative
 *                      weight, n_epochs < 1, a negative a or b, negative_sample_rate outside 0..64
 *   SCC_ERR_NONFINITE  a non-finite weight, init coordinate, gamma or learning_rate
 * Timer family "umap_layout", one entry per call. */
SCC_API int scc_umap_layout(scc_ctx* ctx, int64_t n, const int64_t* indptr /* host [n + 1] */,
                            const int32_t* cols, const double* vals, const double* init /* host [n][2] */,
                            const scc_umap_params* prm, double* Y /* host [n][2] */);
/* scc_knn_scores (k = n_neighbors - 1, same scores, dims and refusals), scc_umap_graph and
 * scc_umap_layout in one call without the table or the graph leaving the device: bit for bit
 * what the three calls return one after the other.  n_neighbors in 2..SCC_KNN_MAX_K + 1 and at
 * most n.  init: host [n][2], or NULL for the first two score columns scaled so that the
 * largest absolute coordinate is 10 (umap-learn's PCA initialisation without its noise term).
 * Only Y crosses to the host, and the graph when indptr, cols and vals are given (cap, nnz:
 * as scc_umap_graph; all three NULL: no graph is copied).  Timer families "knn_scores",
 * "umap_graph" and "umap_layout", one entry per call each. */
SCC_API int scc_umap_scores(scc_ctx* ctx, int64_t n, const void* scores /* device [n][16], NULL = kept */,
                            int32_t dims /* 1..15, 0 = all */, int32_t n_neighbors, const scc_umap_params* prm,
                            const double* init, double* Y /* host [n][2] */, int64_t* indptr, int32_t* cols,
                            double* vals, int64_t cap, int64_t* nnz);

/* ---- SNN graph and modularity clustering of the cells ----------------------
 * The step in front of the README's example: its `seuratObj$RNA_snn_res.0.2` is
 * what Seurat's FindNeighbors + FindClusters make of the PCA scores.  Here: the
 * shared-nearest-neighbour graph of a k-NN table by Seurat's ComputeSNN rule,
 * a deterministic multilevel modularity clustering of a symmetric weighted
 * graph, and both behind scc_knn_scores in one call.  No floating-point atomic
 * is used; the clustering's weights are integers, so its sums are exact in any
 * order: two calls return the same bits.  Agreement with Seurat, igraph or
 * leidenalg has not been measured (none was available); the rules are restated
 * in NumPy in tests/snn_reference.py.  Not done: Leiden or SLM refinement,
 * Seurat's grouping of singletons, a random vertex order, more than one device.
 * All three run on devices[0] only, in workspace buffers of their own ("sn_*",
 * "mc_*"; the fused call also in scc_knn_scores'): a refused call leaves the
 * context, the kept scores and any kept distance as they were. */

/* The SNN graph of a k-NN table in scc_knn_scores' output form (0-based, the cell itself left
 * out; distances are not an input).  K = k + 1 is Seurat's k.param, N_i = {i} + idx[i].  For
 * every pair i != j with s = |N_i & N_j| >= 1 (every two-hop pair, not only listed
 * neighbours): w = (double)s / (double)(K + (K - s)), kept iff w >= prune in f64.  The diagonal
 * (Seurat stores w = 1 there) is NOT stored: a choice of this engine, so that the output feeds
 * scc_modularity_cluster as it is.  Output: host CSR as scc_umap_graph returns it (indptr
 * int64, columns ascending within a row, (i, j) and (j, i) the same bits), rows of any length up
 * to n - 1; shared: the counts s parallel to vals, or NULL.  cap: the entries cols, vals and
 * shared hold; *nnz the graph's entries.  No bound such as 2 n k holds: when cap is too small
 * the call returns SCC_ERR_INVALID with *nnz set to the entries needed, and the caller may call
 * again.
 *   SCC_ERR_INVALID      n < 2, k < 1 or k > n - 1, an index outside 0..n-1 or listed twice in
 *                        a row, a row listing itself, prune outside [0, 1], cap too small
 *   SCC_ERR_NONFINITE    a non-finite prune
 *   SCC_ERR_UNSUPPORTED  k > SCC_KNN_MAX_K
 * Timer family "snn_graph", one entry per call. */
SCC_API int scc_snn_graph(scc_ctx* ctx, int64_t n, int32_t k, const int32_t* idx /* host [n][k] */,
                          double prune /* Seurat's default: 1.0 / 15 */, int64_t* indptr /* host [n + 1] */,
                          int32_t* cols /* host [cap] */, double* vals /* host [cap] */,
                          int32_t* shared /* host [cap] or NULL */, int64_t cap, int64_t* nnz);
/* Multilevel modularity clustering of a symmetric weighted graph (host CSR without a diagonal,
 * columns strictly ascending within a row, (i, j) and (j, i) the same bits: what scc_snn_graph
 * and scc_umap_graph return).  Weights enter as q = (int64)rint(w 2^32); an entry with q = 0 is
 * absent.  m2 = sum q.  One level on a graph whose vertex degrees k_i are the row sums (a coarse
 * level's self-loop included): every vertex starts in its own community; sweeps are synchronous,
 * each reading the previous sweep's communities, totals tot_c and sizes.  For vertex i in c_i
 * the candidates are c_i and the communities of its neighbours j != i:
 *   kin(c) = sum of q_ij over j in c, j != i;  t = tot_c - (c == c_i ? k_i : 0)
 *   g(c)   = (double)kin - ((resolution (double)k_i) (double)t) / (double)m2, in that order
 * c* has the largest g, ties to the smallest id; i moves iff c* != c_i, g(c*) > g(c_i) and not
 * (both communities have one member and c* > c_i).  No move: the level ends.  Else
 * Q = sum over community ids c = 0 .. (the level's vertices - 1) of
 * (double)in_c / m2 - (resolution ((double)tot_c / m2)) ((double)tot_c / m2) (in_c: every entry
 * inside c; an id without members gives 0), summed as thread t of 1024 adds terms t, t + 1024,
 * ... and a halving tree follows; Q <= the previous Q: the sweep is discarded and the level
 * ends.  At most 256 sweeps a level.  Then the communities with members are renumbered in
 * ascending id and become the next level's vertices (integer sums of the entries, the
 * self-loop all entries inside; m2 is kept); levels repeat until one merges nothing, at most
 * SCC_MODULARITY_MAX_LEVELS.  A graph without weight (m2 = 0) is left as n clusters, 0 levels.
 * labels: host [n], numbered by (size descending, smallest member ascending): 0 is the largest.
 * modularity: the last accepted Q (level 0's initial Q if none).  n_levels: levels run, the
 * last one that merged nothing included.  sweeps: host [SCC_MODULARITY_MAX_LEVELS], the sweeps
 * run in each level (a discarded or moveless last one included), 0 beyond n_levels.  Each of
 * n_clusters, modularity, n_levels, sweeps may be NULL.
 *   SCC_ERR_INVALID      n < 1, an inconsistent CSR (indptr, a column outside 0..n-1, columns
 *                        not ascending), a diagonal entry, a negative weight, a missing or
 *                        differing transpose entry, resolution <= 0
 *   SCC_ERR_NONFINITE    a non-finite weight or resolution
 *   SCC_ERR_UNSUPPORTED  a weight above 2^20, or m2 >= 2^62
 * All checked before anything is uploaded.  Timer family "modularity_cluster", one entry per
 * call. */
#define SCC_MODULARITY_MAX_LEVELS 32
SCC_API int scc_modularity_cluster(scc_ctx* ctx, int64_t n, const int64_t* indptr /* host [n + 1] */,
                                   const int32_t* cols, const double* vals, double resolution,
                                   int32_t* labels /* host [n] */, int32_t* n_clusters, double* modularity,
                                   int32_t* n_levels, int32_t* sweeps);
/* scc_knn_scores (k = k_param - 1, same scores, dims and refusals), scc_snn_graph and
 * scc_modularity_cluster in one call without the table or the graph leaving the device: bit
 * for bit what the three calls return one after the other.  k_param in 2..SCC_KNN_MAX_K + 1 and
 * at most n.  Only the labels cross to the host, and the graph when indptr, cols and vals are
 * given (cap, nnz: as scc_snn_graph; all three NULL: no graph is copied, *nnz is still set).
 * Timer families "knn_scores", "snn_graph" and "modularity_cluster", one entry per call each. */
SCC_API int scc_snn_clusters_scores(scc_ctx* ctx, int64_t n, const void* scores /* device [n][16], NULL = kept */,
                                    int32_t dims /* 1..15, 0 = all */, int32_t k_param, double prune,
                                    double resolution, int32_t* labels /* host [n] */, int32_t* n_clusters,
                                    double* modularity, int32_t* n_levels, int32_t* sweeps, int64_t* indptr,
                                    int32_t* cols, double* vals, int64_t cap, int64_t* nnz);

/* ---- heatmap inputs (cellTypeDEPlot.R:168-253) ---------------------------
 * What both reference functions end with (Fast:456-464, slow:288-296):
 * cellTypeDEPlot(dataMatrix[deGeneUnion, ], ...) hands the |U| x N block to
 * ComplexHeatmap::Heatmap(cluster_rows = TRUE, use_raster = TRUE), which
 * clusters the GENE rows (dist, hclust "complete", a dendrogram reorder by
 * -rowMeans) and rasterises every cell; the colour ramp needs the extrema of x
 * and |x| (cellTypeDEPlot.R:174-222).  These four calls compute those inputs;
 * the drawing stays with the caller.  The two device calls run on devices[0]
 * only; their host outputs may each be NULL.
 *
 * scc_gene_distance: dist = dist(X[U, ], "euclidean"), the genes as
 * observations over ALL n_cells cells, packed in R `dist` order (nu (nu-1)/2
 * doubles).  Each entry is sqrt(sum_c (x_ac - x_bc)^2) from the direct
 * differences (no Gram identity: no cancellation, identical rows give exactly
 * 0.0), the cells split into slabs whose partial sums are added in a fixed
 * order: two calls return the same bits, and within 2 N 2^-53 relative of the
 * exact value.  row_mean[u] = rowMeans(X[U, ])[u], from the double-double
 * column sums the PCA's centring uses.  range = {min x, max x, min |x|,
 * max |x|} over the nu x N block, a sparse dataset's implicit zeros included
 * (elements of the input, exact).
 *   SCC_ERR_INVALID    nu < 2, a gene out of range or listed twice, a dataset
 *                      of another context
 *   SCC_ERR_NONFINITE  a non-finite value in the block (counted on the device
 *                      before any output is copied; no NaN distance is returned)
 *   SCC_ERR_OOM        the [N][ld] panel (ld = nu rounded up to 64) plus the
 *                      slabs do not fit in half of the free device memory (the
 *                      rule of scc_hclust_ward_d2_dev)
 * Both device calls work in workspace buffers of their own ("hm_*"): the
 * engine-kept distance and scores of an earlier scc_distance / scc_pca_scores,
 * and the PCA's panel, are left as they were (a later NULL-distance
 * scc_silhouette returns what it returned before).  Timer family "gene_dist"
 * (one entry per call: the pair kernel and the slab reduction). */
SCC_API int scc_gene_distance(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host [nu] */, int32_t nu,
                              double* dist /* host [nu (nu-1)/2] */, double* row_mean /* host [nu] */,
                              double* range /* host [4] */);
/* stats::hclust(d, "complete") on a host packed `dist` vector (host code, no
 * device): merge, height, order as scc_hclust_ward_d2.  Heights are entries of
 * dist, unmodified.  An O(n^2) NN-chain (complete linkage is reducible); on
 * exact ties the lowest index wins, and the result is then a valid
 * complete-linkage tree that R (which merges the globally closest pair at
 * every step) may resolve otherwise.  SCC_ERR_NONFINITE: a non-finite entry. */
SCC_API int scc_hclust_complete(const double* dist, int64_t n, int32_t* merge, double* height, int32_t* order);
/* stats::reorder.dendrogram(as.dendrogram(tree), wts, agglo.FUN = mean) (host
 * code): a leaf's value is wts[leaf], an inner node's the mean of its two
 * children's values (R's mean(): long-double sum, one correction pass);
 * children are placed in increasing value, an equal pair keeps its order.
 * merge: column-major (n-1) x 2 as hclust returns it; merge_out: the same
 * with the two entries of a row swapped where the children swap (it no longer
 * obeys hclust's singletons-first rule, which as.dendrogram does not need);
 * order_out [n]: the resulting 1-based leaf order.  Either output may be NULL.
 * ComplexHeatmap's default row weight is -rowMeans(mat).  SCC_ERR_INVALID: a
 * merge matrix that is not a tree over n leaves. */
SCC_API int scc_dendro_reorder(const int32_t* merge, int64_t n, const double* wts /* [n] */, int32_t* merge_out,
                               int32_t* order_out);
/* The raster ComplexHeatmap draws with use_raster = TRUE, reduced to `width`
 * columns: out row r is gene genes[row_order[r] - 1]; out column b is the
 * mean of that gene over the cells cell_order[floor(b N / width) ..
 * floor((b + 1) N / width)), summed in cell_order order and divided once.
 * 1 <= width <= N; with width == N the output is the reordered matrix itself,
 * bit for bit.  row_order: 1-based positions into genes (a permutation of
 * 1..nu); cell_order: 1-based cells (a permutation of 1..N, an hclust $order).
 * out: host f64 [nu][width], row-major.  nu >= 1.  SCC_ERR_INVALID: an order
 * that is not a permutation, a bad width, a gene out of range or listed
 * twice; SCC_ERR_OOM as scc_gene_distance (the panel plus the [width][ld]
 * device raster).  Workspace: as scc_gene_distance.  Timer family
 * "heatmap_raster". */
SCC_API int scc_heatmap_raster(scc_ctx* ctx, const scc_dataset* ds, const int32_t* genes /* host [nu] */, int32_t nu,
                               const int32_t* row_order /* host [nu] */, const int32_t* cell_order /* host [N] */,
                               int32_t width, double* out /* host [nu][width] */);

/* ---- diagnostics (tests): the PCA eigensolver's parts on device pointers --
 * Not on the R path.  Each synchronises the device and returns 0 on success.
 *   scc_diag_eigen_topk   top-k eigenpairs of a device n x n symmetric A (lda)
 *                         through the engine's eigensolver (Z [n][16], W [k]);
 *                         *path: which solver answered (0 direct, 1 subspace
 *                         iteration, 2 Chebyshev-filtered subspace iteration)
 *   scc_diag_small_syev   the one-workgroup solver for n <= 64 (Rayleigh-Ritz)
 *   scc_diag_cholinv      T = R^-1 of G + shift_rel tr(G) I = R^T R, P = 48 or 64
 *   scc_diag_eig_last_path  the calling thread's last answer path */
SCC_API int scc_diag_eigen_topk(const double* A, int n, int lda, int k, double* Z, double* W, int* path);
SCC_API int scc_diag_small_syev(const double* H, int n, int ldh, int k, double* Y, double* theta, unsigned* flag);
SCC_API int scc_diag_cholinv(const double* G, int P, double shift_rel, double* T, unsigned* flag);
SCC_API int scc_diag_eig_last_path(void);
/* Which ingest the calling thread's last DE run (scc_de_run, a gene shard, or
 * the DE of scc_de_distance) took: 0 none yet, 1 the full read of the stored
 * matrix (the validating first call, SLOW runs, dense datasets,
 * SCC_INGEST_FULL=1), 2 the lean transpose of a validated dataset, 3 the
 * regroup of the dataset's gene-major mirror. */
SCC_API int scc_diag_ingest_last_path(void);
/* Which rank route the calling thread's last DE run took: 0 no run yet, 2 the
 * walk of the dataset's value order (a FAST Wilcoxon run at K <= 16 over the
 * whole gene range on one device, on a dataset that holds the order;
 * SCC_RANK_VORDER=0 turns it off), 1 every other run: the per-call value
 * buckets, and the runs that rank nothing or rank elsewhere (SLOW, the t and
 * bimod tests, gene shards, K > 16, scc_de_markers). */
SCC_API int scc_diag_rank_last_route(void);
/* Whether that run formed the cross-bucket term of the rank sums per run: 1 on
 * rank route 2 at K <= 16 with the matrix-core bucket kernel as the call's only
 * bucket kernel (one histogram row per run of a gene's buckets inside a chunk
 * of the bucket list; SCC_RANK_RUNS=0 turns it off), 0 every other run: a row
 * per bucket and the cross kernel over buckets. */
SCC_API int scc_diag_rank_last_runs(void);
/* What the calling thread's last calls took from the dataset's gene-major
 * mirror beyond the ingest: bit 1 its last PCA gather (scc_distance,
 * scc_de_distance, scc_pca_scores) filled the panel and the column means from
 * the mirror.  Bit 0: its last DE run took the per-cluster gene statistics
 * from the mirror, without the regroup (a run on the value-order route, rank
 * route 2, at K <= 36; SCC_STATS_MIRROR=0 turns it off).  The ingest path
 * such a run reports stays 3. */
SCC_API int scc_diag_mirror_last_uses(void);
/* Nearest-neighbour scans (one row each; one pass over the centroids each) of
 * the context's last scc_hclust_ward_d2_dev or scc_hclust_ward_d2_scores, for
 * bandwidth figures; -1 without a context. */
SCC_API int64_t scc_diag_hclust_last_scans(const scc_ctx* ctx);
/* s_memtime stamps of the last scc_diag_small_syev's phases [8] */
SCC_API int scc_diag_small_syev_stamps(unsigned long long* out);

/* ---- diagnostics (tests): the DE p-value device functions on host arrays --
 * Not on the R path.  Evaluates, element by element, the same device function
 * the (pair, gene) test kernel calls, so that tests can sweep its whole domain
 * (cluster sizes, tails and branches no dataset reaches).  All pointers are
 * host pointers of n elements; arrays a kind does not read may be NULL.
 *   kind 0  wilcox.test p from u2 = i0 (twice the statistic), the tie term i1
 *           and the sizes m, nn (>= 1); the exact distribution table is built
 *           as a run builds it, at the largest size below 50 passed.  out holds
 *           2n values: the p, then 1.0 / 0.0 for the exact / normal branch.
 *   kind 1  Welch two-sided p from t = a and df = b (2 pt(-|t|, df))
 *   kind 2  the normal tail beyond |z|, z = a (min of pnorm's two tails)
 *   kind 3  pchisq(a, df = 3, lower.tail = FALSE) of the bimod test
 * Synchronises the device; returns 0 on success. */
SCC_API int scc_diag_pvalues(int kind, int n, const double* a, const double* b, const long long* i0,
                             const long long* i1, const int* m, const int* nn, double* out);

#ifdef __cplusplus
}
#endif
#endif /* SCC_H */
