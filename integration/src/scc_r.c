/*
 * scc_r.c — R `.Call` glue for libscc (include/scc.h).  Compiled only where R
 * headers exist (R CMD INSTALL of the scConsensus package with this file in
 * src/; R is absent from the build container).  The glue never lets a C++
 * frame unwind through R: every libscc entry point returns an int status, and
 * Rf_error() is raised only here, after the library call returned.
 *
 * Bindings (reference call sites they replace):
 *   C_scc_dataset   as.matrix(dataMatrix) per pair (Fast:368) / dataIn (slow:32):
 *                   ONE upload per call of the R function, held as an external
 *                   pointer that the DE and distance calls share
 *   C_scc_de_fast   R/reclusterDEConsensusFast.R:57-392 (pair loop, ComputePairWiseDE, top_n, unique)
 *   C_scc_de_slow   R/reclusterDEConsensus.R:32-227
 *   C_scc_markers   the reference README's FindAllMarkers step (README.md:143-153):
 *                   ComputePairWiseDE(cluster, all other selected cells) for every
 *                   cluster, one engine pass (scc_de_markers)
 *   C_scc_distance  R/reclusterDEConsensusFast.R:398-400 (prcomp_irlba + dist), :403 (1 - cor)
 *   C_scc_release   frees the device copy early (the finalizer does it otherwise)
 *   C_scc_devices   nCores (Fast:33,61-65) -> the context's device list
 *   C_scc_si        deepSplitInfo's silhouette SI (Fast:433) on the engine-kept dist
 *   C_scc_cutree    dynamicTreeCut::cutreeDynamic(..., distM = as.matrix(d), pamStage = FALSE)
 *                   (Fast:421-427) on the packed dist: no N x N host matrix
 *                   (options(scConsensus.engineCut = TRUE))
 *   C_scc_hclust    hclust(d, "ward.D2") (Fast:406-411) restated in C++
 *                   (options(scConsensus.engineTree = TRUE))
 *   C_scc_distance_dev, C_scc_hclust_dev, C_scc_cutree_dev
 *                   options(scConsensus.engineTree = "device"): the distance
 *                   stays in the engine (Fast:398-400), the tree (Fast:406-411,
 *                   slow:242-247) and the cuts (Fast:421-427, slow:257-263) are
 *                   computed on it there; no "dist" object reaches R
 *   C_scc_pca_scores, C_scc_hclust_scores, C_scc_cutree_scores
 *                   options(scConsensus.engineTree = "scores"): the engine stops
 *                   after the PCA (Fast:398-399) and keeps the scores; the tree
 *                   and the cuts are computed from them, no distance exists
 *   C_scc_si_scores C_scc_si on that route, from the engine-kept scores
 *                   (options(scConsensus.engineScoresSI = TRUE))
 *   C_scc_knn       sccKnn: the exact k nearest neighbours of every cell from the
 *                   PCA scores, the search umap(d = pca.data) starts with
 *   C_scc_umap      sccUmap: that search, UMAP's fuzzy simplicial set and its
 *                   layout from the PCA scores in one engine call
 *   C_scc_find_clusters  sccFindClusters: that search, the SNN graph and a
 *                   modularity clustering from the PCA scores in one engine call
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "scc.h"

static scc_ctx* g_ctx = NULL;
static int g_ndev = 1;  /* devices of g_ctx: 0 .. g_ndev - 1 */

static void ensure_ctx(void)
{
    if (g_ctx) return;
    scc_opts o;
    memset(&o, 0, sizeof(o));
    int32_t devs[64];
    if (g_ndev > 1) {
        for (int k = 0; k < g_ndev; ++k) devs[k] = k;
        o.n_devices = g_ndev;
        o.devices = devs;
    }
    if (scc_ctx_create(&o, &g_ctx) != SCC_OK) Rf_error("scConsensus engine: no MI355X (HIP) device available");
}

/* nCores (Fast:33, the PSOCK workers of Fast:61-65) -> the engine's device
 * list: min(nCores, visible GPUs) devices, ONE job sharded over them (gene
 * blocks for the DE, column slices for dist).  Recreates the context when
 * the count changes (datasets of the old context must be released first:
 * the wrappers hold one only inside a call). */
SEXP C_scc_devices(SEXP n_cores)
{
    int32_t nvis = 0;
    scc_device_count(&nvis);
    if (nvis < 1) Rf_error("scConsensus engine: no MI355X (HIP) device available");
    int want = Rf_asInteger(n_cores);
    if (want == NA_INTEGER || want < 1) want = 1;
    if (want > nvis) want = nvis;
    if (want > 64) want = 64;
    if (g_ctx && want != g_ndev) {
        scc_ctx_destroy(g_ctx);
        g_ctx = NULL;
    }
    g_ndev = want;
    ensure_ctx();
    return Rf_ScalarInteger(want);
}

static void check(int rc)
{
    if (rc != SCC_OK) Rf_error("scConsensus engine error %d: %s", rc, scc_ctx_last_error(g_ctx));
}

/* ---- the dataset handle: external pointer tagged "scc_dataset", its
 * protected slot holding c(G, N) */
static SEXP ds_tag(void) { return Rf_install("scc_dataset"); }

static void ds_finalize(SEXP h)
{
    scc_dataset* ds = (scc_dataset*)R_ExternalPtrAddr(h);
    if (ds) {
        scc_dataset_destroy(ds);
        R_ClearExternalPtr(h);
    }
}

static scc_dataset* ds_of(SEXP h, int* G, int* N)
{
    if (TYPEOF(h) != EXTPTRSXP || R_ExternalPtrTag(h) != ds_tag())
        Rf_error("scConsensus engine: not a dataset handle (use C_scc_dataset)");
    scc_dataset* ds = (scc_dataset*)R_ExternalPtrAddr(h);
    if (!ds) Rf_error("scConsensus engine: the dataset handle was released");
    SEXP dims = R_ExternalPtrProtected(h);
    if (G) *G = INTEGER(dims)[0];
    if (N) *N = INTEGER(dims)[1];
    return ds;
}

/* dgCMatrix slots (@p int, @i int, @x double), dgRMatrix slots (@p, @j, @x;
 * dim has a third entry 1) or a base double matrix -> device-resident dataset */
SEXP C_scc_dataset(SEXP x, SEXP p, SEXP i, SEXP dim)
{
    ensure_ctx();
    scc_dataset* ds = NULL;
    const int G = INTEGER(dim)[0], N = INTEGER(dim)[1];
    if (Rf_isNull(p)) {
        check(scc_dataset_create_dense(g_ctx, REAL(x), G, N, SCC_PTR_HOST, &ds));
    } else if (XLENGTH(dim) > 2 && INTEGER(dim)[2] == 1) {
        /* dgRMatrix @p is int[G+1] over genes, @j the cell columns */
        int64_t* p64 = (int64_t*)R_alloc((size_t)G + 1, sizeof(int64_t));
        for (int g = 0; g <= G; ++g) p64[g] = INTEGER(p)[g];
        check(scc_dataset_create_csr(g_ctx, p64, INTEGER(i), REAL(x), G, N, (int64_t)XLENGTH(x), SCC_PTR_HOST, &ds));
    } else {
        /* dgCMatrix @p is int[N+1]: widen to int64 once */
        int64_t* p64 = (int64_t*)R_alloc((size_t)N + 1, sizeof(int64_t));
        for (int c = 0; c <= N; ++c) p64[c] = INTEGER(p)[c];
        check(scc_dataset_create_csc(g_ctx, p64, INTEGER(i), REAL(x), G, N, (int64_t)XLENGTH(x), SCC_PTR_HOST, &ds));
    }
    SEXP dims = PROTECT(Rf_allocVector(INTSXP, 2));
    INTEGER(dims)[0] = G;
    INTEGER(dims)[1] = N;
    SEXP h = PROTECT(R_MakeExternalPtr(ds, ds_tag(), dims));
    R_RegisterCFinalizerEx(h, ds_finalize, TRUE);
    UNPROTECT(2);
    return h;
}

SEXP C_scc_release(SEXP h)
{
    if (TYPEOF(h) == EXTPTRSXP && R_ExternalPtrTag(h) == ds_tag()) ds_finalize(h);
    return R_NilValue;
}

/* returns list(union = int (1-based gene rows), nodg = int[N]) */
SEXP C_scc_de_fast(SEXP h, SEXP code, SEXP K, SEXP qthr, SEXP lfc, SEXP minpct, SEXP topn, SEXP test)
{
    ensure_ctx();
    int N = 0;
    scc_dataset* ds = ds_of(h, NULL, &N);
    if (XLENGTH(code) != N) Rf_error("scConsensus engine: %d cluster codes for %d cells", (int)XLENGTH(code), N);
    scc_de_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.mode = SCC_DE_FAST;
    prm.q_val_thrs = Rf_asReal(qthr);
    prm.log_fc_thrs = Rf_asReal(lfc);
    prm.min_per_cent = Rf_asReal(minpct);
    prm.top_n = Rf_asInteger(topn);
    /* test.use = method (Fast:372) as its SCC_TEST_* code: 0 wilcox, 1 t (the values the
     * earlier logical "t test?" argument took), 2 bimod; the engine rejects any other */
    prm.test = Rf_asInteger(test);
    scc_de_result* r = NULL;
    int rc = scc_de_run(g_ctx, ds, INTEGER(code), Rf_asInteger(K), &prm, &r);
    if (rc != SCC_OK && !r) check(rc);
    int32_t npairs = 0, nu = 0;
    int64_t nrows = 0;
    scc_de_result_counts(r, &npairs, &nrows, &nu);
    SEXP uni = PROTECT(Rf_allocVector(INTSXP, nu));
    scc_de_result_union(r, INTEGER(uni));
    for (int k = 0; k < nu; ++k) INTEGER(uni)[k] += 1;
    SEXP nodg = PROTECT(Rf_allocVector(INTSXP, N));
    scc_de_result_nodg(r, INTEGER(nodg));
    scc_de_result_destroy(r);
    if (rc != SCC_OK) {
        UNPROTECT(2);
        check(rc);
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, uni);
    SET_VECTOR_ELT(out, 1, nodg);
    UNPROTECT(3);
    return out;
}

/* One-vs-rest markers of every cluster (scc_de_markers).  Returns list(cluster =
 * int (1-based cluster index per row), gene = int (1-based gene row), p_val,
 * avg_logFC, pct.1, pct.2, p_val_adj = double, kept, top = logical, union = int
 * (1-based gene rows)); rows cluster-major, in order(p_val, -avg_logFC) inside a
 * cluster.  pct.1 / pct.2 are fractions as Seurat reports them (the engine's
 * per cent / 100). */
SEXP C_scc_markers(SEXP h, SEXP code, SEXP K, SEXP qthr, SEXP lfc, SEXP minpct, SEXP topn, SEXP onlypos)
{
    ensure_ctx();
    int N = 0;
    scc_dataset* ds = ds_of(h, NULL, &N);
    if (XLENGTH(code) != N) Rf_error("scConsensus engine: %d cluster codes for %d cells", (int)XLENGTH(code), N);
    scc_markers_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.q_val_thrs = Rf_asReal(qthr);
    prm.log_fc_thrs = Rf_asReal(lfc);
    prm.min_per_cent = Rf_asReal(minpct);
    prm.top_n = Rf_asInteger(topn);
    prm.only_pos = Rf_asLogical(onlypos) == TRUE;
    prm.test = SCC_TEST_WILCOX;
    scc_de_result* r = NULL;
    int rc = scc_de_markers(g_ctx, ds, INTEGER(code), Rf_asInteger(K), &prm, &r);
    if (rc != SCC_OK) { /* includes SCC_ERR_RSTOP: a cluster of fewer than 3 cells stops in R too */
        if (r) scc_de_result_destroy(r);
        check(rc);
    }
    int32_t nclu = 0, nu = 0;
    int64_t nrows = 0;
    scc_de_result_counts(r, &nclu, &nrows, &nu);
    const char* names[] = {"cluster", "gene", "p_val", "avg_logFC", "pct.1", "pct.2", "p_val_adj", "kept", "top",
                           "union", ""};
    SEXP out = PROTECT(Rf_mkNamed(VECSXP, names));
    SEXP cl = PROTECT(Rf_allocVector(INTSXP, nrows)), gene = PROTECT(Rf_allocVector(INTSXP, nrows));
    SEXP p = PROTECT(Rf_allocVector(REALSXP, nrows)), fc = PROTECT(Rf_allocVector(REALSXP, nrows));
    SEXP p1 = PROTECT(Rf_allocVector(REALSXP, nrows)), p2 = PROTECT(Rf_allocVector(REALSXP, nrows));
    SEXP q = PROTECT(Rf_allocVector(REALSXP, nrows));
    SEXP kept = PROTECT(Rf_allocVector(LGLSXP, nrows)), top = PROTECT(Rf_allocVector(LGLSXP, nrows));
    SEXP uni = PROTECT(Rf_allocVector(INTSXP, nu));
    int32_t* per = (int32_t*)R_alloc(nclu > 0 ? nclu : 1, sizeof(int32_t));
    uint8_t* fl = (uint8_t*)R_alloc(nrows > 0 ? nrows : 1, 1);
    rc = scc_de_result_rows(r, per, INTEGER(gene), REAL(p), REAL(q), REAL(fc), REAL(p1), REAL(p2), NULL, NULL, fl);
    scc_de_result_union(r, INTEGER(uni));
    scc_de_result_destroy(r);
    if (rc != SCC_OK) {
        UNPROTECT(11);
        check(rc);
    }
    int64_t k = 0;
    for (int a = 0; a < nclu; ++a)
        for (int i = 0; i < per[a]; ++i, ++k) INTEGER(cl)[k] = a + 1;
    for (k = 0; k < nrows; ++k) {
        INTEGER(gene)[k] += 1;
        REAL(p1)[k] /= 100.0;
        REAL(p2)[k] /= 100.0;
        LOGICAL(kept)[k] = (fl[k] & 1) != 0;
        LOGICAL(top)[k] = (fl[k] & 2) != 0;
    }
    for (int u = 0; u < nu; ++u) INTEGER(uni)[u] += 1;
    SEXP cols[] = {cl, gene, p, fc, p1, p2, q, kept, top, uni};
    for (int f = 0; f < 10; ++f) SET_VECTOR_ELT(out, f, cols[f]);
    UNPROTECT(11);
    return out;
}

/* returns list(union, q = matrix[G, P], logfc = matrix[G, P], de = raw matrix, nodg) */
SEXP C_scc_de_slow(SEXP h, SEXP code, SEXP K, SEXP qthr, SEXP fc, SEXP msf)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    if (XLENGTH(code) != N) Rf_error("scConsensus engine: %d cluster codes for %d cells", (int)XLENGTH(code), N);
    scc_de_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.mode = SCC_DE_SLOW;
    prm.top_n = 30;
    prm.q_val_thrs = Rf_asReal(qthr);
    prm.fc_thrs = Rf_asReal(fc);
    prm.mean_scaling_factor = Rf_asReal(msf);
    scc_de_result* r = NULL;
    int rc = scc_de_run(g_ctx, ds, INTEGER(code), Rf_asInteger(K), &prm, &r);
    if (rc != SCC_OK) { /* includes SCC_ERR_RSTOP: R itself would stop() here */
        if (r) scc_de_result_destroy(r);
        check(rc);
    }
    int32_t npairs = 0, nu = 0;
    int64_t nrows = 0;
    scc_de_result_counts(r, &npairs, &nrows, &nu);
    SEXP uni = PROTECT(Rf_allocVector(INTSXP, nu));
    scc_de_result_union(r, INTEGER(uni));
    for (int k = 0; k < nu; ++k) INTEGER(uni)[k] += 1;
    SEXP q = PROTECT(Rf_allocMatrix(REALSXP, G, npairs));
    SEXP lf = PROTECT(Rf_allocMatrix(REALSXP, G, npairs));
    SEXP de = PROTECT(Rf_allocMatrix(RAWSXP, G, npairs));
    scc_de_result_pair_vectors(r, NULL, REAL(q), REAL(lf), NULL, RAW(de));
    SEXP nodg = PROTECT(Rf_allocVector(INTSXP, N));
    scc_de_result_nodg(r, INTEGER(nodg));
    scc_de_result_destroy(r);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 5));
    SET_VECTOR_ELT(out, 0, uni);
    SET_VECTOR_ELT(out, 1, q);
    SET_VECTOR_ELT(out, 2, lf);
    SET_VECTOR_ELT(out, 3, de);
    SET_VECTOR_ELT(out, 4, nodg);
    UNPROTECT(6);
    return out;
}

/* returns a "dist" object body (double vector, N(N-1)/2, R order); the R
 * wrapper sets the Size/Diag/Upper/method attributes and class "dist".  The
 * engine streams it from HBM into this vector in column tiles (pageable
 * memory: a pinned staging ring). */
SEXP C_scc_distance(SEXP h, SEXP genes, SEXP metric, SEXP ncomp)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int k = 0; k < nu; ++k) {
        g0[k] = INTEGER(genes)[k] - 1;
        if (g0[k] < 0 || g0[k] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[k] + 1);
    }
    SEXP d = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)N * (N - 1) / 2));
    int rc = scc_distance(g_ctx, ds, g0, nu, Rf_asInteger(metric), Rf_asInteger(ncomp), REAL(d), SCC_PTR_HOST, 0);
    if (rc != SCC_OK) {
        UNPROTECT(1);
        check(rc);
    }
    UNPROTECT(1);
    return d;
}

/* mean(summary(cluster::silhouette(groups, as.matrix(d)))$clus.avg.widths)
 * (Fast:433) on the engine-kept output of the last C_scc_distance call.
 * R's silhouette() returns NA for fewer than 2 groups or as many groups as
 * cells, and summary(NA)$clus.avg.widths then stops ("$ operator is invalid
 * for atomic vectors"): the same stop here.  Any other failure (no kept
 * distance of this size, a HIP error) is an error too, never a silent NA. */
SEXP C_scc_si(SEXP groups)
{
    ensure_ctx();
    const int N = LENGTH(groups);
    int32_t* g = (int32_t*)R_alloc((size_t)N, sizeof(int32_t));
    for (int k = 0; k < N; ++k) g[k] = INTEGER(groups)[k];
    double* avg = (double*)R_alloc((size_t)N, sizeof(double));
    int32_t ng = 0;
    int rc = scc_silhouette(g_ctx, N, g, NULL, 0, NULL, avg, &ng);
    if (rc == SCC_ERR_INVALID && ng > 0 && (ng < 2 || ng >= N))
        Rf_error("$ operator is invalid for atomic vectors");
    check(rc);
    double s = 0.0;
    for (int k = 0; k < ng; ++k) s += avg[k];
    return Rf_ScalarReal(s / ng);
}

/* C_scc_si for options(scConsensus.engineTree = "scores"): the same mean, the
 * silhouette computed from the engine-kept scores of the last C_scc_pca_scores
 * call (scc_silhouette_scores: d = dist(scores) entry by entry, no N x N
 * matrix; the SI of C_scc_si on the f64 distance of the same scores, bit for
 * bit).  The same stop for fewer than 2 groups or as many groups as cells. */
SEXP C_scc_si_scores(SEXP groups)
{
    ensure_ctx();
    const int N = LENGTH(groups);
    int32_t* g = (int32_t*)R_alloc((size_t)N, sizeof(int32_t));
    for (int k = 0; k < N; ++k) g[k] = INTEGER(groups)[k];
    double* avg = (double*)R_alloc((size_t)N, sizeof(double));
    int32_t ng = 0;
    int rc = scc_silhouette_scores(g_ctx, N, g, NULL, NULL, avg, &ng);
    if (rc == SCC_ERR_INVALID && ng > 0 && (ng < 2 || ng >= N))
        Rf_error("$ operator is invalid for atomic vectors");
    check(rc);
    double s = 0.0;
    for (int k = 0; k < ng; ++k) s += avg[k];
    return Rf_ScalarReal(s / ng);
}

/* n from the length of a "dist" body, n (n - 1) / 2 */
static int64_t dist_n(SEXP d)
{
    const double nd = (double)XLENGTH(d);
    int64_t n = (int64_t)((1.0 + sqrt(1.0 + 8.0 * nd)) / 2.0 + 0.5);
    if (n * (n - 1) / 2 != (int64_t)XLENGTH(d)) Rf_error("scConsensus engine: not a dist body (length %.0f)", nd);
    return n;
}

/* cutreeDynamic(dendro, distM = as.matrix(d), deepSplit, pamStage = FALSE,
 * minClusterSize) with method "hybrid" and the default cut height
 * (Fast:421-427), on the packed d: merge is the hclust merge matrix ((n-1) x 2
 * integer, column-major as R stores it), height its heights.  Returns the
 * integer labels (0 = unassigned, 1.. by decreasing size), as cutreeDynamic. */
SEXP C_scc_cutree(SEXP merge, SEXP height, SEXP d, SEXP deep, SEXP minsize)
{
    const int64_t n = dist_n(d);
    if (XLENGTH(merge) != 2 * (n - 1) || XLENGTH(height) != n - 1)
        Rf_error("scConsensus engine: merge / height do not match the dist of %lld cells", (long long)n);
    SEXP m = PROTECT(Rf_coerceVector(merge, INTSXP));
    SEXP lab = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_cutree_hybrid(INTEGER(m), REAL(height), n, REAL(d), Rf_asInteger(deep), Rf_asInteger(minsize),
                                     INTEGER(lab), NULL);
    UNPROTECT(2);
    if (rc != SCC_OK) Rf_error("scConsensus engine: cutree failed (%d)", rc);
    return lab;
}

/* hclust(d, method = "ward.D2") (Fast:406-411): list(merge, height, order) of
 * an R hclust object (the wrapper adds labels / method / call / dist.method) */
SEXP C_scc_hclust(SEXP d)
{
    const int64_t n = dist_n(d);
    SEXP merge = PROTECT(Rf_allocMatrix(INTSXP, (int)(n - 1), 2));
    SEXP height = PROTECT(Rf_allocVector(REALSXP, n - 1));
    SEXP order = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_hclust_ward_d2(REAL(d), n, INTEGER(merge), REAL(height), INTEGER(order));
    if (rc != SCC_OK) {
        UNPROTECT(3);
        Rf_error("scConsensus engine: hclust failed (%d)", rc);
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, merge);
    SET_VECTOR_ELT(out, 1, height);
    SET_VECTOR_ELT(out, 2, order);
    UNPROTECT(4);
    return out;
}

/* C_scc_distance with the output kept in the engine (HBM-resident, read by
 * C_scc_hclust_dev / C_scc_cutree_dev / C_scc_si): returns the cell count */
SEXP C_scc_distance_dev(SEXP h, SEXP genes, SEXP metric, SEXP ncomp)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int k = 0; k < nu; ++k) {
        g0[k] = INTEGER(genes)[k] - 1;
        if (g0[k] < 0 || g0[k] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[k] + 1);
    }
    check(scc_distance(g_ctx, ds, g0, nu, Rf_asInteger(metric), Rf_asInteger(ncomp), NULL, SCC_PTR_DEVICE, 0));
    return Rf_ScalarInteger(N);
}

/* C_scc_hclust on the engine-kept distance of n cells (scc_hclust_ward_d2_dev:
 * the same merge / height / order as C_scc_hclust on the same values) */
SEXP C_scc_hclust_dev(SEXP n_cells)
{
    ensure_ctx();
    const int64_t n = Rf_asInteger(n_cells);
    if (n < 2) Rf_error("scConsensus engine: hclust needs at least two cells");
    SEXP merge = PROTECT(Rf_allocMatrix(INTSXP, (int)(n - 1), 2));
    SEXP height = PROTECT(Rf_allocVector(REALSXP, n - 1));
    SEXP order = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_hclust_ward_d2_dev(g_ctx, n, NULL, 0, INTEGER(merge), REAL(height), INTEGER(order));
    if (rc != SCC_OK) {
        UNPROTECT(3);
        check(rc);
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, merge);
    SET_VECTOR_ELT(out, 1, height);
    SET_VECTOR_ELT(out, 2, order);
    UNPROTECT(4);
    return out;
}

/* C_scc_cutree with distM read from the engine-kept distance (scc_cutree_hybrid_dev) */
SEXP C_scc_cutree_dev(SEXP merge, SEXP height, SEXP deep, SEXP minsize)
{
    ensure_ctx();
    const int64_t n = (int64_t)XLENGTH(height) + 1;
    if (XLENGTH(merge) != 2 * (n - 1))
        Rf_error("scConsensus engine: merge / height do not match (%lld cells)", (long long)n);
    SEXP m = PROTECT(Rf_coerceVector(merge, INTSXP));
    SEXP lab = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_cutree_hybrid_dev(g_ctx, INTEGER(m), REAL(height), n, NULL, 0, Rf_asInteger(deep),
                                         Rf_asInteger(minsize), INTEGER(lab), NULL);
    UNPROTECT(2);
    check(rc);
    return lab;
}

/* The PCA half of C_scc_distance alone (scc_pca_scores): the scores stay in the
 * engine for C_scc_hclust_scores / C_scc_cutree_scores, no distance is computed
 * or kept: returns the cell count */
SEXP C_scc_pca_scores(SEXP h, SEXP genes, SEXP ncomp)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int k = 0; k < nu; ++k) {
        g0[k] = INTEGER(genes)[k] - 1;
        if (g0[k] < 0 || g0[k] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[k] + 1);
    }
    check(scc_pca_scores(g_ctx, ds, g0, nu, Rf_asInteger(ncomp)));
    return Rf_ScalarInteger(N);
}

/* sccKnn: the PCA of C_scc_pca_scores (prcomp_irlba(n = ncomp) of the reference
 * README's example), then the exact k nearest other cells of every cell under
 * dist(scores[, 1:dims]) (scc_knn_scores: no N x N matrix).  Returns
 * list(indexes, distances), N x k matrices, indexes 1-based, each row ordered
 * by (distance, index); the cell itself is not listed (the R wrapper adds it). */
SEXP C_scc_knn(SEXP h, SEXP genes, SEXP ncomp, SEXP dims, SEXP k)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes), kk = Rf_asInteger(k);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int q = 0; q < nu; ++q) {
        g0[q] = INTEGER(genes)[q] - 1;
        if (g0[q] < 0 || g0[q] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[q] + 1);
    }
    if (kk < 1 || kk > N - 1) Rf_error("scConsensus engine: k = %d neighbours of %d cells", kk, N);
    check(scc_pca_scores(g_ctx, ds, g0, nu, Rf_asInteger(ncomp)));
    int32_t* idx = (int32_t*)R_alloc((size_t)N * kk, sizeof(int32_t)); /* row-major [N][k] */
    double* dist = (double*)R_alloc((size_t)N * kk, sizeof(double));
    check(scc_knn_scores(g_ctx, N, NULL, Rf_asInteger(dims), kk, idx, dist));
    SEXP ri = PROTECT(Rf_allocMatrix(INTSXP, N, kk));
    SEXP rd = PROTECT(Rf_allocMatrix(REALSXP, N, kk));
    for (int i = 0; i < N; ++i)
        for (int s = 0; s < kk; ++s) { /* R matrices are column-major */
            INTEGER(ri)[(size_t)s * N + i] = idx[(size_t)i * kk + s] + 1;
            REAL(rd)[(size_t)s * N + i] = dist[(size_t)i * kk + s];
        }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SET_VECTOR_ELT(out, 0, ri);
    SET_VECTOR_ELT(out, 1, rd);
    UNPROTECT(3);
    return out;
}

/* sccUmap: the PCA of C_scc_pca_scores, then scc_umap_scores on the kept scores
 * (the neighbour search, the fuzzy simplicial set and the layout without the
 * table or the graph leaving the device).  par: numeric(9) = n_epochs, a, b,
 * gamma, negative_sample_rate, learning_rate, set_op_mix_ratio, seed (below
 * 2^53), unused; init: an N x 2 numeric matrix or NULL (the first two score
 * columns scaled to a largest absolute coordinate of 10).  Returns the N x 2
 * layout. */
SEXP C_scc_umap(SEXP h, SEXP genes, SEXP ncomp, SEXP dims, SEXP n_neighbors, SEXP par, SEXP init)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes), nn = Rf_asInteger(n_neighbors);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int q = 0; q < nu; ++q) {
        g0[q] = INTEGER(genes)[q] - 1;
        if (g0[q] < 0 || g0[q] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[q] + 1);
    }
    if (nn < 2 || nn > N) Rf_error("scConsensus engine: n_neighbors = %d of %d cells", nn, N);
    if (LENGTH(par) < 8) Rf_error("scConsensus engine: C_scc_umap needs 8 parameters");
    const double* pv = REAL(par);
    scc_umap_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.local_connectivity = 1.0;
    prm.bandwidth = 1.0;
    prm.n_epochs = (int32_t)pv[0];
    prm.a = pv[1];
    prm.b = pv[2];
    prm.gamma = pv[3];
    prm.negative_sample_rate = (int32_t)pv[4];
    prm.learning_rate = pv[5];
    prm.set_op_mix_ratio = pv[6];
    prm.seed = (uint64_t)pv[7];
    double* y0 = NULL;
    if (!Rf_isNull(init)) { /* column-major N x 2 -> [N][2] */
        if (LENGTH(init) != 2 * N) Rf_error("scConsensus engine: init must be an N x 2 matrix");
        y0 = (double*)R_alloc((size_t)N * 2, sizeof(double));
        for (int i = 0; i < N; ++i) {
            y0[2 * (size_t)i] = REAL(init)[i];
            y0[2 * (size_t)i + 1] = REAL(init)[(size_t)N + i];
        }
    }
    check(scc_pca_scores(g_ctx, ds, g0, nu, Rf_asInteger(ncomp)));
    double* y = (double*)R_alloc((size_t)N * 2, sizeof(double));
    check(scc_umap_scores(g_ctx, N, NULL, Rf_asInteger(dims), nn, &prm, y0, y, NULL, NULL, NULL, 0, NULL));
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, N, 2));
    for (int i = 0; i < N; ++i) {
        REAL(out)[i] = y[2 * (size_t)i];
        REAL(out)[(size_t)N + i] = y[2 * (size_t)i + 1];
    }
    UNPROTECT(1);
    return out;
}

/* sccFindClusters: the PCA of C_scc_pca_scores, then scc_snn_clusters_scores on
 * the kept scores (the neighbour search, the SNN graph and the modularity
 * clustering without the table or the graph leaving the device).  par:
 * numeric(2) = prune, resolution.  Returns list(labels = integer(N), 0-based
 * with 0 the largest cluster, modularity, sweeps = the sweeps run per level). */
SEXP C_scc_find_clusters(SEXP h, SEXP genes, SEXP ncomp, SEXP dims, SEXP k_param, SEXP par)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes), kp = Rf_asInteger(k_param);
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int q = 0; q < nu; ++q) {
        g0[q] = INTEGER(genes)[q] - 1;
        if (g0[q] < 0 || g0[q] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[q] + 1);
    }
    if (kp < 2 || kp > N) Rf_error("scConsensus engine: k.param = %d of %d cells", kp, N);
    if (LENGTH(par) < 2) Rf_error("scConsensus engine: C_scc_find_clusters needs 2 parameters");
    check(scc_pca_scores(g_ctx, ds, g0, nu, Rf_asInteger(ncomp)));
    SEXP labels = PROTECT(Rf_allocVector(INTSXP, N));
    int32_t n_clusters = 0, n_levels = 0, sweeps[SCC_MODULARITY_MAX_LEVELS];
    double q = 0.0;
    check(scc_snn_clusters_scores(g_ctx, N, NULL, Rf_asInteger(dims), kp, REAL(par)[0], REAL(par)[1],
                                  (int32_t*)INTEGER(labels), &n_clusters, &q, &n_levels, sweeps, NULL, NULL, NULL, 0,
                                  NULL));
    SEXP sw = PROTECT(Rf_allocVector(INTSXP, n_levels));
    for (int l = 0; l < n_levels; ++l) INTEGER(sw)[l] = sweeps[l];
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, labels);
    SET_VECTOR_ELT(out, 1, Rf_ScalarReal(q));
    SET_VECTOR_ELT(out, 2, sw);
    UNPROTECT(3);
    return out;
}

/* hclust(dist(scores), "ward.D2") from the engine-kept scores of n cells
 * (scc_hclust_ward_d2_scores: no N x N matrix anywhere) */
SEXP C_scc_hclust_scores(SEXP n_cells)
{
    ensure_ctx();
    const int64_t n = Rf_asInteger(n_cells);
    if (n < 2) Rf_error("scConsensus engine: hclust needs at least two cells");
    SEXP merge = PROTECT(Rf_allocMatrix(INTSXP, (int)(n - 1), 2));
    SEXP height = PROTECT(Rf_allocVector(REALSXP, n - 1));
    SEXP order = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_hclust_ward_d2_scores(g_ctx, n, NULL, INTEGER(merge), REAL(height), INTEGER(order));
    if (rc != SCC_OK) {
        UNPROTECT(3);
        check(rc);
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SET_VECTOR_ELT(out, 0, merge);
    SET_VECTOR_ELT(out, 1, height);
    SET_VECTOR_ELT(out, 2, order);
    UNPROTECT(4);
    return out;
}

/* C_scc_cutree with distM computed from the engine-kept scores (scc_cutree_hybrid_scores) */
SEXP C_scc_cutree_scores(SEXP merge, SEXP height, SEXP deep, SEXP minsize)
{
    ensure_ctx();
    const int64_t n = (int64_t)XLENGTH(height) + 1;
    if (XLENGTH(merge) != 2 * (n - 1))
        Rf_error("scConsensus engine: merge / height do not match (%lld cells)", (long long)n);
    SEXP m = PROTECT(Rf_coerceVector(merge, INTSXP));
    SEXP lab = PROTECT(Rf_allocVector(INTSXP, n));
    const int rc = scc_cutree_hybrid_scores(g_ctx, INTEGER(m), REAL(height), n, NULL, Rf_asInteger(deep),
                                            Rf_asInteger(minsize), INTEGER(lab), NULL);
    UNPROTECT(2);
    check(rc);
    return lab;
}

/* The heatmap's gene rows (cellTypeDEPlot.R:225-253: Heatmap(cluster_rows = TRUE)):
 * dist() of the union's rows over all cells on the device (scc_gene_distance),
 * hclust "complete" and ComplexHeatmap's reorder by -rowMeans on the host
 * (scc_hclust_complete, scc_dendro_reorder).  Returns list(merge, height, order,
 * range = c(min x, max x, min |x|, max |x|), rowMeans); merge is the reordered
 * one (as.dendrogram takes it; it no longer lists singletons first). */
SEXP C_scc_heatmap_rows(SEXP h, SEXP genes)
{
    ensure_ctx();
    int G = 0, N = 0;
    scc_dataset* ds = ds_of(h, &G, &N);
    const int nu = LENGTH(genes);
    if (nu < 2) Rf_error("scConsensus engine: the row tree needs at least two genes");
    int32_t* g0 = (int32_t*)R_alloc((size_t)nu, sizeof(int32_t));
    for (int k = 0; k < nu; ++k) {
        g0[k] = INTEGER(genes)[k] - 1;
        if (g0[k] < 0 || g0[k] >= G) Rf_error("scConsensus engine: gene row %d out of range", g0[k] + 1);
    }
    double* d = (double*)R_alloc((size_t)nu * (size_t)(nu - 1) / 2, sizeof(double));
    double* w = (double*)R_alloc((size_t)nu, sizeof(double));
    int32_t* m0 = (int32_t*)R_alloc(2 * (size_t)(nu - 1), sizeof(int32_t));
    SEXP merge = PROTECT(Rf_allocMatrix(INTSXP, nu - 1, 2));
    SEXP height = PROTECT(Rf_allocVector(REALSXP, nu - 1));
    SEXP order = PROTECT(Rf_allocVector(INTSXP, nu));
    SEXP range = PROTECT(Rf_allocVector(REALSXP, 4));
    SEXP means = PROTECT(Rf_allocVector(REALSXP, nu));
    int rc = scc_gene_distance(g_ctx, ds, g0, nu, d, REAL(means), REAL(range));
    if (rc == SCC_OK) rc = scc_hclust_complete(d, nu, m0, REAL(height), NULL);
    if (rc == SCC_OK) {
        for (int k = 0; k < nu; ++k) w[k] = -REAL(means)[k];
        rc = scc_dendro_reorder(m0, nu, w, INTEGER(merge), INTEGER(order));
    }
    if (rc != SCC_OK) {
        UNPROTECT(5);
        check(rc);
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 5));
    SET_VECTOR_ELT(out, 0, merge);
    SET_VECTOR_ELT(out, 1, height);
    SET_VECTOR_ELT(out, 2, order);
    SET_VECTOR_ELT(out, 3, range);
    SET_VECTOR_ELT(out, 4, means);
    UNPROTECT(6);
    return out;
}

static const R_CallMethodDef call_methods[] = {
    {"C_scc_heatmap_rows", (DL_FUNC)&C_scc_heatmap_rows, 2},
    {"C_scc_dataset", (DL_FUNC)&C_scc_dataset, 4},
    {"C_scc_release", (DL_FUNC)&C_scc_release, 1},
    {"C_scc_de_fast", (DL_FUNC)&C_scc_de_fast, 8},
    {"C_scc_de_slow", (DL_FUNC)&C_scc_de_slow, 6},
    {"C_scc_markers", (DL_FUNC)&C_scc_markers, 8},
    {"C_scc_distance", (DL_FUNC)&C_scc_distance, 4},
    {"C_scc_si", (DL_FUNC)&C_scc_si, 1},
    {"C_scc_devices", (DL_FUNC)&C_scc_devices, 1},
    {"C_scc_cutree", (DL_FUNC)&C_scc_cutree, 5},
    {"C_scc_hclust", (DL_FUNC)&C_scc_hclust, 1},
    {"C_scc_distance_dev", (DL_FUNC)&C_scc_distance_dev, 4},
    {"C_scc_hclust_dev", (DL_FUNC)&C_scc_hclust_dev, 1},
    {"C_scc_cutree_dev", (DL_FUNC)&C_scc_cutree_dev, 4},
    {"C_scc_pca_scores", (DL_FUNC)&C_scc_pca_scores, 3},
    {"C_scc_hclust_scores", (DL_FUNC)&C_scc_hclust_scores, 1},
    {"C_scc_cutree_scores", (DL_FUNC)&C_scc_cutree_scores, 4},
    {"C_scc_si_scores", (DL_FUNC)&C_scc_si_scores, 1},
    {"C_scc_knn", (DL_FUNC)&C_scc_knn, 5},
    {"C_scc_umap", (DL_FUNC)&C_scc_umap, 7},
    {"C_scc_find_clusters", (DL_FUNC)&C_scc_find_clusters, 6},
    {NULL, NULL, 0}};

/* the package is scConsensus (NAMESPACE: useDynLib(scConsensus, .registration = TRUE)) */
void R_init_scConsensus(DllInfo* dll)
{
    R_registerRoutines(dll, NULL, call_methods, NULL, NULL);
    R_useDynamicSymbols(dll, FALSE);
}
