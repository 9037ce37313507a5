// scc_de.cpp — the DE driver behind scc_de_run and the gene-shard / record
// entry points (include/scc.h): one engine run as a list of phases (de_run),
// the device-list run, the group-pair runs for K > 128, the one-vs-rest marker
// run (scc_de_markers: its own phase list over the same phases), the result
// accessors.
//
// The whole DE stage is one stream-ordered launch sequence (the bigger genes
// run on a side stream concurrently with the LDS-resident ones); the host
// synchronises once per call to read the union size.
#include "scc_internal.hpp"

#include <array>
#include <cstring>
#include <memory>
#include <thread>

using namespace scc_rt;

// stage DE_FULL: the whole DE for genes [glo, ghi) (all genes: scc_de_run).
// stage DE_SHARD: the per-(pair, gene) stage for the gene shard [glo, ghi),
//   packed into `shard` (zero outside the shard, so the shards of all ranks
//   combine by an integer sum: scc_de_shard_bytes layout) -- no selection.
// stage DE_FINISH: `shard` holds every gene's (pair, gene) cells (the sum of
//   all ranks' shards); per-pair BH, filters, top-N and the union, on the
//   context that ran this rank's DE_SHARD for the same inputs.
// stage DE_SHARD_REC / DE_FINISH_REC: the same with the compact exchange
//   (scc_de_record per tested (pair, gene) cell; scc_exchange.hip).
enum { DE_FULL = 0, DE_SHARD = 1, DE_FINISH = 2, DE_SHARD_REC = 3, DE_FINISH_REC = 4 };

extern "C" {
int scc_rec_blocks(long long cells);
hipError_t scc_launch_rec_count(const uint8_t* flags, int G, int P, int glo, int ghi, int all, uint32_t* cnt,
                                hipStream_t st);
hipError_t scc_launch_rec_pack(const uint8_t* flags, int G, int P, int glo, int ghi, int all, const long long* off,
                               const double* p, const double* lfc, const double* pct1, const double* pct2,
                               const long long* u2, const long long* t, scc_de_record* out, hipStream_t st);
hipError_t scc_launch_rec_scatter(const scc_de_record* rec, long long n, int G, int P, double* p, double* lfc,
                                  double* pct1, double* pct2, long long* u2, long long* t, uint8_t* flags, int* err,
                                  int plo, int phi, hipStream_t st);
}

struct RecIO {  // the compact exchange's buffers (DE_SHARD_REC out, DE_FINISH_REC in)
    void* out = nullptr;
    int64_t cap = 0;
    int64_t* n_out = nullptr;
    const void* in = nullptr;
    const int64_t* counts = nullptr;
    int nblocks = 0;
    int64_t stride = 0;
    // DE_FINISH_REC for pairs [pair_lo, pair_hi) only: the per-gene first
    // occurrence keys go to first_out (device u64 [G]) and no result is built
    int pair_lo = 0, pair_hi = 0;
    void* first_out = nullptr;
};

extern "C" void scc_rank_split_diag(hipStream_t st, int ngenes);

// which ingest a compute stage takes (the values scc_diag_ingest_last_path reports)
enum IngestRoute {
    INGEST_NONE = 0,    // a finish stage
    INGEST_FULL = 1,    // every entry read and checked (the validating call, SLOW, dense, SCC_INGEST_FULL)
    INGEST_LEAN = 2,    // the transpose of a validated dataset: a gene shard's tiles, or the row indices only
    INGEST_MIRROR = 3,  // the regroup of the dataset's gene-major mirror
};

// everything one engine run decides on the host before its first launch
struct DePlan {
    const scc_dataset* ds;
    const scc_de_params* prm;
    void* shard;       // DE_SHARD out / DE_FINISH in
    const RecIO* rio;  // DE_SHARD_REC / DE_FINISH_REC
    int stage;
    bool shard_stage, finish_stage;
    bool pairs_only;  // DE_FINISH_REC for rio's pair range only: first-occurrence keys out, no result
    int G, N, K, P, glo, ghi;
    int64_t GK, nnz1;
    size_t PG;
    bool fast, norank, all_pairs;
    bool markers;  // the one-vs-rest run (scc_de_markers): P = K "pairs", its own rank kernel, no all-pairs rank lists
    int test;
    std::vector<int> nclu;
    // the host cell tables (c->host_tables; not in a finish stage): sizes and offsets
    int nkept, nc, nc_kept, ns, gt, ntile, nwaves;
    size_t o_ccp0, o_cccode, o_sccc0, o_clcc, o_nclu, o_code8, tab_n;
    // rank work items (LDS capacities depend on the tested-pair list size)
    int ntp_max, cap_s, cap_m, wave_target, bucket_cap, item_cap, bucket_target;
    size_t acc_n;  // rank accumulators: S, E, X per (pair, gene), F per (cluster, gene)
    bool resplit, stamps;  // SCC_RESPLIT, SCC_STAMPS (they size rank buffers)
    int fat_cap;
    IngestRoute route;  // without the mirror; ensure_mirror sets INGEST_MIRROR
    bool try_mirror;
    // decided once per run, after ensure_mirror (de_run): the rank stage walks the
    // dataset's value order; the statistics come from the mirror, no regroup
    bool vorder, stats_mirror;
    // ... and forms the cross-bucket term per run (rank_runs_route)
    bool rank_runs;
    double log_thr;  // SLOW (set by slow_threshold; a finish stage: the shard run's)
};

// the device buffers of one run: named slots of the context's grow-only workspace
struct DeBuffers {
    int *d_tab, *d_nodg, *d_splitg, *d_counts, *d_err, *d_tested, *d_union, *d_nu, *d_genebk;
    const int *d_perm, *d_ccp0, *d_cccode, *d_sccc0, *d_clcc, *d_nclu;  // views into d_tab
    const signed char* d_code8;                                         // (the codes as int8: the mirror's regroup)
    uint32_t *d_cnt, *d_cntpos, *d_cntneg, *d_gix, *d_gwin, *d_cscr;
    long long *d_gstart, *d_scan, *d_rowoff, *d_bnd;
    unsigned long long *d_keys, *d_keys2, *d_acc, *d_gkmin, *d_first;
    unsigned long long *accS, *accE, *accX, *accF;  // views into d_acc
    uint8_t *d_gcode, *d_gsc, *d_codes2, *d_flags;
    ScRankItem *d_items, *d_sbk;
    unsigned int* d_hbg;
    dd *d_wexp, *d_gexp;
    dd* d_sume;  // [K][G] undivided expm1 sums (the one-vs-rest run only; else nullptr)
    double *d_mx, *d_me, *d_vx, *d_mpos, *d_m2pos, *d_minpos, *d_maxpos;
    double *d_p, *d_lfc, *d_pct1, *d_pct2;
    long long *d_u2, *d_t;
    // rank stage: split genes' tested pairs, HBM tested-pair tables, re-split lists, diagnostic stamps
    uint32_t* gene_tp;
    int* gene_nt;
    char* tp_scr;
    ScRankItem *fatbk, *fat2;
    int4 *rsseg, *fatg;
    unsigned long long* st_buf;
    // record packer (DE_SHARD_REC)
    uint32_t* d_rc;
    long long *d_roff, *d_rscr;
    // rows (FAST) / per-pair vectors (SLOW) and the selection's scratch
    int* d_row_gene;
    double *d_row_p, *d_row_q, *d_row_lfc, *d_row_pct1, *d_row_pct2;
    long long *d_row_u2, *d_row_t;
    uint8_t* d_row_flags;
    double* d_slow_q;
    uint8_t* d_slow_de;
    void *d_rec, *d_key;
};

// error-word bit 0x20 (k_pair_test): the bimod p of a cell its pair tests is NaN
static const char kBimodNaN[] =
    "bimod: the p-value of a tested gene is NaN (constant positive values in both clusters and pooled: "
    "lrt = Inf - Inf); R's NA p_val_adj ends in stop() at dataMatrix[deGeneUnion, ]";

// The device error word at each exit of a run, as return code and message.
// Input and test conditions (1, 2, 4, 8, 0x20) where ingest and tests can
// have run; 16 (a record out of range) where records were scattered, under the
// name of the entry point called; 0x200 (k_pair_select) last -- at the full
// exit only after the result has been handed out (AT_RESULT).  Bit 0x100 (FAST
// NA q in a kept pair: R builds NA rows and does not stop) is informational.
enum DeExit { AT_SHARD, AT_PAIRS, AT_FULL, AT_RESULT };
static int de_error(scc_ctx* c, int e, DeExit at)
{
    if (at == AT_SHARD || at == AT_FULL) {
        if (e & 1) return fail(c, SCC_ERR_NONFINITE, "input holds non-finite values");
        if (e & 2) return fail(c, SCC_ERR_INVALID, "row index out of range");
        if (e & 4) return fail(c, SCC_ERR_INVALID, "row indices not strictly increasing within a column (dgCMatrix)");
        if (e & 8) return fail(c, SCC_ERR_RSTOP, "t.test: data are essentially constant (R stop())");
        if (e & 0x20) return fail(c, SCC_ERR_RSTOP, kBimodNaN);
    }
    if (at == AT_FULL && (e & 16)) return fail(c, SCC_ERR_INVALID, "scc_de_finish_records: record out of range");
    if (at == AT_PAIRS && (e & 16)) return fail(c, SCC_ERR_INVALID, "scc_de_finish_records_pairs: record out of range");
    // SLOW NA in the DE logical vector (slow:165-186)
    if ((at == AT_PAIRS || at == AT_RESULT) && (e & 0x200))
        return fail(c, SCC_ERR_RSTOP, "NA in the DE logical vector: R stops at if(sum(...) <= 1)");
    return SCC_OK;
}

// cluster sizes (host: the codes are a host array at the R boundary)
static int cluster_sizes(scc_ctx* c, const int32_t* code, int64_t N, int K, bool fast, std::vector<int>& nclu)
{
    nclu.assign(K, 0);
    for (int64_t i = 0; i < N; ++i) {
        const int a = code[i];
        if (a < -1 || a >= K) return fail(c, SCC_ERR_INVALID, "code out of range");
        if (a >= 0) nclu[a]++;
    }
    for (int a = 0; a < K; ++a) {
        if (nclu[a] == 0) return fail(c, SCC_ERR_INVALID, "empty cluster");
        // ComputePairWiseDE: min.cells.group = 3 (Fast:76,208-213)
        if (fast && nclu[a] < 3) return fail(c, SCC_ERR_RSTOP, "cluster has fewer than 3 cells (R stop())");
    }
    return SCC_OK;
}

static int de_check_args(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                         int stage, void* shard, scc_de_result** out, const RecIO* rio)
{
    const bool shard_stage = stage == DE_SHARD || stage == DE_SHARD_REC;
    if (!c || !ds || !code || !prm || (!shard_stage && !out && !(rio && rio->first_out)) || ((stage == DE_SHARD || stage == DE_FINISH) && !shard) ||
        ((stage == DE_SHARD_REC || stage == DE_FINISH_REC) && !rio))
        return fail(c, SCC_ERR_INVALID, "scc_de_run: null argument");
    if (out) *out = nullptr;
    if (ds->ctx != c) return fail(c, SCC_ERR_INVALID, "dataset belongs to another context");
    if (prm->mode != SCC_DE_FAST && prm->mode != SCC_DE_SLOW) return fail(c, SCC_ERR_INVALID, "bad mode");
    if (prm->test != SCC_TEST_WILCOX &&
        ((prm->test != SCC_TEST_T && prm->test != SCC_TEST_BIMOD) || prm->mode != SCC_DE_FAST))
        return fail(c, SCC_ERR_INVALID, "test: SCC_TEST_WILCOX, or SCC_TEST_T / SCC_TEST_BIMOD with SCC_DE_FAST");
    if (K < 2) return fail(c, SCC_ERR_INVALID, "need at least two clusters");
    if (K > kMaxK)
        return fail(c, SCC_ERR_UNSUPPORTED,
                    "K > 128 clusters: one engine run holds 128 (scc_de_run cuts larger K into group-pair runs; "
                    "the gene-shard entry points do not)");
    return SCC_OK;
}

// Cells in cluster order: kept cells by code, then unkept ones.  Count
// chunks of <= kCountChunk cells never straddle clusters; scatter chunks
// group <= scatter_cc count chunks of one cluster.  H: the permutation, the
// chunk tables, the cluster sizes and the codes as int8; their offsets to pl.
static void cell_tables(const int32_t* code, int N, int K, const std::vector<int>& nclu, int scatter_cc,
                        std::vector<int>& H, DePlan* pl)
{
    std::vector<int> start(K + 1, 0);
    for (int a = 0; a < K; ++a) start[a + 1] = start[a] + nclu[a];
    const int nkept = start[K];
    std::vector<int> perm(N), fill(start.begin(), start.end() - 1);
    int u = nkept;
    for (int i = 0; i < N; ++i) perm[code[i] >= 0 ? fill[code[i]]++ : u++] = i;
    std::vector<int> cc_p0, cc_code, sc_cc0, cl_cc(K + 1);
    for (int a = 0; a < K; ++a) {
        cl_cc[a] = (int)cc_code.size();
        for (int p = start[a]; p < start[a + 1]; p += kCountChunk) {
            cc_p0.push_back(p);
            cc_code.push_back(a);
        }
    }
    const int nc_kept = (int)cc_code.size();
    cl_cc[K] = nc_kept;
    for (int a = 0; a < K; ++a)
        for (int q = cl_cc[a]; q < cl_cc[a + 1]; q += scatter_cc) sc_cc0.push_back(q);
    const int ns = (int)sc_cc0.size();
    sc_cc0.push_back(nc_kept);
    for (int p = nkept; p < N; p += kCountChunk) {
        cc_p0.push_back(p);
        cc_code.push_back(-1);
    }
    const int nc = (int)cc_code.size();
    cc_p0.push_back(N);
    H.clear();
    H.insert(H.end(), perm.begin(), perm.end());
    pl->o_ccp0 = H.size();
    H.insert(H.end(), cc_p0.begin(), cc_p0.end());
    pl->o_cccode = H.size();
    H.insert(H.end(), cc_code.begin(), cc_code.end());
    pl->o_sccc0 = H.size();
    H.insert(H.end(), sc_cc0.begin(), sc_cc0.end());
    pl->o_clcc = H.size();
    H.insert(H.end(), cl_cc.begin(), cl_cc.end());
    pl->o_nclu = H.size();
    H.insert(H.end(), nclu.begin(), nclu.end());
    // the cells' codes as int8 (-1: unkept; K <= 128), for the mirror's regroup
    pl->o_code8 = H.size();
    H.resize(pl->o_code8 + ((size_t)N + 3) / 4, 0);
    signed char* c8 = (signed char*)(H.data() + pl->o_code8);
    for (int i = 0; i < N; ++i) c8[i] = (signed char)code[i];
    pl->nkept = nkept, pl->nc = nc, pl->nc_kept = nc_kept, pl->ns = ns, pl->tab_n = H.size();
}

// Cluster validation and the run's plan.  A finish stage reads no cell order
// (the shards / records carry every statistic): it builds no host tables.
static int de_plan(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                   int stage, int64_t glo64, int64_t ghi64, void* shard, const RecIO* rio, DePlan* p)
{
    p->ds = ds, p->prm = prm, p->shard = shard, p->rio = rio, p->stage = stage;
    p->shard_stage = stage == DE_SHARD || stage == DE_SHARD_REC;
    p->finish_stage = stage == DE_FINISH || stage == DE_FINISH_REC;
    p->pairs_only = rio && rio->first_out;
    const int G = p->G = (int)ds->G, N = p->N = (int)ds->N;
    p->K = K, p->P = K * (K - 1) / 2;
    const bool fast = p->fast = prm->mode == SCC_DE_FAST;
    int rc = cluster_sizes(c, code, N, K, fast, p->nclu);
    if (rc) return rc;
    if (glo64 < 0 || ghi64 > G || glo64 > ghi64) return fail(c, SCC_ERR_INVALID, "gene shard out of range");
    p->glo = (int)glo64, p->ghi = (int)ghi64;
    p->GK = (int64_t)G * K;
    p->PG = (size_t)p->P * G;
    p->nnz1 = std::max<int64_t>(ds->nnz, 1);
    const bool ttest = fast && prm->test == SCC_TEST_T;  // DiffTTest (Fast:185-196): no rank stage
    const bool bimod = fast && prm->test == SCC_TEST_BIMOD;  // DiffExpTest (Fast:93-133): moments of x > 0
    p->norank = ttest || bimod;  // both tests are functions of per-(gene, cluster) moments
    p->test = ttest ? SCC_TEST_T : bimod ? SCC_TEST_BIMOD : SCC_TEST_WILCOX;
    p->all_pairs = !fast || prm->test_all;
    p->acc_n = 3 * p->PG + (size_t)p->GK;
    if (p->finish_stage) return SCC_OK;
    // scatter chunks of 2 count chunks (64 cells) when a cell has >= 16 stored
    // values per gene tile (config B / D: ~29; ingest B 0.45 -> 0.40 ms, D 5.97
    // -> 5.79), else 8 (config E: ~8 per tile, where small chunks leave the
    // workgroups too little work for their fixed cost: 64 cells 16.5 ms, 128
    // cells 12.0-12.2, 192 cells 11.0, 256 cells 10.4-10.5, round 6); SCC_SC_CC overrides
    const int64_t ntile_h = (ds->G + scc_ingest_gene_tile() - 1) / scc_ingest_gene_tile();
    const bool dense_tiles = ds->nnz >= 16 * (int64_t)std::max(1, N) * std::max<int64_t>(1, ntile_h);
    const int scatter_cc =
        std::min(kScatterCC, std::max(1, env_int("SCC_SC_CC", dense_tiles ? 2 : kScatterCC)));
    cell_tables(code, N, K, p->nclu, scatter_cc, c->host_tables, p);
    p->gt = scc_ingest_gene_tile();
    p->ntile = (G + p->gt - 1) / p->gt;
    p->nwaves = p->nc * SCC_ING_HIST_WAVES;
    p->ntp_max = p->P;
    // small items: 4 workgroups per CU; medium: 2 per CU (LDS budget per workgroup)
    p->cap_s = scc_rank_item_cap(0, env_int("SCC_CAP_SMALL", kCapSmall), p->ntp_max, K, 40 * 1024);
    p->cap_m = std::max(p->cap_s, scc_rank_item_cap(1, env_int("SCC_CAP_MEDIUM", kCapMedium), p->ntp_max, K, 80 * 1024));
    p->wave_target = 32;  // value buckets of < 64 elements: one wave each
    p->bucket_cap = (int)std::min<int64_t>(3 * p->nnz1 / p->wave_target + 2 * (int64_t)G + 64, 1 << 29);
    p->item_cap = p->bucket_cap;
    p->bucket_target = std::max(64, p->cap_m / 2);
    p->resplit = env_int("SCC_RESPLIT", 1) != 0;
    p->fat_cap = (int)std::min<int64_t>(p->nnz1 / 64 + 64, 1 << 28);
    p->stamps = env_int("SCC_STAMPS", 0) != 0;
    // The ingest route.  A validated sparse dataset, FAST: a gene shard reads
    // its tiles only; all genes of a dataset without explicit zeros: the
    // counting pass reads the row indices only (the scatter reads the CSC in
    // full).  The same runs regroup the dataset's gene-major mirror instead,
    // when it exists or can be built (ensure_mirror); SCC_INGEST_MIRROR=0
    // forces the transpose, SCC_INGEST_FULL=1 the full read.
    const char* ife = getenv("SCC_INGEST_FULL");
    const bool lean_ok = !ds->dense && ds->validated && ds->d_nodg && fast && !(ife && atoi(ife));
    p->route = lean_ok && (p->glo > 0 || p->ghi < G || ds->no_zeros) ? INGEST_LEAN : INGEST_FULL;
    p->try_mirror = lean_ok && env_int("SCC_INGEST_MIRROR", 1) != 0;
    return SCC_OK;
}

// The run's workspace buffers.  A finish stage requests only what it reads or
// writes: a request that grows a buffer reallocates it, and any reallocation
// makes the eigensolver's captured graphs unreachable (ws_gen).
static int de_alloc(scc_ctx* c, const DePlan& pl, DeBuffers* b)
{
    int rc;
    const int G = pl.G, N = pl.N, K = pl.K, P = pl.P;
    const int64_t GK = pl.GK, nnz1 = pl.nnz1;
    const size_t PG = pl.PG;
    const bool fast = pl.fast;
#define WS(name, n, ptr)                                  \
    do {                                                  \
        if ((rc = ws(c, name, (size_t)(n), &(ptr)))) return rc; \
    } while (0)
    WS("nodg", N, b->d_nodg);  // (a finish stage: the result's d_nodg is what the shard run left here)
    WS("err", 4, b->d_err);
    if (!pl.finish_stage) {
        const int nc = pl.nc, ntile = pl.ntile, nwaves = pl.nwaves, item_cap = pl.item_cap, bucket_cap = pl.bucket_cap;
        const bool ttest = pl.test == SCC_TEST_T, bimod = pl.test == SCC_TEST_BIMOD;
        WS("tables", pl.tab_n, b->d_tab);
        WS("cnt", (size_t)(nc + 1) * G, b->d_cnt);
        WS("bnd", pl.ds->dense ? 1 : (size_t)N * (ntile + 1), b->d_bnd);
        WS("gstart", G + 1, b->d_gstart);
        WS("scan", scc_scan_scratch_blocks(G) + 1, b->d_scan);
        WS("keys", nnz1, b->d_keys);
        const bool lists = !pl.markers;  // the all-pairs rank stage's work lists
        if (lists) {
            WS("gix", 2 * (size_t)nnz1, b->d_gix);
            WS("gcode", nnz1, b->d_gcode);
            WS("gwin", nnz1, b->d_gwin);
            WS("gsc", nnz1, b->d_gsc);
        }
        WS("keys2", nnz1, b->d_keys2);
        WS("codes2", nnz1, b->d_codes2);
        {
            void* p;
            if ((rc = ws_get(c, "wexp", sizeof(double) * 2 * (nwaves + 1), &p))) return rc;
            b->d_wexp = (dd*)p;
            b->d_gexp = (dd*)((char*)p + sizeof(double) * 2 * nwaves);
            if (pl.markers) {  // the clusters' undivided expm1 sums: the rest's mean divides a sum of them
                if ((rc = ws_get(c, "sum_e", sizeof(double) * 2 * (size_t)GK, &p))) return rc;
                b->d_sume = (dd*)p;
            }
        }
        // (the mirror's build and the transpose scan the count rows' columns; a regroup of a built mirror does not)
        if (!(pl.try_mirror && pl.ds->m_gptr)) WS("colscan", scc_ingest_colscan_scratch(nc, G), b->d_cscr);
        if (lists) WS("splitg", (size_t)G, b->d_splitg);
        WS("counts", SCC_NCOUNTS * SCC_CNT_STRIDE, b->d_counts);
        WS("mx", GK, b->d_mx);
        WS("me", GK, b->d_me);
        WS("cntpos", GK, b->d_cntpos);
        WS("cntneg", GK, b->d_cntneg);
        WS("vx", ttest ? GK : 1, b->d_vx);
        WS("mpos", bimod ? GK : 1, b->d_mpos);
        WS("m2pos", bimod ? GK : 1, b->d_m2pos);
        WS("minpos", bimod ? GK : 1, b->d_minpos);
        WS("maxpos", bimod ? GK : 1, b->d_maxpos);
        WS("acc", pl.acc_n, b->d_acc);
        if (lists) {
            WS("items", 3 * (size_t)item_cap, b->d_items);
            WS("sbuckets", (size_t)bucket_cap, b->d_sbk);
            WS("hbg", (size_t)bucket_cap * K, b->d_hbg);
            WS("genebk", 2 * (size_t)G, b->d_genebk);
            WS("gkmin", (size_t)G, b->d_gkmin);
        }
        if (lists && !pl.norank) {
            WS("gene_tp", (size_t)G * P, b->gene_tp);
            WS("gene_nt", (size_t)G, b->gene_nt);
            if (scc_rank_tables_global(pl.ntp_max, K)) {  // items' tested-pair tables in HBM, one slice per workgroup
                const int ncu_items = c->n_cu > 0 ? c->n_cu : 256;
                WS("tp_scr", (size_t)4 * ncu_items * scc_rank_tables_stride(pl.ntp_max, K), b->tp_scr);
            }
            if (pl.resplit) {
                WS("fatbk", (size_t)pl.fat_cap, b->fatbk);
                WS("rsseg", (size_t)pl.fat_cap, b->rsseg);
                WS("fatg", (size_t)G, b->fatg);
                WS("fat2", (size_t)pl.fat_cap, b->fat2);
            }
            if (pl.stamps) WS("d_rstamps", (size_t)3 * item_cap * 8, b->st_buf);
        }
        if (pl.stage == DE_SHARD_REC) {
            const int nb = std::max(1, scc_rec_blocks((long long)P * (pl.ghi - pl.glo)));
            WS("rec_cnt", nb, b->d_rc);
            WS("rec_off", nb + 1, b->d_roff);
            WS("rec_scr", scc_scan_scratch_blocks(nb) + 1, b->d_rscr);
        }
        b->d_perm = b->d_tab, b->d_ccp0 = b->d_tab + pl.o_ccp0, b->d_cccode = b->d_tab + pl.o_cccode;
        b->d_sccc0 = b->d_tab + pl.o_sccc0, b->d_clcc = b->d_tab + pl.o_clcc, b->d_nclu = b->d_tab + pl.o_nclu;
        b->d_code8 = (const signed char*)(b->d_tab + pl.o_code8);
        b->accS = b->d_acc, b->accE = b->d_acc + PG, b->accX = b->d_acc + 2 * PG, b->accF = b->d_acc + 3 * PG;
    }
    // the (pair, gene) fields
    WS("p", PG, b->d_p);
    WS("lfc", PG, b->d_lfc);
    WS("pct1", fast ? PG : 1, b->d_pct1);
    WS("pct2", fast ? PG : 1, b->d_pct2);
    WS("u2", PG, b->d_u2);
    WS("t", PG, b->d_t);
    WS("flags", PG, b->d_flags);
    WS("tested", P, b->d_tested);
    WS("rowoff", P + 1, b->d_rowoff);
    WS("first", G, b->d_first);
    WS("union", G, b->d_union);
    WS("nu", 4, b->d_nu);
    if (pl.shard_stage) return SCC_OK;  // no selection
    // FAST rows: one per (pair, gene) flag at most, so PG rows hold every row
    // offset count_tested can produce from any flag contents -- including the
    // stale flags a pair-range finish leaves outside its range
    const size_t rowcap = fast ? PG : 1;
    WS("row_gene", rowcap, b->d_row_gene);
    WS("row_p", rowcap, b->d_row_p);
    WS("row_q", rowcap, b->d_row_q);
    WS("row_lfc", rowcap, b->d_row_lfc);
    WS("row_pct1", rowcap, b->d_row_pct1);
    WS("row_pct2", rowcap, b->d_row_pct2);
    WS("row_u2", rowcap, b->d_row_u2);
    WS("row_t", rowcap, b->d_row_t);
    WS("row_flags", rowcap, b->d_row_flags);
    WS("slow_q", fast ? 1 : PG, b->d_slow_q);
    WS("slow_de", fast ? 1 : PG, b->d_slow_de);
    if ((rc = ws_get(c, "rec_scratch", PG * scc_select_rec_bytes(), &b->d_rec))) return rc;
    if ((rc = ws_get(c, "key_scratch", std::max<size_t>(PG, G) * scc_select_key_bytes(), &b->d_key))) return rc;
    return SCC_OK;
#undef WS
}

// the tables through a pinned buffer (an asynchronous DMA; every earlier
// DE call ended with a synchronisation, so no copy out of it is pending)
static int upload_tables(scc_ctx* c, const DeBuffers& B)
{
    const std::vector<int>& H = c->host_tables;
    const int* tab_src = H.data();
    if (c->h_tab_n < H.size()) {
        if (c->h_tab) hipHostFree(c->h_tab);
        c->h_tab = nullptr;
        c->h_tab_n = 0;
        if (hipHostMalloc((void**)&c->h_tab, sizeof(int) * H.size(), hipHostMallocDefault) == hipSuccess)
            c->h_tab_n = H.size();
        else
            hipGetLastError();
    }
    if (c->h_tab) {
        std::memcpy(c->h_tab, H.data(), sizeof(int) * H.size());
        tab_src = c->h_tab;
    }
    HIPCHK(c, hipMemcpyAsync(B.d_tab, tab_src, sizeof(int) * H.size(), hipMemcpyHostToDevice, c->s0));
    return SCC_OK;
}

// the mirror's bytes (with its segment table: 4 B per gene and segment of SCC_MIRROR_SEG cells)
static size_t mirror_bytes(int G, int N, int64_t nnz1)
{
    const size_t seg_n = (size_t)G * ((size_t)(N + SCC_MIRROR_SEG - 1) / SCC_MIRROR_SEG + 1);
    return sizeof(long long) * ((size_t)G + 1) + sizeof(int) * (size_t)G +
           (sizeof(unsigned int) + sizeof(unsigned long long)) * (size_t)nnz1 + sizeof(unsigned int) * seg_n;
}

// the value order's bytes: the sorted cells, the cut table's starts and the
// cuts at their bound (two buckets in a row hold more than 64 entries)
static size_t vorder_cut_bound(int G, int64_t nnz1) { return sizeof(unsigned int) * ((size_t)(2 * nnz1 / 65) + (size_t)G + 1); }
static size_t vorder_bytes(int G, int64_t nnz1)
{
    return sizeof(unsigned int) * ((size_t)nnz1 + (size_t)G + 1) + vorder_cut_bound(G, nnz1);
}

// The value order of a mirrored dataset (scc_vorder.hip), built once under
// its own timer when the mirror and the order together fit the mirror's
// memory rule; else the mirror stays alone and the rank stage keeps its
// per-call buckets.  SCC_RANK_VORDER=0 (read at each call) skips the build.
static int ensure_vorder(scc_ctx* c, const DePlan* pl, const DeBuffers& B)
{
    const scc_dataset* ds = pl->ds;
    const int G = pl->G, N = pl->N;
    const int64_t nnz1 = pl->nnz1;
    if (ds->m_vcell || !ds->m_gptr || G < 1 || env_int("SCC_RANK_VORDER", 1) == 0) return SCC_OK;
    // (the mirror is allocated already: the free memory it took counts as free for the rule)
    const size_t m_bytes = mirror_bytes(G, N, nnz1), both = m_bytes + vorder_bytes(G, nnz1);
    size_t mfree = 0, mtot = 0;
    bool room = hipMemGetInfo(&mfree, &mtot) == hipSuccess && both <= (mfree + m_bytes) / 4;
    (void)hipGetLastError();
    const char* mb = getenv("SCC_INGEST_MIRROR_MAX_BYTES");
    if (mb && *mb && (double)both > atof(mb)) room = false;
    if (!room) return SCC_OK;
    if (hipMalloc((void**)&ds->m_vcell, sizeof(unsigned int) * (size_t)nnz1) != hipSuccess ||
        hipMalloc((void**)&ds->m_vbk_ptr, sizeof(unsigned int) * ((size_t)G + 1)) != hipSuccess) {
        (void)hipGetLastError();
        vorder_free(ds);
        return SCC_OK;
    }
    hipError_t e;
    {
        Scope sc(c, "rank_vorder_build", c->s0);
        // (the sort's scratch: the run's keys2 and keys, [nnz1] u64 each, not yet written by this run)
        e = scc_launch_vorder_build(ds->m_gptr, G, ds->m_cell, ds->m_key, ds->m_vcell, ds->m_vbk_ptr, &ds->m_vbk,
                                    &ds->m_vnbk, B.d_cnt, B.d_gstart, B.d_scan, vorder_cut_bound(G, nnz1),
                                    B.d_keys2, nnz1, B.d_keys, sizeof(unsigned long long) * (size_t)nnz1, c->s0);
    }
    if (e == hipErrorOutOfMemory) {  // the sort's scratch or the cut table: no order
        (void)hipGetLastError();
        vorder_free(ds);
        return SCC_OK;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        vorder_free(ds);
        return fail(c, SCC_ERR_HIP, std::string("value order build failed: ") + hipGetErrorString(e));
    }
    if (!ds->m_vbk) vorder_free(ds);
    return SCC_OK;
}

// The dataset's gene-major mirror (FAST runs on a validated sparse dataset,
// whole range and gene shards alike): built here once, under its own timer,
// when it fits in a quarter of the free memory (the tile-start cache's
// rule; SCC_INGEST_MIRROR_MAX_BYTES lowers the limit, a test knob), else
// the transpose stays.  With a mirror the run's route becomes INGEST_MIRROR.
static int ensure_mirror(scc_ctx* c, DePlan* pl, const DeBuffers& B)
{
    const scc_dataset* ds = pl->ds;
    const int G = pl->G, N = pl->N;
    const int64_t nnz1 = pl->nnz1;
    hipStream_t s0 = c->s0;
    if (!ds->m_gptr) {
        const size_t seg_n = (size_t)G * ((size_t)(N + SCC_MIRROR_SEG - 1) / SCC_MIRROR_SEG + 1);
        const size_t m_bytes = mirror_bytes(G, N, nnz1);
        size_t mfree = 0, mtot = 0;
        bool room = hipMemGetInfo(&mfree, &mtot) == hipSuccess && m_bytes <= mfree / 4;
        (void)hipGetLastError();
        const char* mb = getenv("SCC_INGEST_MIRROR_MAX_BYTES");
        if (mb && *mb && (double)m_bytes > atof(mb)) room = false;
        if (room) {
            if (hipMalloc((void**)&ds->m_gptr, sizeof(long long) * ((size_t)G + 1)) != hipSuccess ||
                hipMalloc((void**)&ds->m_order, sizeof(int) * (size_t)G) != hipSuccess ||
                hipMalloc((void**)&ds->m_cell, sizeof(unsigned int) * (size_t)nnz1) != hipSuccess ||
                hipMalloc((void**)&ds->m_key, sizeof(unsigned long long) * (size_t)nnz1) != hipSuccess ||
                hipMalloc((void**)&ds->m_seg, sizeof(unsigned int) * seg_n) != hipSuccess) {
                (void)hipGetLastError();
                mirror_free(ds);
            } else {
                std::vector<long long> gp((size_t)G + 1);
                hipError_t e;
                {
                    // (nc >= ceil(N / 32), the build's chunks: the run's count rows and scratch hold the build's)
                    Scope sc(c, "ingest_mirror_build", s0);
                    e = scc_launch_mirror_build(ds->d_indptr, ds->d_rows, ds->d_vals, nnz1, N, G, B.d_cnt, B.d_cscr,
                                                B.d_scan, ds->m_gptr, ds->m_cell, ds->m_key, ds->m_seg, s0);
                    // the genes by descending length: the regroup's dispatch order
                    if (e == hipSuccess)
                        e = hipMemcpyAsync(gp.data(), ds->m_gptr, sizeof(long long) * gp.size(),
                                           hipMemcpyDeviceToHost, s0);
                    if (e == hipSuccess) e = hipStreamSynchronize(s0);
                    if (e == hipSuccess) {
                        std::vector<int> ord(G);
                        for (int g = 0; g < G; ++g) ord[g] = g;
                        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
                            return gp[x + 1] - gp[x] > gp[y + 1] - gp[y];
                        });
                        e = hipMemcpy(ds->m_order, ord.data(), sizeof(int) * (size_t)G, hipMemcpyHostToDevice);
                    }
                }
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    mirror_free(ds);
                    return fail(c, SCC_ERR_HIP, std::string("mirror build failed: ") + hipGetErrorString(e));
                }
            }
        }
    }
    if (!ds->m_gptr) return SCC_OK;
    pl->route = INGEST_MIRROR;
    if (int rc = ensure_vorder(c, pl, B)) return rc;
    if (ds->d_tbnd) {  // the transpose's tile starts: not needed any more
        hipFree(ds->d_tbnd);
        ds->d_tbnd = nullptr;
    }
    return SCC_OK;
}

// the genes' starts in d_keys (the mirror's own when every cell is kept)
static long long* gene_starts(const DePlan& pl, const DeBuffers& B)
{
    const bool whole = pl.glo == 0 && pl.ghi == pl.G;
    return pl.route == INGEST_MIRROR && whole && pl.nkept == pl.N ? pl.ds->m_gptr : B.d_gstart;
}

static int ingest_mirror(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const scc_dataset* ds = pl.ds;
    const int G = pl.G, N = pl.N, K = pl.K, glo = pl.glo, ghi = pl.ghi, nc = pl.nc;
    hipStream_t s0 = c->s0;
    Scope sc(c, "ingest", s0);
    HIPCHK(c, scc_launch_de_clear(B.d_err, B.d_counts, pl.norank ? nullptr : B.d_acc, (long long)pl.acc_n, B.d_first,
                                  (int)G, glo, ghi, s0));
    HIPCHK(c, hipMemcpyAsync(B.d_nodg, ds->d_nodg, sizeof(int) * N, hipMemcpyDeviceToDevice, s0));
    const bool whole = glo == 0 && ghi == G;
    long long* gstart_run = gene_starts(pl, B);
    if (gstart_run == B.d_gstart) {
        uint32_t* d_total = B.d_cnt + (size_t)nc * G;  // (the totals row of the transpose; zero outside a shard)
        if (!whole) HIPCHK(c, hipMemsetAsync(d_total, 0, sizeof(uint32_t) * G, s0));
        HIPCHK(c, scc_launch_mirror_total(ds->m_gptr, ds->m_cell, B.d_code8, glo, ghi, d_total, s0));
        HIPCHK(c, scc_launch_scan(d_total, G, B.d_gstart, B.d_scan, B.d_gstart + G, s0));
    }
    // (the value-order route reads neither the regrouped keys nor the offset rows, and k_mir_stats reads the mirror)
    if (!pl.stats_mirror)
        HIPCHK(c, scc_launch_mirror_regroup(ds->m_gptr, ds->m_cell, ds->m_key, B.d_code8,
                                            whole ? ds->m_order : nullptr, glo, ghi, K, G, B.d_clcc, gstart_run,
                                            B.d_cnt, B.d_keys, s0));
    return SCC_OK;
}

static int ingest_transpose(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const scc_dataset* ds = pl.ds;
    const int G = pl.G, N = pl.N, glo = pl.glo, ghi = pl.ghi, nc = pl.nc, ntile = pl.ntile;
    const bool fast = pl.fast, lean = pl.route == INGEST_LEAN;
    const bool hist_rng = lean && (glo > 0 || ghi < G);  // a gene shard: its tiles only
    const bool hist_ro = lean && !hist_rng;              // all genes, no explicit zeros: the row indices only
    hipStream_t s0 = c->s0;
    Scope sc(c, "ingest", s0);
    // error words, counters, rank accumulators and first-occurrence keys in one launch
    HIPCHK(c, scc_launch_de_clear(B.d_err, B.d_counts, pl.norank ? nullptr : B.d_acc, (long long)pl.acc_n, B.d_first,
                                  (int)G, glo, ghi, s0));
    if (lean && !ds->d_tbnd) {  // once per dataset: every cell's gene-tile starts
        // (8 B per (cell, tile): ~0.6 GB at config E, held until the dataset
        // is destroyed, outside the workspace; taken only while it leaves
        // three quarters of the free memory to the runs' workspaces, else
        // the counting pass keeps its per-run binary searches: INTEGRATION.md)
        const size_t tb_bytes = sizeof(long long) * (size_t)N * (ntile + 1);
        size_t mfree = 0, mtot = 0;
        const bool room = hipMemGetInfo(&mfree, &mtot) == hipSuccess && tb_bytes <= mfree / 4;
        (void)hipGetLastError();
        if (!room || hipMalloc((void**)&ds->d_tbnd, tb_bytes) != hipSuccess) {
            (void)hipGetLastError();
            ds->d_tbnd = nullptr;
        } else {
            HIPCHK(c, scc_launch_tile_bounds(ds->d_indptr, ds->d_rows, N, pl.gt, ntile, ds->d_tbnd, s0));
        }
    }
    // (the tile-start cache: the scatter reads it instead of the run's bnd)
    const long long* tbnd = lean ? ds->d_tbnd : nullptr;
    if ((hist_ro || (hist_rng && ds->no_zeros)) && tbnd && env_int("SCC_COUNT_RO", 1) != 0)
        HIPCHK(c, scc_launch_ingest_count_ro(ds->d_indptr, ds->d_rows, G, B.d_perm, B.d_ccp0, B.d_cccode, nc,
                                             hist_rng ? glo : 0, hist_rng ? ghi : G, tbnd, B.d_cnt, s0));
    else
        HIPCHK(c, scc_launch_ingest_hist(ds->d_indptr, ds->d_rows, ds->d_vals, ds->d_dense, G, B.d_perm, B.d_ccp0,
                                         B.d_cccode, nc, ntile, B.d_cnt, B.d_bnd, B.d_nodg, B.d_wexp, fast ? 0 : 1, glo,
                                         ghi, hist_rng ? 1 : (hist_ro ? 2 : 0), tbnd, B.d_err, s0));
    if (lean) HIPCHK(c, hipMemcpyAsync(B.d_nodg, ds->d_nodg, sizeof(int) * N, hipMemcpyDeviceToDevice, s0));
    // range mode: count rows and their column scan over the shard's gene
    // tiles only; the totals row is zero elsewhere (gstart: empty genes)
    int cg0 = 0, cg1 = G;
    if (hist_rng) {
        scc_ingest_count_range(G, glo, ghi, &cg0, &cg1);
        HIPCHK(c, hipMemsetAsync(B.d_cnt + (size_t)nc * G, 0, sizeof(uint32_t) * G, s0));
    }
    HIPCHK(c, scc_launch_ingest_colscan(B.d_cnt, nc, pl.nc_kept, G, cg0, cg1, B.d_cscr, s0));
    const uint32_t* d_total = B.d_cnt + (size_t)nc * G;
    HIPCHK(c, scc_launch_scan(d_total, G, B.d_gstart, B.d_scan, B.d_gstart + G, s0));
    HIPCHK(c, scc_launch_ingest_scatter(ds->d_indptr, ds->d_rows, ds->d_vals, ds->d_dense, G, B.d_perm, B.d_ccp0,
                                        B.d_sccc0, pl.ns, B.d_cnt, B.d_gstart, B.d_bnd, tbnd, ntile, glo, ghi, B.d_keys,
                                        s0));
    if (!fast) HIPCHK(c, scc_launch_reduce_dd(B.d_wexp, pl.nwaves, B.d_gexp, s0));
    return SCC_OK;
}

static int gene_stats(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    Scope sc(c, "gene_stats", c->s0);
    if (pl.stats_mirror) {
        const scc_dataset* ds = pl.ds;
        HIPCHK(c, scc_launch_mirror_stats(ds->m_gptr, ds->m_cell, ds->m_key, B.d_code8, ds->m_order, pl.G, pl.K,
                                          gene_starts(pl, B), B.d_nclu, B.d_me, B.d_cntpos, B.d_cntneg, c->s0));
        return SCC_OK;
    }
    ScStatsLaunch S{};
    S.gstart = gene_starts(pl, B);
    S.keys = B.d_keys;
    S.G = pl.G, S.K = pl.K, S.glo = pl.glo, S.gn = pl.ghi - pl.glo;
    S.mode = pl.prm->mode, S.test = pl.test;
    S.n_clu = B.d_nclu, S.coff = B.d_cnt, S.cl_cc = B.d_clcc;
    S.mean_x = B.d_mx, S.mean_e = B.d_me, S.cnt_pos = B.d_cntpos, S.cnt_neg = B.d_cntneg;
    S.var_x = B.d_vx;
    S.mean_pos = B.d_mpos, S.m2_pos = B.d_m2pos, S.min_pos = B.d_minpos, S.max_pos = B.d_maxpos;
    S.sum_e = B.d_sume;
    HIPCHK(c, scc_launch_gene_stats(&S, c->s0));
    return SCC_OK;
}

// SLOW: log(meanScalingFactor * mean(expm1(X))) (slow:36) gates the pair
// filter; a scalar read back here.
static int slow_threshold(scc_ctx* c, const DePlan& pl, const DeBuffers& B, double* log_thr)
{
    double gx[2];
    HIPCHK(c, hipMemcpyAsync(gx, B.d_gexp, sizeof(double) * 2, hipMemcpyDeviceToHost, c->s0));
    HIPCHK(c, hipStreamSynchronize(c->s0));
    // R: LDOUBLE two-pass mean over G*N entries (zeros included) -> double
    const double tot = (double)pl.G * (double)pl.N;
    double q = gx[0] / tot;
    double r = std::fma(-q, tot, gx[0]) + gx[1];
    const double mean = q + r / tot;
    *log_thr = std::log(pl.prm->mean_scaling_factor * mean);
    return SCC_OK;
}

// the launch record of pair_filter and pair_test
static ScTestLaunch test_launch(const scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    ScTestLaunch T{};
    T.K = pl.K, T.G = pl.G, T.P = pl.P, T.glo = pl.glo, T.ghi = pl.ghi;
    T.mode = pl.prm->mode, T.test = pl.test, T.all_pairs = pl.all_pairs ? 1 : 0;
    T.min_pct = pl.prm->min_per_cent, T.lfc_thr = pl.prm->log_fc_thrs, T.log_thr = pl.log_thr;
    T.n_clu = B.d_nclu;
    T.mean_x = B.d_mx, T.mean_e = B.d_me, T.cnt_pos = B.d_cntpos, T.cnt_neg = B.d_cntneg;
    T.accS = B.accS, T.accE = B.accE, T.accX = B.accX, T.accF = B.accF;
    T.var_x = B.d_vx;
    T.mean_pos = B.d_mpos, T.m2_pos = B.d_m2pos, T.min_pos = B.d_minpos, T.max_pos = B.d_maxpos;
    T.err = B.d_err;
    T.wtab = c->d_wtab, T.woff = c->d_woff;
    T.out_p = B.d_p, T.out_lfc = B.d_lfc, T.out_pct1 = B.d_pct1, T.out_pct2 = B.d_pct2;
    T.out_u2 = B.d_u2, T.out_t = B.d_t, T.out_flags = B.d_flags;
    return T;
}

// ---------------------------------------------------------------- rank stage
static ScRankLaunch rank_launch(const DePlan& pl, const DeBuffers& B)
{
    const int K = pl.K, P = pl.P;
    ScRankLaunch L{};
    L.gstart = gene_starts(pl, B);
    L.keys = B.d_keys;
    L.G = pl.G, L.K = K, L.P = P, L.all_pairs = pl.all_pairs ? 1 : 0;
    L.coff = B.d_cnt, L.cl_cc = B.d_clcc, L.flags = B.d_flags;
    L.cap_s = pl.cap_s, L.cap_m = pl.cap_m, L.bucket_target = pl.bucket_target, L.wave_target = pl.wave_target;
    L.rw_slots = P <= 128 ? 2 : P <= 256 ? 4 : P <= 512 ? 8 : 16;
    L.dbg = env_int("SCC_RW_DEBUG", 0);
    L.rw_mfma = env_int("SCC_RANK_MFMA", 1);
    L.rw_mfma16 = env_int("SCC_RANK_MFMA16", -1);
    L.cross_wave = env_int("SCC_CROSS_WAVE", 0);
    L.bucket_cap = pl.bucket_cap, L.sbuckets = B.d_sbk, L.hbg = B.d_hbg;
    L.gene_bk = B.d_genebk, L.gkmin = B.d_gkmin;
    L.ntp_max = pl.ntp_max, L.item_cap = pl.item_cap, L.items = B.d_items;
    L.counts = B.d_counts, L.split_genes = B.d_splitg;
    L.keys2 = B.d_keys2, L.codes2 = B.d_codes2;
    L.gix = B.d_gix, L.gwin = B.d_gwin, L.gcode = B.d_gcode, L.gsc = B.d_gsc;
    L.nnz = pl.nnz1;
    L.accS = B.accS, L.accE = B.accE, L.accX = B.accX, L.accF = B.accF;
    L.gene_tp = B.gene_tp, L.gene_nt = B.gene_nt;
    if (scc_rank_tables_global(pl.ntp_max, K)) {  // items' tested-pair tables in HBM, one slice per workgroup
        L.tp_global = 1;
        L.tp_scr_stride = scc_rank_tables_stride(pl.ntp_max, K);
        L.tp_scr = B.tp_scr;
    }
    if (pl.resplit) {
        L.fat_cap = L.fat2_cap = pl.fat_cap;
        L.fatbk = B.fatbk, L.rsseg = B.rsseg, L.fatg = B.fatg, L.fat2 = B.fat2;
    }
    return L;
}

static int rank_log(scc_ctx* c, hipStream_t s0, const int* d_counts);

// The value-order route: a FAST Wilcoxon run over the whole gene range on one
// device, on a dataset that holds the order (SCC_RANK_VORDER=0, read at each
// call: the per-call buckets).  The route is a call's, never a gene's; de_run
// asks once, after ensure_mirror, and keeps the answer in the plan.
static bool rank_vorder_route(const scc_ctx* c, const DePlan& pl)
{
    const scc_dataset* ds = pl.ds;
    return ds->m_vcell && ds->m_vbk && ds->m_gptr && pl.route == INGEST_MIRROR && pl.fast && !pl.norank &&
           !pl.markers && !pl.shard_stage && pl.glo == 0 && pl.ghi == pl.G && c->peers.empty() &&
           ds->m_vnbk <= pl.bucket_cap && !pl.stamps && env_int("SCC_RANK_VORDER", 1) != 0;
}

// On that route at K <= 16 one launch of k_rank_mfma16<1, true> takes every
// bucket (the same conditions as rank_waves_launches_t's): it can add the
// cross-bucket term inside each run itself and leave one histogram row per run
// (SCC_RANK_RUNS=0: a row per bucket and k_rank_cross over buckets).
static bool rank_runs_route(const DePlan& pl)
{
    const int mfma = env_int("SCC_RANK_MFMA", 1), mfma16 = env_int("SCC_RANK_MFMA16", -1);
    return pl.vorder && pl.K <= 16 && (mfma == 2 || mfma16 != 0) && env_int("SCC_RW_DEBUG", 0) == 0 &&
           env_int("SCC_RANK_RUNS", 1) != 0;
}

// On that route the rank kernels read the mirror, the order and the call's
// codes, so the regroup's only reader left is k_gene_stats: k_mir_stats gives
// its three arrays from the mirror instead, up to the K its lane sums fit
// (SCC_STATS_MIRROR=0, read at each call: regroup + k_gene_stats).
static bool stats_mirror_route(const DePlan& pl)
{
    return pl.vorder && pl.test == SCC_TEST_WILCOX && pl.ds->m_order && pl.K <= scc_mirror_stats_max_k() &&
           env_int("SCC_STATS_MIRROR", 1) != 0;
}

// classify, the dataset's buckets into the wave list, the pair counts, the
// cross terms: no split, no re-split, no LDS items, no fork to s1
static int rank_stage_vorder(scc_ctx* c, const DePlan& pl, const DeBuffers& B, ScRankLaunch& L)
{
    int rc;
    hipStream_t s0 = c->s0;
    const scc_dataset* ds = pl.ds;
    L.vcell = ds->m_vcell, L.vbk_ptr = ds->m_vbk_ptr, L.vbk = ds->m_vbk, L.vgptr = ds->m_gptr;
    L.code8 = B.d_code8;
    L.fatbk = nullptr;  // (no re-split parents: k_rank_cross_seg has nothing to add)
    const int ncu = c->n_cu > 0 ? c->n_cu : 256;
    L.rank_runs = pl.rank_runs ? 1 : 0;
    L.rk_grid = 8 * ncu;
    // (the accumulators' bound: a test lowers it to drive the flush inside a run)
    L.run_bound = (unsigned int)std::max(1, env_int("SCC_RANK_RUN_BOUND", 0x7fffffff));
    HIPCHK(c, scc_launch_rank_classify(&L, s0));
    HIPCHK(c, scc_launch_rank_vorder_list(&L, std::max(1, std::min((pl.G + 7) / 8, 1 << 20)), s0));  // (8 genes a workgroup)
    if (L.dbg == 7) scc_rank_mfma_stamps(s0, 0);
    // K <= 16: one launch (k_rank_mfma16<1, true>), no side stream; else the slot
    // classes' and the matrix-core class's launches on s0 and the two side streams
    const int rw_side = (pl.K > 16 && env_int("SCC_RW_STREAMS", 1) != 0 && L.dbg != 7) ? 2 : 0;
    HIPCHK(c, scc_launch_rank_waves(&L, L.rk_grid, s0, c->sw, rw_side, c->ev_wfork, c->ev_wj));
    if (L.dbg == 7) scc_rank_mfma_stamps(s0, 1);
    HIPCHK(c, scc_launch_rank_cross(&L, 4 * ncu, s0));
    if (env_int("SCC_RANK_LOG", 0) && (rc = rank_log(c, s0, B.d_counts))) return rc;
    g_rank_last_route = 2;
    g_rank_last_runs = L.rank_runs;
    return SCC_OK;
}

// the rank stage's work counters on the host (diagnostics; synchronises s0)
static hipError_t read_counts(const int* d_counts, hipStream_t s0, int* h)
{
    int t[SCC_NCOUNTS * SCC_CNT_STRIDE];
    hipError_t e = hipMemcpyAsync(t, d_counts, sizeof(t), hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    for (int i = 0; i < SCC_NCOUNTS; ++i) h[i] = t[i * SCC_CNT_STRIDE];
    return e;
}

// SCC_STAMPS: the items' phase clocks, [3][item_cap][8] u64 (the re-split's 8 in the last slot)
static int rank_stamps_begin(scc_ctx* c, hipStream_t s0, unsigned long long* st_buf, int item_cap, ScRankLaunch& L)
{
    HIPCHK(c, hipMemsetAsync(st_buf, 0, sizeof(unsigned long long) * 3 * item_cap * 8, s0));
    L.stamps = st_buf;
    L.stamp_base[0] = 0;
    L.stamp_base[1] = item_cap;
    L.stamp_base[2] = 2 * item_cap;
    return SCC_OK;
}

// SCC_RW_DEBUG >= 9: per-gene split clocks (diagnostic; 10: without the unstaged stores)
static int rank_split_clocks(scc_ctx* c, hipStream_t s0, const int* d_counts)
{
    int hc[SCC_NCOUNTS];
    HIPCHK(c, read_counts(d_counts, s0, hc));
    scc_rank_split_diag(s0, hc[RK_CNT_SPLIT_GENES] + hc[RK_CNT_BIG_GENES]);
    return SCC_OK;
}

// SCC_STAMPS: the re-split on s0 alone, with its phase clocks
static int rank_resplit_clocks(scc_ctx* c, hipStream_t s0, const ScRankLaunch& L, unsigned long long* st_buf,
                               int item_cap, int ncu)
{
    // re-split phase clocks (summed over parents): 8 u64 after the item stamps
    ScRankLaunch R = L;
    R.stamps = st_buf + (size_t)3 * item_cap * 8 - 8;
    HIPCHK(c, hipMemsetAsync(R.stamps, 0, 64, s0));
    HIPCHK(c, scc_launch_rank_resplit(&R, 4 * ncu, s0));
    unsigned long long h[8];
    HIPCHK(c, hipMemcpyAsync(h, R.stamps, 64, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    fprintf(stderr, "[scc stamps] resplit parents %llu, mean cycles: load %.0f bins %.0f scatter %.0f list %.0f cross %.0f\n",
            h[7], h[0] / (double)std::max(1ull, h[7]), h[1] / (double)std::max(1ull, h[7]),
            h[2] / (double)std::max(1ull, h[7]), h[3] / (double)std::max(1ull, h[7]),
            h[4] / (double)std::max(1ull, h[7]));
    HIPCHK(c, hipMemsetAsync(R.stamps, 0, 64, s0));
    return SCC_OK;
}

// SCC_RANK_LOG: the rank stage's work lists
static int rank_log(scc_ctx* c, hipStream_t s0, const int* d_counts)
{
    int h[SCC_NCOUNTS];
    HIPCHK(c, read_counts(d_counts, s0, h));
    fprintf(stderr, "[scc rank] items %d/%d/%d split genes %d wave buckets %d bucket ids %d parents %d "
            "segments %d second-level %d\n", h[RK_CNT_ITEMS0], h[RK_CNT_ITEMS0 + 1], h[RK_CNT_ITEMS0 + 2],
            h[RK_CNT_SPLIT_GENES] + h[RK_CNT_BIG_GENES], h[RK_CNT_WAVE_SLOTS], h[RK_CNT_BUCKET_IDS], h[RK_CNT_FAT],
            h[RK_CNT_SEGMENTS], h[RK_CNT_FAT2]);
    return SCC_OK;
}

// SCC_STAMPS: the class report
static int rank_stamps_report(scc_ctx* c, hipStream_t s0, const unsigned long long* st_buf, int item_cap,
                              const int* d_counts)
{
    std::vector<unsigned long long> h((size_t)3 * item_cap * 8);
    int cnts[SCC_NCOUNTS];
    HIPCHK(c, hipMemcpyAsync(h.data(), st_buf, h.size() * 8, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, read_counts(d_counts, s0, cnts));
    const char* ph[] = {"setup", "sort", "fixup+codes", "partition", "pairs", "ties"};
    fprintf(stderr, "[scc stamps] split genes %d\n", cnts[RK_CNT_SPLIT_GENES]);
    for (int cls = 0; cls < 3; ++cls) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        int nb = 0;
        for (int b = 0; b < cnts[RK_CNT_ITEMS0 + cls]; ++b) {
            const unsigned long long* t = &h[((size_t)cls * item_cap + b) * 8];
            if (!t[0] || !t[6]) continue;
            for (int q = 0; q < 6; ++q) acc[q] += (double)(t[q + 1] - t[q]);
            ++nb;
        }
        fprintf(stderr, "[scc stamps] rank class %d: %d items (%d full), mean cycles:", cls, cnts[RK_CNT_ITEMS0 + cls], nb);
        for (int q = 0; q < 6; ++q) fprintf(stderr, " %s %.0f", ph[q], nb ? acc[q] / nb : 0.0);
        fprintf(stderr, "\n");
    }
    return SCC_OK;
}

// classify, split, re-split, then the wave buckets on s0 (and side streams)
// beside the LDS items on s1, then the cross terms on s0
static int rank_stage(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    int rc;
    hipStream_t s0 = c->s0, s1 = c->s1;
    Scope sc(c, "gene_rank", s0);
    ScRankLaunch L = rank_launch(pl, B);
    if (pl.vorder) return rank_stage_vorder(c, pl, B, L);
    if (pl.stamps && (rc = rank_stamps_begin(c, s0, B.st_buf, pl.item_cap, L))) return rc;
    HIPCHK(c, scc_launch_rank_classify(&L, s0));
    const int ncu = c->n_cu > 0 ? c->n_cu : 256;
    HIPCHK(c, scc_launch_rank_split(&L, 2 * ncu, s0));
    if (L.dbg >= 9 && (rc = rank_split_clocks(c, s0, B.d_counts))) return rc;
    if (pl.stamps) {
        if ((rc = rank_resplit_clocks(c, s0, L, B.st_buf, pl.item_cap, ncu))) return rc;
    } else {
        // (not on small jobs: at config B the fork and join cost more than
        // the overlap of two ~10-us launches)
        // (SCC_RW_STREAMS=2 forces them at any size: the streams test)
        const int rw_mode = env_int("SCC_RW_STREAMS", 1);
        const int rs_side = (rw_mode >= 2 || (rw_mode != 0 && pl.ds->nnz > (64ll << 20))) ? 2 : 0;
        HIPCHK(c, scc_launch_rank_resplit(&L, 4 * ncu, s0, c->sw, rs_side, c->ev_wfork, c->ev_wj));
    }
    // buckets of <= 64 elements (one wave each) beside the fat buckets (LDS
    // items; SCC_ITEMS_SERIAL=1 runs them after the waves on one stream)
    const bool items_serial = env_int("SCC_ITEMS_SERIAL", 0) != 0;
    hipStream_t si = items_serial ? s0 : s1;
    if (!items_serial) {
        HIPCHK(c, hipEventRecord(c->ev_fork, s0));
        HIPCHK(c, hipStreamWaitEvent(s1, c->ev_fork, 0));
    }
    if (L.dbg == 7) scc_rank_mfma_stamps(s0, 0);
    // the slot classes on s0 and two side streams (SCC_RW_STREAMS=0: all on s0)
    // (forked only when a second class launch exists: config B has one)
    // (sides: one side stream and the items' stream s1 -- a second side
    // stream shared the first one's hardware queue, GPU_MAX_HW_QUEUES = 4)
    const int rw_side = (env_int("SCC_RW_STREAMS", 1) != 0 && L.dbg != 7) ? 2 : 0;
    const hipStream_t wsides[2] = {c->sw[0], si};
    HIPCHK(c, scc_launch_rank_waves(&L, 8 * ncu, s0, si != s0 ? wsides : c->sw, rw_side, c->ev_wfork, c->ev_wj));
    if (L.dbg == 7) scc_rank_mfma_stamps(s0, 1);
    HIPCHK(c, scc_launch_rank_items(&L, 1, 2 * ncu, si));
    HIPCHK(c, scc_launch_rank_items(&L, 0, 4 * ncu, si));
    HIPCHK(c, scc_launch_rank_items(&L, 2, ncu, si));
    if (!items_serial) {
        HIPCHK(c, hipEventRecord(c->ev_join, s1));
        HIPCHK(c, hipStreamWaitEvent(s0, c->ev_join, 0));
    }
    HIPCHK(c, scc_launch_rank_cross(&L, 4 * ncu, s0));
    HIPCHK(c, scc_launch_rank_cross_seg(&L, 4 * ncu, s0));
    if (env_int("SCC_RANK_LOG", 0) && (rc = rank_log(c, s0, B.d_counts))) return rc;
    if (pl.stamps && (rc = rank_stamps_report(c, s0, B.st_buf, pl.item_cap, B.d_counts))) return rc;
    return SCC_OK;
}

// ---------------------------------------------------------------- exchange
// the (pair, gene) fields a shard carries, in scc_de_shard_bytes order
struct Field {
    void* p;
    size_t es;
};
static std::array<Field, 7> shard_fields(const DePlan& pl, const DeBuffers& B)
{
    return {{{B.d_p, 8}, {B.d_lfc, 8}, {pl.fast ? (void*)B.d_pct1 : nullptr, 8}, {pl.fast ? (void*)B.d_pct2 : nullptr, 8},
             {B.d_u2, 8}, {B.d_t, 8}, {B.d_flags, 1}}};
}

// DE_SHARD: the dense layout, zero outside the shard
static int shard_pack(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const int G = pl.G, P = pl.P, glo = pl.glo, ghi = pl.ghi;
    hipStream_t s0 = c->s0;
    char* dst = (char*)pl.shard;
    HIPCHK(c, hipMemsetAsync(dst, 0, scc_de_shard_bytes(pl.K, G), s0));
    for (const Field& f : shard_fields(pl, B)) {
        if (f.p && ghi > glo)
            HIPCHK(c, hipMemcpy2DAsync(dst + glo * f.es, G * f.es, (const char*)f.p + glo * f.es, G * f.es,
                                       (size_t)(ghi - glo) * f.es, P, hipMemcpyDeviceToDevice, s0));
        dst += pl.PG * f.es;
    }
    return SCC_OK;
}

// DE_SHARD_REC: compact records of the tested cells of this shard, (pair, gene) order
static int shard_records(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const int G = pl.G, P = pl.P, glo = pl.glo, ghi = pl.ghi;
    const bool fast = pl.fast;
    const RecIO* rio = pl.rio;
    hipStream_t s0 = c->s0;
    const long long cells = (long long)P * (ghi - glo);
    const int nb = std::max(1, scc_rec_blocks(cells));
    const int all = fast ? 0 : 1;
    HIPCHK(c, hipMemsetAsync(B.d_rc, 0, sizeof(uint32_t) * nb, s0));
    HIPCHK(c, scc_launch_rec_count(B.d_flags, G, P, glo, ghi, all, B.d_rc, s0));
    HIPCHK(c, scc_launch_scan(B.d_rc, nb, B.d_roff, B.d_rscr, B.d_roff + nb, s0));
    long long nrec = 0;
    HIPCHK(c, hipMemcpyAsync(&nrec, B.d_roff + nb, sizeof(long long), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    *rio->n_out = nrec;
    if (nrec > rio->cap)
        return fail(c, SCC_ERR_INVALID, "scc_de_run_shard_records: record buffer too small (cap < n_records)");
    HIPCHK(c, scc_launch_rec_pack(B.d_flags, G, P, glo, ghi, all, B.d_roff, B.d_p, B.d_lfc, fast ? B.d_pct1 : nullptr,
                                  fast ? B.d_pct2 : nullptr, B.d_u2, B.d_t, (scc_de_record*)rio->out, s0));
    return SCC_OK;
}

// DE_FINISH: every gene's (pair, gene) fields from the summed shards
static int finish_load_dense(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const char* src = (const char*)pl.shard;
    for (const Field& f : shard_fields(pl, B)) {
        if (f.p) HIPCHK(c, hipMemcpyAsync(f.p, src, pl.PG * f.es, hipMemcpyDeviceToDevice, c->s0));
        src += pl.PG * f.es;
    }
    return SCC_OK;
}

// DE_FINISH_REC: the fields cleared, then every block's records scattered into them
static int finish_scatter_records(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const int G = pl.G, P = pl.P;
    const size_t PG = pl.PG;
    const bool fast = pl.fast;
    const RecIO* rio = pl.rio;
    hipStream_t s0 = c->s0;
    // pair-split selection (first_out): only this rank's pair rows are
    // read, so only they are cleared and scattered.  FAST reads a cell's
    // statistics only where its flag is set (k_pair_select), so of the
    // range only the flags are cleared; SLOW clears every field of the
    // range.  Outside the range the flags keep older contents: they only
    // size the other pairs' row offsets (at most one row per cell, so the
    // range's rows stay inside the row buffers) and no row there is read.
    const bool pb = pl.pairs_only;
    const int plo = pb ? rio->pair_lo : 0, phi = pb ? rio->pair_hi : P;
    for (const Field& f : shard_fields(pl, B)) {
        if (!f.p) continue;
        if (!pb)
            HIPCHK(c, hipMemsetAsync(f.p, 0, PG * f.es, s0));
        else if (phi > plo && (f.p == (void*)B.d_flags || !fast))
            HIPCHK(c, hipMemsetAsync((char*)f.p + (size_t)plo * G * f.es, 0, (size_t)(phi - plo) * G * f.es, s0));
    }
    HIPCHK(c, hipMemsetAsync(B.d_err, 0, sizeof(int) * 4, s0));
    const scc_de_record* rec = (const scc_de_record*)rio->in;
    for (int b = 0; b < rio->nblocks; ++b)
        HIPCHK(c, scc_launch_rec_scatter(rec + (size_t)b * rio->stride, rio->counts[b], G, P, B.d_p, B.d_lfc,
                                         fast ? B.d_pct1 : nullptr, fast ? B.d_pct2 : nullptr, B.d_u2, B.d_t, B.d_flags,
                                         B.d_err, plo, phi, s0));
    return SCC_OK;
}

// ---------------------------------------------------------------- selection
// Per-pair BH, filters and top-N, then the union.  A pairs-only finish ends
// here: its first-occurrence keys go to the caller and its errors are reported.
static int pair_select(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const int G = pl.G, P = pl.P;
    const bool fast = pl.fast;
    const scc_de_params* prm = pl.prm;
    const RecIO* rio = pl.rio;
    hipStream_t s0 = c->s0;
    Scope sc(c, "pair_select", s0);
    // (a compute stage's first-occurrence keys were reset by scc_launch_de_clear at the ingest)
    if (pl.finish_stage) HIPCHK(c, hipMemsetAsync(B.d_first, 0xFF, sizeof(unsigned long long) * G, s0));
    if (fast) HIPCHK(c, scc_launch_count_tested(B.d_flags, G, P, B.d_tested, B.d_rowoff, s0));
    ScSelectLaunch S{};
    S.K = pl.K, S.G = G, S.P = P, S.mode = prm->mode;
    S.top_n = fast ? prm->top_n : 30;
    S.cap = env_int("SCC_SELECT_CAP", kSelectCap);
    S.q_thr = prm->q_val_thrs;
    S.lfc_cut = fast ? 0.0 : std::log(prm->fc_thrs);
    S.p = B.d_p, S.lfc = B.d_lfc, S.pct1 = B.d_pct1, S.pct2 = B.d_pct2;
    S.u2 = B.d_u2, S.t = B.d_t, S.flags = B.d_flags;
    S.row_off = B.d_rowoff, S.rec_scratch = B.d_rec, S.key_scratch = B.d_key;
    S.row_gene = B.d_row_gene, S.row_p = B.d_row_p, S.row_q = B.d_row_q, S.row_lfc = B.d_row_lfc;
    S.row_pct1 = B.d_row_pct1, S.row_pct2 = B.d_row_pct2;
    S.row_u2 = B.d_row_u2, S.row_t = B.d_row_t, S.row_flags = B.d_row_flags;
    S.slow_q = B.d_slow_q, S.slow_de = B.d_slow_de;
    S.first_occ = B.d_first, S.err = B.d_err;
    S.plo = pl.pairs_only ? rio->pair_lo : 0;
    S.phi = pl.pairs_only ? rio->pair_hi : P;
    HIPCHK(c, scc_launch_pair_select(&S, s0));
    if (pl.pairs_only) {
        HIPCHK(c, hipMemcpyAsync(rio->first_out, B.d_first, sizeof(unsigned long long) * G, hipMemcpyDeviceToDevice,
                                 s0));
        int e = 0;
        HIPCHK(c, hipMemcpyAsync(&e, B.d_err, sizeof(int), hipMemcpyDeviceToHost, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        return de_error(c, e, AT_PAIRS);
    }
    HIPCHK(c, scc_launch_union(B.d_first, G, B.d_key, env_int("SCC_UNION_CAP", kUnionCap), B.d_union, B.d_nu, s0));
    return SCC_OK;
}

// one pinned staging buffer (c->h_stage), one synchronisation: [0] |U|, [1]
// error bits, [2..3] FAST row count (i64), [4, 4 + P) tested rows per pair,
// then the union (up to G entries)
static int stage_pack(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    const int G = pl.G, P = pl.P;
    const bool fast = pl.fast;
    const size_t stage_n = 4 + (size_t)P + (size_t)G;
    if (c->h_stage_n < stage_n) {
        if (c->h_stage) hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        c->h_stage_n = 0;
        if (hipHostMalloc((void**)&c->h_stage, sizeof(int) * stage_n, hipHostMallocMapped) != hipSuccess) {
            hipGetLastError();
            c->h_stage = nullptr;
            return fail(c, SCC_ERR_OOM, "pinned staging allocation failed");
        }
        c->h_stage_n = stage_n;
    }
    int* hs = c->h_stage;
    int* hs_dev = nullptr;  // the same pinned buffer as the device sees it
    HIPCHK(c, hipHostGetDevicePointer((void**)&hs_dev, hs, 0));
    HIPCHK(c, scc_launch_stage_pack(B.d_nu, B.d_err, fast ? B.d_rowoff + P : nullptr, fast ? B.d_tested : nullptr, P,
                                    B.d_union, G, hs_dev, c->s0));
    HIPCHK(c, hipStreamSynchronize(c->s0));
    return check_pending_eig(c);  // an earlier device-output scc_distance
}

// after an error-free run whose ingest read every entry: the dataset is
// validated and its nodg cached (for later gene-shard runs)
static int note_validated(scc_ctx* c, const DePlan& pl, const DeBuffers& B, int err_bits)
{
    const scc_dataset* ds = pl.ds;
    if (pl.route != INGEST_FULL || ds->validated || ds->dense) return SCC_OK;
    ds->no_zeros = !(err_bits & 0x1000);  // the full read saw no explicit zero
    if (!ds->d_nodg && hipMalloc((void**)&ds->d_nodg, sizeof(int) * pl.N) != hipSuccess) {
        hipGetLastError();
        ds->d_nodg = nullptr;
        return SCC_OK;  // no cache: later shards keep reading everything
    }
    HIPCHK(c, hipMemcpyAsync(ds->d_nodg, B.d_nodg, sizeof(int) * pl.N, hipMemcpyDeviceToDevice, c->s0));
    HIPCHK(c, hipStreamSynchronize(c->s0));
    ds->validated = true;
    return SCC_OK;
}

// the result: host copies out of the staging buffer, device views into the workspace
static scc_de_result* build_result(scc_ctx* c, const DePlan& pl, const DeBuffers& B, int n_union)
{
    const int P = pl.P;
    const int* hs = c->h_stage;
    scc_de_result* r = new scc_de_result();
    r->ctx = c;
    r->generation = c->generation;
    r->mode = pl.prm->mode, r->K = pl.K, r->P = P, r->G = pl.G, r->N = pl.N;
    r->d_union = B.d_union;
    r->log_thr = pl.log_thr;
    r->union_genes.assign(hs + 4 + P, hs + 4 + P + n_union);
    if (pl.fast) {
        long long nrows = 0;
        std::memcpy(&nrows, &hs[2], sizeof(long long));
        r->pair_tested.assign(hs + 4, hs + 4 + P);
        r->n_rows = nrows;
    }
    r->d_nodg = B.d_nodg;
    r->d_row_gene = B.d_row_gene, r->d_row_p = B.d_row_p, r->d_row_q = B.d_row_q, r->d_row_lfc = B.d_row_lfc;
    r->d_row_pct1 = B.d_row_pct1, r->d_row_pct2 = B.d_row_pct2;
    r->d_row_u2 = B.d_row_u2, r->d_row_t = B.d_row_t, r->d_row_flags = B.d_row_flags;
    r->d_p = B.d_p, r->d_q = B.d_slow_q, r->d_lfc = B.d_lfc, r->d_u2 = B.d_u2, r->d_de = B.d_slow_de;
    return r;
}

// ---------------------------------------------------------------- one engine run
static int de_run(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                  int stage, int64_t glo64, int64_t ghi64, void* shard, scc_de_result** out,
                  const RecIO* rio = nullptr)
{
    int rc;
    if ((rc = de_check_args(c, ds, code, K, prm, stage, shard, out, rio))) return rc;
    scc_enter(c);
    DePlan pl{};
    if ((rc = de_plan(c, ds, code, K, prm, stage, glo64, ghi64, shard, rio, &pl))) return rc;
    DeBuffers B{};
    if ((rc = de_alloc(c, pl, &B))) return rc;
    if ((rc = ensure_wtab(c, exact_test_max_size(pl.nclu)))) return rc;
    hipStream_t s0 = c->s0;
    c->generation++;
    const int64_t sig[6] = {pl.G, pl.N, K, prm->mode, ds->nnz, (int64_t)(intptr_t)ds};
    if (pl.finish_stage) {
        if (!std::equal(sig, sig + 6, c->shard_sig))
            return fail(c, SCC_ERR_INVALID, "scc_de_finish: this context ran no scc_de_run_shard for these inputs");
        pl.log_thr = c->shard_log_thr;
        if ((rc = stage == DE_FINISH ? finish_load_dense(c, pl, B) : finish_scatter_records(c, pl, B))) return rc;
    } else {
        if ((rc = upload_tables(c, B))) return rc;
        if (pl.try_mirror && (rc = ensure_mirror(c, &pl, B))) return rc;
        pl.vorder = rank_vorder_route(c, pl);
        pl.rank_runs = rank_runs_route(pl);
        pl.stats_mirror = stats_mirror_route(pl);
        g_ingest_last_path = pl.route;
        g_rank_last_route = 1;  // (rank_stage: 2 on the value-order route)
        g_rank_last_runs = 0;
        g_mirror_last_uses = (g_mirror_last_uses & ~1) | (pl.stats_mirror ? 1 : 0);
        if ((rc = pl.route == INGEST_MIRROR ? ingest_mirror(c, pl, B) : ingest_transpose(c, pl, B))) return rc;
        if ((rc = gene_stats(c, pl, B))) return rc;
        if (!pl.fast && (rc = slow_threshold(c, pl, B, &pl.log_thr))) return rc;
        const ScTestLaunch T = test_launch(c, pl, B);
        {
            Scope sc(c, "pair_filter", s0);
            HIPCHK(c, scc_launch_pair_filter(&T, s0));
        }
        if (!pl.norank && (rc = rank_stage(c, pl, B))) return rc;
        {
            Scope sc(c, "pair_test", s0);
            HIPCHK(c, scc_launch_pair_test(&T, s0));
        }
    }
    if (pl.shard_stage) {
        if ((rc = stage == DE_SHARD ? shard_pack(c, pl, B) : shard_records(c, pl, B))) return rc;
        std::copy(sig, sig + 6, c->shard_sig);
        c->shard_log_thr = pl.log_thr;
        HIPCHK(c, hipStreamSynchronize(s0));
        int e = 0;
        HIPCHK(c, hipMemcpy(&e, B.d_err, sizeof(int), hipMemcpyDeviceToHost));
        if ((rc = de_error(c, e, AT_SHARD))) return rc;
        return note_validated(c, pl, B, e);
    }
    if ((rc = pair_select(c, pl, B)) || pl.pairs_only) return rc;
    if ((rc = stage_pack(c, pl, B))) return rc;
    const int n_union = c->h_stage[0], err_bits = c->h_stage[1];
    if ((rc = de_error(c, err_bits, AT_FULL))) return rc;
    if ((rc = note_validated(c, pl, B, err_bits))) return rc;
    if (n_union < 0 || n_union > pl.G) return fail(c, SCC_ERR_HIP, "union size out of range");
    *out = build_result(c, pl, B, n_union);
    // selection-stage conditions (k_pair_select), reported after the result is built
    return de_error(c, err_bits, AT_RESULT);
}

// ---------------------------------------------------------------- one-vs-rest markers
// scc_de_markers: for every cluster a, ComputePairWiseDE(cells.1 = a, cells.2 =
// the other kept cells) and the caller's selection (Fast:229-351, 376-392), in
// one engine pass.  The run is a DE_FULL FAST plan whose "pairs" are the K
// clusters: every [P][G] field is [K][G], so the ingest, the statistics, the
// selection (BH, top-N, first-occurrence union, tested-rows > 1) and the
// result are the all-pairs route's own phases; the filter, the rank kernel
// (one sort per gene serves all K tests, scc_rank_rest.hip) and the test are
// the one-vs-rest ones.  It runs on the context's first device.
static int markers_plan(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                        const scc_de_params* dp, DePlan* p)
{
    int rc = de_plan(c, ds, code, K, dp, DE_FULL, 0, ds->G, nullptr, nullptr, p);
    if (rc) return rc;
    p->markers = true;
    p->P = K;
    p->PG = (size_t)p->GK;
    p->acc_n = (size_t)p->GK + (size_t)p->G;  // R2 per (cluster, gene), T per gene
    return SCC_OK;
}

// the largest group of an exact test: cluster a and its rest both below 50 cells
static int markers_exact_size(const std::vector<int>& nclu)
{
    int nsel = 0, m = 0;
    for (int v : nclu) nsel += v;
    for (int v : nclu)
        if (v < 50 && nsel - v < 50) m = std::max(m, std::max(v, nsel - v));
    return m;
}

static ScRestTestLaunch rest_launch(const scc_ctx* c, const DePlan& pl, const DeBuffers& B, int only_pos)
{
    ScRestTestLaunch T{};
    T.K = pl.K, T.G = pl.G, T.only_pos = only_pos, T.all = pl.all_pairs ? 1 : 0;
    T.min_pct = pl.prm->min_per_cent, T.lfc_thr = pl.prm->log_fc_thrs;
    T.n_clu = B.d_nclu, T.sum_e = B.d_sume, T.cnt_pos = B.d_cntpos, T.cnt_neg = B.d_cntneg;
    T.accR = B.d_acc, T.accT = B.d_acc + pl.PG;
    T.wtab = c->d_wtab, T.woff = c->d_woff;
    T.out_p = B.d_p, T.out_lfc = B.d_lfc, T.out_pct1 = B.d_pct1, T.out_pct2 = B.d_pct2;
    T.out_u2 = B.d_u2, T.out_t = B.d_t, T.out_flags = B.d_flags;
    return T;
}

static int rank_rest_stage(scc_ctx* c, const DePlan& pl, const DeBuffers& B)
{
    Scope sc(c, "rank_rest", c->s0);
    ScRestRankLaunch L{};
    L.gstart = gene_starts(pl, B);
    L.keys = B.d_keys;
    L.G = pl.G, L.K = pl.K, L.all = pl.all_pairs ? 1 : 0;
    L.coff = B.d_cnt, L.cl_cc = B.d_clcc, L.flags = B.d_flags;
    L.keys2 = B.d_keys2, L.codes2 = B.d_codes2;
    L.accR = B.d_acc, L.accT = B.d_acc + pl.PG;
    HIPCHK(c, scc_launch_rank_rest(&L, c->s0));
    return SCC_OK;
}

extern "C" int scc_de_markers(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                              const scc_markers_params* mp, scc_de_result** out)
{
    if (!c || !ds || !code || !mp || !out) return fail(c, SCC_ERR_INVALID, "scc_de_markers: null argument");
    *out = nullptr;
    if (ds->ctx != c) return fail(c, SCC_ERR_INVALID, "dataset belongs to another context");
    if (mp->test == SCC_TEST_T || mp->test == SCC_TEST_BIMOD)
        return fail(c, SCC_ERR_UNSUPPORTED, "scc_de_markers: SCC_TEST_WILCOX only");
    if (mp->test != SCC_TEST_WILCOX) return fail(c, SCC_ERR_INVALID, "scc_de_markers: bad test");
    if (K < 2) return fail(c, SCC_ERR_INVALID, "need at least two clusters");
    if (K > kMaxK) return fail(c, SCC_ERR_UNSUPPORTED, "scc_de_markers: K > 128 clusters");
    for (int32_t v : mp->reserved)
        if (v != 0) return fail(c, SCC_ERR_INVALID, "scc_de_markers: reserved fields must be zero");
    scc_de_params dp{};
    dp.mode = SCC_DE_FAST, dp.top_n = mp->top_n, dp.q_val_thrs = mp->q_val_thrs, dp.log_fc_thrs = mp->log_fc_thrs;
    dp.min_per_cent = mp->min_per_cent, dp.fc_thrs = 1.5, dp.mean_scaling_factor = 5.0;
    dp.test_all = mp->test_all ? 1 : 0, dp.test = SCC_TEST_WILCOX;
    int rc;
    scc_enter(c);
    DePlan pl{};
    if ((rc = markers_plan(c, ds, code, K, &dp, &pl))) return rc;
    DeBuffers B{};
    if ((rc = de_alloc(c, pl, &B))) return rc;
    if ((rc = ensure_wtab(c, markers_exact_size(pl.nclu)))) return rc;
    hipStream_t s0 = c->s0;
    c->generation++;
    if ((rc = upload_tables(c, B))) return rc;
    if (pl.try_mirror && (rc = ensure_mirror(c, &pl, B))) return rc;
    g_ingest_last_path = pl.route;
    g_rank_last_route = 1;
    g_rank_last_runs = 0;
    g_mirror_last_uses &= ~1;  // (one-vs-rest: regroup + k_gene_stats)
    if ((rc = pl.route == INGEST_MIRROR ? ingest_mirror(c, pl, B) : ingest_transpose(c, pl, B))) return rc;
    if ((rc = gene_stats(c, pl, B))) return rc;
    const ScRestTestLaunch T = rest_launch(c, pl, B, mp->only_pos ? 1 : 0);
    {
        Scope sc(c, "rest_filter", s0);
        HIPCHK(c, scc_launch_rest_filter(&T, s0));
    }
    if ((rc = rank_rest_stage(c, pl, B))) return rc;
    {
        Scope sc(c, "rest_test", s0);
        HIPCHK(c, scc_launch_rest_test(&T, s0));
    }
    if ((rc = pair_select(c, pl, B))) return rc;
    if ((rc = stage_pack(c, pl, B))) return rc;
    const int n_union = c->h_stage[0], err_bits = c->h_stage[1];
    if ((rc = de_error(c, err_bits, AT_FULL))) return rc;
    if ((rc = note_validated(c, pl, B, err_bits))) return rc;
    if (n_union < 0 || n_union > pl.G) return fail(c, SCC_ERR_HIP, "union size out of range");
    scc_de_result* r = build_result(c, pl, B, n_union);
    r->d_t = B.d_t;
    *out = r;
    return de_error(c, err_bits, AT_RESULT);
}

// ---------------------------------------------------------------- device list
// ONE DE job over the context's devices (scc_opts.n_devices > 1; SURVEY 8e:
// gene row-blocks, then a gather of compact per-(pair, tested gene) records):
// each device runs the per-(pair, gene) stage of its gene block and packs its
// tested cells (scc_de_record, 64 B) -- one host thread per device --, the
// records are copied to devices[0] (xGMI peer copies) and the per-pair BH,
// filters, top-N and union run there: the scc_de_finish_records result, equal
// to the one-device run bit for bit.  Blocks are balanced by the genes'
// stored values (a CSC row histogram, computed once per dataset).
static int gene_blocks(scc_ctx* c, const scc_dataset* ds, int D, std::vector<int64_t>& cut)
{
    const int64_t G = ds->G;
    cut.assign(D + 1, 0);
    cut[D] = G;
    if (!ds->dense && ds->gene_w.empty() && ds->nnz > 0) {
        unsigned int* d_h = nullptr;
        int rc = ws(c, "row_hist", (size_t)G, &d_h);
        if (rc) return rc;
        HIPCHK(c, scc_launch_row_hist(ds->d_rows, ds->nnz, (int)G, d_h, c->s0));
        std::vector<unsigned int> h(G);
        HIPCHK(c, hipMemcpyAsync(h.data(), d_h, sizeof(unsigned int) * G, hipMemcpyDeviceToHost, c->s0));
        HIPCHK(c, hipStreamSynchronize(c->s0));
        ds->gene_w.assign(h.begin(), h.end());
    }
    std::vector<double> cw(G + 1, 0.0);
    for (int64_t g = 0; g < G; ++g) cw[g + 1] = cw[g] + (ds->gene_w.empty() ? 1.0 : 1.0 + (double)ds->gene_w[g]);
    for (int d = 1; d < D; ++d) {
        const double share = cw[G] * d / D;
        int64_t g = std::lower_bound(cw.begin(), cw.end(), share) - cw.begin();
        // non-empty blocks while genes last
        g = std::max<int64_t>(g, std::min<int64_t>(G, cut[d - 1] + 1));
        cut[d] = std::min<int64_t>(g, G);
    }
    return SCC_OK;
}

static int de_run_multi(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                        scc_de_result** out)
{
    *out = nullptr;
    if (ds->reps.size() != c->peers.size()) return fail(c, SCC_ERR_INVALID, "dataset has no replica on every device");
    const int D = 1 + (int)c->peers.size();
    std::vector<scc_ctx*> eng{c};
    std::vector<const scc_dataset*> dsr{ds};
    for (size_t i = 0; i < c->peers.size(); ++i) {
        eng.push_back(c->peers[i]);
        dsr.push_back(ds->reps[i]);
    }
    scc_enter(c);
    std::vector<int64_t> cut;
    int rc = gene_blocks(c, ds, D, cut);
    if (rc) return rc;
    const int64_t P = (int64_t)K * (K - 1) / 2;
    std::vector<int> rcs(D, SCC_OK);
    std::vector<int64_t> nrec(D, 0);
    std::vector<void*> rbuf(D, nullptr);
    {
        std::vector<std::thread> th;
        for (int d = 0; d < D; ++d)
            th.emplace_back([&, d] {
                scc_ctx* x = eng[d];
                hipSetDevice(x->device);
                const int64_t cap = std::max<int64_t>(1, P * (cut[d + 1] - cut[d]));
                if ((rcs[d] = ws_get(x, "mrec", (size_t)cap * sizeof(scc_de_record), &rbuf[d]))) return;
                RecIO io;
                io.out = rbuf[d];
                io.cap = cap;
                io.n_out = &nrec[d];
                rcs[d] = de_run(x, dsr[d], code, K, prm, DE_SHARD_REC, cut[d], cut[d + 1], nullptr, nullptr, &io);
            });
        for (auto& t : th) t.join();
    }
    scc_enter(c);
    for (int d = 0; d < D; ++d)
        if (rcs[d]) return d ? fail(c, rcs[d], eng[d]->err) : rcs[d];
    const int64_t stride = std::max<int64_t>(1, *std::max_element(nrec.begin(), nrec.end()));
    void* all = nullptr;
    if ((rc = ws_get(c, "mrec_all", (size_t)D * stride * sizeof(scc_de_record), &all))) return rc;
    for (int d = 0; d < D; ++d) {
        if (!nrec[d]) continue;
        char* dst = (char*)all + (size_t)d * stride * sizeof(scc_de_record);
        const size_t bytes = (size_t)nrec[d] * sizeof(scc_de_record);
        if (eng[d]->device == c->device)
            HIPCHK(c, hipMemcpyAsync(dst, rbuf[d], bytes, hipMemcpyDeviceToDevice, c->s0));
        else
            HIPCHK(c, hipMemcpyPeerAsync(dst, c->device, rbuf[d], eng[d]->device, bytes, c->s0));
    }
    RecIO io;
    io.in = all;
    io.counts = nrec.data();
    io.nblocks = D;
    io.stride = stride;
    return de_run(c, ds, code, K, prm, DE_FINISH_REC, 0, ds->G, nullptr, out, &io);
}

// one engine run of <= 128 clusters: on the context's device, or sharded over its device list
static int de_run_one(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                      scc_de_result** out)
{
    if (!c->peers.empty() && K <= kMaxK) return de_run_multi(c, ds, code, K, prm, out);
    return de_run(c, ds, code, K, prm, DE_FULL, 0, ds->G, nullptr, out);
}

// ---------------------------------------------------------------- any K
// More clusters than one engine run ranks (7-bit codes, 128): the K clusters
// are cut into ng = ceil(K / gmax) groups of balanced size (gmax = 64, or
// SCC_GROUP_SIZE), and the engine runs once per group pair (u < v) on the cells
// of those <= 128 clusters (the others get code -1).  Every per-pair quantity
// of both DE paths depends on the pair's two clusters alone (FAST: pct,
// log-mean logFC, filters, test, BH over the pair's own rows, top_n,
// Fast:229-392; SLOW: test, mean difference, gate with the GLOBAL threshold of
// every entry -- the same in every run, since the ingest sums expm1 over all
// cells whatever their code --, BH with n = G, first 30, slow:36,90-227), so a
// global pair (i, j) is taken from exactly one run: the run of its two groups,
// or for a pair inside one group the first run holding that group.  A run's
// clusters keep the global order, so Cluster1 / Cluster2 orientation and the
// within-run pair order are the global ones.  Rows (FAST) and per-pair vectors
// are moved into the global (i, j) order on the device (k_seg_copy); the
// union is unique() over the pairs' top lists in (i, j) order, i.e. genes by
// their smallest (pair, rank) key: each run's keys are renumbered to global
// pairs and MIN-folded (k_first_remap), then ordered once (k_union).
static int de_run_grouped(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K, const scc_de_params* prm,
                          int gmax, scc_de_result** out)
{
    *out = nullptr;
    const bool fast = prm->mode == SCC_DE_FAST;
    if (prm->mode != SCC_DE_FAST && prm->mode != SCC_DE_SLOW) return fail(c, SCC_ERR_INVALID, "bad mode");
    const int64_t G = ds->G, N = ds->N;
    const int64_t P = (int64_t)K * (K - 1) / 2;
    if (P >= ((int64_t)1 << 31)) return fail(c, SCC_ERR_UNSUPPORTED, "more than 2^31 cluster pairs");
    std::vector<int> nclu;
    if (int bad = cluster_sizes(c, code, N, K, fast, nclu)) return bad;
    scc_enter(c);
    hipStream_t s0 = c->s0;
    const int ng = (K + gmax - 1) / gmax;
    std::vector<int> gid(K);
    std::vector<std::vector<int>> grp(ng);
    for (int u = 0; u < ng; ++u)
        for (int a = (int)((int64_t)u * K / ng); a < (int)((int64_t)(u + 1) * K / ng); ++a) {
            grp[u].push_back(a);
            gid[a] = u;
        }
    const bool vectors = !fast || prm->test_all;  // the dense [P][G] per-pair vectors
    const size_t PG = (size_t)P * (size_t)G;
    int rc;
    double *g_p = nullptr, *g_lfc = nullptr, *g_q = nullptr;
    long long* g_u2 = nullptr;
    uint8_t* g_de = nullptr;
    unsigned long long* g_first = nullptr;
#define WSG(name, n, ptr)                                       \
    do {                                                        \
        if ((rc = ws(c, name, (size_t)(n), &(ptr)))) return rc; \
    } while (0)
    WSG("grp_first", G, g_first);
    if (vectors) {
        WSG("grp_p", PG, g_p);
        WSG("grp_lfc", PG, g_lfc);
        WSG("grp_u2", PG, g_u2);
        if (!fast) {
            WSG("grp_q", PG, g_q);
            WSG("grp_de", PG, g_de);
        }
    }
    HIPCHK(c, hipMemsetAsync(g_first, 0xFF, sizeof(unsigned long long) * G, s0));
    // FAST rows: staged in run order (grow-preserving buffers), then gathered
    // into the global pair order at the end
    struct RowField {
        const char* stage;
        const char* fin;
        int es;
    };
    static const RowField rf[9] = {{"grp_s_gene", "grp_row_gene", 4}, {"grp_s_p", "grp_row_p", 8},
                                   {"grp_s_q", "grp_row_q", 8},       {"grp_s_lfc", "grp_row_lfc", 8},
                                   {"grp_s_pct1", "grp_row_pct1", 8}, {"grp_s_pct2", "grp_row_pct2", 8},
                                   {"grp_s_u2", "grp_row_u2", 8},     {"grp_s_t", "grp_row_t", 8},
                                   {"grp_s_flags", "grp_row_flags", 1}};
    int64_t staged = 0;
    std::vector<int64_t> st_off(fast ? P : 0, 0), st_cnt(fast ? P : 0, 0);
    std::vector<char> covered(ng, 0);
    std::vector<int32_t> sub(N);
    std::vector<long long> lp2gp, seg;
    bool rstop = false;
    std::string rstop_msg;
    double log_thr = 0.0;
    for (int u = 0; u < ng; ++u)
        for (int v = u + 1; v < ng; ++v) {
            std::vector<int> cl(grp[u]);
            cl.insert(cl.end(), grp[v].begin(), grp[v].end());
            const int Kl = (int)cl.size();
            std::vector<int> lut(K, -1);
            for (int l = 0; l < Kl; ++l) lut[cl[l]] = l;
            for (int64_t i = 0; i < N; ++i) sub[i] = code[i] >= 0 ? lut[code[i]] : -1;
            scc_de_result* r = nullptr;
            rc = de_run_one(c, ds, sub.data(), Kl, prm, &r);
            if (rc) {
                if (rc != SCC_ERR_RSTOP || !r) {
                    scc_de_result_destroy(r);
                    return rc;
                }
                rstop = true;
                rstop_msg = c->err;
            }
            log_thr = r->log_thr;
            const int Pl = Kl * (Kl - 1) / 2;
            lp2gp.assign(Pl, 0);
            std::vector<char> take(Pl, 0);
            {
                int lp = 0;
                for (int li = 0; li < Kl; ++li)
                    for (int lj = li + 1; lj < Kl; ++lj, ++lp) {
                        const int64_t gi = cl[li], gj = cl[lj];
                        lp2gp[lp] = gi * K - gi * (gi + 1) / 2 + (gj - gi - 1);
                        take[lp] = gid[gi] != gid[gj] || !covered[gid[gi]];
                    }
            }
            covered[u] = covered[v] = 1;
            long long *d_lp2gp = nullptr, *d_seg = nullptr;
            unsigned long long* d_first = nullptr;
            WSG("grp_lp2gp", Pl, d_lp2gp);
            WSG("first", G, d_first);  // the run's per-gene first-occurrence keys
            HIPCHK(c, hipMemcpyAsync(d_lp2gp, lp2gp.data(), sizeof(long long) * Pl, hipMemcpyHostToDevice, s0));
            HIPCHK(c, scc_launch_first_remap(d_first, (int)G, d_lp2gp, g_first, s0));
            if (vectors) {  // per-pair [G] vectors: one segment per taken pair
                seg.clear();
                for (int lp = 0; lp < Pl; ++lp)
                    if (take[lp]) {
                        seg.push_back((long long)lp * G);
                        seg.push_back(lp2gp[lp] * G);
                        seg.push_back(G);
                    }
                const long long ns = (long long)seg.size() / 3;
                WSG("grp_seg", seg.size(), d_seg);
                HIPCHK(c, hipMemcpyAsync(d_seg, seg.data(), sizeof(long long) * seg.size(), hipMemcpyHostToDevice, s0));
                HIPCHK(c, scc_launch_seg_copy(r->d_p, g_p, 8, d_seg, ns, s0));
                HIPCHK(c, scc_launch_seg_copy(r->d_lfc, g_lfc, 8, d_seg, ns, s0));
                HIPCHK(c, scc_launch_seg_copy(r->d_u2, g_u2, 8, d_seg, ns, s0));
                if (!fast) {
                    HIPCHK(c, scc_launch_seg_copy(r->d_q, g_q, 8, d_seg, ns, s0));
                    HIPCHK(c, scc_launch_seg_copy(r->d_de, g_de, 1, d_seg, ns, s0));
                }
                HIPCHK(c, hipStreamSynchronize(s0));  // d_seg is rewritten by the next segment table
            }
            if (fast) {  // the taken pairs' rows, appended to the staging buffers
                seg.clear();
                int64_t lo = 0, add = 0;
                for (int lp = 0; lp < Pl; ++lp) {
                    const int64_t n = r->pair_tested[lp];
                    if (take[lp] && n > 0) {
                        seg.push_back(lo);
                        seg.push_back(staged + add);
                        seg.push_back(n);
                    }
                    if (take[lp]) {
                        st_off[lp2gp[lp]] = staged + add;
                        st_cnt[lp2gp[lp]] = n;
                        add += n;
                    }
                    lo += n;
                }
                const long long ns = (long long)seg.size() / 3;
                if (ns > 0) {
                    WSG("grp_seg", seg.size(), d_seg);
                    HIPCHK(c, hipMemcpyAsync(d_seg, seg.data(), sizeof(long long) * seg.size(), hipMemcpyHostToDevice,
                                             s0));
                    const void* src[9] = {r->d_row_gene, r->d_row_p,  r->d_row_q,  r->d_row_lfc, r->d_row_pct1,
                                          r->d_row_pct2, r->d_row_u2, r->d_row_t, r->d_row_flags};
                    for (int f = 0; f < 9; ++f) {
                        void* dst = nullptr;
                        if ((rc = ws_keep(c, rf[f].stage, (size_t)(staged + add) * rf[f].es, (size_t)staged * rf[f].es,
                                          &dst)))
                            return rc;
                        HIPCHK(c, scc_launch_seg_copy(src[f], dst, rf[f].es, d_seg, ns, s0));
                    }
                    HIPCHK(c, hipStreamSynchronize(s0));
                }
                staged += add;
            }
            scc_de_result_destroy(r);
        }
    scc_de_result* r = new scc_de_result();
    r->ctx = c;
    r->mode = prm->mode;
    r->K = K;
    r->P = (int)P;
    r->G = G;
    r->N = N;
    r->log_thr = log_thr;
    std::unique_ptr<scc_de_result> hold(r);
    if (fast) {  // staged rows -> the global (i, j) order
        r->pair_tested.resize(P);
        seg.clear();
        int64_t row = 0;
        for (int64_t p = 0; p < P; ++p) {
            r->pair_tested[p] = (int32_t)st_cnt[p];
            if (st_cnt[p] > 0) {
                seg.push_back(st_off[p]);
                seg.push_back(row);
                seg.push_back(st_cnt[p]);
            }
            row += st_cnt[p];
        }
        r->n_rows = row;
        const long long ns = (long long)seg.size() / 3;
        long long* d_seg = nullptr;
        WSG("grp_seg", std::max<size_t>(seg.size(), 3), d_seg);
        if (ns > 0)
            HIPCHK(c, hipMemcpyAsync(d_seg, seg.data(), sizeof(long long) * seg.size(), hipMemcpyHostToDevice, s0));
        void* fin[9];
        for (int f = 0; f < 9; ++f) {
            if ((rc = ws_get(c, rf[f].fin, (size_t)std::max<int64_t>(row, 1) * rf[f].es, &fin[f]))) return rc;
            void* stg = nullptr;
            if ((rc = ws_keep(c, rf[f].stage, (size_t)std::max<int64_t>(staged, 1) * rf[f].es, (size_t)staged * rf[f].es,
                              &stg)))
                return rc;
            HIPCHK(c, scc_launch_seg_copy(stg, fin[f], rf[f].es, d_seg, ns, s0));
        }
        r->d_row_gene = (const int*)fin[0];
        r->d_row_p = (const double*)fin[1];
        r->d_row_q = (const double*)fin[2];
        r->d_row_lfc = (const double*)fin[3];
        r->d_row_pct1 = (const double*)fin[4];
        r->d_row_pct2 = (const double*)fin[5];
        r->d_row_u2 = (const long long*)fin[6];
        r->d_row_t = (const long long*)fin[7];
        r->d_row_flags = (const uint8_t*)fin[8];
    }
    r->d_p = g_p;
    r->d_lfc = g_lfc;
    r->d_u2 = g_u2;
    r->d_q = g_q;
    r->d_de = g_de;
    r->vectors = vectors;
    {  // the union: genes ordered by their smallest global (pair, rank) key
        void* d_key = nullptr;
        int *d_union = nullptr, *d_nu = nullptr, *d_nodg = nullptr;
        if ((rc = ws_get(c, "key_scratch", (size_t)G * scc_select_key_bytes(), &d_key))) return rc;
        WSG("union", G, d_union);
        WSG("nu", 4, d_nu);
        WSG("nodg", N, d_nodg);  // every run wrote the same nodg (clustering-independent)
        HIPCHK(c, scc_launch_union(g_first, (int)G, d_key, env_int("SCC_UNION_CAP", kUnionCap), d_union, d_nu, s0));
        int nu = 0;
        HIPCHK(c, hipMemcpyAsync(&nu, d_nu, sizeof(int), hipMemcpyDeviceToHost, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        if (nu < 0 || nu > G) return fail(c, SCC_ERR_HIP, "union size out of range");
        r->union_genes.resize(nu);
        if (nu) HIPCHK(c, hipMemcpy(r->union_genes.data(), d_union, sizeof(int) * nu, hipMemcpyDeviceToHost));
        r->d_nodg = d_nodg;
    }
    r->generation = c->generation;
    *out = hold.release();
    if (rstop) return fail(c, SCC_ERR_RSTOP, rstop_msg);
    return SCC_OK;
#undef WSG
}

extern "C" int scc_de_run(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                          const scc_de_params* prm, scc_de_result** out)
{
    if (!c || !ds || !code || !prm || !out) return fail(c, SCC_ERR_INVALID, "scc_de_run: null argument");
    *out = nullptr;
    if (ds->ctx != c) return fail(c, SCC_ERR_INVALID, "dataset belongs to another context");
    // SCC_GROUP_SIZE (test knob): group-pair runs of groups <= this size as
    // soon as K exceeds two groups (default 64: K > 128)
    const int gmax = std::min(std::max(env_int("SCC_GROUP_SIZE", kGroupMax), 1), kGroupMax);
    if (K > 2 * gmax) return de_run_grouped(c, ds, code, K, prm, gmax, out);
    return de_run_one(c, ds, code, K, prm, out);
}

extern "C" int64_t scc_de_shard_bytes(int32_t K, int64_t n_genes)
{
    const int64_t PG = (int64_t)K * (K - 1) / 2 * n_genes;
    return (PG * 49 + 7) / 8 * 8;  // p, lfc, pct1, pct2 (f64), u2, ties (i64), flags (u8); 8-byte multiple
}

extern "C" int scc_de_run_shard(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                                const scc_de_params* prm, int64_t gene_lo, int64_t gene_hi, void* shard)
{
    return de_run(c, ds, code, K, prm, DE_SHARD, gene_lo, gene_hi, shard, nullptr);
}

extern "C" int scc_de_finish(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                             const scc_de_params* prm, const void* shards_sum, scc_de_result** out)
{
    return de_run(c, ds, code, K, prm, DE_FINISH, 0, ds ? ds->G : 0, const_cast<void*>(shards_sum), out);
}

extern "C" int scc_de_run_shard_records(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                                        const scc_de_params* prm, int64_t gene_lo, int64_t gene_hi, void* records,
                                        int64_t cap, int64_t* n_records)
{
    if (!records || !n_records || cap < 0) return fail(c, SCC_ERR_INVALID, "scc_de_run_shard_records: null argument");
    RecIO io;
    io.out = records;
    io.cap = cap;
    io.n_out = n_records;
    *n_records = 0;
    return de_run(c, ds, code, K, prm, DE_SHARD_REC, gene_lo, gene_hi, nullptr, nullptr, &io);
}

extern "C" int scc_de_finish_records(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                                     const scc_de_params* prm, const void* records, const int64_t* counts,
                                     int32_t n_blocks, int64_t stride, scc_de_result** out)
{
    if (!counts || n_blocks < 1 || stride < 0 || (!records && stride > 0))
        return fail(c, SCC_ERR_INVALID, "scc_de_finish_records: bad record blocks");
    for (int b = 0; b < n_blocks; ++b)
        if (counts[b] < 0 || counts[b] > stride) return fail(c, SCC_ERR_INVALID, "scc_de_finish_records: count > stride");
    RecIO io;
    io.in = records;
    io.counts = counts;
    io.nblocks = n_blocks;
    io.stride = stride;
    return de_run(c, ds, code, K, prm, DE_FINISH_REC, 0, ds ? ds->G : 0, nullptr, out, &io);
}

extern "C" int scc_de_finish_records_pairs(scc_ctx* c, const scc_dataset* ds, const int32_t* code, int32_t K,
                                           const scc_de_params* prm, const void* records, const int64_t* counts,
                                           int32_t n_blocks, int64_t stride, int32_t pair_lo, int32_t pair_hi,
                                           void* first_occ)
{
    if (!counts || n_blocks < 1 || stride < 0 || (!records && stride > 0) || !first_occ)
        return fail(c, SCC_ERR_INVALID, "scc_de_finish_records_pairs: bad arguments");
    const int P = K * (K - 1) / 2;
    if (pair_lo < 0 || pair_hi > P || pair_lo > pair_hi)
        return fail(c, SCC_ERR_INVALID, "scc_de_finish_records_pairs: pair range out of bounds");
    if (!prm || prm->mode != SCC_DE_FAST)
        return fail(c, SCC_ERR_UNSUPPORTED, "scc_de_finish_records_pairs: FAST mode only");
    for (int b = 0; b < n_blocks; ++b)
        if (counts[b] < 0 || counts[b] > stride)
            return fail(c, SCC_ERR_INVALID, "scc_de_finish_records_pairs: count > stride");
    RecIO io;
    io.in = records;
    io.counts = counts;
    io.nblocks = n_blocks;
    io.stride = stride;
    io.pair_lo = pair_lo;
    io.pair_hi = pair_hi;
    io.first_out = first_occ;
    return de_run(c, ds, code, K, prm, DE_FINISH_REC, 0, ds ? ds->G : 0, nullptr, nullptr, &io);
}

extern "C" int scc_de_union_first_occ(scc_ctx* c, const void* first_occ, int64_t G64, int32_t* genes,
                                      int32_t* n_union)
{
    if (!c || !first_occ || !genes || !n_union || G64 < 1 || G64 > INT32_MAX)
        return fail(c, SCC_ERR_INVALID, "scc_de_union_first_occ: bad arguments");
    const int G = (int)G64;
    scc_enter(c);
    hipStream_t s0 = c->s0;
    int rc;
    void* d_key = nullptr;
    int *d_union = nullptr, *d_nu = nullptr;
    if ((rc = ws_get(c, "key_scratch", (size_t)G * scc_select_key_bytes(), &d_key))) return rc;
    if ((rc = ws(c, "union", G, &d_union))) return rc;
    if ((rc = ws(c, "nu", 4, &d_nu))) return rc;
    HIPCHK(c, scc_launch_union((const unsigned long long*)first_occ, G, d_key, env_int("SCC_UNION_CAP", kUnionCap),
                               d_union, d_nu, s0));
    int nu = 0;
    HIPCHK(c, hipMemcpyAsync(&nu, d_nu, sizeof(int), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (nu < 0 || nu > G) return fail(c, SCC_ERR_HIP, "scc_de_union_first_occ: bad union size");
    if (nu) HIPCHK(c, hipMemcpy(genes, d_union, sizeof(int) * nu, hipMemcpyDeviceToHost));
    *n_union = nu;
    return SCC_OK;
}

static int check_live(const scc_de_result* r)
{
    if (!r) return SCC_ERR_INVALID;
    if (r->generation != r->ctx->generation)
        return fail(r->ctx, SCC_ERR_INVALID, "result is stale: copy it out before the next scc_de_run");
    hipSetDevice(r->ctx->device);
    return SCC_OK;
}

extern "C" int scc_de_result_counts(const scc_de_result* r, int32_t* n_pairs, int64_t* n_rows, int32_t* n_union)
{
    if (!r) return SCC_ERR_INVALID;
    if (n_pairs) *n_pairs = r->P;
    if (n_rows) *n_rows = r->n_rows;
    if (n_union) *n_union = (int32_t)r->union_genes.size();
    return SCC_OK;
}

extern "C" int scc_de_result_union(const scc_de_result* r, int32_t* genes)
{
    if (!r || !genes) return SCC_ERR_INVALID;
    std::copy(r->union_genes.begin(), r->union_genes.end(), genes);
    return SCC_OK;
}

template <class T>
static int d2h(scc_ctx* c, T* dst, const T* src, size_t n)
{
    if (!dst || n == 0) return SCC_OK;
    HIPCHK(c, hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost));
    return SCC_OK;
}

extern "C" int scc_de_result_rows(const scc_de_result* r, int32_t* pair_rows, int32_t* gene, double* p, double* q,
                                  double* lfc, double* pct1, double* pct2, int64_t* u2, int64_t* ties,
                                  uint8_t* flags)
{
    int rc = check_live(r);
    if (rc) return rc;
    if (r->mode != SCC_DE_FAST) return fail(r->ctx, SCC_ERR_INVALID, "rows exist for SCC_DE_FAST only");
    scc_ctx* c = r->ctx;
    const size_t n = (size_t)r->n_rows;
    if (pair_rows) std::copy(r->pair_tested.begin(), r->pair_tested.end(), pair_rows);
    if ((rc = d2h(c, gene, r->d_row_gene, n))) return rc;
    if ((rc = d2h(c, p, r->d_row_p, n))) return rc;
    if ((rc = d2h(c, q, r->d_row_q, n))) return rc;
    if ((rc = d2h(c, lfc, r->d_row_lfc, n))) return rc;
    if ((rc = d2h(c, pct1, r->d_row_pct1, n))) return rc;
    if ((rc = d2h(c, pct2, r->d_row_pct2, n))) return rc;
    if ((rc = d2h(c, (long long*)u2, r->d_row_u2, n))) return rc;
    if ((rc = d2h(c, (long long*)ties, r->d_row_t, n))) return rc;
    if ((rc = d2h(c, flags, r->d_row_flags, n))) return rc;
    return SCC_OK;
}

extern "C" int scc_de_result_pair_vectors(const scc_de_result* r, double* p, double* q, double* lfc, int64_t* u2,
                                          uint8_t* de)
{
    int rc = check_live(r);
    if (rc) return rc;
    scc_ctx* c = r->ctx;
    const size_t n = (size_t)r->P * (size_t)r->G;
    if (!r->vectors && (p || lfc || u2))
        return fail(c, SCC_ERR_INVALID, "per-pair vectors of a FAST group-pair run exist with test_all = 1 only");
    if ((rc = d2h(c, p, r->d_p, n))) return rc;
    if ((rc = d2h(c, lfc, r->d_lfc, n))) return rc;
    if ((rc = d2h(c, (long long*)u2, r->d_u2, n))) return rc;
    if (r->mode == SCC_DE_SLOW) {
        if ((rc = d2h(c, q, r->d_q, n))) return rc;
        if ((rc = d2h(c, de, r->d_de, n))) return rc;
    } else if (q || de) {
        return fail(c, SCC_ERR_INVALID, "q/de vectors exist for SCC_DE_SLOW only");
    }
    return SCC_OK;
}

extern "C" int scc_de_result_log_threshold(const scc_de_result* r, double* log_thr)
{
    if (!r || !log_thr) return SCC_ERR_INVALID;
    *log_thr = r->log_thr;
    return SCC_OK;
}

extern "C" int scc_de_result_nodg(const scc_de_result* r, int32_t* nodg)
{
    int rc = check_live(r);
    if (rc) return rc;
    return d2h(r->ctx, nodg, r->d_nodg, (size_t)r->N);
}

extern "C" int scc_de_result_ties(const scc_de_result* r, int64_t* ties)
{
    int rc = check_live(r);
    if (rc) return rc;
    if (!r->d_t) return fail(r->ctx, SCC_ERR_INVALID, "scc_de_result_ties: an scc_de_markers result only");
    return d2h(r->ctx, (long long*)ties, r->d_t, (size_t)r->P * (size_t)r->G);
}

extern "C" void scc_de_result_destroy(scc_de_result* r) { delete r; }

