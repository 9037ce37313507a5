// scc_umap.cpp — C ABI of the UMAP stages (include/scc.h: scc_umap_graph,
// scc_umap_layout, scc_umap_scores; kernels: scc_umap.hip).
//
// Each stage has a device form that works on workspace buffers ("um_*") and
// leaves its result there; the three entry points check their host arguments,
// upload, run the device forms and copy the answer back.  scc_umap_scores runs
// scc_knn_scores' device stage (scc_distance.cpp: knn_scores_device) in front,
// so the table and the graph never leave the device.  Runs on devices[0] only.
#include "scc_internal.hpp"

using namespace scc_rt;

extern "C" {
hipError_t scc_launch_umap_graph_weights(const double* dist, int n, int k, double target, double* rowsum, double* total,
                                         double* rho, double* sigma, double* w, hipStream_t st);
hipError_t scc_launch_umap_graph_count(const int* idx, int n, int k, int inter, int* cnt, long long* indptr,
                                       hipStream_t st);
hipError_t scc_launch_umap_graph_fill(const int* idx, const double* w, int n, int k, int inter, double mix,
                                      const long long* indptr, long long nnz, int* cur, int* cols_u, double* vals_u,
                                      int* rowid, int* cols, double* vals, hipStream_t st);
hipError_t scc_launch_umap_init_scores(const double* P, int n, unsigned long long* amax, double* Y, hipStream_t st);
hipError_t scc_launch_umap_layout(const long long* indptr, const int* cols, const double* vals, int n, long long nnz,
                                  int n_epochs, double a, double b, double gamma, double nsr, double lr,
                                  unsigned long long seed, unsigned long long* wmax, double* next, double* nneg,
                                  double* Ya, double* Yb, hipStream_t st);
}

namespace {

struct Graph {  // device CSR in the workspace
    long long* indptr = nullptr;
    int* cols = nullptr;
    double* vals = nullptr;
    double *rho = nullptr, *sigma = nullptr, *w = nullptr;  // per row, and the directed weights [n][k]
    long long nnz = 0;
};

int check_graph_params(scc_ctx* c, const char* who, const scc_umap_params* p)
{
    if (p->local_connectivity != 1.0)
        return fail(c, SCC_ERR_UNSUPPORTED, std::string(who) + ": local_connectivity other than 1");
    if (p->bandwidth != 1.0) return fail(c, SCC_ERR_UNSUPPORTED, std::string(who) + ": bandwidth other than 1");
    if (!(p->set_op_mix_ratio >= 0.0 && p->set_op_mix_ratio <= 1.0))
        return fail(c, SCC_ERR_INVALID, std::string(who) + ": set_op_mix_ratio outside [0, 1]");
    return SCC_OK;
}

int check_layout_params(scc_ctx* c, const char* who, const scc_umap_params* p, double* a, double* b)
{
    if (p->n_epochs < 1) return fail(c, SCC_ERR_INVALID, std::string(who) + ": n_epochs below 1");
    if (p->negative_sample_rate < 0 || p->negative_sample_rate > 64)
        return fail(c, SCC_ERR_INVALID, std::string(who) + ": negative_sample_rate outside 0..64");
    if (!std::isfinite(p->a) || !std::isfinite(p->b) || !std::isfinite(p->gamma) || !std::isfinite(p->learning_rate))
        return fail(c, SCC_ERR_NONFINITE, std::string(who) + ": a non-finite a, b, gamma or learning_rate");
    if (p->a < 0.0 || p->b < 0.0) return fail(c, SCC_ERR_INVALID, std::string(who) + ": a negative a or b");
    const bool dflt = p->a == 0.0 && p->b == 0.0;
    *a = dflt ? SCC_UMAP_A : p->a;
    *b = dflt ? SCC_UMAP_B : p->b;
    return SCC_OK;
}

// the graph of a device table d_idx, d_dist [n][k] (valid: scc_umap_graph checks a caller's, the k-NN stage's is)
int graph_device(scc_ctx* c, int n, int k, const int* d_idx, const double* d_dist, double mix, Graph* g)
{
    hipStream_t s0 = c->s0;
    const size_t nk = (size_t)n * k;
    const int inter = mix == 0.0;
    int rc;
    double *d_rowsum, *d_total, *d_w, *d_vals_u;
    int *d_cnt, *d_cols_u, *d_rowid;
    if ((rc = ws(c, "um_rowsum", (size_t)n, &d_rowsum))) return rc;
    if ((rc = ws(c, "um_total", 1, &d_total))) return rc;
    if ((rc = ws(c, "um_rho", (size_t)n, &g->rho))) return rc;
    if ((rc = ws(c, "um_sigma", (size_t)n, &g->sigma))) return rc;
    if ((rc = ws(c, "um_w", nk, &d_w))) return rc;
    g->w = d_w;
    if ((rc = ws(c, "um_cnt", (size_t)n, &d_cnt))) return rc;
    if ((rc = ws(c, "um_indptr", (size_t)n + 1, &g->indptr))) return rc;
    Scope sc(c, "umap_graph", s0);
    HIPCHK(c, scc_launch_umap_graph_weights(d_dist, n, k, std::log2((double)(k + 1)), d_rowsum, d_total, g->rho,
                                            g->sigma, d_w, s0));
    HIPCHK(c, scc_launch_umap_graph_count(d_idx, n, k, inter, d_cnt, g->indptr, s0));
    HIPCHK(c, hipMemcpyAsync(&g->nnz, g->indptr + n, sizeof(long long), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (g->nnz < 0 || g->nnz > (long long)(2 * nk))
        return fail(c, SCC_ERR_HIP, "umap graph: the entry count is out of range");
    const size_t ne = (size_t)g->nnz;
    if ((rc = ws(c, "um_cols_u", ne, &d_cols_u))) return rc;
    if ((rc = ws(c, "um_vals_u", ne, &d_vals_u))) return rc;
    if ((rc = ws(c, "um_rowid", ne, &d_rowid))) return rc;
    if ((rc = ws(c, "um_cols", ne, &g->cols))) return rc;
    if ((rc = ws(c, "um_vals", ne, &g->vals))) return rc;
    if (ne)
        HIPCHK(c, scc_launch_umap_graph_fill(d_idx, d_w, n, k, inter, mix, g->indptr, g->nnz, d_cnt, d_cols_u, d_vals_u,
                                             d_rowid, g->cols, g->vals, s0));
    return SCC_OK;
}

// the layout of a device CSR from the initialisation in "um_Ya"; *Y: the device result [n][2]
int layout_device(scc_ctx* c, int n, const Graph& g, const scc_umap_params* p, double a, double b, double* d_Ya,
                  double** Y)
{
    hipStream_t s0 = c->s0;
    int rc;
    double *d_Yb, *d_next, *d_nneg;
    unsigned long long* d_wmax;
    if ((rc = ws(c, "um_Yb", 2 * (size_t)n, &d_Yb))) return rc;
    if ((rc = ws(c, "um_next", (size_t)g.nnz, &d_next))) return rc;
    if ((rc = ws(c, "um_nneg", (size_t)g.nnz, &d_nneg))) return rc;
    if ((rc = ws(c, "um_wmax", 1, &d_wmax))) return rc;
    Scope sc(c, "umap_layout", s0);
    HIPCHK(c, scc_launch_umap_layout(g.indptr, g.cols, g.vals, n, g.nnz, p->n_epochs, a, b, p->gamma,
                                     (double)p->negative_sample_rate, p->learning_rate, p->seed, d_wmax, d_next, d_nneg,
                                     d_Ya, d_Yb, s0));
    *Y = (p->n_epochs & 1) ? d_Yb : d_Ya;
    return SCC_OK;
}

int copy_graph_out(scc_ctx* c, const char* who, int n, const Graph& g, int64_t* indptr, int32_t* cols, double* vals,
                   int64_t cap, int64_t* nnz)
{
    if (nnz) *nnz = g.nnz;
    if (g.nnz > cap) return fail(c, SCC_ERR_INVALID, std::string(who) + ": cap is below the graph's entries");
    static_assert(sizeof(long long) == sizeof(int64_t), "indptr is copied as it is");
    HIPCHK(c, hipMemcpyAsync(indptr, g.indptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->s0));
    if (g.nnz) {
        HIPCHK(c, hipMemcpyAsync(cols, g.cols, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost, c->s0));
        HIPCHK(c, hipMemcpyAsync(vals, g.vals, sizeof(double) * (size_t)g.nnz, hipMemcpyDeviceToHost, c->s0));
    }
    return SCC_OK;
}

}  // namespace

extern "C" int scc_umap_graph(scc_ctx* c, int64_t n, int32_t k, const int32_t* idx, const double* dist,
                              const scc_umap_params* prm, int64_t* indptr, int32_t* cols, double* vals, int64_t cap,
                              int64_t* nnz, double* rho, double* sigma, double* weights)
{
    if (!c || !idx || !dist || !prm || !indptr || !cols || !vals)
        return fail(c, SCC_ERR_INVALID, "scc_umap_graph: null argument");
    if (n < 2 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_umap_graph: bad cell count");
    if (k < 1 || k > n - 1) return fail(c, SCC_ERR_INVALID, "scc_umap_graph: k outside 1..n-1");
    if (k > SCC_KNN_MAX_K) return fail(c, SCC_ERR_UNSUPPORTED, "scc_umap_graph: k above SCC_KNN_MAX_K");
    int rc;
    if ((rc = check_graph_params(c, "scc_umap_graph", prm))) return rc;
    const int N = (int)n;
    const size_t nk = (size_t)N * k;
    for (size_t t = 0; t < nk; ++t)
        if (!std::isfinite(dist[t])) return fail(c, SCC_ERR_NONFINITE, "scc_umap_graph: a non-finite distance");
    for (int i = 0; i < N; ++i) {
        const int32_t* ri = idx + (size_t)i * k;
        const double* rd = dist + (size_t)i * k;
        for (int s = 0; s < k; ++s) {
            if (ri[s] < 0 || ri[s] >= N) return fail(c, SCC_ERR_INVALID, "scc_umap_graph: an index outside 0..n-1");
            if (rd[s] < 0.0) return fail(c, SCC_ERR_INVALID, "scc_umap_graph: a negative distance");
            if (s && rd[s] < rd[s - 1])
                return fail(c, SCC_ERR_INVALID, "scc_umap_graph: a row is not ascending in distance");
            for (int q = 0; q < s; ++q)
                if (ri[q] == ri[s]) return fail(c, SCC_ERR_INVALID, "scc_umap_graph: an index listed twice in a row");
        }
    }
    scc_enter(c);
    hipStream_t s0 = c->s0;
    int* d_idx;
    double* d_dist;
    if ((rc = ws(c, "um_idx", nk, &d_idx))) return rc;
    if ((rc = ws(c, "um_dist", nk, &d_dist))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_idx, idx, sizeof(int32_t) * nk, hipMemcpyHostToDevice, s0));
    HIPCHK(c, hipMemcpyAsync(d_dist, dist, sizeof(double) * nk, hipMemcpyHostToDevice, s0));
    Graph g;
    if ((rc = graph_device(c, N, k, d_idx, d_dist, prm->set_op_mix_ratio, &g))) return rc;
    if ((rc = copy_graph_out(c, "scc_umap_graph", N, g, indptr, cols, vals, cap, nnz))) return rc;
    if (rho) HIPCHK(c, hipMemcpyAsync(rho, g.rho, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s0));
    if (sigma) HIPCHK(c, hipMemcpyAsync(sigma, g.sigma, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s0));
    if (weights) HIPCHK(c, hipMemcpyAsync(weights, g.w, sizeof(double) * nk, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    return SCC_OK;
}

extern "C" int scc_umap_layout(scc_ctx* c, int64_t n, const int64_t* indptr, const int32_t* cols, const double* vals,
                               const double* init, const scc_umap_params* prm, double* Y)
{
    if (!c || !indptr || !init || !prm || !Y) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: null argument");
    if (n < 1 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: bad vertex count");
    int rc;
    double a, b;
    if ((rc = check_layout_params(c, "scc_umap_layout", prm, &a, &b))) return rc;
    const int N = (int)n;
    if (indptr[0] != 0) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: indptr does not start at 0");
    for (int i = 0; i < N; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: indptr is not ascending");
    const int64_t ne = indptr[N];
    if (ne > ((int64_t)1 << 40) || (ne && (!cols || !vals)))
        return fail(c, SCC_ERR_INVALID, "scc_umap_layout: bad entry count or null graph");
    for (int64_t p = 0; p < ne; ++p) {
        if (cols[p] < 0 || cols[p] >= N) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: a column outside 0..n-1");
        if (!std::isfinite(vals[p])) return fail(c, SCC_ERR_NONFINITE, "scc_umap_layout: a non-finite weight");
        if (vals[p] < 0.0) return fail(c, SCC_ERR_INVALID, "scc_umap_layout: a negative weight");
    }
    for (size_t t = 0; t < 2 * (size_t)N; ++t)
        if (!std::isfinite(init[t])) return fail(c, SCC_ERR_NONFINITE, "scc_umap_layout: a non-finite init coordinate");
    scc_enter(c);
    hipStream_t s0 = c->s0;
    Graph g;
    g.nnz = ne;
    double *d_Ya, *d_Y;
    if ((rc = ws(c, "um_indptr", (size_t)N + 1, &g.indptr))) return rc;
    if ((rc = ws(c, "um_cols", (size_t)ne, &g.cols))) return rc;
    if ((rc = ws(c, "um_vals", (size_t)ne, &g.vals))) return rc;
    if ((rc = ws(c, "um_Ya", 2 * (size_t)N, &d_Ya))) return rc;
    HIPCHK(c, hipMemcpyAsync(g.indptr, indptr, sizeof(int64_t) * ((size_t)N + 1), hipMemcpyHostToDevice, s0));
    if (ne) {
        HIPCHK(c, hipMemcpyAsync(g.cols, cols, sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, s0));
        HIPCHK(c, hipMemcpyAsync(g.vals, vals, sizeof(double) * (size_t)ne, hipMemcpyHostToDevice, s0));
    }
    HIPCHK(c, hipMemcpyAsync(d_Ya, init, sizeof(double) * 2 * (size_t)N, hipMemcpyHostToDevice, s0));
    if ((rc = layout_device(c, N, g, prm, a, b, d_Ya, &d_Y))) return rc;
    HIPCHK(c, hipMemcpyAsync(Y, d_Y, sizeof(double) * 2 * (size_t)N, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    return SCC_OK;
}

extern "C" int scc_umap_scores(scc_ctx* c, int64_t n, const void* scores, int32_t dims, int32_t n_neighbors,
                               const scc_umap_params* prm, const double* init, double* Y, int64_t* indptr,
                               int32_t* cols, double* vals, int64_t cap, int64_t* nnz)
{
    if (!c || !prm || !Y) return fail(c, SCC_ERR_INVALID, "scc_umap_scores: null argument");
    const bool want_graph = indptr || cols || vals;
    if (want_graph && !(indptr && cols && vals))
        return fail(c, SCC_ERR_INVALID, "scc_umap_scores: the graph needs indptr, cols and vals");
    if (n < 2 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_umap_scores: bad cell count");
    if (dims < 0 || dims > 15) return fail(c, SCC_ERR_INVALID, "scc_umap_scores: dims outside 0..15");
    const int k = n_neighbors - 1;
    if (k < 1 || k > n - 1) return fail(c, SCC_ERR_INVALID, "scc_umap_scores: n_neighbors outside 2..n");
    if (k > SCC_KNN_MAX_K) return fail(c, SCC_ERR_UNSUPPORTED, "scc_umap_scores: n_neighbors above SCC_KNN_MAX_K + 1");
    int rc;
    double a, b;
    if ((rc = check_graph_params(c, "scc_umap_scores", prm))) return rc;
    if ((rc = check_layout_params(c, "scc_umap_scores", prm, &a, &b))) return rc;
    const int N = (int)n;
    if (init)
        for (size_t t = 0; t < 2 * (size_t)N; ++t)
            if (!std::isfinite(init[t]))
                return fail(c, SCC_ERR_NONFINITE, "scc_umap_scores: a non-finite init coordinate");
    scc_enter(c);
    hipStream_t s0 = c->s0;
    const double* P = (const double*)scores;
    if (!P && (rc = kept_scores_device(c, N, "scc_umap_scores", &P))) return rc;
    int* d_idx;
    double *d_dist, *d_Ya, *d_Y;
    if ((rc = knn_scores_device(c, N, P, dims, k, "scc_umap_scores", &d_idx, &d_dist))) return rc;
    Graph g;
    if ((rc = graph_device(c, N, k, d_idx, d_dist, prm->set_op_mix_ratio, &g))) return rc;
    if (want_graph && (rc = copy_graph_out(c, "scc_umap_scores", N, g, indptr, cols, vals, cap, nnz))) return rc;
    if (!want_graph && nnz) *nnz = g.nnz;
    if ((rc = ws(c, "um_Ya", 2 * (size_t)N, &d_Ya))) return rc;
    if (init) {
        HIPCHK(c, hipMemcpyAsync(d_Ya, init, sizeof(double) * 2 * (size_t)N, hipMemcpyHostToDevice, s0));
    } else {
        unsigned long long* d_amax;
        if ((rc = ws(c, "um_amax", 1, &d_amax))) return rc;
        HIPCHK(c, scc_launch_umap_init_scores(P, N, d_amax, d_Ya, s0));
    }
    if ((rc = layout_device(c, N, g, prm, a, b, d_Ya, &d_Y))) return rc;
    HIPCHK(c, hipMemcpyAsync(Y, d_Y, sizeof(double) * 2 * (size_t)N, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    return SCC_OK;
}
