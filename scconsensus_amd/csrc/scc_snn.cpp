// scc_snn.cpp — C ABI of the SNN graph and the modularity clustering
// (include/scc.h: scc_snn_graph, scc_modularity_cluster, scc_snn_clusters_scores;
// kernels: scc_snn.hip).
//
// Each stage has a device form that works on workspace buffers ("sn_*", "mc_*")
// and leaves its result there; the entry points check their host arguments
// before anything is uploaded, run the device forms and copy the answer back.
// scc_snn_clusters_scores runs scc_knn_scores' device stage (scc_distance.cpp:
// knn_scores_device) in front, so the table and both graphs never leave the
// device.  The clustering's host loop reads one small record per sweep (the
// moves and Q) and decides; the device holds every array.  Runs on devices[0].
#include "scc_internal.hpp"

using namespace scc_rt;

typedef long long i64;
typedef unsigned long long u64;

extern "C" {
hipError_t scc_launch_snn_sets(const int* idx, int n, int k, int* S, int* rcnt, i64* rptr, hipStream_t st);
hipError_t scc_launch_snn_count(const int* S, int n, int k, const i64* rptr, int* cur, int* R, double prune, int* cnt,
                                i64* indptr, hipStream_t st);
hipError_t scc_launch_snn_fill(const int* S, int n, int k, const i64* rptr, const int* R, double prune,
                               const i64* indptr, i64 nnz, int* cur, int* cols_u, int* s_u, int* rowid, int* cols,
                               int* shared, double* vals, hipStream_t st);
hipError_t scc_launch_mc_quant(const double* vals, i64 nnz, i64* q, hipStream_t st);
hipError_t scc_launch_mc_degree(const i64* indptr, const i64* q, int n, i64* deg, u64* head, hipStream_t st);
hipError_t scc_launch_mc_init(const i64* deg, int n, int* comm, i64* tot, int* size, hipStream_t st);
hipError_t scc_launch_mc_move(const i64* indptr, const int* cols, const i64* q, const i64* deg, int n, i64 longest,
                              const int* comm, const i64* tot, const int* size, double gamma, double m2, int* gkeys,
                              u64* gsums, int* comm_new, int* moved, hipStream_t st);
int scc_mc_short_row(void);
hipError_t scc_launch_mc_state(const i64* indptr, const int* cols, const i64* q, const i64* deg, int n, const int* comm,
                               double gamma, double m2, i64* tot, int* size, i64* inc, double* term, double* out_q,
                               hipStream_t st);
hipError_t scc_launch_mc_renumber(const i64* indptr, const int* cols, int n, i64 nnz, const int* comm, const int* size,
                                  int* flag, i64* newid, int n0, int* member, u64* key, hipStream_t st);
hipError_t scc_mc_aggregate_bytes(i64 nnz, size_t* bytes);
hipError_t scc_launch_mc_aggregate(void* tmp, size_t tmp_bytes, const u64* key, const i64* q, i64 nnz, int bits,
                                   u64* key_s, i64* q_s, u64* ukey, i64* uq, i64* ne, hipStream_t st);
hipError_t scc_launch_mc_coarse(const u64* ukey, i64 ne, int nc, int* cols, int* cnt, i64* indptr, hipStream_t st);
}

namespace {

constexpr int kMaxSweeps = 256;
constexpr int kMaxLevels = SCC_MODULARITY_MAX_LEVELS;

struct SnnGraph {  // device CSR in the workspace
    i64* indptr = nullptr;
    int* cols = nullptr;
    int* shared = nullptr;
    double* vals = nullptr;
    i64 nnz = 0;
};

struct ClusterOut {
    int n_clusters = 0, n_levels = 0;
    double modularity = 0.0;
    int sweeps[kMaxLevels] = {0};
};

int check_prune(scc_ctx* c, const char* who, double prune)
{
    if (!std::isfinite(prune)) return fail(c, SCC_ERR_NONFINITE, std::string(who) + ": a non-finite prune");
    if (!(prune >= 0.0 && prune <= 1.0)) return fail(c, SCC_ERR_INVALID, std::string(who) + ": prune outside [0, 1]");
    return SCC_OK;
}

int check_resolution(scc_ctx* c, const char* who, double gamma)
{
    if (!std::isfinite(gamma)) return fail(c, SCC_ERR_NONFINITE, std::string(who) + ": a non-finite resolution");
    if (!(gamma > 0.0)) return fail(c, SCC_ERR_INVALID, std::string(who) + ": resolution not above 0");
    return SCC_OK;
}

// the SNN graph of a device table d_idx [n][k] (valid: scc_snn_graph checks a caller's, the k-NN stage's is)
int snn_device(scc_ctx* c, int n, int k, const int* d_idx, double prune, SnnGraph* g)
{
    hipStream_t s0 = c->s0;
    const size_t nK = (size_t)n * (k + 1);
    int rc;
    int *d_S, *d_rcnt, *d_cur, *d_R, *d_cnt, *d_cols_u, *d_su, *d_rowid;
    i64* d_rptr;
    if ((rc = ws(c, "sn_S", nK, &d_S))) return rc;
    if ((rc = ws(c, "sn_R", nK, &d_R))) return rc;
    if ((rc = ws(c, "sn_rcnt", (size_t)n, &d_rcnt))) return rc;
    if ((rc = ws(c, "sn_rptr", (size_t)n + 1, &d_rptr))) return rc;
    if ((rc = ws(c, "sn_cur", (size_t)n, &d_cur))) return rc;
    if ((rc = ws(c, "sn_cnt", (size_t)n, &d_cnt))) return rc;
    if ((rc = ws(c, "sn_indptr", (size_t)n + 1, &g->indptr))) return rc;
    Scope sc(c, "snn_graph", s0);
    HIPCHK(c, scc_launch_snn_sets(d_idx, n, k, d_S, d_rcnt, d_rptr, s0));
    HIPCHK(c, scc_launch_snn_count(d_S, n, k, d_rptr, d_cur, d_R, prune, d_cnt, g->indptr, s0));
    HIPCHK(c, hipMemcpyAsync(&g->nnz, g->indptr + n, sizeof(i64), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (g->nnz < 0 || g->nnz > (i64)n * (n - 1)) return fail(c, SCC_ERR_HIP, "snn graph: the entry count is out of range");
    const size_t ne = (size_t)g->nnz;
    if ((rc = ws(c, "sn_cols_u", ne, &d_cols_u))) return rc;
    if ((rc = ws(c, "sn_s_u", ne, &d_su))) return rc;
    if ((rc = ws(c, "sn_rowid", ne, &d_rowid))) return rc;
    if ((rc = ws(c, "sn_cols", ne, &g->cols))) return rc;
    if ((rc = ws(c, "sn_shared", ne, &g->shared))) return rc;
    if ((rc = ws(c, "sn_vals", ne, &g->vals))) return rc;
    if (ne)
        HIPCHK(c, scc_launch_snn_fill(d_S, n, k, d_rptr, d_R, prune, g->indptr, g->nnz, d_cur, d_cols_u, d_su, d_rowid,
                                      g->cols, g->shared, g->vals, s0));
    return SCC_OK;
}

int copy_snn_out(scc_ctx* c, const char* who, int n, const SnnGraph& g, int64_t* indptr, int32_t* cols, double* vals,
                 int32_t* shared, int64_t cap, int64_t* nnz)
{
    if (nnz) *nnz = g.nnz;
    if (g.nnz > cap) return fail(c, SCC_ERR_INVALID, std::string(who) + ": cap is below the graph's entries");
    static_assert(sizeof(i64) == sizeof(int64_t), "indptr is copied as it is");
    HIPCHK(c, hipMemcpyAsync(indptr, g.indptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->s0));
    if (g.nnz) {
        const size_t ne = (size_t)g.nnz;
        HIPCHK(c, hipMemcpyAsync(cols, g.cols, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, c->s0));
        HIPCHK(c, hipMemcpyAsync(vals, g.vals, sizeof(double) * ne, hipMemcpyDeviceToHost, c->s0));
        if (shared) HIPCHK(c, hipMemcpyAsync(shared, g.shared, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, c->s0));
    }
    return SCC_OK;
}

// labels numbered by (size descending, smallest member ascending) from the members' final communities
void number_labels(const std::vector<int>& member, int nc, int32_t* labels, int* n_clusters)
{
    const int n = (int)member.size();
    std::vector<int> size(nc, 0), first(nc, n), order, newid(nc, -1);
    for (int v = 0; v < n; ++v) {
        ++size[member[v]];
        first[member[v]] = std::min(first[member[v]], v);
    }
    for (int q = 0; q < nc; ++q)
        if (size[q]) order.push_back(q);
    std::sort(order.begin(), order.end(),
              [&](int a, int b) { return size[a] != size[b] ? size[a] > size[b] : first[a] < first[b]; });
    for (size_t r = 0; r < order.size(); ++r) newid[order[r]] = (int)r;
    for (int v = 0; v < n; ++v) labels[v] = newid[member[v]];
    *n_clusters = (int)order.size();
}

// The clustering of a device CSR (n0 vertices, integer weights q; columns ascending, symmetric: a caller's graph is
// checked by scc_modularity_cluster, scc_snn_graph's is).  The level's graph alternates between two buffer sets.
int cluster_device(scc_ctx* c, int n0, const i64* d_indptr, const int* d_cols, const i64* d_q, i64 nnz0, double gamma,
                   int32_t* labels, ClusterOut* out)
{
    hipStream_t s0 = c->s0;
    int rc;
    Scope sc(c, "modularity_cluster", s0);
    const size_t N0 = (size_t)n0, E0 = (size_t)std::max<i64>(nnz0, 1);
    i64 *d_deg, *d_tot[2], *d_inc, *d_newid, *d_ip[2], *d_qq[2], *d_qs, *d_ne;
    int *d_comm[2], *d_size[2], *d_moved, *d_flag, *d_member, *d_cc[2], *d_gkeys = nullptr;
    u64 *d_head, *d_key, *d_keys, *d_ukey, *d_gsums = nullptr;
    double *d_term, *d_q_out;
    if ((rc = ws(c, "mc_deg", N0, &d_deg))) return rc;
    if ((rc = ws(c, "mc_tot0", N0, &d_tot[0])) || (rc = ws(c, "mc_tot1", N0, &d_tot[1]))) return rc;
    if ((rc = ws(c, "mc_inc", N0, &d_inc))) return rc;
    if ((rc = ws(c, "mc_newid", N0 + 1, &d_newid))) return rc;
    if ((rc = ws(c, "mc_comm0", N0, &d_comm[0])) || (rc = ws(c, "mc_comm1", N0, &d_comm[1]))) return rc;
    if ((rc = ws(c, "mc_size0", N0, &d_size[0])) || (rc = ws(c, "mc_size1", N0, &d_size[1]))) return rc;
    if ((rc = ws(c, "mc_flag", N0, &d_flag))) return rc;
    if ((rc = ws(c, "mc_member", N0, &d_member))) return rc;
    if ((rc = ws(c, "mc_term", N0, &d_term))) return rc;
    if ((rc = ws(c, "mc_head", 2, &d_head))) return rc;
    if ((rc = ws(c, "mc_moved", 1, &d_moved))) return rc;
    if ((rc = ws(c, "mc_qout", 1, &d_q_out))) return rc;
    if ((rc = ws(c, "mc_ne", 1, &d_ne))) return rc;
    // the coarse graphs (never more entries or rows than level 0) and the aggregation's arrays
    if ((rc = ws(c, "mc_ip0", N0 + 1, &d_ip[0])) || (rc = ws(c, "mc_ip1", N0 + 1, &d_ip[1]))) return rc;
    if ((rc = ws(c, "mc_cols0", E0, &d_cc[0])) || (rc = ws(c, "mc_cols1", E0, &d_cc[1]))) return rc;
    if ((rc = ws(c, "mc_q0", E0, &d_qq[0])) || (rc = ws(c, "mc_q1", E0, &d_qq[1]))) return rc;
    if ((rc = ws(c, "mc_key", E0, &d_key)) || (rc = ws(c, "mc_keys", E0, &d_keys))) return rc;
    if ((rc = ws(c, "mc_ukey", E0, &d_ukey)) || (rc = ws(c, "mc_qs", E0, &d_qs))) return rc;
    size_t tmp_bytes = 0;
    HIPCHK(c, scc_mc_aggregate_bytes(std::max<i64>(nnz0, 1), &tmp_bytes));
    char* d_tmp;
    if ((rc = ws(c, "mc_tmp", tmp_bytes, &d_tmp))) return rc;

    std::vector<int> member(N0);
    for (int v = 0; v < n0; ++v) member[v] = v;
    HIPCHK(c, hipMemcpyAsync(d_member, member.data(), sizeof(int) * N0, hipMemcpyHostToDevice, s0));

    const i64* ip = d_indptr;
    const int* cc = d_cols;
    const i64* qq = d_q;
    int n = n0, nc_final = n0;
    i64 nnz = nnz0;
    double m2d = 0.0;
    *out = ClusterOut();
    for (int level = 0; level < kMaxLevels; ++level) {
        u64 head[2];
        HIPCHK(c, scc_launch_mc_degree(ip, qq, n, d_deg, d_head, s0));
        HIPCHK(c, hipMemcpyAsync(head, d_head, sizeof(head), hipMemcpyDeviceToHost, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        if (level == 0) {
            if (head[0] == 0) break;  // no weight at all: every vertex is a cluster of its own
            if (head[0] >= (1ull << 62)) return fail(c, SCC_ERR_UNSUPPORTED, "modularity: the total weight is 2^62 or more");
            m2d = (double)(i64)head[0];
        }
        const i64 longest = (i64)head[1];
        if (longest > scc_mc_short_row()) {  // rows for the global tables: 2 slots per entry
            if ((rc = ws(c, "mc_gkeys", 2 * (size_t)nnz, &d_gkeys))) return rc;
            if ((rc = ws(c, "mc_gsums", 2 * (size_t)nnz, &d_gsums))) return rc;
        }
        int a = 0;
        HIPCHK(c, scc_launch_mc_init(d_deg, n, d_comm[a], d_tot[a], d_size[a], s0));
        HIPCHK(c, scc_launch_mc_state(ip, cc, qq, d_deg, n, d_comm[a], gamma, m2d, d_tot[a], d_size[a], d_inc, d_term,
                                      d_q_out, s0));
        double q_old = 0.0;
        HIPCHK(c, hipMemcpyAsync(&q_old, d_q_out, sizeof(double), hipMemcpyDeviceToHost, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        if (level == 0) out->modularity = q_old;
        int sweeps = 0, accepted = 0;
        while (sweeps < kMaxSweeps) {
            ++sweeps;
            const int b = a ^ 1;
            int moved = 0;
            double q_new = 0.0;
            HIPCHK(c, scc_launch_mc_move(ip, cc, qq, d_deg, n, longest, d_comm[a], d_tot[a], d_size[a], gamma, m2d,
                                         d_gkeys, d_gsums, d_comm[b], d_moved, s0));
            HIPCHK(c, scc_launch_mc_state(ip, cc, qq, d_deg, n, d_comm[b], gamma, m2d, d_tot[b], d_size[b], d_inc, d_term,
                                          d_q_out, s0));
            HIPCHK(c, hipMemcpyAsync(&moved, d_moved, sizeof(int), hipMemcpyDeviceToHost, s0));
            HIPCHK(c, hipMemcpyAsync(&q_new, d_q_out, sizeof(double), hipMemcpyDeviceToHost, s0));
            HIPCHK(c, hipStreamSynchronize(s0));
            if (moved == 0) break;
            if (q_new <= q_old) break;  // the sweep is discarded: buffer a still holds the accepted state
            a = b;
            q_old = q_new;
            ++accepted;
        }
        if (accepted) out->modularity = q_old;
        out->sweeps[level] = sweeps;
        out->n_levels = level + 1;
        // renumber the communities that have members; the members follow; the coarse keys
        HIPCHK(c, scc_launch_mc_renumber(ip, cc, n, nnz, d_comm[a], d_size[a], d_flag, d_newid, n0, d_member, d_key, s0));
        i64 nc64 = 0;
        HIPCHK(c, hipMemcpyAsync(&nc64, d_newid + n, sizeof(i64), hipMemcpyDeviceToHost, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        if (nc64 < 1 || nc64 > n) return fail(c, SCC_ERR_HIP, "modularity: the community count is out of range");
        nc_final = (int)nc64;
        if (nc64 == n) break;  // the level merged nothing (the members' renumbering was the identity)
        if (level + 1 == kMaxLevels) break;
        const int nb = level & 1;
        i64 ne = 0;
        if (nnz > 0) {
            int bits = 33;
            while (bits < 64 && (nc64 >> (bits - 32)) != 0) ++bits;
            HIPCHK(c, scc_launch_mc_aggregate(d_tmp, tmp_bytes, d_key, qq, nnz, bits, d_keys, d_qs, d_ukey, d_qq[nb], d_ne,
                                              s0));
            HIPCHK(c, hipMemcpyAsync(&ne, d_ne, sizeof(i64), hipMemcpyDeviceToHost, s0));
            HIPCHK(c, hipStreamSynchronize(s0));
            if (ne < 1 || ne > nnz) return fail(c, SCC_ERR_HIP, "modularity: the coarse entry count is out of range");
        }
        HIPCHK(c, scc_launch_mc_coarse(d_ukey, ne, (int)nc64, d_cc[nb], d_flag, d_ip[nb], s0));
        ip = d_ip[nb];
        cc = d_cc[nb];
        qq = d_qq[nb];
        n = (int)nc64;
        nnz = ne;
    }
    HIPCHK(c, hipMemcpyAsync(member.data(), d_member, sizeof(int) * N0, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    for (int v = 0; v < n0; ++v)
        if (member[v] < 0 || member[v] >= nc_final) return fail(c, SCC_ERR_HIP, "modularity: a member outside its level");
    number_labels(member, nc_final, labels, &out->n_clusters);
    return SCC_OK;
}

void copy_cluster_out(const ClusterOut& o, int32_t* n_clusters, double* modularity, int32_t* n_levels, int32_t* sweeps)
{
    if (n_clusters) *n_clusters = o.n_clusters;
    if (modularity) *modularity = o.modularity;
    if (n_levels) *n_levels = o.n_levels;
    if (sweeps)
        for (int l = 0; l < kMaxLevels; ++l) sweeps[l] = o.sweeps[l];
}

}  // namespace

extern "C" int scc_snn_graph(scc_ctx* c, int64_t n, int32_t k, const int32_t* idx, double prune, int64_t* indptr,
                             int32_t* cols, double* vals, int32_t* shared, int64_t cap, int64_t* nnz)
{
    if (!c || !idx || !indptr || !cols || !vals) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: null argument");
    if (n < 2 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: bad cell count");
    if (k < 1 || k > n - 1) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: k outside 1..n-1");
    if (k > SCC_KNN_MAX_K) return fail(c, SCC_ERR_UNSUPPORTED, "scc_snn_graph: k above SCC_KNN_MAX_K");
    int rc;
    if ((rc = check_prune(c, "scc_snn_graph", prune))) return rc;
    const int N = (int)n;
    const size_t nk = (size_t)N * k;
    for (int i = 0; i < N; ++i) {
        const int32_t* ri = idx + (size_t)i * k;
        for (int s = 0; s < k; ++s) {
            if (ri[s] < 0 || ri[s] >= N) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: an index outside 0..n-1");
            if (ri[s] == i) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: a row lists itself");
            for (int q = 0; q < s; ++q)
                if (ri[q] == ri[s]) return fail(c, SCC_ERR_INVALID, "scc_snn_graph: an index listed twice in a row");
        }
    }
    scc_enter(c);
    hipStream_t s0 = c->s0;
    int* d_idx;
    if ((rc = ws(c, "sn_idx", nk, &d_idx))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_idx, idx, sizeof(int32_t) * nk, hipMemcpyHostToDevice, s0));
    SnnGraph g;
    if ((rc = snn_device(c, N, k, d_idx, prune, &g))) return rc;
    if ((rc = copy_snn_out(c, "scc_snn_graph", N, g, indptr, cols, vals, shared, cap, nnz))) return rc;
    HIPCHK(c, hipStreamSynchronize(s0));
    return SCC_OK;
}

extern "C" int scc_modularity_cluster(scc_ctx* c, int64_t n, const int64_t* indptr, const int32_t* cols,
                                      const double* vals, double resolution, int32_t* labels, int32_t* n_clusters,
                                      double* modularity, int32_t* n_levels, int32_t* sweeps)
{
    const char* who = "scc_modularity_cluster";
    if (!c || !indptr || !labels) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: null argument");
    if (n < 1 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: bad vertex count");
    int rc;
    if ((rc = check_resolution(c, who, resolution))) return rc;
    const int N = (int)n;
    if (indptr[0] != 0) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: indptr does not start at 0");
    for (int i = 0; i < N; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: indptr is not ascending");
    const int64_t ne = indptr[N];
    if (ne > ((int64_t)1 << 40) || (ne && (!cols || !vals)))
        return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: bad entry count or null graph");
    std::vector<i64> q((size_t)ne);
    unsigned long long m2 = 0;
    for (int i = 0; i < N; ++i)
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            if (cols[p] < 0 || cols[p] >= N)
                return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: a column outside 0..n-1");
            if (p > indptr[i] && cols[p] <= cols[p - 1])
                return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: a row's columns do not ascend");
            if (cols[p] == i) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: a diagonal entry");
            if (!std::isfinite(vals[p])) return fail(c, SCC_ERR_NONFINITE, "scc_modularity_cluster: a non-finite weight");
            if (vals[p] < 0.0) return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: a negative weight");
            if (vals[p] > 1048576.0) return fail(c, SCC_ERR_UNSUPPORTED, "scc_modularity_cluster: a weight above 2^20");
            q[(size_t)p] = (i64)std::rint(vals[p] * 4294967296.0);
            m2 += (unsigned long long)q[(size_t)p];  // each at most 2^52: no wrap before the test below
            if (m2 >= (1ull << 62))
                return fail(c, SCC_ERR_UNSUPPORTED, "scc_modularity_cluster: the total weight is 2^62 or more");
        }
    for (int i = 0; i < N; ++i)  // (i, j) and (j, i) hold the same bits
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            const int j = cols[p];
            const int32_t* lo = cols + indptr[j];
            const int32_t* hi = cols + indptr[j + 1];
            const int32_t* at = std::lower_bound(lo, hi, i);
            if (at == hi || *at != i || std::memcmp(&vals[at - cols], &vals[p], sizeof(double)) != 0)
                return fail(c, SCC_ERR_INVALID, "scc_modularity_cluster: the graph is not symmetric");
        }
    scc_enter(c);
    hipStream_t s0 = c->s0;
    i64 *d_indptr, *d_q;
    int* d_cols;
    const size_t E = (size_t)std::max<int64_t>(ne, 1);
    if ((rc = ws(c, "mc_in_indptr", (size_t)N + 1, &d_indptr))) return rc;
    if ((rc = ws(c, "mc_in_cols", E, &d_cols))) return rc;
    if ((rc = ws(c, "mc_in_q", E, &d_q))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_indptr, indptr, sizeof(int64_t) * ((size_t)N + 1), hipMemcpyHostToDevice, s0));
    if (ne) {
        HIPCHK(c, hipMemcpyAsync(d_cols, cols, sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, s0));
        HIPCHK(c, hipMemcpyAsync(d_q, q.data(), sizeof(i64) * (size_t)ne, hipMemcpyHostToDevice, s0));
    }
    HIPCHK(c, hipStreamSynchronize(s0));  // (q is a local)
    ClusterOut o;
    if ((rc = cluster_device(c, N, d_indptr, d_cols, d_q, ne, resolution, labels, &o))) return rc;
    copy_cluster_out(o, n_clusters, modularity, n_levels, sweeps);
    return SCC_OK;
}

extern "C" int scc_snn_clusters_scores(scc_ctx* c, int64_t n, const void* scores, int32_t dims, int32_t k_param,
                                       double prune, double resolution, int32_t* labels, int32_t* n_clusters,
                                       double* modularity, int32_t* n_levels, int32_t* sweeps, int64_t* indptr,
                                       int32_t* cols, double* vals, int64_t cap, int64_t* nnz)
{
    const char* who = "scc_snn_clusters_scores";
    if (!c || !labels) return fail(c, SCC_ERR_INVALID, "scc_snn_clusters_scores: null argument");
    const bool want_graph = indptr || cols || vals;
    if (want_graph && !(indptr && cols && vals))
        return fail(c, SCC_ERR_INVALID, "scc_snn_clusters_scores: the graph needs indptr, cols and vals");
    if (n < 2 || n > ((int64_t)1 << 27)) return fail(c, SCC_ERR_INVALID, "scc_snn_clusters_scores: bad cell count");
    if (dims < 0 || dims > 15) return fail(c, SCC_ERR_INVALID, "scc_snn_clusters_scores: dims outside 0..15");
    const int k = k_param - 1;
    if (k < 1 || k > n - 1) return fail(c, SCC_ERR_INVALID, "scc_snn_clusters_scores: k_param outside 2..n");
    if (k > SCC_KNN_MAX_K) return fail(c, SCC_ERR_UNSUPPORTED, "scc_snn_clusters_scores: k_param above SCC_KNN_MAX_K + 1");
    int rc;
    if ((rc = check_prune(c, who, prune))) return rc;
    if ((rc = check_resolution(c, who, resolution))) return rc;
    const int N = (int)n;
    scc_enter(c);
    hipStream_t s0 = c->s0;
    const double* P = (const double*)scores;
    if (!P && (rc = kept_scores_device(c, N, who, &P))) return rc;
    int* d_idx;
    double* d_dist;
    if ((rc = knn_scores_device(c, N, P, dims, k, who, &d_idx, &d_dist))) return rc;
    SnnGraph g;
    if ((rc = snn_device(c, N, k, d_idx, prune, &g))) return rc;
    if (want_graph && (rc = copy_snn_out(c, who, N, g, indptr, cols, vals, nullptr, cap, nnz))) return rc;
    if (!want_graph && nnz) *nnz = g.nnz;
    i64* d_q;
    if ((rc = ws(c, "mc_in_q", (size_t)std::max<i64>(g.nnz, 1), &d_q))) return rc;
    HIPCHK(c, scc_launch_mc_quant(g.vals, g.nnz, d_q, s0));
    ClusterOut o;
    if ((rc = cluster_device(c, N, g.indptr, g.cols, d_q, g.nnz, resolution, labels, &o))) return rc;
    copy_cluster_out(o, n_clusters, modularity, n_levels, sweeps);
    return SCC_OK;
}
