// scc_runtime.cpp — host runtime behind the C ABI (include/scc.h).
//
// Owns the HIP device, two streams, a grow-only HBM workspace, the exact
// Wilcoxon count table, and optional HIP-event kernel timers; creates and
// destroys the datasets.  The DE driver is scc_de.cpp.  No CPU fallback
// exists: without a HIP device every entry point returns SCC_ERR_HIP.
#include "scc_internal.hpp"

#include <atomic>
#include <cstring>

using namespace scc_rt;

// ====================================================================== ctx
static int ctx_create_one(int device, bool profile, scc_ctx** out)
{
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        hipGetLastError();
        return SCC_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return SCC_ERR_INVALID;
    static std::atomic<uint64_t> next_serial{1};
    scc_ctx* c = new scc_ctx();
    c->serial = next_serial.fetch_add(1);
    c->device = device;
    c->profile = profile;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->s0, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s1, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&c->sw[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->sw[1], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_wj[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_wj[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_wfork, hipEventDisableTiming) != hipSuccess) {
        hipGetLastError();
        delete c;
        return SCC_ERR_HIP;
    }
    c->own_s0 = c->s0;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) {
        hipGetLastError();
        c->n_cu = 256;
    }
    *out = c;
    return SCC_OK;
}

extern "C" int scc_ctx_create(const scc_opts* opts, scc_ctx** out)
{
    if (!out) return SCC_ERR_INVALID;
    *out = nullptr;
    const bool profile = opts ? (opts->profile != 0) : false;
    const int nd = (opts && opts->n_devices > 1) ? opts->n_devices : 1;
    if (nd > 1 && !opts->devices) return SCC_ERR_INVALID;
    const int dev0 = nd > 1 ? opts->devices[0] : (opts ? opts->device : 0);
    scc_ctx* c = nullptr;
    int rc = ctx_create_one(dev0, profile, &c);
    if (rc) return rc;
    for (int i = 1; i < nd; ++i) {
        scc_ctx* p = nullptr;
        if ((rc = ctx_create_one(opts->devices[i], profile, &p))) {
            scc_ctx_destroy(c);
            return rc;
        }
        c->peers.push_back(p);
        if (p->device != c->device) {  // xGMI peer access both ways (already enabled is fine)
            hipSetDevice(c->device);
            if (hipDeviceEnablePeerAccess(p->device, 0) != hipSuccess) hipGetLastError();
            hipSetDevice(p->device);
            if (hipDeviceEnablePeerAccess(c->device, 0) != hipSuccess) hipGetLastError();
        }
    }
    scc_enter(c);
    *out = c;
    return SCC_OK;
}

extern "C" int scc_device_count(int32_t* n)
{
    if (!n) return SCC_ERR_INVALID;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess) {
        hipGetLastError();
        nd = 0;
    }
    *n = nd;
    return SCC_OK;
}

extern "C" void scc_distance_release(scc_ctx* c);

extern "C" void scc_ctx_destroy(scc_ctx* c)
{
    if (!c) return;
    for (scc_ctx* p : c->peers) scc_ctx_destroy(p);
    c->peers.clear();
    scc_enter(c);
    scc_distance_release(c);
    hipStreamSynchronize(c->s0);
    hipStreamSynchronize(c->s1);
    for (auto& kv : c->ws) {
        scc_fsi_forget(kv.second.first, kv.second.second);
        hipFree(kv.second.first);
    }
    for (auto& pe : c->pending) {
        hipEventDestroy(pe.a);
        hipEventDestroy(pe.b);
    }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->h_tab) hipHostFree(c->h_tab);
    if (c->h_flag) hipHostFree(c->h_flag);
    if (c->ev_genes) hipEventSynchronize(c->ev_genes), hipEventDestroy(c->ev_genes);
    if (c->h_genes) hipHostFree(c->h_genes);
    if (c->h_dstage) hipHostFree(c->h_dstage);
    if (c->h_core) hipHostFree(c->h_core);
    hipEventDestroy(c->ev_fork);
    hipEventDestroy(c->ev_join);
    for (int i = 0; i < 2; ++i) {
        hipStreamSynchronize(c->sw[i]);
        hipStreamDestroy(c->sw[i]);
        hipEventDestroy(c->ev_wj[i]);
    }
    hipEventDestroy(c->ev_wfork);
    hipStreamSynchronize(c->s0);
    hipStreamDestroy(c->own_s0);
    hipStreamDestroy(c->s1);
    delete c;
}

extern "C" const char* scc_ctx_last_error(const scc_ctx* c) { return c ? c->err.c_str() : "null context"; }

namespace scc_rt {
void scc_enter(const scc_ctx* c)
{
    hipSetDevice(c->device);
    (void)hipGetLastError();
}

int check_pending_eig(scc_ctx* c)
{
    if (!c->eig_flag_pending || !c->h_flag) return SCC_OK;
    c->eig_flag_pending = false;
    const unsigned int v = *(volatile unsigned int*)c->h_flag;
    *(volatile unsigned int*)c->h_flag = 0;
    c->eig_err = v;
    if (v) return fail(c, SCC_ERR_HIP, "scc_distance: eigensolver workgroup hand-off timed out");
    return SCC_OK;
}

}  // namespace scc_rt

extern "C" int scc_ctx_synchronize(scc_ctx* c)
{
    if (!c) return SCC_ERR_INVALID;
    scc_enter(c);
    HIPCHK(c, hipStreamSynchronize(c->s0));
    HIPCHK(c, hipStreamSynchronize(c->s1));
    for (scc_ctx* p : c->peers) {
        int rc = scc_ctx_synchronize(p);
        if (rc) return fail(c, rc, p->err);
    }
    scc_enter(c);
    return check_pending_eig(c);
}

extern "C" int scc_ctx_set_stream(scc_ctx* c, void* stream, int32_t external)
{
    if (!c) return SCC_ERR_INVALID;
    scc_enter(c);
    HIPCHK(c, hipStreamSynchronize(c->s0));  // work already queued on the old stream first
    c->s0 = external ? (hipStream_t)stream : c->own_s0;
    return SCC_OK;
}

extern "C" int scc_ctx_kernel_time(const scc_ctx* cc, const char* name, double* total_ms, int64_t* launches)
{
    scc_ctx* c = const_cast<scc_ctx*>(cc);
    if (!c || !name) return SCC_ERR_INVALID;
    scc_enter(c);
    resolve_timers(c);
    auto it = c->timers.find(name);
    if (total_ms) *total_ms = it == c->timers.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->timers.end() ? 0 : it->second.n;
    return SCC_OK;
}

extern "C" void scc_ctx_reset_timers(scc_ctx* c)
{
    if (!c) return;
    scc_enter(c);
    resolve_timers(c);
    c->timers.clear();
}

// ====================================================================== dataset
// device list: the dataset's replica on every peer engine (the same device:
// its buffers borrowed; another device: owned copies over xGMI)
static int replicate(scc_ctx* c, scc_dataset* d)
{
    for (scc_ctx* p : c->peers) {
        scc_dataset* r = new scc_dataset();
        r->ctx = p;
        r->device = p->device;
        r->G = d->G;
        r->N = d->N;
        r->nnz = d->nnz;
        r->dense = d->dense;
        d->reps.push_back(r);
        if (p->device == c->device) {
            r->d_indptr = d->d_indptr;
            r->d_rows = d->d_rows;
            r->d_vals = d->d_vals;
            r->d_dense = d->d_dense;
            r->owned = false;
            continue;
        }
        r->owned = true;
        hipSetDevice(p->device);
        auto peer = [&](void** dst, const void* src, size_t bytes) {
            if (hipMalloc(dst, std::max<size_t>(bytes, 8)) != hipSuccess) {
                hipGetLastError();
                *dst = nullptr;
                return false;
            }
            if (bytes && hipMemcpyPeerAsync(*dst, p->device, src, c->device, bytes, p->s0) != hipSuccess) {
                hipGetLastError();
                return false;
            }
            return true;
        };
        bool ok = true;
        if (d->dense) {
            ok = peer((void**)&r->d_dense, d->d_dense, sizeof(double) * (size_t)d->G * d->N);
        } else {
            ok = peer((void**)&r->d_indptr, d->d_indptr, sizeof(long long) * (d->N + 1)) &&
                 peer((void**)&r->d_rows, d->d_rows, sizeof(int) * d->nnz) &&
                 peer((void**)&r->d_vals, d->d_vals, sizeof(double) * d->nnz);
        }
        if (!ok || hipStreamSynchronize(p->s0) != hipSuccess) {
            hipGetLastError();
            hipSetDevice(c->device);
            return fail(c, SCC_ERR_OOM, "dataset replication to a peer device failed");
        }
    }
    scc_enter(c);
    return SCC_OK;
}

static int finish_create(scc_ctx* c, scc_dataset* d, scc_dataset** out)
{
    int rc = replicate(c, d);
    if (rc) {
        scc_dataset_destroy(d);
        return rc;
    }
    *out = d;
    return SCC_OK;
}

extern "C" int scc_dataset_create_csc(scc_ctx* c, const int64_t* indptr, const int32_t* rows, const double* vals,
                                      int64_t G, int64_t N, int64_t nnz, int32_t kind, scc_dataset** out)
{
    if (!c || !out || !indptr || G <= 0 || N <= 0 || nnz < 0 || (nnz > 0 && (!rows || !vals)))
        return fail(c, SCC_ERR_INVALID, "scc_dataset_create_csc: bad arguments");
    if (G > INT32_MAX || N > INT32_MAX) return fail(c, SCC_ERR_UNSUPPORTED, "dimensions exceed int32");
    scc_enter(c);
    scc_dataset* d = new scc_dataset();
    d->ctx = c;
    d->device = c->device;
    d->G = G;
    d->N = N;
    d->nnz = nnz;
    if (kind == SCC_PTR_DEVICE) {
        d->d_indptr = (long long*)indptr;
        d->d_rows = (int*)rows;
        d->d_vals = (double*)vals;
        d->owned = false;
    } else {
        d->owned = true;
        if (hipMalloc(&d->d_indptr, sizeof(long long) * (N + 1)) != hipSuccess ||
            hipMalloc(&d->d_rows, sizeof(int) * std::max<int64_t>(nnz, 1)) != hipSuccess ||
            hipMalloc(&d->d_vals, sizeof(double) * std::max<int64_t>(nnz, 1)) != hipSuccess) {
            hipGetLastError();
            scc_dataset_destroy(d);
            return fail(c, SCC_ERR_OOM, "dataset allocation failed");
        }
        hipMemcpyAsync(d->d_indptr, indptr, sizeof(long long) * (N + 1), hipMemcpyHostToDevice, c->s0);
        if (nnz > 0) {
            hipMemcpyAsync(d->d_rows, rows, sizeof(int) * nnz, hipMemcpyHostToDevice, c->s0);
            hipMemcpyAsync(d->d_vals, vals, sizeof(double) * nnz, hipMemcpyHostToDevice, c->s0);
        }
        if (hipStreamSynchronize(c->s0) != hipSuccess) {
            hipGetLastError();
            scc_dataset_destroy(d);
            return fail(c, SCC_ERR_HIP, "dataset upload failed");
        }
    }
    return finish_create(c, d, out);
}

extern "C" int scc_dataset_create_csr(scc_ctx* c, const int64_t* indptr, const int32_t* cols, const double* vals,
                                      int64_t G, int64_t N, int64_t nnz, int32_t kind, scc_dataset** out)
{
    if (!c || !out || !indptr || G <= 0 || N <= 0 || nnz < 0 || (nnz > 0 && (!cols || !vals)))
        return fail(c, SCC_ERR_INVALID, "scc_dataset_create_csr: bad arguments");
    if (G > INT32_MAX || N > INT32_MAX) return fail(c, SCC_ERR_UNSUPPORTED, "dimensions exceed int32");
    if (nnz > UINT32_MAX) return fail(c, SCC_ERR_UNSUPPORTED, "more than 2^32 stored values");
    if (G > kCsrMaxGenes)  // before any allocation or upload
        return fail(c, SCC_ERR_UNSUPPORTED, "scc_dataset_create_csr: more than 262,144 genes");
    scc_enter(c);
    hipStream_t s0 = c->s0;
    // the CSR on the device (borrowed, or a temporary upload)
    long long* d_ip = nullptr;
    int* d_cols = nullptr;
    double* d_vals = nullptr;
    std::vector<void*> tmp;
    auto cleanup = [&]() {
        hipStreamSynchronize(s0);
        for (void* p : tmp) hipFree(p);
    };
    auto dalloc = [&](void** p, size_t bytes) {
        if (hipMalloc(p, std::max<size_t>(bytes, 8)) != hipSuccess) {
            hipGetLastError();
            *p = nullptr;
            return false;
        }
        tmp.push_back(*p);
        return true;
    };
    if (kind == SCC_PTR_DEVICE) {
        d_ip = (long long*)indptr;
        d_cols = (int*)cols;
        d_vals = (double*)vals;
    } else {
        if (!dalloc((void**)&d_ip, sizeof(long long) * (G + 1)) || !dalloc((void**)&d_cols, sizeof(int) * nnz) ||
            !dalloc((void**)&d_vals, sizeof(double) * nnz)) {
            cleanup();
            return fail(c, SCC_ERR_OOM, "CSR upload allocation failed");
        }
        hipMemcpyAsync(d_ip, indptr, sizeof(long long) * (G + 1), hipMemcpyHostToDevice, s0);
        if (nnz > 0) {
            hipMemcpyAsync(d_cols, cols, sizeof(int) * nnz, hipMemcpyHostToDevice, s0);
            hipMemcpyAsync(d_vals, vals, sizeof(double) * nnz, hipMemcpyHostToDevice, s0);
        }
    }
    // host-side shape checks on the row pointer (G+1 words)
    std::vector<long long> hip_(G + 1);
    if (hipMemcpyAsync(hip_.data(), d_ip, sizeof(long long) * (G + 1), hipMemcpyDeviceToHost, s0) != hipSuccess ||
        hipStreamSynchronize(s0) != hipSuccess) {
        hipGetLastError();
        cleanup();
        return fail(c, SCC_ERR_HIP, "CSR upload failed");
    }
    if (hip_[0] != 0 || hip_[G] != nnz) {
        cleanup();
        return fail(c, SCC_ERR_INVALID, "CSR indptr must start at 0 and end at nnz");
    }
    for (int64_t g = 0; g < G; ++g)
        if (hip_[g + 1] < hip_[g]) {
            cleanup();
            return fail(c, SCC_ERR_INVALID, "CSR indptr is not non-decreasing");
        }
    // the transpose's plan and scratch (scc_csr.hip: bounds, region and group
    // offsets, the 10-B-per-entry intermediate)
    ScCsrPlan plan;
    if (scc_csr_plan(G, N, nnz, &plan) != 0) {
        cleanup();
        return fail(c, SCC_ERR_UNSUPPORTED, "scc_dataset_create_csr: the transpose has no plan for these dimensions");
    }
    void* scratch = nullptr;
    int* d_err = nullptr;
    if (!dalloc(&scratch, plan.bytes) || !dalloc((void**)&d_err, sizeof(int))) {
        cleanup();
        return fail(c, SCC_ERR_OOM, "CSR transpose scratch allocation failed");
    }
    scc_dataset* d = new scc_dataset();
    d->ctx = c;
    d->device = c->device;
    d->G = G;
    d->N = N;
    d->nnz = nnz;
    d->owned = true;
    if (hipMalloc(&d->d_indptr, sizeof(long long) * (N + 1)) != hipSuccess ||
        hipMalloc(&d->d_rows, sizeof(int) * std::max<int64_t>(nnz, 1)) != hipSuccess ||
        hipMalloc(&d->d_vals, sizeof(double) * std::max<int64_t>(nnz, 1)) != hipSuccess) {
        hipGetLastError();
        cleanup();
        scc_dataset_destroy(d);
        return fail(c, SCC_ERR_OOM, "dataset allocation failed");
    }
    // validation first (columns in range, strictly ascending per gene), then
    // the transpose only over a valid matrix
    int herr = 0;
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(int), s0);
    if (e == hipSuccess) e = scc_launch_csr_check(&plan, d_ip, d_cols, scratch, d_err, s0);
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e == hipSuccess && herr) {
        cleanup();
        scc_dataset_destroy(d);
        return fail(c, SCC_ERR_INVALID, "CSR column index out of range or not strictly ascending within a gene");
    }
    if (e == hipSuccess)
        e = scc_launch_csr_to_csc(&plan, d_ip, d_cols, d_vals, scratch, d->d_indptr, d->d_rows, d->d_vals, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    cleanup();
    if (e != hipSuccess) {
        hipGetLastError();
        scc_dataset_destroy(d);
        return fail(c, SCC_ERR_HIP, std::string("CSR transpose failed: ") + hipGetErrorString(e));
    }
    return finish_create(c, d, out);
}

extern "C" int scc_dataset_create_dense(scc_ctx* c, const double* x, int64_t G, int64_t N, int32_t kind,
                                        scc_dataset** out)
{
    if (!c || !out || !x || G <= 0 || N <= 0) return fail(c, SCC_ERR_INVALID, "scc_dataset_create_dense: bad arguments");
    if (G > INT32_MAX || N > INT32_MAX) return fail(c, SCC_ERR_UNSUPPORTED, "dimensions exceed int32");
    scc_enter(c);
    scc_dataset* d = new scc_dataset();
    d->ctx = c;
    d->device = c->device;
    d->G = G;
    d->N = N;
    d->nnz = G * N;
    d->dense = true;
    if (kind == SCC_PTR_DEVICE) {
        d->d_dense = (double*)x;
    } else {
        d->owned = true;
        if (hipMalloc(&d->d_dense, sizeof(double) * G * N) != hipSuccess) {
            hipGetLastError();
            delete d;
            return fail(c, SCC_ERR_OOM, "dataset allocation failed");
        }
        if (hipMemcpy(d->d_dense, x, sizeof(double) * G * N, hipMemcpyHostToDevice) != hipSuccess) {
            hipGetLastError();
            scc_dataset_destroy(d);
            return fail(c, SCC_ERR_HIP, "dataset upload failed");
        }
    }
    return finish_create(c, d, out);
}

extern "C" int scc_dataset_read_csc(scc_dataset* d, int64_t* indptr, int32_t* rows, double* vals)
{
    if (!d || !indptr || (!rows != !vals))
        return fail(d ? d->ctx : nullptr, SCC_ERR_INVALID, "scc_dataset_read_csc: bad arguments");
    if (d->dense || !d->d_indptr) return fail(d->ctx, SCC_ERR_INVALID, "scc_dataset_read_csc: not a sparse dataset");
    scc_enter(d->ctx);
    hipStream_t s0 = d->ctx->s0;
    hipError_t e = hipMemcpyAsync(indptr, d->d_indptr, sizeof(int64_t) * (d->N + 1), hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess && d->nnz > 0 && rows)
        e = hipMemcpyAsync(rows, d->d_rows, sizeof(int32_t) * d->nnz, hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess && d->nnz > 0 && vals)
        e = hipMemcpyAsync(vals, d->d_vals, sizeof(double) * d->nnz, hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e != hipSuccess) {
        hipGetLastError();
        return fail(d->ctx, SCC_ERR_HIP, std::string("scc_dataset_read_csc: ") + hipGetErrorString(e));
    }
    return SCC_OK;
}

void scc_rt::mirror_free(const scc_dataset* d)
{
    hipFree(d->m_gptr);
    hipFree(d->m_cell);
    hipFree(d->m_key);
    hipFree(d->m_order);
    hipFree(d->m_seg);
    vorder_free(d);
    d->m_gptr = nullptr;
    d->m_cell = nullptr;
    d->m_key = nullptr;
    d->m_order = nullptr;
    d->m_seg = nullptr;
}

// the mirror's value order (freed wherever the mirror is)
void scc_rt::vorder_free(const scc_dataset* d)
{
    hipFree(d->m_vcell);
    hipFree(d->m_vbk_ptr);
    hipFree(d->m_vbk);
    d->m_vcell = nullptr;
    d->m_vbk_ptr = nullptr;
    d->m_vbk = nullptr;
    d->m_vnbk = 0;
}

// which rank route the calling thread's last DE run took: 0 no run yet, 1 the
// per-call value buckets (split, re-split, in-wave sort, LDS items; also every
// run that ranks nothing or ranks elsewhere: SLOW, the t and bimod tests, gene
// shards, the one-vs-rest run), 2 the walk of the dataset's value order
thread_local int scc_rt::g_rank_last_route = 0;
extern "C" SCC_API int scc_diag_rank_last_route(void) { return g_rank_last_route; }
// 1: that run (route 2) formed the cross-bucket term per run, from one histogram
// row per (gene, chunk); 0: a row per bucket and k_rank_cross, or no such run
thread_local int scc_rt::g_rank_last_runs = 0;
extern "C" SCC_API int scc_diag_rank_last_runs(void) { return g_rank_last_runs; }

// which ingest the calling thread's last DE run took: 0 none yet, 1 the full
// read (the validating call, SLOW, dense, SCC_INGEST_FULL), 2 the lean
// transpose of a validated dataset, 3 the regroup of the dataset's mirror
thread_local int scc_rt::g_ingest_last_path = 0;
extern "C" SCC_API int scc_diag_ingest_last_path(void) { return g_ingest_last_path; }

// what the calling thread's last calls read from the mirror: bit 1 the last PCA
// gather (scc_distance, scc_pca_scores) filled its panel from the mirror; bit 0
// (statistics in the regroup's workgroups) has no route and stays 0
thread_local int scc_rt::g_mirror_last_uses = 0;
extern "C" SCC_API int scc_diag_mirror_last_uses(void) { return g_mirror_last_uses; }

extern "C" void scc_dataset_destroy(scc_dataset* d)
{
    if (!d) return;
    for (scc_dataset* r : d->reps) scc_dataset_destroy(r);
    d->reps.clear();
    if (d->owned || d->d_nodg || d->d_tbnd || d->m_gptr) {
        hipSetDevice(d->device);
        hipDeviceSynchronize();
    }
    mirror_free(d);
    if (d->owned) {
        hipFree(d->d_indptr);
        hipFree(d->d_rows);
        hipFree(d->d_vals);
        hipFree(d->d_dense);
    }
    hipFree(d->d_nodg);
    hipFree(d->d_tbnd);
    delete d;
}

// the DE driver lives in scc_de.cpp, the distance entry points in scc_distance.cpp
