// scc_heatmap.cpp — C ABI of the heatmap's device inputs (include/scc.h:
// scc_gene_distance, scc_heatmap_raster; kernels: scc_heatmap.hip; the two
// host functions scc_hclust_complete / scc_dendro_reorder: scc_cluster.cpp).
//
// Both calls gather X[U, ] of all cells into a panel of their own ("hm_X"; the
// PCA's "d_X", the kept scores "d_P" and the kept distance "d_dist" are not
// touched), run on devices[0] of the context, and return after one
// synchronisation with every host output written.
#include "scc_internal.hpp"

#include <new>

using namespace scc_rt;

extern "C" {
hipError_t scc_launch_gather(const long long* indptr, const int* rows, const double* vals, const double* dense,
                             int G, int N, int Npad, int* umap, const int* genes, int nu, int ld, double* Xc,
                             hipStream_t st);
hipError_t scc_launch_center(double* Xc, int N, int nu, int ld, dd* part, int nchunk, double* mean, int apply,
                             hipStream_t st);
}

namespace {

constexpr int kMeanChunks = 512;  // as the PCA's centring (scc_distance.cpp)

// bytes the context already holds under a workspace name
size_t ws_held(const scc_ctx* c, const char* name)
{
    auto it = c->ws.find(name);
    return it == c->ws.end() ? 0 : it->second.second;
}

// The rule of scc_hclust_ward_d2_dev for the call's large buffers: what has to
// be allocated on top of what the context holds must fit in half of the free
// device memory.
int fits(scc_ctx* c, const char* who, const char* const* names, const size_t* bytes, int n)
{
    size_t extra = 0, total = 0;
    for (int i = 0; i < n; ++i) {
        total += bytes[i];
        if (ws_held(c, names[i]) < bytes[i]) extra += bytes[i] + bytes[i] / 8;  // ws_get's growth margin
    }
    if (!extra) return SCC_OK;
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    if (extra > free_b / 2)
        return fail(c, SCC_ERR_OOM, std::string(who) + ": the panel and its scratch (" + std::to_string(total >> 20) +
                                        " MiB) exceed half of the " + std::to_string(free_b >> 20) +
                                        " MiB of free device memory");
    return SCC_OK;
}

// nu genes in [0, G), none listed twice
int check_genes(scc_ctx* c, const char* who, const int32_t* genes, int nu, int G)
{
    std::vector<uint8_t> seen((size_t)G, 0);
    for (int u = 0; u < nu; ++u) {
        if (genes[u] < 0 || genes[u] >= G) return fail(c, SCC_ERR_INVALID, std::string(who) + ": gene index out of range");
        if (seen[(size_t)genes[u]]) return fail(c, SCC_ERR_INVALID, std::string(who) + ": a gene is listed twice");
        seen[(size_t)genes[u]] = 1;
    }
    return SCC_OK;
}

// X[U, ] of every cell into the heatmap's own panel
int gather_panel(scc_ctx* c, const scc_dataset* ds, const int32_t* genes, int nu, int ld, int Npad, double** X)
{
    const int G = (int)ds->G, N = (int)ds->N;
    int rc;
    int *d_genes, *d_umap;
    if ((rc = ws(c, "hm_genes", (size_t)nu, &d_genes))) return rc;
    if ((rc = ws(c, "hm_umap", (size_t)G, &d_umap))) return rc;
    if ((rc = ws(c, "hm_X", (size_t)Npad * ld, X))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_genes, genes, sizeof(int) * (size_t)nu, hipMemcpyHostToDevice, c->s0));
    Scope sc(c, "heatmap_gather", c->s0);
    HIPCHK(c, scc_launch_gather(ds->d_indptr, ds->d_rows, ds->d_vals, ds->d_dense, G, N, Npad, d_umap, d_genes, nu, ld,
                                *X, c->s0));
    return SCC_OK;
}

}  // namespace

extern "C" int scc_gene_distance(scc_ctx* c, const scc_dataset* ds, const int32_t* genes, int32_t nu, double* dist,
                                 double* row_mean, double* range)
{
    if (!c || !ds || !genes) return fail(c, SCC_ERR_INVALID, "scc_gene_distance: null argument");
    if (ds->ctx != c) return fail(c, SCC_ERR_INVALID, "scc_gene_distance: the dataset belongs to another context");
    if (nu < 2) return fail(c, SCC_ERR_INVALID, "scc_gene_distance: need at least two genes");
    const int G = (int)ds->G, N = (int)ds->N;
    if (N < 1) return fail(c, SCC_ERR_INVALID, "scc_gene_distance: no cells");
    int rc;
    try {
        if ((rc = check_genes(c, "scc_gene_distance", genes, nu, G))) return rc;
    } catch (const std::bad_alloc&) {
        return fail(c, SCC_ERR_OOM, "scc_gene_distance: host allocation failed");
    }
    scc_enter(c);
    hipStream_t s0 = c->s0;
    const int ld = (nu + 63) & ~63;
    const int Npad = (N + 15) & ~15;
    const size_t npairs = (size_t)nu * (size_t)(nu - 1) / 2;
    const size_t slab_n = scc_gene_dist_slab_doubles(Npad, ld);
    {
        const char* const names[3] = {"hm_X", "hm_slabs", "hm_dist"};
        const size_t bytes[3] = {sizeof(double) * (size_t)Npad * ld, sizeof(double) * slab_n, sizeof(double) * npairs};
        if ((rc = fits(c, "scc_gene_distance", names, bytes, 3))) return rc;
    }
    double *d_X, *d_slabs, *d_dist, *d_mean, *d_range;
    void *d_part, *d_rscr;
    unsigned int* d_bad;
    if ((rc = gather_panel(c, ds, genes, nu, ld, Npad, &d_X))) return rc;
    if ((rc = ws(c, "hm_slabs", slab_n, &d_slabs))) return rc;
    if ((rc = ws(c, "hm_dist", npairs, &d_dist))) return rc;
    if ((rc = ws(c, "hm_mean", (size_t)ld, &d_mean))) return rc;
    if ((rc = ws(c, "hm_range", (size_t)4, &d_range))) return rc;
    if ((rc = ws(c, "hm_bad", (size_t)1, &d_bad))) return rc;
    if ((rc = ws_get(c, "hm_part", sizeof(double) * 2 * (size_t)kMeanChunks * ld, &d_part))) return rc;
    if ((rc = ws_get(c, "hm_rscr", scc_hm_range_scratch_bytes(), &d_rscr))) return rc;
    {
        // rowMeans: the PCA's double-double column sums of the panel (the means only, nothing is centred)
        Scope sc(c, "heatmap_mean", s0);
        HIPCHK(c, scc_launch_center(d_X, N, nu, ld, (dd*)d_part, kMeanChunks, d_mean, 0, s0));
    }
    {
        Scope sc(c, "heatmap_range", s0);
        HIPCHK(c, scc_launch_hm_range(d_X, N, nu, ld, d_rscr, d_range, d_bad, s0));
    }
    {
        Scope sc(c, "gene_dist", s0);
        HIPCHK(c, scc_launch_gene_dist(d_X, Npad, nu, ld, d_slabs, d_dist, s0));
    }
    // the count decides whether anything is an answer: nothing is copied out before it is read
    unsigned int bad = 0;
    double h_range[4];
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipMemcpyAsync(h_range, d_range, sizeof(h_range), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (bad)
        return fail(c, SCC_ERR_NONFINITE, "scc_gene_distance: " + std::to_string(bad) +
                                              " non-finite value(s) in the union's rows");
    if (dist) HIPCHK(c, hipMemcpyAsync(dist, d_dist, sizeof(double) * npairs, hipMemcpyDeviceToHost, s0));
    if (row_mean) HIPCHK(c, hipMemcpyAsync(row_mean, d_mean, sizeof(double) * (size_t)nu, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (range) std::copy(h_range, h_range + 4, range);
    return SCC_OK;
}

extern "C" int scc_heatmap_raster(scc_ctx* c, const scc_dataset* ds, const int32_t* genes, int32_t nu,
                                  const int32_t* row_order, const int32_t* cell_order, int32_t width, double* out)
{
    if (!c || !ds || !genes || !row_order || !cell_order)
        return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: null argument");
    if (ds->ctx != c) return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: the dataset belongs to another context");
    if (nu < 1) return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: empty gene list");
    const int G = (int)ds->G, N = (int)ds->N;
    if (width < 1 || width > N) return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: width must be in [1, N]");
    int rc;
    std::vector<int> cell0;
    std::vector<double> R;
    try {
        if ((rc = check_genes(c, "scc_heatmap_raster", genes, nu, G))) return rc;
        std::vector<uint8_t> seen((size_t)std::max(N, (int)nu), 0);
        for (int r = 0; r < nu; ++r) {
            if (row_order[r] < 1 || row_order[r] > nu || seen[(size_t)row_order[r] - 1])
                return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: row_order is not a permutation of 1..nu");
            seen[(size_t)row_order[r] - 1] = 1;
        }
        std::fill(seen.begin(), seen.end(), 0);
        cell0.resize((size_t)N);
        for (int i = 0; i < N; ++i) {
            if (cell_order[i] < 1 || cell_order[i] > N || seen[(size_t)cell_order[i] - 1])
                return fail(c, SCC_ERR_INVALID, "scc_heatmap_raster: cell_order is not a permutation of 1..N");
            seen[(size_t)cell_order[i] - 1] = 1;
            cell0[(size_t)i] = cell_order[i] - 1;
        }
        if (out) R.resize((size_t)width * (size_t)nu);
    } catch (const std::bad_alloc&) {
        return fail(c, SCC_ERR_OOM, "scc_heatmap_raster: host allocation failed");
    }
    scc_enter(c);
    hipStream_t s0 = c->s0;
    const int ld = (nu + 63) & ~63;
    const int Npad = (N + 15) & ~15;
    {
        const char* const names[2] = {"hm_X", "hm_rast"};
        const size_t bytes[2] = {sizeof(double) * (size_t)Npad * ld, sizeof(double) * (size_t)width * nu};
        if ((rc = fits(c, "scc_heatmap_raster", names, bytes, 2))) return rc;
    }
    double *d_X, *d_R;
    int* d_cell;
    if ((rc = gather_panel(c, ds, genes, nu, ld, Npad, &d_X))) return rc;
    if ((rc = ws(c, "hm_rast", (size_t)width * nu, &d_R))) return rc;
    if ((rc = ws(c, "hm_cell", (size_t)N, &d_cell))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_cell, cell0.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, s0));
    {
        Scope sc(c, "heatmap_raster", s0);
        HIPCHK(c, scc_launch_heatmap_raster(d_X, N, nu, ld, d_cell, width, d_R, s0));
    }
    if (out) HIPCHK(c, hipMemcpyAsync(R.data(), d_R, sizeof(double) * R.size(), hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (out)  // the device raster is [width][nu] in the genes' order: transposed and permuted here
        for (int r = 0; r < nu; ++r) {
            const size_t g = (size_t)row_order[r] - 1;
            double* o = out + (size_t)r * width;
            for (int b = 0; b < width; ++b) o[b] = R[(size_t)b * nu + g];
        }
    return SCC_OK;
}
