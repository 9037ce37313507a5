// scc_cluster.hpp — the parts of scc_cluster.cpp that the host entry points
// (scc_hclust_ward_d2, scc_cutree_hybrid) share with the device-resident ones
// (scc_distance.cpp: scc_hclust_ward_d2_dev, scc_cutree_hybrid_dev).
#pragma once
#include <cstdint>
#include <functional>
#include <string>

namespace scc_cl {

// hclust's post-processing of the NN-chain's n - 1 steps (a, b: the merged
// nodes as the chain reported them; h2: the SQUARED merge distances): sqrt of
// the heights, stable sort by height, union-find relabelling to R's merge
// convention and the left-to-right leaf order (order may be null).
void hclust_finish(int64_t n, const int32_t* a, const int32_t* b, const double* h2, int32_t* merge, double* height,
                   int32_t* order);

// distM[core, core] for the tree cut's core scatter: block[j * cs + i] =
// d(core[i], core[j]) (core: 1-based object ids; 0 on the diagonal).  Returns
// SCC_OK or an error code (the cut stops and returns it).
using CoreFetch = std::function<int(const int32_t* core, int cs, double* block)>;

// cutreeDynamic(method = "hybrid", pamStage = FALSE) with the distance read
// through `fetch` only
int cutree_hybrid(const int32_t* merge, const double* height, int64_t n, const CoreFetch& fetch, int deep_split,
                  int min_cluster_size, int32_t* labels, double* cut_out, std::string& err);

}  // namespace scc_cl
