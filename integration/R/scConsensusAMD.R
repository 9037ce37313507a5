# scConsensusAMD.R — drop-in R wrappers that route the data-parallel core of
# scConsensus to the MI355X engine (libscc via .Call; see INTEGRATION.md).
#
# Signatures and return objects are those of the reference:
#   reclusterDEConsensusFast  R/reclusterDEConsensusFast.R:22-33, returns :446-450
#   reclusterDEConsensus      R/reclusterDEConsensus.R:20-29,      returns :278-282
# Kept in R (host), exactly as the reference does them: cluster selection
# (table / grepl("grey") / locale order), hclust(ward.D2), cutreeDynamic,
# labels2colors, silhouette, saveRDS, printing and cellTypeDEPlot (opt-in:
# its gene-row tree from the engine, options(scConsensus.engineHeatmapRows)).

# Cluster selection exactly as Fast:39-47 / slow:38-48: table() over ALL of
# consensusClusterLabels (locale collation), "> minClusterSize", no "grey";
# then each matrix column's code (0-based index into the kept clusters, -1
# for cells of other clusters or without a label).
.scc_codes <- function(consensusClusterLabels, dataMatrix, minClusterSize) {
  colorCounts <- table(consensusClusterLabels)
  keep <- names(colorCounts[colorCounts > minClusterSize])
  keep <- keep[!grepl("grey", keep)]
  if (is.null(names(consensusClusterLabels))) names(consensusClusterLabels) <- colnames(dataMatrix)
  colLabels <- consensusClusterLabels[colnames(dataMatrix)]
  code <- match(as.character(colLabels), keep) - 1L
  code[is.na(code)] <- -1L
  list(clusters = keep, code = as.integer(code))
}

.scc_slots <- function(m) {
  if (inherits(m, "dgCMatrix")) {
    list(x = m@x, p = m@p, i = m@i, dim = dim(m))
  } else if (inherits(m, "dgRMatrix")) {
    # gene-major CSR: a third dim entry 1L selects scc_dataset_create_csr
    list(x = m@x, p = m@p, i = m@j, dim = c(dim(m), 1L))
  } else {
    m <- as.matrix(m)
    storage.mode(m) <- "double"
    list(x = m, p = NULL, i = NULL, dim = dim(m))
  }
}

# the matrix uploaded ONCE per call of the R function; DE and distance share
# the device copy through this handle (freed by C_scc_release or the GC)
.scc_dataset <- function(m) {
  s <- .scc_slots(m)
  .Call("C_scc_dataset", s$x, s$p, s$i, s$dim)
}

.scc_dist <- function(h, genes, n_cells, metric = 0L) {
  d <- .Call("C_scc_distance", h, as.integer(genes), as.integer(metric), 0L)
  structure(d, Size = n_cells, Diag = FALSE, Upper = FALSE,
            method = if (metric == 0L) "euclidean" else "pearson", class = "dist")
}

# hclust(ward.D2) as Fast:406-411; with options(scConsensus.engineTree = TRUE)
# the engine's C++ restatement (no fastcluster needed; same merge rule)
.scc_hclust <- function(d) {
  if (isTRUE(getOption("scConsensus.engineTree", FALSE))) {
    t <- .Call("C_scc_hclust", d)
    return(structure(list(merge = t[[1]], height = t[[2]], order = t[[3]], labels = attr(d, "Labels"),
                          method = "ward.D2", call = match.call(), dist.method = attr(d, "method")),
                     class = "hclust"))
  }
  if (requireNamespace("fastcluster", quietly = TRUE)) fastcluster::hclust(d, method = "ward.D2")
  else stats::hclust(d, method = "ward.D2")
}

.scc_tree_and_colors <- function(d, deepSplitValues, minClusterSize, with_si) {
  tree <- .scc_hclust(d)
  # cutreeDynamic needs distM = as.matrix(d): N^2 doubles on the host (5.4 GB
  # at 26k cells, 80 GB at 100k, 320 GB at 200k).  options(scConsensus.engineCut
  # = TRUE) runs the engine's restatement of the hybrid cut on the packed d
  # instead (parity against dynamicTreeCut itself unpinned: INTEGRATION.md)
  engine_cut <- isTRUE(getOption("scConsensus.engineCut", FALSE))
  dm <- if (engine_cut) NULL else as.matrix(d)
  colors <- list()
  for (dsv in deepSplitValues) {
    grp <- if (engine_cut) {
      .Call("C_scc_cutree", tree$merge, as.double(tree$height), d, as.integer(dsv), as.integer(minClusterSize))
    } else {
      dynamicTreeCut::cutreeDynamic(dendro = tree, distM = dm, deepSplit = dsv,
                                    pamStage = FALSE, minClusterSize = minClusterSize)
    }
    colors[[paste("deepsplit:", dsv)]] <- WGCNA::labels2colors(grp)
    # deepSplitInfo's SI (Fast:433, computed and discarded by the reference):
    # the engine's silhouette on its HBM-resident copy of d (no N x N matrix)
    if (with_si) invisible(.Call("C_scc_si", as.integer(grp)))
  }
  names(colors) <- paste("deepsplit:", deepSplitValues)
  list(tree = tree, colors = colors)
}

# options(scConsensus.engineTree = "device"): the distance stays in the engine's
# HBM, hclust(ward.D2) (Fast:406-411, slow:242-247) and the hybrid cuts
# (Fast:421-427, slow:257-263) run on it there; no "dist" object and no
# as.matrix(d) on the host.  Same tree and labels as engineTree = TRUE with
# engineCut = TRUE (the engine's restatements; parity against fastcluster /
# dynamicTreeCut themselves unpinned: INTEGRATION.md)
.scc_tree_on_device <- function() identical(getOption("scConsensus.engineTree", FALSE), "device")

.scc_tree_and_colors_dev <- function(h, genes, n_cells, deepSplitValues, minClusterSize, with_si, metric = 0L) {
  .Call("C_scc_distance_dev", h, as.integer(genes), as.integer(metric), 0L)
  t <- .Call("C_scc_hclust_dev", as.integer(n_cells))
  tree <- structure(list(merge = t[[1]], height = t[[2]], order = t[[3]], labels = NULL,
                         method = "ward.D2", call = match.call(),
                         dist.method = if (metric == 0L) "euclidean" else "pearson"),
                    class = "hclust")
  colors <- list()
  for (dsv in deepSplitValues) {
    grp <- .Call("C_scc_cutree_dev", tree$merge, as.double(tree$height), as.integer(dsv), as.integer(minClusterSize))
    colors[[paste("deepsplit:", dsv)]] <- WGCNA::labels2colors(grp)
    if (with_si) invisible(.Call("C_scc_si", as.integer(grp)))
  }
  names(colors) <- paste("deepsplit:", deepSplitValues)
  list(tree = tree, colors = colors)
}

# options(scConsensus.engineTree = "scores"): no distance at all.  The engine
# stops after the PCA (Fast:398-399, slow:234-235) and keeps the N x 15 scores;
# hclust(ward.D2) runs on centroids of the scores and the hybrid cuts compute
# their distM entries from them (128 bytes per cell instead of 8 N^2: the only
# route at cell counts whose matrix fits nowhere).  The same tree as the other
# engine routes whenever no two candidate dissimilarities lie within rounding
# of each other; on exact ties (duplicate cells) a valid Ward tree that may
# resolve the tie differently.  deepSplitInfo's SI (Fast:433, computed and
# discarded by the reference) is computed only with
# options(scConsensus.engineScoresSI = TRUE): the engine's silhouette from the
# scores (C_scc_si_scores: dist(scores) entry by entry, no N x N matrix; the SI
# of the other routes, bit for bit, for equal groups).  Without the option the
# route makes no silhouette call; Fast:433's stop for fewer than 2 groups is
# kept either way.
.scc_tree_from_scores <- function() identical(getOption("scConsensus.engineTree", FALSE), "scores")

.scc_tree_and_colors_scores <- function(h, genes, n_cells, deepSplitValues, minClusterSize, with_si) {
  .Call("C_scc_pca_scores", h, as.integer(genes), 0L)
  t <- .Call("C_scc_hclust_scores", as.integer(n_cells))
  tree <- structure(list(merge = t[[1]], height = t[[2]], order = t[[3]], labels = NULL,
                         method = "ward.D2", call = match.call(), dist.method = "euclidean"),
                    class = "hclust")
  colors <- list()
  for (dsv in deepSplitValues) {
    grp <- .Call("C_scc_cutree_scores", tree$merge, as.double(tree$height), as.integer(dsv), as.integer(minClusterSize))
    colors[[paste("deepsplit:", dsv)]] <- WGCNA::labels2colors(grp)
    # silhouette() of fewer than 2 (or of n) groups is NA and Fast:433 stops on it
    k <- length(unique(grp))
    if (with_si && (k < 2L || k >= n_cells)) stop("$ operator is invalid for atomic vectors")
    if (with_si && isTRUE(getOption("scConsensus.engineScoresSI", FALSE)))
      invisible(.Call("C_scc_si_scores", as.integer(grp)))
  }
  names(colors) <- paste("deepsplit:", deepSplitValues)
  list(tree = tree, colors = colors)
}

# ---- the heatmap's gene rows on the engine (opt-in) --------------------------
# cellTypeDEPlot ends in ComplexHeatmap::Heatmap(cluster_rows = TRUE), which
# runs dist() over the |U| gene rows (|U|^2 N / 2 subtract-multiply-adds on one
# R thread), hclust("complete") and a reorder by -rowMeans.  sccHeatmapRows
# computes the same row tree through the engine (C_scc_heatmap_rows: the
# distance on the device, the tree and the reorder in libscc's host code) and
# returns it as an "hclust" object, already reordered, with the colour ramp's
# inputs attached:
#   attr(, "range")    c(min x, max x, min |x|, max |x|) over dataMatrix[deGeneUnion, ]
#   attr(, "rowMeans") rowMeans(dataMatrix[deGeneUnion, ])
# dataset: the matrix (dgCMatrix, dgRMatrix or base matrix) or a handle of
# .scc_dataset; deGeneUnion: row names or 1-based row indices.  On exact ties
# the tree is a valid complete-linkage tree that stats::hclust may resolve
# otherwise.  $merge is the reordered matrix (children in drawing order), so it
# does not list singletons first; as.dendrogram does not need that.
sccHeatmapRows <- function(dataset, deGeneUnion) {
  own <- !inherits(dataset, "externalptr")
  if (own && is.character(deGeneUnion)) {
    rows <- match(deGeneUnion, rownames(dataset))
    labels <- deGeneUnion
  } else {
    rows <- as.integer(deGeneUnion)
    labels <- if (own && !is.null(rownames(dataset))) rownames(dataset)[rows] else NULL
  }
  if (anyNA(rows)) stop("sccHeatmapRows: a gene of deGeneUnion is not a row of the matrix")
  h <- if (own) .scc_dataset(dataset) else dataset
  if (own) on.exit(.Call("C_scc_release", h), add = TRUE)
  t <- .Call("C_scc_heatmap_rows", h, as.integer(rows))
  tree <- structure(list(merge = t[[1]], height = t[[2]], order = t[[3]], labels = labels,
                         method = "complete", call = match.call(), dist.method = "euclidean"),
                    class = "hclust")
  attr(tree, "range") <- t[[4]]
  attr(tree, "rowMeans") <- t[[5]]
  tree
}

# ---- the neighbour graph of the cells on the engine --------------------------
# The reference README's example ends with prcomp_irlba(n = 15) on the marker
# union, pca.data <- pca.obj$x[, 1:8] and umap::umap(d = pca.data), whose first
# step is a k-nearest-neighbour search over the cells.  sccKnn runs the PCA and
# that search on the engine (C_scc_knn: exact, no N x N matrix) and returns
# list(indexes, distances), two N x k matrices, indexes 1-based, each row in
# (distance, index) order: the shape umap::umap.knn(indexes, distances) takes
# for umap(d, knn = ), and uwot's nn_method = list(idx = , dist = ).
#   genes         row names or 1-based row indices (the marker union)
#   n             components the PCA keeps (at most 15)
#   dims          leading components the distance uses (the README's 8)
#   include_self  TRUE: column 1 is the cell itself at distance 0, followed by
#                 its k - 1 nearest other cells; FALSE: the k nearest others.
#                 Whether a package expects the cell itself first was not
#                 checked against umap or uwot (neither was at hand), which is
#                 why it is a parameter: compare with the package's own
#                 knn output before relying on the default.
sccKnn <- function(dataMatrix, genes, k = 15, n = 15, dims = 8, include_self = TRUE) {
  rows <- if (is.character(genes)) match(genes, rownames(dataMatrix)) else as.integer(genes)
  if (anyNA(rows)) stop("sccKnn: a gene is not a row of the matrix")
  others <- as.integer(k) - if (include_self) 1L else 0L
  if (others < 1L) stop("sccKnn: k leaves no neighbour besides the cell itself")
  if (dims < 1L || dims > n) stop("sccKnn: dims must lie in 1..n")
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  t <- .Call("C_scc_knn", h, as.integer(rows), as.integer(n), as.integer(dims), others)
  indexes <- t[[1]]
  distances <- t[[2]]
  if (include_self) {
    indexes <- cbind(seq_len(nrow(indexes)), indexes)
    distances <- cbind(0, distances)
  }
  rownames(indexes) <- rownames(distances) <- colnames(dataMatrix)
  list(indexes = indexes, distances = distances)
}

# ---- UMAP of the cells on the engine -----------------------------------------
# The README's last step, umap::umap(d = pca.data), in one engine call
# (C_scc_umap: the PCA, the exact neighbour search, the fuzzy simplicial set and
# the stochastic-gradient layout; the table and the graph stay on the device).
# Returns the N x 2 layout, rows named by cell: what umap::umap(...)$layout holds.
# The rules are umap-learn's; the result is deterministic for a seed, and it has
# not been compared with the umap or uwot packages (neither was at hand).
#   n_neighbors   counts the cell itself, as umap.defaults$n_neighbors does (2..65)
#   a, b          the curve constants; NULL: the pair fitted for min_dist = 0.1,
#                 spread = 1 (another min_dist or spread: fit a and b with
#                 umap-learn's find_ab_params recipe, e.g. by nls(), and pass them)
#   init          an N x 2 matrix, or NULL for the first two components scaled to
#                 a largest absolute coordinate of 10 (no spectral initialisation)
sccUmap <- function(dataMatrix, genes, n_neighbors = 15, n = 15, dims = 8, n_epochs = 200, a = NULL, b = NULL,
                    gamma = 1, negative_sample_rate = 5, learning_rate = 1, set_op_mix_ratio = 1, seed = 0,
                    init = NULL) {
  rows <- if (is.character(genes)) match(genes, rownames(dataMatrix)) else as.integer(genes)
  if (anyNA(rows)) stop("sccUmap: a gene is not a row of the matrix")
  if (n_neighbors < 2L) stop("sccUmap: n_neighbors leaves no neighbour besides the cell itself")
  if (dims < 1L || dims > n) stop("sccUmap: dims must lie in 1..n")
  if (is.null(a) != is.null(b)) stop("sccUmap: give both a and b, or neither")
  if (!is.null(init) && !identical(dim(init), c(ncol(dataMatrix), 2L))) stop("sccUmap: init must be N x 2")
  par <- c(n_epochs, if (is.null(a)) 0 else a, if (is.null(b)) 0 else b, gamma, negative_sample_rate,
           learning_rate, set_op_mix_ratio, seed, 0)
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  layout <- .Call("C_scc_umap", h, as.integer(rows), as.integer(n), as.integer(dims), as.integer(n_neighbors),
                  as.numeric(par), if (is.null(init)) NULL else matrix(as.numeric(init), ncol = 2))
  rownames(layout) <- colnames(dataMatrix)
  layout
}

# ---- SNN graph and modularity clustering on the engine -------------------------
# The step in front of the README's example: its seuratObj$RNA_snn_res.0.2 is what
# Seurat's FindNeighbors + FindClusters make of the PCA scores.  One engine call
# (C_scc_find_clusters: the PCA, the exact neighbour search, the SNN graph by
# Seurat's ComputeSNN rule and a deterministic multilevel modularity clustering;
# the table and the graph stay on the device).  Returns a factor of cluster labels
# named by cell, "0" the largest cluster as in Seurat, ready for
# plotContingencyTable and reclusterDEConsensusFast; attributes "modularity" and
# "sweeps".  The rules are restated in tests/snn_reference.py; the result has not
# been compared with Seurat (it was not at hand), and there is no Leiden or SLM
# refinement, no grouping of singletons and no random vertex order.
#   k.param     counts the cell itself, as FindNeighbors' k.param does (2..65)
#   prune.SNN   pairs whose shared-neighbour weight is below it are dropped
sccFindClusters <- function(dataMatrix, genes, k.param = 20, n = 15, dims = n, prune.SNN = 1 / 15, resolution = 0.8) {
  rows <- if (is.character(genes)) match(genes, rownames(dataMatrix)) else as.integer(genes)
  if (anyNA(rows)) stop("sccFindClusters: a gene is not a row of the matrix")
  if (k.param < 2L) stop("sccFindClusters: k.param leaves no neighbour besides the cell itself")
  if (dims < 1L || dims > n) stop("sccFindClusters: dims must lie in 1..n")
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  res <- .Call("C_scc_find_clusters", h, as.integer(rows), as.integer(n), as.integer(dims), as.integer(k.param),
               as.numeric(c(prune.SNN, resolution)))
  labels <- factor(res[[1]], levels = seq_len(max(res[[1]]) + 1L) - 1L)
  names(labels) <- colnames(dataMatrix)
  attr(labels, "modularity") <- res[[2]]
  attr(labels, "sweeps") <- res[[3]]
  labels
}

# The drawing for options(scConsensus.engineHeatmapRows = TRUE): the wrapper's
# own plotting helper, written from ComplexHeatmap's documented arguments.  Rows
# follow the engine's tree (cluster_rows = a dendrogram, row_dend_reorder =
# FALSE: it is reordered already), columns follow cellTree as given, the ramp
# runs over [min |x|, max |x|] from the engine's range, and the cells carry
# their consensus label, one colour strip per deepSplit and a bar of nodg.
.scc_heatmap_plot <- function(mat, rowTree, nodg, cellTree, clusterLabels, dynamicColorsList, filename) {
  rng <- attr(rowTree, "range")
  stops <- seq(rng[3], rng[4], length.out = 5)
  ramp <- circlize::colorRamp2(stops, grDevices::colorRampPalette(c("slateblue1", "white", "red", "darkred"))(5))
  strips <- as.data.frame(dynamicColorsList, check.names = FALSE, stringsAsFactors = FALSE)
  stripCols <- lapply(strips, function(v) stats::setNames(unique(v), unique(v)))
  strips[["consensus"]] <- as.character(clusterLabels[colnames(mat)])
  top <- ComplexHeatmap::HeatmapAnnotation(
    df = strips, col = stripCols,
    NODG = ComplexHeatmap::anno_barplot(nodg),
    which = "column", annotation_name_side = "left")
  ht <- ComplexHeatmap::Heatmap(
    matrix = as.matrix(mat), col = ramp, name = "expression",
    cluster_rows = stats::as.dendrogram(rowTree), row_dend_reorder = FALSE,
    cluster_columns = stats::as.dendrogram(cellTree), column_dend_reorder = FALSE,
    top_annotation = top, show_column_names = FALSE,
    row_names_gp = grid::gpar(fontsize = 5), use_raster = TRUE)
  grDevices::pdf(paste0(filename, ".pdf"), width = 50, height = 50)
  on.exit(grDevices::dev.off(), add = TRUE)
  ComplexHeatmap::draw(ht)
  invisible(ht)
}

# the last step of both functions: the reference's cellTypeDEPlot (default), or
# with options(scConsensus.engineHeatmapRows = TRUE) the helper above on the
# engine's row tree
.scc_plot <- function(h, mat, genes, nodg, cellTree, clusterLabels, dynamicColorsList, plotName) {
  if (isTRUE(getOption("scConsensus.engineHeatmapRows", FALSE)) && length(genes) >= 2L) {
    rowTree <- sccHeatmapRows(h, genes)
    rowTree$labels <- rownames(mat)
    .scc_heatmap_plot(mat, rowTree, nodg, cellTree, clusterLabels, dynamicColorsList, plotName)
  } else {
    cellTypeDEPlot(dataMatrix = mat, nodg = nodg, cellTree = cellTree,
                   clusterLabels = clusterLabels, dynamicColorsList = dynamicColorsList,
                   colScheme = "violet", filename = plotName)
  }
}

reclusterDEConsensusFast <- function(dataMatrix, consensusClusterLabels, method = "wilcox",
                                     qValThrs = 0.1, logFCThrs = 0.5, deepSplitValues = 1:4,
                                     minClusterSize = 10, minPerCent = 20,
                                     filename = "de_gene_object.rds", plotName = "DE_Heatmap",
                                     NumbertopDEGenes = 30, nCores = 1) {
  # test.use = method (Fast:372): "wilcox", "t" and "bimod" run on the engine
  # (SCC_TEST_* codes 0, 1, 2); "roc" yields no p_val_adj, which Fast:377 filters on
  tests <- c("wilcox", "t", "bimod")
  if (!(method %in% tests)) stop("Unknown test: ", method)
  sel <- .scc_codes(consensusClusterLabels, dataMatrix, minClusterSize)
  # nCores PSOCK workers (Fast:61-65) -> min(nCores, GPUs) devices of ONE sharded job
  .Call("C_scc_devices", as.integer(nCores))
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  res <- .Call("C_scc_de_fast", h, sel$code, length(sel$clusters),
               as.double(qValThrs), as.double(logFCThrs), as.double(minPerCent),
               as.integer(NumbertopDEGenes), match(method, tests) - 1L)
  deGeneUnion <- rownames(dataMatrix)[res[[1]]]
  print(str(deGeneUnion))
  tc <- if (.scc_tree_from_scores()) {
    .scc_tree_and_colors_scores(h, res[[1]], ncol(dataMatrix), deepSplitValues, minClusterSize, with_si = TRUE)
  } else if (.scc_tree_on_device()) {
    .scc_tree_and_colors_dev(h, res[[1]], ncol(dataMatrix), deepSplitValues, minClusterSize, with_si = TRUE)
  } else {
    d <- .scc_dist(h, res[[1]], ncol(dataMatrix))
    .scc_tree_and_colors(d, deepSplitValues, minClusterSize, with_si = TRUE)
  }
  out <- list("deGeneUnion" = deGeneUnion, "cellTree" = tc$tree, "dynamicColors" = tc$colors)
  saveRDS(object = out, file = filename)
  .scc_plot(h, dataMatrix[deGeneUnion, ], res[[1]], res[[2]], tc$tree, consensusClusterLabels, tc$colors, plotName)
  out
}

reclusterDEConsensus <- function(dataMatrix, consensusClusterLabels, method = "Wilcoxon",
                                 meanScalingFactor = 5, qValThrs, fcThrs, deepSplitValues = 1:4,
                                 minClusterSize = 10, filename = "de_gene_object.rds",
                                 plotName = "DE_Heatmap") {
  if (method != "Wilcoxon") {
    print("Incorrect method chosen.")
    return(NULL)
  }
  sel <- .scc_codes(consensusClusterLabels, dataMatrix, minClusterSize)
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  res <- .Call("C_scc_de_slow", h, sel$code, length(sel$clusters),
               as.double(qValThrs), as.double(fcThrs), as.double(meanScalingFactor))
  K <- length(sel$clusters)
  qValueList <- rep(list(list()), K); logFCList <- rep(list(list()), K); deGeneList <- rep(list(list()), K)
  pcol <- 0L
  for (a in seq_len(K - 1)) for (b in (a + 1):K) {
    pcol <- pcol + 1L
    de <- as.integer(res[[4]][, pcol]) == 1L
    print(paste0(sel$clusters[a], ", ", sel$clusters[b], " DE genes: ", sum(de)))
    qValueList[[a]][[b]] <- res[[2]][, pcol]
    logFCList[[a]][[b]] <- res[[3]][, pcol]
    deGeneList[[a]][[b]] <- rownames(dataMatrix)[de]
  }
  names(qValueList) <- names(logFCList) <- names(deGeneList) <- sel$clusters
  saveRDS(object = qValueList, file = "qValueList.rds")
  saveRDS(object = logFCList, file = "logFCList.rds")
  saveRDS(object = deGeneList, file = "deGeneList.rds")
  deGeneUnion <- rownames(dataMatrix)[res[[1]]]
  print(str(deGeneUnion))
  saveRDS(deGeneUnion, file = "deGeneUnion.rds")
  tc <- if (.scc_tree_from_scores()) {
    .scc_tree_and_colors_scores(h, res[[1]], ncol(dataMatrix), deepSplitValues, minClusterSize, with_si = FALSE)
  } else if (.scc_tree_on_device()) {
    .scc_tree_and_colors_dev(h, res[[1]], ncol(dataMatrix), deepSplitValues, minClusterSize, with_si = FALSE)
  } else {
    d <- .scc_dist(h, res[[1]], ncol(dataMatrix))
    .scc_tree_and_colors(d, deepSplitValues, minClusterSize, with_si = FALSE)
  }
  out <- list("deGeneUnion" = deGeneUnion, "cellTree" = tc$tree, "dynamicColors" = tc$colors)
  saveRDS(object = out, file = filename)
  .scc_plot(h, as.matrix(dataMatrix)[deGeneUnion, ], res[[1]], res[[5]], tc$tree, consensusClusterLabels, tc$colors,
            plotName)
  out
}

# One-vs-rest marker genes of every selected cluster in one engine pass
# (scc_de_markers): the reference README's annotation step,
#   FindAllMarkers(min.pct = minPerCent / 100, logfc.threshold = logFCThrs, only.pos = onlyPos)
#   %>% group_by(cluster) %>% top_n(NumbertopDEGenes, avg_logFC)         (README.md:143-153)
# with ComputePairWiseDE's rules for each cluster against all other selected
# cells (Fast:73-355, 376-392; test.use = "wilcox" only).  Clusters are selected
# as in reclusterDEConsensusFast (.scc_codes).  Returns a Seurat-shaped data
# frame (p_val, avg_logFC, pct.1, pct.2, p_val_adj, cluster, gene), every tested
# row, cluster-major and inside a cluster in order(p_val, -avg_logFC); the
# columns kept (p_val_adj < qValThrs in a cluster with more than one row) and top
# (kept and within the top NumbertopDEGenes of |avg_logFC|, ties kept) mark what
# the reference's filter and top_n leave; attr(, "deGeneUnion") is unique() over
# the top rows.
sccFindAllMarkers <- function(dataMatrix, clusterLabels, minClusterSize = 10, minPerCent = 20,
                              logFCThrs = 0.5, qValThrs = 0.1, onlyPos = FALSE,
                              NumbertopDEGenes = 30) {
  sel <- .scc_codes(clusterLabels, dataMatrix, minClusterSize)
  if (length(sel$clusters) < 2) stop("need at least two clusters with > minClusterSize cells")
  h <- .scc_dataset(dataMatrix)
  on.exit(.Call("C_scc_release", h), add = TRUE)
  res <- .Call("C_scc_markers", h, sel$code, length(sel$clusters), as.double(qValThrs),
               as.double(logFCThrs), as.double(minPerCent), as.integer(NumbertopDEGenes),
               isTRUE(onlyPos))
  genes <- rownames(dataMatrix)
  out <- data.frame(p_val = res$p_val, avg_logFC = res$avg_logFC, pct.1 = res$pct.1, pct.2 = res$pct.2,
                    p_val_adj = res$p_val_adj,
                    cluster = factor(sel$clusters[res$cluster], levels = sel$clusters),
                    gene = genes[res$gene], kept = res$kept, top = res$top,
                    check.names = FALSE, stringsAsFactors = FALSE)
  attr(out, "deGeneUnion") <- genes[res$union]
  out
}
