"""Host-side mirror of the reference R API (same names, argument meaning and
error behaviour), running the data-parallel core on the MI355X engine.

Reference signatures:
  reclusterDEConsensusFast(dataMatrix, consensusClusterLabels, method = "wilcox",
      qValThrs = 0.1, logFCThrs = 0.5, deepSplitValues = 1:4, minClusterSize = 10,
      minPerCent = 20, filename = "de_gene_object.rds", plotName = "DE_Heatmap",
      NumbertopDEGenes = 30, nCores = 1)              R/reclusterDEConsensusFast.R:22-33
  reclusterDEConsensus(dataMatrix, consensusClusterLabels, method = "Wilcoxon",
      meanScalingFactor = 5, qValThrs, fcThrs, deepSplitValues = 1:4,
      minClusterSize = 10, filename = "de_gene_object.rds", plotName = "DE_Heatmap")
                                                       R/reclusterDEConsensus.R:20-29

What runs where: cluster selection (A0), printing and the
saved object stay on the host like in R; the pairwise DE, BH/filters/union and
the distance matrix run in libscc on the GPU; hclust(ward.D2), cutreeDynamic
(hybrid, pamStage = FALSE) and labels2colors run on the host as the reference
keeps them there (libscc's host functions scc_hclust_ward_d2 /
scc_cutree_hybrid).  With ``tree="device"`` (opt-in) the
distance stays in HBM and the tree and the cuts are computed on it there
(scc_hclust_ward_d2_dev / scc_cutree_hybrid_dev: the same results bit for
bit, no host copy of the distance).  With ``tree="scores"`` (opt-in) no
distance is computed at all: the tree and the cuts come from the N x 15 PCA
scores (scc_pca_scores / scc_hclust_ward_d2_scores / scc_cutree_hybrid_scores),
for cell counts whose N x N matrix fits nowhere.  That route returns the same
tree whenever no two candidate dissimilarities lie within rounding of each
other; on exact ties (duplicate cells) it returns a valid Ward tree that may
resolve the tie differently.  The ComplexHeatmap plot itself (PDF, colours,
annotation bars) is not drawn here, but what it computes before drawing is:
with ``heatmap=True`` (or an integer raster width) both functions add
``ret["heatmap"]`` (see ``heatmap_data``: the gene-row tree of
cellTypeDEPlot's ``cluster_rows = TRUE``, the row means, the colour ramp's
extrema and the binned raster), and with ``save=True`` write it to
``plotName + ".npz"``; ``plotName`` is otherwise unused.
"""
from __future__ import annotations

import numpy as np

from . import _native as nat

_ENGINES: dict = {}


def _engine(device: int = 0) -> nat.Engine:
    if device not in _ENGINES:
        _ENGINES[device] = nat.Engine(device)
    return _ENGINES[device]


def select_clusters(labels, min_cluster_size: int, cluster_order=None):
    """A0 (Fast:40-53, slow:39-54): table(labels); keep count > minClusterSize;
    drop names containing "grey".  Returns (names, code[N]) with code = -1 for
    cells not compared.  R orders table() names by the locale's collation;
    the default here is code-point order (R's C locale) — pass
    ``cluster_order`` to reproduce another collation."""
    raw = np.asarray(labels, dtype=object)
    # R's table() drops NA and `labels == x` never matches NA (Fast:40-44): a
    # missing label (None / NaN / pandas NA) is no cluster, its cell coded -1
    missing = np.fromiter((_is_missing(v) for v in raw), bool, len(raw))
    labels = raw.astype(str)
    names, counts = np.unique(labels[~missing], return_counts=True)
    if cluster_order is not None:
        pos = {n: i for i, n in enumerate(cluster_order)}
        idx = sorted(range(len(names)), key=lambda i: pos.get(names[i], len(pos) + i))
        names, counts = names[idx], counts[idx]
    keep = [str(n) for n, c in zip(names, counts) if c > min_cluster_size and "grey" not in str(n)]
    lut = {n: i for i, n in enumerate(keep)}
    code = np.fromiter((lut.get(s, -1) for s in labels), np.int32, len(labels))
    code[missing] = -1
    return keep, code


def _is_missing(v) -> bool:
    if v is None:
        return True
    if isinstance(v, (float, np.floating)):
        return bool(np.isnan(v))
    try:
        import pandas as pd
        return v is pd.NA or v is pd.NaT
    except ImportError:  # pragma: no cover
        return False


def _as_matrix(dataMatrix):
    """Accept scipy.sparse (genes x cells), numpy dense (genes x cells) or a
    synth.Dataset; return ('csc' | 'csr', indptr, idx, vals, G, N) or ('dense', X)."""
    try:
        import scipy.sparse as sp
        if sp.issparse(dataMatrix) and dataMatrix.format == "csr":  # gene-major: transposed on the device
            m = dataMatrix.copy() if not dataMatrix.has_sorted_indices else dataMatrix
            m.sort_indices()
            return "csr", m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64), \
                m.shape[0], m.shape[1]
        if sp.issparse(dataMatrix):
            m = dataMatrix.tocsc()
            m.sort_indices()
            return "csc", m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64), \
                m.shape[0], m.shape[1]
    except ImportError:  # pragma: no cover
        pass
    if hasattr(dataMatrix, "indptr") and hasattr(dataMatrix, "labels"):
        d = dataMatrix
        return "csc", d.indptr, d.indices, d.data, d.G, d.N
    X = np.asarray(dataMatrix, np.float64)
    return "dense", X


def _upload(eng, m):
    if m[0] == "csc":
        _, indptr, rows, vals, G, N = m
        return eng.dataset_csc(indptr, rows, vals, G, N)
    if m[0] == "csr":
        _, indptr, cols, vals, G, N = m
        return eng.dataset_csr(indptr, cols, vals, G, N)
    return eng.dataset_dense(m[1])


# WGCNA standardColors(): the 34 base colours (labels2colors' palette for
# labels 1..34).  WGCNA extends the list with the rest of R's colors() in a
# fixed pseudo-random order; R is absent here, so labels above 34 use the
# first entries of that extension as recalled (unpinned) and then "colorK".
STANDARD_COLORS = [
    "turquoise", "blue", "brown", "yellow", "green", "red", "black", "pink", "magenta", "purple", "greenyellow",
    "tan", "salmon", "cyan", "midnightblue", "lightcyan", "grey60", "lightgreen", "lightyellow", "royalblue",
    "darkred", "darkgreen", "darkturquoise", "darkgrey", "orange", "darkorange", "white", "skyblue", "saddlebrown",
    "steelblue", "paleturquoise", "violet", "darkolivegreen", "darkmagenta",
    "sienna3", "yellowgreen", "skyblue3", "plum1", "orangered4", "mediumpurple3", "lightsteelblue1", "lightcyan1",
    "ivory", "floralwhite", "darkorange2", "brown4", "bisque4", "darkslateblue", "plum2", "thistle2", "thistle1",
    "salmon4", "palevioletred3", "navajowhite2", "maroon", "lightpink4", "lavenderblush3", "honeydew1",
    "darkseagreen4", "coral1", "antiquewhite4", "coral2", "mediumorchid", "skyblue2", "yellow4", "skyblue1", "plum",
    "orangered3", "mediumpurple2", "lightsteelblue", "lightcoral", "indianred4", "firebrick4", "darkolivegreen4",
    "brown2", "blue2", "darkviolet", "plum3", "thistle3", "thistle",
]


def labels2colors(labels):
    """WGCNA::labels2colors(labels) for numeric labels (Fast:428): 0 -> "grey",
    k -> standardColors()[k]."""
    lab = np.asarray(labels)
    return [("grey" if v == 0 else STANDARD_COLORS[v - 1] if v <= len(STANDARD_COLORS) else f"color{v}")
            for v in lab.tolist()]


def _hclust_ward_d2(dist_packed, N):
    """fastcluster::hclust(d, "ward.D2") (Fast:406-411) -> R hclust fields."""
    merge, height, order = nat.hclust_ward_d2(dist_packed, N)
    return {"merge": merge, "height": height, "order": order, "method": "ward.D2", "dist.method": "euclidean"}


def _hclust_ward_d2_dev(eng, N):
    """The same tree from the engine-kept distance (tree="device")."""
    merge, height, order = eng.hclust_ward_d2_dev(N)
    return {"merge": merge, "height": height, "order": order, "method": "ward.D2", "dist.method": "euclidean"}


def _hclust_ward_d2_scores(eng, N):
    """The tree from the engine-kept PCA scores (tree="scores")."""
    merge, height, order = eng.hclust_ward_d2_scores(N)
    return {"merge": merge, "height": height, "order": order, "method": "ward.D2", "dist.method": "euclidean"}


def _check_tree(tree):
    if tree not in ("host", "device", "scores"):
        raise ValueError(f"tree must be 'host', 'device' or 'scores', not {tree!r}")
    return tree == "device"


def _distance_and_tree(eng, ds, uni, N, tree):
    """Fast:398-411, slow:234-247: (d, cellTree).  d is the packed host vector
    for tree="host" and None otherwise (tree="device": it stays in the engine;
    tree="scores": it is never computed)."""
    if tree == "scores":
        eng.pca_scores(ds, uni)
        return None, _hclust_ward_d2_scores(eng, N)
    on_device = tree == "device"
    d = eng.distance(ds, uni, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0 if on_device else None)
    return d, (_hclust_ward_d2_dev(eng, N) if on_device else _hclust_ward_d2(d, N))


def _dynamic_colors(tree, dist_packed, deepSplitValues, minClusterSize, eng=None, info=None, cut_eng=None,
                    scores_eng=None, scores_si=False):
    """Fast:418-431: cutreeDynamic(dendro, distM = as.matrix(d), deepSplit = dsv,
    pamStage = FALSE, minClusterSize) -> labels2colors, named "deepsplit: dsv".
    With ``eng`` (FAST, which computes the silhouette for every deepSplit):
    R's stop when a deepSplit yields < 2 groups; with a list ``info`` too, the
    reference's deepSplitInfo rows
    (Fast:433: DeepSplit, NumbersOfClusters, SI = mean of
    summary(cluster::silhouette(groups, as.matrix(d)))$clus.avg.widths), the
    silhouette computed by the engine on its HBM-resident copy of d.
    With ``cut_eng`` the cut reads that HBM-resident copy too (dist_packed is
    not used).  With ``scores_eng`` there is no distance: the cut computes its
    distM entries from the engine-kept scores; the rows' SI is None unless
    ``scores_si``, which computes it from the scores too (silhouette_scores:
    the SI of the matrix routes, bit for bit, for equal labels)."""
    out = {}
    N = len(tree["order"])
    for dsv in deepSplitValues:
        if scores_eng is not None:
            lab, _ = scores_eng.cutree_hybrid_scores(tree["merge"], tree["height"], int(dsv), int(minClusterSize))
        elif cut_eng is not None:
            lab, _ = cut_eng.cutree_hybrid_dev(tree["merge"], tree["height"], int(dsv), int(minClusterSize))
        else:
            lab, _ = nat.cutree_hybrid(tree["merge"], tree["height"], dist_packed, int(dsv), int(minClusterSize))
        out[f"deepsplit: {dsv}"] = labels2colors(lab)
        if eng is not None:
            lab = np.asarray(lab, np.int32)
            k = len(np.unique(lab))
            if not 2 <= k < N:
                # silhouette() returns NA and summary(NA)$clus.avg.widths stops (Fast:433)
                raise RuntimeError("$ operator is invalid for atomic vectors (silhouette of "
                                   f"{k} group(s) at deepSplit {dsv}, Fast:433)")
            if info is not None:  # the SI the reference computes and discards
                if scores_eng is None:
                    si = float(np.mean(eng.silhouette(N, lab)[1]))
                else:
                    si = float(np.mean(scores_eng.silhouette_scores(N, lab)[1])) if scores_si else None
                info.append({"DeepSplit": dsv, "NumbersOfClusters": k, "SI": si})
    return out


def _heatmap(eng, ds, uni, cell_tree, width=None, row_reorder="-mean"):
    """heatmap_data on an uploaded dataset (cellTypeDEPlot.R:168-253)."""
    if row_reorder not in ("-mean", None):
        raise ValueError(f"row_reorder must be '-mean' or None, not {row_reorder!r}")
    uni = np.ascontiguousarray(uni, np.int32)
    nu, N = len(uni), ds.N
    col_order = np.asarray(cell_tree["order"], np.int32)
    if width is None or width is True:
        width = min(N, 4096)
    d, means, rng = eng.gene_distance(ds, uni)
    merge, height, order = nat.hclust_complete(d, nu)
    if row_reorder == "-mean":  # ComplexHeatmap's default: reorder.dendrogram(, -rowMeans(mat), mean)
        merge, order = nat.dendro_reorder(merge, -means)
    raster = eng.heatmap_raster(ds, uni, order, col_order, int(width))
    return {"rowTree": {"merge": merge, "height": height, "order": order, "method": "complete",
                        "dist.method": "euclidean"},
            "rowOrder": order, "colOrder": col_order, "rowMeans": means, "range": rng, "raster": raster}


def heatmap_data(dataMatrix, union_idx, cellTree, width=None, row_reorder="-mean", device=0):
    """What cellTypeDEPlot(dataMatrix[deGeneUnion, ], ...) computes before it
    draws (ComplexHeatmap::Heatmap(cluster_rows = TRUE, use_raster = TRUE),
    cellTypeDEPlot.R:168-253), on the engine: a dict with
      rowTree   hclust(dist(X[U, ]), "complete") of the gene rows (merge,
                height, order, method), reordered by ``row_reorder`` ("-mean":
                reorder.dendrogram by -rowMeans with agglo.FUN = mean, the
                ComplexHeatmap default; None: the tree as hclust returns it)
      rowOrder  rowTree's 1-based leaf order (positions into union_idx)
      colOrder  cellTree["order"]
      rowMeans  rowMeans(X[U, ])
      range     min x, max x, min |x|, max |x| over the block (the colour ramp)
      raster    |U| x width bin means in (rowOrder, colOrder) order;
                width=None: min(N, 4096)
    union_idx: 0-based gene rows (at least two)."""
    eng = _engine(device)
    ds = _upload(eng, _as_matrix(dataMatrix))
    try:
        return _heatmap(eng, ds, union_idx, cellTree, width, row_reorder)
    finally:
        ds.close()


def _heatmap_opt(eng, ds, uni, cell_tree, heatmap, save, plotName):
    """The recluster* functions' ``heatmap`` keyword: False / True / a raster width."""
    if heatmap is False or heatmap is None:
        return None
    hm = _heatmap(eng, ds, uni, cell_tree, None if heatmap is True else int(heatmap))
    if save and plotName:
        np.savez(plotName + ".npz", merge=hm["rowTree"]["merge"], height=hm["rowTree"]["height"],
                 rowOrder=hm["rowOrder"], colOrder=hm["colOrder"], rowMeans=hm["rowMeans"], range=hm["range"],
                 raster=hm["raster"])
    return hm


def _save(obj, filename):
    if not filename:
        return
    import pickle
    with open(filename if filename.endswith(".pkl") else filename + ".pkl", "wb") as f:
        pickle.dump(obj, f)


def reclusterDEConsensusFast(dataMatrix, consensusClusterLabels, method="wilcox", qValThrs=0.1, logFCThrs=0.5,
                             deepSplitValues=(1, 2, 3, 4), minClusterSize=10, minPerCent=20,
                             filename="de_gene_object.rds", plotName="DE_Heatmap", NumbertopDEGenes=30, nCores=1,
                             *, gene_names=None, cluster_order=None, device=0, save=False, return_details=False,
                             tree="host", scores_si=False, heatmap=False):
    on_device = _check_tree(tree)
    if scores_si and tree != "scores":
        raise ValueError('scores_si=True needs tree="scores" (the other routes compute SI from the distance)')
    if method not in ("wilcox", "t", "bimod"):
        # Fast:306-333: "roc" yields no p_val_adj, which the caller filters on (Fast:343-351,377)
        raise NotImplementedError(f"Unknown test: {method} (this engine implements test.use = 'wilcox', 't' "
                                  "and 'bimod')")
    eng = _engine(device)
    m = _as_matrix(dataMatrix)
    N = m[-1] if m[0] in ("csc", "csr") else m[1].shape[1]
    G = m[-2] if m[0] in ("csc", "csr") else m[1].shape[0]
    names, code = select_clusters(consensusClusterLabels, minClusterSize, cluster_order)
    if len(names) < 2:
        raise ValueError("need at least two clusters with > minClusterSize cells")
    ds = _upload(eng, m)
    # any K: more than 128 clusters run as group-pair runs inside libscc (scc_de_run)
    res = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, q_val_thrs=qValThrs, log_fc_thrs=logFCThrs,
                     min_per_cent=float(minPerCent), top_n=NumbertopDEGenes,
                     fetch="rows" if return_details else "union", test=method)
    if res.status == nat.SCC_ERR_RSTOP:
        raise RuntimeError(res.message)
    uni = res.union
    gnames = np.asarray(gene_names if gene_names is not None else [f"gene{g}" for g in range(G)], dtype=object)
    print(f" chr [1:{len(uni)}] " + " ".join(f'"{g}"' for g in gnames[uni[:5]]) + (" ..." if len(uni) > 5 else ""))
    if len(uni) == 0:
        raise RuntimeError("no DE genes (R fails on an empty deGenes data frame, Fast:386)")
    # tree="device": the distance stays in the engine (d is None), the tree, the cuts and the silhouette read it there;
    # tree="scores": no distance, the tree and the cuts (and with scores_si the silhouette) read the engine-kept scores
    d, cell_tree = _distance_and_tree(eng, ds, uni, N, tree)
    info = [] if return_details else None  # deepSplitInfo: computed by the reference, never returned (Fast:433)
    ret = {"deGeneUnion": list(gnames[uni]), "cellTree": cell_tree,
           "dynamicColors": _dynamic_colors(cell_tree, d, deepSplitValues, minClusterSize, eng, info,
                                            cut_eng=eng if on_device else None,
                                            scores_eng=eng if tree == "scores" else None,
                                            scores_si=bool(scores_si))}
    hm = _heatmap_opt(eng, ds, uni, cell_tree, heatmap, save, plotName)
    if hm is not None:
        ret["heatmap"] = hm
    if save:
        _save(ret, filename)
    if return_details:
        ret["_details"] = {"clusters": names, "code": code, "de": res, "dist": d, "union_idx": uni,
                           "deepSplitInfo": info}
    ds.close()
    return ret


def reclusterDEConsensus(dataMatrix, consensusClusterLabels, method="Wilcoxon", meanScalingFactor=5, qValThrs=None,
                         fcThrs=None, deepSplitValues=(1, 2, 3, 4), minClusterSize=10, filename="de_gene_object.rds",
                         plotName="DE_Heatmap", *, gene_names=None, cluster_order=None, device=0, save=False,
                         return_details=False, tree="host", heatmap=False):
    on_device = _check_tree(tree)
    if qValThrs is None or fcThrs is None:
        raise TypeError('argument "qValThrs"/"fcThrs" is missing, with no default')
    if method == "edgeR":
        raise NotImplementedError("edgeR branch stays on the host in the reference design (SURVEY D3)")
    if method != "Wilcoxon":
        print("Incorrect method chosen.")  # slow:158-161
        return None
    eng = _engine(device)
    m = _as_matrix(dataMatrix)
    N = m[-1] if m[0] in ("csc", "csr") else m[1].shape[1]
    G = m[-2] if m[0] in ("csc", "csr") else m[1].shape[0]
    names, code = select_clusters(consensusClusterLabels, minClusterSize, cluster_order)
    if len(names) < 2:
        raise ValueError("need at least two clusters with > minClusterSize cells")
    ds = _upload(eng, m)
    res = eng.de_run(ds, code, len(names), nat.SCC_DE_SLOW, q_val_thrs=qValThrs, fc_thrs=fcThrs,
                     mean_scaling_factor=float(meanScalingFactor), fetch="all")
    if res.status == nat.SCC_ERR_RSTOP:
        raise RuntimeError(res.message)
    gnames = np.asarray(gene_names if gene_names is not None else [f"gene{g}" for g in range(G)], dtype=object)
    K = len(names)
    p = 0
    qlist, lflist, delist = {}, {}, {}
    for i in range(K - 1):
        for j in range(i + 1, K):
            n_de = int((res.de[p] == 1).sum())
            print(f"{names[i]}, {names[j]} DE genes: {n_de}")  # slow:172-178
            qlist[(names[i], names[j])] = res.q[p]
            lflist[(names[i], names[j])] = res.logfc[p]
            delist[(names[i], names[j])] = list(gnames[res.de[p] == 1])
            p += 1
    uni = res.union
    if len(uni) == 0:
        raise RuntimeError("empty DE gene union")
    d, cell_tree = _distance_and_tree(eng, ds, uni, N, tree)
    ret = {"deGeneUnion": list(gnames[uni]), "cellTree": cell_tree,
           "dynamicColors": _dynamic_colors(cell_tree, d, deepSplitValues, minClusterSize,
                                            cut_eng=eng if on_device else None,
                                            scores_eng=eng if tree == "scores" else None)}
    hm = _heatmap_opt(eng, ds, uni, cell_tree, heatmap, save, plotName)
    if hm is not None:
        ret["heatmap"] = hm
    if save:
        _save({"qValueList": qlist, "logFCList": lflist, "deGeneList": delist}, "de_lists")
        _save(ret, filename)
    if return_details:
        ret["_details"] = {"clusters": names, "code": code, "de": res, "dist": d, "union_idx": uni}
    ds.close()
    return ret


def findAllMarkers(dataMatrix, clusterLabels, minClusterSize=10, minPerCent=20, logFCThrs=0.5, qValThrs=0.1,
                   onlyPos=False, NumbertopDEGenes=30, device=0, *, gene_names=None, cluster_order=None):
    """One-vs-rest marker genes of every cluster in one engine pass
    (scc_de_markers): the reference README's ``FindAllMarkers(min.pct,
    logfc.threshold, only.pos)`` followed by ``top_n(NumbertopDEGenes,
    avg_logFC)`` per cluster (README.md:143-153), each cluster tested against
    all other selected cells with ComputePairWiseDE's rules (Fast:73-355).
    Clusters are selected as in the two recluster functions
    (``select_clusters``: more than minClusterSize cells, no "grey").

    Returns ``{"markers": {cluster name: table}, "union": [gene names],
    "union_idx": int32 rows, "clusters": names}``; a table is a dict of
    equal-length arrays ``gene``, ``gene_idx``, ``p_val``, ``avg_logFC``,
    ``pct.1``, ``pct.2``, ``p_val_adj``, ``kept`` (p_val_adj < qValThrs in a
    cluster with more than one tested row) and ``top`` (kept and within the top
    NumbertopDEGenes of |avg_logFC|, ties kept), rows in R's order(p_val,
    -avg_logFC).  ``union`` is unique() over the clusters' top rows in order."""
    eng = _engine(device)
    m = _as_matrix(dataMatrix)
    G = m[-2] if m[0] in ("csc", "csr") else m[1].shape[0]
    names, code = select_clusters(clusterLabels, minClusterSize, cluster_order)
    if len(names) < 2:
        raise ValueError("need at least two clusters with > minClusterSize cells")
    ds = _upload(eng, m)
    try:
        res = eng.de_markers(ds, code, len(names), q_val_thrs=qValThrs, log_fc_thrs=logFCThrs,
                             min_per_cent=float(minPerCent), top_n=NumbertopDEGenes, only_pos=bool(onlyPos),
                             fetch="rows")
    finally:
        ds.close()
    if res.status == nat.SCC_ERR_RSTOP:
        raise RuntimeError(res.message)
    gnames = np.asarray(gene_names if gene_names is not None else [f"gene{g}" for g in range(G)], dtype=object)
    r = res.rows
    starts = np.concatenate([[0], np.cumsum(r.pair_tested)]).astype(np.int64)
    markers = {}
    for a, name in enumerate(names):
        s = slice(int(starts[a]), int(starts[a + 1]))
        markers[name] = {"gene": gnames[r.gene[s]], "gene_idx": r.gene[s].copy(), "p_val": r.p[s].copy(),
                         "avg_logFC": r.avg_logfc[s].copy(), "pct.1": r.pct1[s].copy(), "pct.2": r.pct2[s].copy(),
                         "p_val_adj": r.q[s].copy(), "kept": r.de[s].copy(), "top": r.top[s].copy()}
    return {"markers": markers, "union": list(gnames[res.union]), "union_idx": res.union, "clusters": names}


def nearest_neighbors(dataMatrix, genes, k=15, ncomp=15, dims=None, include_self=True, device=0, *,
                      gene_names=None):
    """The exact k-nearest-neighbour graph of the cells from their PCA scores,
    the search the reference README's last step starts with
    (``prcomp_irlba(n = 15)`` on the marker union, ``pca.data <-
    pca.obj$x[, 1:8]``, ``umap::umap(d = pca.data)``, README.md:152-155), on
    the engine and without an N x N matrix (scc_pca_scores, scc_knn_scores).

    genes: the gene rows the PCA runs on (findAllMarkers' ``union_idx``), as
    0-based row indices, or as names when ``gene_names`` lists every row's
    name.  ncomp: components the PCA keeps (at most 15).  dims: leading
    components the distance uses (None: all ncomp; the README uses 8 of 15).

    Returns ``{"indexes": int32 [N, k] 0-based, "distances": float64 [N, k],
    "scores": float64 [N, ncomp]}``, each row ordered by (distance, index).
    With ``include_self`` column 0 is the cell itself at distance 0 and the
    k - 1 nearest other cells follow; without it, the k nearest other cells.
    Whether a consumer expects the cell itself first differs between packages,
    which is why it is a parameter."""
    g = np.asarray(genes)
    if g.dtype.kind in "USO":
        if gene_names is None:
            raise ValueError("genes given by name need gene_names")
        pos = {name: r for r, name in enumerate(gene_names)}
        try:
            g = np.array([pos[name] for name in g], np.int32)
        except KeyError as e:
            raise ValueError(f"unknown gene {e.args[0]!r}") from None
    g = np.ascontiguousarray(g, np.int32)
    k, ncomp = int(k), int(ncomp)
    dims = ncomp if dims is None else int(dims)
    if not 1 <= dims <= ncomp:
        raise ValueError("dims must lie in 1..ncomp")
    others = k - 1 if include_self else k
    if others < 1:
        raise ValueError("k leaves no neighbour besides the cell itself")
    eng = _engine(device)
    ds = _upload(eng, _as_matrix(dataMatrix))
    try:
        N = ds.N
        eng.pca_scores(ds, g, ncomp)
        idx, dist = eng.knn_scores(N, others, dims)
        scores = eng.last_pca_scores(N)
    finally:
        ds.close()
    if include_self:
        idx = np.concatenate([np.arange(N, dtype=np.int32)[:, None], idx], axis=1)
        dist = np.concatenate([np.zeros((N, 1)), dist], axis=1)
    return {"indexes": idx, "distances": dist, "scores": scores}


def umap_ab_params(min_dist=0.1, spread=1.0):
    """The curve constants (a, b) of 1 / (1 + a d^(2b)) for min_dist and spread:
    umap-learn's find_ab_params recipe (scipy.optimize.curve_fit on 300 points
    of [0, 3 spread]).  Without scipy only the default pair is available, from
    the constants that recipe gave (nat.UMAP_A, nat.UMAP_B)."""
    min_dist, spread = float(min_dist), float(spread)
    if not (spread > 0.0 and 0.0 <= min_dist <= spread):
        raise ValueError("min_dist must lie in [0, spread] and spread be positive")
    try:
        from scipy.optimize import curve_fit
    except ImportError:
        if (min_dist, spread) == (0.1, 1.0):
            return nat.UMAP_A, nat.UMAP_B
        raise ValueError("fitting a, b for a non-default min_dist or spread needs scipy") from None
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


def umap(dataMatrix, genes, n_neighbors=15, ncomp=15, dims=None, n_epochs=200, min_dist=0.1, spread=1.0, seed=0,
         init=None, set_op_mix_ratio=1.0, gamma=1.0, negative_sample_rate=5, learning_rate=1.0, return_graph=False,
         device=0, *, gene_names=None):
    """The reference README's last step, ``umap::umap(d = pca.data)`` on
    ``pca.data <- pca.obj$x[, 1:8]`` (README.md:152-160), on the engine: the PCA
    of the gene rows, the exact neighbour search, the fuzzy simplicial set and
    the stochastic-gradient layout (scc_pca_scores, scc_umap_scores) without
    the table or the graph leaving the device.  Deterministic for a seed.  The
    rules are umap-learn's (tests/umap_reference.py restates them); agreement
    with the umap, uwot or umap-learn packages has not been measured.

    genes, ncomp, dims, gene_names: as ``nearest_neighbors``.  n_neighbors
    counts the cell itself (2..65).  init: an [N, 2] array, or None for the
    first two score columns scaled so that the largest absolute coordinate is
    10 (no spectral initialisation).  a, b are fitted from min_dist and spread
    (``umap_ab_params``).

    Returns ``{"layout": float64 [N, 2], "graph": (indptr, cols, vals) or
    None}``, the graph (symmetric CSR, columns ascending) only with
    ``return_graph``."""
    g = np.asarray(genes)
    if g.dtype.kind in "USO":
        if gene_names is None:
            raise ValueError("genes given by name need gene_names")
        pos = {name: r for r, name in enumerate(gene_names)}
        try:
            g = np.array([pos[name] for name in g], np.int32)
        except KeyError as e:
            raise ValueError(f"unknown gene {e.args[0]!r}") from None
    g = np.ascontiguousarray(g, np.int32)
    n_neighbors, ncomp = int(n_neighbors), int(ncomp)
    dims = ncomp if dims is None else int(dims)
    if not 1 <= dims <= ncomp:
        raise ValueError("dims must lie in 1..ncomp")
    if n_neighbors < 2:
        raise ValueError("n_neighbors leaves no neighbour besides the cell itself")
    a, b = umap_ab_params(min_dist, spread)
    eng = _engine(device)
    ds = _upload(eng, _as_matrix(dataMatrix))
    try:
        eng.pca_scores(ds, g, ncomp)
        out = eng.umap_scores(ds.N, n_neighbors, dims, None, init, n_epochs, a, b, gamma, negative_sample_rate,
                              learning_rate, seed, set_op_mix_ratio, return_graph=bool(return_graph))
    finally:
        ds.close()
    return {"layout": out[0], "graph": out[1]} if return_graph else {"layout": out, "graph": None}


def find_clusters(dataMatrix, genes, k_param=20, ncomp=15, dims=None, prune=1.0 / 15.0, resolution=0.8,
                  return_graph=False, device=0, *, gene_names=None):
    """The step in front of the reference README's example: its
    ``seuratObj$RNA_snn_res.0.2`` is what Seurat's ``FindNeighbors`` +
    ``FindClusters`` make of the PCA scores.  On the engine: the PCA of the
    gene rows, the exact neighbour search, the shared-nearest-neighbour graph
    (Seurat's ComputeSNN rule) and a deterministic multilevel modularity
    clustering (scc_pca_scores, scc_snn_clusters_scores) without the table or
    the graph leaving the device.  The rules are restated in
    tests/snn_reference.py; agreement with Seurat has not been measured, and
    there is no Leiden or SLM refinement, no grouping of singletons and no
    random vertex order.

    genes, ncomp, dims, gene_names: as ``nearest_neighbors``.  k_param counts
    the cell itself (2..65).  Returns ``{"labels": int32 [N] (0 the largest
    cluster; ``reclusterDEConsensusFast`` takes them as they are),
    "n_clusters", "modularity", "n_levels", "sweeps", "graph": (indptr, cols,
    vals) or None}``, the graph only with ``return_graph``."""
    g = np.asarray(genes)
    if g.dtype.kind in "USO":
        if gene_names is None:
            raise ValueError("genes given by name need gene_names")
        pos = {name: r for r, name in enumerate(gene_names)}
        try:
            g = np.array([pos[name] for name in g], np.int32)
        except KeyError as e:
            raise ValueError(f"unknown gene {e.args[0]!r}") from None
    g = np.ascontiguousarray(g, np.int32)
    k_param, ncomp = int(k_param), int(ncomp)
    dims = ncomp if dims is None else int(dims)
    if not 1 <= dims <= ncomp:
        raise ValueError("dims must lie in 1..ncomp")
    if k_param < 2:
        raise ValueError("k_param leaves no neighbour besides the cell itself")
    eng = _engine(device)
    ds = _upload(eng, _as_matrix(dataMatrix))
    try:
        eng.pca_scores(ds, g, ncomp)
        out = eng.snn_clusters_scores(ds.N, k_param, dims, prune, resolution, None, return_graph=bool(return_graph))
    finally:
        ds.close()
    out.setdefault("graph", None)
    out.pop("nnz", None)
    return out
