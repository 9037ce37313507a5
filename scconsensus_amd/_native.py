"""ctypes binding of ``lib/libscc.so`` — the C ABI declared in ``include/scc.h``.

There is no fallback: if the HIP library is missing this module raises, and if
no MI355X is visible ``Engine()`` raises ``SccError(SCC_ERR_HIP)``.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import weakref
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libscc.so")

SCC_OK = 0
SCC_ERR_INVALID = 1
SCC_ERR_HIP = 2
SCC_ERR_OOM = 3
SCC_ERR_NONFINITE = 4
SCC_ERR_RSTOP = 5
SCC_ERR_UNSUPPORTED = 6
SCC_DE_FAST = 0
SCC_DE_SLOW = 1
SCC_TEST_WILCOX = 0
SCC_TEST_T = 1
SCC_TEST_BIMOD = 2
_TEST_CODES = {"wilcox": SCC_TEST_WILCOX, "t": SCC_TEST_T, "bimod": SCC_TEST_BIMOD}
SCC_DIST_PCA_EUCLID = 0
SCC_DIST_PEARSON = 1
SCC_PTR_HOST = 0
SCC_PTR_DEVICE = 1
HCLUST_MERGES_PER_LAUNCH = 1024  # SCC_HCLUST_MERGES_PER_LAUNCH: merges per chain launch of hclust_ward_d2_dev
HCLUST_VEC_SCAN_NODES = 512  # SCC_HCLUST_VEC_SCAN_NODES: nodes a scan workgroup of hclust_ward_d2_scores owns
HCLUST_VEC_SCANS_PER_BATCH = 1024  # SCC_HCLUST_VEC_SCANS_PER_BATCH: scans (two launches each) between state reads

# every symbol include/scc.h declares (tests check the library exports them all)
EXPORTS = [
    "scc_ctx_create", "scc_device_count", "scc_ctx_destroy", "scc_ctx_last_error", "scc_ctx_synchronize", "scc_ctx_set_stream",
    "scc_ctx_kernel_time",
    "scc_ctx_reset_timers", "scc_dataset_create_csc", "scc_dataset_create_csr", "scc_dataset_create_dense", "scc_dataset_destroy",
    "scc_dataset_read_csc",
    "scc_de_run", "scc_de_shard_bytes", "scc_de_run_shard", "scc_de_finish", "scc_de_run_shard_records",
    "scc_de_finish_records", "scc_de_finish_records_pairs", "scc_de_union_first_occ", "scc_de_result_counts", "scc_de_result_union", "scc_de_result_rows",
    "scc_de_result_pair_vectors", "scc_de_result_log_threshold", "scc_de_result_nodg", "scc_de_result_destroy",
    "scc_de_markers", "scc_de_result_ties",
    "scc_distance", "scc_de_distance", "scc_distance_cols", "scc_pca_shard_colsum", "scc_pca_shard_gram", "scc_pca_shard_scores", "scc_pca_shard_eigen", "scc_pca_shard_project",
    "scc_distance_scores", "scc_silhouette", "scc_last_pca_scores",
    "scc_hclust_ward_d2", "scc_cutree_hybrid", "scc_hclust_ward_d2_dev", "scc_cutree_hybrid_dev",
    "scc_pca_scores", "scc_hclust_ward_d2_scores", "scc_cutree_hybrid_scores", "scc_silhouette_scores",
    "scc_knn_scores", "scc_umap_graph", "scc_umap_layout", "scc_umap_scores",
    "scc_snn_graph", "scc_modularity_cluster", "scc_snn_clusters_scores",
    "scc_gene_distance", "scc_hclust_complete", "scc_dendro_reorder", "scc_heatmap_raster",
    "scc_diag_eigen_topk", "scc_diag_small_syev", "scc_diag_cholinv", "scc_diag_eig_last_path",
    "scc_diag_ingest_last_path", "scc_diag_rank_last_route", "scc_diag_rank_last_runs", "scc_diag_mirror_last_uses", "scc_diag_hclust_last_scans",
    "scc_diag_small_syev_stamps", "scc_diag_pvalues",
]


class SccError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"scc error {code}: {msg}")
        self.code = code


class Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("profile", ctypes.c_int32), ("n_devices", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5), ("devices", ctypes.POINTER(ctypes.c_int32))]


class DeParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("top_n", ctypes.c_int32), ("q_val_thrs", ctypes.c_double),
                ("log_fc_thrs", ctypes.c_double), ("min_per_cent", ctypes.c_double), ("fc_thrs", ctypes.c_double),
                ("mean_scaling_factor", ctypes.c_double), ("test_all", ctypes.c_int32),
                ("test", ctypes.c_int32)]


class MarkersParams(ctypes.Structure):
    _fields_ = [("top_n", ctypes.c_int32), ("only_pos", ctypes.c_int32), ("test", ctypes.c_int32),
                ("test_all", ctypes.c_int32), ("q_val_thrs", ctypes.c_double), ("log_fc_thrs", ctypes.c_double),
                ("min_per_cent", ctypes.c_double), ("reserved", ctypes.c_int32 * 4)]


class UmapParams(ctypes.Structure):
    _fields_ = [("local_connectivity", ctypes.c_double), ("bandwidth", ctypes.c_double),
                ("set_op_mix_ratio", ctypes.c_double), ("n_epochs", ctypes.c_int32),
                ("negative_sample_rate", ctypes.c_int32), ("a", ctypes.c_double), ("b", ctypes.c_double),
                ("gamma", ctypes.c_double), ("learning_rate", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("reserved", ctypes.c_int32 * 4)]


MODULARITY_MAX_LEVELS = 32  # scc.h: SCC_MODULARITY_MAX_LEVELS

# find_ab_params(spread = 1, min_dist = 0.1) (scc.h: SCC_UMAP_A, SCC_UMAP_B)
UMAP_A = 1.5769434602697652
UMAP_B = 0.8950608778515733


def _umap_params(set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, n_epochs=200, a=0.0, b=0.0, gamma=1.0,
                 negative_sample_rate=5, learning_rate=1.0, seed=0):
    return UmapParams(float(local_connectivity), float(bandwidth), float(set_op_mix_ratio), int(n_epochs),
                      int(negative_sample_rate), float(a), float(b), float(gamma), float(learning_rate),
                      int(seed) & 0xFFFFFFFFFFFFFFFF)


_lib = None
_live_datasets: "weakref.WeakSet" = weakref.WeakSet()
_live_engines: "weakref.WeakSet" = weakref.WeakSet()
_shutdown = False


@atexit.register
def _teardown():
    # release device objects in dependency order while the HIP runtime is
    # still alive (interpreter-exit __del__ order is arbitrary)
    global _shutdown
    for d in list(_live_datasets):
        d.close()
    for e in list(_live_engines):
        e.close()
    _shutdown = True


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -m scconsensus_amd.build` (hipcc, gfx950)")
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    P = ctypes.POINTER
    i32, i64, dbl, u8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_uint8
    sig = {
        "scc_ctx_create": (ctypes.c_int, [P(Opts), P(vp)]),
        "scc_device_count": (ctypes.c_int, [P(i32)]),
        "scc_ctx_destroy": (None, [vp]),
        "scc_ctx_last_error": (ctypes.c_char_p, [vp]),
        "scc_ctx_synchronize": (ctypes.c_int, [vp]),
        "scc_ctx_set_stream": (ctypes.c_int, [vp, vp, i32]),
        "scc_ctx_kernel_time": (ctypes.c_int, [vp, ctypes.c_char_p, P(dbl), P(i64)]),
        "scc_ctx_reset_timers": (None, [vp]),
        "scc_dataset_create_csc": (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, i32, P(vp)]),
        "scc_dataset_create_csr": (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, i32, P(vp)]),
        "scc_dataset_create_dense": (ctypes.c_int, [vp, vp, i64, i64, i32, P(vp)]),
        "scc_dataset_destroy": (None, [vp]),
        "scc_dataset_read_csc": (ctypes.c_int, [vp, vp, vp, vp]),
        "scc_de_run": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), P(vp)]),
        "scc_de_shard_bytes": (i64, [i32, i64]),
        "scc_de_run_shard": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), i64, i64, vp]),
        "scc_de_finish": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), vp, P(vp)]),
        "scc_de_run_shard_records": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), i64, i64, vp, i64, P(i64)]),
        "scc_de_finish_records": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), vp, vp, i32, i64, P(vp)]),
        "scc_de_finish_records_pairs": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), vp, vp, i32, i64, i32, i32, vp]),
        "scc_de_union_first_occ": (ctypes.c_int, [vp, vp, i64, vp, P(i32)]),
        "scc_de_result_counts": (ctypes.c_int, [vp, P(i32), P(i64), P(i32)]),
        "scc_de_result_union": (ctypes.c_int, [vp, vp]),
        "scc_de_result_rows": (ctypes.c_int, [vp] + [vp] * 10),
        "scc_de_result_pair_vectors": (ctypes.c_int, [vp] + [vp] * 5),
        "scc_de_result_log_threshold": (ctypes.c_int, [vp, P(dbl)]),
        "scc_de_result_nodg": (ctypes.c_int, [vp, vp]),
        "scc_de_result_destroy": (None, [vp]),
        "scc_de_markers": (ctypes.c_int, [vp, vp, vp, i32, P(MarkersParams), P(vp)]),
        "scc_de_result_ties": (ctypes.c_int, [vp, vp]),
        "scc_distance": (ctypes.c_int, [vp, vp, vp, i32, i32, i32, vp, i32, i32]),
        "scc_de_distance": (ctypes.c_int, [vp, vp, vp, i32, P(DeParams), i32, i32, vp, i32, i32, P(vp)]),
        "scc_distance_cols": (ctypes.c_int, [vp, vp, vp, i32, i32, i32, i64, i64, vp, i32, i32]),
        "scc_pca_shard_colsum": (ctypes.c_int, [vp, vp, vp, i32, i64, i64, vp]),
        "scc_pca_shard_gram": (ctypes.c_int, [vp, vp, i32, vp]),
        "scc_pca_shard_scores": (ctypes.c_int, [vp, vp, i32, vp]),
        "scc_pca_shard_eigen": (ctypes.c_int, [vp, vp, i32, vp]),
        "scc_pca_shard_project": (ctypes.c_int, [vp, vp, i32, vp]),
        "scc_distance_scores": (ctypes.c_int, [vp, vp, i64, i64, i64, vp, i32, i32]),
        "scc_silhouette": (ctypes.c_int, [vp, i64, vp, vp, i32, vp, vp, P(i32)]),
        "scc_last_pca_scores": (ctypes.c_int, [vp, vp, P(i32)]),
        "scc_hclust_ward_d2": (ctypes.c_int, [vp, i64, vp, vp, vp]),
        "scc_cutree_hybrid": (ctypes.c_int, [vp, vp, i64, vp, i32, i32, vp, P(dbl)]),
        "scc_hclust_ward_d2_dev": (ctypes.c_int, [vp, i64, vp, i32, vp, vp, vp]),
        "scc_cutree_hybrid_dev": (ctypes.c_int, [vp, vp, vp, i64, vp, i32, i32, i32, vp, P(dbl)]),
        "scc_pca_scores": (ctypes.c_int, [vp, vp, vp, i32, i32]),
        "scc_hclust_ward_d2_scores": (ctypes.c_int, [vp, i64, vp, vp, vp, vp]),
        "scc_cutree_hybrid_scores": (ctypes.c_int, [vp, vp, vp, i64, vp, i32, i32, vp, P(dbl)]),
        "scc_silhouette_scores": (ctypes.c_int, [vp, i64, vp, vp, vp, vp, P(i32)]),
        "scc_knn_scores": (ctypes.c_int, [vp, i64, vp, i32, i32, vp, vp]),
        "scc_umap_graph": (ctypes.c_int, [vp, i64, i32, vp, vp, P(UmapParams), vp, vp, vp, i64, P(i64), vp, vp, vp]),
        "scc_umap_layout": (ctypes.c_int, [vp, i64, vp, vp, vp, vp, P(UmapParams), vp]),
        "scc_umap_scores": (ctypes.c_int, [vp, i64, vp, i32, i32, P(UmapParams), vp, vp, vp, vp, vp, i64, P(i64)]),
        "scc_snn_graph": (ctypes.c_int, [vp, i64, i32, vp, dbl, vp, vp, vp, vp, i64, P(i64)]),
        "scc_modularity_cluster": (ctypes.c_int, [vp, i64, vp, vp, vp, dbl, vp, P(i32), P(dbl), P(i32), vp]),
        "scc_snn_clusters_scores": (ctypes.c_int, [vp, i64, vp, i32, i32, dbl, dbl, vp, P(i32), P(dbl), P(i32), vp, vp,
                                                   vp, vp, i64, P(i64)]),
        "scc_gene_distance": (ctypes.c_int, [vp, vp, vp, i32, vp, vp, vp]),
        "scc_hclust_complete": (ctypes.c_int, [vp, i64, vp, vp, vp]),
        "scc_dendro_reorder": (ctypes.c_int, [vp, i64, vp, vp, vp]),
        "scc_heatmap_raster": (ctypes.c_int, [vp, vp, vp, i32, vp, vp, i32, vp]),
        "scc_diag_hclust_last_scans": (i64, [vp]),
        "scc_diag_eigen_topk": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, P(ctypes.c_int)]),
        "scc_diag_small_syev": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, vp]),
        "scc_diag_cholinv": (ctypes.c_int, [vp, i32, dbl, vp, vp]),
        "scc_diag_eig_last_path": (ctypes.c_int, []),
        "scc_diag_ingest_last_path": (ctypes.c_int, []),
        "scc_diag_rank_last_route": (ctypes.c_int, []),
        "scc_diag_rank_last_runs": (ctypes.c_int, []),
        "scc_diag_mirror_last_uses": (ctypes.c_int, []),
        "scc_diag_small_syev_stamps": (ctypes.c_int, [vp]),
        "scc_diag_pvalues": (ctypes.c_int, [i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@dataclass
class FastRows:
    pair_tested: np.ndarray
    row_pair: np.ndarray
    gene: np.ndarray
    p: np.ndarray
    q: np.ndarray
    avg_logfc: np.ndarray
    pct1: np.ndarray
    pct2: np.ndarray
    u2: np.ndarray
    ties: np.ndarray
    de: np.ndarray
    top: np.ndarray


@dataclass
class DeResult:
    mode: int
    K: int
    n_pairs: int
    union: np.ndarray
    nodg: np.ndarray
    rows: FastRows | None = None       # FAST
    p: np.ndarray | None = None        # [P, G]
    q: np.ndarray | None = None        # SLOW [P, G]
    logfc: np.ndarray | None = None    # [P, G]
    u2: np.ndarray | None = None       # [P, G]
    de: np.ndarray | None = None       # SLOW [P, G]
    ties: np.ndarray | None = None     # [K, G] (de_markers, fetch="all")
    log_thr: float = 0.0
    status: int = 0
    message: str = ""


class Dataset:
    def __init__(self, engine, handle, G, N):
        self.engine, self.handle, self.G, self.N = engine, handle, G, N
        _live_datasets.add(self)

    def close(self):
        if self.handle and not _shutdown:
            self.engine.lib.scc_dataset_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    n = ctypes.c_int32()
    load().scc_device_count(ctypes.byref(n))
    return n.value


class Engine:
    """One MI355X device (``device`` = HIP ordinal), or ONE job over a device
    list (``devices``: HIP ordinals, devices[0] the primary; scc_opts.devices)."""

    def __init__(self, device: int = 0, profile: bool = False, devices=None):
        self.lib = load()
        h = ctypes.c_void_p()
        o = Opts(device, 1 if profile else 0)
        if devices is not None and len(devices) > 1:
            self._devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
            o.n_devices = len(devices)
            o.devices = self._devs
        rc = self.lib.scc_ctx_create(ctypes.byref(o), ctypes.byref(h))
        if rc != SCC_OK:
            raise SccError(rc, "scc_ctx_create failed (no HIP device?)")
        self.ctx = h
        _live_engines.add(self)

    def close(self):
        if self.ctx and not _shutdown:
            for d in list(_live_datasets):
                if d.engine is self:
                    d.close()
            self.lib.scc_ctx_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SCC_OK:
            raise SccError(rc, self.lib.scc_ctx_last_error(self.ctx).decode())

    # -------------------------------------------------------------- datasets
    def dataset_csc(self, indptr, rows, vals, G, N) -> Dataset:
        indptr = np.ascontiguousarray(indptr, np.int64)
        rows = np.ascontiguousarray(rows, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        h = ctypes.c_void_p()
        self._check(self.lib.scc_dataset_create_csc(self.ctx, _ptr(indptr), _ptr(rows), _ptr(vals), G, N, len(vals),
                                                    SCC_PTR_HOST, ctypes.byref(h)))
        return Dataset(self, h, G, N)

    def dataset_csc_device(self, indptr_ptr, rows_ptr, vals_ptr, G, N, nnz) -> Dataset:
        h = ctypes.c_void_p()
        self._check(self.lib.scc_dataset_create_csc(self.ctx, ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(rows_ptr),
                                                    ctypes.c_void_p(vals_ptr), G, N, nnz, SCC_PTR_DEVICE,
                                                    ctypes.byref(h)))
        return Dataset(self, h, G, N)

    def dataset_csr(self, indptr, cols, vals, G, N) -> Dataset:
        """Gene-major CSR (genes x cells: indptr[G+1], cell columns, values),
        transposed on the device into the resident dgCMatrix layout."""
        indptr = np.ascontiguousarray(indptr, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        h = ctypes.c_void_p()
        self._check(self.lib.scc_dataset_create_csr(self.ctx, _ptr(indptr), _ptr(cols), _ptr(vals), G, N, len(vals),
                                                    SCC_PTR_HOST, ctypes.byref(h)))
        return Dataset(self, h, G, N)

    def dataset_csr_device(self, indptr_ptr, cols_ptr, vals_ptr, G, N, nnz) -> Dataset:
        h = ctypes.c_void_p()
        self._check(self.lib.scc_dataset_create_csr(self.ctx, ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(cols_ptr),
                                                    ctypes.c_void_p(vals_ptr), G, N, nnz, SCC_PTR_DEVICE,
                                                    ctypes.byref(h)))
        return Dataset(self, h, G, N)

    def read_csc(self, ds: Dataset):
        """The dataset's resident dgCMatrix (indptr, rows, vals) on the host."""
        indptr = np.empty(ds.N + 1, np.int64)
        self._check(self.lib.scc_dataset_read_csc(ds.handle, _ptr(indptr), None, None))
        nnz = int(indptr[-1])
        rows = np.empty(max(nnz, 1), np.int32)
        vals = np.empty(max(nnz, 1), np.float64)
        self._check(self.lib.scc_dataset_read_csc(ds.handle, _ptr(indptr), _ptr(rows), _ptr(vals)))
        return indptr, rows[:nnz], vals[:nnz]

    def dataset_dense(self, X_gene_major) -> Dataset:
        """X as a genes x cells array; passed to the engine in R's column-major layout."""
        X = np.asarray(X_gene_major, np.float64)
        G, N = X.shape
        col = np.ascontiguousarray(X.T)  # N x G row-major == G x N column-major
        h = ctypes.c_void_p()
        self._check(self.lib.scc_dataset_create_dense(self.ctx, _ptr(col), G, N, SCC_PTR_HOST, ctypes.byref(h)))
        return Dataset(self, h, G, N)

    # -------------------------------------------------------------- DE
    def de_run(self, ds: Dataset, code, K, mode=SCC_DE_FAST, q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0,
               top_n=30, fc_thrs=1.5, mean_scaling_factor=5.0, fetch="all", test_all=None, test="wilcox") -> DeResult:
        """test_all (FAST): also compute U / p for the (pair, gene) cells the
        feature filters drop; default: only when the full per-pair vectors are
        fetched (fetch="all")."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor,
                              fetch == "all" if test_all is None else test_all, test)
        r = ctypes.c_void_p()
        rc = self.lib.scc_de_run(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm), ctypes.byref(r))
        return self._collect(r, rc, ds, mode, K, fetch)

    def de_markers(self, ds: Dataset, code, K, q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30,
                   only_pos=False, fetch="rows", test_all=None, test="wilcox") -> DeResult:
        """One-vs-rest marker genes (scc_de_markers): cluster a against every
        other kept cell, for all K clusters in one engine pass.  The result has
        the K clusters in the place of pairs: ``rows`` is cluster-major
        (``pair_tested[a]`` rows of cluster a; pct1 the cluster, pct2 the rest).
        fetch="all" adds the dense [K, G] ``p``, ``logfc``, ``u2`` and ``ties``;
        test_all (default: with fetch="all") computes them for the cells the
        feature filters drop too."""
        if test not in _TEST_CODES:
            raise ValueError(f"test must be 'wilcox', 't' or 'bimod', not {test!r}")
        code = np.ascontiguousarray(code, np.int32)
        prm = MarkersParams(top_n, 1 if only_pos else 0, _TEST_CODES[test],
                            1 if (fetch == "all" if test_all is None else test_all) else 0, q_val_thrs, log_fc_thrs,
                            min_per_cent)
        r = ctypes.c_void_p()
        rc = self.lib.scc_de_markers(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm), ctypes.byref(r))
        return self._collect(r, rc, ds, SCC_DE_FAST, K, fetch, ties=True)

    @staticmethod
    def _de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor, test_all,
                   test="wilcox"):
        if test not in _TEST_CODES:
            raise ValueError(f"test must be 'wilcox', 't' or 'bimod', not {test!r}")
        return DeParams(mode, top_n, q_val_thrs, log_fc_thrs, min_per_cent, fc_thrs, mean_scaling_factor,
                        1 if test_all else 0, _TEST_CODES[test])

    def de_shard_bytes(self, K, G) -> int:
        return int(self.lib.scc_de_shard_bytes(K, G))

    def de_run_shard(self, ds: Dataset, code, K, gene_lo, gene_hi, shard_ptr, mode=SCC_DE_FAST, q_val_thrs=0.1,
                     log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, fc_thrs=1.5, mean_scaling_factor=5.0,
                     test_all=False, test="wilcox"):
        """Per-(pair, gene) DE cells of genes [gene_lo, gene_hi) into the device
        buffer at shard_ptr (de_shard_bytes(K, G) bytes, zero outside the shard)."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor,
                              test_all, test)
        self._check(self.lib.scc_de_run_shard(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm), gene_lo,
                                              gene_hi, ctypes.c_void_p(shard_ptr)))

    def de_finish(self, ds: Dataset, code, K, shards_sum_ptr, mode=SCC_DE_FAST, q_val_thrs=0.1, log_fc_thrs=0.5,
                  min_per_cent=20.0, top_n=30, fc_thrs=1.5, mean_scaling_factor=5.0, fetch="all",
                  test_all=False, test="wilcox") -> DeResult:
        """Selection and union from the summed shards of every rank (device)."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor,
                              test_all, test)
        r = ctypes.c_void_p()
        rc = self.lib.scc_de_finish(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm),
                                    ctypes.c_void_p(shards_sum_ptr), ctypes.byref(r))
        return self._collect(r, rc, ds, mode, K, fetch)

    REC_BYTES = 64  # sizeof(scc_de_record)

    def de_run_shard_records(self, ds: Dataset, code, K, gene_lo, gene_hi, rec_ptr, cap, mode=SCC_DE_FAST,
                             q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, fc_thrs=1.5,
                             mean_scaling_factor=5.0, test_all=False, test="wilcox") -> int:
        """Compact records (scc_de_record, 64 B) of the tested (pair, gene)
        cells of genes [gene_lo, gene_hi) into the device buffer at rec_ptr
        (capacity ``cap`` records); returns their number."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor,
                              test_all, test)
        n = ctypes.c_int64()
        self._check(self.lib.scc_de_run_shard_records(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm), gene_lo,
                                                      gene_hi, ctypes.c_void_p(rec_ptr), cap, ctypes.byref(n)))
        return n.value

    def de_finish_records(self, ds: Dataset, code, K, rec_ptr, counts, stride, mode=SCC_DE_FAST, q_val_thrs=0.1,
                          log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, fc_thrs=1.5, mean_scaling_factor=5.0,
                          fetch="all", test_all=False, test="wilcox") -> DeResult:
        """Selection and union from the gathered records of every rank (device
        blocks ``stride`` records apart, ``counts[r]`` valid in block r)."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(mode, q_val_thrs, log_fc_thrs, min_per_cent, top_n, fc_thrs, mean_scaling_factor,
                              test_all, test)
        cnt = np.ascontiguousarray(counts, np.int64)
        r = ctypes.c_void_p()
        rc = self.lib.scc_de_finish_records(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm),
                                            ctypes.c_void_p(rec_ptr or None), _ptr(cnt), len(cnt), int(stride),
                                            ctypes.byref(r))
        return self._collect(r, rc, ds, mode, K, fetch)

    def de_finish_records_pairs(self, ds: Dataset, code, K, rec_ptr, counts, stride, pair_lo, pair_hi, first_ptr,
                                q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, test_all=False,
                                test="wilcox", **_):
        """FAST selection of the pairs [pair_lo, pair_hi) from the gathered
        records; the genes' first-occurrence keys go to ``first_ptr`` (device
        uint64 [G]; combine the ranks' arrays by MIN, then de_union_first_occ)."""
        code = np.ascontiguousarray(code, np.int32)
        prm = self._de_params(SCC_DE_FAST, q_val_thrs, log_fc_thrs, min_per_cent, top_n, 1.5, 5.0, test_all, test)
        cnt = np.ascontiguousarray(counts, np.int64)
        self._check(self.lib.scc_de_finish_records_pairs(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm),
                                                         ctypes.c_void_p(rec_ptr or None), _ptr(cnt), len(cnt),
                                                         int(stride), int(pair_lo), int(pair_hi),
                                                         ctypes.c_void_p(first_ptr)))

    def de_union_first_occ(self, first_ptr, G):
        """deGeneUnion (reference order) from a combined first-occurrence array."""
        out = np.zeros(G, np.int32)
        nu = ctypes.c_int32()
        self._check(self.lib.scc_de_union_first_occ(self.ctx, ctypes.c_void_p(first_ptr), G, _ptr(out),
                                                    ctypes.byref(nu)))
        return out[: nu.value].copy()

    def _collect(self, r, rc, ds, mode, K, fetch, ties=False) -> DeResult:
        msg = ""
        if rc != SCC_OK:
            msg = self.lib.scc_ctx_last_error(self.ctx).decode()
            if not r.value:
                raise SccError(rc, msg)
        try:
            npairs, nrows, nu = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()
            self._check(self.lib.scc_de_result_counts(r, ctypes.byref(npairs), ctypes.byref(nrows), ctypes.byref(nu)))
            uni = np.zeros(nu.value, np.int32)
            self._check(self.lib.scc_de_result_union(r, _ptr(uni)))
            out = DeResult(mode, K, npairs.value, uni, np.zeros(0, np.int32), status=rc, message=msg)
            if fetch == "union":
                return out
            nodg = np.zeros(ds.N, np.int32)
            self._check(self.lib.scc_de_result_nodg(r, _ptr(nodg)))
            out.nodg = nodg
            if fetch == "nodg":  # what the R glue's C_scc_de_fast returns: the union and nodg
                return out
            P, G = npairs.value, ds.G
            if mode == SCC_DE_FAST:
                n = nrows.value
                tested = np.zeros(P, np.int32)
                a = dict(gene=np.zeros(n, np.int32), p=np.zeros(n), q=np.zeros(n), lfc=np.zeros(n),
                         pct1=np.zeros(n), pct2=np.zeros(n), u2=np.zeros(n, np.int64), t=np.zeros(n, np.int64),
                         fl=np.zeros(n, np.uint8))
                self._check(self.lib.scc_de_result_rows(r, _ptr(tested), _ptr(a["gene"]), _ptr(a["p"]), _ptr(a["q"]),
                                                        _ptr(a["lfc"]), _ptr(a["pct1"]), _ptr(a["pct2"]),
                                                        _ptr(a["u2"]), _ptr(a["t"]), _ptr(a["fl"])))
                out.rows = FastRows(tested, np.repeat(np.arange(P, dtype=np.int32), tested), a["gene"], a["p"],
                                    a["q"], a["lfc"], a["pct1"], a["pct2"], a["u2"], a["t"], (a["fl"] & 1) > 0,
                                    (a["fl"] & 2) > 0)
                if fetch == "all":
                    pv, lf, u2 = np.zeros((P, G)), np.zeros((P, G)), np.zeros((P, G), np.int64)
                    self._check(self.lib.scc_de_result_pair_vectors(r, _ptr(pv), None, _ptr(lf), _ptr(u2), None))
                    out.p, out.logfc, out.u2 = pv, lf, u2
                    if ties:
                        out.ties = np.zeros((P, G), np.int64)
                        self._check(self.lib.scc_de_result_ties(r, _ptr(out.ties)))
            else:
                pv, qv, lf = np.zeros((P, G)), np.zeros((P, G)), np.zeros((P, G))
                u2, de = np.zeros((P, G), np.int64), np.zeros((P, G), np.uint8)
                self._check(self.lib.scc_de_result_pair_vectors(r, _ptr(pv), _ptr(qv), _ptr(lf), _ptr(u2), _ptr(de)))
                out.p, out.q, out.logfc, out.u2, out.de = pv, qv, lf, u2, de
                lt = ctypes.c_double()
                self._check(self.lib.scc_de_result_log_threshold(r, ctypes.byref(lt)))
                out.log_thr = lt.value
            return out
        finally:
            self.lib.scc_de_result_destroy(r)

    # -------------------------------------------------------------- distance
    def distance(self, ds: Dataset, genes, metric=SCC_DIST_PCA_EUCLID, ncomp=0, out=None, f32=False,
                 device_out_ptr=None):
        genes = np.ascontiguousarray(genes, np.int32)
        N = ds.N
        npairs = N * (N - 1) // 2
        if device_out_ptr is not None:  # 0 -> engine-owned HBM-resident output
            self._check(self.lib.scc_distance(self.ctx, ds.handle, _ptr(genes), len(genes), metric, ncomp,
                                              ctypes.c_void_p(device_out_ptr or None), SCC_PTR_DEVICE,
                                              1 if f32 else 0))
            return None
        if out is None:
            out = np.empty(npairs, np.float32 if f32 else np.float64)
        self._check(self.lib.scc_distance(self.ctx, ds.handle, _ptr(genes), len(genes), metric, ncomp, _ptr(out),
                                          SCC_PTR_HOST, 1 if f32 else 0))
        return out

    def de_distance(self, ds: Dataset, code, K, mode=SCC_DE_FAST, metric=SCC_DIST_PCA_EUCLID, ncomp=0, out=None,
                    f32=False, device_out_ptr=None, fetch="union", **de_kw):
        """scc_de_distance: the DE, then the distance over its union, in one
        C call.  Returns (DeResult, distance) — the distance None for device
        output (device_out_ptr; 0 keeps it in the engine)."""
        code = np.ascontiguousarray(code, np.int32)
        kw = dict(q_val_thrs=0.1, log_fc_thrs=0.5, min_per_cent=20.0, top_n=30, fc_thrs=1.5, mean_scaling_factor=5.0,
                  test_all=None, test="wilcox")
        unknown = set(de_kw) - set(kw)
        if unknown:
            raise TypeError(f"de_distance: unknown DE arguments {sorted(unknown)}")
        kw.update(de_kw)
        prm = self._de_params(mode, kw["q_val_thrs"], kw["log_fc_thrs"], kw["min_per_cent"], kw["top_n"],
                              kw["fc_thrs"], kw["mean_scaling_factor"],
                              fetch == "all" if kw["test_all"] is None else kw["test_all"], kw["test"])
        r = ctypes.c_void_p()
        if device_out_ptr is not None:
            dst, kind, res = ctypes.c_void_p(device_out_ptr or None), SCC_PTR_DEVICE, None
        else:
            res = out if out is not None else np.empty(ds.N * (ds.N - 1) // 2, np.float32 if f32 else np.float64)
            dst, kind = _ptr(res), SCC_PTR_HOST
        rc = self.lib.scc_de_distance(self.ctx, ds.handle, _ptr(code), K, ctypes.byref(prm), metric, ncomp, dst, kind,
                                      1 if f32 else 0, ctypes.byref(r))
        if rc != SCC_OK and r.value:  # the DE succeeded, the distance failed: free the result, raise
            self.lib.scc_de_result_destroy(r)
            self._check(rc)
        de = self._collect(r, rc, ds, mode, K, fetch)
        return de, res

    def distance_cols(self, ds: Dataset, genes, col_lo, col_hi, metric=SCC_DIST_PCA_EUCLID, ncomp=0, out=None,
                      f32=False, device_out_ptr=None):
        """Columns [col_lo, col_hi) of the packed distance vector (a contiguous slice)."""
        genes = np.ascontiguousarray(genes, np.int32)
        N = ds.N
        n = col_hi * (2 * N - col_hi - 1) // 2 - col_lo * (2 * N - col_lo - 1) // 2
        if device_out_ptr is not None:
            self._check(self.lib.scc_distance_cols(self.ctx, ds.handle, _ptr(genes), len(genes), metric, ncomp, col_lo,
                                                   col_hi, ctypes.c_void_p(device_out_ptr or None), SCC_PTR_DEVICE,
                                                   1 if f32 else 0))
            return None
        if out is None:
            out = np.empty(n, np.float32 if f32 else np.float64)
        self._check(self.lib.scc_distance_cols(self.ctx, ds.handle, _ptr(genes), len(genes), metric, ncomp, col_lo,
                                               col_hi, _ptr(out), SCC_PTR_HOST, 1 if f32 else 0))
        return out

    # ---------------------------------------------------------- sharded PCA
    def pca_shard_colsum(self, ds: Dataset, genes, cell_lo, cell_hi, part_ptr):
        genes = np.ascontiguousarray(genes, np.int32)
        self._check(self.lib.scc_pca_shard_colsum(self.ctx, ds.handle, _ptr(genes), len(genes), cell_lo, cell_hi,
                                                  ctypes.c_void_p(part_ptr)))

    def pca_shard_gram(self, parts_ptr, world, gram_ptr):
        self._check(self.lib.scc_pca_shard_gram(self.ctx, ctypes.c_void_p(parts_ptr), world, ctypes.c_void_p(gram_ptr)))

    def pca_shard_scores(self, gram_ptr, scores_ptr, ncomp=0):
        self._check(self.lib.scc_pca_shard_scores(self.ctx, ctypes.c_void_p(gram_ptr), ncomp,
                                                  ctypes.c_void_p(scores_ptr)))

    def pca_shard_eigen(self, gram_ptr, vecs_ptr, ncomp=0):
        self._check(self.lib.scc_pca_shard_eigen(self.ctx, ctypes.c_void_p(gram_ptr), ncomp, ctypes.c_void_p(vecs_ptr)))

    def pca_shard_project(self, vecs_ptr, scores_ptr, ncomp=0):
        self._check(self.lib.scc_pca_shard_project(self.ctx, ctypes.c_void_p(vecs_ptr), ncomp,
                                                   ctypes.c_void_p(scores_ptr)))

    def distance_scores(self, scores_ptr, N, col_lo, col_hi, out=None, f32=False, device_out_ptr=None):
        """Packed `dist` columns [col_lo, col_hi) from a device [N][16] score matrix."""
        n = col_hi * (2 * N - col_hi - 1) // 2 - col_lo * (2 * N - col_lo - 1) // 2
        if device_out_ptr is not None:
            self._check(self.lib.scc_distance_scores(self.ctx, ctypes.c_void_p(scores_ptr), N, col_lo, col_hi,
                                                     ctypes.c_void_p(device_out_ptr or None), SCC_PTR_DEVICE,
                                                     1 if f32 else 0))
            return None
        if out is None:
            out = np.empty(n, np.float32 if f32 else np.float64)
        self._check(self.lib.scc_distance_scores(self.ctx, ctypes.c_void_p(scores_ptr), N, col_lo, col_hi, _ptr(out),
                                                 SCC_PTR_HOST, 1 if f32 else 0))
        return out

    def silhouette(self, N, groups, dist_device_ptr=None, f32=False):
        """(widths [N], per-cluster average widths in sorted group order) of
        cluster::silhouette(groups, as.matrix(d)); d = the engine-kept output
        of the last full distance() call unless a device pointer is given."""
        groups = np.ascontiguousarray(groups, np.int32)
        C = len(np.unique(groups))
        w, ca, k = np.zeros(N), np.zeros(max(C, 1)), ctypes.c_int32()
        self._check(self.lib.scc_silhouette(self.ctx, N, _ptr(groups), ctypes.c_void_p(dist_device_ptr or None),
                                            1 if f32 else 0, _ptr(w), _ptr(ca), ctypes.byref(k)))
        return w, ca[:k.value]

    def hclust_ward_d2_dev(self, N, dist_device_ptr=None, f32=False):
        """hclust_ward_d2 on a device-resident packed distance (the engine-kept
        output of the last full distance() call unless a device pointer is
        given): the same (merge, height, order), bit for bit, and the packed
        vector never leaves the device."""
        N = int(N)
        if N < 2:
            raise ValueError("hclust_ward_d2_dev needs at least two observations")
        merge = np.zeros(2 * (N - 1), np.int32)
        height = np.zeros(N - 1)
        order = np.zeros(N, np.int32)
        self._check(self.lib.scc_hclust_ward_d2_dev(self.ctx, N, ctypes.c_void_p(dist_device_ptr or None),
                                                    1 if f32 else 0, _ptr(merge), _ptr(height), _ptr(order)))
        return merge.reshape(2, N - 1).T.copy(), height, order

    def cutree_hybrid_dev(self, merge, height, deep_split, min_cluster_size, dist_device_ptr=None, f32=False):
        """cutree_hybrid with distM read from a device-resident packed distance
        (same rule as hclust_ward_d2_dev): (labels, cut height)."""
        merge = np.asarray(merge)
        n = merge.shape[0] + 1
        m = np.ascontiguousarray(merge.T.reshape(-1), np.int32)
        h = np.ascontiguousarray(height, np.float64)
        if h.shape != (n - 1,):
            raise ValueError("shape mismatch between merge and height")
        lab = np.zeros(n, np.int32)
        cut = ctypes.c_double()
        self._check(self.lib.scc_cutree_hybrid_dev(self.ctx, _ptr(m), _ptr(h), n,
                                                   ctypes.c_void_p(dist_device_ptr or None), 1 if f32 else 0,
                                                   int(deep_split), int(min_cluster_size), _ptr(lab),
                                                   ctypes.byref(cut)))
        return lab, cut.value

    def pca_scores(self, ds: Dataset, genes, ncomp=0):
        """The PCA half of distance(): the [N][16] scores stay in the engine
        (last_pca_scores reads them), no distance is computed or kept."""
        genes = np.ascontiguousarray(genes, np.int32)
        self._check(self.lib.scc_pca_scores(self.ctx, ds.handle, _ptr(genes), len(genes), ncomp))

    def hclust_ward_d2_scores(self, N, scores_device_ptr=None):
        """hclust(dist(scores), "ward.D2") from a device [N][16] score matrix
        (the engine-kept scores unless a device pointer is given), without
        the N x N matrix: (merge, height, order) as hclust_ward_d2.  The tree
        of the matrix routes whenever no two candidate dissimilarities lie
        within rounding of each other; on exact ties a valid Ward tree that
        may resolve the tie differently."""
        N = int(N)
        if N < 2:
            raise ValueError("hclust_ward_d2_scores needs at least two observations")
        merge = np.zeros(2 * (N - 1), np.int32)
        height = np.zeros(N - 1)
        order = np.zeros(N, np.int32)
        self._check(self.lib.scc_hclust_ward_d2_scores(self.ctx, N, ctypes.c_void_p(scores_device_ptr or None),
                                                       _ptr(merge), _ptr(height), _ptr(order)))
        return merge.reshape(2, N - 1).T.copy(), height, order

    def cutree_hybrid_scores(self, merge, height, deep_split, min_cluster_size, scores_device_ptr=None):
        """cutree_hybrid with distM computed from a device [N][16] score matrix
        (same rule as hclust_ward_d2_scores): (labels, cut height)."""
        merge = np.asarray(merge)
        n = merge.shape[0] + 1
        m = np.ascontiguousarray(merge.T.reshape(-1), np.int32)
        h = np.ascontiguousarray(height, np.float64)
        if h.shape != (n - 1,):
            raise ValueError("shape mismatch between merge and height")
        lab = np.zeros(n, np.int32)
        cut = ctypes.c_double()
        self._check(self.lib.scc_cutree_hybrid_scores(self.ctx, _ptr(m), _ptr(h), n,
                                                      ctypes.c_void_p(scores_device_ptr or None), int(deep_split),
                                                      int(min_cluster_size), _ptr(lab), ctypes.byref(cut)))
        return lab, cut.value

    def silhouette_scores(self, N, groups, scores_device_ptr=None):
        """silhouette() for d = dist(scores) of a device [N][16] score matrix
        (same rule as hclust_ward_d2_scores), without the N x N matrix:
        (widths, per-cluster average widths), bit for bit what silhouette()
        returns on the f64 distance of the same scores."""
        N = int(N)
        groups = np.ascontiguousarray(groups, np.int32)
        if groups.shape != (N,):
            raise ValueError("groups must hold one id per cell")
        C = len(np.unique(groups))
        w, ca, k = np.zeros(N), np.zeros(max(C, 1)), ctypes.c_int32()
        self._check(self.lib.scc_silhouette_scores(self.ctx, N, _ptr(groups),
                                                   ctypes.c_void_p(scores_device_ptr or None), _ptr(w), _ptr(ca),
                                                   ctypes.byref(k)))
        return w, ca[:k.value]

    def knn_scores(self, N, k, dims=0, scores_device_ptr=None):
        """The exact k nearest neighbours of every cell under dist(scores) of a
        device [N][16] score matrix (same rule as hclust_ward_d2_scores),
        without the N x N matrix: (idx int32 [N, k] 0-based, dist float64
        [N, k]), each row ordered by (distance, index), the cell itself left
        out; the distances are bit for bit entries of distance_scores.  Only
        the first `dims` components enter (0: all 15)."""
        N, k = int(N), int(k)
        idx = np.empty((N, max(k, 1)), np.int32)
        dist = np.empty((N, max(k, 1)))
        self._check(self.lib.scc_knn_scores(self.ctx, N, ctypes.c_void_p(scores_device_ptr or None), int(dims), k,
                                            _ptr(idx), _ptr(dist)))
        return idx, dist

    # -------------------------------------------------------------- UMAP
    def umap_graph(self, idx, dist, set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0,
                   return_rho_sigma=False):
        """The fuzzy simplicial set of a k-NN table in knn_scores' output form
        (n_neighbors = k + 1: the cell counts as its own first neighbour):
        the symmetric CSR (indptr int64 [N + 1], cols int32, vals float64),
        columns ascending within a row; with return_rho_sigma also the rows'
        rho and sigma and the directed weights [N, k]."""
        idx = np.ascontiguousarray(idx, np.int32)
        dist = np.ascontiguousarray(dist, np.float64)
        if idx.ndim != 2 or idx.shape != dist.shape:
            raise ValueError("idx and dist must be [N, k] arrays of one shape")
        N, k = idx.shape
        cap = max(2 * N * k, 1)
        indptr, cols, vals = np.zeros(N + 1, np.int64), np.empty(cap, np.int32), np.empty(cap)
        rho, sigma, w = np.empty(max(N, 1)), np.empty(max(N, 1)), np.empty((max(N, 1), max(k, 1)))
        nnz = ctypes.c_int64()
        prm = _umap_params(set_op_mix_ratio, local_connectivity, bandwidth)
        self._check(self.lib.scc_umap_graph(self.ctx, N, k, _ptr(idx), _ptr(dist), ctypes.byref(prm), _ptr(indptr),
                                            _ptr(cols), _ptr(vals), cap, ctypes.byref(nnz), _ptr(rho), _ptr(sigma),
                                            _ptr(w)))
        g = (indptr, cols[:nnz.value].copy(), vals[:nnz.value].copy())
        return g + (rho[:N], sigma[:N], w[:N, :k]) if return_rho_sigma else g

    def umap_layout(self, indptr, cols, vals, init, n_epochs=200, a=0.0, b=0.0, gamma=1.0, negative_sample_rate=5,
                    learning_rate=1.0, seed=0):
        """The stochastic-gradient layout of a symmetric weighted CSR graph
        from init [N, 2]: float64 [N, 2].  a = b = 0: the constants fitted for
        min_dist = 0.1, spread = 1.  Two calls return the same bits."""
        indptr = np.ascontiguousarray(indptr, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        init = np.ascontiguousarray(init, np.float64)
        N = len(indptr) - 1
        if N < 1 or init.shape != (N, 2) or cols.shape != vals.shape or cols.ndim != 1:
            raise ValueError("umap_layout: indptr [N + 1], cols and vals of one length, init [N, 2]")
        if len(cols) < indptr[-1]:
            raise ValueError("umap_layout: cols and vals are shorter than indptr[-1]")
        Y = np.empty((N, 2))
        prm = _umap_params(1.0, 1.0, 1.0, n_epochs, a, b, gamma, negative_sample_rate, learning_rate, seed)
        self._check(self.lib.scc_umap_layout(self.ctx, N, _ptr(indptr), _ptr(cols), _ptr(vals), _ptr(init),
                                             ctypes.byref(prm), _ptr(Y)))
        return Y

    def umap_scores(self, N, n_neighbors=15, dims=0, scores_device_ptr=None, init=None, n_epochs=200, a=0.0, b=0.0,
                    gamma=1.0, negative_sample_rate=5, learning_rate=1.0, seed=0, set_op_mix_ratio=1.0,
                    local_connectivity=1.0, bandwidth=1.0, return_graph=False):
        """knn_scores (k = n_neighbors - 1), umap_graph and umap_layout in one
        call on a device [N][16] score matrix (same rule as knn_scores), the
        table and the graph staying on the device: the layout float64 [N, 2],
        bit for bit what the three calls give; with return_graph also the CSR
        triple.  init None: the first two score columns scaled so that the
        largest absolute coordinate is 10."""
        N, nn = int(N), int(n_neighbors)
        if init is not None:
            init = np.ascontiguousarray(init, np.float64)
            if init.shape != (N, 2):
                raise ValueError("init must be [N, 2]")
        Y = np.empty((max(N, 1), 2))
        prm = _umap_params(set_op_mix_ratio, local_connectivity, bandwidth, n_epochs, a, b, gamma,
                           negative_sample_rate, learning_rate, seed)
        nnz = ctypes.c_int64()
        indptr = cols = vals = None
        cap = 0
        if return_graph:
            cap = max(2 * N * max(nn - 1, 0), 1)
            indptr, cols, vals = np.zeros(max(N, 0) + 1, np.int64), np.empty(cap, np.int32), np.empty(cap)
        self._check(self.lib.scc_umap_scores(self.ctx, N, ctypes.c_void_p(scores_device_ptr or None), int(dims), nn,
                                             ctypes.byref(prm), _ptr(init), _ptr(Y), _ptr(indptr), _ptr(cols),
                                             _ptr(vals), cap, ctypes.byref(nnz)))
        if return_graph:
            return Y, (indptr, cols[:nnz.value].copy(), vals[:nnz.value].copy())
        return Y

    # -------------------------------------------------------------- SNN graph and clustering
    def snn_graph(self, idx, prune=1.0 / 15.0, return_shared=False, cap=None):
        """The shared-nearest-neighbour graph of a k-NN table in knn_scores'
        output form (Seurat's ComputeSNN rule, k.param = k + 1, the diagonal
        not stored): the symmetric CSR (indptr int64 [N + 1], cols int32, vals
        float64), columns ascending within a row; with return_shared also the
        shared counts (int32, parallel to vals).  The entries have no bound
        such as 2 N k: a first call that finds its buffers too small is
        repeated with the size it reported (cap given: one call with buffers
        of cap entries, refused when they are too small)."""
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.ndim != 2:
            raise ValueError("idx must be an [N, k] array")
        N, k = idx.shape
        indptr = np.zeros(N + 1, np.int64)
        nnz = ctypes.c_int64()
        retry = cap is None
        cap = max(4 * N * (k + 1), 1) if retry else max(int(cap), 1)
        while True:
            cols, vals, shared = np.empty(cap, np.int32), np.empty(cap), np.empty(cap, np.int32)
            rc = self.lib.scc_snn_graph(self.ctx, N, k, _ptr(idx), float(prune), _ptr(indptr), _ptr(cols), _ptr(vals),
                                        _ptr(shared), cap, ctypes.byref(nnz))
            if retry and rc == SCC_ERR_INVALID and nnz.value > cap:
                cap, nnz.value = nnz.value, 0
                continue
            self._check(rc)
            break
        g = (indptr, cols[:nnz.value].copy(), vals[:nnz.value].copy())
        return g + (shared[:nnz.value].copy(),) if return_shared else g

    def modularity_cluster(self, indptr, cols, vals, resolution=1.0):
        """Deterministic multilevel modularity clustering of a symmetric
        weighted CSR graph (snn_graph's or umap_graph's output form): a dict
        of labels (int32 [N], 0 the largest cluster), n_clusters, modularity,
        n_levels and sweeps (the sweeps run in each level)."""
        indptr = np.ascontiguousarray(indptr, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        N = len(indptr) - 1
        if N < 1 or cols.shape != vals.shape or cols.ndim != 1:
            raise ValueError("modularity_cluster: indptr [N + 1], cols and vals of one length")
        if len(cols) < indptr[-1]:
            raise ValueError("modularity_cluster: cols and vals are shorter than indptr[-1]")
        labels = np.empty(N, np.int32)
        nc, nl, q = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        sweeps = np.zeros(MODULARITY_MAX_LEVELS, np.int32)
        self._check(self.lib.scc_modularity_cluster(self.ctx, N, _ptr(indptr), _ptr(cols), _ptr(vals),
                                                    float(resolution), _ptr(labels), ctypes.byref(nc),
                                                    ctypes.byref(q), ctypes.byref(nl), _ptr(sweeps)))
        return {"labels": labels, "n_clusters": nc.value, "modularity": q.value, "n_levels": nl.value,
                "sweeps": sweeps[:nl.value].tolist()}

    def snn_clusters_scores(self, N, k_param=20, dims=0, prune=1.0 / 15.0, resolution=0.8, scores_device_ptr=None,
                            return_graph=False):
        """knn_scores (k = k_param - 1), snn_graph and modularity_cluster in
        one call on a device [N][16] score matrix (same rule as knn_scores),
        the table and the graph staying on the device: modularity_cluster's
        dict, bit for bit what the three calls give; with return_graph also
        "graph", the SNN CSR triple."""
        N, kp = int(N), int(k_param)
        labels = np.empty(max(N, 1), np.int32)
        nc, nl, q = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        sweeps = np.zeros(MODULARITY_MAX_LEVELS, np.int32)
        nnz = ctypes.c_int64()
        indptr = cols = vals = None
        cap = max(4 * N * max(kp, 1), 1) if return_graph else 0
        while True:
            if return_graph:
                indptr, cols, vals = np.zeros(max(N, 0) + 1, np.int64), np.empty(cap, np.int32), np.empty(cap)
            rc = self.lib.scc_snn_clusters_scores(self.ctx, N, ctypes.c_void_p(scores_device_ptr or None), int(dims), kp,
                                                  float(prune), float(resolution), _ptr(labels), ctypes.byref(nc),
                                                  ctypes.byref(q), ctypes.byref(nl), _ptr(sweeps), _ptr(indptr),
                                                  _ptr(cols), _ptr(vals), cap, ctypes.byref(nnz))
            if return_graph and rc == SCC_ERR_INVALID and nnz.value > cap:
                cap, nnz.value = nnz.value, 0
                continue
            self._check(rc)
            break
        out = {"labels": labels[:N], "n_clusters": nc.value, "modularity": q.value, "n_levels": nl.value,
               "sweeps": sweeps[:nl.value].tolist(), "nnz": nnz.value}
        if return_graph:
            out["graph"] = (indptr, cols[:nnz.value].copy(), vals[:nnz.value].copy())
        return out

    # -------------------------------------------------------------- heatmap inputs
    def gene_distance(self, ds: Dataset, genes):
        """dist(X[genes, ], "euclidean") with the genes as observations over
        all cells (packed R `dist` order), rowMeans and {min x, max x,
        min |x|, max |x|} of the block: (dist, row_mean, range)."""
        genes = np.ascontiguousarray(genes, np.int32)
        nu = len(genes)
        d = np.empty(max(nu * (nu - 1) // 2, 1))
        mean, rng = np.empty(max(nu, 1)), np.empty(4)
        self._check(self.lib.scc_gene_distance(self.ctx, ds.handle, _ptr(genes), nu, _ptr(d), _ptr(mean), _ptr(rng)))
        return d[: nu * (nu - 1) // 2], mean[:nu], rng

    def heatmap_raster(self, ds: Dataset, genes, row_order, cell_order, width):
        """The |genes| x width raster: row r is gene genes[row_order[r] - 1],
        column b the mean over the cells cell_order[floor(b N / width) ..
        floor((b + 1) N / width)) (both orders 1-based permutations)."""
        genes = np.ascontiguousarray(genes, np.int32)
        ro = np.ascontiguousarray(row_order, np.int32)
        co = np.ascontiguousarray(cell_order, np.int32)
        if ro.shape != (len(genes),) or co.shape != (ds.N,):
            raise ValueError("row_order must hold one entry per gene and cell_order one per cell")
        width = int(width)
        out = np.empty((len(genes), max(width, 1)))
        self._check(self.lib.scc_heatmap_raster(self.ctx, ds.handle, _ptr(genes), len(genes), _ptr(ro), _ptr(co),
                                                width, _ptr(out)))
        return out

    def hclust_last_scans(self):
        """Nearest-neighbour scans of the last hclust_ward_d2_dev or hclust_ward_d2_scores (diagnostics)."""
        return int(self.lib.scc_diag_hclust_last_scans(self.ctx))

    def last_pca_scores(self, N):
        k = ctypes.c_int32()
        self._check(self.lib.scc_last_pca_scores(self.ctx, None, ctypes.byref(k)))
        s = np.zeros((N, k.value))
        self._check(self.lib.scc_last_pca_scores(self.ctx, _ptr(s), ctypes.byref(k)))
        return s

    # -------------------------------------------------------------- timers
    def kernel_time(self, name):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self.lib.scc_ctx_kernel_time(self.ctx, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def reset_timers(self):
        self.lib.scc_ctx_reset_timers(self.ctx)

    def synchronize(self):
        self._check(self.lib.scc_ctx_synchronize(self.ctx))

    def set_stream(self, stream_handle):
        """Launch on the caller's HIP stream (an int handle, e.g. torch's
        ``torch.cuda.current_stream().cuda_stream``; 0 is the legacy default
        stream); ``None``: back to the engine's own stream."""
        self._check(self.lib.scc_ctx_set_stream(self.ctx, ctypes.c_void_p(stream_handle or None),
                                                0 if stream_handle is None else 1))

    def on_stream(self, stream_handle):
        """Context manager: the engine's work goes on ``stream_handle`` inside."""
        eng = self

        class _On:
            def __enter__(self):
                eng.set_stream(stream_handle)
                return eng

            def __exit__(self, *exc):
                eng.set_stream(None)
                return False
        return _On()


# ---------------------------------------------------------------- diagnostics
DIAG_WILCOX, DIAG_T, DIAG_PNORM, DIAG_PCHISQ3 = 0, 1, 2, 3


def diag_pvalues(kind, a=None, b=None, u2=None, tie=None, m=None, n=None):
    """scc_diag_pvalues: the DE p-value device functions on arrays (tests).
    DIAG_WILCOX (u2, tie, m, n) returns (p, exact_used); DIAG_T (a = t, b = df),
    DIAG_PNORM (a = z) and DIAG_PCHISQ3 (a = x) return p."""
    def arr(v, dt):
        return None if v is None else np.ascontiguousarray(v, dt)
    a, b = arr(a, np.float64), arr(b, np.float64)
    u2, tie, m, n = arr(u2, np.int64), arr(tie, np.int64), arr(m, np.int32), arr(n, np.int32)
    used = (u2, tie, m, n) if kind == DIAG_WILCOX else (a, b) if kind == DIAG_T else (a,)
    if any(v is None for v in used) or len({v.shape for v in used}) != 1 or used[0].ndim != 1:
        raise ValueError("diag_pvalues: the kind's arguments must be 1-d arrays of one length")
    cnt = len(used[0])
    out = np.empty(2 * cnt if kind == DIAG_WILCOX else cnt)
    rc = load().scc_diag_pvalues(int(kind), cnt, _ptr(a), _ptr(b), _ptr(u2), _ptr(tie), _ptr(m), _ptr(n), _ptr(out))
    if rc != 0:
        raise SccError(SCC_ERR_HIP if 0 <= kind <= 3 else SCC_ERR_INVALID, "scc_diag_pvalues failed")
    return (out[:cnt], out[cnt:] != 0) if kind == DIAG_WILCOX else out


# ---------------------------------------------------------------- host clustering
# Host functions of libscc (no device, no Engine): the reference keeps tree
# building and tree cutting on the host (Fast:406-427).

def hclust_ward_d2(dist_packed, n):
    """fastcluster::hclust(d, "ward.D2") -> (merge (n-1, 2) int32 in R's
    convention, height (n-1,), order (n,) 1-based)."""
    d = np.ascontiguousarray(dist_packed, np.float64)
    if d.shape != (n * (n - 1) // 2,):
        raise ValueError("dist_packed must hold n(n-1)/2 entries")
    merge = np.zeros(2 * (n - 1), np.int32)
    height = np.zeros(n - 1)
    order = np.zeros(n, np.int32)
    rc = load().scc_hclust_ward_d2(_ptr(d), n, _ptr(merge), _ptr(height), _ptr(order))
    if rc != SCC_OK:
        raise SccError(rc, "scc_hclust_ward_d2 failed")
    return merge.reshape(2, n - 1).T.copy(), height, order


def cutree_hybrid(merge, height, dist_packed, deep_split=1, min_cluster_size=20):
    """dynamicTreeCut::cutreeDynamic(method = "hybrid", pamStage = FALSE)
    labels (0 = unassigned) and the default cut height used."""
    merge = np.asarray(merge)
    n = merge.shape[0] + 1
    m = np.ascontiguousarray(merge.T.reshape(-1), np.int32)
    h = np.ascontiguousarray(height, np.float64)
    d = np.ascontiguousarray(dist_packed, np.float64)
    if d.shape != (n * (n - 1) // 2,) or h.shape != (n - 1,):
        raise ValueError("shape mismatch between merge, height and dist_packed")
    lab = np.zeros(n, np.int32)
    cut = ctypes.c_double()
    rc = load().scc_cutree_hybrid(_ptr(m), _ptr(h), n, _ptr(d), int(deep_split), int(min_cluster_size), _ptr(lab),
                                  ctypes.byref(cut))
    if rc != SCC_OK:
        raise SccError(rc, "scc_cutree_hybrid failed (deepSplit must be 0..4)")
    return lab, cut.value



def hclust_complete(dist_packed, n):
    """stats::hclust(d, "complete") -> (merge, height, order) as
    hclust_ward_d2; heights are entries of dist_packed.  On exact ties the
    lowest index wins: a valid complete-linkage tree R may resolve otherwise."""
    d = np.ascontiguousarray(dist_packed, np.float64)
    if d.shape != (n * (n - 1) // 2,):
        raise ValueError("dist_packed must hold n(n-1)/2 entries")
    merge = np.zeros(2 * (n - 1), np.int32)
    height = np.zeros(n - 1)
    order = np.zeros(n, np.int32)
    rc = load().scc_hclust_complete(_ptr(d), n, _ptr(merge), _ptr(height), _ptr(order))
    if rc != SCC_OK:
        raise SccError(rc, "scc_hclust_complete failed")
    return merge.reshape(2, n - 1).T.copy(), height, order


def dendro_reorder(merge, wts):
    """stats::reorder.dendrogram(as.dendrogram(tree), wts, agglo.FUN = mean):
    (merge with the swapped rows, the new 1-based leaf order)."""
    merge = np.asarray(merge)
    n = merge.shape[0] + 1
    m = np.ascontiguousarray(merge.T.reshape(-1), np.int32)
    w = np.ascontiguousarray(wts, np.float64)
    if w.shape != (n,):
        raise ValueError("wts must hold one weight per leaf")
    mo = np.zeros(2 * (n - 1), np.int32)
    order = np.zeros(n, np.int32)
    rc = load().scc_dendro_reorder(_ptr(m), n, _ptr(w), _ptr(mo), _ptr(order))
    if rc != SCC_OK:
        raise SccError(rc, "scc_dendro_reorder failed (merge is not a tree over len(wts) leaves)")
    return mo.reshape(2, n - 1).T.copy(), order
