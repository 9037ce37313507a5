"""Time the heatmap's device inputs (scc_gene_distance, scc_heatmap_raster)
at a config's DE-gene union, beside scipy's pdist of the same panel.

heatmap_bench.py [--configs B[,D]] [--reps 5] [--width 4096] [--pdist-max-terms 2e10] [--out FILE]

Per config: the FAST DE's union on the config's matrix (B from bench.py's
cached host input; C/D/E generated on the device), then
  gene_distance   the "gene_dist" timer family (the pair kernel and its slab
                  reduction) and the wall time of the whole call (gather,
                  means, range, kernel, copies out); the achieved FP64 rate
                  counts 3 flops per term (subtract, multiply, add) over the
                  nu (nu - 1) / 2 pairs the caller gets, not the padded tiles
  heatmap_raster  the "heatmap_raster" family and the call's wall time; GB/s
                  over the nu x N panel values it reads
  pdist           scipy.spatial.distance.pdist(X[U, ]) on the host, one run
                  (skipped above --pdist-max-terms subtract-multiply-adds)
One JSON line per config; with --out also a markdown table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scconsensus_amd import _native as nat  # noqa: E402
from scconsensus_amd import api, synth  # noqa: E402

STAGES = "gene_dist,heatmap_raster"  # only these two get timing events


def upload(eng, cfg):
    """(dataset, labels, host dense block getter) for a config."""
    if cfg in ("A", "B"):
        import bench
        d = bench.host_dataset(cfg, synth.CONFIGS[cfg]["seed"])
        ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
        return ds, d.labels, d, None
    import torch
    dd = synth.generate_device(cfg, torch.device("cuda", 0))
    torch.cuda.synchronize()
    ds = eng.dataset_csc_device(dd.indptr.data_ptr(), dd.indices.data_ptr(), dd.data.data_ptr(), dd.G, dd.N, dd.nnz)
    return ds, dd.labels, None, dd


def union_block(d, dd, uni):
    """X[U, ] as a dense host array (for pdist)."""
    if d is None:
        d = dd.to_host()
    m = d.scipy_csc().tocsr()[uni]
    return np.asarray(m.todense(), np.float64)


def run(cfg, reps, width, pdist_max_terms):
    os.environ["SCC_PROFILE_STAGES"] = STAGES
    if cfg not in ("A", "B"):  # torch brings up its device before libscc loads, as bench.py has it
        import torch
        torch.cuda.init()
    eng = nat.Engine(0, profile=True)
    ds, labels, d, dd = upload(eng, cfg)
    names, code = api.select_clusters(labels, 10)
    uni = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    nu, N = len(uni), ds.N
    width = min(width, N)
    rows = np.arange(1, nu + 1, dtype=np.int32)
    cells = np.random.default_rng(0).permutation(N).astype(np.int32) + 1  # an hclust order is a permutation
    row = {"config": cfg, "cells": N, "union": nu, "width": width, "reps": reps}
    try:
        for _ in range(2):  # warm-up: code objects, workspace
            dist, mean, rng = eng.gene_distance(ds, uni)
            eng.heatmap_raster(ds, uni, rows, cells, width)
    except nat.SccError as e:
        if e.code != nat.SCC_ERR_OOM:
            raise
        row["skipped"] = str(e)
        print(json.dumps(row), flush=True)
        return row
    eng.synchronize()
    eng.reset_timers()
    t0 = time.perf_counter()
    for _ in range(reps):
        dist, mean, rng = eng.gene_distance(ds, uni)
    t1 = time.perf_counter()
    for _ in range(reps):
        eng.heatmap_raster(ds, uni, rows, cells, width)
    t2 = time.perf_counter()
    kd, kr = eng.kernel_time("gene_dist"), eng.kernel_time("heatmap_raster")
    terms = nu * (nu - 1) / 2.0 * N
    row.update(gene_dist_kernel_ms=kd[0] / kd[1], gene_dist_call_ms=(t1 - t0) / reps * 1e3,
               gene_dist_fp64_tflops=3.0 * terms / (kd[0] / kd[1]) / 1e9,
               raster_kernel_ms=kr[0] / kr[1], raster_call_ms=(t2 - t1) / reps * 1e3,
               raster_read_GBps=8.0 * nu * N / (kr[0] / kr[1]) / 1e6)
    if terms <= pdist_max_terms:
        from scipy.spatial.distance import pdist
        B = union_block(d, dd, uni)
        t3 = time.perf_counter()
        ref = pdist(B)
        row["pdist_ms"] = (time.perf_counter() - t3) * 1e3
        row["max_rel_diff_vs_pdist"] = float(np.max(np.abs(dist - ref) / np.maximum(ref, 1e-300)))
        row["call_speedup_vs_pdist"] = row["pdist_ms"] / row["gene_dist_call_ms"]
    else:
        row["pdist_ms"] = None
    print(json.dumps(row), flush=True)
    ds.close()
    eng.close()
    return row


def table(rows):
    out = ["| config | cells | union | gene_dist kernel ms | gene_dist call ms | FP64 TFLOP/s (3 flops/term) | "
           "pdist ms | raster kernel ms | raster call ms | raster GB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "skipped" in r:
            out.append(f"| {r['config']} | {r['cells']} | {r['union']} | not run: {r['skipped']} |||||||")
            continue
        pd = "not run" if r["pdist_ms"] is None else f"{r['pdist_ms']:.1f}"
        out.append(f"| {r['config']} | {r['cells']} | {r['union']} | {r['gene_dist_kernel_ms']:.3f} | "
                   f"{r['gene_dist_call_ms']:.2f} | {r['gene_dist_fp64_tflops']:.2f} | {pd} | "
                   f"{r['raster_kernel_ms']:.3f} | {r['raster_call_ms']:.2f} | {r['raster_read_GBps']:.0f} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--pdist-max-terms", type=float, default=2e10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(c, a.reps, a.width, a.pdist_max_terms) for c in a.configs.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table(rows))
