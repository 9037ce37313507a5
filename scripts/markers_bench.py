"""Time the one-vs-rest marker call (scc_de_markers) beside the only route the
engine had before it: K scc_de_run calls with binary codes (cluster a -> 0,
every other kept cell -> 1), and beside the all-pairs scc_de_run for scale.

markers_bench.py [--configs B[,D]] [--reps 5] [--warmup 2] [--out FILE]

Per config, with the dataset resident (B from bench.py's cached host input;
C/D/E generated on the device):
  markers      wall time of Engine.de_markers (fetch="union": the union and the
               counts come back, as for the other two), median of --reps calls;
               its rank stage from the context's "rank_rest" timer, and in a
               separate pass with every stage timed the stage split
  binary_sum   the sum over a of the wall times of de_run(binary code of a,
               K = 2), median of --reps sums
  all_pairs    wall time of the all-pairs de_run and its "gene_rank" timer
Timed passes bracket only the rank stage with events (SCC_PROFILE_STAGES); no
counters are collected.  One JSON line per config; with --out a markdown table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scconsensus_amd import _native as nat  # noqa: E402
from scconsensus_amd import api, synth  # noqa: E402

SPLIT = ["ingest", "gene_stats", "rest_filter", "rank_rest", "rest_test", "pair_select"]


def upload(eng, cfg):
    if cfg in ("A", "B"):
        import bench
        d = bench.host_dataset(cfg, synth.CONFIGS[cfg]["seed"])
        return eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N), d.labels, d
    import torch
    dd = synth.generate_device(cfg, torch.device("cuda", 0))
    torch.cuda.synchronize()
    ds = eng.dataset_csc_device(dd.indptr.data_ptr(), dd.indices.data_ptr(), dd.data.data_ptr(), dd.G, dd.N, dd.nnz)
    return ds, dd.labels, dd


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def run(cfg, reps, warmup):
    os.environ["SCC_PROFILE_STAGES"] = "rank_rest,gene_rank"
    if cfg not in ("A", "B"):  # torch brings up its device before libscc loads, as bench.py has it
        import torch
        torch.cuda.init()
    eng = nat.Engine(0, profile=True)
    ds, labels, keep = upload(eng, cfg)
    names, code = api.select_clusters(labels, 10)
    K = len(names)
    codes = [np.where(code < 0, -1, np.where(code == a, 0, 1)).astype(np.int32) for a in range(K)]

    def markers():
        return eng.de_markers(ds, code, K, fetch="union")

    def binary():
        return [eng.de_run(ds, c, 2, nat.SCC_DE_FAST, fetch="union") for c in codes]

    def pairs():
        return eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="union")

    row = {"config": cfg, "cells": ds.N, "genes": ds.G, "K": K, "reps": reps}
    for name, fn, timer in (("markers", markers, "rank_rest"), ("binary_sum", binary, "gene_rank"),
                            ("all_pairs", pairs, "gene_rank")):
        for _ in range(warmup):  # code objects, workspace, the dataset's mirror
            fn()
        eng.synchronize()
        eng.reset_timers()
        ms = timed(fn, reps)
        k = eng.kernel_time(timer)
        row[f"{name}_ms"] = statistics.median(ms)
        row[f"{name}_ms_min"], row[f"{name}_ms_max"] = min(ms), max(ms)
        row[f"{name}_rank_ms"] = k[0] / reps  # per call of fn (binary_sum: over its K runs)
    row["union_markers"] = int(len(markers().union))
    row["speedup_vs_binary_sum"] = row["binary_sum_ms"] / row["markers_ms"]
    # the markers call's stage split: a pass of its own with every stage timed
    os.environ["SCC_PROFILE_STAGES"] = ""
    eng.synchronize()
    eng.reset_timers()
    for _ in range(reps):
        markers()
    row["markers_stages_ms"] = {s: eng.kernel_time(s)[0] / reps for s in SPLIT}
    print(json.dumps(row), flush=True)
    ds.close()
    eng.close()
    return row


def table(rows):
    out = ["| config | cells x genes | K | markers ms (min-max) | rank_rest ms | K binary de_run calls, sum ms (min-max) | "
           "their gene_rank ms | ratio sum / markers | all-pairs de_run ms | its gene_rank ms |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} | {r['cells']} x {r['genes']} | {r['K']} | {r['markers_ms']:.2f} "
                   f"({r['markers_ms_min']:.2f}-{r['markers_ms_max']:.2f}) | {r['markers_rank_ms']:.2f} | "
                   f"{r['binary_sum_ms']:.2f} ({r['binary_sum_ms_min']:.2f}-{r['binary_sum_ms_max']:.2f}) | "
                   f"{r['binary_sum_rank_ms']:.2f} | {r['speedup_vs_binary_sum']:.2f} | {r['all_pairs_ms']:.2f} | "
                   f"{r['all_pairs_rank_ms']:.2f} |")
    out += ["", "Stage split of the markers call (ms per call, every stage timed, a pass of its own):", "",
            "| config | " + " | ".join(SPLIT) + " |", "|---|" + "---|" * len(SPLIT)]
    for r in rows:
        out.append(f"| {r['config']} | " + " | ".join(f"{r['markers_stages_ms'][s]:.3f}" for s in SPLIT) + " |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(c, a.reps, a.warmup) for c in a.configs.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table(rows))
