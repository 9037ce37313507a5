"""Time scc_silhouette on the config-B distance vector (HBM-resident).

sil_bench.py [CONFIG]: one JSON line for scc_silhouette on CONFIG (default B).

sil_bench.py --scores [--configs A,B] [--blobs 50000,200000] [--out FILE]:
scc_silhouette_scores (the widths from the PCA scores, no N x N matrix) beside
it.  Per config: both on one engine in one session, alternating, the kernel
time of each from timing events, and whether the widths are equal bit for bit.
Per blob size (cell counts no distance fits): seeded blob points as scores, the
scores route alone, labels from the deepSplit 1-4 cuts of the scores tree, the
kernel and wall time per cut and the device memory in use.  One JSON line per
measurement; the tables go to profiles/silhouette_scores.md."""
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

REPS = 5
MCS = 10
DEEP_SPLITS = (1, 2, 3, 4)
# the unmeasured model the kernel was written against: ~30 fp64 vector operations per ordered pair
MODEL_OPS_PER_PAIR = 30
# only the two silhouettes get timing events (a timed tree is two events per launch of its chain)
STAGES = "silhouette,silhouette_scores"


def distance_route(cfg):
    d = synth.generate(cfg)
    names, code = api.select_clusters(d.labels, 10)
    eng = nat.Engine(0, profile=True)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    r = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union")
    eng.distance(ds, r.union, device_out_ptr=0)
    for _ in range(2):
        eng.silhouette(d.N, code)
    eng.synchronize()
    eng.reset_timers()
    for _ in range(REPS):
        w, ca = eng.silhouette(d.N, code)
    ms = eng.kernel_time("silhouette")
    t = ms[0] / ms[1]
    stored = 8.0 * d.N * (d.N - 1) / 2
    print(json.dumps({"config": cfg, "cells": d.N, "clusters": int(len(np.unique(code))), "silhouette_ms": t,
                      "stored_dist_GBps": stored / t / 1e6, "read_GBps_both_halves": 2 * stored / t / 1e6,
                      "SI": float(np.mean(ca))}), flush=True)


def both_routes(cfg):
    """scc_silhouette on the kept distance and scc_silhouette_scores on the kept scores, alternating."""
    d = synth.generate(cfg)
    names, code = api.select_clusters(d.labels, 10)
    eng = nat.Engine(0, profile=True)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    r = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union")
    eng.distance(ds, r.union, device_out_ptr=0)  # keeps the distance and the scores it was formed from
    for _ in range(2):
        eng.silhouette(d.N, code)
        eng.silhouette_scores(d.N, code)
    eng.synchronize()
    eng.reset_timers()
    for _ in range(REPS):
        wd, cd = eng.silhouette(d.N, code)
        ws, cs = eng.silhouette_scores(d.N, code)
    md, ms = eng.kernel_time("silhouette"), eng.kernel_time("silhouette_scores")
    row = {"config": cfg, "cells": d.N, "clusters": int(len(np.unique(code))), "reps": REPS,
           "silhouette_ms": md[0] / md[1], "silhouette_scores_ms": ms[0] / ms[1],
           "identical": bool(np.array_equal(wd, ws) and np.array_equal(cd, cs)), "SI": float(np.mean(cs))}
    row["pairs_per_s"] = float(d.N) * d.N / row["silhouette_scores_ms"] * 1e3
    print(json.dumps(row), flush=True)
    eng.close()
    return row


def blob_points(n, seed):
    """Seeded Gaussian blobs in 15 dimensions as [n][16] scores (tree_bench.py's)."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=6.0, size=(50, 15))
    p = np.zeros((n, 16))
    p[:, :15] = centers[rng.integers(0, 50, n)] + rng.normal(size=(n, 15))
    return p


def blob_route(n):
    """The scores route alone: tree, four cuts, one silhouette per cut."""
    import torch
    eng = nat.Engine(0, profile=True)
    free0 = torch.cuda.mem_get_info()[0]
    t = torch.tensor(blob_points(n, 4), device="cuda")
    torch.cuda.synchronize()
    eng.silhouette_scores(3000, np.arange(3000, dtype=np.int32) % 3, t.data_ptr())  # warm-up: code objects
    t0 = time.perf_counter()
    m, h, _ = eng.hclust_ward_d2_scores(n, t.data_ptr())
    tree_s = time.perf_counter() - t0
    cuts = []
    for dsv in DEEP_SPLITS:
        lab, _ = eng.cutree_hybrid_scores(m, h, dsv, MCS, t.data_ptr())
        eng.synchronize()
        eng.reset_timers()
        t0 = time.perf_counter()
        w, ca = eng.silhouette_scores(n, lab, t.data_ptr())
        wall = time.perf_counter() - t0
        ms, calls = eng.kernel_time("silhouette_scores")
        w2, _ = eng.silhouette_scores(n, lab, t.data_ptr())
        cuts.append({"deepSplit": dsv, "groups": int(len(ca)), "kernel_ms": ms / calls, "wall_s": wall,
                     "SI": float(np.mean(ca)), "finite": bool(np.all(np.isfinite(w))),
                     "repeatable": bool(np.array_equal(w, w2))})
    in_use = free0 - torch.cuda.mem_get_info()[0]  # the scores, the engine's workspace, the allocator's slack
    eng.close()
    row = {"cells": n, "tree_s": tree_s, "cuts": cuts, "device_bytes_in_use": int(in_use),
           "matrix_bytes": 4.0 * n * (n - 1)}
    print(json.dumps(row), flush=True)
    return row


def markdown(rows, blobs):
    out = ["# Silhouette widths from the PCA scores against the distance route", "",
           "Written by `scripts/sil_bench.py --scores` on one MI355X host.  `scc_silhouette` reads the engine-kept",
           "packed f64 distance; `scc_silhouette_scores` computes every entry from two rows of the kept [N][16]",
           "scores with the dist kernel's arithmetic and sums in the same order.  Both on one engine in one",
           f"session, alternating, {REPS} repetitions after 2 warm-up calls; kernel time from timing events (the",
           "non-finite count, the sums and the widths kernel of a call).  The labels are the cluster codes.", "",
           "| config | cells | groups | silhouette ms | silhouette_scores ms | pairs / s (scores) | widths identical | SI |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} | {r['cells']} | {r['clusters']} | {r['silhouette_ms']:.3f} | "
                   f"{r['silhouette_scores_ms']:.3f} | {r['pairs_per_s']:.3g} | {r['identical']} | {r['SI']:.6f} |")
    out += ["", "The 2.2 ms of `scc_silhouette` at config B recorded in DESIGN.md is the figure the first column",
            "repeats.  Nobody set a speed target between the two routes: the scores route exists for the cell",
            "counts below, where there is no distance to read."]
    if blobs:
        out += ["", "Cell counts no packed distance fits: seeded Gaussian blob points (50 centres, 15 dimensions) as",
                "scores, the scores route alone.  Labels: the deepSplit 1-4 cuts of the scores tree (minClusterSize",
                f"{MCS}; label 0, unassigned, counts as a group as in the reference).  One call per cut: its kernel time,",
                "its wall time (label upload and the copy of the widths included).  Model (unmeasured, from the",
                f"issue): N^2 ordered pairs x ~{MODEL_OPS_PER_PAIR} fp64 vector operations.  Device memory in use: the drop in free",
                "device memory from before the scores are uploaded to after the last call (the scores, 8 N C",
                "doubles of partial sums, O(N) besides, allocator slack).", "",
                "| cells | tree s | deepSplit | groups | kernel ms | wall s | pairs / s | model lane-operations / s | "
                "SI | finite | repeatable | device memory in use | 4 N^2 packed distance |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for b in blobs:
            n = b["cells"]
            for c in b["cuts"]:
                pps = float(n) * n / c["kernel_ms"] * 1e3
                out.append(f"| {n} | {b['tree_s']:.3f} | {c['deepSplit']} | {c['groups']} | {c['kernel_ms']:.1f} | "
                           f"{c['wall_s']:.3f} | {pps:.3g} | {pps * MODEL_OPS_PER_PAIR:.3g} | {c['SI']:.6f} | "
                           f"{c['finite']} | {c['repeatable']} | {b['device_bytes_in_use'] / 1e6:.0f} MB | "
                           f"{b['matrix_bytes'] / 1e9:.1f} GB |")
        out += ["", "The model's rate column is pairs / s times its operation count: what the vector units would have to",
                "sustain if the model's operations were all the kernel did.  It leaves out the four one-hot fp64 MFMAs",
                "per 16 x 4 entries (64 clusters are swept whatever the group count, as on the distance route) and the",
                "128 bytes of LDS a lane reads per entry.  The products are 128 flop per entry: at the 78.6 TFLOP/s",
                "fp64 MFMA peak they alone are N^2 x 1.6 ps, 65 ms at 200,000 cells, so the one-hot sweep, not the",
                "entry arithmetic, is the larger term; no counters were collected to confirm the split.",
                "The one condition set for this route: a silhouette takes less than the same size's tree (the tree s",
                "column; 6.05 s at 200,000 cells in `profiles/hclust_scores.md`)."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="B")
    ap.add_argument("--scores", action="store_true", help="measure scc_silhouette_scores beside scc_silhouette")
    ap.add_argument("--configs", default="A,B")
    ap.add_argument("--blobs", default="50000,200000", help="comma-separated cell counts for the scores route alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_scores.md"))
    a = ap.parse_args()
    if not a.scores:
        distance_route(a.config)
        return
    os.environ["SCC_PROFILE_STAGES"] = STAGES
    if a.blobs:  # torch holds the blob scores: its runtime starts before the engine's first call
        import torch
        torch.cuda.init()
    rows = [both_routes(c) for c in a.configs.split(",") if c]
    blobs = [blob_route(int(v)) for v in a.blobs.split(",") if v]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(rows, blobs))
    print(a.out)


if __name__ == "__main__":
    main()
