"""Time scc_snn_clusters_scores (k-NN, SNN graph and modularity clustering from
the PCA scores in one call) against the host route and write
profiles/snn_cluster.md.

snn_bench.py [--configs B] [--blobs 200000] [--resolutions 0.2,0.8] [--reps 5] [--host-reps 5] [--out FILE]
             [--no-host]

Per config (the kept scores of its marker-union PCA, all 15 components,
k_param = 20) and per resolution: the wall time of the fused call and the
kernel time of its three timer families, medians of --reps calls after a
warm-up call; the levels, the sweeps and the device memory the call added.  At
every config the host route a user has without this stage runs on the same
scores, alternating with the fused call: the engine's k-NN (scc_knn_scores),
scipy's M M^T for the SNN graph (tests/snn_reference.py: snn_graph) and
networkx's Louvain on the result, 16 host threads allowed (networkx itself runs
on one).  Per blob size (seeded blob points as scores) the fused call alone.

The host part (skipped with --no-host) measures what the quality test's margin
rests on: the shortfall of the NumPy reference's modularity against the best
of networkx's Louvain over seeds 0..4 on the test's four inputs.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import snn_reference as sr  # noqa: E402

HOST_THREADS = 16
FAMILIES = ("knn_scores", "snn_graph", "modularity_cluster")
K_PARAM = 20
PRUNE = 1.0 / 15.0


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def nx_graph(indptr, cols, vals):
    import networkx as nx
    G = nx.Graph()
    n = len(indptr) - 1
    G.add_nodes_from(range(n))
    row = np.repeat(np.arange(n), np.diff(indptr))
    up = cols > row
    G.add_weighted_edges_from(zip(row[up].tolist(), cols[up].tolist(), vals[up].tolist()))
    return G


# ------------------------------------------------------------------ host part
def quality_rows():
    import networkx as nx
    import test_snn_reference as tr
    rows = []
    for n, scale, gamma in tr.QUALITY:
        (indptr, cols, vals, _), _ = tr.blob_graph(n, scale)
        out = sr.modularity_cluster(indptr, cols, vals, gamma)
        G = nx_graph(indptr, cols, vals)
        mine = [set(np.flatnonzero(out["labels"] == c).tolist()) for c in range(out["n_clusters"])]
        q_mine = nx.community.modularity(G, mine, weight="weight", resolution=gamma)
        q_nx = [nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=s),
                                        weight="weight", resolution=gamma) for s in range(5)]
        rows.append({"cells": n, "scale": scale, "resolution": gamma, "nnz": int(indptr[-1]), "q_reference": q_mine,
                     "q_networkx_best": max(q_nx), "q_networkx_worst": min(q_nx), "shortfall": max(q_nx) - q_mine,
                     "clusters": out["n_clusters"], "levels": out["n_levels"], "sweeps": out["sweeps"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


# ---------------------------------------------------------------- device part
def host_route(eng, n, ptr, gamma):
    """What a user has today: the engine's table, scipy's product, networkx's Louvain.  Seconds per stage."""
    import networkx as nx
    t0 = time.perf_counter()
    idx, _ = eng.knn_scores(n, K_PARAM - 1, 0, ptr)
    t1 = time.perf_counter()
    indptr, cols, vals, _ = sr.snn_graph(idx, PRUNE)
    t2 = time.perf_counter()
    G = nx_graph(indptr, cols, vals)
    comms = nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=0)
    t3 = time.perf_counter()
    return {"knn_s": t1 - t0, "snn_s": t2 - t1, "louvain_s": t3 - t2, "wall_s": t3 - t0, "clusters": len(comms)}


def measure(eng, torch, tag, n, t, gamma, reps, host_reps):
    ptr = t.data_ptr()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    free0, _ = torch.cuda.mem_get_info()
    out = eng.snn_clusters_scores(n, K_PARAM, 0, PRUNE, gamma, ptr, return_graph=True)  # warm-up, and the graph
    free1, _ = torch.cuda.mem_get_info()
    g = out["graph"]
    walls, ms, hosts = [], {f: [] for f in FAMILIES}, []
    same = True
    for r in range(max(reps, host_reps)):
        if r < reps:
            eng.synchronize()
            eng.reset_timers()
            t0 = time.perf_counter()
            again = eng.snn_clusters_scores(n, K_PARAM, 0, PRUNE, gamma, ptr)
            walls.append(time.perf_counter() - t0)
            same = same and np.array_equal(again["labels"], out["labels"]) and again["modularity"] == out["modularity"]
            for f in FAMILIES:
                v, calls = eng.kernel_time(f)
                ms[f].append(v / max(calls, 1))
        if r < host_reps:  # the routes alternate
            hosts.append(host_route(eng, n, ptr, gamma))
    row = {"input": tag, "cells": n, "k_param": K_PARAM, "resolution": gamma, "reps": reps, "nnz": int(g[0][-1]),
           "longest_row": int(np.diff(g[0]).max()), "clusters": out["n_clusters"], "levels": out["n_levels"],
           "sweeps": out["sweeps"], "modularity": out["modularity"], "wall_s": median(walls), "wall_s_all": walls,
           "same_bits": bool(same), "device_bytes_added": int(free0 - free1)}
    for f in FAMILIES:
        row[f + "_ms"] = median(ms[f])
    if hosts:
        row["host_reps"] = len(hosts)
        for key in ("knn_s", "snn_s", "louvain_s", "wall_s"):
            row["host_" + key] = median([h[key] for h in hosts])
        row["host_wall_s_all"] = [h["wall_s"] for h in hosts]
        row["host_clusters"] = hosts[0]["clusters"]
        row["fused_faster_than_host"] = bool(row["wall_s"] < row["host_wall_s"])
    print(json.dumps(row), flush=True)
    return row


def config_scores(eng, torch, cfg):
    from scconsensus_amd import _native as nat
    from scconsensus_amd import api, synth
    d = synth.generate(cfg)
    names, code = api.select_clusters(d.labels, 10)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    r = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union")
    eng.pca_scores(ds, r.union)
    x = eng.last_pca_scores(d.N)
    ds.close()
    p = np.zeros((d.N, 16))
    p[:, :x.shape[1]] = x
    return d.N, torch.tensor(p, device="cuda")


def markdown(rows, quality):
    out = ["# SNN graph and modularity clustering on the engine", "",
           "Written by `scripts/snn_bench.py`.  No Seurat, igraph or leidenalg was available: nothing here compares with",
           "them.  The rules are restated in NumPy in `tests/snn_reference.py`.", ""]
    if quality:
        worst = max(r["shortfall"] for r in quality)
        out += ["## What the quality test's margin rests on (host, measured)", "",
                "SNN graphs (k = 19, prune 1/15) of 8 unit-spread Gaussian blobs in 8 dimensions, centres at `scale` times",
                "a standard normal, seed 1.  Q is `networkx.community.modularity` on the float64 graph; networkx: the best",
                "and the worst of `louvain_communities` over seeds 0..4.", "",
                "| cells | scale | resolution | nnz | Q reference | Q networkx best | worst | shortfall | clusters | levels | "
                "sweeps |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        out += [f"| {r['cells']} | {r['scale']} | {r['resolution']} | {r['nnz']} | {r['q_reference']:.6f} | "
                f"{r['q_networkx_best']:.6f} | {r['q_networkx_worst']:.6f} | {r['shortfall']:.6f} | {r['clusters']} | "
                f"{r['levels']} | {r['sweeps']} |" for r in quality]
        out += ["", f"Largest shortfall {worst:.6f}; `tests/test_snn_reference.py` allows twice that.  A negative",
                "shortfall means the reference is ahead of networkx's best.", ""]
    if rows:
        out += ["## Device timings (measured)", "",
                f"One MI355X, `scc_snn_clusters_scores` at k_param = {K_PARAM}, prune = 1/15, all 15 components; medians",
                "after a warm-up call.  Wall: the fused call with the copy of its labels.  Kernel ms: the call's three",
                "timer families (the clustering's includes its host loop's waits: one small read per sweep).  Device",
                "memory: what the input's first call added to the device's used memory (the grow-only workspace, the",
                "k-NN stage's included): 0 where nothing grew, and a later input's figure is the growth beyond the",
                "earlier inputs'.", "",
                "| input | cells | resolution | nnz | longest row | clusters | levels | sweeps | wall s | knn ms | snn ms | "
                "cluster ms | device MiB | same bits |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            out.append(f"| {r['input']} | {r['cells']} | {r['resolution']} | {r['nnz']} | {r['longest_row']} | "
                       f"{r['clusters']} | {r['levels']} | {r['sweeps']} | {r['wall_s']:.4f} | {r['knn_scores_ms']:.3f} | "
                       f"{r['snn_graph_ms']:.3f} | {r['modularity_cluster_ms']:.3f} | "
                       f"{r['device_bytes_added'] / 2 ** 20:.0f} | {r['same_bits']} |")
        out.append("")
        host = [r for r in rows if "host_wall_s" in r]
        if host:
            out += ["## The speed condition (measured)", "",
                    f"The host route on the same scores, alternating with the fused call, {HOST_THREADS} host threads",
                    "allowed: the engine's k-NN, scipy's M M^T, then the networkx graph and `louvain_communities`.", "",
                    "| input | resolution | fused s | host s | k-NN s | scipy SNN s | networkx s | host reps | host clusters | "
                    "fused faster |", "|---|---|---|---|---|---|---|---|---|---|"]
            out += [f"| {r['input']} | {r['resolution']} | {r['wall_s']:.4f} | {r['host_wall_s']:.2f} | {r['host_knn_s']:.3f} | "
                    f"{r['host_snn_s']:.2f} | {r['host_louvain_s']:.2f} | {r['host_reps']} | {r['host_clusters']} | "
                    f"{r['fused_faster_than_host']} |" for r in host]
            out.append("")
        out += ["## Arithmetic on counts (not measured)", "",
                "The pair walk of `k_snn_pairs` visits, for every row, the rows that hold each of its K members and merges",
                "two K-lists per visit: about n K^2 candidates of at most 2 K integer steps, twice (count and fill).  At",
                f"200,000 cells and K = {K_PARAM} that is 2 x 200000 x 400 x 40 = 6.4e9 steps at most; the measured snn ms",
                "above divides into it.  A sweep reads every entry once for the moves and once for the state: 2 nnz",
                "entries of 12 bytes (column and weight) plus one community read each.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B")
    ap.add_argument("--blobs", default="200000")
    ap.add_argument("--resolutions", default="0.2,0.8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snn_cluster.md"))
    a = ap.parse_args()
    quality = rows = None
    if not a.no_host:
        quality = quality_rows()
    if not a.no_device:
        os.environ["SCC_PROFILE_STAGES"] = ",".join(FAMILIES)
        import torch
        from scconsensus_amd import _native as nat
        torch.cuda.init()  # torch holds the scores: its runtime starts before the engine's first call
        torch.set_num_threads(HOST_THREADS)
        eng = nat.Engine(0, profile=True)
        rows = []
        gammas = [float(v) for v in a.resolutions.split(",") if v]
        for cfg in [c for c in a.configs.split(",") if c]:
            n, t = config_scores(eng, torch, cfg)
            rows += [measure(eng, torch, f"config {cfg}", n, t, g, a.reps, a.host_reps) for g in gammas]
            del t
        for n in [int(v) for v in a.blobs.split(",") if v]:
            p = np.zeros((n, 16))
            p[:, :8] = sr.blobs(n, 3.0, seed=1)[0]
            t = torch.tensor(p, device="cuda")
            rows += [measure(eng, torch, "blobs", n, t, g, a.reps, 0) for g in gammas]
            del t
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(rows, quality))
    print(a.out)
    slow = [r for r in rows or [] if r.get("fused_faster_than_host") is False]
    assert not slow, "the fused call is not faster than the host route"


if __name__ == "__main__":
    main()
