"""Time scc_umap_scores (k-NN, fuzzy simplicial set and layout from the PCA
scores in one call) and write profiles/umap_layout.md.

umap_bench.py [--configs A,B] [--blobs 200000] [--epochs 200] [--out FILE] [--no-host]

Per config (the kept scores of its marker-union PCA, dims 8 as in the README)
and per blob size (seeded blob points as scores): the wall time of the fused
call and the kernel time of its three timer families (knn_scores, umap_graph,
umap_layout), medians of 5 after a warm-up call, and the layout's interactions
per second: the attractions and draws of the run, counted from the schedule on
the host (tests/umap_reference.py: schedule_counts), over the layout's kernel
time.  At config B the NumPy reference lays out the same graph from the same
initialisation with the same epochs on the host: the only host route this
repository can run (no umap, uwot or umap-learn is installed).

The host part (skipped with --no-host) measures what the layout tests' bounds
rest on: the deviation between the float64 reference and the same reference in
np.longdouble, and the reference's quality at n = 3000 over five seeds.
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
import umap_reference as ur  # noqa: E402
import ward_vector_reference as wv  # noqa: E402

REPS = 5
HOST_THREADS = 16
FAMILIES = ("knn_scores", "umap_graph", "umap_layout")


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


# ------------------------------------------------------------------ host part
def rounding_rows():
    """float64 against longdouble reference at the layout tests' shapes (their tables come from the device; the
    host's exact table of the same points differs from it in the last bits of the distances only)."""
    rows = []

    def one(tag, g, init):
        for ep in (1, 2, 10):
            y64 = ur.layout(g[0], g[1], g[2], init, n_epochs=ep, seed=7)
            yld = ur.layout(g[0], g[1], g[2], init, n_epochs=ep, seed=7, dtype=np.longdouble)
            dev = float(np.max(np.abs(y64.astype(np.longdouble) - yld)))
            ext = float(np.max(np.ptp(y64, axis=0)))
            rows.append({"graph": tag, "epochs": ep, "rounding": dev, "extent": ext,
                         "bound": max(100.0 * dev, 1e-12 * ext)})
            print(json.dumps(rows[-1]), flush=True)
    for n in (17, 65, 1025):
        x = wv.blobs(n)
        idx, dist = ur.knn_table(x, 14)
        one(f"blobs n = {n}, n_neighbors = 15", ur.fuzzy_graph(idx, dist), ur.pca_init(x))
    idx, dist = ur.hub_table(300, 4)
    one("hub n = 300", ur.fuzzy_graph(idx, dist), np.random.default_rng(300).normal(scale=5.0, size=(300, 2)))
    return rows


def quality_rows():
    from sklearn.manifold import trustworthiness
    x, lab = ur.blobs(3000, dim=8, n_blobs=6, seed=3000)
    idx, dist = ur.knn_table(x, 14)
    g = ur.fuzzy_graph(idx, dist)
    init = ur.pca_init(x)
    rows = [{"seed": "init", "trustworthiness": float(trustworthiness(x, init, n_neighbors=15)),
             "purity": ur.label_purity(init, lab)}]
    for seed in range(5):
        y = ur.layout(g[0], g[1], g[2], init, n_epochs=200, seed=seed)
        rows.append({"seed": seed, "trustworthiness": float(trustworthiness(x, y, n_neighbors=15)),
                     "purity": ur.label_purity(y, lab)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


# ---------------------------------------------------------------- device part
def measure(eng, tag, n, t, dims, nn, epochs, host_reference):
    ptr = t.data_ptr()
    y, g = eng.umap_scores(n, nn, dims, ptr, n_epochs=epochs, seed=0, return_graph=True)  # warm-up, and the graph
    walls, ms = [], {f: [] for f in FAMILIES}
    for _ in range(REPS):
        eng.synchronize()
        eng.reset_timers()
        t0 = time.perf_counter()
        again = eng.umap_scores(n, nn, dims, ptr, n_epochs=epochs, seed=0)
        walls.append(time.perf_counter() - t0)
        for f in FAMILIES:
            v, calls = eng.kernel_time(f)
            ms[f].append(v / max(calls, 1))
    att, draws = ur.schedule_counts(g[0], g[2], epochs)
    lay = median(ms["umap_layout"])
    row = {"input": tag, "cells": n, "dims": dims, "n_neighbors": nn, "epochs": epochs, "reps": REPS,
           "nnz": int(g[0][-1]), "longest_row": int(np.diff(g[0]).max()), "wall_s": median(walls), "wall_s_all": walls,
           "same_bits": bool(np.array_equal(y, again)), "attractions": att, "draws": draws,
           "interactions_per_s": (att + draws) / lay * 1e3}
    for f in FAMILIES:
        row[f + "_ms"] = median(ms[f])
    if host_reference:
        x16 = t.cpu().numpy()
        init = x16[:, :2] * (10.0 / np.abs(x16[:, :2]).max())
        t0 = time.perf_counter()
        ref = ur.layout(g[0], g[1], g[2], init, n_epochs=epochs, seed=0)
        row["reference_layout_wall_s"] = time.perf_counter() - t0
        row["reference_finite"] = bool(np.all(np.isfinite(ref)))
        row["fused_faster_than_reference"] = bool(row["wall_s"] < row["reference_layout_wall_s"])
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


def markdown(rows, rounding, quality, epochs):
    out = ["# UMAP on the engine: graph and layout from the PCA scores", "",
           "Written by `scripts/umap_bench.py`.  No `umap`, `uwot` or `umap-learn` package was available: nothing here",
           "compares with them.  The host route is `tests/umap_reference.py`, the NumPy restatement of the same rules.", ""]
    if rounding:
        out += ["## What the layout tests' bound rests on (host)", "",
                "`tests/test_gpu_umap.py` compares the device layout with the float64 reference after 1, 2 and 10 epochs",
                "and allows 100 times the largest deviation between the float64 reference and the same reference in",
                "`np.longdouble`, but no less than 1e-12 of the layout's extent; it measures that deviation itself, on",
                "the device's own graph.  The same measurement on the host's exact tables of the same points:", "",
                "| graph | epochs | float64 - longdouble | extent | bound |", "|---|---|---|---|---|"]
        out += [f"| {r['graph']} | {r['epochs']} | {r['rounding']:.3g} | {r['extent']:.3g} | {r['bound']:.3g} |"
                for r in rounding]
        out += ["", "The deviation grows by orders of magnitude per epoch where two points come close (the repulsion's",
                "coefficient reaches 2 b / 0.001 per unit of distance), which is why the bound is measured per case and",
                "not fixed.", ""]
    if quality:
        tr = [r["trustworthiness"] for r in quality if r["seed"] != "init"]
        pu = [r["purity"] for r in quality if r["seed"] != "init"]
        out += ["## The reference's quality at 3,000 blob points over five seeds (host)", "",
                "6 blobs in 8 dimensions, n_neighbors = 15, 200 epochs, PCA initialisation; trustworthiness is sklearn's",
                "at k = 15, purity the share of a point's 15 nearest 2-D neighbours that carry its label.", "",
                "| seed | trustworthiness | purity |", "|---|---|---|"]
        out += [f"| {r['seed']} | {r['trustworthiness']:.5f} | {r['purity']:.5f} |" for r in quality]
        out += ["", f"Spread over the seeds: trustworthiness {max(tr) - min(tr):.5f}, purity {max(pu) - min(pu):.5f}.  The",
                "200-epoch device test allows the device these margins (0.0014 and 0) below the reference's values on",
                "the same graph and seed.", ""]
    if rows:
        out += ["## Device timings", "",
                f"One MI355X, `scc_umap_scores` with n_epochs = {epochs}, negative_sample_rate = 5, default initialisation;",
                f"medians of {REPS} calls after a warm-up call.  Wall: the fused call with the copy of its N x 2 result.",
                "Kernel ms: the call's three timer families.  Interactions: the attractions and draws of the run,",
                "counted from the schedule on the host, over the layout's kernel time.", "",
                "| input | cells | dims | n_neighbors | nnz | longest row | wall s | knn ms | graph ms | layout ms | "
                "interactions | interactions / s | same bits twice |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            out.append(f"| {r['input']} | {r['cells']} | {r['dims']} | {r['n_neighbors']} | {r['nnz']} | "
                       f"{r['longest_row']} | {r['wall_s']:.4f} | {r['knn_scores_ms']:.3f} | {r['umap_graph_ms']:.3f} | "
                       f"{r['umap_layout_ms']:.3f} | {r['attractions'] + r['draws']} | {r['interactions_per_s']:.3g} | "
                       f"{r['same_bits']} |")
        out.append("")
        for r in rows:
            if "reference_layout_wall_s" in r:
                out += [f"The speed condition, at {r['input']}: the fused call (k-NN, graph and layout) takes "
                        f"{r['wall_s']:.4f} s; the NumPy reference's layout alone, on the same graph, initialisation and "
                        f"epochs with {HOST_THREADS} host threads allowed, takes {r['reference_layout_wall_s']:.1f} s "
                        f"({r['reference_layout_wall_s'] / r['wall_s']:.0f} times as long).", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="A,B")
    ap.add_argument("--blobs", default="200000")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap_layout.md"))
    a = ap.parse_args()
    rounding = quality = rows = None
    if not a.no_host:
        rounding, quality = rounding_rows(), quality_rows()
    if not a.no_device:
        os.environ["SCC_PROFILE_STAGES"] = ",".join(FAMILIES)
        import torch
        from scconsensus_amd import _native as nat
        torch.cuda.init()  # torch holds the scores: its runtime starts before the engine's first call
        eng = nat.Engine(0, profile=True)
        rows = []
        for cfg in [c for c in a.configs.split(",") if c]:
            n, t = config_scores(eng, torch, cfg)
            rows.append(measure(eng, f"config {cfg}", n, t, 8, 15, a.epochs, cfg == "B"))
            del t
        for n in [int(v) for v in a.blobs.split(",") if v]:
            p = np.zeros((n, 16))
            p[:, :15] = wv.blobs(n)
            t = torch.tensor(p, device="cuda")
            rows.append(measure(eng, "blobs", n, t, 0, 15, a.epochs, False))
            del t
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(rows, rounding, quality, a.epochs))
    print(a.out)
    slow = [r for r in rows or [] if r.get("fused_faster_than_reference") is False]
    assert not slow, "the fused call is not faster than the NumPy reference at config B"


if __name__ == "__main__":
    main()
