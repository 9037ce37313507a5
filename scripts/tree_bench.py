"""Time the tree + cut stage three ways on one machine in one session:

  host route    scc_distance to a host buffer, scc_hclust_ward_d2, four
                scc_cutree_hybrid (deepSplit 1..4)
  device route  scc_distance engine-kept, scc_hclust_ward_d2_dev (expand +
                chain), four scc_cutree_hybrid_dev
  scores route  scc_pca_scores, scc_hclust_ward_d2_scores, four
                scc_cutree_hybrid_scores (no distance at all)

and write two tables: host against device (default profiles/hclust_device.md)
with the hclust_dev kernel time, the scans per merge and the chain kernel's
achieved bytes/s, and all three routes (default profiles/hclust_scores.md)
with the scores route's time per scan beside k_hc_chain's and, for shapes the
matrix routes cannot hold (--blobs), the scores route alone on seeded blob
points.  Usage: tree_bench.py [--configs A,B] [--reps-a 3] [--blobs 200000]
[--out F] [--scores-out F]
"""
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

DEEP_SPLITS = (1, 2, 3, 4)
MCS = 10
# one CU's streaming rate by where the rows are served from (microarchitecture
# notes, indexed-row gathers by one workgroup per CU): HBM sweep .. the XCD's L2
ONE_CU_GBPS = (23.0, 73.0)
# the scores route against the other two (tests/test_ward_vector_reference.py)
HEIGHT_RTOL = 1e-12
MIN_GAP = 1e-9


def host_route(eng, ds, union, N):
    t0 = time.perf_counter()
    dist = eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID)
    t1 = time.perf_counter()
    m, h, o = nat.hclust_ward_d2(dist, N)
    t2 = time.perf_counter()
    labs = [nat.cutree_hybrid(m, h, dist, k, MCS)[0] for k in DEEP_SPLITS]
    t3 = time.perf_counter()
    return dict(dist_s=t1 - t0, hclust_s=t2 - t1, cuts_s=t3 - t2, total_s=t3 - t0), (m, h, o, labs)


def device_route(eng, ds, union, N):
    t0 = time.perf_counter()
    eng.distance(ds, union, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0)
    eng.synchronize()
    t1 = time.perf_counter()
    m, h, o = eng.hclust_ward_d2_dev(N)
    t2 = time.perf_counter()
    labs = [eng.cutree_hybrid_dev(m, h, k, MCS)[0] for k in DEEP_SPLITS]
    t3 = time.perf_counter()
    return dict(dist_s=t1 - t0, hclust_s=t2 - t1, cuts_s=t3 - t2, total_s=t3 - t0), (m, h, o, labs)


def scores_route(eng, ds, union, N):
    """(dist_s is the PCA alone: this route computes no distance)"""
    t0 = time.perf_counter()
    eng.pca_scores(ds, union)
    t1 = time.perf_counter()
    m, h, o = eng.hclust_ward_d2_scores(N)
    t2 = time.perf_counter()
    labs = [eng.cutree_hybrid_scores(m, h, k, MCS)[0] for k in DEEP_SPLITS]
    t3 = time.perf_counter()
    return dict(dist_s=t1 - t0, hclust_s=t2 - t1, cuts_s=t3 - t2, total_s=t3 - t0, scans=eng.hclust_last_scans()), \
        (m, h, o, labs)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and \
        all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def min_gap(h):
    return float(np.min(np.diff(h) / h[1:])) if len(h) > 1 else float("inf")


def same_within(sc, host):
    """The scores route against the host route: merge, order and labels
    equal, heights within HEIGHT_RTOL; (ok, worst relative height error)."""
    rel = float(np.max(np.abs(sc[1] - host[1]) / host[1]))
    ok = np.array_equal(sc[0], host[0]) and np.array_equal(sc[2], host[2]) and rel <= HEIGHT_RTOL and \
        all(np.array_equal(x, y) for x, y in zip(sc[3], host[3]))
    return bool(ok), rel


def run(cfg, reps):
    d = synth.generate(cfg)
    N = d.N
    names, code = api.select_clusters(d.labels, MCS)
    eng = nat.Engine(0)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    device_route(eng, ds, union, N)  # warm-up: code objects, workspace, pinned buffers
    scores_route(eng, ds, union, N)
    host, dev, sco = [], [], []
    identical = True
    scores_ok, worst_rel, gap = True, 0.0, float("inf")
    for _ in range(reps):  # alternating
        th, rh = host_route(eng, ds, union, N)
        td, rd = device_route(eng, ds, union, N)
        ts, rs = scores_route(eng, ds, union, N)
        host.append(th)
        dev.append(td)
        sco.append(ts)
        identical = identical and same(rh, rd)
        ok, rel = same_within(rs, rh)
        scores_ok = scores_ok and ok
        worst_rel = max(worst_rel, rel)
        gap = min(gap, min_gap(rh[1]))
    eng.close()
    # kernel times in a run of their own (timing events around every launch)
    prof = nat.Engine(0, profile=True)
    dsp = prof.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    prof.distance(dsp, union, nat.SCC_DIST_PCA_EUCLID, device_out_ptr=0)
    prof.synchronize()
    prof.reset_timers()
    prof.hclust_ward_d2_dev(N)
    chain_ms, launches = prof.kernel_time("hclust_dev")
    expand_ms, _ = prof.kernel_time("hclust_expand")
    scans = prof.hclust_last_scans()
    prof.close()
    # bytes the chain needs, from the shapes (an upper bound: removed nodes'
    # entries are skipped): a scan reads one row and the flags; a merge reads
    # two rows, the sizes and the flags and writes a row and a column
    chain_bytes = scans * 9.0 * N + (N - 1) * 41.0 * N
    med = lambda rows, k: float(np.median([r[k] for r in rows]))  # noqa: E731
    return dict(config=cfg, cells=N, union=int(len(union)), reps=reps, identical=bool(identical),
                host={k: med(host, k) for k in host[0]}, device={k: med(dev, k) for k in dev[0]},
                scores={k: med(sco, k) for k in sco[0]},
                host_all=[r["total_s"] for r in host], device_all=[r["total_s"] for r in dev],
                scores_all=[r["total_s"] for r in sco],
                scores_same_tree=bool(scores_ok), scores_worst_height_rel=worst_rel, host_min_gap=gap,
                gap_condition=bool(gap >= MIN_GAP),
                hclust_dev_ms=chain_ms, chain_launches=int(launches), hclust_expand_ms=expand_ms,
                scans=int(scans), scans_per_merge=scans / (N - 1), chain_bytes=chain_bytes,
                chain_GBps=chain_bytes / chain_ms / 1e6,
                expand_GBps=(8.0 * N * (N - 1) / 2 + 8.0 * N * N) / expand_ms / 1e6)


def blob_points(n, seed):
    """Seeded Gaussian blobs in 15 dimensions as [n][16] scores (the recipe of
    tests/ward_vector_reference.blobs with 50 centres)."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(scale=6.0, size=(50, 15))
    p = np.zeros((n, 16))
    p[:, :15] = centers[rng.integers(0, 50, n)] + rng.normal(size=(n, 15))
    return p


def valid_tree(m, h, o):
    n = len(o)
    used = m.reshape(-1)
    return bool(np.array_equal(np.sort(-used[used < 0]), np.arange(1, n + 1)) and
                np.array_equal(np.sort(used[used > 0]), np.arange(1, n - 1)) and
                np.all(np.isfinite(h)) and np.all(np.diff(h) >= 0) and
                np.array_equal(np.sort(o), np.arange(1, n + 1)))


def run_blobs(n):
    """The scores route alone on n blob points (no matrix route holds them)."""
    import torch
    eng = nat.Engine(0)
    free0 = torch.cuda.mem_get_info()[0]
    t = torch.tensor(blob_points(n, 4), device="cuda")
    torch.cuda.synchronize()
    eng.hclust_ward_d2_scores(min(n, 3000), t.data_ptr())  # warm-up: code objects
    t0 = time.perf_counter()
    m, h, o = eng.hclust_ward_d2_scores(n, t.data_ptr())
    t1 = time.perf_counter()
    scans = eng.hclust_last_scans()
    labs = [eng.cutree_hybrid_scores(m, h, k, MCS, t.data_ptr())[0] for k in DEEP_SPLITS]
    t2 = time.perf_counter()
    in_use = free0 - torch.cuda.mem_get_info()[0]  # the scores, the engine's workspace, the allocator's slack
    eng.close()
    return dict(cells=n, hclust_s=t1 - t0, cuts_s=t2 - t1, scans=int(scans), scans_per_merge=scans / (n - 1),
                us_per_scan=(t1 - t0) / scans * 1e6, scan_bytes=145.0 * n, scan_GBps=145.0 * n * scans / (t1 - t0) / 1e9,
                device_bytes_in_use=int(in_use), matrix_bytes=8.0 * n * n, valid=valid_tree(m, h, o),
                clusters=[int(len(np.unique(x[x > 0]))) for x in labs])


def markdown(rows):
    out = ["# Tree and cut: host route against device route", "",
           "Written by `scripts/tree_bench.py` on one MI355X host, both routes in one session, alternating.",
           "Host route: `scc_distance` to a host buffer, `scc_hclust_ward_d2`, four `scc_cutree_hybrid`",
           "(deepSplit 1-4, minClusterSize 10).  Device route: `scc_distance` engine-kept,",
           "`scc_hclust_ward_d2_dev` (expand + chain), four `scc_cutree_hybrid_dev`.  Wall seconds, medians",
           "over the repetitions; every run's trees and labels were compared.", "",
           "| config | cells | reps | route | dist | hclust | 4 cuts | total | all totals |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for name, key in (("host", "host"), ("device", "device")):
            t = r[key]
            out.append(f"| {r['config']} | {r['cells']} | {r['reps']} | {name} | {t['dist_s']:.4f} | {t['hclust_s']:.4f} | "
                       f"{t['cuts_s']:.4f} | {t['total_s']:.4f} | "
                       + " ".join(f"{v:.4f}" for v in r[key + "_all"]) + " |")
    out += ["", "| config | identical results | host / device total | hclust host / device |", "|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} | {r['identical']} | {r['host']['total_s'] / r['device']['total_s']:.1f}x | "
                   f"{r['host']['hclust_s'] / r['device']['hclust_s']:.1f}x |")
    out += ["", "Kernel times (timing events, a profiled run of its own):", "",
            "| config | hclust_expand ms | expand GB/s | hclust_dev ms | launches | scans | scans / merge | "
            "chain bytes (model) | chain GB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} | {r['hclust_expand_ms']:.3f} | {r['expand_GBps']:.0f} | {r['hclust_dev_ms']:.2f} | "
                   f"{r['chain_launches']} | {r['scans']} | {r['scans_per_merge']:.3f} | {r['chain_bytes'] / 1e9:.2f} GB | "
                   f"{r['chain_GBps']:.1f} |")
    out += ["", "Chain bytes are computed from the shapes, an upper bound (entries of removed nodes are skipped):",
            "`scans * 9 N + (N - 1) * 41 N` — a scan reads one row (8 N) and the active flags (N); a merge reads",
            "two rows, the sizes and the flags (25 N) and writes a row and a column (16 N; the column's stores are",
            f"one 8-byte word per 64-byte line).  One CU streams {ONE_CU_GBPS[0]:.0f}-{ONE_CU_GBPS[1]:.0f} GB/s depending on",
            "whether the rows come from HBM or from the XCD's L2 (measured row gathers by one workgroup per CU);",
            "the chain kernel is one workgroup on one CU.", ""]
    return "\n".join(out)


def markdown_scores(rows, blobs):
    out = ["# Tree and cut from the PCA scores against the two matrix routes", "",
           "Written by `scripts/tree_bench.py` on one MI355X host, the three routes in one session, alternating.",
           "Host route: `scc_distance` to a host buffer, `scc_hclust_ward_d2`, four `scc_cutree_hybrid`",
           "(deepSplit 1-4, minClusterSize 10).  Device route: `scc_distance` engine-kept, `scc_hclust_ward_d2_dev`,",
           "four `scc_cutree_hybrid_dev`.  Scores route: `scc_pca_scores` (its time stands in the dist column: no",
           "distance is computed), `scc_hclust_ward_d2_scores`, four `scc_cutree_hybrid_scores`.  Wall seconds,",
           "medians over the repetitions.", "",
           "| config | cells | reps | route | dist | hclust | 4 cuts | total | all totals |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for key in ("host", "device", "scores"):
            t = r[key]
            out.append(f"| {r['config']} | {r['cells']} | {r['reps']} | {key} | {t['dist_s']:.4f} | {t['hclust_s']:.4f} | "
                       f"{t['cuts_s']:.4f} | {t['total_s']:.4f} | "
                       + " ".join(f"{v:.4f}" for v in r[key + "_all"]) + " |")
    out += ["", "Every run's results were compared: device against host with `array_equal`; scores against host with",
            f"`merge`, `order` and the four label vectors equal and the heights within a relative {HEIGHT_RTOL:g}, under the",
            f"condition that the smallest relative gap between consecutive host heights is at least {MIN_GAP:g}.", "",
            "| config | device identical | smallest host gap | condition holds | scores: same tree and labels | "
            "worst relative height error |", "|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} | {r['identical']} | {r['host_min_gap']:.3g} | {r['gap_condition']} | "
                   f"{r['scores_same_tree']} | {r['scores_worst_height_rel']:.3g} |")
    out += ["", "Time per nearest-neighbour scan.  `k_hc_chain` (one workgroup, one row of the 8 N^2-byte matrix per scan):",
            "its kernel time from timing events over its scans, merges' updates included.  Scores route (two",
            "launches per scan, 145 N bytes: 16 centroid components, the size and the flag of every node): the wall",
            "time of `scc_hclust_ward_d2_scores` over its scans, batching and state reads included.", "",
            "| config | cells | scans (device) | k_hc_chain us / scan | scans (scores) | scores us / scan | bytes / scan | "
            "scores GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        s = r["scores"]
        us = s["hclust_s"] / s["scans"] * 1e6
        out.append(f"| {r['config']} | {r['cells']} | {r['scans']} | {r['hclust_dev_ms'] * 1e3 / r['scans']:.2f} | "
                   f"{int(s['scans'])} | {us:.2f} | {145 * r['cells'] / 1e6:.2f} MB | "
                   f"{145.0 * r['cells'] * s['scans'] / s['hclust_s'] / 1e9:.0f} |")
    if blobs:
        out += ["", "Shapes the matrix routes cannot hold: seeded Gaussian blob points (50 centres, 15 dimensions) as",
                "scores, the scores route alone.  The tree is checked for validity (every observation and every",
                "earlier row used once, heights finite and non-decreasing); there is nothing to compare it with.",
                "Device memory in use: the drop in free device memory from before the scores are uploaded to after",
                "the last cut (the scores, the engine's workspace, allocator slack).", "",
                "| cells | hclust s | 4 cuts s | scans | scans / merge | us / scan | bytes / scan | GB/s | device memory in use | "
                "8 N^2 working copy | valid tree | clusters per deepSplit |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for b in blobs:
            out.append(f"| {b['cells']} | {b['hclust_s']:.3f} | {b['cuts_s']:.3f} | {b['scans']} | {b['scans_per_merge']:.3f} | "
                       f"{b['us_per_scan']:.2f} | {b['scan_bytes'] / 1e6:.2f} MB | {b['scan_GBps']:.0f} | "
                       f"{b['device_bytes_in_use'] / 1e6:.0f} MB | {b['matrix_bytes'] / 1e9:.1f} GB | {b['valid']} | "
                       f"{' '.join(str(k) for k in b['clusters'])} |")
    out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="A,B")
    ap.add_argument("--reps-a", type=int, default=3)
    ap.add_argument("--blobs", default="200000", help="comma-separated cell counts for the scores route alone ('' for none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hclust_device.md"))
    ap.add_argument("--scores-out", default=os.path.join(ROOT, "profiles", "hclust_scores.md"))
    a = ap.parse_args()
    blob_sizes = [int(v) for v in a.blobs.split(",") if v]
    if blob_sizes:  # torch holds the blob scores: its runtime starts before the engine's first call
        import torch
        torch.cuda.init()
    rows = []
    for cfg in [c for c in a.configs.split(",") if c]:
        r = run(cfg, a.reps_a if cfg == "A" else 1)
        print(json.dumps(r), flush=True)
        rows.append(r)
    blobs = []
    for n in blob_sizes:
        b = run_blobs(n)
        print(json.dumps(b), flush=True)
        blobs.append(b)
    for path, text in ((a.out, markdown(rows)), (a.scores_out, markdown_scores(rows, blobs))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
