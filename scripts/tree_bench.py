"""Time the tree + cut stage both ways on one machine in one session:

  host route    scc_distance to a host buffer, scc_hclust_ward_d2, four
                scc_cutree_hybrid (deepSplit 1..4)
  device route  scc_distance engine-kept, scc_hclust_ward_d2_dev (expand +
                chain), four scc_cutree_hybrid_dev

and write the table to a markdown file (default profiles/hclust_device.md)
with the hclust_dev kernel time, the scans per merge and the chain kernel's
achieved bytes/s.  Usage: tree_bench.py [--configs A,B] [--reps-a 3] [--out F]
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


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and \
        all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def run(cfg, reps):
    d = synth.generate(cfg)
    N = d.N
    names, code = api.select_clusters(d.labels, MCS)
    eng = nat.Engine(0)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    union = eng.de_run(ds, code, len(names), nat.SCC_DE_FAST, fetch="union").union
    device_route(eng, ds, union, N)  # warm-up: code objects, workspace, pinned buffers
    host, dev = [], []
    identical = True
    for _ in range(reps):  # alternating
        th, rh = host_route(eng, ds, union, N)
        td, rd = device_route(eng, ds, union, N)
        host.append(th)
        dev.append(td)
        identical = identical and same(rh, rd)
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
                host_all=[r["total_s"] for r in host], device_all=[r["total_s"] for r in dev],
                hclust_dev_ms=chain_ms, chain_launches=int(launches), hclust_expand_ms=expand_ms,
                scans=int(scans), scans_per_merge=scans / (N - 1), chain_bytes=chain_bytes,
                chain_GBps=chain_bytes / chain_ms / 1e6,
                expand_GBps=(8.0 * N * (N - 1) / 2 + 8.0 * N * N) / expand_ms / 1e6)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="A,B")
    ap.add_argument("--reps-a", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hclust_device.md"))
    a = ap.parse_args()
    rows = []
    for cfg in a.configs.split(","):
        r = run(cfg, a.reps_a if cfg == "A" else 1)
        print(json.dumps(r), flush=True)
        rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(rows))


if __name__ == "__main__":
    main()
