"""Time the FAST DE stage for each test.use value the engine runs (wilcox, t,
bimod): eng.de_run(..., fetch="union") on bench.py's config-B input, the three
tests alternating inside every round so that drift of a shared host hits them
alike.  A call ends in a device synchronisation (the union comes back to the
host), so the host clock around it is the call time; the median over the
rounds is reported, with the per-stage split of a separate profiled engine
(opts.profile: HIP events around each stage, which slow the host and are kept
out of the timed rounds).

    python scripts/de_test_bench.py [--config B] [--steps 30] [--warmup 5]
                                    [--lib other/libscc.so] [--out file.json]

--lib times another build of the library (e.g. the parent commit's) with this
tree's Python layer; tests that build does not know are reported as null.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ["ingest", "gene_stats", "pair_filter", "gene_rank", "pair_test", "pair_select"]
TESTS = ["wilcox", "t", "bimod"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: at least 20 timed rounds")

    import bench
    from scconsensus_amd import _native as nat
    from scconsensus_amd import api
    from scconsensus_amd.synth import CONFIGS
    if a.lib:
        nat.LIB_PATH = os.path.abspath(a.lib)
    d = bench.host_dataset(a.config, CONFIGS[a.config]["seed"])
    names, code = api.select_clusters(d.labels, 10)
    K = len(names)

    def run(eng, ds, test):
        return eng.de_run(ds, code, K, nat.SCC_DE_FAST, fetch="union", test=test)

    eng = nat.Engine(0)
    ds = eng.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    tests, unions = [], {}
    for t in TESTS:
        try:
            unions[t] = int(len(run(eng, ds, t).union))
            tests.append(t)
        except nat.SccError as e:  # an older --lib build without this test
            if e.code != nat.SCC_ERR_INVALID:
                raise
    for _ in range(a.warmup):
        for t in tests:
            run(eng, ds, t)
    ms = {t: [] for t in tests}
    for _ in range(a.steps):
        for t in tests:
            eng.synchronize()
            t0 = time.perf_counter()
            run(eng, ds, t)
            ms[t].append((time.perf_counter() - t0) * 1e3)
    ds.close()
    eng.close()

    prof = nat.Engine(0, profile=True)
    dp = prof.dataset_csc(d.indptr, d.indices, d.data, d.G, d.N)
    stage_ms = {}
    for t in tests:
        for _ in range(a.warmup):
            run(prof, dp, t)
        prof.synchronize()
        prof.reset_timers()
        for _ in range(a.steps):
            run(prof, dp, t)
        stage_ms[t] = {s: round(prof.kernel_time(s)[0] / a.steps, 4) for s in STAGES}
    dp.close()
    prof.close()

    def row(t):
        if t not in ms:
            return None
        v = sorted(ms[t])
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4),
                "p90_ms": round(v[int(0.9 * (len(v) - 1))], 4), "union": unions[t], "stage_ms": stage_ms[t]}

    out = {"config": a.config, "genes": d.G, "cells": d.N, "clusters": K, "nnz": int(len(d.data)),
           "steps": a.steps, "warmup": a.warmup, "call": 'de_run(SCC_DE_FAST, fetch="union")',
           "lib": os.path.relpath(nat.LIB_PATH, ROOT), "tests": {t: row(t) for t in TESTS}}
    if "t" in ms and "bimod" in ms:
        out["bimod_over_t"] = round(out["tests"]["bimod"]["median_ms"] / out["tests"]["t"]["median_ms"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
