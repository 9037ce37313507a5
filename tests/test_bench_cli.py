"""bench.py's command line: a plain run keeps to the headline figure (`--full`
adds the side measurements), `--dump-outputs` writes the last timed step's
outputs within its size budget, and the cached host input is the generator's
output bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from scconsensus_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_skips_side_measurements():
    a = bench._args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.steps == 3 and a.warmup == 1 and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_pearson and a.no_transfers


def test_full_keeps_the_switches():
    a = bench._args(["--full"])
    assert a.full and not (a.no_cpu_baseline or a.no_pearson or a.no_transfers)
    a = bench._args(["--full", "--no-pearson", "--dump-outputs", "x"])
    assert a.no_pearson and not a.no_transfers and a.dump_outputs == "x"


def test_dump_outputs_small_arrays_whole(tmp_path):
    arrays = {"union": np.arange(7, dtype=np.int32), "m": np.arange(12.0).reshape(3, 4)}
    bench.dump_outputs(str(tmp_path / "o"), arrays)
    assert sorted(os.listdir(tmp_path / "o")) == ["m.npy", "union.npy"]
    u = np.load(tmp_path / "o" / "union.npy")
    assert u.dtype == np.float64 and np.array_equal(u, np.arange(7.0))
    assert np.array_equal(np.load(tmp_path / "o" / "m.npy"), arrays["m"])


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 200)
    big = np.random.default_rng(0).normal(size=(50, 40))
    arrays = {"big": big, "small": np.arange(10.0)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.shape == (100,) and np.isin(s, big).all()
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 8 * 200 + 2 * 128  # the payload within the budget (+ the .npy headers)
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))  # the same sample every time


def test_host_dataset_cache_bitwise(tmp_path, monkeypatch):
    calls = []
    gen = synth.generate

    def small(name, seed=None):
        calls.append(seed)
        return gen(name, G=150, N=240, K=4, seed=seed)

    monkeypatch.setattr(synth, "generate", small)
    monkeypatch.setattr(bench, "INPUT_CACHE", str(tmp_path / "cache"))
    d0 = bench.host_dataset("A", 7)
    d1 = bench.host_dataset("A", 7)
    assert calls == [7] and len(os.listdir(tmp_path / "cache")) == 1
    assert (d1.G, d1.N) == (d0.G, d0.N)
    for f in ("indptr", "indices", "data"):
        x0, x1 = getattr(d0, f), getattr(d1, f)
        assert x0.dtype == x1.dtype and np.array_equal(x0, x1), f
    assert d1.labels.dtype == object and list(d1.labels) == list(d0.labels)
    assert d1.gene_names == d0.gene_names and d1.cell_names == d0.cell_names
    bench.host_dataset("A", 8)  # another seed: another entry
    assert calls == [7, 8] and len(os.listdir(tmp_path / "cache")) == 2


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    """One plain config-A run: the result line carries the headline fields and
    none of the side measurements; the dump holds the last step's DE union,
    the PCA scores and the silhouette widths over the engine-kept distance."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "A", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "cell-pairs/s" and r["dtype"] == "f64"
    assert r["higher_is_better"] is True
    N = r["config"]["cells"]
    assert r["value"] == pytest.approx(N * (N - 1) / 2 / (r["ms_per_step"] / 1e3), rel=1e-12)
    assert "cpu_baseline" not in r and "cold_call_ms" not in r and "pearson" not in r["stage_ms"]
    assert set(r["end_to_end_ms"]) == {"hbm_resident", "value_uses"}
    assert sorted(os.listdir(out)) == ["dist_silhouette_widths.npy", "pca_scores.npy", "union.npy"]
    u, s, w = (np.load(out / f) for f in ("union.npy", "pca_scores.npy", "dist_silhouette_widths.npy"))
    assert u.dtype == s.dtype == w.dtype == np.float64
    assert len(u) == r["config"]["union"] and np.all(np.diff(np.sort(u)) > 0) and u.min() >= 0
    assert u.max() < r["config"]["genes"]
    assert s.shape == (N, 15) and np.isfinite(s).all() and np.abs(s.sum(0)).max() < 1e-6 * np.abs(s).max() * N
    assert w.shape == (N,) and np.isfinite(w).all() and np.abs(w).max() <= 1.0
