"""bench.py's plain line and --dump-outputs (what the last timed step returned, as DIR/<name>.npy).

CPU: dump_outputs writes every ShardResult field exactly, in float64, rank rows concatenated behind the merged
Counts.  GPU: one small plain run prints the headline keys only, times --steps steps, and dumps split rows that add
up to the generator's record count; the extras are in the line only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADLINE = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "uncompressed_gbps", "kernel_ms"]
FULL_ONLY = ["roofline", "stage_rooflines", "hbm_copy_peak", "e2e_h2d", "cpu_baseline", "parity"]
FIELDS = ("first_block_pos", "first_offset", "nonempty", "n_records")


def test_dump_outputs_writes_every_field_exactly(tmp_path):
    import bench
    from sbam import dist as sdist
    rng = np.random.default_rng(7)
    parts = []
    for k in (3, 5):  # two ranks' rows; values past 2^32 (block positions of a 10 GB file, Counts of 27e9 offsets)
        parts.append(sdist.ShardResult(rng.integers(0, 1 << 40, sdist.N_COUNT_WORDS),
                                       *(rng.integers(0, 1 << 40, k) for _ in FIELDS)))
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), parts)
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in ("counts",) + FIELDS)
    got = np.load(out / "counts.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int64), parts[0].counts)
    for n in FIELDS:
        got = np.load(out / (n + ".npy"))
        assert got.dtype == np.float64 and got.shape == (8,)
        assert np.array_equal(got.astype(np.int64), np.concatenate([getattr(p, n) for p in parts]))


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size-gb", "0.05", "--tile-mb", "8",
           "--tiles", "1", "--steps", "2", "--warmup", "1", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_last_step(tmp_path):
    line, err = run_bench("--dump-outputs", str(tmp_path / "d"))
    assert list(line) == HEADLINE
    assert line["steps"] == 2 and err.count("] step ") == 2  # --steps sets the number of timed steps
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value is file bytes / step time; file_gb is rounded to 1e-3 of ~0.05 (1 %), ms_per_step to 1e-3 ms
    assert line["value"] == pytest.approx(line["config"]["file_gb"] / (line["ms_per_step"] * 1e-3), rel=2e-2)
    d = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in ("counts",) + FIELDS}
    assert all(a.dtype == np.float64 for a in d.values())
    from sbam import dist as sdist
    assert d["counts"].shape == (sdist.N_COUNT_WORDS,)
    assert int(d["n_records"].sum()) == line["config"]["records"]
    assert sdist.unpack_counts(d["counts"].astype(np.int64))["n_success"] == line["config"]["records"]
    assert bool(d["nonempty"].all()) and np.all(np.diff(d["first_block_pos"]) > 0)


@pytest.mark.gpu
def test_full_run_adds_the_extras():
    line, _ = run_bench("--full", "--cpu-sample-mb", "20", "--e2e-windows", "2", "--e2e-steps", "1")
    assert list(line)[:len(HEADLINE)] == HEADLINE
    assert all(k in line for k in FULL_ONLY)
    assert line["parity"]["ok"] is True and line["e2e_h2d"]["parity_ok"] is True
    assert line["cpu_baseline"]["value"] > 0 and line["hbm_copy_peak"]["value"] > 0
