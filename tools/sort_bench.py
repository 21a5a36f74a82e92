#!/usr/bin/env python3
"""sort_bench.py — the time of sbam_sort_records (the coordinate sort's GPU passes) on one MI355X.

    python tools/sort_bench.py [--size-gb 10] [--read-len 150 | --read-len 0] [--repeats 5] [--no-torch]

The synthetic file of tools/synth.py (bench.py's generator: --read-len 150 Illumina-like, --read-len 0 the long-read
config) resident in HBM: full check, load_records(use_success_bitmap=True), then --repeats sorts of the loaded records.
Prints ONE JSON line:

* `sort_ms`, `sort_keys_ms`: the "sort" and "sort_keys" device times (sbam_last_kernel_ms: the whole call, the host's
  read of the histograms included; its keys and histograms), the medians of --repeats sorts after one untimed sort
  that allocates, all of them in `sort_ms_runs`;
* `passes`, `n_out_of_order`: sbam_sort_records' totals; `records_per_s` = records / `sort_ms`;
* `torch_sort_ms`: torch.sort(keys, stable=True) over the same keys as int64 (the sign bit flipped, so that the signed
  order is the keys' unsigned one) on the same device, CUDA events around the call, the median of --repeats after one
  untimed call; `parity`: torch's indices equal the library's order;
* `floor_ms` = passes x 2 x 16 B x records at `hbm_copy_peak` (tools/hbm_peak.hip, measured in this process after the
  sorts), and `ratio` = floor_ms / (sort_ms - sort_keys_ms): what share of the passes' time the traffic floor explains.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "spark-bam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from fields_bench import copy_peak, log  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=10.0, help="compressed GB")
    ap.add_argument("--read-len", type=int, default=150, help="0 = the long-read config")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--split-mb", type=float, default=2.0)
    ap.add_argument("--tile-mb", type=float, default=64.0)
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x5EEDBA11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.sort comparison")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    a = ap.parse_args()
    torch = None
    if not a.no_torch:  # (first: torch and libsbam.so then share one HIP runtime)
        import torch
        torch.cuda.set_device(a.device)
    import sbam
    import synth
    t0 = time.perf_counter()
    s = synth.SynthBam.for_size(int(a.size_gb * 1e9), tile_mb=a.tile_mb, seed=a.seed, threads=a.threads,
                                read_len=a.read_len, distinct=a.tiles > 1, cycle=max(a.tiles, 1))
    data = s.bytes()
    log(f"[sort_bench] {data.size / 1e9:.2f} GB, {s.n_records} records, generated in {time.perf_counter() - t0:.1f}s")
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        c = f.check_full_counts(0, f.uncompressed_size)
        _, cols = f.load_records(int(a.split_mb * (1 << 20)), use_success_bitmap=True, columns=("ref_id", "pos"))
        n = f.n_loaded
        if not (n == s.n_records == c.n_success):
            raise SystemExit(f"records: loaded {n}, generated {s.n_records}, checker {c.n_success}")
        totals = f.sort_records()  # (untimed: allocates the sort's buffers)
        runs, keys_runs = [], []
        for _ in range(a.repeats):
            f.sort_records()
            runs.append(f.kernel_ms("sort"))
            keys_runs.append(f.kernel_ms("sort_keys"))
        order = f.sort_order()
    keys = (cols["ref_id"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        (cols["pos"].view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    del cols
    torch_ms, parity = None, None
    if torch is not None:
        tk = torch.from_numpy((keys ^ np.uint64(1 << 63)).view(np.int64)).to(f"cuda:{a.device}")
        tr = []
        for k in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, idx = torch.sort(tk, stable=True)
            e1.record()
            torch.cuda.synchronize()
            if k:
                tr.append(e0.elapsed_time(e1))
        torch_ms = float(np.median(tr))
        parity = bool(np.array_equal(idx.cpu().numpy(), order))
        del tk, idx
        torch.cuda.empty_cache()
        if not parity:
            raise SystemExit("parity: torch.sort(stable=True) and sbam_sort_records give different orders")
    else:
        below = int((keys[1:] < keys[:-1]).sum())
        if below != totals["n_out_of_order"] or bool((keys[order][1:] < keys[order][:-1]).any()):
            raise SystemExit("parity: the order does not sort the keys, or the out-of-order count differs")
    peak = copy_peak(a.device)
    ms, kms = float(np.median(runs)), float(np.median(keys_runs))
    floor_ms = totals["passes"] * 2 * 16 * n / (peak * 1e9) * 1e3
    print(json.dumps({
        "metric": "sbam_sort_records device ms (coordinate sort: keys, histograms, radix passes)",
        "read_len": a.read_len, "file_gb": round(data.size / 1e9, 3), "records": n,
        "sort_ms": round(ms, 3), "sort_ms_runs": [round(x, 3) for x in runs], "sort_keys_ms": round(kms, 3),
        "passes": totals["passes"], "n_out_of_order": totals["n_out_of_order"],
        "records_per_s": round(n / (ms * 1e-3)), "torch_sort_ms": None if torch_ms is None else round(torch_ms, 3),
        "hbm_copy_peak": round(peak, 1), "floor_ms": round(floor_ms, 3),
        "ratio": round(floor_ms / max(ms - kms, 1e-9), 3), "parity": {"ok": True, "torch": parity}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
