#!/usr/bin/env python3
"""index_bench.py — the time of sbam_build_index (the BAI writer's GPU pass) on one MI355X.

    python tools/index_bench.py [--size-gb 10] [--read-len 150 | --read-len 0] [--repeats 5]

The synthetic file of tools/synth.py (bench.py's generator: --read-len 150 Illumina-like, --read-len 0 the long-read
config) resident in HBM: full check, load_records(use_success_bitmap=True), load_record_fields over the whole file in
batches (for scale), then --repeats builds of the index on the loaded columns.  Prints ONE JSON line:

* `index_ms`: the "index" device time of a build (sbam_last_kernel_ms: the first pass through the linear index's
  fill, the host's read of the counters between the passes included; the median of --repeats builds after one untimed
  build that allocates, all of them in `index_ms_runs`);
* `write_bai_ms`: wall time of sbam_write_bai (runs, linear index and metadata to the host, then the assembly);
  `assemble_ms`: wall time of sbam_bai_assemble alone on host arrays; `bai_bytes` the result's size;
* `load_records_ms`, `record_fields_ms`: the device times of the same run's record decode and field gather;
* `bytes_min`: 40 B of columns per record plus its CIGAR ops, what the pass has to read at least; `gbps` = that /
  `index_ms`; `hbm_copy_peak` (tools/hbm_peak.hip, measured in this process after the builds) and `ratio` = gbps / it;
* `totals`: sbam_build_index's; `parity`: every record is counted once (mapped + unmapped + without coordinates), the
  bytes parse, and a second assembly from the copied-out arrays gives the same bytes.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "spark-bam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from fields_bench import batches, copy_peak, log  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=10.0, help="compressed GB")
    ap.add_argument("--read-len", type=int, default=150, help="0 = the long-read config")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-gb", type=float, default=4.0, help="record bytes per load_record_fields call")
    ap.add_argument("--split-mb", type=float, default=2.0)
    ap.add_argument("--tile-mb", type=float, default=64.0)
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x5EEDBA11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    a = ap.parse_args()
    import sbam
    import synth
    from sbam import bai
    t0 = time.perf_counter()
    s = synth.SynthBam.for_size(int(a.size_gb * 1e9), tile_mb=a.tile_mb, seed=a.seed, threads=a.threads,
                                read_len=a.read_len, distinct=a.tiles > 1, cycle=max(a.tiles, 1))
    data = s.bytes()
    log(f"[index_bench] {data.size / 1e9:.2f} GB, {s.n_records} records, generated in {time.perf_counter() - t0:.1f}s")
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        c = f.check_full_counts(0, f.uncompressed_size)
        split = int(a.split_mb * (1 << 20))
        _, cols = f.load_records(split, use_success_bitmap=True, columns=("block_size",))
        load_ms = f.kernel_ms("load_records")
        n = f.n_loaded
        if not (n == s.n_records == c.n_success):
            raise SystemExit(f"records: loaded {n}, generated {s.n_records}, checker {c.n_success}")
        fields_ms, cigar_ops = 0.0, 0
        for i0, k in batches(cols["block_size"], int(a.batch_gb * 1e9)):
            rf = f.load_record_fields(i0, k, host=False)
            fields_ms += f.kernel_ms("record_fields")
            cigar_ops += rf.totals["cigar_ops"]
        del cols
        totals = f.build_index(split)  # (untimed: allocates the index's buffers)
        runs = []
        for _ in range(a.repeats):
            f.build_index(split)
            runs.append(f.kernel_ms("index"))
        out = f.build_bai(split, require_sorted=False)  # (builds once more; write_bai alone is timed below)
        nb = ctypes.c_int64(0)
        buf = np.zeros(len(out), np.uint8)
        t = time.perf_counter()
        f._check(f.L.sbam_write_bai(f.ctx, buf.ctypes.data, buf.size, ctypes.byref(nb)))
        write_ms = (time.perf_counter() - t) * 1e3
        r = f.index_refs()
        rr = f.index_runs()
        t = time.perf_counter()
        out2 = sbam.bai_assemble(totals["n_ref"], rr, r.intv_off, r.ioffset, r.off_beg, r.off_end, r.n_mapped,
                                 r.n_unmapped, r.n_no_coor)
        assemble_ms = (time.perf_counter() - t) * 1e3 / 2  # (bai_assemble sizes, then writes: two assemblies)
        counted = int(r.n_mapped.sum() + r.n_unmapped.sum()) + r.n_no_coor
        ok = counted == n == totals["n_records"] and out2 == out == buf.tobytes() and len(bai.parse_bai(out)) == totals["n_ref"]
        ok &= bai.parse_n_no_coor(out) == r.n_no_coor
        if not ok:
            raise SystemExit(f"parity: {counted} records counted of {n}, or the assembled bytes differ")
    peak = copy_peak(a.device)
    ms = float(np.median(runs))
    bytes_min = 40 * n + 4 * cigar_ops
    gbps = bytes_min / (ms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "sbam_build_index device ms (BAI writer: spans, runs, linear index, metadata)",
        "read_len": a.read_len, "file_gb": round(data.size / 1e9, 3), "records": n, "cigar_ops": cigar_ops,
        "index_ms": round(ms, 3), "index_ms_runs": [round(x, 3) for x in runs],
        "write_bai_ms": round(write_ms, 3), "assemble_ms": round(assemble_ms, 3), "bai_bytes": len(out),
        "load_records_ms": round(load_ms, 3), "record_fields_ms": round(fields_ms, 3),
        "bytes_min": bytes_min, "gbps": round(gbps, 1), "hbm_copy_peak": round(peak, 1),
        "ratio": round(gbps / peak, 3), "totals": totals, "parity": {"ok": True}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
