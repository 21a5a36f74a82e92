#!/usr/bin/env python3
"""fields_bench.py — the bandwidth of sbam_load_record_fields' gather on one MI355X.

    python tools/fields_bench.py [--size-gb 10] [--read-len 150 | --read-len 0] [--repeats 3] [--batch-gb 4]

The synthetic file of tools/synth.py (bench.py's generator: --read-len 150 Illumina-like, --read-len 0 the long-read
config) resident in HBM: full check, load_records(use_success_bitmap=True), then load_record_fields over the whole
file in batches of at most --batch-gb of record bytes, columns left on the device.  Prints ONE JSON line:

* `ms`: the summed "record_fields" device time of a pass over the file (sbam_last_kernel_ms; the median of --repeats
  passes, all of them in `ms_runs`), `sizes_ms` the sizes + scan time beside it;
* `bytes_read`: the variable-length bytes of the records (block_size - 32 each), `bytes_written`: the five columns;
  `gbps` = their sum / `ms`;
* `hbm_copy_peak` (tools/hbm_peak.hip, measured in this process after the passes) and `ratio` = gbps / that;
* `column_ms`: the same device time of one pass per column alone (where the time goes);
* `parity`: before the timed passes, every batch's totals equal its offset columns' last entries and the batches'
  record bytes, and the `qual` bytes of a sampled 1 % of the records (runs of 256) equal the stream slices.
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


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def copy_peak(device: int) -> float:
    """GB/s (read + write) of tools/hbm_peak.hip's 4 GiB device-to-device copy: bench.py's hbm_copy_peak."""
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "build", "libhbmpeak.so"))
    lib.hbm_copy_peak.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_double)]
    n, best = 4 << 30, None
    for nt in (0, 1):
        for grid in (2048, 8192, 32768):
            ms = ctypes.c_double(0.0)
            if lib.hbm_copy_peak(device, n, 10, grid, nt, ctypes.byref(ms)) == 0 and ms.value > 0:
                best = ms.value if best is None else min(best, ms.value)
    if best is None:
        raise RuntimeError("hbm_copy_peak failed")
    return 2 * n / (best * 1e-3) / 1e9


def batches(block_size: np.ndarray, cap_bytes: int):
    """(i0, n) runs of records holding at most cap_bytes of record bytes each (at least one record)."""
    ends = np.cumsum(block_size.astype(np.int64) + 4)
    out, i0, base = [], 0, 0
    while i0 < ends.size:
        i1 = max(int(np.searchsorted(ends, base + cap_bytes, side="right")), i0 + 1)
        out.append((i0, i1 - i0))
        base, i0 = int(ends[i1 - 1]), i1
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=10.0, help="compressed GB")
    ap.add_argument("--read-len", type=int, default=150, help="0 = the long-read config")
    ap.add_argument("--repeats", type=int, default=3)
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
    t0 = time.perf_counter()
    s = synth.SynthBam.for_size(int(a.size_gb * 1e9), tile_mb=a.tile_mb, seed=a.seed, threads=a.threads,
                                read_len=a.read_len, distinct=a.tiles > 1, cycle=max(a.tiles, 1))
    data = s.bytes()
    log(f"[fields_bench] {data.size / 1e9:.2f} GB, {s.n_records} records, generated in {time.perf_counter() - t0:.1f}s")
    rng = np.random.default_rng(a.seed & 0xffffffff)
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        L = f.uncompressed_size
        c = f.check_full_counts(0, L)
        sizes, cols = f.load_records(int(a.split_mb * (1 << 20)), use_success_bitmap=True,
                                     columns=("offset", "block_size", "bin_mq_nl", "flag_nc", "l_seq"))
        n = f.n_loaded
        if not (n == s.n_records == c.n_success):
            raise SystemExit(f"records: loaded {n}, generated {s.n_records}, checker {c.n_success}")
        plan = batches(cols["block_size"], int(a.batch_gb * 1e9))
        bytes_read = int(cols["block_size"].astype(np.int64).sum()) - 32 * n
        # parity pass (host copies of qual and the offsets; not timed)
        written, sampled = 0, 0
        for i0, k in plan:
            rf = f.load_record_fields(i0, k, fields=("qual",))
            t = rf.totals
            ok = (int(rf.name_off[-1]), int(rf.cigar_off[-1]), int(rf.seq_off[-1]), int(rf.aux_off[-1])) == \
                (t["name_bytes"], t["cigar_ops"], t["seq_bases"], t["aux_bytes"])
            ok &= rf.qual.size == t["seq_bases"]
            ls = cols["l_seq"][i0:i0 + k].astype(np.int64)
            lrn = (cols["bin_mq_nl"][i0:i0 + k] & 0xff).astype(np.int64)
            nc = (cols["flag_nc"][i0:i0 + k] & 0xffff).astype(np.int64)
            bs = cols["block_size"][i0:i0 + k].astype(np.int64)
            ok &= t["seq_bases"] == int(ls.sum()) and t["cigar_ops"] == int(nc.sum())
            ok &= t["name_bytes"] == int(np.maximum(lrn - 1, 0).sum())
            ok &= t["aux_bytes"] == int((bs - 32 - lrn - 4 * nc - (ls + 1) // 2 - ls).sum())
            if not ok:
                raise SystemExit(f"parity: totals of batch [{i0}, {i0 + k}) disagree with its columns")
            written += t["name_bytes"] + 4 * t["cigar_ops"] + 2 * t["seq_bases"] + t["aux_bytes"]
            off = cols["offset"][i0:i0 + k]
            qstart = off + 36 + lrn + 4 * nc + (ls + 1) // 2
            for r0 in rng.integers(0, max(k - 256, 1), max(k // 25600, 1)).tolist():
                r1 = min(r0 + 256, k)
                x0, x1 = int(off[r0]), int(off[r1 - 1] + 4 + bs[r1 - 1])
                raw = np.frombuffer(f.read_uncompressed(x0, x1 - x0), np.uint8)
                for r in range(r0, r1):
                    q = int(qstart[r]) - x0
                    if not np.array_equal(raw[q:q + int(ls[r])], rf.qual[int(rf.seq_off[r]):int(rf.seq_off[r + 1])]):
                        raise SystemExit(f"parity: qual of record {i0 + r} differs from the stream")
                sampled += r1 - r0
            del rf
        # timed passes: all five columns, left on the device
        runs, size_runs = [], []
        for _ in range(a.repeats):
            ms = sz = 0.0
            for i0, k in plan:
                f.load_record_fields(i0, k, host=False)
                ms += f.kernel_ms("record_fields")
                sz += f.kernel_ms("record_field_sizes")
            runs.append(ms)
            size_runs.append(sz)
        ms = float(np.median(runs))
        # where the time goes: one pass per column alone
        column_ms = {}
        for col in ("name", "cigar", "seq", "qual", "aux"):
            t = 0.0
            for i0, k in plan:
                f.load_record_fields(i0, k, fields=(col,), host=False)
                t += f.kernel_ms("record_fields")
            column_ms[col] = round(t, 3)
    peak = copy_peak(a.device)
    gbps = (bytes_read + written) / (ms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "record_fields gather GB/s (record bytes read + column bytes written) / device time",
        "read_len": a.read_len, "file_gb": round(data.size / 1e9, 3), "records": n, "batches": len(plan),
        "ms": round(ms, 3), "ms_runs": [round(x, 3) for x in runs], "sizes_ms": round(float(np.median(size_runs)), 3),
        "bytes_read": bytes_read, "bytes_written": written, "gbps": round(gbps, 1),
        "gbps_runs": [round((bytes_read + written) / (x * 1e-3) / 1e9, 1) for x in runs],
        "hbm_copy_peak": round(peak, 1), "ratio": round(gbps / peak, 3), "column_ms": column_ms,
        "parity": {"batches": len(plan), "qual_records_sampled": sampled, "ok": True}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
