#!/usr/bin/env python3
"""crc_bench.py — the time of sbam_check_crc (the BGZF block CRC32 check) on one MI355X.

    python tools/crc_bench.py [--size-gb 10] [--read-len 150 | --read-len 0] [--level 6 | --level 0] [--repeats 5]

The synthetic file of tools/synth.py (bench.py's generator: --read-len 150 Illumina-like, --read-len 0 the long-read
config, --level 0 stored blocks) resident in HBM and inflated once; one untimed check, then --repeats checks of the
whole table.  Prints ONE JSON line:

* `crc_ms`: the "crc" device time of a check (sbam_last_kernel_ms), the median of the --repeats runs, all of them in
  `crc_ms_runs`;
* `inflate_ms`: the "inflate" device time of the same run's inflate, and `crc_over_inflate` = crc_ms / inflate_ms;
* `gbps`: uncompressed bytes / crc_ms (the check reads every stream byte once; the 4 footer bytes and 8 result bytes
  per block are left out); `hbm_copy_peak` (tools/hbm_peak.hip, measured in this process after the checks) and
  `ratio` = gbps / it (a copy moves each byte twice, the check reads it once);
* `n_blocks`, `n_bad` (must be 0, else the tool stops);
* `parity`: --sample blocks (evenly spread, the first and last included) whose computed CRC equals
  zlib.crc32(read_uncompressed(...)) and the footer's value.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

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
    ap.add_argument("--level", type=int, default=6, help="zlib level of the BGZF blocks (0 = stored)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=4096, help="blocks compared with zlib.crc32 on the host")
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
                                read_len=a.read_len, level=a.level, distinct=a.tiles > 1, cycle=max(a.tiles, 1))
    data = s.bytes()
    log(f"[crc_bench] {data.size / 1e9:.2f} GB, level {a.level}, generated in {time.perf_counter() - t0:.1f}s")
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        inflate_ms = f.kernel_ms("inflate")
        r = f.check_crc()  # (untimed: allocates the result arrays, loads the code object)
        runs = []
        for _ in range(a.repeats):
            r = f.check_crc()
            runs.append(f.kernel_ms("crc"))
        if r["n_bad"]:
            raise SystemExit(f"{r['n_bad']} of {r['n_blocks']} blocks mismatch, the first at index {r['first_bad']}")
        computed, stored = f.block_crcs()
        _, _, us, uo = f.blocks()
        nb = r["n_blocks"]
        pick = np.unique(np.linspace(0, nb - 1, min(a.sample, nb)).astype(np.int64)) if nb else np.zeros(0, np.int64)
        for b in pick.tolist():
            want = zlib.crc32(f.read_uncompressed(int(uo[b]), int(us[b])))
            if not (want == int(computed[b]) == int(stored[b])):
                raise SystemExit(f"parity: block {b}: zlib {want:08x}, computed {int(computed[b]):08x}, "
                                 f"footer {int(stored[b]):08x}")
        ubytes = r["bytes"]
    peak = copy_peak(a.device)
    ms = float(np.median(runs))
    gbps = ubytes / (ms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "sbam_check_crc device ms (CRC32 of every BGZF block's inflated bytes against its footer)",
        "read_len": a.read_len, "level": a.level, "file_gb": round(data.size / 1e9, 3),
        "uncompressed_gb": round(ubytes / 1e9, 3), "n_blocks": nb, "n_bad": r["n_bad"],
        "crc_ms": round(ms, 3), "crc_ms_runs": [round(x, 3) for x in runs], "inflate_ms": round(inflate_ms, 3),
        "crc_over_inflate": round(ms / inflate_ms, 4), "gbps": round(gbps, 1), "hbm_copy_peak": round(peak, 1),
        "ratio": round(gbps / peak, 3), "parity": {"ok": True, "blocks": int(pick.size)}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
