#!/usr/bin/env python3
"""write_bench.py — the time of sbam_write_bam (gather, deflate, BGZF framing) on one MI355X.

    python tools/write_bench.py [--size-gb 0.08] [--read-len 150 | --read-len 0] [--level 0 | --level 1] [--huffman fixed | dynamic]
                                [--repeats 5]

The synthetic file of tools/synth.py (bench.py's generator: --read-len 150 Illumina-like, --read-len 0 the long-read
config) resident in HBM, inflated, its records loaded; one untimed write of every record, then --repeats writes.  The
default size keeps the output inside one batch of deflate slots (4096 blocks), so the "write_deflate" and "write_frame"
times cover the whole file.  Prints ONE JSON line per level (both levels without --level); --huffman dynamic writes
level 1 as 1 | SBAM_WRITE_DYNAMIC (per block the smallest of stored, fixed and dynamic Huffman; its deflate stage is one
launch, so `deflate_ms` is its only timer) and adds `huffman` and `n_blocks_by_form` to level 1's line:

* `select_ms`, `gather_ms`, `deflate_ms`, `frame_ms`: device times (sbam_last_kernel_ms), medians of the --repeats
  runs; `write_ms` their sum and `gbps` = uncompressed output bytes / write_ms;
* `inflate_ms`: the "inflate" device time of the input (about the same bytes), `write_over_inflate` = write_ms / it;
* `hbm_copy_peak` (tools/hbm_peak.hip) and `ratio` = gbps / it;
* `comp_bytes`, `n_blocks`, `n_stored_blocks`;
* `zlib1_ms`, `zlib1_bytes`: the same blocks through zlib level 1 (raw deflate + 26 bytes each) on --threads host
  threads, `zlib1_gbps`, `speedup_over_zlib1` = zlib1_ms / write_ms and `size_over_zlib1` = comp_bytes / zlib1_bytes;
* `parity`: every output is a gzip-readable file, and the levels' outputs inflate to the same stream (the one the
  host's zlib run compresses).
"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "spark-bam_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from fields_bench import copy_peak, log  # noqa: E402

BB = 65498
STAGES = ("write_select", "write_gather", "write_deflate", "write_frame")


def zlib1(u: bytes, threads: int):
    """(seconds, bytes) of every 65498-byte block of u through zlib level 1 as raw deflate, + 26 bytes of frame."""
    def one(o):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(c.compress(u[o:o + BB]) + c.flush()) + 26
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        total = sum(ex.map(one, range(0, len(u), BB), chunksize=64))
    return time.perf_counter() - t0, total


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=0.08, help="compressed GB of the input")
    ap.add_argument("--read-len", type=int, default=150, help="0 = the long-read config")
    ap.add_argument("--level", type=int, default=None, help="writer level 0 or 1 (default: both)")
    ap.add_argument("--huffman", choices=("fixed", "dynamic"), default="fixed", help="level 1's Huffman codes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tile-mb", type=float, default=16.0)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x5EEDBA11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    a = ap.parse_args()
    import sbam
    import synth
    t0 = time.perf_counter()
    s = synth.SynthBam.for_size(int(a.size_gb * 1e9), tile_mb=a.tile_mb, seed=a.seed, threads=a.threads,
                                read_len=a.read_len, distinct=True)
    data = s.bytes()
    log(f"[write_bench] {data.size / 1e9:.3f} GB, read_len {a.read_len}, generated in {time.perf_counter() - t0:.1f}s")
    lines = []
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        inflate_ms = f.kernel_ms("inflate")
        f.load_records(sbam.LOCAL_FS_BLOCK_SIZE, columns=None)
        want, z = None, None
        for level in ((0, 1) if a.level is None else (a.level,)):
            huffman = a.huffman if level else "fixed"
            r = f.write_bam(level=level, huffman=huffman)  # (untimed: allocates the buffers, loads the code objects)
            if r["n_blocks"] > 4096:
                raise SystemExit(f"{r['n_blocks']} blocks: more than one batch, the stage times would cover the last only")
            if want is None:
                want = gzip.decompress(r["bytes"])
                z = zlib1(want, a.threads)
            elif gzip.decompress(r["bytes"]) != want:
                raise SystemExit(f"parity: level {level} does not inflate to level 0's stream")
            st, cs, _ = f.written_blocks()
            whole = np.frombuffer(r["bytes"], np.uint8)
            forms = np.bincount((whole[st + 18] >> 1) & 3, minlength=3).tolist()  # BTYPE of every payload
            runs = {k: [] for k in STAGES}
            for _ in range(a.repeats):
                r = f.write_bam(level=level, huffman=huffman)
                for k in STAGES:
                    runs[k].append(f.kernel_ms(k))
            med = {k: float(np.median(v)) for k, v in runs.items()}
            ms = sum(med.values())
            lines.append({
                "metric": "sbam_write_bam device ms (select + gather + deflate + frame of every record)",
                "read_len": a.read_len, "level": level, "huffman": huffman if level else None,
                "n_blocks_by_form": {"stored": forms[0], "fixed": forms[1], "dynamic": forms[2]},
                "uncompressed_gb": round(r["ubytes"] / 1e9, 4),
                "n_records": r["n_records"], "n_blocks": r["n_blocks"], "n_stored_blocks": r["n_stored_blocks"],
                "comp_bytes": r["comp_bytes"], "select_ms": round(med["write_select"], 3),
                "gather_ms": round(med["write_gather"], 3), "deflate_ms": round(med["write_deflate"], 3),
                "frame_ms": round(med["write_frame"], 3), "write_ms": round(ms, 3),
                "deflate_ms_runs": [round(x, 3) for x in runs["write_deflate"]],
                "gbps": round(r["ubytes"] / (ms * 1e-3) / 1e9, 2), "inflate_ms": round(inflate_ms, 3),
                "write_over_inflate": round(ms / inflate_ms, 3), "zlib1_threads": a.threads,
                "zlib1_ms": round(z[0] * 1e3, 1), "zlib1_bytes": z[1],
                "zlib1_gbps": round(len(want) / z[0] / 1e9, 3), "speedup_over_zlib1": round(z[0] * 1e3 / ms, 1),
                "size_over_zlib1": round((r["comp_bytes"] - 28) / z[1], 4), "parity": {"ok": True}})
    peak = copy_peak(a.device)
    for ln in lines:
        ln["hbm_copy_peak"] = round(peak, 1)
        ln["ratio"] = round(ln["gbps"] / peak, 4)
        print(json.dumps(ln))
    return 0


if __name__ == "__main__":
    sys.exit(main())
