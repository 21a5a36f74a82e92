#!/usr/bin/env python3
"""tags_bench.py — the device time of sbam_load_record_tags on one MI355X.

    python tools/tags_bench.py [--size-gb 10] [--read-len 150 | --read-len 0] [--repeats 3] [--batch-gb 4]

The synthetic file of tools/synth.py (bench.py's generator; its records carry NM MD AS XS RG with --read-len 150 and
NM AS RG in the long-read config, --read-len 0) resident in HBM: full check, load_records(use_success_bitmap=True),
then load_record_tags over the whole file in batches of at most --batch-gb of record bytes, columns left on the
device, for four query sets: (NM), (NM, AS, XS), (RG + bytes), (MD + bytes).  Prints ONE JSON line:

* per query set: `ms` = the summed "record_tags" device time of a pass (sbam_last_kernel_ms; the median of --repeats
  passes, all of them in `ms_runs`), `bytes_read` = the records' tag bytes plus the fixed-field columns the walk reads
  (20 B per record) plus, with bytes, the value bytes read again by the gather, `bytes_written` = the cells (14 B per
  record and tag) plus offsets, positions and value bytes, `gbps` = their sum / `ms`, `ratio` = gbps / hbm_copy_peak,
  and `vs_aux_gather` = `ms` / the "record_fields" time of load_record_fields(fields=("aux",)) over the same batches
  (that gather reads the same tag bytes);
* `hbm_copy_peak` (tools/hbm_peak.hip, measured in this process after the passes), as fields_bench.py;
* `parity`: before the timed passes, a sampled 1 % of the records (runs of 256) of every batch is checked against
  sbam.sam.find_tags over the stream's bytes for the query NM AS XS RG MD with bytes for RG and MD.
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

from fields_bench import batches, copy_peak, log  # noqa: E402

QUERIES = {"NM": (("NM",), ()), "NM,AS,XS": (("NM", "AS", "XS"), ()), "RG+bytes": (("RG",), ("RG",)),
           "MD+bytes": (("MD",), ("MD",))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=10.0, help="compressed GB")
    ap.add_argument("--read-len", type=int, default=150, help="0 = the long-read config")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-gb", type=float, default=4.0, help="record bytes per load_record_tags call")
    ap.add_argument("--split-mb", type=float, default=2.0)
    ap.add_argument("--tile-mb", type=float, default=64.0)
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x5EEDBA11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    a = ap.parse_args()
    import sbam
    import synth
    from sbam import sam
    t0 = time.perf_counter()
    s = synth.SynthBam.for_size(int(a.size_gb * 1e9), tile_mb=a.tile_mb, seed=a.seed, threads=a.threads,
                                read_len=a.read_len, distinct=a.tiles > 1, cycle=max(a.tiles, 1))
    data = s.bytes()
    log(f"[tags_bench] {data.size / 1e9:.2f} GB, {s.n_records} records, generated in {time.perf_counter() - t0:.1f}s")
    rng = np.random.default_rng(a.seed & 0xffffffff)
    with sbam.BamFile(data, device=a.device, path="synth.bam") as f:
        c = f.check_full_counts(0, f.uncompressed_size)
        _, cols = f.load_records(int(a.split_mb * (1 << 20)), use_success_bitmap=True,
                                 columns=("offset", "block_size", "bin_mq_nl", "flag_nc", "l_seq"))
        n = f.n_loaded
        if not (n == s.n_records == c.n_success):
            raise SystemExit(f"records: loaded {n}, generated {s.n_records}, checker {c.n_success}")
        plan = batches(cols["block_size"], int(a.batch_gb * 1e9))
        ls, bs = cols["l_seq"].astype(np.int64), cols["block_size"].astype(np.int64)
        aux_len = bs - 32 - (cols["bin_mq_nl"] & 0xff) - 4 * (cols["flag_nc"] & 0xffff).astype(np.int64) - (ls + 1) // 2 - ls
        aux_start = cols["offset"] + 4 + bs - aux_len
        aux_bytes = int(aux_len.sum())
        # parity pass (host copies; not timed)
        q, by = ("NM", "AS", "XS", "RG", "MD"), ("RG", "MD")
        sampled = 0
        for i0, k in plan:
            rt = f.load_record_tags(q, i0, k, bytes_for=by)
            texts = {t: rt.texts(t) for t in by}
            for r0 in rng.integers(0, max(k - 256, 1), max(k // 25600, 1)).tolist():
                r1 = min(r0 + 256, k)
                x0 = int(aux_start[i0 + r0])
                raw = f.read_uncompressed(x0, int(aux_start[i0 + r1 - 1] + aux_len[i0 + r1 - 1]) - x0)
                for r in range(r0, r1):
                    p = int(aux_start[i0 + r]) - x0
                    for j, g in enumerate(sam.find_tags(raw[p:p + int(aux_len[i0 + r])], q)):
                        got = (int(rt.type[j, r]), int(rt.sub[j, r]), int(rt.rel[j, r]), int(rt.value[j, r]))
                        want = (0, 0, -1, 0) if g is None else (ord(g[0]), ord(g[1]) if g[1] else 0, g[2], g[3])
                        if got != want or (q[j] in by and texts[q[j]][r] != (None if g is None else g[4])):
                            raise SystemExit(f"parity: tag {q[j]} of record {i0 + r}: {got} vs {want}")
                sampled += r1 - r0
            del rt, texts
        # the aux-only gather of load_record_fields over the same batches
        aux_runs = []
        for _ in range(a.repeats):
            ms = 0.0
            for i0, k in plan:
                f.load_record_fields(i0, k, fields=("aux",), host=False)
                ms += f.kernel_ms("record_fields")
            aux_runs.append(ms)
        aux_ms = float(np.median(aux_runs))
        results = {}
        for label, (tags, bytes_for) in QUERIES.items():
            runs, value_bytes = [], 0
            for rep in range(a.repeats):
                ms = 0.0
                for i0, k in plan:
                    rt = f.load_record_tags(tags, i0, k, bytes_for=bytes_for, host=False)
                    ms += f.kernel_ms("record_tags")
                    if rep == 0:
                        value_bytes += sum(v["bytes"] for v in rt.totals.values())
                runs.append(ms)
            results[label] = (runs, value_bytes, len(tags), len(bytes_for))
    peak = copy_peak(a.device)
    out = {"metric": "record_tags device ms and GB/s (bytes read + written) per query set", "read_len": a.read_len,
           "file_gb": round(data.size / 1e9, 3), "records": n, "batches": len(plan), "aux_bytes": aux_bytes,
           "aux_gather_ms": round(aux_ms, 3), "aux_gather_ms_runs": [round(x, 3) for x in aux_runs],
           "hbm_copy_peak": round(peak, 1), "queries": {},
           "parity": {"batches": len(plan), "records_sampled": sampled, "ok": True}}
    for label, (runs, value_bytes, nq, nb) in results.items():
        ms = float(np.median(runs))
        rd = aux_bytes + 20 * n + value_bytes + (16 * n if nb else 0)  # (the scans and the gather re-read lengths and positions)
        wr = 14 * nq * n + nb * (16 * n + 8) + value_bytes
        gbps = (rd + wr) / (ms * 1e-3) / 1e9
        out["queries"][label] = {"ms": round(ms, 3), "ms_runs": [round(x, 3) for x in runs], "bytes_read": rd,
                                 "bytes_written": wr, "gbps": round(gbps, 1), "ratio": round(gbps / peak, 3),
                                 "vs_aux_gather": round(ms / aux_ms, 3) if aux_ms > 0 else None}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
