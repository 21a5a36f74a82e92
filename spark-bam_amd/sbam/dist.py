"""Multi-GPU driver: one process per GPU, byte-range shards of one BAM, tiny collectives.

Shard planning follows the reference's partitioning (one task per Hadoop FileSplit,
load/.../spark/load/SplitRDD.scala:33-52): rank r owns a contiguous run of Hadoop splits; it loads the
compressed bytes of those splits plus a halo (records and 10-record checker chains straddle shard edges),
starts its BGZF stream at FindBlockStart(first split start) and stops checking at the block where rank
r+1 starts.  The only cross-GPU traffic is what Spark's driver does with tiny data:

* ``all_gather`` of each split's first-record Pos / non-empty flag / record count
  (``mapPartitions(first).collect``, CanLoadBam.scala:262-271);
* ``all_reduce(sum)`` of the full-check Counts table (``reduceByKey(_ |+| _)``, FullCheck.scala:160-168).

A chain that leaves the loaded bytes reports HALO; the shard grows its halo and re-runs (adaptive halo for long
reads: ``GpuShard.run``, the one place a shard's stream is rebuilt and its work run).  The per-shard work is pluggable,
so the distributed logic is testable on CPU (gloo) with a CPU-side per-shard function; production uses ``GpuShard``.

``run_file`` is the file-level driver: rank 0 parses the BAM header and broadcasts ContigLengths
(CanLoadBam.scala:179-180: the driver reads the header once and ships it to every task), every rank preads
only its own byte range + halo, and without a process group the same shards run one after another on this
process's GPU (a file larger than one GPU's HBM, or a one-GPU rehearsal of an N-GPU run).  ``WindowPipe`` streams
one rank's range through two contexts in windows (CanLoadBam.scala:281-334 at more than HBM per GPU).  How many
windows a range needs and what a context is sized for come from ``sbam.bgzf_sample`` (re-exported here).
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

import sbam
from sbam import Counts, N_COUNT_WORDS
from sbam.bgzf_sample import (auto_windows, bgzf_buffer_stats, bgzf_ratio, bgzf_sample_stats,  # noqa: F401
                              deflate_token_count, hbm_bytes_per_compressed_byte)


def hadoop_splits(file_size: int, split_size: int):
    """FileInputFormat rule (SPLIT_SLOP 1.1), same arithmetic as sbam_file_splits."""
    out, off, rem = [], 0, file_size
    while rem / split_size > 1.1:
        out.append((off, off + split_size))
        off += split_size
        rem -= split_size
    if rem > 0:
        out.append((off, file_size))
    return out


@dataclass
class ShardPlan:
    rank: int
    world: int
    split_first: int  # first Hadoop split index owned
    split_count: int
    lo: int  # first compressed byte owned (start of the first owned split)
    owned_hi: int  # start of the next rank's first split (or file size)
    file_size: int

    def load_range(self, halo: int):
        return self.lo, min(self.file_size, self.owned_hi + halo)


def plan_shards(file_size: int, split_size: int, world: int) -> List[ShardPlan]:
    sp = hadoop_splits(file_size, split_size)
    ns = len(sp)
    plans = []
    for r in range(world):
        i0, i1 = r * ns // world, (r + 1) * ns // world
        lo = sp[i0][0] if i0 < ns else file_size
        hi = sp[i1][0] if i1 < ns else file_size
        plans.append(ShardPlan(r, world, i0, i1 - i0, lo, hi, file_size))
    return plans


@dataclass
class ShardResult:
    counts: np.ndarray  # int64[N_COUNT_WORDS]: sbam.Counts.pack()
    first_block_pos: np.ndarray  # int64[split_count]
    first_offset: np.ndarray  # int64[split_count]
    nonempty: np.ndarray  # int64[split_count]
    n_records: np.ndarray  # int64[split_count]


def pack_counts(c: Counts) -> np.ndarray:
    return c.pack()


def unpack_counts(v: np.ndarray) -> dict:
    return dict(vars(Counts.unpack(v)))


def shard_pass(f, p: ShardPlan, split_size: int, R: int = 10) -> ShardResult:
    """One shard's hot path once its stream is inflated (``f``: sbam.BamFile over the shard's bytes, or any
    object with the same methods): full check of the positions of the blocks the shard owns (from its first
    block to the block where the next shard starts), then the owned Hadoop splits' first records and counts."""
    if p.owned_hi >= p.file_size:
        x1 = f.uncompressed_size
    else:
        st, _, _, uo = f.blocks()
        nb = f.find_block_start(p.owned_hi)
        b = int(np.searchsorted(st, nb))
        x1 = int(uo[b]) if b < st.size else f.uncompressed_size
    counts = f.check_full_counts(0, x1, R)
    if p.split_count:
        bp, off, nonempty, n = f.split_records_arrays(split_size, first=p.split_first, count=p.split_count,
                                                      reads_to_check=R, use_success_bitmap=True)
    else:
        bp = off = nonempty = n = np.zeros(0, np.int64)
    return ShardResult(pack_counts(counts), bp.astype(np.int64), off.astype(np.int64), nonempty.astype(np.int64),
                       n.astype(np.int64))


def shard_load(f, p: ShardPlan, split_size: int, R: int = 10, use_success_bitmap: bool = False,
               eager_proof: bool = True, columns: Optional[Sequence[str]] = None):
    """One shard's loadReads: the owned Hadoop splits' records decoded into device columns
    (sbam_load_records; CanLoadBam.scala:281-334).  Returns the partition sizes; with `columns`, the columns are
    copied out as well: (partition sizes, {column: ndarray}).

    eager_proof: first run the eager checker over the shard (its calls' bitmap stays on the device) so that the
    splits' record chains come from that bitmap once sbam_load_records has proved it — every set bit from a
    split's first record hops (block_size) to the next set bit — instead of one lane walking each split's chain
    record by record (twice: counts, then offsets).  The records are the same either way: a bitmap that fails
    the proof falls back to the walk."""
    if not p.split_count:
        sizes, cols = np.zeros(0, np.int64), {k: np.zeros(0, sbam.RECORD_COLUMNS[k]) for k in columns or ()}
    else:
        if eager_proof and not use_success_bitmap:
            f.check_eager_device(0, f.uncompressed_size, R)
            use_success_bitmap = True
        sizes, cols = f.load_records(split_size, first=p.split_first, count=p.split_count, reads_to_check=R,
                                     use_success_bitmap=use_success_bitmap, columns=columns)
    return sizes if columns is None else (sizes, cols)


class GpuShard:
    """Per-rank GPU work for one shard: scan → inflate → full check (owned positions) → split records."""

    def __init__(self, plan: ShardPlan, source: Callable[[int, int], np.ndarray], split_size: int,
                 contig_lengths: Sequence[int], device: int = 0, halo: int = 2 << 20, reads_to_check: int = 10):
        self.plan, self.source, self.split_size = plan, source, split_size
        self.contig_lengths = np.asarray(contig_lengths, np.int64)
        self.device, self.halo, self.R = device, halo, reads_to_check
        self.retries = 0  # halo retries so far (each grows the halo 4x and re-runs the shard)
        self._reserved = 0  # compressed bytes the context's device buffers were last sized for (reserve)
        lo, hi = plan.load_range(halo)
        self.f = sbam.BamFile(source(lo, hi), device=device, base_offset=lo, file_size=plan.file_size, inflate=False)

    def reload(self, plan: ShardPlan, data: np.ndarray, source: Optional[Callable[[int, int], np.ndarray]] = None):
        """Stream the next byte-range window through this shard's context (sbam_load: device allocations are
        kept): `data` = the bytes of plan.load_range(self.halo).  `source` replaces the byte source a halo retry
        reads from (it must not hand back a buffer another window is being staged into)."""
        self.plan = plan
        if source is not None:
            self.source = source
        lo, _ = plan.load_range(self.halo)
        self.f.load(data, base_offset=lo, file_size=plan.file_size)

    def reserve(self, comp: int, sample: np.ndarray):
        """Size the context once for loads of up to `comp` compressed bytes (device buffers are grow-only: a context
        that first meets a larger window than before would hipFree + hipMalloc tens of GB inside a timed step), from
        the compression ratio and block size of the BGZF bytes `sample` (+12 %)."""
        if self._reserved >= comp:
            return
        ratio, per_block = bgzf_buffer_stats(sample)
        U = int(comp * ratio * 1.12) + (1 << 20)
        self.f.reserve(comp, int(comp / per_block * 1.12) + 1024, U, U // 200)
        self._reserved = comp

    def run(self, fn):
        """fn(f, plan) on the shard's inflated stream: reset → scan → inflate → fn.  A chain that leaves the
        loaded bytes (HaloException) grows the halo 4x and runs the shard again, until the range reaches the end
        of the file."""
        while True:
            try:
                self.f.reset()
                self.f.run(contig_lengths=self.contig_lengths)
                return fn(self.f, self.plan)
            except sbam.HaloException:
                if self.plan.load_range(self.halo)[1] >= self.plan.file_size:
                    raise
                self.halo *= 4
                self.retries += 1
                # the grown range goes into the same context (sbam_load keeps its device allocations and only grows
                # the ones the larger range needs), so a retry costs one H2D copy and the re-run, not a new context
                lo, hi = self.plan.load_range(self.halo)
                self.f.load(self.source(lo, hi), base_offset=lo, file_size=self.plan.file_size)

    def step(self) -> ShardResult:
        """compute-splits + full-check of the shard."""
        return self.run(lambda f, p: shard_pass(f, p, self.split_size, self.R))

    def load_step(self) -> np.ndarray:
        """loadReads of the shard: scan → inflate → FindBlockStart/FindRecordStart → record chains → columns."""
        return self.run(lambda f, p: shard_load(f, p, self.split_size, self.R))

    def load_columns(self, columns: Sequence[str]):
        """load_step with the decoded record columns copied out: (partition sizes, {column: ndarray})."""
        return self.run(lambda f, p: shard_load(f, p, self.split_size, self.R, columns=columns))

    def close(self):
        if self.f is not None:
            self.f.close()
            self.f = None


def combine(results: Sequence[ShardResult], file_size: int):
    """Rank-0 assembly of gathered shard results → (Split list, partition sizes, merged counts)."""
    from sbam import Pos, Split
    firsts, sizes = [], []
    counts = np.zeros(N_COUNT_WORDS, np.int64)
    for r in results:
        counts += r.counts
        for b, o, ne, n in zip(r.first_block_pos, r.first_offset, r.nonempty, r.n_records):
            sizes.append(int(n))
            if ne:
                firsts.append(Pos(int(b), int(o)))
    ends = firsts[1:] + [Pos(file_size, 0)]
    return [Split(a, b) for a, b in zip(firsts, ends)], sizes, counts


def gather_results(res: ShardResult, plans: Sequence[ShardPlan], device=None) -> Optional[List[ShardResult]]:
    """all_gather of per-shard results (fixed-size int64 rows) + all_reduce of counts via torch.distributed.
    Returns the per-rank list on every rank (counts of each entry are the merged totals on rank 0's row)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size()
    maxs = max(p.split_count for p in plans)
    row = np.zeros(4 * maxs, np.int64)
    k = len(res.n_records)
    for j, a in enumerate((res.first_block_pos, res.first_offset, res.nonempty, res.n_records)):
        row[j * maxs: j * maxs + k] = a
    t = torch.from_numpy(row)
    c = torch.from_numpy(res.counts.copy())
    if device is not None:
        t, c = t.to(device), c.to(device)
    out = torch.empty(world * row.size, dtype=torch.int64, device=t.device)
    dist.all_gather_into_tensor(out, t)
    dist.all_reduce(c, op=dist.ReduceOp.SUM)
    out = out.cpu().numpy().reshape(world, 4, maxs)
    merged = c.cpu().numpy()
    results = []
    for r, p in enumerate(plans):
        n = p.split_count
        results.append(ShardResult(merged if r == 0 else np.zeros_like(merged), out[r, 0, :n], out[r, 1, :n],
                                   out[r, 2, :n], out[r, 3, :n]))
    return results


# ---- file-level driver ----------------------------------------------------------------------------------------

def device_free_bytes(device: int) -> int:
    import torch
    return int(torch.cuda.mem_get_info(device)[0])


def file_source(path: str) -> Tuple[Callable[..., np.ndarray], int]:
    """(source, file size) for a BAM on disk: source(lo, hi[, out]) preads bytes [lo, hi) into a new (or the given)
    uint8 array — a rank touches only its own byte range, never the whole file."""
    size = os.path.getsize(path)

    def source(lo: int, hi: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        hi = min(hi, size)
        buf = np.empty(hi - lo, np.uint8) if out is None else out[: hi - lo]
        mv = memoryview(buf)
        fd = os.open(path, os.O_RDONLY)
        try:
            got = 0
            while got < hi - lo:
                n = os.preadv(fd, [mv[got: min(hi - lo, got + (1 << 30))]], lo + got)
                if n <= 0:
                    raise IOError(f"{path}: short read at {lo + got}")
                got += n
        finally:
            os.close(fd)
        return buf

    return source, size


def read_bam_header(source: Callable[[int, int], np.ndarray], file_size: int, device: int = 0,
                    probe: int = 1 << 20) -> Tuple[np.ndarray, List[str]]:
    """(ContigLengths, contig names) from the header at the start of the file (ContigLengths.scala:20-37 via htsjdk's
    header reader; bam/header/Header.scala:26-60): the first `probe` bytes are inflated on the GPU and parsed
    (sbam_header); a header longer than the probe doubles it."""
    from sbam.cli import header_names
    hi = min(file_size, probe)
    while True:
        try:
            with sbam.BamFile(source(0, hi), device=device, file_size=file_size, inflate=False) as f:
                f.inflate()
                return f.header()[1], header_names(f)
        except sbam.SbamError as e:
            if "truncated header" not in str(e) or hi >= file_size:
                raise
            hi = min(file_size, 2 * hi)


def read_contig_lengths(source: Callable[[int, int], np.ndarray], file_size: int, device: int = 0,
                        probe: int = 1 << 20) -> np.ndarray:
    """ContigLengths of the file's header (read_bam_header)."""
    return read_bam_header(source, file_size, device, probe)[0]


def broadcast_lengths(lens: Optional[np.ndarray], device=None) -> np.ndarray:
    """Rank 0's ContigLengths to every rank (the reference broadcasts the header's lengths to its tasks)."""
    import torch
    import torch.distributed as dist
    n = torch.tensor([0 if lens is None else len(lens)], dtype=torch.int64, device=device)
    dist.broadcast(n, src=0)
    t = torch.zeros(int(n.item()), dtype=torch.int64, device=device)
    if dist.get_rank() == 0:
        t.copy_(torch.from_numpy(np.asarray(lens, np.int64)))
    dist.broadcast(t, src=0)
    return t.cpu().numpy()


@dataclass
class RunResult:
    splits: list  # [sbam.Split] (compute-splits)
    partition_sizes: List[int]  # records per Hadoop split
    counts: dict  # merged full-check Counts (unpack_counts)
    contig_lengths: np.ndarray


def _dist_ready() -> bool:
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized()
    except ImportError:
        return False


def _placement(world: Optional[int], device: Optional[int]):
    """Where a file-level driver runs: (in a process group?, world, rank, the shards this process runs, device).  In a
    torch.distributed group the shards are the ranks (one each, on GPU LOCAL_RANK; the collectives run even at world
    size 1, so RCCL is exercised); without one, `world` shards (default 1) run one after another on `device`."""
    if _dist_ready():
        import torch.distributed as dist
        rank = dist.get_rank()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", 0))
        return True, dist.get_world_size(), rank, [rank], device
    world = world or 1
    return False, world, 0, list(range(world)), 0 if device is None else device


def run_file(path, split_size: Optional[int] = None, world: Optional[int] = None, device: Optional[int] = None,
             halo: int = 2 << 20, reads_to_check: int = 10, coll_device=None,
             open_shard: Optional[Callable[[ShardPlan, Callable, int, np.ndarray], object]] = None,
             read_header: Optional[Callable[[Callable, int, int], np.ndarray]] = None) -> RunResult:
    """full-check + compute-splits of one BAM over byte-range shards (FullCheck.scala:141-191 with the splits of
    CanLoadBam.scala:245-279).  `path`: a file name, or a (source, file_size) pair.

    In a torch.distributed process group (RCCL on GPUs; gloo to rehearse) the shards are the ranks: rank 0 reads
    the header and broadcasts ContigLengths, each rank preads [lo, owned_hi + halo) of its own shard, and the
    results meet in one all_gather + one all_reduce (gather_results); every rank returns the whole result.
    Without a process group, `world` shards (default 1) run one after another on `device`.
    `open_shard(plan, source, split_size, contig_lengths)` / `read_header(source, size, device)` replace the GPU
    shard and header reader (CPU tests)."""
    split_size = sbam.effective_split_size(split_size)
    source, size = file_source(path) if isinstance(path, (str, os.PathLike)) else path
    grouped, world, rank, ranks, device = _placement(world, device)
    read_header = read_header or read_contig_lengths
    lens = read_header(source, size, device) if rank == 0 else None
    if grouped:
        lens = broadcast_lengths(lens, coll_device)
    if open_shard is None:
        def open_shard(plan, src, ss, cl):
            return GpuShard(plan, src, ss, cl, device=device, halo=halo, reads_to_check=reads_to_check)
    plans = plan_shards(size, split_size, world)
    results = []
    for r in ranks:
        sh = open_shard(plans[r], source, split_size, lens)
        try:
            results.append(sh.step())
        finally:
            sh.close()
    if grouped:
        results = gather_results(results[0], plans, device=coll_device)
    splits, sizes, counts = combine(results, size)
    return RunResult(splits, sizes, unpack_counts(counts), np.asarray(lens, np.int64))


def owned_blocks(f, p: ShardPlan) -> np.ndarray:
    """Block mask of the blocks shard `p` owns in its context `f`: from its first block up to the block where the next
    shard's stream starts (FindBlockStart of that shard's first split), as shard_pass does."""
    st = f.blocks()[0]
    if p.owned_hi >= p.file_size:
        return np.ones(st.size, bool)
    b = int(np.searchsorted(st, f.find_block_start(p.owned_hi)))
    m = np.zeros(st.size, bool)
    m[:b] = True
    return m


def full_check_file(path, limit: int = 10, ranges=None, reads_to_check: int = 10, world: Optional[int] = None,
                    device: Optional[int] = None, halo: int = 2 << 20, coll_device=None,
                    records_path: Optional[str] = None, split_size: int = 2 << 20):
    """`full-check` over byte-range shards (FullCheck.scala:88-323 with Blocks' partitions, Blocks.scala:141-207).
    Each shard full-checks the blocks it owns and samples its first `limit` close calls of keys 1 and 2 (and its
    disagreements with the `.records` truth) as PosMetadata lines — the next record of a sampled position may lie in
    the halo, which grows when needed.  In a process group (RCCL on GPUs) rank 0 reads the header and broadcasts the
    contig lengths (device tensor) and names; the Counts meet in one all_reduce on `coll_device` (reduceByKey,
    FullCheck.scala:160-168) and the sampled lines in one all_gather_object (the driver's take(limit)).  Without a
    process group, `world` shards run one after another on `device` (a file larger than HBM in windows).
    Returns the merged sbam.cli.FullCheckParts on every rank."""
    from sbam.cli import FullCheckParts, FullCheckReport, merge_parts
    source, size = file_source(path) if isinstance(path, (str, os.PathLike)) else path
    grouped, world, rank, ranks, device = _placement(world, device)
    lens, names = read_bam_header(source, size, device) if rank == 0 else (None, None)
    if grouped:
        import torch.distributed as dist
        lens = broadcast_lengths(lens, coll_device)
        box = [names]
        dist.broadcast_object_list(box, src=0, device=coll_device)
        names = box[0]
    plans = plan_shards(size, split_size, world)
    parts = []
    for r in ranks:
        sh = GpuShard(plans[r], source, split_size, lens, device=device, halo=halo, reads_to_check=reads_to_check)
        try:
            parts.append(sh.run(lambda f, p: FullCheckReport(
                f, None, records_path, limit, ranges, reads_to_check, blocks=owned_blocks(f, p), names=names).parts()))
        finally:
            sh.close()
    if grouped:
        import torch
        mine = parts[0]
        c = torch.from_numpy(mine.pack())
        if coll_device is not None:
            c = c.to(coll_device)
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        v = c.cpu().numpy()
        lists = [None] * world
        dist.all_gather_object(lists, (mine.close, mine.truth))
        # the reduced Counts ride on the first part; every part keeps its own sampled lines (file order = rank order)
        parts = [FullCheckParts.unpack(v if i == 0 else np.zeros_like(v), close, truth)
                 for i, (close, truth) in enumerate(lists)]
    return merge_parts(parts, limit)


def check_crc_file(path, world: int = 1, device: int = 0, split_size: int = 2 << 20, halo: int = 2 << 20) -> dict:
    """`check-crc` over `world` byte-range windows, one after another on one context (a file larger than HBM): every
    window scans and inflates its range and checks the CRC32 of the blocks it owns (owned_blocks, as full_check_file's
    ungrouped branch), so every block of the file is counted once.  `path`: a file name, or a (source, file_size)
    pair.  Returns the merged totals (n_blocks, n_bad, bytes), `bad`: the sorted (file offset, stored, computed) of the
    mismatching blocks, and `windows`: each window's n_blocks.  Needs no BAM header, so any BGZF file serves.  Not for
    use inside a process group."""
    source, size = file_source(path) if isinstance(path, (str, os.PathLike)) else path
    plans = plan_shards(size, split_size, max(1, int(world)))
    out = {"n_blocks": 0, "n_bad": 0, "bytes": 0, "bad": [], "windows": []}

    def window(f, p):
        own = int(owned_blocks(f, p).sum())  # (the owned blocks are the table's first ones)
        r = f.check_crc(0, own)
        if r["n_bad"]:
            computed, stored = f.block_crcs()
            r["bad_values"] = [(int(o), int(stored[b]), int(computed[b])) for b, o in zip(r["bad"], r["bad_offsets"])]
        return r

    sh = None
    try:
        for p in plans:
            lo, hi = p.load_range(halo)
            if p.lo >= p.owned_hi:  # more windows than Hadoop splits: nothing to own
                out["windows"].append(0)
                continue
            if sh is None:
                sh = GpuShard(p, source, split_size, (), device=device, halo=halo)
            else:
                sh.halo = halo
                sh.reload(p, source(lo, hi))
            r = sh.run(window)
            for k in ("n_blocks", "n_bad", "bytes"):
                out[k] += r[k]
            out["bad"] += r.get("bad_values", [])
            out["windows"].append(r["n_blocks"])
    finally:
        if sh is not None:
            sh.close()
    out["bad"].sort()
    return out


class WindowPipe:
    """A rank's byte range streamed through two contexts in W windows (`wplans`: the windows' ShardPlans): while
    window w computes on one context, a loader thread copies window w+1's bytes into the other (sbam_load's host →
    device copy) and a stager thread stages window w+2 into host memory (`stage(lo, hi, k)` into staging buffer
    k).  Windows are numbered across steps (g = step · W + w): window g uses context g mod 2 and staging buffer
    g mod 3, so the pipeline runs on from one step into the next — the last window of a step computes while the
    next step's window 0 is copied (`prefetch=True`; `drop_prefetch()` discards one that no step will use).
    Without a pending prefetch a step starts with window 0 loaded in the foreground.  `run_window(shard)` is the
    per-window work (GpuShard.step / load_step / anything on shard.f).  Buffer k is restaged only after the copy
    that read it has finished (window g+2 reuses window g-1's buffer, whose copy ended before window g-1 computed)."""
    NBUF = 3

    def __init__(self, wplans, stage, split_size, contig_lengths, device, run_window, halo: int = 2 << 20,
                 prefetch: bool = False):
        from concurrent.futures import ThreadPoolExecutor
        self.wplans, self.stage, self.split_size = wplans, stage, split_size
        self.contig_lengths, self.device, self.run_window, self.halo = contig_lengths, device, run_window, halo
        self.prefetch = prefetch
        self.loader = ThreadPoolExecutor(max_workers=1)
        self.stager = ThreadPoolExecutor(max_workers=1)
        self.ctx = [None, None]
        self._inflight = []   # loader futures of the running step
        self.g = 0            # global number of the next step's window 0
        self._next = None     # (load future of window g, {g': staged future}) carried over from the last step

    def _range(self, g):
        sh = self.ctx[g % 2]
        return self.wplans[g % len(self.wplans)].load_range(sh.halo if sh is not None else self.halo)

    def _stage(self, g):
        lo, hi = self._range(g)
        return lo, hi, self.stage(lo, hi, g % self.NBUF)

    def _load(self, g, staged):
        wp = self.wplans[g % len(self.wplans)]
        j, k = g % 2, g % self.NBUF
        lo, hi, buf = staged.result()
        if (lo, hi) != self._range(g):  # the context's halo grew since staging: stage again
            lo, hi = self._range(g)
            buf = self.stage(lo, hi, k)
        src = self._source(lo, hi, buf)
        if self.ctx[j] is None:
            self.ctx[j] = GpuShard(wp, src, self.split_size, self.contig_lengths, device=self.device, halo=self.halo)
        else:
            self.ctx[j].reload(wp, buf, src)
        sh = self.ctx[j]
        # sized once for the largest window of the plan (at the context's halo), not window by window
        sh.reserve(max(b - a for a, b in (p.load_range(sh.halo) for p in self.wplans)), buf)
        return sh

    def _source(self, lo, hi, buf):
        """The byte source of one loaded window: its staged bytes for its own range; any other range (a halo retry)
        is staged into a private buffer, never into a shared staging slot."""
        def src(a, b):
            return buf if (a, b) == (lo, hi) else self.stage(a, b, None)
        return src

    def drop_prefetch(self):
        """Wait for and discard a prefetched window 0 (the next step then loads it in the foreground)."""
        if self._next is not None:
            fut, staged = self._next
            fut.result()
            for f in staged.values():
                f.result()
            self._next = None  # window self.g is loaded again (same context) by the next step

    def step(self) -> list:
        W = len(self.wplans)
        g0 = self.g
        if self._next is not None:
            fut, staged = self._next
            self._next = None
        else:
            staged = {g: self.stager.submit(self._stage, g) for g in range(g0, g0 + min(2, W))}
            fut = None
        try:
            return self._windows(g0, W, staged, fut)
        except BaseException:
            # a failed window (a non-halo error, or a halo retry that reached EOF): drain the loads and stagings still
            # in flight — they drive the other context and the staging buffers — so that a retried step starts clean
            for f in ([fut] if fut is not None else []) + list(staged.values()) + list(self._inflight):
                try:
                    f.result()
                except BaseException:
                    pass
            self._inflight = []
            self._next = None
            raise

    def _windows(self, g0, W, staged, fut) -> list:
        self._inflight = []
        out = []
        sh = self._load(g0, staged[g0]) if fut is None else None
        dbg = os.environ.get("SBAM_PIPE_DEBUG")
        for w in range(W):
            g = g0 + w
            t0 = time.perf_counter()
            if sh is None:
                sh = fut.result()
            if dbg:
                print(f"[pipe] window {g}: waited {1e3 * (time.perf_counter() - t0):.1f} ms for its load", file=sys.stderr)
            last = w + 1 == W
            if not last or self.prefetch:
                if g + 1 not in staged:
                    staged[g + 1] = self.stager.submit(self._stage, g + 1)
                fut = self.loader.submit(self._load, g + 1, staged[g + 1])
                self._inflight.append(fut)
            if (w + 2 < W or self.prefetch) and g + 2 not in staged:
                staged[g + 2] = self.stager.submit(self._stage, g + 2)
            t1 = time.perf_counter()
            out.append(self.run_window(sh))
            if dbg:
                print(f"[pipe] window {g}: ran {1e3 * (time.perf_counter() - t1):.1f} ms", file=sys.stderr)
            sh = None
        self.g = g0 + W
        if self.prefetch:
            self._next = (fut, {k: v for k, v in staged.items() if k >= self.g})
        return out

    def close(self):
        self.loader.shutdown()
        self.stager.shutdown()
        for sh in self.ctx:
            if sh is not None:
                sh.close()
        self.ctx = [None, None]
