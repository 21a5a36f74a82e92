"""The BAM writer on the GPU (sbam_write_bam, sbam_test_deflate): every output block is a valid BGZF block that a
standard inflater turns back into the input slice; the uncompressed side equals the reference's htsjdk-rewrite golden
(2.100-1000.bam with its .blocks and .records); selections equal the same selection made on the host; level 1 stays
within 1.30x of zlib level 1."""
import ctypes
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import FIXTURES, fixture_bytes

pytestmark = pytest.mark.gpu

BB = 65498
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 65497, 65498, 65499, 2 * 65498]
SPLIT = 100000


def check_bgzf(whole: bytes, want: bytes, block_bytes: int = BB, with_eof: bool = True):
    """Block validity, the same way for every output: header fields, BSIZE, a bare inflate that ends exactly at the
    payload's end and gives the input slice, CRC32, ISIZE, the EOF block, gzip over the whole.  Returns the blocks as
    (start, csize, usize, stored)."""
    if with_eof:
        assert whole[-28:] == EOF_BLOCK
    end = len(whole) - (28 if with_eof else 0)
    blocks, p, u = [], 0, 0
    while p < end:
        h = whole[p:p + 18]
        assert h[0] == 31 and h[1] == 139 and h[2] == 8 and h[3] == 4, p          # ID1, ID2, CM, FLG
        assert h[10:12] == b"\x06\x00" and h[12:14] == b"BC" and h[14:16] == b"\x02\x00", p  # XLEN = 6, BC, SLEN
        csize = int.from_bytes(h[16:18], "little") + 1
        assert p + csize <= end, p
        payload = whole[p + 18:p + csize - 8]
        d = zlib.decompressobj(-15)
        out = d.decompress(payload)
        assert d.eof and d.unused_data == b"", p
        n = min(block_bytes, len(want) - u)
        assert n > 0 and out == want[u:u + n], p
        crc, isize = struct.unpack("<II", whole[p + csize - 8:p + csize])
        assert crc == zlib.crc32(out) and isize == n, p
        blocks.append((p, csize, n, (payload[0] & 6) == 0))
        p += csize
        u += n
    assert p == end and u == len(want)
    if with_eof:
        assert gzip.decompress(whole) == want
    return blocks


def deflate(data: bytes, block_bytes: int = 0, level: int = 1, with_eof: bool = True):
    """sbam_test_deflate -> (BGZF bytes, n_stored_blocks)."""
    import sbam
    L = sbam.load_library()
    buf = np.frombuffer(data, np.uint8) if data else np.zeros(0, np.uint8)
    bb = block_bytes or BB
    cap = len(data) + 31 * ((len(data) + bb - 1) // bb) + 28
    out = np.zeros(cap, np.uint8)
    n, ns = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.sbam_test_deflate(0, buf.ctypes.data if buf.size else None, buf.size, block_bytes, level,
                             1 if with_eof else 0, out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(ns))
    assert rc == sbam.SBAM_OK, rc
    return out[:n.value].tobytes(), ns.value


def literal_only_stored(block: bytes) -> bool:
    """The writer's rule for a block without matches: stored when the fixed-Huffman form (3 header bits, 8 bits per
    byte below 144 and 9 above, 7 bits of end-of-block) is larger than the 5 + n bytes of the stored form."""
    bits = 3 + sum(8 if b < 144 else 9 for b in block) + 7
    return (bits + 7) // 8 > len(block) + 5


@pytest.fixture(scope="module")
def inflated():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gzip.decompress(fixture_bytes(name))
        return cache[name]
    return get


def _fill(name, n, inflated):
    rng = np.random.default_rng(0xDEF1A7E)
    if name == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if name == "random_ge144":
        return rng.integers(144, 256, n, dtype=np.uint8).tobytes()
    if name == "zeros":
        return bytes(n)
    if name == "ones":
        return b"\xff" * n
    if name.startswith("period"):
        k = int(name[6:])
        unit = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
        return (unit * (n // k + 1))[:n]
    assert name == "5k"
    return inflated("5k.bam")[:128 << 10][:n]


FILLS = ["random", "random_ge144", "zeros", "ones", "period2", "period3", "period7", "period255", "period259", "5k"]


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("fill", FILLS)
def test_deflate_sizes_and_fills(fill, level, inflated):
    """Sizes around every path change (empty, below the minimum match, one row of 64, the maximum match, one block,
    two blocks) over random, all-9-bit, constant, periodic and BAM bytes: every block is valid, and n_stored_blocks
    counts the blocks that are in the stored form.  Random fills have no matches, so their blocks are stored exactly
    when the literal-only fixed-Huffman form is larger than the stored one (every block of 257 bytes or more; a block
    of a few bytes is smaller as Huffman, e.g. 1 byte: 3 bytes against 6)."""
    for n in SIZES:
        data = _fill(fill, n, inflated)
        whole, n_stored = deflate(data, 0, level)
        blocks = check_bgzf(whole, data)
        assert len(blocks) == (n + BB - 1) // BB
        assert n_stored == sum(b[3] for b in blocks), (fill, n)
        if level == 0:
            assert all(b[3] for b in blocks)
        elif fill.startswith("random"):
            want = [literal_only_stored(data[o:o + BB]) for o in range(0, n, BB)]
            assert [b[3] for b in blocks] == want, (fill, n)
            if n >= 257:
                assert blocks[0][3]
        elif n >= 65497 and fill != "5k":  # constant and periodic bytes collapse into long matches
            assert not blocks[0][3] and blocks[0][1] < 26 + 4000, (fill, n, blocks[0])


def test_deflate_distance_limits():
    """Bytes below 144 (8-bit literals, no repeats but the one built in) whose second half repeats the first at
    distance exactly 32768: matches are the only way under one byte per byte, and at least half of the repeated bytes
    must go into them (a lane finds the repeat only when no later position took its bucket, but one lane per row is
    enough to start a 258-byte match).  With the repeat at 32769 no match is allowed: every byte is a literal and the
    stream still decodes."""
    rng = np.random.default_rng(32768)
    r = rng.integers(0, 144, 32769, dtype=np.uint8).tobytes()
    at = r[:32768] + r[:32730]
    whole, _ = deflate(at)
    (blk,) = check_bgzf(whole, at)
    assert not blk[3] and blk[1] - 26 < 32768 + 32730 // 2, blk
    past = r + r[:32729]
    whole, _ = deflate(past)
    (blk,) = check_bgzf(whole, past)
    assert blk[1] - 26 >= len(past), blk


def test_deflate_every_match_length():
    """A 300-byte random prefix P, then P[:L] + a separator for every L in 3..258."""
    rng = np.random.default_rng(258)
    p = rng.integers(0, 144, 300, dtype=np.uint8).tobytes()
    data = p + b"".join(p[:n] + bytes([144 + n % 112]) for n in range(3, 259))
    whole, _ = deflate(data)
    (blk,) = check_bgzf(whole, data)
    assert not blk[3] and blk[1] < len(data) // 4


@pytest.mark.parametrize("block_bytes", [1, 64, 4096, 65498])
def test_deflate_block_bytes(block_bytes, inflated):
    """70000 bytes cut every 1, 64, 4096 and 65498 bytes: every block inflates on its own (no match reaches into the
    block before), at both levels; 70000 one-byte blocks also run through more than one batch of slots."""
    data = inflated("5k.bam")[:70000]
    for level in (0, 1):
        whole, _ = deflate(data, block_bytes, level)
        blocks = check_bgzf(whole, data, block_bytes)
        assert len(blocks) == (70000 + block_bytes - 1) // block_bytes


def test_deflate_is_deterministic(inflated):
    data = inflated("5k.bam")[:128 << 10]
    for bb in (0, 64):
        a, b = deflate(data, bb), deflate(data, bb)
        assert a == b


def test_deflate_argument_errors():
    import sbam
    L = sbam.load_library()
    out = np.zeros(64, np.uint8)
    n = ctypes.c_int64(0)
    one = np.ones(1, np.uint8)
    for bb, level in ((-1, 1), (65499, 1), (0, 2)):
        assert L.sbam_test_deflate(0, one.ctypes.data, 1, bb, level, 1, out.ctypes.data, 64, ctypes.byref(n),
                                   None) == sbam.ERR_ARG
    assert L.sbam_test_deflate(0, one.ctypes.data, 1, 0, 1, 1, out.ctypes.data, 10, ctypes.byref(n), None) == sbam.ERR_ARG
    assert n.value > 10


# ---- the reference's golden ------------------------------------------------------------------------------------
def _sidecar(name):
    with open(os.path.join(FIXTURES, name)) as fh:
        return [tuple(int(v) for v in ln.split(",")) for ln in fh if ln.strip()]


def _ordinals(starts, block_pos, offsets):
    return list(zip(np.searchsorted(np.asarray(starts), np.asarray(block_pos)).tolist(), np.asarray(offsets).tolist()))


@pytest.fixture(scope="module")
def two_bam():
    import sbam
    with sbam.BamFile(fixture_bytes("2.bam"), path="2.bam") as f:
        f.load_records(SPLIT, columns=None)
        yield f


@pytest.mark.parametrize("level", [0, 1])
def test_reference_golden(two_bam, level, inflated):
    """htsjdk-rewrite -r 100-1000 2.bam (HTSJDKRewriteTest.scala:14-24): the same uncompressed blocks, bytes and record
    positions as the reference's writer left in 2.100-1000.bam, .blocks and .records; the output passes check_crc and
    its own index-records agrees with written_records()."""
    import sbam
    from sbam.cli import index_records_lines
    f = two_bam
    want = inflated("2.100-1000.bam")
    gold_blocks, gold_records = _sidecar("2.100-1000.bam.blocks"), _sidecar("2.100-1000.bam.records")
    r = f.write_bam(ranges=[(100, 1000)], level=level)
    whole = r["bytes"]
    blocks = check_bgzf(whole, want)
    st, cs, us = f.written_blocks()
    assert us.tolist() == [b[2] for b in gold_blocks] == [65498] * 8 + [54346]
    assert [(a, b, c) for a, b, c, _ in blocks] == list(zip(st.tolist(), cs.tolist(), us.tolist()))
    assert r["n_records"] == 900 == len(gold_records) and r["ubytes"] == len(want) == 578330
    assert r["header_bytes"] == 5650 and r["n_blocks"] == 9 and r["comp_bytes"] == len(whole)
    assert r["n_stored_blocks"] == (9 if level == 0 else sum(b[3] for b in blocks))
    bp, bo = f.written_records()
    got = _ordinals(st, bp, bo)
    assert got == _ordinals([b[0] for b in gold_blocks], [p for p, _ in gold_records], [o for _, o in gold_records])
    with sbam.BamFile(whole, path="rewritten.bam") as g:
        c = g.check_crc()
        assert c["n_bad"] == 0 and c["n_blocks"] == 9  # (the block table ends at the EOF block)
        assert index_records_lines(g) == [f"{p},{o}" for p, o in zip(bp.tolist(), bo.tolist())]


# ---- selections ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five_k():
    import sbam
    with sbam.BamFile(fixture_bytes("5k.bam"), path="5k.bam") as f:
        _, cols = f.load_records(SPLIT, columns=("offset", "block_size", "flag_nc"))
        u = f.read_uncompressed(0, f.uncompressed_size)
        yield f, cols, u, f.offset_of(f.header_end)


def _host_selection(u, header_end, cols, mask, with_header=True):
    parts = [u[:header_end]] if with_header else []
    off, bs = cols["offset"].tolist(), cols["block_size"].tolist()
    parts += [u[off[i]:off[i] + 4 + bs[i]] for i in np.flatnonzero(mask).tolist()]
    return b"".join(parts)


def _range_mask(n, ranges):
    m = np.zeros(n, bool)
    for lo, hi in ranges:
        m[lo:hi] = True
    return m


@pytest.mark.parametrize("case", ["keep", "ranges", "both", "empty", "all"])
def test_selections(five_k, case):
    """keep = mapped reads (a numpy array, uploaded), three disjoint ranges, both ANDed, nothing, everything: the
    output inflates to the header plus the same records picked on the host from load_records' offsets, and the written
    records' positions are where those records start in the new stream."""
    f, cols, u, hx = five_k
    n = cols["offset"].size
    mapped = ((cols["flag_nc"] >> 16) & 4) == 0
    ranges = [(3, 40), (40, 41), (n - 700, n - 1)]
    keep, rg, mask = None, None, np.ones(n, bool)
    if case in ("keep", "both"):
        keep = mapped
        mask = mask & mapped
    if case in ("ranges", "both"):
        rg = ranges
        mask = mask & _range_mask(n, ranges)
    if case == "empty":
        rg = [(5, 5)]
        mask = np.zeros(n, bool)
    assert case in ("empty", "all") or 0 < mask.sum() < n
    want = _host_selection(u, hx, cols, mask)
    r = f.write_bam(ranges=rg, keep=keep, level=1)
    check_bgzf(r["bytes"], want)
    assert r["n_records"] == int(mask.sum()) and r["ubytes"] == len(want) and r["header_bytes"] == hx
    if case == "empty":
        assert r["n_blocks"] == 1 and r["ubytes"] == hx  # the header's block and the EOF block
    st, _, _ = f.written_blocks()
    bp, bo = f.written_records()
    sizes = 4 + cols["block_size"][mask].astype(np.int64)
    starts = hx + np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes.size else np.zeros(0, np.int64)
    assert np.array_equal(np.searchsorted(st, bp) * BB + bo, starts)
    if case == "keep":  # bool or uint8: the same file
        assert f.write_bam(keep=mapped.astype(np.uint8))["bytes"] == r["bytes"]
        with pytest.raises(ValueError):
            f.write_bam(keep=mapped[:-1])


_TENSOR_CHILD = """
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
import sbam
with sbam.BamFile(open(sys.argv[1], "rb").read()) as f:
    _, cols = f.load_records(int(sys.argv[3]), columns=("flag_nc",))
    flag = torch.from_numpy(cols["flag_nc"].astype(np.int64)).to("cuda:0") >> 16
    keep = (flag & 4) == 0
    assert keep.is_cuda and keep.dtype == torch.bool
    f.write_bam(sys.argv[2], keep=keep)
"""


def test_keep_device_tensor(five_k, tmp_path):
    """keep = (flag & 4) == 0 computed as a torch bool tensor on the device: its pointer goes to the kernel as it is.
    (A child process that initialises torch first: torch and libsbam.so then share one HIP runtime.)"""
    import subprocess
    import sys
    from conftest import ROOT
    f, cols, u, hx = five_k
    out = tmp_path / "mapped.bam"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "spark-bam_amd"))
    p = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, os.path.join(FIXTURES, "5k.bam"), str(out), str(SPLIT)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    mapped = ((cols["flag_nc"] >> 16) & 4) == 0
    assert 0 < mapped.sum() < mapped.size
    check_bgzf(out.read_bytes(), _host_selection(u, hx, cols, mapped))


def test_shards_concatenate(five_k):
    """with_header / with_eof: header + first half, then second half + EOF, concatenated, are one valid BAM that
    inflates to the whole-file output's bytes."""
    f, cols, u, hx = five_k
    n = cols["offset"].size
    whole = f.write_bam()["bytes"]
    want = _host_selection(u, hx, cols, np.ones(n, bool))
    assert gzip.decompress(whole) == want
    a = f.write_bam(ranges=[(0, n // 2)], with_eof=False)["bytes"]
    b = f.write_bam(ranges=[(n // 2, n)], with_header=False)["bytes"]
    cut = len(_host_selection(u, hx, cols, _range_mask(n, [(0, n // 2)])))
    check_bgzf(a, want[:cut], with_eof=False)
    check_bgzf(b, want[cut:])
    assert gzip.decompress(a + b) == want


def test_long_reads_cross_blocks():
    """The long-read generator at its smallest size: records larger than a block are laid across block boundaries."""
    import sbam
    import synth
    s = synth.SynthBam(tile_mb=1, copies=1, read_len=0, threads=8)
    with sbam.BamFile(s.bytes(), path="long.bam") as f:
        _, cols = f.load_records(32 << 20, columns=("offset", "block_size"))
        n = cols["offset"].size
        assert n > 4 and int(cols["block_size"].max()) > BB
        big = int(np.argmax(cols["block_size"]))
        lo, hi = max(0, big - 3), min(n, big + 3)
        u = f.read_uncompressed(0, f.uncompressed_size)
        want = _host_selection(u, f.offset_of(f.header_end), cols, _range_mask(n, [(lo, hi)]))
        for level in (0, 1):
            r = f.write_bam(ranges=[(lo, hi)], level=level)
            check_bgzf(r["bytes"], want)
            assert r["n_records"] == hi - lo and r["n_blocks"] >= 2


# ---- errors ----------------------------------------------------------------------------------------------------
def test_errors():
    """No records loaded and with_header on a shard are SBAM_ERR_STATE; ranges out of order, overlapping or past the
    end and block_bytes out of range are SBAM_ERR_ARG."""
    import sbam
    data = fixture_bytes("2.bam")
    with sbam.BamFile(data, path="2.bam") as f:
        with pytest.raises(sbam.SbamError) as ei:
            f.write_bam()
        assert f.L.sbam_last_error(f.ctx).contents.code == sbam.ERR_STATE and "sbam_load_records" in str(ei.value)
        f.load_records(SPLIT, columns=None)
        n = f.n_loaded
        for kw in ({"ranges": [(10, 5)]}, {"ranges": [(0, 10), (5, 20)]}, {"ranges": [(20, 30), (0, 10)]},
                   {"ranges": [(0, n + 1)]}, {"ranges": [(-1, 3)]}, {"block_bytes": 65499}, {"block_bytes": -1},
                   {"level": 2}):
            with pytest.raises(sbam.SbamError):
                f.write_bam(**kw)
            assert f.L.sbam_last_error(f.ctx).contents.code == sbam.ERR_ARG, kw
        assert f.write_bam(ranges=[(0, n)], block_bytes=0)["n_records"] == n  # 0 = the default
        st = f.blocks()[0]
        lens = f.contig_lengths
    lo = int(st[2])
    assert lo < SPLIT
    with sbam.BamFile(data[lo:], base_offset=lo, file_size=len(data), contig_lengths=lens, path="2.bam") as g:
        g.load_records(SPLIT, first=1, columns=None)  # (split 0 starts in front of the shard)
        assert g.n_loaded > 0
        with pytest.raises(sbam.SbamError):
            g.write_bam()
        assert g.L.sbam_last_error(g.ctx).contents.code == sbam.ERR_STATE
        r = g.write_bam(with_header=False)  # a shard's records alone
        assert r["header_bytes"] == 0 and r["n_records"] == g.n_loaded


# ---- CLI -------------------------------------------------------------------------------------------------------
def test_cli_rewrite(tmp_path, inflated):
    """htsjdk-rewrite -r 100-1000 -b -i 2.bam OUT: OUT inflates to the golden's bytes, OUT.blocks' third column and
    OUT.records, mapped to (block ordinal, offset), equal the fixture's."""
    from sbam import cli
    out = tmp_path / "2.100-1000.bam"
    assert cli.main(["htsjdk-rewrite", "-r", "100-1000", "-b", "-i", os.path.join(FIXTURES, "2.bam"), str(out)]) == 0
    assert gzip.decompress(out.read_bytes()) == inflated("2.100-1000.bam")
    gold_blocks, gold_records = _sidecar("2.100-1000.bam.blocks"), _sidecar("2.100-1000.bam.records")
    blocks = [tuple(int(v) for v in ln.split(",")) for ln in open(str(out) + ".blocks") if ln.strip()]
    records = [tuple(int(v) for v in ln.split(",")) for ln in open(str(out) + ".records") if ln.strip()]
    assert [b[2] for b in blocks] == [b[2] for b in gold_blocks]
    assert _ordinals([b[0] for b in blocks], [p for p, _ in records], [o for _, o in records]) == \
        _ordinals([b[0] for b in gold_blocks], [p for p, _ in gold_records], [o for _, o in gold_records])


# ---- size ------------------------------------------------------------------------------------------------------
def test_level1_size_against_zlib(inflated):
    """Level 1 at 65498 bytes per block is at most 1.30x the same blocks through zlib level 1 (raw deflate + 26 bytes
    each) on the inflated 2.100-1000.bam (whole), 5k.bam and 1.bam (first 1.5 MB each).  The cap is 30 % over zlib:
    a CPU model of the simplest admissible encoder (4-byte hash, 2^13 one-entry buckets, greedy, minimum match 4,
    fixed Huffman, stored fallback) gave 1.166, 1.166 and 1.206; a model of this kernel's rows (candidates from
    earlier rows only) 1.216, 1.213 and 1.242."""
    ratios = {}
    for name, cut in (("2.100-1000.bam", None), ("5k.bam", 1500000), ("1.bam", 1500000)):
        u = inflated(name)[:cut]
        z = 0
        for o in range(0, len(u), BB):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z += len(c.compress(u[o:o + BB]) + c.flush()) + 26
        whole, _ = deflate(u, 0, 1, with_eof=False)
        check_bgzf(whole, u, with_eof=False)
        ratios[name] = len(whole) / z
        print(f"level-1 size ratio to zlib -1 on {name}: {ratios[name]:.4f} ({len(whole)} / {z})")
    assert all(r <= 1.30 for r in ratios.values()), ratios
