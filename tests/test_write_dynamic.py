"""The BAM writer's dynamic-Huffman mode (level 1 | SBAM_WRITE_DYNAMIC): per block the smallest of the stored form, the
fixed code and a dynamic code over the same LZ77 tokens as plain level 1.  Every output goes through
test_write_bam.check_bgzf; the kernel's code lengths are the host core's (test_deflate_dynamic_host's program) for the
tokens its own stream holds; the sizes are within 3 % of zlib level 1 and at most 0.85 of plain level 1; levels 0 and
1 give the bytes the parent commit gave (tests/golden/write_level1_digests.json)."""
import ctypes
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT, fixture_bytes
from test_deflate_dynamic_host import host, huffman, parse_dynamic, token_counts  # noqa: F401  (host: a fixture)
from test_write_bam import (BB, FILLS, SIZES, SPLIT, _fill, _host_selection, _ordinals, _range_mask,  # noqa: F401
                            _sidecar, check_bgzf, deflate, five_k, inflated, two_bam)

pytestmark = pytest.mark.gpu

DYN = 1 | 0x100  # 1 | SBAM_WRITE_DYNAMIC


def btypes(whole, blocks):
    return [(whole[p + 18] >> 1) & 3 for p, _, _, _ in blocks]


def payload(whole, block):
    return whole[block[0] + 18:block[0] + block[1] - 8]


def checked(data, block_bytes=0, with_eof=True):
    """deflate in the new mode, through check_bgzf -> (bytes, blocks, BTYPE per block)."""
    whole, n_stored = deflate(data, block_bytes, DYN, with_eof)
    blocks = check_bgzf(whole, data, block_bytes or BB, with_eof)
    bt = btypes(whole, blocks)
    assert n_stored == bt.count(0) == sum(b[3] for b in blocks)
    return whole, blocks, bt


def test_flag_value():
    import sbam
    assert DYN == 1 | sbam.SBAM_WRITE_DYNAMIC


@pytest.mark.parametrize("fill", FILLS)
def test_sizes_and_fills(fill, inflated):
    """test_write_bam's sizes and fills in the new mode: every block valid, n_stored_blocks the count of BTYPE-00
    payloads, and no block larger than the same block at plain level 1 (the same tokens, the smallest form).  A random
    block of 65498 bytes is stored, a 5k one has BTYPE 10, a 1-byte block BTYPE 01 in 3 bytes."""
    for n in SIZES:
        data = _fill(fill, n, inflated)
        whole, blocks, bt = checked(data)
        fixed, _ = deflate(data, 0, 1)
        fblocks = check_bgzf(fixed, data)
        assert len(blocks) == len(fblocks) == (n + BB - 1) // BB
        assert all(d[1] <= f[1] for d, f in zip(blocks, fblocks)), (fill, n, blocks, fblocks)
        if n == 1:
            assert bt == [1] and blocks[0][1] == 26 + 3, (fill, blocks)
        if n >= 65498 and fill == "random":
            assert bt[0] == 0, (fill, n)
        if n >= 65498 and fill == "random_ge144":  # 112 values: under 7 bits each as a dynamic code
            assert bt[0] == 2 and blocks[0][1] < 65498 * 7 // 8, (fill, n)
        if n >= 65498 and fill == "5k":
            assert bt[0] == 2 and blocks[0][1] < fblocks[0][1], (n, blocks[0], fblocks[0])


@pytest.mark.parametrize("block_bytes", [1, 64, 4096, 65498])
def test_block_bytes(block_bytes, inflated):
    """70000 bytes cut every 1, 64, 4096 and 65498 bytes; 70000 one-byte blocks run through 18 batches of 4096 slots
    (and through every workgroup's token record more than once)."""
    data = inflated("5k.bam")[:70000]
    _, blocks, bt = checked(data, block_bytes)
    assert len(blocks) == (70000 + block_bytes - 1) // block_bytes
    if block_bytes == 1:
        assert set(bt) == {1}
    if block_bytes >= 4096:
        assert bt[0] == 2


def test_reused_inputs():
    """The distance-limit pair and the every-match-length input of test_write_bam in the new mode; a block of zeros
    uses at most two distance codes; 300 bytes of period 259 (one match, one distance code)."""
    rng = np.random.default_rng(32768)
    r = rng.integers(0, 144, 32769, dtype=np.uint8).tobytes()
    at = r[:32768] + r[:32730]
    _, (blk,), bt = checked(at)
    assert bt == [2] and blk[1] - 26 < 32768 + 32730 // 2, blk
    past = r + r[:32729]
    whole, (blk,), bt = checked(past)
    assert bt == [2] and not any(t[0] == "M" for t in parse_dynamic(payload(whole, blk))["tokens"])
    rng = np.random.default_rng(258)
    p = rng.integers(0, 144, 300, dtype=np.uint8).tobytes()
    data = p + b"".join(p[:n] + bytes([144 + n % 112]) for n in range(3, 259))
    whole, (blk,), bt = checked(data)
    assert bt[0] != 0 and blk[1] < len(data) // 4
    for n in (65498, 4096, 300):
        whole, (blk,), bt = checked(bytes(n))
        assert bt[0] != 0
        if bt[0] == 2:
            d = parse_dynamic(payload(whole, blk))
            assert [v for v in d["dist"] if v] == [1, 1], (n, d["dist"])  # the one in use and the pair's other
    unit = np.random.default_rng(259).integers(0, 256, 259, dtype=np.uint8).tobytes()
    checked((unit * 2)[:300])


def test_length_limits():
    """A 46367-byte block whose byte histogram is Fibonacci (1, 1, 2, 3, ... 17711 over 22 values and the end of block,
    order shuffled): whatever tokens the search finds, the block inflates."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(46367)
    values = rng.permutation(256)[:22]
    data = np.repeat(values.astype(np.uint8), fib)
    assert data.size == 46367
    rng.shuffle(data)
    _, _, bt = checked(data.tobytes())
    assert bt == [2]


@pytest.mark.parametrize("name", ["5k.bam", "1.bam"])
def test_host_and_device_agree(name, inflated, host):
    """The first 65498 inflated bytes: the kernel's dynamic header parsed here (HLIT, HDIST, HCLEN, the lengths), its
    tokens decoded and counted, and the host program's code builder run on those counts: the header's three length
    arrays are the host's."""
    data = inflated(name)[:BB]
    whole, (blk,), bt = checked(data)
    assert bt == [2]
    d = parse_dynamic(payload(whole, blk))
    lc, dc = token_counts(d["tokens"])
    assert d["lit"] == host.build_lengths(lc, 15)
    assert d["dist"] == host.build_lengths(dc, 15)
    cl_counts = np.bincount(d["cl_used"], minlength=19).tolist()
    assert d["cl"] == host.build_lengths(cl_counts, 7)
    print(f"{name}: header {d['header_bits']} bits, HLIT {d['hlit']} HDIST {d['hdist']} HCLEN {d['hclen']}, longest "
          f"lit/dist/cl code {max(d['lit'])}/{max(d['dist'])}/{max(d['cl'])}, unlimited code-length code depth "
          f"{huffman(cl_counts)[1]}, {len(d['tokens'])} tokens")


def test_is_deterministic(inflated):
    data = inflated("5k.bam")[:128 << 10]
    for bb in (0, 64):
        assert deflate(data, bb, DYN) == deflate(data, bb, DYN)


def test_reference_golden(two_bam, inflated):
    """htsjdk-rewrite -r 100-1000 2.bam in the new mode: the uncompressed side is the reference golden's, nine blocks
    (eight of 65498 bytes, one of 54346), the .records positions at the same (block ordinal, offset) pairs."""
    import sbam
    f = two_bam
    want = inflated("2.100-1000.bam")
    gold_blocks, gold_records = _sidecar("2.100-1000.bam.blocks"), _sidecar("2.100-1000.bam.records")
    r = f.write_bam(ranges=[(100, 1000)], level=1, huffman="dynamic")
    whole = r["bytes"]
    blocks = check_bgzf(whole, want)
    st, cs, us = f.written_blocks()
    assert us.tolist() == [b[2] for b in gold_blocks] == [65498] * 8 + [54346]
    assert [(a, b, c) for a, b, c, _ in blocks] == list(zip(st.tolist(), cs.tolist(), us.tolist()))
    assert r["n_records"] == 900 and r["ubytes"] == len(want) and r["n_blocks"] == 9 and r["comp_bytes"] == len(whole)
    assert r["n_stored_blocks"] == 0 and btypes(whole, blocks) == [2] * 9
    bp, bo = f.written_records()
    assert _ordinals(st, bp, bo) == _ordinals([b[0] for b in gold_blocks], [p for p, _ in gold_records],
                                              [o for _, o in gold_records])
    assert r["bytes"] == f.write_bam(ranges=[(100, 1000)], level=1 | sbam.SBAM_WRITE_DYNAMIC)["bytes"]


def test_round_trip_through_the_library(five_k):
    """5k.bam written whole in the new mode and opened again: no block this writer makes goes to the inflater's exact
    per-lane path (inflate_fallbacks equals the stored blocks), every CRC32 matches, and the records decode to the
    columns of the source (all but the compressed-side block_pos)."""
    import sbam
    f, _, u, _ = five_k
    _, src = f.load_records(SPLIT)
    r = f.write_bam(huffman="dynamic")
    with sbam.BamFile(r["bytes"], path="rewritten.bam") as g:
        assert g.uncompressed_size == len(u) and g.read_uncompressed(0, len(u)) == u
        assert g.inflate_fallbacks() == r["n_stored_blocks"]
        c = g.check_crc()
        assert c["n_bad"] == 0 and c["n_blocks"] == r["n_blocks"]
        _, cols = g.load_records(SPLIT)
        assert cols["offset"].size == src["offset"].size == r["n_records"]
        for k in src:
            if k not in ("block_pos", "block_off"):
                assert np.array_equal(cols[k], src[k]), k
        reads = [x for part in g.load_reads(SPLIT) for x in part]
    with sbam.BamFile(fixture_bytes("5k.bam"), path="5k.bam") as h:
        assert reads == [x for part in h.load_reads(SPLIT) for x in part]


def test_selection_and_shards(five_k):
    """keep ANDed with ranges, and the two-shard concatenation, in the new mode against the selection made on the
    host."""
    f, cols, u, hx = five_k
    n = cols["offset"].size
    mapped = ((cols["flag_nc"] >> 16) & 4) == 0
    ranges = [(3, 40), (40, 41), (n - 700, n - 1)]
    mask = mapped & _range_mask(n, ranges)
    assert 0 < mask.sum() < n
    want = _host_selection(u, hx, cols, mask)
    r = f.write_bam(ranges=ranges, keep=mapped, huffman="dynamic")
    check_bgzf(r["bytes"], want)
    assert r["n_records"] == int(mask.sum()) and r["ubytes"] == len(want)
    want = _host_selection(u, hx, cols, np.ones(n, bool))
    a = f.write_bam(ranges=[(0, n // 2)], with_eof=False, huffman="dynamic")["bytes"]
    b = f.write_bam(ranges=[(n // 2, n)], with_header=False, huffman="dynamic")["bytes"]
    cut = len(_host_selection(u, hx, cols, _range_mask(n, [(0, n // 2)])))
    check_bgzf(a, want[:cut], with_eof=False)
    check_bgzf(b, want[cut:])
    assert gzip.decompress(a + b) == want


def test_errors(two_bam):
    """0 | SBAM_WRITE_DYNAMIC, 1 | 0x200 and 2 | SBAM_WRITE_DYNAMIC are SBAM_ERR_ARG from sbam_test_deflate and from
    sbam_write_bam; write_bam(level=0, huffman="dynamic") raises before the library is called."""
    import sbam
    L = sbam.load_library()
    out = np.zeros(64, np.uint8)
    n = ctypes.c_int64(0)
    one = np.ones(1, np.uint8)
    for level in (0 | 0x100, 1 | 0x200, 2 | 0x100, 1 | 0x100 | 0x200, -1):
        assert L.sbam_test_deflate(0, one.ctypes.data, 1, 0, level, 1, out.ctypes.data, 64, ctypes.byref(n),
                                   None) == sbam.ERR_ARG, level
        with pytest.raises(sbam.SbamError) as ei:
            two_bam.write_bam(level=level)
        assert two_bam.L.sbam_last_error(two_bam.ctx).contents.code == sbam.ERR_ARG, level
        assert "SBAM_WRITE_DYNAMIC" in str(ei.value)
    assert L.sbam_test_deflate(0, one.ctypes.data, 1, 0, DYN, 1, out.ctypes.data, 64, ctypes.byref(n), None) == sbam.SBAM_OK
    with pytest.raises(ValueError):
        two_bam.write_bam(level=0, huffman="dynamic")
    with pytest.raises(ValueError):
        two_bam.write_bam(huffman="static")


def test_size_against_zlib_and_level1(inflated):
    """At 65498 bytes per block on test_level1_size_against_zlib's three streams: at most 1.03 x the same blocks through
    zlib level 1 (a model of this kernel's tokens under optimal codes gave 1.0035, 0.9993 and 1.0066), and at most
    0.85 x this library's plain level 1 (the model: 0.8251, 0.8237, 0.8104)."""
    ratios = {}
    for name, cut in (("2.100-1000.bam", None), ("5k.bam", 1500000), ("1.bam", 1500000)):
        u = inflated(name)[:cut]
        z = 0
        for o in range(0, len(u), BB):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z += len(c.compress(u[o:o + BB]) + c.flush()) + 26
        whole, _ = deflate(u, 0, DYN, with_eof=False)
        check_bgzf(whole, u, with_eof=False)
        fixed, _ = deflate(u, 0, 1, with_eof=False)
        ratios[name] = (len(whole) / z, len(whole) / len(fixed))
        print(f"dynamic size on {name}: {ratios[name][0]:.4f} x zlib -1 ({len(whole)} / {z}), "
              f"{ratios[name][1]:.4f} x plain level 1 ({len(whole)} / {len(fixed)})")
    assert all(a <= 1.03 and b <= 0.85 for a, b in ratios.values()), ratios


def test_levels_0_and_1_did_not_move(inflated):
    """The outputs of levels 0 and 1 on the size streams (65498 bytes per block, no EOF block) and on the first 128 KiB
    of 5k.bam at 64 bytes per block have the SHA-256 recorded on the commit named in the golden file, which had no
    dynamic mode."""
    with open(os.path.join(ROOT, "tests", "golden", "write_level1_digests.json")) as fh:
        gold = json.load(fh)["digests"]
    got = {}
    for level in (0, 1):
        for name, cut in (("2.100-1000.bam", None), ("5k.bam", 1500000), ("1.bam", 1500000)):
            whole, _ = deflate(inflated(name)[:cut], 0, level, with_eof=False)
            got[f"level{level}:{name}:bb0:noeof"] = hashlib.sha256(whole).hexdigest()
        whole, _ = deflate(inflated("5k.bam")[:128 << 10], 64, level)
        got[f"level{level}:5k.bam[:131072]:bb64:eof"] = hashlib.sha256(whole).hexdigest()
    assert got == gold
