"""The BGZF block CRC32 check on the GPU (sbam_check_crc, verify_crc, check_crc_file, `check-crc`) against zlib.crc32.

The BGZF files are built here with real CRCs (tests/test_inflate_streams.py's bgzf_block writes a zero CRC field).  They
are not BAMs: contexts are opened with inflate=False and inflated by hand, so sbam_header never runs."""
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import ALL_BAMS, FIXTURES, GOLDEN, fixture_bytes
from test_inflate_streams import EOF_BLOCK

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383,
           16384, 16385, 65279, 65280]


def crc_block(data: bytes, level: int = 0, crc=None) -> bytes:
    """One BGZF block of `data` (level 0: stored) with its CRC32 (or `crc`) and ISIZE in the footer."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = c.compress(data) + c.flush()
    bsize = 18 + len(payload) + 8 - 1
    assert bsize < 65536, len(data)
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize)
    return hdr + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data))


def bgzf_file(chunks, level=0) -> bytes:
    return b"".join(crc_block(d, level) for d in chunks) + EOF_BLOCK


def open_bgzf(data, **kw):
    import sbam
    f = sbam.BamFile(data, inflate=False, **kw)
    f.inflate()
    return f


def block_starts(data: bytes):
    out, pos = [], 0
    while pos < len(data):
        out.append(pos)
        pos += int.from_bytes(data[pos + 16:pos + 18], "little") + 1
    return out[:-1]  # (without the EOF block)


def stored_file(seed: int, n: int = 40):
    r = np.random.default_rng(seed)
    chunks = [r.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in r.integers(100, 3000, n)]
    return chunks, bytearray(bgzf_file(chunks))


@pytest.mark.parametrize("name", ALL_BAMS)
def test_fixture_crcs(name):
    """Every block of every fixture: computed == stored == zlib.crc32 of the block's inflated bytes."""
    import sbam
    with sbam.BamFile(fixture_bytes(name), path=name) as f:
        r = f.check_crc()
        st, cs, us, uo = f.blocks()
        assert r["n_blocks"] == st.size and r["n_bad"] == 0 and r["first_bad"] == -1 and r["bad"].size == 0
        assert r["bytes"] == f.uncompressed_size
        computed, stored = f.block_crcs()
        want = np.array([zlib.crc32(f.read_uncompressed(int(o), int(n))) for o, n in zip(uo, us)], np.uint32)
        assert np.array_equal(computed, want) and np.array_equal(stored, want)
        assert f.kernel_ms("crc") > 0


def test_lengths_and_alignments():
    """Stored random blocks of every length at which the kernel takes another path (pieces, rows, the cut last piece),
    zlib-6 blocks of 65535 and 65536 bytes (sbam_inflate accepts ISIZE up to 65536), small blocks added until the
    blocks' stream offsets take every value mod 16, then all-0x00 and all-0xFF blocks, whose CRCs differ only through
    the init term."""
    r = np.random.default_rng(7)
    chunks = [r.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENGTHS]
    blocks = [crc_block(d) for d in chunks]
    for n in (65535, 65536):  # compressible: 16 symbols
        d = r.integers(0, 16, n, dtype=np.uint8).tobytes()
        chunks.append(d)
        blocks.append(crc_block(d, 6))
    offs = np.cumsum([0] + [len(d) for d in chunks])
    seen, cur = set(int(o) % 16 for o in offs[:-1]), int(offs[-1])
    for want in range(16):
        if want in seen:
            continue
        for n in ((want - cur) % 16 or 16, 100):  # a filler that ends at the missing alignment, then a block there
            chunks.append(r.integers(0, 256, n, dtype=np.uint8).tobytes())
            blocks.append(crc_block(chunks[-1]))
            seen.add(cur % 16)
            cur += n
    for fill in (b"\0", b"\xff"):
        for n in (1, 2, 64, 1024, 65280):
            chunks.append(fill * n)
            blocks.append(crc_block(chunks[-1]))
    assert zlib.crc32(b"\0") != zlib.crc32(b"\0\0")
    with open_bgzf(b"".join(blocks) + EOF_BLOCK) as f:
        uo = f.blocks()[3]
        assert uo.size == len(chunks) and set((uo % 16).tolist()) == set(range(16))
        res = f.check_crc()
        computed, stored = f.block_crcs()
        want = np.array([zlib.crc32(d) for d in chunks], np.uint32)
        for b in range(len(chunks)):
            assert computed[b] == want[b], (b, len(chunks[b]), int(uo[b]) % 16)
        assert np.array_equal(stored, want) and res["n_bad"] == 0


def test_many_small_blocks():
    """3000 blocks of 1..200 bytes: more blocks than a workgroup has waves, and than the grid has workgroups' first
    pass; the scan's > 512-candidates path."""
    r = np.random.default_rng(11)
    chunks = [r.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in r.integers(1, 201, 3000)]
    with open_bgzf(bgzf_file(chunks)) as f:
        res = f.check_crc()
        computed, stored = f.block_crcs()
        want = np.array([zlib.crc32(d) for d in chunks], np.uint32)
        assert res["n_blocks"] == 3000 and res["n_bad"] == 0 and res["bytes"] == sum(map(len, chunks))
        assert np.array_equal(computed, want) and np.array_equal(stored, want)


def flip_footer(data: bytearray, starts, b: int, bit: int = 0):
    """Flip one bit of block b's stored CRC."""
    end = starts[b + 1] if b + 1 < len(starts) else len(data) - len(EOF_BLOCK)
    data[end - 8 + bit // 8] ^= 1 << (bit % 8)


def test_detects_corruption():
    """A 40-block stored file: one bit of the footer CRC of block 0, 17 and the last, one payload byte of a stored
    block (inflate still succeeds), and two of these at once: n_bad, first_bad, bad and bad_offsets are exact and every
    other block's computed value is unchanged."""
    chunks, good = stored_file(3)
    starts = block_starts(bytes(good))
    want = np.array([zlib.crc32(d) for d in chunks], np.uint32)

    def run(data, bad, changed=None):
        with open_bgzf(bytes(data)) as f:
            r = f.check_crc()
            computed, stored = f.block_crcs()
        assert r["n_blocks"] == 40 and r["n_bad"] == len(bad) and r["first_bad"] == (bad[0] if bad else -1)
        assert r["bad"].tolist() == bad and r["bad_offsets"].tolist() == [starts[b] for b in bad]
        w = want.copy()
        for b, v in (changed or {}).items():
            w[b] = v
        assert np.array_equal(computed, w)
        return stored

    assert np.array_equal(run(good, []), want)
    for b, bit in ((0, 0), (17, 13), (39, 31)):
        d = bytearray(good)
        flip_footer(d, starts, b, bit)
        stored = run(d, [b])
        assert stored[b] == want[b] ^ (1 << bit) and np.array_equal(np.delete(stored, b), np.delete(want, b))
    # a payload byte of stored block 23: 18 header bytes, 5 of the stored DEFLATE block, then the data
    d = bytearray(good)
    assert d[starts[23] + 18 + 5 + 7] == chunks[23][7]
    d[starts[23] + 18 + 5 + 7] ^= 0x40
    c23 = bytearray(chunks[23])
    c23[7] ^= 0x40
    run(d, [23], {23: zlib.crc32(bytes(c23))})
    flip_footer(d, starts, 5, 9)
    run(d, [5, 23], {23: zlib.crc32(bytes(c23))})


@pytest.mark.parametrize("level", [1, 6, 9, 12])
def test_libdeflate_corpus_zero_footers(level):
    """The libdeflate-written corpus has a zero CRC field: every block of the table is reported bad, computed is
    zlib.crc32 of the block as zlib inflates it, stored is zero."""
    with open(os.path.join(GOLDEN, "deflate", "libdeflate_l%d.bgzf" % level), "rb") as fh:
        data = fh.read()
    starts = block_starts(data)
    want = []
    for s in starts:
        bsize = int.from_bytes(data[s + 16:s + 18], "little") + 1
        want.append(zlib.crc32(zlib.decompress(data[s + 18:s + bsize - 8], -15)))
    assert len(starts) == 13
    with open_bgzf(data) as f:
        r = f.check_crc()
        computed, stored = f.block_crcs()
    assert r["n_blocks"] == 13 and r["n_bad"] == 13 and r["first_bad"] == 0 and r["bad"].tolist() == list(range(13))
    assert r["bad_offsets"].tolist() == starts
    assert np.array_equal(computed, np.array(want, np.uint32)) and not stored.any()


def test_ranges_and_state():
    """Subranges, the empty range, bad ranges (SBAM_ERR_ARG), and SBAM_ERR_STATE before inflate, after reset and after
    load until the stages run again; block_crcs outside the checked range."""
    import ctypes
    import sbam
    chunks, data = stored_file(5)
    want = np.array([zlib.crc32(d) for d in chunks], np.uint32)
    L = sbam.load_library()
    t = sbam._CrcTotals()
    with sbam.BamFile(bytes(data), inflate=False) as f:
        assert L.sbam_check_crc(f.ctx, 0, -1, ctypes.byref(t)) == sbam.ERR_STATE
        assert L.sbam_get_block_crcs(f.ctx, 0, 1, None, None) == sbam.ERR_STATE
        f.inflate()
        assert L.sbam_get_block_crcs(f.ctx, 0, 1, None, None) == sbam.ERR_STATE  # no check yet
        r = f.check_crc(7, 19)
        assert (r["n_blocks"], r["n_bad"], r["first_bad"]) == (12, 0, -1)
        assert r["bytes"] == sum(len(d) for d in chunks[7:19])
        computed, stored = f.block_crcs()
        assert np.array_equal(computed, want[7:19]) and np.array_equal(stored, want[7:19])
        assert np.array_equal(f.block_crcs(10, 3)[0], want[10:13])
        for b0, n in ((6, 2), (18, 2), (0, 40)):
            assert L.sbam_get_block_crcs(f.ctx, b0, n, None, None) == sbam.ERR_STATE
        with pytest.raises(sbam.SbamError):
            f.block_crcs(0, 40)
        assert L.sbam_get_block_crcs(f.ctx, -1, 2, None, None) == sbam.ERR_ARG
        r = f.check_crc(5, 5)
        assert (r["n_blocks"], r["n_bad"], r["first_bad"], r["bytes"]) == (0, 0, -1, 0) and r["bad"].size == 0
        r = f.check_crc(39)
        assert r["n_blocks"] == 1 and f.block_crcs()[0].tolist() == [want[39]]
        for b0, b1 in ((-1, 3), (5, 4), (0, 41), (41, 41)):
            assert L.sbam_check_crc(f.ctx, b0, b1, ctypes.byref(t)) == sbam.ERR_ARG
        assert L.sbam_check_crc(f.ctx, 0, -1, None) == sbam.SBAM_OK  # totals may be NULL
        f.reset()
        assert L.sbam_check_crc(f.ctx, 0, -1, ctypes.byref(t)) == sbam.ERR_STATE
        assert L.sbam_get_block_crcs(f.ctx, 0, 1, None, None) == sbam.ERR_STATE
        f.n_blocks = f._scan()
        assert L.sbam_check_crc(f.ctx, 0, -1, ctypes.byref(t)) == sbam.ERR_STATE
        f.inflate()
        assert f.check_crc()["n_blocks"] == 40
        f.load(bytes(data))
        assert L.sbam_check_crc(f.ctx, 0, -1, ctypes.byref(t)) == sbam.ERR_STATE
        assert L.sbam_get_block_crcs(f.ctx, 0, 1, None, None) == sbam.ERR_STATE
        f.n_blocks = f._scan()
        f.inflate()
        assert L.sbam_get_block_crcs(f.ctx, 0, 1, None, None) == sbam.ERR_STATE  # a new stream: no check yet
        assert f.check_crc()["n_bad"] == 0 and np.array_equal(f.block_crcs()[0], want)


def test_verify_flag():
    """verify_crc=True: a fixture loads and decodes as without it; a corrupted file raises CrcException with the
    block's offset and both values; the context then loads good bytes; with the flag off the corrupted bytes load
    exactly as they always did."""
    import sbam
    bam = fixture_bytes("2.bam")
    with sbam.BamFile(bam) as f:
        sizes, cols = f.load_records(100000)
    with sbam.BamFile(bam, verify_crc=True) as f:
        assert f.kernel_ms("crc") > 0
        s2, c2 = f.load_records(100000)
        assert np.array_equal(s2, sizes) and all(np.array_equal(c2[k], cols[k]) for k in cols)
        assert not np.any(np.subtract(*f.block_crcs())) and f.block_crcs()[0].size == f.n_blocks
    chunks, good = stored_file(9)
    starts = block_starts(bytes(good))
    want = [zlib.crc32(d) for d in chunks]
    bad = bytearray(good)
    flip_footer(bad, starts, 21, 4)
    flip_footer(bad, starts, 30, 4)
    with pytest.raises(sbam.CrcException) as ei:
        open_bgzf(bytes(bad), verify_crc=True)
    e = ei.value
    assert (e.position, e.expected, e.actual) == (starts[21], want[21] ^ 16, want[21])
    assert str(e) == "CRC32 mismatch in block at %d: footer %08x, computed %08x" % (starts[21], want[21] ^ 16, want[21])
    assert isinstance(e, IOError)
    L = sbam.load_library()
    with sbam.BamFile(bytes(bad), inflate=False, verify_crc=True) as f:
        with pytest.raises(sbam.CrcException):
            f.inflate()
        assert L.sbam_read_uncompressed(f.ctx, 0, 0, None) == sbam.ERR_STATE  # the stream stage is unset
        f.load(bytes(good))  # the flag is sticky: this inflate checks too, and passes
        f.n_blocks = f._scan()
        n = f.inflate()
        assert f.read_uncompressed(0, n) == b"".join(chunks) and f.check_crc()["n_bad"] == 0
        f.load(bytes(bad))
        f.n_blocks = f._scan()
        with pytest.raises(sbam.CrcException):
            f.inflate()
        f.set_verify_crc(False)
        assert f.inflate() == n
    with open_bgzf(bytes(bad)) as f:  # flag off: loads as it always did
        assert f.read_uncompressed(0, f.uncompressed_size) == b"".join(chunks)
        assert f.check_crc()["bad"].tolist() == [21, 30]


def corrupt_5k(tmp_path):
    """5k.bam with the footers of two blocks far apart corrupted: (path, bytes, starts, the two block indices)."""
    data = bytearray(fixture_bytes("5k.bam"))
    starts = block_starts(bytes(data))
    pair = [3, len(starts) - 4]
    for b in pair:
        flip_footer(data, starts, b, 17)
    path = tmp_path / "5k.corrupt.bam"
    path.write_bytes(bytes(data))
    return str(path), bytes(data), starts, pair


def test_check_crc_file_windows(tmp_path):
    """check_crc_file over three byte-range windows gives the whole-file check's totals and bad blocks, each block
    counted once."""
    import sbam
    from sbam import dist
    path, data, starts, pair = corrupt_5k(tmp_path)
    split = 200 << 10
    plans = dist.plan_shards(len(data), split, 3)
    assert all(p.owned_hi > p.lo for p in plans)
    assert sum(p.lo <= starts[b] < p.owned_hi for p in plans for b in pair) == 2
    assert len({next(p.rank for p in plans if p.lo <= starts[b] < p.owned_hi) for b in pair}) == 2
    with sbam.BamFile(data) as f:
        whole = f.check_crc()
        computed, stored = f.block_crcs()
    assert whole["bad"].tolist() == pair
    r = dist.check_crc_file(path, world=3, split_size=split)
    assert (r["n_blocks"], r["n_bad"], r["bytes"]) == (whole["n_blocks"], 2, whole["bytes"])
    assert r["bad"] == [(starts[b], int(stored[b]), int(computed[b])) for b in pair]
    assert len(r["windows"]) == 3 and all(n > 0 for n in r["windows"]) and sum(r["windows"]) == len(starts)
    one = dist.check_crc_file(path, world=1)
    assert one["bad"] == r["bad"] and one["windows"] == [len(starts)]


def test_cli_check_crc(tmp_path, capsys):
    """`check-crc`: exit 0 and `All CRC32s match` on 2.bam; exit 1 and the two offsets on a corrupted 5k.bam, also in
    windows; `index-bam --verify-crc` on the corrupted copy fails with the exception's message and writes nothing."""
    from sbam import cli
    assert cli.main(["check-crc", os.path.join(FIXTURES, "2.bam")]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out == ["25 blocks, 1606522 uncompressed bytes checked", "All CRC32s match"]  # (+ the EOF block: 26)
    path, data, starts, pair = corrupt_5k(tmp_path)
    for extra in ([], ["--windows", "2"]):
        assert cli.main(["check-crc"] + extra + [path]) == 1
        out = capsys.readouterr().out.splitlines()
        assert out[0].startswith("%d blocks, " % len(starts)) and out[1] == "2 of %d blocks with a CRC32 mismatch:" % len(starts)
        assert [ln.split(":")[0] for ln in out[2:]] == ["\t%d" % starts[b] for b in pair] and len(out) == 4
    assert cli.main(["check-crc", "-l", "1", path]) == 1
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 4 and out[3] == "\t…"
    bai = tmp_path / "out.bai"
    assert cli.main(["index-bam", "--verify-crc", "-o", str(bai), path]) == 1
    err = capsys.readouterr().err
    assert "CRC32 mismatch in block at %d: footer " % starts[pair[0]] in err and not bai.exists()
    assert cli.main(["index-bam", "-o", str(bai), path]) == 0 and bai.exists()  # flag off: as before
