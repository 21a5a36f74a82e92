"""sbam_load_record_fields: names, CIGARs, bases, qualities and tags of decoded records as device CSR columns, against
the plain-Python reference decoder of tests/test_sam_text.py (itself pinned by the reference's 2.sam and 5k.sam).

* every fixture, split sizes 100 KiB and 1 << 40, record lists from the chain walk and from the success bitmap;
* `cli view` of 2.bam and 5k.bam against the reference's SAM text;
* hand-built records inserted into 2.bam's stream: the smallest shapes at which the gather's tiling, its source
  alignment, its nibble parity and its record search can go wrong (see handmade_bam);
* batches, field masks, arena reuse, long reads, state / argument errors, a record that overruns its block_size, and
  the layout of the two new ABI structs."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from conftest import ALL_BAMS, FIXTURES, ROOT, fixture_bytes
from test_eager_wave import bgzf
from test_sam_text import (DATA_COLUMNS, OFFSET_COLUMNS, decoded, golden_sam, record_chain, ref_fields, slice_fields,
                           stream_header)

gpu = pytest.mark.gpu
ALL = DATA_COLUMNS


def assert_fields(got, want, fields=ALL, what=""):
    for k in OFFSET_COLUMNS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), f"{what} {k}"
    for k in DATA_COLUMNS:
        if k in fields:
            g, w = getattr(got, k), getattr(want, k)
            assert g.dtype == w.dtype and g.size == w.size, f"{what} {k}: {g.size} vs {w.size}"
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{what} {k}: {bad.size} differ, first at {bad[:4]}: {g[bad[:4]]} vs {w[bad[:4]]}"
        else:
            assert getattr(got, k) is None, f"{what} {k} was not selected"


# ---- fixtures ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("split_size", [100 * 1024, 1 << 40])
@pytest.mark.parametrize("name", ALL_BAMS)
def test_fixture_columns(name, split_size, bitmap, gpu_files, oracle_files):
    o, offs, want, _, _ = decoded(name, oracle_files)
    g = gpu_files(name)
    if bitmap:
        g.check_full_counts(0, g.uncompressed_size)
    _, cols = g.load_records(split_size, use_success_bitmap=bitmap, columns=("offset",))
    assert cols["offset"].tolist() == offs
    got = g.load_record_fields()
    assert got.n == len(offs) and got.i0 == 0
    assert_fields(got, want, what=name)
    assert got.totals == {"name_bytes": want.name.size, "cigar_ops": want.cigar.size, "seq_bases": want.seq.size,
                          "aux_bytes": want.aux.size}
    assert g.kernel_ms("record_fields") > 0


@gpu
@pytest.mark.parametrize("name", ["2", "5k"])
def test_cli_view_equals_the_reference_sam(name, tmp_path):
    from sbam import cli
    hdr, want = golden_sam(name)
    out = tmp_path / "view.sam"
    assert cli.main(["view", os.path.join(FIXTURES, name + ".bam"), str(out)]) == 0
    assert out.read_text(encoding="latin-1").split("\n") == want + [""]
    assert cli.main(["view", "-h", "-m", "100k", os.path.join(FIXTURES, name + ".bam"), str(out)]) == 0
    assert out.read_text(encoding="latin-1").split("\n") == hdr + want + [""]


# ---- hand-built records -------------------------------------------------------------------------------------------
def record(name: bytes, ops, packed: bytes, qual: bytes, l_seq: int, aux: bytes = b"", nul: bool = True) -> bytes:
    """One BAM record (SAM spec §4.2); `name` without its NUL, `packed` the nibble-packed bases."""
    name = name + b"\x00" if nul else name
    body = struct.pack("<iiBBHHHiiii", 0, 100, len(name), 30, 4680, len(ops), 0, l_seq, -1, -1, 0) + name
    body += b"".join(struct.pack("<I", op) for op in ops) + packed + qual + aux
    return struct.pack("<i", len(body)) + body


def _rand_record(rng, name: bytes, l_seq: int, aux: bytes = b"", ops=None) -> bytes:
    packed = rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
    qual = rng.integers(0, 64, l_seq, dtype=np.uint8).tobytes()
    return record(name, [(max(l_seq, 1) << 4) | 0] if ops is None else ops, packed, qual, l_seq, aux)


@pytest.fixture(scope="module")
def handmade_bam(oracle_files):
    """2.bam's stream with hand-built records inserted after its record 800 and appended at its end:

    * l_seq 0, 1, 2, 7, 8, 9, 15, 16, 17 (around the 8 bases a lane writes), once with and once without tags;
    * a sequence with all 16 nibble codes (also starting at an odd output base); a quality run of 0xFF;
    * n_cigar = 0; l_read_name = 1 (an empty name); l_read_name = 255; records with no aux bytes;
    * one 400 000-base record (larger than any tile, spanning seven BGZF blocks) between 1-base records whose name
      lengths put the four before it and the four after it at all four offsets mod 4;
    * names of 1..8 bytes in a row, so record offsets cover every residue mod 4 (and mod 8);
    * the last record of the file is hand-built."""
    o, offs, _, _, _ = decoded("2.bam", oracle_files)
    u = o.u[:o.L].tobytes()
    at = offs[800]
    rng = np.random.default_rng(20260701)
    recs = []
    for tags in (b"", b"NMC\x07XZZtag\0"):
        for ls in (0, 1, 2, 7, 8, 9, 15, 16, 17):
            recs.append(_rand_record(rng, b"l%d" % ls, ls, tags))
    codes = bytes((2 * k) << 4 | (2 * k + 1) for k in range(8))
    recs.append(record(b"odd", [(1 << 4) | 0], b"\x10", b"\x05", 1))  # the next sequence starts at an odd base
    recs.append(record(b"all16", [(16 << 4) | 0], codes, bytes(range(16)), 16))
    recs.append(record(b"all16_rev", [(17 << 4) | 0], codes[::-1] + b"\xf0", bytes(range(17)), 17))
    recs.append(record(b"noqual", [(13 << 4) | 0], bytes(rng.integers(0, 256, 7, dtype=np.uint8)), b"\xff" * 13, 13))
    recs.append(_rand_record(rng, b"nocigar", 10, ops=[]))
    recs.append(_rand_record(rng, b"", 5))                              # l_read_name = 1
    recs.append(record(b"", [], b"", b"", 0, nul=False))                 # l_read_name = 0: no name bytes at all
    recs.append(_rand_record(rng, b"N" * 254, 33, b"XAAQ"))             # l_read_name = 255
    for k in range(1, 9):
        recs.append(_rand_record(rng, b"abcdefgh"[:k], 1))
    big = record(b"big", [(400000 << 4) | 0], rng.integers(0, 256, 200000, dtype=np.uint8).tobytes(),
                 rng.integers(0, 64, 400000, dtype=np.uint8).tobytes(), 400000, b"XBBc" + struct.pack("<i3b", 3, 1, 2, 3))
    # a 1-base record with a k-byte name takes 43 + k bytes: names of 2 and 6 bytes step the offset by 1 mod 4
    for k in (2, 6, 2, 6):
        recs.append(_rand_record(rng, b"uvwxyz"[:k], 1))
    recs.append(big)
    for k in (2, 6, 2, 6):
        recs.append(_rand_record(rng, b"uvwxyz"[:k], 1))
    last = _rand_record(rng, b"last", 9, b"NMC\x01")
    u2 = u[:at] + b"".join(recs) + u[at:] + last
    arr = np.frombuffer(u2, np.uint8)
    chain = record_chain(arr, int(o.header_end), len(u2))
    assert len(chain) == len(offs) + len(recs) + 1
    starts = np.array(chain[800:800 + len(recs)])
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}
    near_big = starts[-9:]
    assert set((near_big[:4] % 4).tolist()) == {0, 1, 2, 3} and set((near_big[5:] % 4).tolist()) == {0, 1, 2, 3}
    return bgzf(u2), arr, chain, ref_fields(arr, chain)


@gpu
class TestHandBuilt:
    @pytest.fixture(scope="class")
    def g(self, handmade_bam):
        import sbam
        blob, u, chain, want = handmade_bam
        f = sbam.BamFile(blob, path="handmade.bam")
        assert f.uncompressed_size == u.size
        _, cols = f.load_records(1 << 40, columns=("offset",))
        assert cols["offset"].tolist() == chain
        yield f
        f.close()

    def test_all_columns(self, g, handmade_bam):
        blob, u, chain, want = handmade_bam
        assert_fields(g.load_record_fields(), want, what="handmade")

    def test_the_hand_built_run_alone(self, g, handmade_bam):
        """The batch of just the inserted records (its tiles start inside the 400 000-base record's neighbours), and
        the last record of the file."""
        blob, u, chain, want = handmade_bam
        n_ins = len(chain) - 2500 - 1
        assert_fields(g.load_record_fields(800, n_ins), slice_fields(want, 800, n_ins), what="inserted")
        assert_fields(g.load_record_fields(len(chain) - 1, 1), slice_fields(want, len(chain) - 1, 1), what="last")

    def test_the_big_record_spans_seven_blocks(self, handmade_bam):
        blob, u, chain, want = handmade_bam
        sizes = np.diff(np.array(chain + [u.size]))
        k = int(np.argmax(sizes))
        assert sizes[k] > 7 * 65280 and int(want.seq_off[k + 1] - want.seq_off[k]) == 400000
        assert int(want.seq_off[k] - want.seq_off[k - 1]) == 1 == int(want.seq_off[k + 2] - want.seq_off[k + 1])


# ---- batches, masks, arena reuse -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g2(gpu_files, oracle_files):
    o, offs, want, _, _ = decoded("2.bam", oracle_files)
    g = gpu_files("2.bam")
    g.load_records(1 << 40, columns=None)
    return g, want, len(offs)


@gpu
@pytest.mark.parametrize("i0,n", [(0, 0), (7, 0), (0, 1), (1234, 1), (2499, 1), (311, 977), (1900, 600)])
def test_batches(i0, n, g2):
    g, want, N = g2
    got = g.load_record_fields(i0, n)
    assert (got.i0, got.n) == (i0, n)
    assert_fields(got, slice_fields(want, i0, n), what=f"[{i0}, {i0 + n})")
    if n == 0:
        assert set(got.totals.values()) == {0}


@gpu
def test_consecutive_batches_make_the_whole_and_repeat_exactly(g2):
    g, want, N = g2
    a, b = g.load_record_fields(0, 1111), g.load_record_fields(1111, None)
    assert b.n == N - 1111
    for k in DATA_COLUMNS:
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)]), getattr(want, k)), k
    for k in OFFSET_COLUMNS:
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)[1:] + getattr(a, k)[-1]]), getattr(want, k)), k
    # the same batch again, after a larger one used the arena: the same bytes
    g.load_record_fields(0, N)
    again = g.load_record_fields(1111, None)
    for k in DATA_COLUMNS + OFFSET_COLUMNS:
        assert np.array_equal(getattr(again, k), getattr(b, k)), k


@gpu
@pytest.mark.parametrize("fields", [("seq",), ("qual",), ("name", "aux")])
def test_masks(fields, g2):
    import sbam
    g, want, N = g2
    got = g.load_record_fields(5, 2001, fields=fields)
    assert_fields(got, slice_fields(want, 5, 2001), fields=fields, what="+".join(fields))
    dev, i0, n = sbam._RecordFields(), ctypes.c_int64(), ctypes.c_int64()
    assert g.L.sbam_record_fields_device(g.ctx, ctypes.byref(dev), ctypes.byref(i0), ctypes.byref(n)) == sbam.SBAM_OK
    assert (i0.value, n.value) == (5, 2001)
    for k in DATA_COLUMNS:
        assert bool(getattr(dev, k)) == (k in fields), k
    for k in OFFSET_COLUMNS:
        assert getattr(dev, k), k
    # a data column that was not selected cannot be copied out
    other = next(k for k in DATA_COLUMNS if k not in fields)
    buf = np.zeros(1 << 20, np.uint8)
    assert g.L.sbam_get_record_fields(g.ctx, ctypes.byref(sbam._RecordFields(**{other: buf.ctypes.data}))) == sbam.ERR_ARG
    # host=False leaves everything on the device
    dev_only = g.load_record_fields(5, 2001, fields=fields, host=False)
    assert dev_only.seq_off is None and dev_only.totals == got.totals


# ---- long reads ------------------------------------------------------------------------------------------------------
@gpu
def test_long_reads():
    import oracle
    import sbam
    import synth
    s = synth.SynthBam(tile_mb=4, copies=1, read_len=0, threads=8)
    d = s.bytes()
    o = oracle.BamFile(d, threads=8)
    chain = record_chain(o.u, int(o.header_end), o.L)
    assert len(chain) == s.n_records
    want = ref_fields(o.u[:o.L], chain)
    assert int(np.diff(want.seq_off).max()) > 8192, "no read longer than a tile"
    with sbam.BamFile(d, path="long.bam") as g:
        g.check_full_counts(0, o.L)
        _, cols = g.load_records(256 * 1024, use_success_bitmap=True, columns=("offset",))
        assert cols["offset"].tolist() == chain
        assert_fields(g.load_record_fields(), want, what="long reads")
        half = len(chain) // 2
        assert_fields(g.load_record_fields(half, len(chain) - half), slice_fields(want, half, len(chain) - half),
                      what="long reads, second half")


# ---- errors ------------------------------------------------------------------------------------------------------------
@gpu
def test_state_and_argument_errors():
    import sbam
    tot = sbam._RecordFieldTotals()
    with sbam.BamFile(fixture_bytes("2.bam"), path="2.bam") as g:
        L = g.L
        call = lambda i0, n, mask: L.sbam_load_record_fields(g.ctx, i0, n, mask, ctypes.byref(tot))  # noqa: E731
        assert call(0, 1, 31) == sbam.ERR_STATE
        assert L.sbam_record_fields_device(g.ctx, ctypes.byref(sbam._RecordFields()), None, None) == sbam.ERR_STATE
        g.load_records(1 << 40, columns=None)
        assert call(0, 2500, 31) == sbam.SBAM_OK and tot.seq_bases > 0
        assert call(0, 2501, 31) == sbam.ERR_ARG
        assert call(2500, 1, 31) == sbam.ERR_ARG
        assert call(-1, 1, 31) == sbam.ERR_ARG
        assert call(0, -1, 31) == sbam.ERR_ARG
        assert call(0, 1, 0) == sbam.ERR_ARG
        assert call(0, 1, 32) == sbam.ERR_ARG
        assert call(2500, 0, 4) == sbam.SBAM_OK and tot.seq_bases == 0
        with pytest.raises(ValueError):
            g.load_record_fields(0, 1, fields=("bases",))
        assert call(0, 1, 31) == sbam.SBAM_OK
        g.reset()
        assert call(0, 1, 31) == sbam.ERR_STATE
        g.run()
        g.load_records(1 << 40, columns=None)
        assert call(0, 1, 31) == sbam.SBAM_OK
        g.load(fixture_bytes("1.bam"))
        g.run()
        assert call(0, 1, 31) == sbam.ERR_STATE
        assert L.sbam_get_record_fields(g.ctx, ctypes.byref(sbam._RecordFields())) == sbam.ERR_STATE


@gpu
def test_record_that_overruns_its_block_size(oracle_files):
    """A record mid-chain whose l_seq claims more than block_size holds (the chain follows block_size only, so the
    walk lists it): the sizes step rejects the batch with the record's offset, the gather never sees it, and batches
    that exclude it decode."""
    import sbam
    o, offs, want, _, _ = decoded("2.bam", oracle_files)
    u = bytearray(o.u[:o.L].tobytes())
    bad = 1200
    struct.pack_into("<i", u, offs[bad] + 20, 100000)
    with sbam.BamFile(bgzf(bytes(u)), path="overrun.bam") as g:
        _, cols = g.load_records(1 << 40, columns=("offset",))
        assert cols["offset"].tolist() == offs
        with pytest.raises(sbam.RecordFieldsException):
            g.load_record_fields()
        e = g.L.sbam_last_error(g.ctx).contents
        assert e.code == sbam.ERR_RECORD == 10 and e.position == offs[bad]
        assert g.L.sbam_record_fields_device(g.ctx, ctypes.byref(sbam._RecordFields()), None, None) == sbam.ERR_STATE
        with pytest.raises(sbam.RecordFieldsException):
            g.load_record_fields(bad, 1)
        assert_fields(g.load_record_fields(0, bad), slice_fields(want, 0, bad), what="before the bad record")
        n_after = len(offs) - bad - 1
        assert_fields(g.load_record_fields(bad + 1, n_after), slice_fields(want, bad + 1, n_after), what="after it")
        # a negative l_seq is rejected as well
        struct.pack_into("<i", u, offs[bad] + 20, -1)
        g.load(bgzf(bytes(u)))
        g.run()
        g.load_records(1 << 40, columns=None)
        with pytest.raises(sbam.RecordFieldsException):
            g.load_record_fields(bad - 3, 10)
        assert g.L.sbam_last_error(g.ctx).contents.position == offs[bad]


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_new_struct_layouts_follow_the_header():
    """The ctypes mirrors of sbam_record_fields and sbam_record_field_totals have the header's members in the header's
    order, every member 8 bytes wide (pointers / int64), so offsets are 8 * index and sizes 72 and 32."""
    import sbam
    src = open(os.path.join(ROOT, "include", "sbam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for cname, cls, size in (("sbam_record_fields", sbam._RecordFields, 72),
                             ("sbam_record_field_totals", sbam._RecordFieldTotals, 32)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + cname + r"\s*;", src).group(1)
        members = re.findall(r"(\w+)\s*[;,]", body)
        assert members == [n for n, _ in cls._fields_], cname
        assert ctypes.sizeof(cls) == size == 8 * len(members)
        for i, m in enumerate(members):
            assert getattr(cls, m).offset == 8 * i and getattr(cls, m).size == 8, (cname, m)
    assert re.search(r"#define SBAM_ERR_RECORD 10\b", src) and sbam.ERR_RECORD == 10
    for name, bit in sbam.FIELD_BITS.items():
        assert re.search(rf"#define SBAM_FIELD_{name.upper()} {bit}u\b", src), name
