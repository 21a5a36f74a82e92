"""The BAI writer: sbam_build_index on the GPU, sbam_bai_assemble on the host.

The expected index is this file's own CPU restatement of the rules in include/sbam.h (SAM spec §5.2, §5.3 and the usual
samtools/htslib writer): a zlib-and-struct walk of the BAM, then the bin compression, coalescing and serialisation
order in plain Python.  Test 1 pins the restatement to the reference's own 2.bam.bai and 5k.bam.bai (every bin's chunk
list, every linear index, the metadata pseudo-bins, a trailing n_no_coor of 0); every other test compares the library
with the restatement.  The fixtures list their bins in the writing tool's hash-table order, so equality is on the
parsed structure, never on the bytes."""
import struct
import zlib

import numpy as np
import pytest

from conftest import fixture_bytes

NONE = 0xFFFFFFFFFFFFFFFF
META = 37450
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- the restatement ---------------------------------------------------------------------------------------------
class Walk:
    """The BGZF blocks up to the first empty one (MetadataStream's table), the stream, and the Pos rule: the last block
    whose uoff <= x, advanced past exhausted blocks; the stream's end is the address behind the last block."""

    def __init__(self, data: bytes):
        self.start, self.uoff, parts, pos, x = [], [], [], 0, 0
        while pos + 18 <= len(data):
            xlen, = struct.unpack_from("<H", data, pos + 10)
            n = struct.unpack_from("<H", data, pos + 16)[0] + 1
            raw = zlib.decompressobj(-15).decompress(data[pos + 12 + xlen:pos + n - 8])
            if not raw:
                break
            self.start.append(pos)
            self.uoff.append(x)
            parts.append(raw)
            pos += n
            x += len(raw)
        self.end_addr = pos
        self.u = b"".join(parts)
        self.uoff.append(x)

    def vpos(self, x: int) -> int:
        b = int(np.searchsorted(self.uoff, x, side="right")) - 1
        if b >= len(self.start):
            return self.end_addr << 16
        return (self.start[b] << 16) | (x - self.uoff[b])


def reg2bin(beg: int, end: int) -> int:
    e = end - 1
    for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == e >> sh:
            return base + (beg >> sh)
    return 0


def restate(data: bytes) -> dict:
    """Runs, linear index (None = untouched), metadata and counters of the file, by the rules, record by record."""
    w = Walk(data)
    u = w.u
    i32 = lambda x: struct.unpack_from("<i", u, x)[0]  # noqa: E731
    n_ref = i32(8 + i32(4))
    x = 12 + i32(4)
    for _ in range(n_ref):
        x += 8 + i32(x)
    runs, lin, meta = [], {}, {}
    no_coor = unsorted = n = max_nc = 0
    prev_key = prev_run = None
    while x < len(u):
        bs, ref, pos = i32(x), i32(x + 4), i32(x + 8)
        lrn = u[x + 12]
        fnc = struct.unpack_from("<I", u, x + 16)[0]
        nc, flag = fnc & 0xffff, fnc >> 16
        max_nc = max(max_nc, nc)
        key = (ref & 0xffffffff, pos)
        if prev_key is not None and key < prev_key:
            unsorted += 1
        prev_key = key
        n += 1
        if ref < 0:
            no_coor += 1
            prev_run = None
            x += 4 + bs
            continue
        beg = max(pos, 0)
        ops = struct.unpack_from(f"<{nc}I", u, x + 36 + lrn)
        rlen = sum(op >> 4 for op in ops if (op & 15) in (0, 2, 3, 7, 8))
        end = pos + rlen if not flag & 4 and rlen > 0 else beg + 1
        b = reg2bin(beg, end)
        vbeg, vend = w.vpos(x), w.vpos(x + 4 + bs)
        if prev_run == (ref, b):
            runs[-1][3] = vend
        else:
            runs.append([ref, b, vbeg, vend])
        prev_run = (ref, b)
        li = lin.setdefault(ref, [])
        for win in range(beg >> 14, ((end - 1) >> 14) + 1):
            li.extend([None] * (win + 1 - len(li)))
            li[win] = vbeg if li[win] is None else min(li[win], vbeg)
        m = meta.setdefault(ref, [vbeg, vend, 0, 0])
        m[0], m[1] = min(m[0], vbeg), max(m[1], vend)
        m[3 if flag & 4 else 2] += 1
        x += 4 + bs
    return {"n_ref": n_ref, "runs": runs, "lin": lin, "meta": meta, "n_no_coor": no_coor, "n_unsorted": unsorted,
            "n_records": n, "max_nc": max_nc}


def filled(li):
    out, nxt = list(li), None
    for k in range(len(out) - 1, -1, -1):
        nxt = out[k] if out[k] is not None else nxt
        out[k] = nxt
    return out


def assemble(runs, ref: int) -> dict:
    """{bin: chunk list} of one reference from the raw runs: the host assembly of include/sbam.h, in its order."""
    bins = {}
    for r, b, beg, end in runs:
        if r == ref:
            bins.setdefault(b, []).append((beg, end))
    for lvl in range(5, 0, -1):
        lo, hi = ((1 << 3 * lvl) - 1) // 7, ((1 << 3 * lvl + 3) - 1) // 7
        for b in sorted(k for k in bins if lo <= k < hi):
            if lvl < 5:
                bins[b].sort()
            parent = (b - 1) >> 3
            if (bins[b][-1][1] >> 16) - (bins[b][0][0] >> 16) < 0x10000 and parent in bins:
                bins[parent] += bins.pop(b)
    if 0 in bins:
        bins[0].sort()
    for b, cs in bins.items():
        kept = [cs[0]]
        for c in cs[1:]:
            if kept[-1][1] >> 16 >= c[0] >> 16:
                kept[-1] = (kept[-1][0], max(kept[-1][1], c[1]))
            else:
                kept.append(c)
        bins[b] = kept
    return bins


def expected_refs(idx: dict):
    """Per reference ({bin: chunks} with the pseudo-bin, ioffsets): what parse_bai gives for the index's bytes."""
    out = []
    for r in range(idx["n_ref"]):
        if r not in idx["meta"]:
            out.append(({}, []))
            continue
        bins = assemble(idx["runs"], r)
        m = idx["meta"][r]
        bins[META] = [(m[0], m[1]), (m[2], m[3])]
        out.append((bins, filled(idx["lin"].get(r, []))))
    return out


def parsed(bai_bytes: bytes):
    from sbam import bai
    return [({b: [(c.start, c.end) for c in cs] for b, cs in r.bins.items()}, list(r.ioffsets))
            for r in bai.parse_bai(bai_bytes)]


def bin_order(bai_bytes: bytes):
    """Bin numbers of every reference in the order the bytes list them."""
    p, out = 8, []
    for _ in range(struct.unpack_from("<i", bai_bytes, 4)[0]):
        n_bin, = struct.unpack_from("<i", bai_bytes, p)
        p += 4
        order = []
        for _ in range(n_bin):
            b, nch = struct.unpack_from("<Ii", bai_bytes, p)
            order.append(b)
            p += 8 + 16 * nch
        p += 4 + 8 * struct.unpack_from("<i", bai_bytes, p)[0]
        out.append(order)
    assert p + 8 == len(bai_bytes), "bytes behind the trailing n_no_coor"
    return out


def assemble_args(idx: dict):
    """The arguments of sbam.bai_assemble from a restated index (untouched windows as UINT64_MAX)."""
    nr = idx["n_ref"]
    runs = idx["runs"]
    cols = ([r[0] for r in runs], [r[1] for r in runs], [r[2] for r in runs], [r[3] for r in runs])
    intv_off, io = [0], []
    ob, oe, nm, nu = [NONE] * nr, [0] * nr, [0] * nr, [0] * nr
    for r in range(nr):
        io += [NONE if v is None else v for v in idx["lin"].get(r, [])]
        intv_off.append(len(io))
        if r in idx["meta"]:
            ob[r], oe[r], nm[r], nu[r] = idx["meta"][r]
    return (nr, tuple(np.array(c, t) for c, t in zip(cols, (np.int32, np.uint32, np.uint64, np.uint64))),
            intv_off, np.array(io, np.uint64), np.array(ob, np.uint64), np.array(oe, np.uint64), nm, nu, idx["n_no_coor"])


@pytest.fixture(scope="module")
def restated():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = restate(fixture_bytes(name))
        return cache[name]
    return get


FIXTURE_FACTS = {  # bins on reference 0 (without the pseudo-bin), windows, (off_beg, off_end), mapped, unmapped
    "2.bam": (4, 5, (0x1612, 0x81d0d0000), 2450, 50),
    "5k.bam": (5, 5, (0x9960000, 0xf6bf30000), 4787, 123),
}


# ---- 1. the restatement is the reference's index -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_restatement_equals_reference_index(name, restated):
    from sbam import bai
    want_bytes = fixture_bytes(name + ".bai")
    want = parsed(want_bytes)
    idx = restated(name)
    got = expected_refs(idx)
    assert len(got) == len(want) == idx["n_ref"]
    for r, ((gb, gi), (wb, wi)) in enumerate(zip(got, want)):
        assert gb == wb, f"bins of reference {r}"
        assert gi == wi, f"linear index of reference {r}"
    assert bai.parse_n_no_coor(want_bytes) == 0 == idx["n_no_coor"] and idx["n_unsorted"] == 0
    nb, nw, span, nm, nu = FIXTURE_FACTS[name]
    assert len(got[0][0]) == nb + 1 and len(got[0][1]) == nw
    assert got[0][0][META] == [span, (nm, nu)]
    assert all(None not in idx["lin"][r] for r in idx["lin"]), "the fixtures have no gap in a linear index"


# ---- 2. the host assembly on the fixtures' runs --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_assemble_fixture_runs(name, restated):
    import sbam
    from sbam import bai
    idx = restated(name)
    out = sbam.bai_assemble(*assemble_args(idx))
    assert parsed(out) == parsed(fixture_bytes(name + ".bai"))
    assert bai.parse_n_no_coor(out) == 0
    for order in bin_order(out):  # (also: the size is exact, nothing follows n_no_coor)
        assert order == sorted(order) and (not order or order[-1] == META)


# ---- 3. the host assembly on fabricated runs -----------------------------------------------------------------------
def _one_ref(runs, lin=None, n_ref=1, meta=None):
    lin = {0: [1 << 16]} if lin is None else lin
    meta = {0: [1 << 16, 2 << 16, len(runs), 0]} if meta is None else meta
    return {"n_ref": n_ref, "runs": [list(r) for r in runs], "lin": lin, "meta": meta, "n_no_coor": 7}


def _assembled(idx):
    import sbam
    from sbam import bai
    out = sbam.bai_assemble(*assemble_args(idx))
    assert parsed(out) == [(b, i) for b, i in expected_refs(idx)]
    assert bai.parse_n_no_coor(out) == idx["n_no_coor"]
    for order in bin_order(out):
        assert order == sorted(order) and (not order or order[-1] == META)
    return parsed(out)


def test_assemble_leaf_span_threshold():
    """A leaf whose chunks span 0xFFFF blocks' worth of compressed bytes joins its parent; one spanning 0x10000 stays."""
    parent = (585, 10 << 16, 11 << 16)
    small = _assembled(_one_ref([(0, 4681, 100 << 16, (100 + 0xFFFF) << 16 | 5), (0,) + parent]))
    assert set(small[0][0]) == {585, META} and len(small[0][0][585]) == 2
    kept = _assembled(_one_ref([(0, 4681, 100 << 16, (100 + 0x10000) << 16), (0,) + parent]))
    assert set(kept[0][0]) == {4681, 585, META}


def test_assemble_small_leaf_without_parent_stays():
    got = _assembled(_one_ref([(0, 4682, 100 << 16, 101 << 16)]))
    assert set(got[0][0]) == {4682, META}


def test_assemble_merge_chain_to_bin_zero():
    """One small bin per level, each the parent of the one below: everything ends in bin 0, sorted and coalesced where
    the blocks touch."""
    chain = [4681 + 8 * 8 * 8 * 8, 585 + 8 * 8 * 8, 73 + 8 * 8, 9 + 8, 2, 0]  # (b - 1) >> 3 walks the list
    assert all((chain[k] - 1) >> 3 == chain[k + 1] for k in range(5))
    runs = [(0, b, (10 * (6 - k)) << 16, (10 * (6 - k) + 3) << 16) for k, b in enumerate(chain)]
    got = _assembled(_one_ref(runs))
    assert set(got[0][0]) == {0, META}
    assert got[0][0][0] == sorted((r[2], r[3]) for r in runs)  # six chunks, seven blocks apart: none coalesces


def test_assemble_coalesce_same_block_only():
    same = _assembled(_one_ref([(0, 4681, 5 << 16, 9 << 16 | 100), (0, 4683, 1, 2), (0, 4681, 9 << 16 | 200, 12 << 16)]))
    assert same[0][0][4681] == [(5 << 16, 12 << 16)]
    apart = _assembled(_one_ref([(0, 4681, 5 << 16, 9 << 16 | 100), (0, 4683, 1, 2), (0, 4681, 10 << 16, 12 << 16)]))
    assert apart[0][0][4681] == [(5 << 16, 9 << 16 | 100), (10 << 16, 12 << 16)]


def test_assemble_linear_gap_filled_backwards():
    got = _assembled(_one_ref([(0, 4681, 1 << 16, 2 << 16)], lin={0: [None, 111, None, None, 222]}))
    assert got[0][1] == [111, 111, 222, 222, 222]


def test_assemble_reference_without_records():
    idx = _one_ref([(1, 4681, 1 << 16, 2 << 16)], lin={1: [1 << 16]}, n_ref=3, meta={1: [1 << 16, 2 << 16, 1, 0]})
    got = _assembled(idx)
    assert got[0] == ({}, []) and got[2] == ({}, []) and set(got[1][0]) == {4681, META}
    import sbam
    out = sbam.bai_assemble(*assemble_args(idx))
    assert struct.unpack_from("<ii", out, 8) == (0, 0), "n_bin and n_intv of the empty first reference"


def test_assemble_capacity_too_small():
    import ctypes
    import sbam
    L = sbam.load_library()
    nr, (ref, bn, beg, end), iv, io, ob, oe, nm, nu, nnc = assemble_args(_one_ref([(0, 4681, 1 << 16, 2 << 16)]))
    iv, nm, nu = (np.array(a, np.int64) for a in (iv, nm, nu))
    args = (nr, ref.size) + tuple(a.ctypes.data for a in (ref, bn, beg, end, iv, io, ob, oe, nm, nu)) + (nnc,)
    n = ctypes.c_int64(0)
    assert L.sbam_bai_assemble(*args, None, 0, ctypes.byref(n)) == sbam.ERR_ARG
    need = n.value  # magic, n_ref | n_bin, bin 4681 with one chunk, the pseudo-bin, n_intv, one window | n_no_coor
    assert need == 8 + (4 + (8 + 16) + (8 + 32) + 4 + 8) + 8
    buf = np.full(need, 0xAB, np.uint8)
    assert L.sbam_bai_assemble(*args, buf.ctypes.data, need - 1, ctypes.byref(n)) == sbam.ERR_ARG
    assert n.value == need and np.all(buf == 0xAB), "a short buffer is not written"
    assert L.sbam_bai_assemble(*args, buf.ctypes.data, need, ctypes.byref(n)) == sbam.SBAM_OK and n.value == need


# ---- GPU -----------------------------------------------------------------------------------------------------------
def check_against(f, idx, bai_bytes=None):
    """The built index of BamFile f (runs, linear index, metadata, counters, bytes) equals the restated one."""
    from sbam import bai
    ref, bn, beg, end = f.index_runs()
    got = [list(t) for t in zip(ref.tolist(), bn.tolist(), beg.tolist(), end.tolist())]
    assert got == idx["runs"]
    r = f.index_refs()
    assert (r.n_no_coor, r.n_unsorted, r.n_records) == (idx["n_no_coor"], idx["n_unsorted"], idx["n_records"])
    assert r.intv_off.size == idx["n_ref"] + 1
    for k in range(idx["n_ref"]):
        assert r.ioffset[r.intv_off[k]:r.intv_off[k + 1]].tolist() == filled(idx["lin"].get(k, [])), f"reference {k}"
        m = idx["meta"].get(k, [NONE, 0, 0, 0])
        assert [int(r.off_beg[k]), int(r.off_end[k]), int(r.n_mapped[k]), int(r.n_unmapped[k])] == m, f"reference {k}"
    if bai_bytes is not None:
        assert parsed(bai_bytes) == [(b, i) for b, i in expected_refs(idx)]
        assert bai.parse_n_no_coor(bai_bytes) == idx["n_no_coor"]
        for order in bin_order(bai_bytes):
            assert order == sorted(order) and (not order or order[-1] == META)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_build_bai_fixtures(name, restated):
    import sbam
    with sbam.BamFile(fixture_bytes(name), path=name) as f:
        out = f.build_bai()
        assert parsed(out) == parsed(fixture_bytes(name + ".bai"))
        check_against(f, restated(name), out)
        assert f.kernel_ms("index") > 0


@pytest.mark.gpu
def test_load_bam_intervals_builds_its_index():
    import sbam
    from test_intervals import CASES, brute_offsets
    u = Walk(fixture_bytes("2.bam")).u
    with sbam.BamFile(fixture_bytes("2.bam"), path="2.bam") as g:
        for loci, chunks, n, split, nparts in CASES:
            kw = {} if split is None else {"split_size": split}
            got_chunks, parts = g.load_bam_intervals(None, loci, **kw)
            assert [c.pos_str() for c in got_chunks] == chunks
            assert len(parts) == nparts and sum(p.size for p in parts) == n
            assert np.concatenate(parts).tolist() == brute_offsets(u, loci), "exactly the records of the loci"


@pytest.mark.gpu
def test_synthetic_short_reads_all_references(tmp_path):
    """The bench generator's short-read file: every one of the 84 references, records without coordinates, placed
    unmapped records, and a few order violations at the tile's seams."""
    import sbam
    import synth
    from sbam import cli
    s = synth.SynthBam(tile_mb=2, copies=1, read_len=150)
    data = s.bytes().tobytes()
    idx = restate(data)
    assert idx["n_records"] == s.n_records and len(idx["meta"]) == idx["n_ref"] == 84
    assert idx["n_no_coor"] > 0 and idx["n_unsorted"] > 0 and sum(m[3] for m in idx["meta"].values()) > 0
    with sbam.BamFile(data, path="synth.bam") as f:
        with pytest.raises(sbam.SbamError, match="unsorted positions"):
            f.build_bai()
        out = f.build_bai(require_sorted=False)
        check_against(f, idx, out)
    bam, dst = tmp_path / "s.bam", tmp_path / "s.bai"
    bam.write_bytes(data)
    assert cli.main(["index-bam", "-o", str(dst), str(bam)]) != 0
    assert not dst.exists() and not (tmp_path / "s.bam.bai").exists()
    assert cli.main(["index-bam", "--allow-unsorted", str(bam)]) == 0
    assert parsed((tmp_path / "s.bam.bai").read_bytes()) == parsed(out)


@pytest.mark.gpu
def test_synthetic_long_reads():
    """200-3000-op CIGARs (the wave-per-record path), records over several 16 kb windows, upper-level bins."""
    import sbam
    import synth
    s = synth.SynthBam(tile_mb=2, copies=1, read_len=0, threads=8)
    data = s.bytes().tobytes()
    idx = restate(data)
    assert idx["max_nc"] > sbam.load_library().sbam_index_long_cigar_ops(), "no record reaches the long-CIGAR path"
    assert any(r[1] < 4681 for r in idx["runs"]), "no record lands in an upper-level bin"
    with sbam.BamFile(data, path="long.bam") as f:
        out = f.build_bai(require_sorted=False)
        check_against(f, idx, out)


# hand-built files
BIG = (1 << 29) + 1000  # the reference's length: positions up to 2^29 pass the checker
OPS = "MIDNSHP=X"


def record(ref, pos, cigar=(), flag=0, name=b"read", l_seq=4, n_cigar=None, pad=0):
    """One BAM record (SAM spec §4.2) with `pad` tag bytes; n_cigar overrides the op count the record claims."""
    ops = b"".join(struct.pack("<I", ln << 4 | OPS.index(op)) for ln, op in cigar)
    nc = len(cigar) if n_cigar is None else n_cigar
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 30, 4680, nc, flag, l_seq, -1, -1, 0)
    body += name + b"\0" + ops + b"\x11" * ((l_seq + 1) // 2) + b"\x20" * l_seq + b"X" * pad
    return struct.pack("<i", len(body)) + body


def header(refs=(("chr1", BIG),)):
    text = b"@HD\tVN:1.5\tSO:coordinate\n"
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        h += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return h


def bgzf(chunks) -> bytes:
    """Each chunk as one BGZF block, then the EOF marker."""
    out = b""
    for c in chunks:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = co.compress(c) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(d) + 25) + d
        out += struct.pack("<II", zlib.crc32(c), len(c))
    return out + EOF_BLOCK


def cut(u: bytes, at) -> list:
    at = [0] + list(at) + [len(u)]
    return [u[a:b] for a, b in zip(at, at[1:])]


MAPPED = [record(0, 100 + 10 * k, [(50, "M")]) for k in range(12)]  # (the checker reads ten records ahead)


def built(data, **kw):
    import sbam
    with sbam.BamFile(data, path="hand.bam") as f:
        out = f.build_bai(**kw)
        idx = restate(data)
        check_against(f, idx, out)
        return idx, out


@pytest.mark.gpu
def test_record_ends_at_block_end_and_spans_three_blocks():
    h = header()
    recs = MAPPED + [record(0, 300, [(50, "M")], pad=700), record(0, 310, [(50, "M")])]
    u = h + b"".join(recs)
    first_end = len(h) + len(recs[0])       # record 0 ends exactly at a block's end
    big = len(u) - len(recs[-1]) - len(recs[-2])  # the padded record: cut twice inside it
    data = bgzf(cut(u, [len(h), first_end, big + 200, big + 500]))
    w = Walk(data)
    assert w.vpos(first_end) == w.start[2] << 16, "the first record's vend: the next block's address, offset 0"
    assert w.vpos(big) >> 16 == w.start[2] and w.vpos(big + len(recs[-2])) >> 16 == w.start[4]
    idx, _ = built(data)
    assert len(idx["runs"]) == 1 and idx["runs"][0][3] == w.end_addr << 16, "the last record ends at the EOF marker"


@pytest.mark.gpu
def test_header_only_file():
    idx, out = built(bgzf([header((("chr1", 1000), ("chr2", 2000)))]))
    assert idx["n_records"] == 0 and parsed(out) == [({}, []), ({}, [])]


@pytest.mark.gpu
def test_unmapped_clipped_and_negative_positions():
    """A placed unmapped record without a CIGAR and a mapped one whose CIGAR has no reference length both end at
    pos + 1; pos = -1 on a reference starts at 0."""
    recs = [record(0, -1, [(50, "M")])] + MAPPED + [
        record(0, 20000, (), flag=4, l_seq=0), record(0, 40000, [(3, "S"), (1, "I")]),
        record(0, 50000, [(40000, "M")])]
    data = bgzf([header(), b"".join(recs)])
    idx, _ = built(data)
    assert idx["meta"][0][2:] == [15, 1] and idx["n_unsorted"] == 0
    assert [r[1] for r in idx["runs"]] == [4681, 4681 + 1, 4681 + 2, reg2bin(50000, 90000)]
    assert len(idx["lin"][0]) == (89999 >> 14) + 1


@pytest.mark.gpu
def test_one_bin_of_every_level_and_the_2_29_limit():
    edges = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]
    recs = MAPPED + [record(0, e - 10, [(20, "M")]) for e in edges] + [record(0, (1 << 29) - 100, [(100, "M")])]
    data = bgzf([header(), b"".join(recs)])
    idx, _ = built(data)
    levels = {next(lv for lv in range(6) if r[1] >= ((1 << 3 * lv) - 1) // 7 and r[1] < ((1 << 3 * lv + 3) - 1) // 7)
              for r in idx["runs"]}
    assert levels == {0, 1, 2, 3, 4, 5}
    assert len(idx["lin"][0]) == 1 << 15, "a record ending at exactly 2^29 is indexed"


def _error(data):
    import ctypes
    import sbam
    with sbam.BamFile(data, path="bad.bam") as f:
        with pytest.raises(sbam.RecordFieldsException):
            f.build_bai()
        e = f.L.sbam_last_error(f.ctx).contents
        assert e.code == sbam.ERR_RECORD
        n = ctypes.c_int64(0)
        assert f.L.sbam_write_bai(f.ctx, None, 0, ctypes.byref(n)) == sbam.ERR_STATE, "nothing is produced"
        return int(e.position)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [
    record(0, (1 << 29) - 99, [(100, "M")]),             # ends at 2^29 + 1
    record(1, 500, [(50, "M")]),                         # ref_id = n_ref
    record(0, 500, [(50, "M")], n_cigar=40, pad=8),      # 40 ops claimed, room for 3
], ids=["end_past_2_29", "ref_id_is_n_ref", "cigar_past_block_size"])
def test_record_errors_name_the_first_offender(bad):
    h = header()
    good = b"".join(MAPPED)
    data = bgzf([h, good + bad + bad + record(0, 600, [(50, "M")])])
    assert _error(data) == len(h) + len(good)


@pytest.mark.gpu
def test_state(restated):
    import ctypes
    import sbam
    data = fixture_bytes("2.bam")
    idx = restated("2.bam")
    t, n = sbam._IndexTotals(), ctypes.c_int64(0)
    with sbam.BamFile(data, path="2.bam") as f:
        L, split = f.L, 100000
        assert L.sbam_build_index(f.ctx, ctypes.byref(t)) == sbam.ERR_STATE, "before any load"
        assert L.sbam_write_bai(f.ctx, None, 0, ctypes.byref(n)) == sbam.ERR_STATE, "before a build"
        f.load_records(split, first=1, columns=None)
        assert L.sbam_build_index(f.ctx, ctypes.byref(t)) == sbam.ERR_STATE, "a load that skips split 0"
        f.load_records(split, columns=None)
        assert L.sbam_build_index(f.ctx, ctypes.byref(t)) == sbam.SBAM_OK
        assert (t.n_ref, t.n_records, t.n_no_coor, t.n_unsorted) == (idx["n_ref"], 2500, 0, 0)
        assert t.n_runs == len(idx["runs"]) and t.n_intv_total == sum(len(v) for v in idx["lin"].values())
        one = f.build_bai(split)
        assert f.build_bai(split) == one, "a second build on the same context"
        assert parsed(one) == parsed(fixture_bytes("2.bam.bai"))
        f.reset()
        assert L.sbam_write_bai(f.ctx, None, 0, ctypes.byref(n)) == sbam.ERR_STATE
        f.run()
        assert L.sbam_build_index(f.ctx, ctypes.byref(t)) == sbam.ERR_STATE, "after a reset a build needs a new load"
        assert f.build_bai(split) == one
