"""The BGZF block scan (k_scan_slots_wide / k_scan_write / k_chain_verify and the host walk of sbam_scan_blocks), the
block search (k_find_block_starts) and what reads the block table after them (inflate, pos_of, k_record_columns, the
CRC check), on files that htsjdk never writes: blocks under 2 KiB (more than kScanSlots candidates in a scan chunk),
header-shaped byte patterns inside payloads, truncated files, an EOF marker in the middle, damaged headers past
position 0, headers that straddle the scan's 1 MiB chunks, its 8192-byte workgroup step and its 32-byte pieces, XLEN
other than 6, and zero-length blocks that are not the EOF marker.

Every file is built here (tests/bgzf_writer.py) from the inflated stream of the reference's 2.bam, and every expected
value is the CPU oracle's: MetadataStream.scala:23-54 (or_metadata_stream), FindBlockStart.scala:8-36
(or_find_block_start), UncompressedBytes.scala:17-19 (pos_of), full/Checker.scala (check_full_range), CanLoadBam.scala:
281-334 (load_reads_and_positions).  Each construction has a CPU test that asserts the file has the property it was
built for, so that a change of the writer cannot quietly turn a GPU case into a plain-file test."""
import ctypes
import os
import re

import numpy as np
import pytest

from bgzf_writer import (STORED_OVERHEAD, candidates, deflated_block, eof_marker, fake_header, stored_block,
                         stored_file)
from conftest import FIXTURES, ROOT

CHUNK = 1 << 20  # kScanChunk
SLOTS = 512  # kScanSlots
WG_STEP = 256 * 32  # kScanThreads * kScanWide
EDGE_KS = (0, 1, 3, 4, 14, 15, 16, 17, 18, 31, 32, 33)
NCHK = (0, 1, 5, 40)


# ---- the source stream and the oracle's side --------------------------------------------------------------------

@pytest.fixture(scope="module")
def base():
    """2.bam's inflated stream and its record offsets (2.bam.records)."""
    import oracle
    o = oracle.BamFile(open(os.path.join(FIXTURES, "2.bam"), "rb").read())
    recs = oracle.parse_records_file(os.path.join(FIXTURES, "2.bam.records"))
    return o.u[:o.L].tobytes(), np.array([o.offset_of(p) for p in recs], np.int64), o


def oracle_table(blob, frm: int = 0):
    """or_metadata_stream from file offset `frm`: (start, csize, usize, uoff[:-1]); HeaderParseException as
    ValueError."""
    import oracle
    d = np.frombuffer(bytes(blob), np.uint8)
    cap = d.size // 26 + 2
    st, cs, us, hs = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ep, ei, ea, ee = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    n = oracle.lib().or_metadata_stream(vp(d) if d.size else None, d.size, frm, cap, vp(st), vp(cs), vp(us), vp(hs),
                                        vp(ep), vp(ei), vp(ea), vp(ee))
    if n < 0:
        raise ValueError(f"Position {int(ei[0])}: {int(ea[0])} != {int(ee[0])}")
    uo = np.zeros(n + 1, np.int64)
    uo[1:] = np.cumsum(np.maximum(us[:n], 0).astype(np.int64))
    return st[:n], cs[:n], us[:n], uo[:-1]


def table_of(o):
    return o.start, o.csize, o.usize, o.uoff[:-1]


def assert_table(got, want):
    for name, x, y in zip(("start", "csize", "usize", "uoff"), got, want):
        assert x.size == y.size, f"{name}: {x.size} blocks, the oracle has {y.size}"
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, f"{name}: {bad.size} rows differ, first {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}"


def assert_stream(g, o):
    assert g.uncompressed_size == o.L
    got = np.frombuffer(g.read_uncompressed(0, o.L), np.uint8)
    bad = np.flatnonzero(got != o.u[:o.L])
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:5]}"


def assert_starts(g, o, qs, nchk: int = 5):
    qs = np.unique(np.clip(np.asarray(qs, np.int64), 0, o.D))
    want = np.array([o.find_block_start(int(q), nchk) for q in qs], np.int64)
    got = g.find_block_starts(qs, nchk)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"blocks_to_check {nchk}: {bad.size} answers differ, first queries {qs[bad[:5]]}: "
                           f"{got[bad[:5]]} vs {want[bad[:5]]}")


def windows(centres, r):
    return np.concatenate([np.arange(c - r, c + r + 1) for c in centres])


def chunk_counts(blob):
    return np.bincount(candidates(blob) >> 20, minlength=(len(blob) + CHUNK - 1) // CHUNK)


# ---- constants the constructions are sized by -------------------------------------------------------------------

def test_scan_constants_are_what_the_files_are_built_for():
    """The files below are sized by kScanSlots, kScanChunk and kScanWide; if one moves, rebuild SMALL (blocks of
    kScanChunk / kScanSlots bytes and one byte less) and the edge files (kScanChunk, 256 * kScanWide) to match."""
    src = os.path.join(ROOT, "spark-bam_amd", "csrc")
    internal = open(os.path.join(src, "sbam_internal.h")).read()
    bgzf = open(os.path.join(src, "sbam_bgzf.hip")).read()
    assert re.search(r"constexpr int kScanSlots = 512;", internal), "kScanSlots moved (sbam_internal.h): resize SMALL"
    assert re.search(r"constexpr int kScanChunk = 1 << 20;", internal), "kScanChunk moved (sbam_internal.h)"
    assert re.search(r"constexpr int kScanWide = 32;", bgzf), "kScanWide moved (sbam_bgzf.hip): resize WG_STEP"
    assert re.search(r"constexpr int kScanThreads = 256;", bgzf), "kScanThreads moved (sbam_bgzf.hip): resize WG_STEP"
    assert CHUNK // SLOTS == 2048


# ---- a. small blocks --------------------------------------------------------------------------------------------

def build_small(u, kind):
    if kind == "mixed300":  # 300-byte stored members alternating with deflated ones of the same payload
        n = 300 - STORED_OVERHEAD
        parts = [stored_block(u[x:x + n]) if (x // n) % 2 == 0 else deflated_block(u[x:x + n])
                 for x in range(0, len(u), n)]
        return b"".join(parts) + eof_marker()
    return stored_file(u, int(kind) - STORED_OVERHEAD)


@pytest.fixture(scope="module")
def small(base):
    import oracle
    out = {}
    for kind in ("2047", "2048", "mixed300"):
        blob = build_small(base[0], kind)
        out[kind] = (blob, oracle.BamFile(blob))
    return out


def test_small_blocks_overflow_the_slots_by_one_and_not_at_all(small):
    c47, c48, c300 = (chunk_counts(small[k][0]) for k in ("2047", "2048", "mixed300"))
    assert len(c47) >= 2 and len(c48) >= 2 and len(c300) >= 2  # every file spans two scan chunks
    assert c47.max() == SLOTS + 1 and c47[0] == SLOTS + 1  # 2047-byte blocks: one candidate too many in chunk 0
    assert c48.max() == SLOTS  # 2048-byte blocks: exactly full, no second pass
    assert c300[:-1].min() > 3000  # several thousand per chunk
    for k in ("2047", "2048", "mixed300"):
        blob, o = small[k]
        assert np.array_equal(candidates(blob)[:o.nblocks], o.start)  # (no fakes here: candidates = blocks + marker)
        assert len(blob) < 3 << 20


def small_queries(o):
    rng = np.random.default_rng(11)
    k0, k1 = o.nblocks // 3, int(np.searchsorted(o.start, CHUNK))  # a block of chunk 0, the first of chunk 1
    near = windows([int(o.start[k0]), int(o.start[k1])], 40)
    more = rng.integers(0, o.D + 1, 320 - near.size)
    return np.concatenate([near, more, [0, o.D - 17, o.D]])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["2047", "2048", "mixed300"])
def test_small_blocks(small, kind):
    import sbam
    blob, o = small[kind]
    with sbam.BamFile(blob, path=kind) as g:
        assert_table(g.blocks(), table_of(o))
        assert_stream(g, o)
        qs = small_queries(o)
        assert np.unique(qs).size >= 300
        assert_starts(g, o, qs)


# ---- b. fake headers --------------------------------------------------------------------------------------------

FAKE_PAYLOAD = 20000
FAKE_BLOCK = FAKE_PAYLOAD + STORED_OVERHEAD


def build_fakes(u):
    """Stored members of 20000 payload bytes; 18 payload bytes overwritten by a header pattern at six places (all
    past the BAM header).  Returns the file and {kind: file position of the fake}."""
    nb = (len(u) + FAKE_PAYLOAD - 1) // FAKE_PAYLOAD
    D = (nb - 1) * FAKE_BLOCK + STORED_OVERHEAD + (len(u) - (nb - 1) * FAKE_PAYLOAD) + len(eof_marker())
    pos = lambda k, j: k * FAKE_BLOCK + 23 + j
    plan = {  # kind: (block, payload offset, BSIZE - 1, XLEN)
        "garbage": (10, 5000, 999, 6),  # the chain lands inside the payload
        "next_real": (20, 7000, FAKE_BLOCK - 23 - 7000 - 1, 6),  # the chain lands on block 21's header
        "past_eof": (nb - 1, 1000, 65535, 6),  # in the last data block: ISIZE past EOF
        "empty": (30, 9000, 27, 6),  # a 2-byte payload: looks like the empty block
        "empty_xlen8": (35, 9000, 29, 8),  # the same through hsize = 20
        "straddle": (40, FAKE_PAYLOAD - 18, 35, 6),  # last 18 payload bytes: its footer is block 41's header bytes
    }
    v = bytearray(u)
    where = {}
    for kind, (k, j, bm1, xlen) in plan.items():
        v[k * FAKE_PAYLOAD + j:k * FAKE_PAYLOAD + j + 18] = fake_header(bm1, xlen)
        where[kind] = pos(k, j)
    blob = stored_file(bytes(v), FAKE_PAYLOAD)
    assert len(blob) == D and where["past_eof"] + 65536 > D
    return blob, where


@pytest.fixture(scope="module")
def fakes(base):
    import oracle
    blob, where = build_fakes(base[0])
    return blob, oracle.BamFile(blob), where


def fake_queries(o, where):
    return np.concatenate([windows(list(where.values()), 64), windows(o.start.tolist() + [o.end_block_pos()], 64),
                           np.arange(o.D - 80, o.D + 1)])


def test_fakes_are_candidates_and_take_every_answer_category(fakes, base):
    blob, o, where = fakes
    c = candidates(blob)
    assert set(where.values()) <= set(c.tolist()) and c.size == o.nblocks + 1 + len(where)
    assert o.L == len(base[0]) and o.nblocks == (o.L + FAKE_PAYLOAD - 1) // FAKE_PAYLOAD  # the table skips them all
    real = set(o.start.tolist()) | {o.end_block_pos()}
    at = lambda kind, n=5: o.find_block_start(where[kind], n)
    # FindBlockStart with 5 blocks: rejected when the chain lands on garbage ...
    assert at("garbage") in real and at("straddle") in real
    assert at("straddle") == where["straddle"] + 18 + 8  # (the very next header)
    # ... accepted when it lands on a real block, runs past EOF, or reaches a 2-byte payload
    for kind in ("next_real", "past_eof", "empty", "empty_xlen8"):
        assert at(kind) == where[kind], kind
    assert blob[where["straddle"] + 32:where["straddle"] + 36] == blob[o.start[41] + 6:o.start[41] + 10]
    # with one block checked every fake is accepted, with none every position is
    assert all(at(kind, 1) == p for kind, p in where.items())
    assert o.find_block_start(where["garbage"] + 1, 0) == where["garbage"] + 1
    qs = np.unique(np.clip(fake_queries(o, where), 0, o.D))
    ans = np.array([o.find_block_start(int(q)) for q in qs])
    fake_at = set(where.values())
    assert any(a in fake_at for a in ans) and any(a in real for a in ans)
    assert any(a not in fake_at and a not in real for a in ans)  # EOF inside the first header: the query itself
    assert len(blob) < 3 << 20


@pytest.mark.gpu
def test_fake_headers_table_stream_words(fakes):
    import sbam
    blob, o, where = fakes
    with sbam.BamFile(blob, path="fakes") as g:
        assert_table(g.blocks(), table_of(o))
        assert_stream(g, o)
        got = g.check_full_words(0, o.L)
        bad = np.flatnonzero(got != o.check_full_range(0, o.L))
        assert bad.size == 0, f"{bad.size} checker words differ, first at {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("nchk", NCHK)
def test_fake_headers_block_search(fakes, nchk):
    import sbam
    blob, o, where = fakes
    with sbam.BamFile(blob, path="fakes", inflate=False) as g:
        assert_starts(g, o, fake_queries(o, where), nchk)


# ---- c. truncation, d. an EOF marker in the middle, e. parse errors ---------------------------------------------

@pytest.fixture(scope="module")
def ten(base):
    """Ten deflated members (20000 bytes each of 2.bam's stream, BAM header included) and the EOF marker."""
    import oracle
    u = base[0][:200000]
    blob = b"".join(deflated_block(u[x:x + 20000]) for x in range(0, len(u), 20000)) + eof_marker()
    return blob, oracle.BamFile(blob)


def truncations(o):
    k = 5
    return sorted({o.D - cut for cut in range(64)} | {int(o.start[k]) + e for e in (0, 1, 17, 18, 19)})


def test_truncation_sweep_takes_both_block_counts(ten):
    blob, o = ten
    assert o.nblocks == 10 and o.D == int(o.start[-1] + o.csize[-1]) + 28
    n = {D: oracle_table(blob[:D])[0].size for D in truncations(o)}
    assert {n[o.D - cut] for cut in range(64)} == {10, 9}
    assert n[o.D] == n[o.D - 1] == n[o.D - 28] == 10 and n[o.D - 29] == 9  # marker whole, cut, gone; last block cut
    s5 = int(o.start[5])
    # blocks 0-4 whichever way block 5 ends the stream: EOF inside its header (17 bytes or fewer) or its ISIZE past EOF
    assert [n[s5 + e] for e in (0, 1, 17, 18, 19)] == [5] * 5
    assert oracle_table(blob[:17])[0].size == 0 and oracle_table(eof_marker())[0].size == 0


@pytest.mark.gpu
def test_truncated_files(ten):
    """One context, reloaded per cut (sbam_load + scan): about 70 cuts."""
    import oracle
    import sbam
    blob, o = ten
    cuts = truncations(o)
    inflate_at = {o.D - 5, o.D - 40, int(o.start[5]) + 17}
    assert inflate_at <= set(cuts)
    with sbam.BamFile(blob, path="ten", inflate=False) as g:
        assert_table(g.blocks(), table_of(o))
        for D in cuts:
            g.load(np.frombuffer(blob[:D], np.uint8))
            g.n_blocks = g._scan()
            want = oracle_table(blob[:D])
            assert g.n_blocks == want[0].size, D
            assert_table(g.blocks(), want)
            if D in inflate_at:
                g.inflate()
                assert_stream(g, oracle.BamFile(blob[:D]))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["17 bytes", "1 byte", "marker only"])
def test_no_blocks(what):
    import sbam
    blob = {"17 bytes": stored_block(b"abc")[:17], "1 byte": b"\x1f", "marker only": eof_marker()}[what]
    assert oracle_table(blob)[0].size == 0
    with sbam.BamFile(blob, inflate=False) as g:
        assert g.n_blocks == 0 and g.blocks()[0].size == 0


def test_marker_in_the_middle_stops_the_oracle(ten):
    blob, o = ten
    assert oracle_table(blob + blob)[0].size == o.nblocks and candidates(blob + blob).size == 2 * o.nblocks + 2


@pytest.mark.gpu
def test_marker_in_the_middle(ten):
    """cat a.bam b.bam: MetadataStream stops at a's EOF marker."""
    import oracle
    import sbam
    blob, o = ten
    two = blob + blob
    o2 = oracle.BamFile(two)
    with sbam.BamFile(two, path="two") as g:
        assert g.n_blocks == o.nblocks
        assert_table(g.blocks(), table_of(o2))
        assert_stream(g, o2)
        assert_starts(g, o2, windows([o.D - 28, o.D, o.D + int(o.start[1])], 40))


HEADER_BYTES = ((0, 0x1f), (1, 0x8b), (2, 0x08), (3, 0x04), (12, 0x42), (13, 0x43), (14, 0x02))
PARSE_CASES = [(i, v) for v in (0x00, 0x7f, 0xe5) for i, exp in HEADER_BYTES if v != exp]


def damaged(blob, o, i, v):
    b = bytearray(blob)
    b[int(o.start[3]) + i] = v
    return bytes(b)


def test_parse_errors_are_signed_bytes_per_the_oracle(ten):
    blob, o = ten
    assert len(PARSE_CASES) == 21
    msgs = []
    for i, v in PARSE_CASES:
        with pytest.raises(ValueError) as e:
            oracle_table(damaged(blob, o, i, v))
        msgs.append(str(e.value))
    assert msgs[PARSE_CASES.index((1, 0xe5))] == "Position 1: -27 != -117"
    assert msgs[PARSE_CASES.index((14, 0x7f))] == "Position 14: 127 != 2"
    assert len(set(msgs)) == 21


@pytest.mark.gpu
@pytest.mark.parametrize("i,v", PARSE_CASES)
def test_parse_error_in_the_fourth_block(ten, i, v):
    import sbam
    blob, o = ten
    bad = damaged(blob, o, i, v)
    with pytest.raises(ValueError) as want:
        oracle_table(bad)
    with pytest.raises(sbam.HeaderParseException) as got:
        sbam.BamFile(bad, path="damaged")
    assert str(got.value) == str(want.value)


# ---- f. chunk, workgroup-step and piece edges -------------------------------------------------------------------

def build_chunk_edge(u, k):
    return stored_file(u[:1_150_000], 60000, starts=[CHUNK - k])


def build_step_edges(u):
    return stored_file(u[:500_000], 6000, starts=[WG_STEP * 4 * (i + 1) - k for i, k in enumerate(EDGE_KS)])


LENGTHS = [(CHUNK + e, marker) for e in (0, 1, 17, 18) for marker in (True, False)]


def build_length(u, total, marker):
    return stored_file(u, 60000, marker=marker, total=total)


def test_edge_files_put_headers_where_they_say(base):
    u = base[0]
    for k in EDGE_KS:
        blob = build_chunk_edge(u, k)
        st = oracle_table(blob)[0]
        assert CHUNK - k in st.tolist() and CHUNK + 100000 < len(blob) < 1_300_000, k
    st = oracle_table(build_step_edges(u))[0].tolist()
    for i, k in enumerate(EDGE_KS):
        assert WG_STEP * 4 * (i + 1) - k in st, k
    for total, marker in LENGTHS:
        blob = build_length(u, total, marker)
        st, cs, us, uo = oracle_table(blob)
        assert len(blob) == total and int(st[-1] + cs[-1]) == total - (28 if marker else 0)
        assert candidates(blob).size == st.size + (1 if marker else 0)


def edge_check(blob, qs):
    import oracle
    import sbam
    o = oracle.BamFile(blob)
    with sbam.BamFile(blob, path="edge") as g:
        assert_table(g.blocks(), table_of(o))
        assert_stream(g, o)
        assert_starts(g, o, qs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_KS)
def test_header_across_the_chunk_edge(base, k):
    edge_check(build_chunk_edge(base[0], k), np.arange(CHUNK - 40, CHUNK + 41))


@pytest.mark.gpu
def test_headers_across_the_workgroup_step(base):
    qs = windows([WG_STEP * 4 * (i + 1) for i in range(len(EDGE_KS))], 40)
    edge_check(build_step_edges(base[0]), qs)


@pytest.mark.gpu
@pytest.mark.parametrize("total,marker", LENGTHS)
def test_file_length_at_the_chunk_edge(base, total, marker):
    edge_check(build_length(base[0], total, marker), np.arange(CHUNK - 40, CHUNK + 41))


# ---- g. XLEN and zero-length blocks -----------------------------------------------------------------------------

def build_xlen(u, rec_off):
    """[XLEN 10][empty][empty][XLEN 12][empty, XLEN 11][empty][deflated, XLEN 10][deflated ...][empty][marker].  The
    first cut is a record start (a record begins on the first byte after two empty blocks); the second is 7 bytes
    into a record, whose fixed fields so straddle a run of two empty blocks."""
    r0 = int(rec_off[np.searchsorted(rec_off, 30000)])
    c1 = int(rec_off[np.searchsorted(rec_off, r0 + 25000)]) + 7
    parts = [stored_block(u[:r0], b"XY\x00\x00"), stored_block(b""), stored_block(b""),
             stored_block(u[r0:c1], b"XY\x02\x00ab"), stored_block(b"", b"ZZ\x01\x00q"), stored_block(b"")]
    for i, x in enumerate(range(c1, len(u), 45000)):  # (45000: the last 20 KB split then starts before the last block)
        parts.append(deflated_block(u[x:x + 45000], extra=b"XY\x00\x00" if i == 0 else b""))
    parts += [stored_block(b""), eof_marker()]
    return b"".join(parts), r0, c1


@pytest.fixture(scope="module")
def xlen(base):
    import oracle
    u, rec_off, o2 = base
    blob, r0, c1 = build_xlen(u, rec_off)
    return blob, oracle.BamFile(blob), r0, c1


XLEN_SPLITS = (20 * 1024, 1 << 20)


def test_xlen_file_keeps_the_stream_and_has_the_empty_blocks(xlen, base):
    import oracle
    blob, o, r0, c1 = xlen
    u, rec_off, o2 = base
    assert o.u[:o.L].tobytes() == u
    assert np.array_equal(o.check_full_range(0, o.L), o2.check_full_range(0, o2.L))
    assert o.hsize[:7].tolist() == [22, 18, 18, 24, 23, 18, 22] and set(o.hsize[7:].tolist()) == {18}
    assert o.usize[[1, 2, 4, 5, -1]].tolist() == [0] * 5 and o.csize[1] == 31
    assert r0 in rec_off and o.uoff[1] == o.uoff[2] == o.uoff[3] == r0  # a record starts right after the empty run
    assert o.pos_of(r0) == oracle.Pos(int(o.start[3]), 0)
    assert c1 - 7 in rec_off and o.uoff[4] == o.uoff[5] == o.uoff[6] == c1  # ... and one straddles the next run
    assert o.pos_of(c1) == oracle.Pos(int(o.start[6]), 0)
    assert o.pos_of(o.L) == oracle.Pos(int(o.start[-1]) + 31, 0)
    for S in XLEN_SPLITS:
        parts = oracle.load_reads_and_positions(o, S)
        assert np.array_equal(np.concatenate(parts), rec_off)
        assert S > o.D or sum(1 for p in parts if len(p)) > 3


@pytest.mark.gpu
class TestXlenAndEmptyBlocks:
    @pytest.fixture(scope="class")
    def g(self, xlen):
        import sbam
        f = sbam.BamFile(xlen[0], path="xlen.bam")
        yield f
        f.close()

    def test_table_and_stream(self, g, xlen):
        blob, o, r0, c1 = xlen
        assert_table(g.blocks(), table_of(o))
        assert_stream(g, o)  # (payloads read from start + hsize: 22, 24 and 23 here)
        assert g.inflate_fallbacks() >= 0
        assert_starts(g, o, windows(o.start[:8].tolist() + [o.end_block_pos()], 40))

    def test_checkers(self, g, xlen):
        blob, o, r0, c1 = xlen
        want = o.check_full_range(0, o.L)
        got = g.check_full_words(0, o.L)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} checker words differ, first at {bad[:5]}"
        assert np.array_equal(g.check_eager(0, o.L), (want & 0x80000000) != 0)

    def test_pos_of_around_every_block_edge(self, g, xlen):
        import sbam
        blob, o, r0, c1 = xlen
        xs = np.unique(np.clip(windows(o.uoff.tolist(), 3), 0, o.L))
        for x in xs.tolist():
            want = o.pos_of(x)
            got = g.pos_of(x)
            assert (got.block_pos, got.offset) == (want.block_pos, want.offset), x
            if x < o.L:
                assert g.offset_of(sbam.Pos(want.block_pos, want.offset)) == o.offset_of(want) == x

    @pytest.mark.parametrize("S", XLEN_SPLITS)
    @pytest.mark.parametrize("bitmap", [False, True])
    def test_load_records(self, g, xlen, S, bitmap):
        from test_records import check_columns, expect
        blob, o, r0, c1 = xlen
        sizes, offs = expect(o, S)
        if bitmap:
            g.check_full_counts(0, g.uncompressed_size)
        got_sizes, cols = g.load_records(S, use_success_bitmap=bitmap)
        assert got_sizes.tolist() == sizes
        check_columns(o, offs, cols)

    def test_crcs(self, g, xlen):
        r = g.check_crc()
        assert r["n_bad"] == 0 and r["n_blocks"] == xlen[1].nblocks


# ---- h. shards --------------------------------------------------------------------------------------------------

def shard_starts(which, o, where):
    st = o.start
    if which == "2047":  # one byte past a real start (twice), a start itself, payload bytes, around the chunk edge
        return [int(st[3]) + 1, int(st[600]) + 1, int(st[100]), int(st[250]) + 1000, CHUNK - 1, CHUNK + 7]
    return [int(st[5]) + 1, int(st[41]) + 1, where["garbage"] + 5, where["straddle"] + 9,  # inside a fake header
            where["garbage"] - 10, where["next_real"] - 100]  # before a rejected fake, before an accepted one


def test_shard_starts_find_real_blocks_and_accepted_fakes(small, fakes):
    blob, o, where = fakes
    ans = [o.find_block_start(lo) for lo in shard_starts("fakes", o, where)]
    assert ans[:4] == [int(o.start[6]), int(o.start[42]), int(o.start[11]), int(o.start[41])]
    assert ans[4:] == [int(o.start[11]), where["next_real"]]
    assert oracle_table(blob, ans[5])[0].size == 1 + o.nblocks - 21  # the shard's table: the fake, then blocks 21 ...
    assert o.find_block_start(where["empty"] - 1) == where["empty"]
    assert oracle_table(blob, where["empty"])[0].size == 0  # a table that the fake "empty block" ends at once
    o47 = small["2047"][1]
    assert all(o47.find_block_start(lo) in o47.start.tolist() for lo in shard_starts("2047", o47, None))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["2047", "fakes"])
@pytest.mark.parametrize("n", range(6))
def test_shard_tables(small, fakes, which, n):
    import sbam
    blob, o = small["2047"] if which == "2047" else fakes[:2]
    lo = shard_starts(which, o, fakes[2])[n]
    first = o.find_block_start(lo)
    want = oracle_table(blob, first)
    with sbam.BamFile(blob[lo:], base_offset=lo, file_size=len(blob), inflate=False, path=which) as g:
        st, cs, us, uo = g.blocks()
        if want[0].size:
            assert int(st[0]) == first
        assert_table((st, cs, us, uo), want)


@pytest.mark.gpu
def test_shard_that_starts_at_a_fake_empty_block(fakes):
    """FindBlockStart accepts the fake with the 2-byte payload, and MetadataStream from it ends at once: no blocks."""
    import sbam
    blob, o, where = fakes
    lo = where["empty"] - 1
    with sbam.BamFile(blob[lo:], base_offset=lo, file_size=len(blob), inflate=False) as g:
        assert g.n_blocks == 0
        assert g.find_block_start(lo) == where["empty"]
