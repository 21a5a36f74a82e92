"""Every checker flag as the sole cause of a rejection, in every record-0 kernel, and the flags only a stream end raises.

The reference's BAM files never reject a position for one reason alone (garbage offsets fail many checks at once), never
fail after a passing record, and never hold a boundary value (refPos == length, refIdx == -2, l_seq == INT_MAX ...), so
the eager pass, the success bitmap and every `>` against `>=` go unpinned by them.  This file
builds those records by hand.

Part 1, `TABLE`: a base record that passes every check (mapped, contig 0, name "read/1", one 20M op, 20 bases) and
variants that each change one field, with the flag set full/Checker.scala and PosChecker.scala give for it written as
a literal.  Ten passing records stand in front of every variant, so that the nine before a failing one fail with its
flag at readsBeforeError 1 ... 9.  One stream (`build`) holds the table
  * four times at its front, each variant's start at offset 0, 63, 33 and 30 mod 64 in turn (all four residues mod 4,
    0 and 31 mod 32, 63 mod 64), in interior tiles: k_check_bits and k_eager_wave;
  * a few variants in the last 1, 35, 36 and 37 bytes of a tile, and the 254-character names and 68-op arrays 250 and
    100 bytes before a tile's end (across it, and past the eager wave's 64-byte halo);
  * once more inside the last kInteriorTail bytes, behind a tile-and-a-tail of passing records: k_check in every mode.
The stream is checked under the header's contig table (1000, 0, 1, 2^31 - 1), under 5000 lengths (n_ref > kLdsLens),
under none (n_ref = 0), and under lengths outside [0, INT32_MAX] (a header with l_ref -1 and -5; 2^31 and 2^32 + 5).

Part 2, `END_CASES`: streams of a few hundred bytes that stop inside a record's fixed fields, name or op array (flags
0, 9 and 14), end their chain exactly on the end (Success with fewer than reads_to_check records), or whose last
block_size points past the end or stops short of the record's own bytes.  The "skip past EOF" rule stays parity
unpinned: these cases pin the kernels against the oracle there, not the oracle against the
reference.

Expected values are the oracle's (check_full_range, counts_range); the CPU tests prove that the oracle agrees with the
literals and that the stream covers what it claims, so the GPU tests cannot pass vacuously."""
import numpy as np
import pytest

from record_stream_writer import Stream, implied_size, record
from test_check_general_kernel import check_counts
from test_eager_wave import bgzf
from test_gpu_parity import pair_hist

K_TILE, K_INTERIOR_TAIL = 8192, 262144 + 512  # sbam_check.hip: kTile, kInteriorTail
SUCC = 0x80000000
IMAX, IMIN = 2**31 - 1, -2**31
LENS = (1000, 0, 1, IMAX)
N_REF = len(LENS)
LENS_5000 = LENS + tuple((i * 7919) % 100003 for i in range(N_REF, 5000))
READS_TO_CHECK = (1, 2, 10)
SOLE_FLAGS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18)

M20 = (20 << 4) | 0
BASE = dict(ref_id=0, pos=100, name=b"read/1", mapq=30, flag=0, cigar=(M20,), seq=b"\x11" * 10, qual=b"\x1e" * 20,
            next_ref_id=0, next_pos=200, tlen=150, aux=b"NMC\x07")
ALLOWED = bytes(range(33, 64)) + bytes(range(65, 127))  # Checker.allowedReadNameChars
NAME254 = (ALLOWED * 3)[:254]
OPS68 = ((1 << 4) | 0,) * 68


def word(flags=(), k=0):
    return sum(1 << f for f in flags) | (k << 24)


def rec(**kw):
    return record(**{**BASE, **kw})


def short(**kw):
    """The base record without aux and one quality byte short: block_size = implied size - 1."""
    return rec(aux=b"", qual=b"\x1e" * 19, l_seq=20, **kw)


def bare(l_seq, delta):
    """Fixed fields, name and op only, l_seq as given, block_size = implied size + delta."""
    return rec(l_seq=l_seq, seq=b"", qual=b"", aux=b"", block_size=implied_size(7, 1, l_seq) + delta)


def with_byte(b, at=2, name=b"read/1"):
    n = bytearray(name)
    n[at] = b
    return bytes(n) + b"\x00"


def bad_op(i, ops=OPS68, code=9):
    o = list(ops)
    o[i] = (1 << 4) | code
    return tuple(o)


def make_table():
    """[(label, record bytes, flags of the literal expectation under the header's contig table)]."""
    t = []

    def V(label, flags, r):
        if label not in {v[0] for v in t}:  # (refPos 0 is also contig 1's length)
            t.append((label, r, frozenset(flags)))

    V("base", (), rec())
    # refID / pos (flags 1-4) and next_refID / next_pos (5-8): PosChecker.scala:43-63
    for idx, pos, d, tag in (("ref_id", "pos", 0, "ref"), ("next_ref_id", "next_pos", 4, "next")):
        for ri, f in ((-2, (1,)), (-1, ()), (0, ()), (N_REF - 1, ()), (N_REF, (2,)), (IMIN, (1,)), (IMAX, (2,))):
            V(f"{tag} idx={ri}", [x + d for x in f], rec(**{idx: ri, pos: 0}))
        for c, n in enumerate(LENS):
            for rp, f in ((-2, (3,)), (-1, ()), (0, ()), (n, ()), (n + 1, (4,))):
                if rp <= IMAX:
                    V(f"{tag} contig={c} pos={rp}", [x + d for x in f], rec(**{idx: c, pos: rp}))
        V(f"{tag} idx=-1 pos=INT_MAX", (), rec(**{idx: -1, pos: IMAX}))
        V(f"{tag} idx=-2 pos=-2", (1 + d, 3 + d), rec(**{idx: -2, pos: -2}))
        V(f"{tag} idx=INT_MIN pos=INT_MIN", (1 + d, 3 + d), rec(**{idx: IMIN, pos: IMIN}))
        V(f"{tag} idx=n_ref pos=-2", (2 + d, 3 + d), rec(**{idx: N_REF, pos: -2}))
        V(f"{tag} idx=INT_MAX pos=INT_MIN", (2 + d, 3 + d), rec(**{idx: IMAX, pos: IMIN}))
        V(f"{tag} idx=n_ref pos=INT_MAX", (2 + d,), rec(**{idx: N_REF, pos: IMAX}))
        # in range only under the 5000-entry table: refPos == length and length + 1 there
        for ri in (4095, 4096, 4999, 5000):
            n = LENS_5000[ri] if ri < 5000 else 5
            V(f"{tag} idx={ri} pos=len", (2 + d,), rec(**{idx: ri, pos: n}))
            V(f"{tag} idx={ri} pos=len+1", (2 + d,), rec(**{idx: ri, pos: n + 1}))
    # read name (flags 10-13): full/Checker.scala:73-109
    V("l_read_name=0", (12,), rec(raw_name=b""))
    V("l_read_name=1", (13,), rec(raw_name=b"\x00"))
    V("l_read_name=2", (), rec(name=b"r"))
    V("l_read_name=255", (), rec(name=NAME254))
    V("name last byte not NUL", (10,), rec(raw_name=b"read/1X"))
    V("name last byte not NUL, bad body byte", (10,), rec(raw_name=b"re\x20d/1X"))
    for b in (32, 33, 63, 64, 65, 126, 127, 128, 255, 0):
        V(f"name byte {b}", () if b in ALLOWED else (11,), rec(raw_name=with_byte(b)))
    for i in (0, 63, 64, 65, 253):
        V(f"name254 bad byte at {i}", (11,), rec(raw_name=with_byte(64 if i & 1 else 32, i, NAME254)))
    # CIGAR (flags 15-17): full/Checker.scala:111-136
    for code, f in ((8, ()), (9, (15,)), (15, (15,))):
        V(f"op code {code}", f, rec(cigar=((20 << 4) | code,)))
    V("ops68", (), rec(cigar=OPS68))
    for i in (0, 63, 64, 65, 67):
        V(f"ops68 bad op at {i}", (15,), rec(cigar=bad_op(i)))
    V("mapped n_cigar_op=0", (17,), rec(cigar=()))
    V("mapped l_seq=0", (16,), rec(l_seq=0))
    V("mapped n_cigar_op=0 l_seq=0", (16, 17), rec(cigar=(), l_seq=0))
    V("unmapped n_cigar_op=0 l_seq=0", (), rec(cigar=(), l_seq=0, flag=4))
    V("bad op, l_seq=0", (15,), rec(cigar=((20 << 4) | 9,), l_seq=0))
    # block_size against the implied size (flag 18): full/Checker.scala:68-71, in Java Int arithmetic
    V("block_size=implied", (), rec(aux=b""))
    V("block_size=implied-1", (18,), short())
    V("l_seq=21 block_size=implied", (), rec(aux=b"", seq=b"\x11" * 11, qual=b"\x1e" * 21))
    V("l_seq=21 block_size=implied-1", (18,), rec(aux=b"", seq=b"\x11" * 11, qual=b"\x1e" * 20, l_seq=21))
    for ls in (-1, -2, -3, IMAX, IMIN):
        V(f"l_seq={ls} block_size=implied", (), bare(ls, 0))
        V(f"l_seq={ls} block_size=implied-1", (18,), bare(ls, -1))
    # two faults of different groups (refID/pos, next, name, CIGAR, size): every pair of groups, the close calls of
    # the full-check report (cli/.../check/full/FullCheck.scala:261-297)
    V("pair ref+next", (1, 7), rec(ref_id=-2, next_pos=-2))
    V("pair ref+name", (4, 13), rec(pos=1001, raw_name=b"\x00"))
    V("pair ref+cigar", (2, 15), rec(ref_id=N_REF, cigar=((20 << 4) | 9,)))
    V("pair ref+size", (3, 18), short(pos=-2))
    V("pair next+name", (6, 11), rec(next_ref_id=N_REF, raw_name=with_byte(127)))
    V("pair next+cigar", (8, 17), rec(next_pos=1001, cigar=()))
    V("pair next+size", (5, 18), short(next_ref_id=-2))
    V("pair name+cigar", (10, 16), rec(raw_name=b"read/1X", l_seq=0))
    V("pair name+size", (12, 18), short(raw_name=b""))
    V("pair cigar+size", (15, 18), short(cigar=((20 << 4) | 9,)))
    return t


TABLE = make_table()
INDEX = {label: i for i, (label, _, _) in enumerate(TABLE)}
COPY_RESIDUES = (0, 63, 33, 30)  # variant starts mod 64, one table copy each
EDGE_SHORT = ("base", "ref contig=0 pos=1001", "next contig=0 pos=1001", "block_size=implied-1")
EDGE_LONG = ("l_read_name=255", "name254 bad byte at 64", "name254 bad byte at 253", "ops68", "ops68 bad op at 63",
             "ops68 bad op at 65")
EDGE_PLACES = [(v, d) for v in EDGE_SHORT for d in (1, 35, 36, 37)] + [(v, d) for v in EDGE_LONG for d in (250, 100)]


def build(contig_lengths=LENS):
    """(stream bytes, places): places = [(section, variant index, offset, bytes to the tile's end or None)], section
    "copy0" ... "copy3", "edge", "border"."""
    s = Stream(contig_lengths)
    places = []

    def put(section, i, x=None, edge=None):
        if x is not None:
            s.fill_to(x - 10 * 38, big=200)
        s.tiny(10)
        places.append((section, i, s.add(TABLE[i][1]), edge))

    for j, r in enumerate(COPY_RESIDUES):
        for i in range(len(TABLE)):
            lo = len(s) + 38 + 10 * 38
            put(f"copy{j}", i, lo + (r - lo) % 64)
    for label, d in EDGE_PLACES:
        T = -(-(len(s) + 38 + 10 * 38 + d) // K_TILE) * K_TILE
        put("edge", INDEX[label], T - d, d)
    s.fill_to(len(s) + K_INTERIOR_TAIL + K_TILE + 1024, big=300)
    for i in range(len(TABLE)):
        put("border", i)
    s.tiny(10)
    u, _ = s.finish()
    return u, places


def interior_span(x0, x1, L):
    """[lo, hi) covered by the interior tiles of a launch over [x0, x1): interior_tiles() of sbam_check.hip, as
    test_check_general_kernel.tiles restates it."""
    x0a = x0 & ~63
    lim = min(x1, L - K_INTERIOR_TAIL)
    tlo = 0 if x0 == x0a else 1
    thi = max((lim - x0a) // K_TILE if lim - x0a >= K_TILE else 0, tlo)
    return x0a + tlo * K_TILE, x0a + thi * K_TILE


# ---- contig tables ---------------------------------------------------------------------------------------------
# name -> (lengths in the stream's header, lengths handed to both checkers or None for the header's)
TABLES = {
    "header": (LENS, None),
    "5000": (LENS, LENS_5000),
    "empty": (LENS, ()),
    "negative header": ((1000, -1, -5, IMAX), None),
    "past int32": (LENS, (2**31, 0, 1, 2**32 + 5)),
}


class Case:
    """One stream under one contig table: the oracle's answers, computed once and left unchanged."""

    def __init__(self, u, lens=None):
        import oracle
        self.u, self.lens = u, lens
        self.blob = bgzf(u)
        self.o = oracle.BamFile(self.blob)
        assert self.o.L == len(u)
        if lens is not None:
            self.o.lens = np.zeros(1 << 16, np.int64)
            self.o.lens[:len(lens)] = lens
            self.o.nref = len(lens)
        self.L = self.o.L
        self._w = {}

    def words(self, R):
        if R not in self._w:
            w = self.o.check_full_range(0, self.L, R)
            w.setflags(write=False)
            self._w[R] = w
        return self._w[R]

    def open(self):
        import sbam
        if self.lens is None:
            return sbam.BamFile(self.blob, path="flag_edges.bam")
        return sbam.BamFile(self.blob, path="flag_edges.bam", contig_lengths=np.asarray(self.lens, np.int64))


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            header, lens = TABLES[name]
            u, places = build(header)
            cache[name] = (Case(u, lens), places)
        return cache[name]
    return get


def ranges(places, L):
    """The whole stream and two unaligned sub-ranges that begin inside a variant."""
    a = next(x for sec, i, x, _ in places if sec == "copy0" and TABLE[i][0] == "ref contig=0 pos=1001")
    b = next(x for sec, i, x, _ in places if sec == "copy2" and TABLE[i][0] == "ops68 bad op at 64")
    return [(0, L), (a + 5, interior_span(0, L, L)[1] - 7), (b + 3, L - 3)]


# ---- CPU: the oracle agrees with the literals, and the stream covers what it claims --------------------------------
def test_stream_layout(cases):
    c, places = cases("header")
    assert c.L < 1_000_000
    lo, hi = interior_span(0, c.L, c.L)
    assert lo == 0 and hi % K_TILE == 0 and hi + K_INTERIOR_TAIL <= c.L < hi + K_TILE + K_INTERIOR_TAIL
    for j, r in enumerate(COPY_RESIDUES):
        xs = [x for sec, _, x, _ in places if sec == f"copy{j}"]
        assert len(xs) == len(TABLE) and all(x % 64 == r and x + 600 < hi for x in xs)
    assert {r % 4 for r in COPY_RESIDUES} == {0, 1, 2, 3} and {0, 31} <= {r % 32 for r in COPY_RESIDUES}
    edge = [(TABLE[i][0], x, d) for sec, i, x, d in places if sec == "edge"]
    assert [(v, d) for v, _, d in edge] == EDGE_PLACES
    for v, x, d in edge:
        assert (x + d) % K_TILE == 0 and x + d < hi  # d bytes before the end of an interior tile
    assert {d for _, _, d in edge} == {1, 35, 36, 37, 100, 250}
    for v, x, d in edge:
        if v in EDGE_LONG:  # 36 fixed bytes, then 255 name bytes or 7 and 272 bytes of ops: across the tile's end,
            assert 36 < d < 36 + 255  # and from 100 bytes before it the name too runs past the eager wave's 64-B halo
            assert (d == 100) == (36 + 255 - d > 64) and 36 + 7 + 272 - d > 64
    border = [x for sec, _, x, _ in places if sec == "border"]
    assert len(border) == len(TABLE) and min(border) - 380 >= c.L - K_INTERIOR_TAIL >= hi
    # a tile and a tail of passing records in front of the border copy
    pad0 = max(x for sec, _, x, _ in places if sec == "edge") + 600
    assert min(border) - 380 - pad0 >= K_INTERIOR_TAIL + K_TILE
    rs = ranges(places, c.L)
    starts = {x for _, _, x, _ in places}
    for x0, x1 in rs[1:]:
        assert x0 % 64 and any(x < x0 < x + 40 for x in starts)
        ilo, ihi = interior_span(x0, x1, c.L)
        assert ihi - ilo >= 2 * K_TILE
    assert rs[2][1] > c.L - K_INTERIOR_TAIL


def test_oracle_gives_the_literal_flag_sets(cases):
    c, places = cases("header")
    w = c.words(1)
    assert len(TABLE) >= 120
    for sec, i, x, _ in places:
        label, _, flags = TABLE[i]
        want = word(flags) if flags else SUCC | (1 << 24)
        assert w[x] == want, (sec, label, x, hex(int(w[x])), hex(want))


def test_every_flag_alone_in_every_residue_class_and_tile_kind(cases):
    c, places = cases("header")
    w = c.words(1)
    lo, hi = interior_span(0, c.L, c.L)
    at = np.arange(c.L)
    for f in SOLE_FLAGS:
        hit = at[w == word((f,))]
        assert {int(x) % 4 for x in hit[hit < hi]} == {0, 1, 2, 3}, f
        assert {int(x) % 64 for x in hit[hit < hi]} >= set(COPY_RESIDUES), f
        assert (hit >= hi).any(), f


def test_failures_after_passing_records(cases):
    c, places = cases("header")
    w = c.words(10)
    lo, hi = interior_span(0, c.L, c.L)
    at = np.arange(c.L)
    for f in SOLE_FLAGS:
        for k in range(1, 10):
            hit = at[w == word((f,), k)]
            assert (hit < hi).any() and (hit >= hi).any(), (f, k)
    rbe = c.o.counts_range(0, c.L, 10)[2]
    assert (rbe[2, 1:10] > 0).all() and (rbe[3, 1:10] > 0).all()  # one flag and two, after 1 ... 9 reads
    assert pair_hist(w).sum() > 0


def test_tables_change_the_answers(cases):
    """Under 5000 lengths the variants at refID 4095 ... 4999 are in range (refPos == length passes, + 1 fails); under
    no lengths refID 0 is too large; below zero and past INT32_MAX the length compares as the int64 it is."""
    places = cases("header")[1]
    first = {TABLE[i][0]: x for sec, i, x, _ in places if sec == "copy0"}
    w = cases("5000")[0].words(1)
    for tag, d in (("ref", 0), ("next", 4)):
        for ri in (4095, 4096, 4999):
            assert w[first[f"{tag} idx={ri} pos=len"]] == SUCC | (1 << 24)
            assert w[first[f"{tag} idx={ri} pos=len+1"]] == word((4 + d,))
        assert w[first[f"{tag} idx=5000 pos=len"]] == word((2 + d,))
    w = cases("empty")[0].words(1)
    assert w[first["base"]] == word((2, 6)) and w[first["ref idx=-1"]] == word((6,))
    w = cases("negative header")[0].words(1)
    assert cases("negative header")[0].o.lens[:4].tolist() == [1000, -1, -5, IMAX]
    assert w[first["ref contig=1 pos=-1"]] == SUCC | (1 << 24) and w[first["ref contig=1 pos=0"]] == word((4,))
    assert w[first["ref contig=2 pos=-1"]] == word((4,)) and w[first["ref contig=2 pos=-2"]] == word((3,))
    assert w[first["next contig=2 pos=-1"]] == word((8,)) and w[first["next contig=1 pos=0"]] == word((8,))
    w = cases("past int32")[0].words(1)
    assert w[first["ref contig=0 pos=1001"]] == SUCC | (1 << 24)
    assert w[first["next contig=3 pos=2147483647"]] == SUCC | (1 << 24)


# ---- GPU: the four entry points against the oracle -------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(cases):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = cases(name)[0].open()
        return cache[name]
    yield get
    for g in cache.values():
        g.close()


def assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} mismatches, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


def check_all(g, c, R, x0, x1):
    """check_full_words, check_full_counts (both forms) and check_eager over [x0, x1) against the oracle."""
    want = c.words(R)[x0:x1]
    assert_same(g.check_full_words(x0, x1, R), want, f"words [{x0}, {x1}) R={R}")
    assert_same(g.check_eager(x0, x1, R), (want & SUCC) != 0, f"eager [{x0}, {x1}) R={R}")
    for by_key in (False, True):
        got = check_counts(g, c.o, want, x0, x1, R, by_key)
        assert np.array_equal(got.pair_hist, pair_hist(want)), (x0, x1, R, by_key)


@pytest.mark.gpu
@pytest.mark.parametrize("R", READS_TO_CHECK)
@pytest.mark.parametrize("table", list(TABLES))
def test_flag_table_on_the_gpu(table, R, cases, gpu):
    c, places = cases(table)
    g = gpu(table)
    assert g.uncompressed_size == c.L
    if c.lens is None:  # the caller's values, as the header holds them
        assert g.contig_lengths.tolist() == list(TABLES[table][0])
    else:
        assert g.contig_lengths.tolist() == list(c.lens)
    for x0, x1 in ranges(places, c.L):
        check_all(g, c, R, x0, x1)


# ---- part 2: stream ends ---------------------------------------------------------------------------------------------
def end_stream(tail=b"", records=(), lead=12):
    """(stream, offsets of the lead-in records, offset of the first of `records` / of the tail)."""
    s = Stream(LENS)
    lead_at = [s.add(record()) for _ in range(lead)]
    at = len(s)
    for r in records:
        s.add(r)
    s.junk(tail)
    return s.finish()[0], lead_at, at


def make_end_cases():
    """name -> (stream, {(offset, reads_to_check): literal word})."""
    out = {}

    def case(name, want, tail=b"", records=()):
        u, lead_at, at = end_stream(tail, records)
        out[name] = (u, {(at if x is None else lead_at[x], R): w for (x, R), w in want.items()})

    # the fixed fields: 35 bytes left is tooFewFixedBlockBytes, 36 reads them and misses the name
    case("35 bytes left", {(None, 1): word((0,))}, rec()[:35])
    case("36 bytes left", {(None, 1): word((9,))}, rec()[:36])
    case("37 bytes left", {(None, 1): word((9,))}, rec()[:37])
    # the name: on the end it is read (then the missing op array speaks); one byte short is flag 9 with the position
    # flags and flag 18 kept, and nothing from the CIGAR or the EmptyMapped test
    faulty = dict(ref_id=-2, next_pos=-2, aux=b"", block_size=implied_size(7, 0, 20) - 1)
    case("name ends on the end, no ops", {(None, 1): word((1, 7, 17, 18))}, rec(cigar=(), **faulty)[:43])
    case("name one byte past the end, no ops", {(None, 1): word((1, 7, 9, 18))}, rec(cigar=(), **faulty)[:42])
    case("name one byte past the end", {(None, 1): word((9,))}, rec()[:42])
    # the op array (flag 14), a bad op before the cut (15 only), an empty mapped sequence (14, no 16)
    ops = rec(cigar=OPS68)
    case("ops cut at op 0", {(None, 1): word((14,))}, rec()[:43])
    case("ops cut inside op 0", {(None, 1): word((14,))}, ops[:43 + 3])
    case("ops cut at op 1", {(None, 1): word((14,))}, ops[:43 + 4])
    case("ops cut inside op 65", {(None, 1): word((14,))}, ops[:43 + 4 * 65 + 2])
    case("bad op 0, cut at op 1", {(None, 1): word((15,))}, rec(cigar=bad_op(0))[:43 + 4])
    case("bad op 63, cut inside op 65", {(None, 1): word((15,))}, rec(cigar=bad_op(63))[:43 + 4 * 65 + 2])
    case("bad op 65, cut inside op 65", {(None, 1): word((14,))}, rec(cigar=bad_op(65))[:43 + 4 * 65 + 2])
    case("empty mapped sequence, ops cut", {(None, 1): word((14,))}, rec(l_seq=0)[:43 + 2])
    # the chain ends on the stream's end: Success with fewer than reads_to_check records
    case("chain ends on the end", {(9, 10): SUCC | (3 << 24), (9, 2): SUCC | (2 << 24), (11, 2): SUCC | (1 << 24)})
    # a last block_size past the end: both sides clamp, and the next read finds no fixed bytes (parity unpinned)
    past = rec(block_size=len(rec()) - 4 + 100)
    case("block_size past the end", {(11, 10): word((0,), 2), (11, 2): SUCC | (2 << 24), (3, 10): SUCC | (10 << 24),
                                     (4, 10): word((0,), 9), (3, 11): word((0,), 10), (None, 2): word((0,), 1)},
         records=[past])
    # a last block_size short of the record's own op (l_seq -1: by a byte, -3: by the op) or of its name too (-9:
    # the declared end lies in the fixed fields), while name and op end on the stream's end: the next read starts at
    # the end, the record's declared end lies before it
    for ls in (-1, -3, -9):
        case(f"block_size short of the ops, l_seq={ls}",
             {(None, 1): SUCC | (1 << 24), (None, 2): word((0,), 1), (11, 10): word((0,), 2)}, records=[bare(ls, 0)])
    return out


END_CASES = make_end_cases()


@pytest.fixture(scope="module")
def end_cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(END_CASES[name][0])
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(END_CASES))
def test_oracle_at_the_stream_end(name, end_cases):
    c = end_cases(name)
    assert c.L < 4096
    for (x, R), want in END_CASES[name][1].items():
        got = c.o.check_full(x, R)
        assert got == want, (name, x, R, hex(got), hex(want))


def test_end_cases_raise_the_end_only_flags(end_cases):
    """Flags 9 and 14 occur, each as the sole flag, and flag 0 after 1, 2, 9 passing reads."""
    seen = set()
    for name in END_CASES:
        for R in READS_TO_CHECK:
            seen |= {int(w) for w in end_cases(name).words(R)}
    assert {word((9,)), word((14,)), word((0,), 1), word((0,), 2), word((0,), 9), SUCC | (3 << 24)} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(END_CASES))
def test_stream_ends_on_the_gpu(name, end_cases):
    c = end_cases(name)
    with c.open() as g:
        assert g.uncompressed_size == c.L
        for R in READS_TO_CHECK:
            check_all(g, c, R, 0, c.L)
