"""The block table by following BSIZE hops (k_follow_blocks, k_follow_link and the compaction behind them) and the
block search on the bytes themselves (k_find_block_starts_bytes), on files built here with tests/bgzf_writer.py around
the follow path's own edges: its segments of sbam_follow_segment_bytes() bytes, the slots per segment, the speculative
entry behind a segment's edge, and MetadataStream's stop rules inside a later segment.

Every expected table is the CPU oracle's (or_metadata_stream through test_bgzf_edges.oracle_table, MetadataStream.scala:
23-54) and every expected block start is or_find_block_start's (FindBlockStart.scala:8-36).  Every table case also
asserts sbam_scan_path, so a follow path that always fell back to the byte scan, or never did, fails here.  Each
construction has a CPU test that asserts the file has the property it was built for."""
import numpy as np
import pytest

from bgzf_writer import STORED_OVERHEAD, candidates, deflated_block, eof_marker, fake_header, stored_block, stored_file
from test_bgzf_edges import (NCHK, PARSE_CASES, assert_starts, assert_stream, assert_table, base, build_small,  # noqa: F401
                             damaged, oracle_table, table_of, windows)

FOLLOWED = {"followed": True, "fell_back": False}
FELL_BACK = {"followed": False, "fell_back": True}


def seg() -> int:
    """kFollowSeg of the library under test (loads without a GPU)."""
    import sbam
    return int(sbam.load_library().sbam_follow_segment_bytes())


def nseg(D: int, start_rel: int = 0) -> int:
    S = seg()
    return max(1, (D + S - 1) // S - start_rel // S)


def assert_path(g, want, D, start_rel: int = 0):
    got = g.scan_path()
    assert {k: got[k] for k in want} == want, got
    assert got["segments"] == nseg(D, start_rel), got


def check_file(blob, want_path, stream: bool = False, path: str = "follow"):
    """The table (and the stream) of `blob` against the oracle's, on the path the case was built for."""
    import oracle
    import sbam
    o = oracle.BamFile(blob)
    with sbam.BamFile(blob, path=path, inflate=stream) as g:
        assert_path(g, want_path, len(blob))
        assert g.n_blocks == o.nblocks
        assert_table(g.blocks(), table_of(o))
        if stream:
            assert_stream(g, o)


# ---- a. well-formed files ---------------------------------------------------------------------------------------

MIXED_SIZES = (3000, 20000, 60000, 100, 45000, 0, 9000)


def build_mixed(u):
    """Stored and deflated members of mixed sizes in turn, XLEN 6, 10, 11 and 12, and zero-length stored members that
    are not the EOF marker (a 5-byte stored DEFLATE block, not the marker's 2 bytes), then the marker."""
    extras = (b"", b"XY\x00\x00", b"", b"ZZ\x01\x00q", b"", b"XY\x02\x00ab", b"")
    parts, x, i = [], 0, 0
    while x < len(u):
        n = MIXED_SIZES[i % len(MIXED_SIZES)]
        make = stored_block if i % 2 == 0 or n == 0 else deflated_block  # (deflated nothing is the marker's 2 bytes)
        parts.append(make(u[x:x + n], extra=extras[i % len(extras)] if i % 3 else b""))
        x += n
        i += 1
    return b"".join(parts) + eof_marker()


@pytest.fixture(scope="module")
def mixed(base):
    import oracle
    blob = build_mixed(base[0])
    return blob, oracle.BamFile(blob)


def test_mixed_file_has_what_it_says(mixed, base):
    blob, o = mixed
    S = seg()
    assert S >= 128 << 10 and S & (S - 1) == 0
    assert 4 * S < len(blob) < 8 << 20 and o.L == len(base[0])  # a handful of segments
    assert {18, 22, 23, 24} <= set(o.hsize.tolist())  # XLEN 6, 10, 11, 12
    assert int((o.usize == 0).sum()) >= 5 and int(o.csize.max()) > 60000 and int(o.csize.min()) <= 40
    assert candidates(blob).size == o.nblocks + 1  # no header pattern but the members' own


@pytest.mark.gpu
def test_mixed_blocks_are_followed(mixed):
    check_file(mixed[0], FOLLOWED, stream=True)


EDGE_PHASES = tuple(range(18))  # the member starts k bytes before the segment edge: k = 0 ends a block on the edge


def build_edge(u, k):
    S = seg()
    return stored_file(u[:S + 150_000], 60000, starts=[S - k])


def test_edge_files_put_a_header_across_the_segment_edge(base):
    S = seg()
    for k in EDGE_PHASES:
        st, cs, _, _ = oracle_table(build_edge(base[0], k))
        assert S - k in st.tolist(), k
        if k == 0:
            assert S in (st + cs).tolist()


@pytest.mark.gpu
def test_header_across_the_segment_edge(base):
    """One context, reloaded per phase."""
    import sbam
    g = None
    for k in EDGE_PHASES:
        blob = build_edge(base[0], k)
        if g is None:
            g = sbam.BamFile(blob, path="edge", inflate=False)
        else:
            g.load(np.frombuffer(blob, np.uint8))
            g.n_blocks = g._scan()
        assert_path(g, FOLLOWED, len(blob))
        assert_table(g.blocks(), oracle_table(blob))
    g.close()


LENGTHS = [(k, e, marker) for k in (1, 2) for e in (0, 1, 17, 18) for marker in (True, False)]


def test_length_files_have_their_lengths(base):
    S = seg()
    for k, e, marker in LENGTHS:
        blob = stored_file(base[0], 60000, marker=marker, total=k * S + e)
        st, cs, _, _ = oracle_table(blob)
        assert len(blob) == k * S + e and int(st[-1] + cs[-1]) == len(blob) - (28 if marker else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,e,marker", LENGTHS)
def test_file_length_at_the_segment_edge(base, k, e, marker):
    check_file(stored_file(base[0], 60000, marker=marker, total=k * seg() + e), FOLLOWED)


# ---- b. one block, fewer than 18 bytes, no bytes ------------------------------------------------------------------

TINY = {"one block": stored_block(b"abc") + eof_marker(), "one block, no marker": deflated_block(b"abc" * 50),
        "17 bytes": stored_block(b"abc")[:17], "no bytes": b""}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(TINY))
def test_tiny_files(what):
    import sbam
    blob = TINY[what]
    want = oracle_table(blob)
    assert want[0].size == (1 if what.startswith("one block") else 0)
    with sbam.BamFile(blob, inflate=False) as g:
        assert_path(g, FOLLOWED, len(blob))
        assert g.n_blocks == want[0].size
        assert_table(g.blocks(), want)


# ---- c. fake headers ----------------------------------------------------------------------------------------------

FAKE_PAYLOAD = 20000
FAKE_BLOCK = FAKE_PAYLOAD + STORED_OVERHEAD


def plant(v: bytearray, p: int, bsize_minus_1: int):
    """A header pattern over the 18 payload bytes at file position p of stored_file(v, FAKE_PAYLOAD)."""
    k, j = divmod(p, FAKE_BLOCK)
    j -= 23
    assert 0 <= j <= FAKE_PAYLOAD - 18, (p, j)
    v[k * FAKE_PAYLOAD + j:k * FAKE_PAYLOAD + j + 18] = fake_header(bsize_minus_1)


def next_member(p: int) -> int:
    return (p // FAKE_BLOCK + 1) * FAKE_BLOCK


def fake_positions():
    """{kind: file position}: just behind the first segment edge (the first pattern position at or after it), and in
    the middle of the second segment; both inside a payload."""
    S = seg()
    at = {"edge": S + 10, "middle": S + S // 2 + 10}
    for kind, p in list(at.items()):
        while not 23 <= p % FAKE_BLOCK <= FAKE_BLOCK - 8 - 18 - 200:  # (not in a member's header or footer)
            p += 64
        at[kind] = p
    return at


def build_fake(u, kind):
    """Stored members of 20000 payload bytes with one fake header whose BSIZE leads to the next member's real header."""
    p = fake_positions()[kind]
    v = bytearray(u)
    plant(v, p, next_member(p) - p - 1)
    return stored_file(bytes(v), FAKE_PAYLOAD), p


def test_fakes_sit_where_they_say(base):
    S = seg()
    for kind in ("edge", "middle"):
        blob, p = build_fake(base[0], kind)
        o_st = oracle_table(blob)[0]
        c = candidates(blob)
        assert c.size == o_st.size + 2 and p in c.tolist() and p not in o_st.tolist()  # the table skips it
        assert next_member(p) in o_st.tolist()  # its successor holds a header: a valid-looking entry
        first_behind = {int(c[np.searchsorted(c, g * S)]) for g in range(1, len(blob) // S + 1) if c[-1] >= g * S}
        assert (p in first_behind) == (kind == "edge")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,want", [("edge", FELL_BACK), ("middle", FOLLOWED)])
def test_fake_header_at_a_segment_entry_costs_the_fallback(base, kind, want):
    check_file(build_fake(base[0], kind)[0], want, stream=True)


# ---- d. more blocks in a segment than its slots ---------------------------------------------------------------------

def test_small_blocks_fill_a_segment_past_its_slots(base):
    S = seg()
    slots = S // 2048
    for kind, over in (("2047", True), ("2048", False), ("mixed300", True)):
        st = oracle_table(build_small(base[0], kind))[0]
        per_seg = np.bincount(st // S)
        assert (per_seg.max() > slots) == over and per_seg.size >= 2, kind
        assert over or per_seg.max() == slots  # 2048-byte blocks: exactly full


@pytest.mark.gpu
@pytest.mark.parametrize("kind,want", [("2047", FELL_BACK), ("2048", FOLLOWED), ("mixed300", FELL_BACK)])
def test_small_blocks(base, kind, want):
    check_file(build_small(base[0], kind), want)


# ---- e. stops -------------------------------------------------------------------------------------------------------

def test_marker_in_the_middle_lies_past_the_first_segment(mixed):
    blob, o = mixed
    assert len(blob) - 28 > 2 * seg() and oracle_table(blob + blob)[0].size == o.nblocks


@pytest.mark.gpu
def test_marker_in_the_middle(mixed):
    """cat a.bam b.bam: the chain stops at a's EOF marker, segments behind it contribute nothing."""
    blob, o = mixed
    check_file(blob + blob, FOLLOWED, stream=True)


def cuts(o):
    """Inside a header, a payload and a footer of blocks in the third segment or later, and the same at the end."""
    S = seg()
    k = int(np.searchsorted(o.start, 2 * S)) + 1
    out = []
    for b in (k, k + 1, o.nblocks - 1):
        s, c = int(o.start[b]), int(o.csize[b])
        out += [s + 7, s + 17, s + 18, s + c // 2, s + c - 8, s + c - 3, s + c - 1]
    return sorted(set(out))


def test_cuts_take_both_block_counts(mixed):
    blob, o = mixed
    k = int(np.searchsorted(o.start, 2 * seg())) + 1
    n = {D: oracle_table(blob[:D])[0].size for D in cuts(o)}
    assert n[int(o.start[k]) + 7] == k and n[int(o.start[k]) + int(o.csize[k]) - 1] == k  # cut block: not emitted
    assert n[int(o.start[k + 1]) + 7] == k + 1


@pytest.mark.gpu
def test_truncated_files(mixed):
    """One context, reloaded per cut."""
    import sbam
    blob, o = mixed
    with sbam.BamFile(blob, path="mixed", inflate=False) as g:
        for D in cuts(o):
            g.load(np.frombuffer(blob[:D], np.uint8))
            g.n_blocks = g._scan()
            assert_path(g, FOLLOWED, D)
            assert_table(g.blocks(), oracle_table(blob[:D]))


@pytest.fixture(scope="module")
def ten(base):
    u = base[0][:200000]
    blob = b"".join(deflated_block(u[x:x + 20000]) for x in range(0, len(u), 20000)) + eof_marker()
    import oracle
    return blob, oracle.BamFile(blob)


def scan_error(blob, monkeypatch, follow: bool):
    import sbam
    monkeypatch.setenv("SBAM_SCAN_FOLLOW", "1" if follow else "0")
    with pytest.raises(sbam.HeaderParseException) as e:
        sbam.BamFile(blob, path="damaged", inflate=False)
    v = e.value
    return str(v), getattr(v, "position", None), getattr(v, "expected", None), getattr(v, "actual", None)


@pytest.mark.gpu
@pytest.mark.parametrize("i,v", PARSE_CASES)
def test_parse_error_in_the_fourth_block(ten, monkeypatch, i, v):
    """The followed chain's parse failure runs the byte scan, whose error this is: the oracle's message, and the same
    exception, field by field, as with the follow path switched off."""
    blob, o = ten
    bad = damaged(blob, o, i, v)
    with pytest.raises(ValueError) as want:
        oracle_table(bad)
    got = scan_error(bad, monkeypatch, follow=True)
    assert got[0] == str(want.value)
    assert got == scan_error(bad, monkeypatch, follow=False)


# ---- f. shards ------------------------------------------------------------------------------------------------------

def shard_starts(o):
    S = seg()
    k = int(np.searchsorted(o.start, S)) + 2
    return {"mid-block": int(o.start[k]) + 100, "block start": int(o.start[k + 3]), "near EOF": o.D - 10,
            "first block": 1}


def test_shard_starts_are_what_they_say(mixed):
    blob, o = mixed
    lo = shard_starts(o)
    assert o.find_block_start(lo["mid-block"]) in o.start.tolist() and lo["mid-block"] not in o.start.tolist()
    assert o.find_block_start(lo["block start"]) == lo["block start"]
    assert o.find_block_start(lo["near EOF"]) == lo["near EOF"]  # EOF inside the first header: the start itself
    assert oracle_table(blob, lo["near EOF"])[0].size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mid-block", "block start", "near EOF", "first block"])
def test_shard_tables(mixed, which):
    import sbam
    blob, o = mixed
    lo = shard_starts(o)[which]
    first = o.find_block_start(lo)
    want = oracle_table(blob, first)
    with sbam.BamFile(blob[lo:], base_offset=lo, file_size=len(blob), inflate=False, path=which) as g:
        assert_path(g, FOLLOWED, len(blob) - lo, first - lo)
        st, cs, us, uo = g.blocks()
        if want[0].size:
            assert int(st[0]) == first
        assert_table((st, cs, us, uo), want)


# ---- g. FindBlockStart without a candidate list -----------------------------------------------------------------------

CHAIN_DEPTHS = (1, 2, 5)


def chain_positions():
    """{depth: first fake of a run of `depth` fakes}, each FAKE_BLOCK bytes (its BSIZE + 1) before the next, the last
    one's BSIZE leading into payload bytes: the header test fails `depth` hops behind the first."""
    S = seg()
    return {d: (S // 2 + n * 8 * FAKE_BLOCK) // FAKE_BLOCK * FAKE_BLOCK + 23 + 5000 + 100 * n
            for n, d in enumerate(CHAIN_DEPTHS)}


def build_chains(u):
    v = bytearray(u)
    for d, p in chain_positions().items():
        for h in range(d):
            plant(v, p + h * FAKE_BLOCK, FAKE_BLOCK - 1 if h < d - 1 else 999)
    return stored_file(bytes(v), FAKE_PAYLOAD)


@pytest.fixture(scope="module")
def chains(base):
    import oracle
    blob = build_chains(base[0])
    return blob, oracle.BamFile(blob)


def chain_queries(o):
    rng = np.random.default_rng(7)
    firsts = list(chain_positions().values())
    return np.concatenate([rng.integers(0, o.D + 1, 200), windows(firsts, 12), [p - 3000 for p in firsts],
                           np.arange(o.D - 20, o.D + 1)])


def test_chains_fail_at_their_depth(chains):
    blob, o = chains
    real = set(o.start.tolist())
    for d, p in chain_positions().items():
        assert p not in real
        for n in range(1, 8):  # n headers checked: the fake is taken until the check reaches the failing hop
            assert (o.find_block_start(p, n) == p) == (n <= d), (d, n)
    c = candidates(blob)
    assert c.size == o.nblocks + 1 + sum(CHAIN_DEPTHS)
    # no fake with a header behind it is the first pattern position behind a segment edge: the table is followed
    S = seg()
    first_behind = {int(c[np.searchsorted(c, g * S)]) for g in range(1, len(blob) // S + 1) if c[-1] >= g * S}
    leading = {p + h * FAKE_BLOCK for d, p in chain_positions().items() for h in range(d - 1)}
    assert not (leading & first_behind)


@pytest.mark.gpu
def test_block_search_on_the_bytes(chains, monkeypatch):
    """On a context without candidates (the table was followed) against the oracle; then the same queries on the same
    context once a byte scan has left its candidate list (k_find_block_starts), which must answer the same."""
    import sbam
    blob, o = chains
    qs = np.unique(np.clip(chain_queries(o), 0, o.D))
    with sbam.BamFile(blob, path="chains", inflate=False) as g:
        assert_path(g, FOLLOWED, len(blob))  # (mid-segment fakes; and no candidate list)
        got = {}
        for nchk in NCHK:
            assert_starts(g, o, qs, nchk)
            got[nchk] = g.find_block_starts(qs, nchk)
        monkeypatch.setenv("SBAM_SCAN_FOLLOW", "0")
        g.reset()
        g.n_blocks = g._scan()
        assert g.scan_path() == {"followed": False, "fell_back": False, "segments": 0}
        assert_table(g.blocks(), table_of(o))
        for nchk in NCHK:
            assert np.array_equal(g.find_block_starts(qs, nchk), got[nchk]), nchk
