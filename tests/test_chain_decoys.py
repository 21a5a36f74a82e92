"""The chain pass (csrc/sbam_check.hip: k_p0_list, k_p0_links, k_p0_fast / k_p0_fast16, k_p0_fallback, k_chains) and
the record-chain proof of loadReads (csrc/sbam_records.hip: k_chain_proof, k_split_popcounts, k_split_offsets) on
streams no BAM writer emits: record-shaped decoys inside the aux tails of true records, chain records the checker
rejects, lists shorter than the list pass's vector width, junk behind the last record.  tests/record_stream_writer.py
builds them and says where every record, decoy and hop target lies.

Expected values are the CPU oracle's alone: check_full_range / counts_range for the checker, FindBlockStart →
FindRecordStart → record_chain for the partitions (CanLoadBam.scala:221-241, 281-334).  Which way the GPU took to its
record counts is read from BamFile.records_path() and compared with the predicate in sbam_records.hip's header — the
success bits of [X0, X1) are exactly record_chain(X0, X1) — evaluated from oracle words and the stream, never from
GPU output.  That pins both directions: a proof that holds when it must not (records dropped or invented) and one that
fails when it should hold (the walk hides it, only the time shows).

The tests without the gpu mark check, with the oracle only, that every stream does what its name says and that the
oracle returns partitions (no NoReadFoundException) for every load the GPU tests make."""
import functools
import struct

import numpy as np
import pytest

import bgzf_writer as bw
import record_stream_writer as rw

W_SUCC = 0x80000000
RS = (1, 2, 3, 9, 10)
WHOLE = 1 << 40
TILE, CHUNK = 8192, 131072  # the record-0 pass's tile and the chain pass's chunk, in stream positions


# ---- streams ---------------------------------------------------------------------------------------------------
class Case:
    """One stream as a file: bytes, the writer's offsets, and what the family claims of it."""

    def __init__(self, u, meta, blob, family, **kw):
        self.u, self.meta, self.blob, self.family = u, meta, blob, family
        self.clean = kw.get("clean", False)        # the success bits are exactly the chain
        self.survive = kw.get("survive", ())       # decoys that are Success at every R
        self.r1_only = kw.get("r1_only", ())       # decoys that are Success at R = 1 only
        self.rejected = kw.get("rejected", ())     # chain records that are never Success
        self.tail = kw.get("tail", 0)              # bytes behind the last whole record (the GPU load must raise)
        self.k = kw.get("k", 5)                    # the many-splits load cuts the file into k splits
        self.loads = kw.get("loads")               # [(split size, first, count)], default: whole file, k splits
        self.broken = kw.get("broken", False)      # a list link is missing whatever R is
        self._o, self._w = None, {}

    @property
    def o(self):
        import oracle
        if self._o is None:
            self._o = oracle.BamFile(self.blob)
        return self._o

    def words(self, R, x0=0, x1=None):
        x1 = self.o.L if x1 is None else x1
        if (R, x0, x1) not in self._w:
            self._w[R, x0, x1] = self.o.check_full_range(x0, x1, R)
        return self._w[R, x0, x1]

    def succ(self, R):
        return (self.words(R) & W_SUCC) != 0

    def all_loads(self):
        return self.loads if self.loads is not None else [(WHOLE, 0, None), (len(self.blob) // self.k + 1, 0, None)]


def cut_file(u: bytes, cuts) -> bytes:
    """`u` as stored members that begin at the stream offsets in `cuts` (and at 0), then the EOF marker."""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(u))) + [len(u)]
    return b"".join(bw.stored_block(u[a:b]) for a, b in zip(edges, edges[1:])) + bw.eof_marker()


def body(s, n, i0=0):
    """n true records of mixed sizes, each with an aux tail (so its hop clears its name: a clean link)."""
    for i in range(i0, i0 + n):
        s.add(rw.sized(44 + (i * 7) % 23))


def short_list(n, mixed):
    s = rw.Stream()
    if mixed:
        body(s, n)
    else:
        s.tiny(n)
    u, m = s.finish()
    # (one or two records leave no record start behind the first split's block: the whole file is the only load)
    return Case(u, m, bw.stored_file(u, 60), "short", clean=True, k=3, loads=[(WHOLE, 0, None)] if n <= 2 else None)


def broken_link(j):
    s = rw.Stream()
    body(s, j)
    s.host(at=6 + j % 5, pad=j % 3)
    body(s, 39 - j, j + 1)
    u, m = s.finish()
    return Case(u, m, bw.stored_file(u, 400), "broken", survive=m["decoys"], broken=True, k=4)


# the second decoy of kind f: a tiny record whose every fourth byte is a valid CIGAR op byte, so that it can sit
# inside the first decoy's CIGAR array
F_INNER = rw.record(ref_id=0, pos=0, next_ref_id=0, next_pos=0)


def kind_f_decoy():
    """86 bytes: name "r", 12 CIGAR ops that hold F_INNER, and l_seq = -40, which shrinks the record's implied size so
    that block_size = 34 passes record 0 although the hop (to F_INNER, 38 bytes on) stops short of the CIGAR's end."""
    cig = F_INNER + b"\x00" * 10
    return rw.record(cigar=struct.unpack("<12I", cig), l_seq=-40, block_size=34)


KINDS = ("a", "b", "c1", "c2", "c10", "d", "e", "f")


def place(s, kind, feature="decoy", x=None, at=10, pad=7):
    """One host of the kind, laid so that its (first) decoy, or that decoy's hop target, starts on stream offset x
    (x = None: wherever the stream stands).  Returns (surviving decoys, R = 1 only decoys)."""
    n = {"c1": 2, "c2": 3, "c10": 11}.get(kind, 1)
    decoy = kind_f_decoy() if kind == "f" else rw.record()
    hop = {"a": "next", "b": ("next", 3), "d": ("end", 5), "e": ("end", 0), "f": ("self", 34)}.get(kind, "chain")
    if x is not None:
        rel = rw.TINY + at  # the decoy, from the host's start
        if feature == "target":
            rel = {"a": rel + 38 + pad, "b": rel + 38 + pad + 3}.get(kind, rel + 38)  # c*: the second decoy
        s.fill_to(x - rel, big=1500)
    _, ds = s.host(decoy, at=at, pad=pad, hop=hop, n_decoys=n)
    if kind == "f":  # the inner decoy hops to the host's end and survives; the outer one is PASS0 only
        inner = ds[0] + 38
        s._patch(inner, len(s))
        s.decoys.append(inner)
        s.targets.append(len(s))
        return [inner], [ds[0]]
    return (ds, []) if kind in ("a", "c1", "c2", "c10", "e") else ([], ds)


def kind_mid(kind):
    s = rw.Stream()
    body(s, 30)
    sv, r1 = place(s, kind)
    body(s, 30, 31)
    u, m = s.finish()
    from test_eager_wave import bgzf
    return Case(u, m, bgzf(u, 700), "kind", survive=sv, r1_only=r1, broken=bool(sv), k=3)


# word, tile and chunk edges, ascending and at least 4 KB apart
EDGES = (64 * 70, 64 * 140 + 63, TILE * 2 - 1, TILE * 3, CHUNK - 1, CHUNK + TILE * 2, CHUNK * 2 - 1 - TILE * 2,
         CHUNK * 2)
EDGES2 = (64 * 70 + 63, 64 * 140, TILE * 2, TILE * 3 - 1, CHUNK, CHUNK + TILE * 2 - 1, CHUNK * 2 - 1, CHUNK * 2 + TILE)


def kind_edges(kind, feature, edges):
    s = rw.Stream()
    sv, r1 = [], []
    for x in edges:
        a, b = place(s, kind, feature, x)
        sv += a
        r1 += b
    s.fill_to(CHUNK * 2 + TILE * 3, big=1500)
    u, m = s.finish()
    return Case(u, m, bw.stored_file(u, 5000), "edges", survive=sv, r1_only=r1, broken=bool(sv), k=7)


# (a host that holds a 38-byte decoy is at least 76 bytes long, so its hop never stays inside one word: the one-word
# hop is tests/test_chain_proof_kernels.py's)
GEOMETRY = [(W, al, where) for W in (2, 7, 8, 9, 12) for al in ("mid", "word") for where in ("first", "middle", "last")
            if not (W == 2 and where == "middle")]
GEO_BLOCK = 2432  # payload bytes per geometry: one stored member, one Hadoop split


def hop_geometry():
    """One host per block; the bits (p, q) between the host p and its end q cover W bitmap words, q on bit 41 ("mid",
    p on bit 20) or on bit 0 ("word", p on bit 63); the decoy lies in the first, a middle or the last of them.  Block 0
    holds the header and clean records; the last block is clean (the control split)."""
    s = rw.Stream()
    body(s, 5)
    s.fill_to(GEO_BLOCK, big=300)
    sv = []
    for i, (Wn, al, where) in enumerate(GEOMETRY):
        b0 = GEO_BLOCK * (i + 1)
        p = b0 + 64 * 2 + (20 if al == "mid" else 63)
        q = ((p + 1) // 64 + Wn - 1) * 64 + 41 if al == "mid" else (p + 1) + 64 * Wn
        s.fill_to(p, big=300)
        room = q - p - 2 * rw.TINY  # filler bytes to share between `at` and `pad`
        at = {"first": 0, "last": room, "middle": ((p + 1) // 64 + Wn // 2) * 64 + 5 - p - rw.TINY}[where]
        assert 0 <= at <= room
        h, ds = s.host(at=at, pad=room - at)
        assert h == p and len(s) == q, (h, p, len(s), q)
        sv += ds
        s.fill_to(b0 + GEO_BLOCK, big=300)
    body(s, 40)
    s.fill_to(GEO_BLOCK * (len(GEOMETRY) + 2), big=300)
    u, m = s.finish()
    S = GEO_BLOCK + bw.STORED_OVERHEAD
    loads = [(S, i, 1) for i in range(len(GEOMETRY) + 2)] + [(S, 0, None), (WHOLE, 0, None)]
    return Case(u, m, bw.stored_file(u, GEO_BLOCK), "geometry", survive=sv, broken=True, loads=loads)


REJECTS = {
    "cigar": lambda: rw.record(ref_id=0, pos=5, flag=0, cigar=[(10 << 4) | 9], seq=b"\x11" * 5, qual=b"\x20" * 10),
    "refidx": lambda: rw.record(ref_id=1, pos=5, aux=rw.filler(9)),
    "name": lambda: rw.record(name=b"a\x01b", aux=rw.filler(9)),
}


def rejected(what, where):
    s = rw.Stream()
    n0 = {"first": 0, "mid": 25, "last": 50, "split": 25}[where]
    body(s, n0)
    x = s.add(REJECTS[what]())
    body(s, 50 - n0, n0 + 1)
    u, m = s.finish()
    if where == "split":  # a block starts on the rejected record, and a Hadoop split starts on that block
        blob = cut_file(u, [x])
        return Case(u, m, blob, "rejected", rejected=[x], loads=[(WHOLE, 0, None), (x + bw.STORED_OVERHEAD, 0, None),
                                                                  (x + bw.STORED_OVERHEAD, 1, 1)])
    # (the records within reads_to_check of a rejected last record are no Success: no split may begin among them)
    return Case(u, m, bw.stored_file(u, 500), "rejected", rejected=[x], k=3 if where == "last" else 4)


def split_on_decoy():
    """A block (and a Hadoop split) begins inside a host, 9 bytes before its kind-a decoy: FindRecordStart returns the
    decoy, and the split's chain in the reference starts there."""
    s = rw.Stream()
    body(s, 30)
    _, ds = s.host(at=40, pad=5)
    body(s, 30, 31)
    u, m = s.finish()
    cut = ds[0] - 9
    S = cut + bw.STORED_OVERHEAD
    return Case(u, m, cut_file(u, [cut]), "split_on_decoy", survive=ds, broken=True,
                loads=[(WHOLE, 0, None), (S, 0, None), (S, 0, 1), (S, 1, 1)])


def tail(kind):
    s = rw.Stream()
    body(s, 30)
    junk = b"" if kind == "exact" else rw.sized(60)[:50] if kind == "trunc" else rw.filler(kind)
    x = s.junk(junk)
    r1 = []
    if kind == "trunc":  # a record whose block_size runs past the stream's end passes record 0: Success at R = 1
        r1 = [x]
        s.decoys.append(x)
        s.targets.append(x + 60)
    u, m = s.finish()
    return Case(u, m, bw.stored_file(u, 300), "tail", clean=kind == "exact", tail=len(junk), r1_only=r1,
                loads=None if kind == "exact" else [(WHOLE, 0, None)])


def subrange():
    """Clean records, a host whose kind-b decoy hops 3 bytes past the next record, a block boundary, a host with a
    kind-a decoy, a block boundary on its end, clean records."""
    s = rw.Stream()
    body(s, 30)
    _, db = s.host(at=5, pad=80, hop=("next", 3))  # (121 bytes from the decoy to its target: a word edge between)
    h, ds = s.host(at=30, pad=12)
    end = len(s)
    body(s, 30, 32)
    u, m = s.finish()
    m["host"], m["host_end"] = h, end
    return Case(u, m, cut_file(u, [m["records"][12], h, end]), "subrange", survive=ds, r1_only=db, broken=True)


SHORT_NS = (1, 2, 9, 10, 11, 15, 16, 17, 23, 24, 25, 40)
BUILDERS = {}
for _n in SHORT_NS:
    for _mixed in (False, True):
        BUILDERS[f"short-{_n}-{'mixed' if _mixed else 'tiny'}"] = (functools.partial(short_list, _n, _mixed), RS)
for _j in range(40):
    BUILDERS[f"broken-{_j}"] = (functools.partial(broken_link, _j), (2, 3, 10))
for _k in KINDS:
    BUILDERS[f"kind-{_k}"] = (functools.partial(kind_mid, _k), RS)
    BUILDERS[f"edges-{_k}-decoy"] = (functools.partial(kind_edges, _k, "decoy", EDGES), RS)
    BUILDERS[f"edges-{_k}-decoy2"] = (functools.partial(kind_edges, _k, "decoy", EDGES2), (1, 2, 10))
    if _k in ("a", "b", "c1", "c2", "c10"):  # d, e and f hop to the stream's end or into themselves
        BUILDERS[f"edges-{_k}-target"] = (functools.partial(kind_edges, _k, "target", EDGES), RS)
        BUILDERS[f"edges-{_k}-target2"] = (functools.partial(kind_edges, _k, "target", EDGES2), (1, 2, 10))
BUILDERS["geometry"] = (hop_geometry, (1, 2, 10))
for _what in REJECTS:
    for _where in ("first", "mid", "last", "split"):
        BUILDERS[f"rejected-{_what}-{_where}"] = (functools.partial(rejected, _what, _where), RS)
BUILDERS["split-on-decoy"] = (split_on_decoy, RS)
for _t in ("exact", 1, 35, 36, "trunc"):
    BUILDERS[f"tail-{_t}"] = (functools.partial(tail, _t), (1, 2, 10))
CASES = list(BUILDERS)
BUILDERS["subrange"] = (subrange, RS)  # (test_checked_subrange's, with loads of its own)
CASE_RS = [(name, R) for name in CASES for R in BUILDERS[name][1]]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return BUILDERS[name][0]()


# ---- the oracle's answers ---------------------------------------------------------------------------------------
def expected_load(c, R, S, first, count):
    """(first records xs, chain ends xe, partitions) of Hadoop splits [first, first + count) from the oracle;
    RuntimeError where the reference raises NoReadFoundException."""
    import oracle
    o = c.o
    sp = oracle.hadoop_splits(o.D, S)
    sp = sp[first:] if count is None else sp[first:first + count]
    xs, xe, parts = [], [], []
    for a, b in sp:
        x = o.find_record_start(o.find_block_start(a), R)
        if x is None:
            raise RuntimeError(f"NoReadFoundException: {a}")
        xs.append(x)
        xe.append(o.x_end_of(b))
        parts.append(o.record_chain(x, xe[-1]))
    return xs, xe, parts


def proof_holds(c, R, X0, X1, x0=0, x1=None):
    """sbam_records.hip's predicate: the success bits of [X0, X1) are exactly record_chain(X0, X1).  The bits are the
    oracle's calls at R over the checked range [x0, x1)."""
    w = c.words(R, x0, x1)
    bits = np.flatnonzero((w[X0 - x0:X1 - x0] & W_SUCC) != 0) + X0
    return np.array_equal(bits, c.o.record_chain(X0, X1))


# ---- without a GPU: the streams are what their names say --------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_stream_is_what_its_name_says(name):
    c = case(name)
    o, m = c.o, c.meta
    assert o.L == len(c.u) and np.array_equal(o.u[:o.L], np.frombuffer(c.u, np.uint8))
    assert o.header_end == m["header_end"] and o.nref == 1
    chain = o.record_chain(m["header_end"], o.L).tolist()
    whole = m["records"]
    assert chain == whole
    last_end = whole[-1] + 4 + int.from_bytes(c.u[whole[-1]:whole[-1] + 4], "little")
    assert o.L - last_end == c.tail
    assert not set(m["decoys"]) & set(chain)
    assert sorted(list(c.survive) + list(c.r1_only)) == sorted(m["decoys"])
    for R in BUILDERS[name][1]:
        on = set(np.flatnonzero(c.succ(R)).tolist())
        assert on - set(chain) == set(c.survive) | (set(c.r1_only) if R == 1 else set()), R  # no accidental decoy
        assert not on & set(c.rejected), R
        if c.clean:
            assert sorted(on) == chain, R
    if c.family == "short":
        n = int(name.split("-")[1])
        assert len(chain) == n and int(c.succ(1).sum()) == n  # n PASS0 positions
    if c.family == "kind" or c.family == "edges":
        kind = name.split("-")[1]
        d, t = m["decoys"], m["targets"]
        if kind == "a":
            assert all(x in chain for x in t)
        if kind == "b":
            assert all(x - 3 in chain for x in t)
        if kind.startswith("c"):
            n = int(kind[1:]) + 1
            assert all(t[i] == d[i + 1] for i in range(len(d)) if (i + 1) % n) and \
                all(t[i] in chain for i in range(len(d)) if (i + 1) % n == 0)
        if kind == "d":
            assert all(x > o.L for x in t)
        if kind == "e":
            assert all(x == o.L for x in t)
        if kind == "f":  # the outer decoy's hop is the next PASS0 position and lies before its CIGAR's end
            p0 = np.flatnonzero(c.succ(1))
            for x in c.r1_only:
                nxt = x + 4 + int.from_bytes(c.u[x:x + 4], "little")
                assert nxt == x + 38 and nxt in c.survive and p0[np.searchsorted(p0, x) + 1] == nxt
                assert nxt < x + 36 + c.u[x + 12] + 4 * int.from_bytes(c.u[x + 16:x + 18], "little")
    if c.family == "edges":
        feature = name.split("-")[2]
        got = m["decoys"] if feature.startswith("decoy") else m["targets"] + m["decoys"]
        for x in (EDGES2 if feature.endswith("2") else EDGES):
            assert x in got, (x, feature)
    if c.family == "geometry":
        for (Wn, al, where), d, t in zip(GEOMETRY, m["decoys"], m["targets"]):
            p = max(x for x in whole if x < d)
            assert t in chain and ((t - 1) >> 6) - ((p + 1) >> 6) + 1 == Wn
            word = (d >> 6) - ((p + 1) >> 6)
            assert word == {"first": 0, "last": Wn - 1, "middle": Wn // 2}[where], (Wn, where)
            assert (p % 64, t % 64) == ((20, 41) if al == "mid" else (63, 0))
    if c.family == "split_on_decoy":
        S = c.all_loads()[1][0]
        xs, _, parts = expected_load(c, 10, S, 1, 1)
        assert xs == m["decoys"] and parts[0][0] == m["decoys"][0] and parts[0][1] == m["targets"][0]
    if name.startswith("rejected") and name.endswith("split"):
        S = c.all_loads()[1][0]
        assert c.o.uoff[c.o.block_index_at_or_after(S)] == c.rejected[0]  # split 1 begins on the rejected record


@pytest.mark.parametrize("name", CASES)
def test_oracle_returns_partitions(name):
    """No load of a positive case meets NoReadFoundException; every record of the file is in the whole-file load and
    in the many-splits load exactly once."""
    c = case(name)
    for R in BUILDERS[name][1]:
        for S, first, count in c.all_loads():
            xs, xe, parts = expected_load(c, R, S, first, count)
            if first == 0 and count is None and not c.tail:
                got = np.concatenate(parts).tolist()
                assert sorted(set(got)) == got and set(got) <= set(c.meta["records"]) | set(c.meta["decoys"])
                assert got[-1] == c.meta["records"][-1]
        if len(c.all_loads()) == 2 and c.all_loads()[1][0] != WHOLE:
            assert len(expected_load(c, R, *c.all_loads()[1])[0]) >= 2  # more than one split


def test_predicate_sees_both_directions():
    """The numpy predicate itself: it holds on a clean stream, fails on a surviving decoy and on a rejected chain
    record, and holds again on a range that leaves the offender out."""
    c = case("short-40-mixed")
    assert proof_holds(c, 10, c.meta["header_end"], c.o.L)
    c = case("kind-a")
    d = c.meta["decoys"][0]
    assert not proof_holds(c, 10, c.meta["header_end"], c.o.L)
    assert proof_holds(c, 10, d, c.o.L) and proof_holds(c, 10, c.meta["header_end"], d)
    c = case("rejected-name-mid")
    x = c.rejected[0]
    assert not proof_holds(c, 1, c.meta["header_end"], c.o.L) and proof_holds(c, 1, c.meta["header_end"], x)


# ---- on the GPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_case():
    """The case's file opened on the GPU; one context at a time (the parametrisation keeps a case's tests together)."""
    import sbam
    held = {}

    def get(name):
        if held.get("name") != name:
            if "g" in held:
                held.pop("g").close()
            held["g"] = sbam.BamFile(case(name).blob, path=name)
            held["name"] = name
        return held["g"]
    yield get
    if "g" in held:
        held["g"].close()


def check_checkers(g, c, R, x0, x1):
    """check_full_words (k_chains), check_full_counts (the list pass) and check_eager against the oracle, bit-exact."""
    from test_gpu_parity import pair_hist
    o = c.o
    w = c.words(R, x0, x1)
    on = (w & W_SUCC) != 0
    got = g.check_full_words(x0, x1, R)
    bad = np.flatnonzero(got != w)
    assert bad.size == 0, f"words: {bad.size} mismatches, first {bad[:5] + x0}: {got[bad[:5]]} vs {w[bad[:5]]}"
    counts, npos, rbe, nsucc = o.counts_range(x0, x1, R)
    cn, bits = g.check_full_counts(x0, x1, R, want_bitmap=True)
    assert np.array_equal(cn.totals, counts.sum(0))
    assert np.array_equal(cn.by_key[:3], counts[:3])
    assert np.array_equal(cn.positions, npos)
    assert np.array_equal(cn.reads_before_error, rbe)
    assert cn.n_success == nsucc
    assert np.array_equal(np.flatnonzero(bits), np.flatnonzero(on)), "check_full_counts bitmap"
    assert np.array_equal(cn.pair_hist, pair_hist(w))
    assert np.array_equal(np.flatnonzero(g.check_eager(x0, x1, R)), np.flatnonzero(on)), "check_eager"


def check_load(g, c, R, S, first, count, bitmap, x0=0, x1=None):
    """One load_records against the oracle's partitions, and its path against the predicate.  bitmap: what the device
    bitmap holds (False: not asked for); [x0, x1): the range the check covered."""
    import sbam
    from test_records import check_columns
    x1 = c.o.L if x1 is None else x1
    try:
        xs, xe, parts = expected_load(c, R, S, first, count)
    except RuntimeError:
        with pytest.raises(sbam.NoReadFoundException):
            g.load_records(S, first, count, reads_to_check=R, use_success_bitmap=bool(bitmap))
        return None
    if c.tail:  # RecordStream meets the end of the stream inside a record: UnexpectedEOF, on either path
        with pytest.raises(sbam.SbamError, match="UnexpectedEOF"):
            g.load_records(S, first, count, reads_to_check=R, use_success_bitmap=bool(bitmap))
        return None
    sizes, cols = g.load_records(S, first, count, reads_to_check=R, use_success_bitmap=bool(bitmap))
    assert sizes.tolist() == [len(p) for p in parts]
    check_columns(c.o, np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int64), cols)
    path = g.records_path()
    X0, X1 = min(xs), max(xe)
    tried = bool(bitmap) and X0 >= (x0 & ~63) and X1 <= x1
    assert path["tried"] == tried, path
    holds = tried and X0 >= x0 and proof_holds(c, R, X0, X1, x0, x1)
    assert path["proved"] == holds, (path, X0, X1)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("name,R", CASE_RS)
def test_decoy_stream(name, R, gpu_case, monkeypatch):
    import sbam
    c, g = case(name), gpu_case(name)
    o = c.o
    assert g.uncompressed_size == o.L
    check_checkers(g, c, R, 0, o.L)
    for bitmap in (False, "counts", "eager"):
        if bitmap == "counts":
            g.check_full_counts(0, o.L, R)
        elif bitmap == "eager":
            g.check_eager_device(0, o.L, R)
        for force in (False, True):
            if force:
                monkeypatch.setenv("SBAM_FORCE_PROOF", "1")
            else:
                monkeypatch.delenv("SBAM_FORCE_PROOF", raising=False)
            for S, first, count in c.all_loads():
                path = check_load(g, c, R, S, first, count, bitmap)
                if path is None or not bitmap:
                    continue
                # the list pass's own account of the whole-file check
                assert path["missing_links"] >= 0 and path["failed_fallbacks"] >= 0, path
                if c.clean:
                    assert path["missing_links"] == 0 and path["failed_fallbacks"] == 0, path
                    assert path["proved"]
                if c.broken:
                    assert path["missing_links"] > 0, path


# x1 of the checked range against the host of the "subrange" stream
X1_AT = ("record", "record+1", "before_decoy", "after_decoy", "target", "word_of_b_target")


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("x1_at", X1_AT)
@pytest.mark.parametrize("x0_at", ("zero", "unaligned"))
def test_checked_subrange(x0_at, x1_at, R, gpu_case):
    """check_full_counts / check_eager over [x0, x1) with x1 around a host and its decoy (k_p0_links' last-entry rule,
    walk_chain's `a < x1`), then loads whose splits lie inside the bitmap (tried) or reach past it (not tried)."""
    c, g = case("subrange"), gpu_case("subrange")
    m = c.meta
    h, d, t = m["host"], m["decoys"][1], m["targets"][1]
    assert m["targets"][0] == h + 3  # the kind-b decoy before the host hops to a point at or past x1 that is no record
    # what an earlier check left behind x1 must not be read: Success(0) sets every bit of the whole stream
    assert g.check_full_counts(0, c.o.L, reads_to_check=0).n_success == c.o.L
    x0 = 0 if x0_at == "zero" else m["records"][3] + 1
    # "word_of_b_target": x1 on the first bit of the word that holds the kind-b decoy's target, so that no position of
    # that word is checked and its bits are whatever the Success(0) check left
    tb = m["targets"][0]
    x1 = {"record": h, "record+1": h + 1, "before_decoy": d - 7, "after_decoy": d + 11, "target": t,
          "word_of_b_target": tb & ~63}[x1_at]
    assert m["decoys"][0] < (tb & ~63)
    assert t == m["host_end"] and x0 < m["records"][12]
    check_checkers(g, c, R, x0, x1)
    S = [int(c.o.start[i]) for i in (1, 2, 3)]  # the blocks that begin on records[12], the host and its end
    for bitmap in ("counts", "eager"):
        if bitmap == "counts":
            g.check_full_counts(x0, x1, R)
        else:
            g.check_eager_device(x0, x1, R)
        # split 0 ends on records[12]; splits 0-1 end on the host; splits 0-2 on its end; the whole file reaches L
        for load in ((S[0], 0, 1), (S[1], 0, 1), (S[2], 0, 1), (S[0], 1, 1), (WHOLE, 0, None)):
            check_load(g, c, R, *load, bitmap, x0, x1)


def test_subrange_loads_have_partitions():
    c = case("subrange")
    S = [int(c.o.start[i]) for i in (1, 2, 3)]
    b, a = c.meta["decoys"]
    assert [bool(c.succ(R)[b]) for R in RS] == [True, False, False, False, False] and all(c.succ(R)[a] for R in RS)
    assert not set(c.meta["decoys"]) & set(c.meta["records"])
    assert [int(c.o.uoff[i]) for i in (1, 2, 3)] == [c.meta["records"][12], c.meta["host"], c.meta["host_end"]]
    for R in RS:
        for load in ((S[0], 0, 1), (S[1], 0, 1), (S[2], 0, 1), (S[0], 1, 1), (WHOLE, 0, None)):
            xs, xe, parts = expected_load(c, R, *load)
            assert all(len(p) for p in parts)
        assert expected_load(c, R, S[1], 0, 1)[1] == [c.meta["host"]]
        assert expected_load(c, R, S[2], 0, 1)[1] == [c.meta["host_end"]]
