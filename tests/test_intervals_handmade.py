"""loadBamIntervals against a brute-force filter on hand-built, coordinate-sorted files with several references.

For a sorted file the answer of an interval query needs no index: every record whose [start, end) intersects the loci,
in file order.  `brute` computes that from the builder's own record list (never from the inflated stream or a library
call) by the rule include/sbam.h states for sbam_record_spans and CanLoadBam.region uses ([getStart - 1, getEnd)):
end = 0 for flag 4, else pos + the M/D/N/=/X lengths; kept when ref matches, pos < e and end > a.

Under that rule a mapped record of reference length 0 has the empty region [pos, pos): kept iff a < pos < e; a placed
unmapped record is never kept.  Whether the reference's LociSet.intersects agrees on the empty region cannot be pinned
(that library is not in the reference tree); the documented rule is kept.

The files: four references (one without reads, between two that have some, so that indices and names can drift apart),
records at the edges of the 16 kb windows and of the bins, every CIGAR op, CIGARs past 64 ops, reference skips over
many windows, placed unmapped records, records without coordinates, names and tag bytes of every length, BGZF blocks
of 37 to 9000 bytes.  The CPU tests pin sbam/bai.py and sbam_bai_assemble; the GPU tests pin load_bam_intervals with
all three sources of an index, and record_spans, record_offsets and _vpos_offset on their own."""
import functools
import random
import struct
from collections import namedtuple

import numpy as np
import pytest

from conftest import fixture_bytes
from test_bai_build import BIG, Walk, assemble_args, bgzf, cut, expected_refs, header, record, restate
from test_intervals import walk_spans

SEEDS = [1, 2]
REFS = (("chrA", BIG), ("empty", 5000), ("chrB", 3_000_000), ("chrC", 70_000))
NAMES = [n for n, _ in REFS]
EDGES = (1 << 14, 1 << 15, 1 << 17, 1 << 20)
STRIDES = (37, 700, 1500, 3000, 9000)
REF_OPS = "MDN=X"
NAME_CHARS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-."
DEFAULT_SPLIT = 32 << 20

Rec = namedtuple("Rec", "ref pos flag cigar end x size")  # end: the span's; x: stream offset; size: bytes with the length


# ---- the builder -------------------------------------------------------------------------------------------------
def _cigar(rng, kind):
    if kind == 0:
        return [(50, "M")]
    if kind == 1:
        return [(3, "S"), (20, "M"), (2, "I"), (5, "D"), (9, "N"), (7, "="), (4, "X"), (6, "H"), (1, "P")]
    if kind == 2:
        return [(10, "M"), (rng.choice((20000, 140000, 1 << 17)), "N"), (10, "M")]
    if kind == 3:
        return [(3, "S"), (1, "I")]
    if kind == 4:
        return []
    return [(1, "M")] * rng.randint(1, 89)


class Built:
    """One seeded file: .data (BGZF bytes), .recs (the record list in file order), .walk, .idx (restate(data))."""

    def __init__(self, seed):
        rng = random.Random(seed)
        plan = []  # (ref, pos, cigar, flag)
        for ref, (_, length) in enumerate(REFS):
            if ref == 1:
                continue
            room = min(length, 1 << 29) - 300000 if length > 400000 else length - 1000
            for _ in range(700):
                pos = rng.randrange(min(room, 1 << 21)) if rng.random() < 0.5 else rng.randrange(room)
                kind = rng.randrange(6)
                plan.append((ref, pos, _cigar(rng, kind), 4 if kind == 4 else 0))
            for e in EDGES:
                if e + 1 < room:
                    plan += [(ref, e + d, [(50, "M")], 0) for d in (-60, -50, -1, 0, 1)]
        plan.append((0, -1, [(50, "M")], 0))
        plan = [(r, p, c, f | 4 if rng.random() < 0.05 else f) for r, p, c, f in plan]
        plan.sort(key=lambda t: (t[0], t[1]))  # (stable: ties keep their drawn order)
        plan += [(-1, -1, [], 4)] * 15
        h = header(REFS)
        parts, self.recs, x = [h], [], len(h)
        for ref, pos, cigar, flag in plan:
            name = "".join(rng.choice(NAME_CHARS) for _ in range(rng.randint(1, 254))).encode()
            b = record(ref, pos, cigar, flag=flag, name=name, pad=rng.randrange(300))
            end = 0 if flag & 4 else pos + sum(n for n, op in cigar if op in REF_OPS)
            self.recs.append(Rec(ref, pos, flag, cigar, end, x, len(b)))
            parts.append(b)
            x += len(b)
        self.u = b"".join(parts)
        at, c = [], 0
        while True:
            c += rng.choice(STRIDES)
            if c >= len(self.u):
                break
            at.append(c)
        self.data = bgzf(cut(self.u, at))
        self.walk = Walk(self.data)
        assert self.walk.u == self.u
        self.idx = restate(self.data)
        self.starts = np.array([r.x for r in self.recs], np.int64)
        self.vpos = [self.walk.vpos(r.x) for r in self.recs]
        self.loci = fixed_loci(self.recs) + random_loci(random.Random(1000 + seed), self.recs, REFS, 150)


@functools.lru_cache(maxsize=None)
def built(seed):
    return Built(seed)


# ---- the reference -----------------------------------------------------------------------------------------------
def brute(records, names, loci):
    """Indices into `records` of those kept for `loci` = [(contig, a, e or None)], in file order."""
    want = [(names.index(c), a, float("inf") if e is None else e) for c, a, e in loci if c in names]
    return [i for i, r in enumerate(records) if any(r.ref == ri and r.pos < e and r.end > a for ri, a, e in want)]


def loci_text(loci):
    return ",".join(c if e is None else f"{c}:{a}-{e}" for c, a, e in loci)


def to_query(names, loci):
    """htsjdk's 1-based closed intervals (an open end is 0), an unknown contig as reference -1."""
    return [(names.index(c) if c in names else -1, a + 1, 0 if e is None else e) for c, a, e in loci]


# ---- the loci ----------------------------------------------------------------------------------------------------
def fixed_loci(recs):
    past = max(max(r.pos, r.end) for r in recs if r.ref == 2) + 1000
    return [
        [("chrA", 0, None)],
        [("empty", 0, None)],
        [("nope", 0, None)],
        [("nope", 10, 5000), ("chrC", 100, 5000)],
        [("chrC", 0, 70000), ("chrB", 0, None)],          # two references, out of file order
        [("chrB", past, past + 5000)],                     # behind the last record of chrB
        [("chrA", 1000, 40000), ("chrA", 20000, 100000)],  # overlapping
    ]


def random_loci(rng, recs, refs, n_sets):
    """n_sets sets of 1 to 3 loci that start 50 or 1 before, at or 1 behind a record's pos, a record's end, a 16 kb
    window's edge or a random place, and are 1, 2, 50, 16384 or 200000 long."""
    names = [n for n, _ in refs]
    by_ref = {}
    for r in recs:
        if r.ref >= 0:
            by_ref.setdefault(r.ref, []).append(r)
    out = []
    for _ in range(n_sets):
        one = []
        for _ in range(rng.choice((1, 1, 2, 3))):
            ref = rng.choice(sorted(by_ref))
            length = refs[ref][1]
            how = rng.randrange(4)
            if how == 0:
                x = rng.choice(by_ref[ref]).pos
            elif how == 1:
                x = rng.choice(by_ref[ref]).end
            elif how == 2:
                x = 16384 * rng.randrange(length // 16384 + 1)
            else:
                x = rng.randrange(length)
            a = max(0, x + rng.choice((-50, -1, 0, 1)))
            one.append((names[ref], a, a + rng.choice((1, 2, 50, 16384, 200000))))
        out.append(one)
    return out


def test_brute_on_a_tiny_list():
    """The reference itself, by hand: edges of [pos, end), the empty region, flag 4, an unknown contig, file order."""
    R = lambda ref, pos, end: Rec(ref, pos, 0, None, end, 0, 0)  # noqa: E731
    recs = [R(0, 10, 20), R(0, 15, 15), R(0, 15, 0), R(2, 10, 20), R(-1, -1, 0)]
    names = ["a", "b", "c"]
    assert brute(recs, names, [("a", 19, 25)]) == [0] and brute(recs, names, [("a", 20, 25)]) == []
    assert brute(recs, names, [("a", 0, 11)]) == [0] and brute(recs, names, [("a", 0, 10)]) == []
    assert brute(recs, names, [("a", 14, 16)]) == [0, 1] and brute(recs, names, [("a", 15, 16)]) == [0]
    assert brute(recs, names, [("a", 14, 15)]) == [0], "the empty region [15, 15) needs a < 15 < e"
    assert brute(recs, names, [("c", 0, None), ("a", 0, None)]) == [0, 1, 3]
    assert brute(recs, names, [("b", 0, None)]) == [] and brute(recs, names, [("zz", 0, None)]) == []


# ---- CPU: the file is what it claims -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_file_is_what_it_claims(seed):
    import oracle
    f = built(seed)
    assert len(f.u) < 1 << 20
    per_ref = [sum(r.ref == k for r in f.recs) for k in range(4)]
    assert per_ref[1] == 0 and min(per_ref[0], per_ref[2], per_ref[3]) >= 700 and sum(r.ref < 0 for r in f.recs) == 15
    assert max(len(r.cigar) for r in f.recs) > 64
    assert any(r.pos == -1 and r.ref == 0 for r in f.recs)
    assert any(r.flag & 4 and r.ref >= 0 and r.cigar for r in f.recs), "no placed unmapped record with a CIGAR"
    assert any(not r.flag & 4 and r.end == r.pos for r in f.recs), "no mapped record of reference length 0"
    o = oracle.BamFile(f.data)
    assert o.L == len(f.u)
    ok = np.flatnonzero(o.check_full_range(0, o.L) & oracle.W_SUCCESS)
    assert np.array_equal(ok, f.starts), "every record start is Success and nothing else is"
    for split in (1 << 40, 8000):
        _, parts = oracle.compute_splits(o, split)
        assert np.array_equal(np.concatenate(parts), f.starts), f"split size {split}"
    idx = f.idx
    assert idx["n_unsorted"] == 0 and idx["n_records"] == len(f.recs) and idx["n_no_coor"] == 15
    assert idx["n_ref"] == 4 and sorted(idx["meta"]) == [0, 2, 3]
    levels = {next(lv for lv in range(6) if ((1 << 3 * lv) - 1) // 7 <= r[1] < ((1 << 3 * lv + 3) - 1) // 7)
              for r in idx["runs"]}
    assert len(levels) >= 3
    assert any(max(r.pos, 0) >> 14 < (r.end - 1) >> 14 for r in f.recs if not r.flag & 4 and r.end > r.pos)
    w = f.walk
    assert any(w.vpos(r.x) >> 16 != w.vpos(r.x + r.size - 1) >> 16 for r in f.recs), "no record crosses a block"
    assert any(w.vpos(r.x) & 0xffff for r in f.recs)


@pytest.mark.parametrize("seed", SEEDS)
def test_loci_hit_and_miss(seed):
    f = built(seed)
    assert len(f.loci) == 7 + 150
    kept = [len(brute(f.recs, NAMES, loci)) for loci in f.loci]
    assert sum(k > 0 for k in kept[7:]) >= 75 and sum(k == 0 for k in kept[7:]) >= 10
    assert kept[0] == sum(r.ref == 0 and not r.flag & 4 and (r.end > 0) for r in f.recs) > 500
    assert kept[1] == kept[2] == kept[5] == 0 and kept[3] > 0 and kept[4] > 1000 and kept[6] > 0


# ---- CPU: the host chain -------------------------------------------------------------------------------------------
def _refs_assembled(idx):
    import sbam
    from sbam import bai
    return bai.parse_bai(sbam.bai_assemble(*assemble_args(idx)))


def _refs_restated(idx):
    from sbam import bai
    return [bai.Reference({b: [bai.Chunk(*c) for c in cs] for b, cs in bins.items()}, list(io))
            for bins, io in expected_refs(idx)]


def check_host_chain(recs, vpos, names, refs, loci_sets):
    """file_span's chunks, the records that start inside them and the span rule give brute's records, each once."""
    from sbam import bai
    v = np.array(vpos, np.uint64)
    for loci in loci_sets:
        chunks = bai.file_span(refs, to_query(names, loci))
        got = []
        for c in chunks:
            lo, hi = np.searchsorted(v, np.uint64(c.start)), np.searchsorted(v, np.uint64(c.end))
            got += range(int(lo), int(hi))
        assert got == sorted(set(got)), f"{loci_text(loci)}: a record lies in two chunks, or the chunks are unordered"
        inside = set(brute(recs, names, loci))
        assert [i for i in got if i in inside] == sorted(inside), loci_text(loci)


@pytest.mark.parametrize("source", ["assembled", "restated"])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_chain(seed, source):
    f = built(seed)
    assert f.vpos == sorted(f.vpos)
    refs = (_refs_assembled if source == "assembled" else _refs_restated)(f.idx)
    assert len(refs) == 4 and not refs[1].bins and not refs[1].ioffsets
    check_host_chain(f.recs, f.vpos, NAMES, refs, f.loci)


@pytest.mark.parametrize("seed", SEEDS)
def test_partitions(seed):
    from sbam import bai
    f = built(seed)
    refs = _refs_restated(f.idx)
    whole = bai.file_span(refs, to_query(NAMES, [(n, 0, None) for n in NAMES]))
    assert len(whole) == 1, "a whole-file query of a sorted file is one chunk"
    spread = [(NAMES[r.ref], r.pos, r.pos + 50) for r in f.recs[::150] if r.ref >= 0]
    _check_groups([c.size() for c in whole])
    assert _check_groups([c.size() for c in bai.file_span(refs, to_query(NAMES, spread))]) >= 3


def _check_groups(costs):
    from sbam import bai
    for cap in (1, 5000, 1 << 40):
        groups = bai.capped_cost_groups(costs, float(cap))
        assert [i for g in groups for i in g] == list(range(len(costs)))
        assert all(g for g in groups)
        assert all(len(g) == 1 or sum(costs[i] for i in g) <= cap for g in groups)
        for g, nxt in zip(groups, groups[1:]):  # (greedy: the next chunk did not fit)
            assert sum(costs[i] for i in g) + costs[nxt[0]] > cap
    assert len(bai.capped_cost_groups(costs, float(1 << 40))) == 1
    assert len(bai.capped_cost_groups(costs, 1.0)) == len(costs)
    return len(costs)


# ---- GPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_built():
    import sbam
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sbam.BamFile(built(seed).data, path=f"handmade{seed}.bam")
        return cache[seed]
    yield get
    for g in cache.values():
        g.close()


def check_end_to_end(g, offsets, recs, names, loci_sets, indexes, split):
    """load_bam_intervals with every index of `indexes` keeps exactly brute's records, in file order."""
    from sbam import bai
    kw = {} if split is None else {"split_size": split}
    most = 0
    for loci in loci_sets:
        text = loci_text(loci)
        want = offsets[brute(recs, names, loci)]
        first = None
        for label, index in indexes:
            chunks, parts = g.load_bam_intervals(index, text, **kw)
            got = np.concatenate(parts) if parts else np.zeros(0, np.int64)
            assert np.array_equal(got, want), f"{text} with the {label} index"
            groups = bai.capped_cost_groups([c.size(3.0) for c in chunks], float(split or DEFAULT_SPLIT))
            assert len(parts) == len(groups), f"{text} with the {label} index"
            first = chunks if first is None else first
            assert chunks == first, f"{text}: the chunks of the {label} index differ from the first index's"
            most = max(most, len(parts))
    return most


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, 5000])
@pytest.mark.parametrize("seed", SEEDS)
def test_end_to_end(seed, split, gpu_built):
    import sbam
    f, g = built(seed), gpu_built(seed)
    indexes = [("GPU-built (bai=None)", None), ("build_bai()", g.build_bai()),
               ("host-assembled", sbam.bai_assemble(*assemble_args(f.idx)))]
    most = check_end_to_end(g, f.starts, f.recs, NAMES, f.loci, indexes, split)
    assert most == 1 if split is None else most > 2, "the small split size cuts some query into several partitions"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_end_to_end_on_fixtures(name, gpu_files):
    """40 random loci sets from the fixture's own records (a zlib-and-struct walk), with its .bai and with bai=None."""
    data = fixture_bytes(name)
    refs, spans = walk_spans(Walk(data).u)
    names = [n for n, _ in refs]
    recs = [Rec(ref, pos, 0, None, end, x, 0) for x, ref, pos, end in spans]
    loci = [[(names[0], 0, None)]] + random_loci(random.Random(7), recs, refs, 40)
    kept = [len(brute(recs, names, s)) for s in loci]
    assert sum(k > 0 for k in kept) >= 20
    offsets = np.array([r.x for r in recs], np.int64)
    indexes = [("fixture's", fixture_bytes(name + ".bai")), ("GPU-built (bai=None)", None)]
    check_end_to_end(gpu_files(name), offsets, recs, names, loci, indexes, None)


# record_spans against plain Python
def raw_record(ref, pos, ops=(), flag=0, name=b"read", n_cigar=None, block_size=None):
    """A record from raw CIGAR words (any op code), without bases or tags; n_cigar and block_size override the claims."""
    nc = len(ops) if n_cigar is None else n_cigar
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 30, 4680, nc, flag, 0, -1, -1, 0)
    body += name + b"\0" + struct.pack(f"<{len(ops)}I", *ops)
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def i32_wrap(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def py_span(u, x):
    """sbam_record_spans' rule (include/sbam.h) on stream bytes: the ops wholly inside the stream count."""
    L = len(u)
    if x < 0 or x + 36 > L:
        return (-1, -1, 0)
    ref, pos = struct.unpack_from("<ii", u, x + 4)
    lrn, nc, flag = u[x + 12], *struct.unpack_from("<HH", u, x + 16)
    c, rlen = x + 36 + lrn, 0
    for _ in range(nc):
        if c + 4 > L:
            break
        op, = struct.unpack_from("<I", u, c)
        rlen += op >> 4 if (op & 15) in (0, 2, 3, 7, 8) else 0
        c += 4
    return (ref, pos, 0 if flag & 4 else i32_wrap(pos + rlen))


def span_cases():
    """[(record bytes, expected (ref, start, end))]; the last one's CIGAR is cut off by the stream's end."""
    M = 0
    cases = []
    for t in range(16):  # each op code alone: 0-8 are M I D N S H P = X, 9-15 are none and contribute nothing
        cases.append((raw_record(0, 1000 + t, [(7 + t) << 4 | t]), (0, 1000 + t, 1000 + t + (7 + t if t in (0, 2, 3, 7, 8) else 0))))
    for nc in (0, 1, 64, 65, 65535):
        cases.append((raw_record(1, 2000, [1 << 4 | M] * nc), (1, 2000, 2000 + nc)))
    cases.append((raw_record(0, 3000, [3 << 4 | 4, 1 << 4 | 1]), (0, 3000, 3000)))       # 3S 1I: end == pos
    cases.append((raw_record(0, 3100, [50 << 4 | M], flag=4), (0, 3100, 0)))             # unmapped with a CIGAR
    cases.append((raw_record(0, 3200, [50 << 4 | M], flag=0x4 | 0x10 | 0x400), (0, 3200, 0)))
    cases.append((raw_record(0, 3300, [50 << 4 | M], flag=0xfffb), (0, 3300, 3350)))     # every flag but 4
    cases.append((raw_record(0, -1, [50 << 4 | M]), (0, -1, 49)))
    cases.append((raw_record(-1, -1, [], flag=4), (-1, -1, 0)))
    cases.append((raw_record(0, 4000, [20 << 4 | M], name=b"n"), (0, 4000, 4020)))
    cases.append((raw_record(0, 4100, [20 << 4 | M], name=b"n" * 254), (0, 4100, 4120)))
    cases.append((raw_record(0, (1 << 29) - 100, [100 << 4 | M]), (0, (1 << 29) - 100, 1 << 29)))
    cases.append((raw_record(0, 5000, [((1 << 28) - 1) << 4 | 2, ((1 << 28) - 1) << 4 | 7]), (0, 5000, 5000 + (1 << 29) - 2)))
    # sixteen N of 2^28 - 1: the reference length 2^32 - 16 passes 2^31; htsjdk's getAlignmentEnd adds in Java int
    # arithmetic, so the expected end is pos + rlen reduced to a signed 32-bit value
    cases.append((raw_record(0, 6000, [((1 << 28) - 1) << 4 | 3] * 16), (0, 6000, i32_wrap(6000 + 16 * ((1 << 28) - 1)))))
    assert cases[-1][1][2] == 6000 - 16
    # ten ops claimed, three and a half in the stream
    cut_off = raw_record(2, 7000, [11 << 4 | M] * 4, n_cigar=10, block_size=500)[:-2]
    cases.append((cut_off, (2, 7000, 7033)))
    return cases


@pytest.fixture(scope="module")
def span_stream():
    import sbam
    cases = span_cases()
    h = header((("chr1", BIG), ("chr2", BIG), ("chr3", BIG)))
    offs, x = [], len(h)
    for b, _ in cases:
        offs.append(x)
        x += len(b)
    u = h + b"".join(b for b, _ in cases)
    data = bgzf(cut(u, range(60000, len(u), 60000)))
    with sbam.BamFile(data, path="spans.bam") as g:
        assert g.uncompressed_size == len(u)
        yield g, u, np.array(offs, np.int64), [e for _, e in cases]


def _spans(g, offs):
    return [tuple(t) for t in zip(*(a.tolist() for a in g.record_spans(np.asarray(offs, np.int64))))]


@pytest.mark.gpu
def test_record_spans_cases(span_stream):
    g, u, offs, want = span_stream
    assert [py_span(u, int(x)) for x in offs] == want, "the Python rule and the cases' hand-written spans"
    assert _spans(g, offs) == want


@pytest.mark.gpu
def test_record_spans_stream_end(span_stream):
    import sbam
    g, u, offs, want = span_stream
    L = len(u)
    assert L == offs[-1] + 4 + 32 + 5 + 14, "the last record ends two bytes into its fourth op"
    xs = [L - 36, L - 35, -1, L, L + 1000, -(1 << 40), int(offs[-1])]
    exp = [py_span(u, x) for x in xs]
    assert exp[1:6] == [(-1, -1, 0)] * 5 and exp[0] != (-1, -1, 0) and exp[6] == (2, 7000, 7033)
    assert _spans(g, xs) == exp
    # a bare 36-byte record head as the stream's last bytes: x + 36 == L, its five claimed ops lie behind the stream
    h = header()
    head = raw_record(0, 777, [], n_cigar=5, block_size=100)[:36]
    v = h + raw_record(0, 500, [50 << 4]) + head
    with sbam.BamFile(bgzf([v]), path="head.bam") as f:
        got = _spans(f, [len(h), len(v) - 36, len(v) - 35])
    assert got == [(0, 500, 550), (0, 777, 777), (-1, -1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_record_spans_batches(n, span_stream):
    g, u, offs, want = span_stream
    rng = random.Random(n)
    pick = [rng.randrange(len(offs)) for _ in range(n)]  # unsorted, with repeats
    assert n < 255 or len(set(pick)) < n
    got = g.record_spans(offs[pick])
    assert all(a.size == n for a in got)
    assert _spans(g, offs[pick]) == [want[i] for i in pick]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_record_spans_of_the_built_file(seed, gpu_built):
    f, g = built(seed), gpu_built(seed)
    assert _spans(g, f.starts) == [(r.ref, r.pos, r.end) for r in f.recs]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_record_offsets_at_chunk_edges(seed, gpu_built):
    f, g = built(seed), gpu_built(seed)
    rng = random.Random(50 + seed)
    L, st = len(f.u), f.starts
    pairs = []
    for k in range(30):
        i = rng.randrange(len(st))
        j = rng.randrange(i, len(st))
        pairs.append((int(st[i]), (int(st[j]), int(st[j]) + 1, int(st[j]) - 1, L)[k % 4]))
    x0 = int(st[len(st) // 2])
    pairs += [(x0, L + 1), (x0, L + (1 << 20)), (x0, x0), (x0, x0 + 1), (int(st[0]), L), (int(st[-1]), L)]
    for a, e in pairs:
        want = st[(st >= a) & (st < e)]
        assert np.array_equal(g.record_offsets(a, e), want), (a, e)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_vpos_offset(seed, gpu_built):
    import sbam
    f, g = built(seed), gpu_built(seed)
    w, L = f.walk, len(f.u)
    assert len(w.start) > 100
    for b, start in enumerate(w.start):
        usize = w.uoff[b + 1] - w.uoff[b]
        assert g._vpos_offset(start << 16) == w.uoff[b]
        assert g._vpos_offset(start << 16 | usize) == w.uoff[b + 1], "a block's end is the next block's first byte"
        assert g._vpos_offset(start << 16 | usize // 2) == w.uoff[b] + usize // 2
        nxt = w.start[b + 1] if b + 1 < len(w.start) else w.end_addr
        for inside in (start + 1, nxt - 1):  # (also in the last block, whose end is the EOF marker's address)
            with pytest.raises(sbam.SbamError):
                g._vpos_offset(inside << 16)
    for addr in (w.end_addr, w.end_addr + 1, w.end_addr + 28, len(f.data), len(f.data) + 1000):
        assert g._vpos_offset(addr << 16) == L
    for r, v in zip(f.recs[::97], f.vpos[::97]):
        assert g._vpos_offset(v) == r.x
