"""A context opened on a byte range of a file (a shard: sbam_open with base_offset + len < file_size) answers, at every
position, for every count, record search and partition, either what the whole file answers or HALO — never a verdict
that the bytes behind its last one could change.  GpuShard.run, the streamed benchmark and LazyBlockChecker retry on
HALO and on nothing else.

The shards are byte ranges blob[lo:hi] of one file whose stream is U; a shard's stream is U[a:b) with b on an exact
byte: the file is written as stored BGZF members whose payloads end on every wanted cut.  The cuts walk through a probe
record P (fixed fields, name, 70 CIGAR ops, sequence, qualities, aux tail, and the record behind it); P is placed so
that b falls on chosen bytes of the record-0 pass's 8 KiB tiles; further families put b behind the chain pass's first
chunk and around decoys (tests/record_stream_writer.py).

Expected values are the CPU oracle's window forms (oracle.check_full_window and its kin) on the slice o.u[a:b] of the
whole file's stream: the word and whether its evaluation tested a byte past the window (hit).  hit means HALO; anything
else is bit-exact.  The tests without the gpu mark check the inputs with the oracle alone: a non-hit window word is the
whole file's word, every shard has hit positions whose window verdict differs from the whole file's (so a kernel that
forgets HALO is caught by value), and every cut lies in the field its name says."""
import ctypes
import functools

import numpy as np
import pytest

import bgzf_writer as bw
import record_stream_writer as rw

W_SUCC, W_HALO = 0x80000000, 0x00800000
ERR_HALO = 9
TILE, CHUNK = 8192, 131072  # the record-0 pass's tile and the chain pass's chunk, in stream positions
RS = (1, 2, 10)

# ---- the probe record ---------------------------------------------------------------------------------------------
LRN, NOPS, LSEQ, AUX = 20, 70, 50, 40  # 70 ops: past the 64 that eager_pass_win reads per lane
O_NAME, O_OPS = 36, 36 + LRN
O_SEQ = O_OPS + 4 * NOPS
O_QUAL = O_SEQ + (LSEQ + 1) // 2
O_AUX = O_QUAL + LSEQ
P_SIZE = O_AUX + AUX
# (d, the field that holds the first byte the shard lacks): the shard's stream ends at P + d
CUTS = ([(0, "block_size"), (1, "block_size"), (3, "block_size"), (4, "fixed"), (35, "fixed"), (36, "name"), (37, "name"),
         (O_NAME + LRN - 1, "name"), (O_OPS, "cigar"), (O_OPS + 1, "cigar"), (O_OPS + 2, "cigar"), (O_OPS + 3, "cigar"),
         (O_OPS + 4, "cigar"), (O_OPS + 4 * 64, "cigar"), (O_SEQ - 1, "cigar"), (O_SEQ, "seq"), (O_SEQ + 12, "seq"),
         (O_QUAL + 25, "qual"), (P_SIZE - 1, "aux"), (P_SIZE, "next"), (P_SIZE + 1, "next"), (P_SIZE + 35, "next"),
         (P_SIZE + 36, "next")])
B_MODS = (1, 36, 767, 768, 769, 4096, 8191, 0)  # b mod TILE (768: the tile kernel's staged halo)
PREAMBLE = (38, 44, 38, 51, 38, 38, 60, 38, 47, 38, 38, 55)  # the 12 records before P


def probe() -> bytes:
    r = rw.record(ref_id=0, pos=5, name=b"probe/read:0123456."[:LRN - 1], flag=0, cigar=[(3 << 4) | (i % 3) for i in range(NOPS)],
                  seq=b"\x12" * ((LSEQ + 1) // 2), qual=b"\x21" * LSEQ, aux=rw.filler(AUX))
    assert len(r) == P_SIZE
    return r


def field_of(u: bytes, p: int, x: int) -> str:
    """The field of the record at p that holds stream byte x, read from the record's own lengths."""
    lrn, nc = u[p + 12], int.from_bytes(u[p + 16:p + 18], "little")
    ls, bs = int.from_bytes(u[p + 20:p + 24], "little"), int.from_bytes(u[p:p + 4], "little")
    edges = [(4, "block_size"), (36, "fixed"), (36 + lrn, "name"), (36 + lrn + 4 * nc, "cigar")]
    edges += [(edges[-1][0] + (ls + 1) // 2, "seq")]
    edges += [(edges[-1][0] + ls, "qual"), (4 + bs, "aux")]
    for end, name in edges:
        if x - p < end:
            return name
    return "next"


# ---- streams and shards -------------------------------------------------------------------------------------------
def body(s, n, i0=0):
    for i in range(i0, i0 + n):
        s.add(rw.sized(44 + (i * 7) % 23))


def cut_file(u: bytes, cuts) -> bytes:
    """`u` as stored members that begin at the stream offsets in `cuts` (and at 0), then the EOF marker."""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(u))) + [len(u)]
    out = []
    for x, y in zip(edges, edges[1:]):
        while y - x > 60000:
            out.append(bw.stored_block(u[x:x + 60000]))
            x += 60000
        out.append(bw.stored_block(u[x:y]))
    return b"".join(out) + bw.eof_marker()


class World:
    """One file: the stream, its members, the whole file's oracle answers."""

    def __init__(self, u, meta, edges, b, **kw):
        import oracle
        self.u, self.meta, self.b, self.info = u, meta, b, kw
        near = max(x for x in meta["records"] if x <= b - 60)  # a member that starts on a record shortly before the cut
        self.blob = cut_file(u, list(edges) + [near, b])
        self.o = oracle.BamFile(self.blob)
        assert self.o.L == len(u)
        self.lens = self.o.lens[:self.o.nref].copy()
        self.e2, self.e3, self.e4 = edges[1], edges[2], edges[3]
        self._w = {}

    def words(self, R):
        if R not in self._w:
            self._w[R] = self.o.check_full_range(0, self.o.L, R)
        return self._w[R]

    def block_of(self, x):
        i = int(np.searchsorted(self.o.uoff, x))
        assert int(self.o.uoff[i]) == x, x
        return i


class Shard:
    """blob[lo:hi] of a world, whose stream is U[a:b)."""

    def __init__(self, world, kind):
        self.w, self.kind = world, kind
        o = world.o
        i0 = 0 if kind == "prefix" else world.block_of(world.e2)  # mid-file: from the third member on
        i1 = world.block_of(world.b)
        self.i0, self.i1 = i0, i1
        self.lo, self.hi = int(o.start[i0]), int(o.start[i1])
        self.a, self.b = int(o.uoff[i0]), world.b
        self.L = self.b - self.a
        self.win = o.u[self.a:self.b]
        self._f, self._e, self._l = {}, {}, {}

    def full(self, R):
        import oracle
        if R not in self._f:
            self._f[R] = oracle.check_full_window(self.win, self.w.lens, R)
        return self._f[R]

    def eager(self, R):
        import oracle
        if R not in self._e:
            self._e[R] = oracle.check_eager_window(self.win, self.w.lens, R)
        return self._e[R]

    def expect_words(self, R):
        w, h = self.full(R)
        return np.where(h, np.uint32(W_HALO), w)

    def find(self, x0w, R, mrs=10_000_000):
        import oracle
        return oracle.find_record_start_window_eager(self.win, self.w.lens, x0w, R, mrs)

    def member_starts(self):
        """(file offset, window offset) of every member of the shard."""
        o = self.w.o
        return [(int(o.start[i]), int(o.uoff[i]) - self.a) for i in range(self.i0, self.i1)]

    # loads: Hadoop splits of the whole file, of the size that puts a split's start on the mid-file shard's first byte
    @property
    def S(self):
        return int(self.w.o.start[self.w.block_of(self.w.e2)])

    def loads(self):
        """(first split, count) for: the splits that end before the member e3 (far before the cut: behind them no chain
        leaves the shard, so a bitmap covers them), those that end before the member eight records before the cut, the
        splits that lie inside the shard's bytes (what a ShardPlan whose halo ends at hi owns), and one split more."""
        import oracle
        S, o = self.S, self.w.o
        first = self.lo // S
        owned = self.hi // S - first
        safe = int(o.start[self.w.block_of(self.w.e4)]) // S - first
        pre = int(o.start[self.w.block_of(self.w.e3)]) // S - first
        assert 0 < pre <= safe <= owned
        sp = oracle.hadoop_splits(o.D, S)
        # (a split whose first block lies behind the shard's last one is no split of this shard's)
        inside = [o.block_index_at_or_after(o.find_block_start(s)) < self.i1 for s, _ in sp[first:first + owned + 1]]
        n_in = inside.index(False) if False in inside else len(inside)
        return [(first, n) for n in sorted({pre, safe, min(owned, n_in), min(owned + 1, n_in)})]

    def expected_load(self, R, first, count):
        """The partitions (whole-stream record offsets) of splits [first, first + count), or oracle.HALO."""
        if (R, first, count) not in self._l:
            self._l[R, first, count] = self._expected_load(R, first, count)
        return self._l[R, first, count]

    def _expected_load(self, R, first, count):
        import oracle
        o = self.w.o
        sp = oracle.hadoop_splits(o.D, self.S)[first:first + count]
        assert len(sp) == count
        parts, xs, xe = [], [], []
        for s, e in sp:
            i = o.block_index_at_or_after(o.find_block_start(s))
            assert self.i0 <= i < self.i1, "the split's first block lies outside the shard"
            x = self.find(int(o.uoff[i]) - self.a, R)
            if x == oracle.HALO:
                return oracle.HALO
            assert x is not None
            j = o.block_index_at_or_after(e)
            if j < self.i1:
                end = int(o.uoff[j]) - self.a
            elif self.hi >= e:  # the block at or past the split's end is the one behind the shard's last
                end = self.L
            else:
                return oracle.HALO
            chain, hit = oracle.record_chain_window(self.win, x, end)
            if hit:
                return oracle.HALO
            whole = o.record_chain(self.a + x, o.x_end_of(e))
            assert np.array_equal(chain + self.a, whole), "a window answer that is not the whole file's"
            parts.append(whole)
            xs.append(x)
            xe.append(end)
        return parts, min(xs), max(xe)


def cut_world(m, d):
    """P placed so that (P + d) mod TILE == m, in the second or third tile of a stream three tiles long."""
    s = rw.Stream()
    body(s, 6)
    P = TILE + (m - d) % TILE
    if P + d < TILE + 1024:  # (room for the preamble, and b past the first tile's staged halo)
        P += TILE
    pre = P - sum(PREAMBLE)
    s.fill_to(pre, big=1500)
    e3 = s.records[-1] + 11  # inside the last filler record
    for n in PREAMBLE:
        s.add(rw.sized(n))
    e4 = s.records[-8]
    assert len(s) == P
    s.add(probe())
    body(s, 12, 3)
    s.fill_to(3 * TILE + 100, big=1500)
    u, meta = s.finish()
    meta["P"] = P
    # (P - 5: a member from which P is the first position that is Success or unknown, whatever R is)
    edges = [meta["records"][2], meta["records"][4] + 7, e3, e4, P - 5]
    return World(u, meta, edges, P + d, P=P, d=d)


def chunk_world(past):
    """A stream just over one chain chunk, cut `past` bytes behind the chunk's edge."""
    s = rw.Stream()
    body(s, 6)
    s.fill_to(CHUNK - 700, big=300)
    e3 = s.records[-1] + 11
    for n in PREAMBLE:
        s.add(rw.sized(n))
    e4 = s.records[-8]
    s.fill_to(CHUNK - 20, big=0)
    body(s, 30, 5)
    u, meta = s.finish()
    return World(u, meta, [meta["records"][2], meta["records"][4] + 7, e3, e4], CHUNK + past)


def decoy_world(kind):
    """hop_past: a decoy that is Success in the whole file, the cut between it and its hop target (its host's end).
    hop_on_b: the cut on that target.  before_true: a decoy 120 bytes before a true record T; the decoy hops to a true
    record far behind the cut, T's own chain ends before the cut, and a member starts between the host and the decoy.
    straddle: a 1500-byte true record that the cut halves."""
    s = rw.Stream()
    body(s, 6)
    s.fill_to(TILE + 3000, big=1500)
    e3 = s.records[-1] + 11
    for n in PREAMBLE:
        s.add(rw.sized(n))
    e4 = s.records[-8]
    extra = []
    if kind in ("hop_past", "hop_on_b"):
        h, ds = s.host(at=10, pad=60)
        b = len(s) - (30 if kind == "hop_past" else 0)
        body(s, 14, 2)
    elif kind == "before_true":
        h, ds = s.host(at=60, pad=120 - rw.TINY)
        extra = [ds[0] - 20]
        body(s, 14, 2)
        b = len(s) + 500
    else:
        ds = []
        b = len(s) + 700
    s.fill_to(3 * TILE + 100, big=1500)
    if kind == "before_true":
        far = next(x for x in s.records if x > b + 2000)
        s._patch(ds[0], far)
        s.targets[0] = far
    u, meta = s.finish()
    w = World(u, meta, [meta["records"][2], meta["records"][4] + 7, e3, e4] + extra, b, kind=kind)
    return w


# 16 bytes that read as a record's fixed fields at every 16th byte: block_size = flag_nc = 0x40000 (unmapped, no
# ops, a hop of 256 KiB), refID = l_seq = 65, pos = next_refID = -1, bin_mq_nl = next_pos = 2, and the name, 36 bytes
# on, is "A\0".  Record 0 passes there, so a run of them is denser in PASS0 positions than any run of true records.
DENSE = bytes.fromhex("00000400" "41000000" "ffffffff" "02000000")
DENSE_N = 11264


def dense_world():
    """A host record whose aux tail holds DENSE_N PASS0 positions, 16 bytes apart, each hopping past the cut (and past
    the file's end): more PASS0 positions than the list-form chain pass takes (positions / 32 + 4096), so the counts
    and the eager check run k_chains, two list rounds in the first chunk, and every one of those chains is unknown."""
    s = rw.Stream(contig_lengths=(1000,) * 100)
    body(s, 6)
    for _ in range(16):  # (some splits of the mid-file shard end before the host)
        s.add(rw.sized(300))
    e3 = s.records[-1] + 11
    s.add(rw.record(aux=DENSE * DENSE_N))
    for n in PREAMBLE:
        s.add(rw.sized(n))
    e4 = s.records[-8]
    body(s, 8, 2)
    b = s.add(rw.sized(300)) + 150
    body(s, 12, 5)
    u, meta = s.finish()
    return World(u, meta, [meta["records"][2], meta["records"][4] + 7, e3, e4], b, dense=True)


INTERIOR_TAIL = 262144 + 512  # sbam_check.hip's kInteriorTail: a tile that ends this far before L is "interior"
REACH = 36 + 255 + 4 * 65535  # the farthest byte record 0 can read: fixed fields, a 255-byte name, 65535 ops


def long_world():
    """A prefix shard of L = 3 tiles + INTERIOR_TAIL, so that its first three tiles run in the interior kernels
    (k_check_bits, k_eager_wave, k_check's INTERIOR arm), which have no end-of-stream test.  The cut halves a host
    record whose aux tail is zeros (valid CIGAR ops) with three planted positions of l_read_name = 255 and
    n_cigar_op = 65535: q1 on the last byte of the last interior tile, q2 whose last op ends exactly on L, q3 = q2 + 1
    whose last op lacks one byte."""
    s = rw.Stream()
    body(s, 6)
    s.fill_to(TILE + 2000, big=1500)
    e3 = s.records[-1] + 11
    for n in PREAMBLE:
        s.add(rw.sized(n))
    e4 = s.records[-8]
    H = len(s)
    T = 2 * TILE
    L = T + TILE + INTERIOR_TAIL
    q1, q2 = T + TILE - 1, L - REACH
    aux = bytearray(L + 3000 - (H + rw.TINY))
    for q in (q1, q2, q2 + 1):
        for k in (12, 16, 17):
            aux[q + k - (H + rw.TINY)] = 0xff
    s.add(rw.record(aux=bytes(aux)))
    body(s, 12, 2)
    u, meta = s.finish()
    return World(u, meta, [meta["records"][2], meta["records"][4] + 7, e3, e4], L, long=True, q=(q1, q2, q2 + 1), T=T)


FAMILIES = {}
for _m in B_MODS:
    FAMILIES[f"cuts-{_m}"] = [functools.partial(cut_world, _m, _d) for _d, _ in CUTS]
FAMILIES["chunk"] = [functools.partial(chunk_world, 1), functools.partial(chunk_world, 37)]
DECOYS = ("hop_past", "hop_on_b", "before_true", "straddle")
FAMILIES["decoys"] = [functools.partial(decoy_world, _k) for _k in DECOYS]
FAMILIES["dense"] = [dense_world]
FAMILIES["long"] = [long_world]
NO_LOADS = ("long",)  # (its cut halves the only record behind the splits' blocks: every load is HALO)
KINDS = ("prefix", "mid")


@functools.lru_cache(maxsize=12)
def worlds(family):
    return [f() for f in FAMILIES[family]]


@functools.lru_cache(maxsize=24)
def shards(family, kind):
    return [Shard(w, kind) for w in worlds(family)]


PARAMS = [(f, k) for f in FAMILIES for k in KINDS]
LOAD_PARAMS = [(f, k) for f, k in PARAMS if f not in NO_LOADS]


# ---- without a GPU: the inputs are what the GPU tests need them to be ---------------------------------------------------
def test_cuts_lie_in_their_fields():
    for m in B_MODS:
        for w, (d, field) in zip(worlds(f"cuts-{m}"), CUTS):
            P = w.info["P"]
            assert w.b == P + d and (P + d) % TILE == m
            assert P in w.meta["records"] and w.u[P:P + P_SIZE] == probe()
            nxt = P + P_SIZE
            assert field_of(w.u, P, w.b) == field, (d, field)
            assert field != "next" or nxt in w.meta["records"]
            before = [x for x in w.meta["records"] if x < P]
            assert len(before) >= 12 and all(b - a <= 60 for a, b in zip(before[-12:], before[-11:] + [P]))
    assert {f for _, f in CUTS} == {"block_size", "fixed", "name", "cigar", "seq", "qual", "aux", "next"}
    assert NOPS > 64 and O_OPS + 4 * 64 in [d for d, _ in CUTS]


def test_decoys_are_what_their_names_say():
    ws = dict(zip(DECOYS, worlds("decoys")))
    for kind, w in ws.items():
        chain = w.o.record_chain(w.meta["header_end"], w.o.L).tolist()
        assert chain == w.meta["records"]
        for R in RS:
            on = set(np.flatnonzero(w.words(R) & W_SUCC).tolist())
            assert on - set(chain) == set(w.meta["decoys"]), (kind, R)  # every decoy is Success in the whole file
    w = ws["hop_past"]
    assert w.meta["decoys"][0] < w.b < w.meta["targets"][0]
    w = ws["hop_on_b"]
    assert w.meta["targets"][0] == w.b and w.b in w.meta["records"]
    w = ws["before_true"]
    d, T = w.meta["decoys"][0], w.meta["targets"][0]
    true = min(x for x in w.meta["records"] if x > d)
    assert 0 < true - d <= 200 and T > w.b and T in w.meta["records"]
    after = [x for x in w.meta["records"] if x >= true]
    assert after[10] + 66 < w.b  # T's ten-record chain ends before the cut
    for kind in KINDS:  # the record search from the member that starts 20 bytes before the decoy
        import oracle
        sh = Shard(w, kind)
        x0 = d - 20 - sh.a
        assert (sh.w.block_of(d - 20) >= sh.i0) and sh.find(x0, 10) == oracle.HALO
        assert w.o.find_record_start(int(w.o.start[w.block_of(d - 20)]), 10) == d
        assert not sh.eager(10)[1][true - sh.a] and sh.eager(10)[0][true - sh.a]  # the later true record is decidable
    w = ws["straddle"]
    big = max(x for x in w.meta["records"] if x < w.b)
    assert w.b - big > 100 and big + 1500 - w.b > 100


@pytest.mark.parametrize("family,kind", PARAMS)
def test_window_oracle_and_shards(family, kind):
    """Per shard and R: a non-hit window word is the whole file's; hit and non-hit positions exist; some hit position's
    window verdict differs from the whole file's; the eager hits are a subset of the full ones; every load the GPU
    tests make has an expected value; every shard has a load that returns partitions, and most have one that says HALO."""
    import oracle
    halos = 0
    for sh in shards(family, kind):
        assert (kind == "mid") == (sh.a > 0) and sh.hi < len(sh.w.blob) and sh.L == sh.b - sh.a
        outcomes = set()
        for R in RS:
            whole = sh.w.words(R)[sh.a:sh.b]
            w, h = sh.full(R)
            assert np.array_equal(w[~h], whole[~h]), (family, sh.b, R)
            assert h.any() and not h.all()
            assert (w[h] != whole[h]).any(), (family, sh.b, R, "no hit position differs from the whole file")
            calls, he = sh.eager(R)
            assert np.array_equal(calls[~he], (whole[~he] & W_SUCC) != 0)
            assert not (he & ~h).any() and he.any()
            for first, count in (sh.loads() if family not in NO_LOADS else ()):
                e = sh.expected_load(R, first, count)
                outcomes.add("halo" if e == oracle.HALO else "parts")
            # which chain pass the counts and the eager check take (run_chains: the list form up to this many PASS0
            # positions, record 0 passing being a Success at R = 1)
            p0 = int(((sh.full(1)[0] & W_SUCC) != 0).sum())
            assert (p0 > (sh.L - 100) // 32 + 4096 + 35) == bool(sh.w.info.get("dense")), (family, p0, sh.L)
            for _, x0w in sh.member_starts():
                assert sh.find(x0w, R) is not None
        # (a shard cut on a record's first byte, with no further split inside it, has no load that must say HALO)
        halos += "halo" in outcomes
        assert "parts" in outcomes or family in NO_LOADS, (family, sh.b)
    assert halos >= len(shards(family, kind)) // 2 or family in NO_LOADS


def test_long_shard_reaches_the_interior_kernels():
    w = worlds("long")[0]
    sh = Shard(w, "prefix")
    q1, q2, q3 = w.info["q"]
    T = w.info["T"]
    assert sh.a == 0 and sh.L == T + TILE + INTERIOR_TAIL and T % TILE == 0  # tiles 0 .. T / TILE are interior
    assert T <= q1 < T + TILE <= q2 and q2 + REACH == sh.L
    for R in RS:
        words, h = sh.full(R)
        assert not h[q1] and not h[q2] and h[q3]
        # in an interior tile only a hop makes a position unknown, never a read of record 0
        w1, h1 = sh.full(1)
        assert (w1[:T + TILE][h1[:T + TILE]] == (W_SUCC | 1 << 24)).all()
        assert not words[q2] & (1 << 14) and np.array_equal(words[[q1, q2]], w.words(R)[[q1, q2]])
    for q in (q1, q2, q3):
        assert w.u[q + 12] == 255 and w.u[q + 16:q + 18] == b"\xff\xff"
        assert all(x & 0xf <= 8 for x in w.u[q + 36 + 255:min(q + REACH, sh.L):4])  # every op it reads is valid


def test_dense_world_is_dense():
    w = worlds("dense")[0]
    host = max(x for x in w.meta["records"] if x < w.e4 - len(DENSE) * DENSE_N)
    first = host + rw.TINY
    for sh in (Shard(w, k) for k in KINDS):
        w1, h1 = sh.full(1)
        at = first - sh.a + 16 * np.arange(DENSE_N - 3)  # (the last ones read their name behind the run)
        assert (w1[at] == (W_SUCC | 1 << 24)).all() and h1[at].all()  # record 0 passes, the hop leaves the shard
        assert int(np.flatnonzero(h1)[0]) == at[0]  # ... and the first of them is the shard's first unknown position
        assert at[-1] - at[0] > CHUNK and (at < CHUNK).sum() > 4096  # two list rounds in k_chains' first chunk


def test_window_oracle_on_a_whole_stream():
    """With the whole stream as the window the window forms are the plain ones, and exactly the evaluations that the
    file's end decides are hits."""
    import oracle
    w = worlds("decoys")[0]
    o = w.o
    for R in RS:
        words, hits = oracle.check_full_window(o.u[:o.L], w.lens, R)
        assert np.array_equal(words, w.words(R)) and hits[-35:].all() and not hits[w.meta["records"][0]]
        calls, he = oracle.check_eager_window(o.u[:o.L], w.lens, R)
        assert np.array_equal(calls, (words & W_SUCC) != 0) and not (he & ~hits).any()
    x = w.meta["records"][3]
    assert oracle.find_record_start_window_eager(o.u[:o.L], w.lens, x + 1, 10) == w.meta["records"][4]
    assert oracle.find_record_start_window_eager(o.u[:o.L], w.lens, x + 1, 10, w.meta["records"][4] - x - 1) is None
    chain, hit = oracle.record_chain_window(o.u[:o.L], x, o.L)
    assert not hit and chain.tolist() == w.meta["records"][3:]
    chain, hit = oracle.record_chain_window(o.u[:o.L - 1], x, o.L)
    assert hit and chain.tolist() == w.meta["records"][3:-1]


# ---- on the GPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    """One context for every shard (sbam_load keeps its allocations)."""
    import sbam
    held = {}

    def open_(sh):
        data = np.frombuffer(sh.w.blob[sh.lo:sh.hi], np.uint8)
        if "g" not in held:
            held["g"] = sbam.BamFile(data, base_offset=sh.lo, file_size=len(sh.w.blob), contig_lengths=sh.w.lens)
        else:
            held["g"].load(data, base_offset=sh.lo, file_size=len(sh.w.blob))
            held["g"].run(contig_lengths=sh.w.lens)
        g = held["g"]
        assert g.uncompressed_size == sh.L and not g.loads_to_eof
        return g
    yield open_
    if "g" in held:
        held["g"].close()


def reduce_words(w):
    """The full-check Counts of result words (FullCheck.scala:141-191), in numpy."""
    from test_gpu_parity import pair_hist
    F = (w & 0x7ffff).astype(np.int64)
    k = ((w >> 24) & 0x7f).astype(np.int64)
    succ = (w & W_SUCC) != 0
    tff = ~succ & (F == 1) & (k == 0)
    counted = ~succ & ~tff
    pop = sum((F >> f) & 1 for f in range(19))
    key = pop + (k > 0)
    counts, positions, rbe = np.zeros((21, 19), np.int64), np.zeros(21, np.int64), np.zeros((21, 128), np.int64)
    np.add.at(positions, key[counted], 1)
    for f in range(19):
        np.add.at(counts[:, f], key[counted & (((F >> f) & 1) != 0)], 1)
    m = counted & (k > 0)
    np.add.at(rbe, (key[m], k[m]), 1)
    return {"n_success": int(succ.sum()), "n_too_few_fixed": int(tff.sum()), "counts": counts, "positions": positions,
            "rbe": rbe, "totals": counts.sum(0), "pair": pair_hist(w), "succ": succ}


def raw_counts(g, x0, x1, R, by_key):
    """sbam_check_full_counts itself: (return code, the struct, success bits, sbam_last_error().actual)."""
    import sbam
    c = sbam._Counts()
    bm = np.zeros((x1 - x0 + 63) // 64 + 1, np.uint64)
    rc = g.L.sbam_check_full_counts(g.ctx, x0, x1, R, by_key, ctypes.byref(c), bm.ctypes.data)
    bits = np.unpackbits(bm.view(np.uint8), bitorder="little")[:x1 - x0].astype(bool)
    return rc, c, bits, int(g.L.sbam_last_error(g.ctx).contents.actual)


def check_checkers(g, sh, R):
    L = sh.L
    want = sh.expect_words(R)
    for x0, x1 in ((0, L), (101, L), (37, L - 100)):
        got = g.check_full_words(x0, x1, R)
        bad = np.flatnonzero(got != want[x0:x1])
        assert bad.size == 0, f"words [{x0}, {x1}) of L = {L}: {bad.size} mismatches, first {bad[:5] + x0}: " \
                              f"{[hex(v) for v in got[bad[:5]]]} vs {[hex(v) for v in want[x0:x1][bad[:5]]]}"
    w, h = sh.full(R)
    r = reduce_words(w[~h])
    succ = np.zeros(L, bool)
    succ[~h] = r["succ"]
    for by_key in (0, 1):
        rc, c, bits, actual = raw_counts(g, 0, L, R, by_key)
        assert rc == (ERR_HALO if h.any() else 0)
        assert c.n_halo == h.sum() and (not h.any() or actual == c.n_halo)
        assert (c.n_success, c.n_too_few_fixed, c.n_positions) == (r["n_success"], r["n_too_few_fixed"], L)
        assert np.array_equal(np.ctypeslib.as_array(c.totals), r["totals"])
        assert np.array_equal(np.ctypeslib.as_array(c.positions), r["positions"])
        assert np.array_equal(np.ctypeslib.as_array(c.reads_before_error).reshape(21, 128), r["rbe"])
        assert np.array_equal(np.ctypeslib.as_array(c.pair_hist).reshape(19, 19), r["pair"])
        got = np.ctypeslib.as_array(c.counts).reshape(21, 19)
        assert np.array_equal(got if by_key else got[:3], r["counts"] if by_key else r["counts"][:3])
        assert np.array_equal(np.flatnonzero(bits), np.flatnonzero(succ)), "check_full_counts bitmap"
    calls, he = sh.eager(R)
    got = g.check_eager(0, L, R)
    bad = np.flatnonzero(got != (calls & ~he))
    assert bad.size == 0, f"check_eager: first {bad[:5]}, hit {he[bad[:5]]}"


def bitmap_state(g, sh, R, state):
    """Leave in the context what `state` says; returns the stream range [0, x) a bitmap at R may cover (None: no bitmap
    that this R may use) as (sure, maybe): covered at least to `sure`, at most to `maybe`."""
    L = sh.L
    full_first = int(np.flatnonzero(sh.full(R)[1])[0])
    if state == "none":
        g.reset()
        g.run(contig_lengths=sh.w.lens)
        return None
    if state == "counts":
        x1 = L - 100
        raw_counts(g, 0, x1, R, 0)
        return min(x1, full_first), min(x1, full_first)
    if state == "eager":
        g.check_eager_device(0, L, R)
        return full_first, int(np.flatnonzero(sh.eager(R)[1])[0])
    if state in ("words", "words_sub"):  # k_chains' bitmap, whatever the stream
        x1 = L if state == "words" else L - 100
        g.check_full_words(0, x1, R)
        return min(x1, full_first), min(x1, full_first)
    raw_counts(g, 0, L, {1: 2, 2: 10, 10: 1}[R], 0)  # another R's bitmap: to be ignored
    return None


STATES = ("none", "counts", "eager", "words", "words_sub", "other_R")


def check_find(g, sh, R):
    import oracle
    import sbam
    o = sh.w.o
    calls, he = sh.eager(R)
    decides = calls | he
    for state in STATES:
        bitmap_state(g, sh, R, state)
        for bs, x0w in sh.member_starts():
            want = sh.find(x0w, R)
            cases = [(10_000_000, want)]
            D = int(np.flatnonzero(decides[x0w:])[0])  # the first position that is Success or unknown: it decides
            if D > 0 and state in ("none", "eager"):
                # decided at delta == max_read_size - 1 (Success or HALO: a bitmap that reads "false" at an unknown
                # position says None here), None at max_read_size == delta
                cases += [(D + 1, sh.find(x0w, R, D + 1)), (D, sh.find(x0w, R, D))]
                assert cases[-2][1] == (want if isinstance(want, int) else oracle.HALO) and cases[-1][1] is None
            for mrs, e in cases:
                try:
                    got = g.find_record_start_with_delta(bs, R, mrs)
                except sbam.HaloException:
                    got = oracle.HALO
                if isinstance(e, int):
                    p = o.pos_of(sh.a + e)
                    e = (sbam.Pos(p.block_pos, p.offset), e - x0w)
                assert got == e, (state, bs, x0w, mrs, got, e)


def check_loads(g, sh, R):
    import oracle
    import sbam
    o = sh.w.o
    seen = set()  # (bitmap state, built by k_chains) of the loads whose proof was tried
    for state in ("none", "counts_L", "eager", "words", "words_sub"):
        if state == "counts_L":
            raw_counts(g, 0, sh.L, R, 0)
            h = sh.full(R)[1]
            cover = (int(np.flatnonzero(h)[0]),) * 2
        else:
            cover = bitmap_state(g, sh, R, state)
        for use_bm in ((False,) if state == "none" else (False, True)):
            for first, count in sh.loads():
                e = sh.expected_load(R, first, count)
                kw = dict(reads_to_check=R, use_success_bitmap=use_bm)
                if e == oracle.HALO:
                    with pytest.raises(sbam.HaloException):
                        g.split_records_arrays(sh.S, first, count, **kw)
                    with pytest.raises(sbam.HaloException):
                        g.load_records(sh.S, first, count, columns=None, **kw)
                    continue
                parts, X0, X1 = e
                bp, off, nonempty, n = g.split_records_arrays(sh.S, first, count, **kw)
                assert n.tolist() == [len(p) for p in parts]
                firsts = [o.pos_of(int(p[0])) for p in parts if len(p)]
                assert [(int(a), int(b)) for a, b, ne in zip(bp, off, nonempty) if ne] == \
                    [(p.block_pos, p.offset) for p in firsts]
                sizes, cols = g.load_records(sh.S, first, count, columns=("offset", "block_pos", "block_off", "block_size"),
                                             **kw)
                assert sizes.tolist() == [len(p) for p in parts]
                offs = np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int64)
                assert np.array_equal(cols["offset"] + sh.a, offs)  # the shard's stream offsets, shifted by a
                pos = [o.pos_of(int(x)) for x in offs]  # Pos is the file's
                assert cols["block_pos"].tolist() == [p.block_pos for p in pos]
                assert cols["block_off"].tolist() == [p.offset for p in pos]
                assert cols["block_size"].tolist() == [int.from_bytes(o.u[x:x + 4].tobytes(), "little") for x in offs]
                # which way the counts came: the proof is tried when the bitmap covers the chains, and holds exactly
                # when the Success bits of [X0, X1) are the chain (sbam_records.hip's predicate, on oracle words)
                path = g.records_path()
                if not use_bm or cover is None:
                    assert not path["tried"], path
                    continue
                sure, maybe = cover
                if X1 <= sure or X1 > maybe:
                    assert path["tried"] == (X1 <= sure), (path, X1, cover)
                if path["tried"]:
                    # which chain pass built this bitmap: k_chains for the words, and for the counts and the eager
                    # check where the PASS0 positions outnumber the list form's scratch (the dense family)
                    k_chains = state.startswith("words") or bool(sh.w.info.get("dense"))
                    assert (path["missing_links"] == -1) == k_chains, (state, path)
                    seen.add((state, k_chains))
                    w, h = sh.full(R)
                    bits = np.flatnonzero(((w[X0:X1] & W_SUCC) != 0) & ~h[X0:X1]) + X0
                    holds = np.array_equal(bits + sh.a, np.concatenate(parts))
                    assert path["proved"] == holds, (path, X0, X1)

    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("family,kind", PARAMS)
def test_checkers_on_shards(family, kind, R, ctx):
    for sh in shards(family, kind):
        check_checkers(ctx(sh), sh, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("family,kind", PARAMS)
def test_find_record_start_on_shards(family, kind, R, ctx):
    for sh in shards(family, kind):
        check_find(ctx(sh), sh, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("family,kind", LOAD_PARAMS)
def test_loads_on_shards(family, kind, R, ctx):
    seen = set()
    for sh in shards(family, kind):
        seen |= check_loads(ctx(sh), sh, R)
    # the chain pass behind each kind of bitmap was read from records_path(): k_chains behind the words, and behind the
    # counts and the eager check in the dense family alone
    dense = family == "dense"
    assert seen >= {("counts_L", dense), ("eager", dense), ("words", True), ("words_sub", True)}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
def test_find_record_start_max_read_size_on_a_whole_file(R):
    """Found at delta == max_read_size - 1, None at max_read_size == delta, with and without a bitmap."""
    import sbam
    w = worlds("decoys")[0]
    o = w.o
    with sbam.BamFile(w.blob) as g:
        for state in ("none", "eager"):
            if state == "eager":
                g.check_eager_device(0, o.L, R)
            for i in range(1, o.nblocks):
                bs = int(o.start[i])
                x0 = int(o.uoff[i])
                x = o.find_record_start(bs, R)
                assert x is not None
                for mrs in (x - x0 + 1, x - x0) if x > x0 else (1,):
                    want = o.find_record_start(bs, R, mrs)
                    got = g.find_record_start_with_delta(bs, R, mrs)
                    assert (want is None and got is None) or (got[1] == want - x0 and g.offset_of(got[0]) == want)
