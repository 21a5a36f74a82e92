"""The three record kernels of csrc/sbam_records.hip — k_chain_proof (with hop_ok), k_split_popcounts (its bitmap
popcount and its 64-ary search of the PASS0 list, wave_lower_bound) and k_split_offsets — on bitmaps, streams and lists
injected through sbam_test_chain_proof, against numpy:

  proof      every set bit p of [X0, X1) has 0 <= block_size(p), q = p + 4 + block_size(p) <= L, no set bit in
             (p, min(q, X1)) and, when q < X1, bit q set (the predicate in the file's header);
  counts     the set bits of [xs, xe), or with a list and exact[2] == 0 the list entries in [xs, xe); 0 for xs < 0 or
             xs >= xe; the flag is raised by a split whose xs is not a set bit (not a list entry);
  offsets    the set bits of every split, in order, at the exclusive scan of the counts.

The inputs are chains written here: positions with gaps >= 4 and block_size = gap - 4 at each, so a hop can span 1 to 12
bitmap words with its ends on any bit; each chain is then broken in exactly one way."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def gpu_chain_proof(u, bits, xa, X0, X1, xs=(), xe=(), plist=None, exact=None, L=None):
    """(proof flag, popcount flag, counts, offsets) from the device.  bits: bool array whose [0] is stream offset xa."""
    import sbam
    u = np.ascontiguousarray(u, np.uint8)
    L = u.size if L is None else L
    nw = max((bits.size + 63) // 64, 1)
    padded = np.zeros(nw * 64, np.uint8)
    padded[:bits.size] = bits
    bm = np.packbits(padded, bitorder="little").view(np.uint64)
    xs, xe = np.ascontiguousarray(xs, np.int64), np.ascontiguousarray(xe, np.int64)
    n = xs.size
    counts = np.full(max(n, 1), -7, np.int64)
    cs = np.concatenate([[0], np.cumsum(padded, dtype=np.int64)])  # room for the bitmap's count of every split
    cap = 1 + sum(int(cs[b - xa] - cs[a - xa]) for a, b in zip(xs.tolist(), xe.tolist()) if 0 <= a < b)
    offs = np.full(cap, -7, np.int64)
    fail = np.full(2, -7, np.int32)
    n_off = ctypes.c_int64(0)
    pl = None if plist is None else np.ascontiguousarray(np.append(plist, 0), np.int64)  # (never a null pointer)
    ex = None if exact is None else np.ascontiguousarray(exact, np.uint64)
    rc = sbam.load_library().sbam_test_chain_proof(
        0, u.ctypes.data, L, bm.ctypes.data, nw, xa, X0, X1, xs.ctypes.data, xe.ctypes.data, n,
        None if pl is None else pl.ctypes.data, 0 if plist is None else len(plist),
        None if ex is None else ex.ctypes.data, fail.ctypes.data, counts.ctypes.data, offs.ctypes.data, cap,
        ctypes.byref(n_off))
    assert rc == 0, rc
    return int(fail[0]), int(fail[1]), counts[:n], offs[:n_off.value]


# ---- numpy statements ----------------------------------------------------------------------------------------------
def ref_proof(u, L, bits, xa, X0, X1) -> bool:
    """True when the proof holds (the device flag is its negation)."""
    P = np.flatnonzero(bits[X0 - xa:X1 - xa]) + X0
    if P.size == 0:
        return True
    if P[-1] + 4 > L:
        return False
    bs = np.array([int.from_bytes(u[p:p + 4].tobytes(), "little", signed=True) for p in P.tolist()], np.int64) \
        if P.size < 64 else block_sizes(u, P)
    q = P + 4 + bs
    nxt = np.append(P[1:], X1)
    return bool(np.all((bs >= 0) & (q <= L) & np.where(q < X1, nxt == q, nxt >= X1)))


def block_sizes(u, P):
    b = u[P[:, None] + np.arange(4)].astype(np.int64)
    return (b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24).astype(np.uint32).view(np.int32).astype(np.int64)


def ref_counts(bits, xa, xs, xe, plist=None):
    """(flag, counts, offsets): from the bitmap, or the counts and the flag from the list."""
    cnt, fail, out = [], 0, []
    for a, b in zip(xs, xe):
        if a < 0 or a >= b:
            cnt.append(0)
            continue
        on = np.flatnonzero(bits[a - xa:b - xa]) + a
        out.append(on)
        if plist is None:
            cnt.append(on.size)
            fail |= int(not bits[a - xa])
        else:
            ia, ib = np.searchsorted(plist, a), np.searchsorted(plist, b)
            cnt.append(int(ib - ia))
            fail |= int(not (ia < len(plist) and plist[ia] == a))
    return fail, np.array(cnt, np.int64), np.concatenate(out + [np.zeros(0, np.int64)])


# ---- chains ----------------------------------------------------------------------------------------------------------
def write_chain(pos, L):
    """(stream, bitmap over [0, L)): block_size = gap - 4 at every position; the last record ends on L."""
    pos = np.asarray(pos, np.int64)
    gaps = np.diff(np.append(pos, L))
    assert gaps.min() >= 4
    u = np.zeros(L, np.uint8)
    u[pos[:, None] + np.arange(4)] = ((gaps - 4)[:, None] >> (8 * np.arange(4))) & 0xff
    bits = np.zeros(L, bool)
    bits[pos] = True
    return u, bits


def random_chain(n_pos, seed):
    """Gaps of every kind: inside one word, a few words (the usual record), up to 12 words."""
    rng = np.random.default_rng(seed)
    pos, x = [], 70
    while x < n_pos - 900:
        pos.append(x)
        r = rng.random()
        x += int(rng.integers(4, 64) if r < 0.3 else rng.integers(64, 400) if r < 0.9 else rng.integers(400, 800))
    return np.array(pos, np.int64), x


def put_bs(u, p, v):
    u[p:p + 4] = np.frombuffer(int(v).to_bytes(4, "little", signed=True), np.uint8)


# A ladder of hops p -> q: for every distance in words between p + 1 and q (0 to 12) and several bit positions of the
# two ends, so that hop_ok's loaded-span path (under 8 words) and its bm_any path each see ends on bit 0 and bit 63.
LADDER = [(dw, pb, qb) for dw in range(13) for pb, qb in ((20, 41), (63, 0), (62, 63), (0, 1), (5, 5))
          if dw > 0 or qb - pb >= 4]


def ladder():
    pos, x = [], 64
    hops = []
    for dw, pb, qb in LADDER:
        p = (x // 64 + 2) * 64 + pb
        q = ((p + 1) // 64 + dw) * 64 + qb
        assert q - p >= 4
        pos += [p] if not pos or pos[-1] != p else []
        pos.append(q)
        hops.append((p, q))
        x = q
    L = pos[-1] + 40
    return np.array(sorted(set(pos)), np.int64), L, hops


def inside_classes(p, q):
    """Offsets of every class inside the hop: its ends, both sides of every word edge it crosses (a sample for long
    hops), and its middle."""
    c = {p + 1, q - 1, (p + q) // 2}
    words = list(range((p + 1) // 64 + 1, (q - 1) // 64 + 1))
    for w in words[:2] + words[-2:] + words[len(words) // 2:len(words) // 2 + 1]:
        c |= {w * 64 - 1, w * 64}
    return sorted(x for x in c if p < x < q)


@pytest.fixture(scope="module")
def ladder_chain():
    pos, L, hops = ladder()
    u, bits = write_chain(pos, L)
    return pos, L, hops, u, bits


def test_ladder_holds_and_counts(ladder_chain):
    pos, L, hops, u, bits = ladder_chain
    assert ref_proof(u, L, bits, 0, int(pos[0]), L)
    xs = [int(pos[0]), int(pos[3]), -1, int(pos[5]), int(pos[7]), int(pos[2]) + 1]
    xe = [L, int(pos[9]), 50, int(pos[5]), int(pos[7]) + 1, int(pos[8])]
    fp, fc, cnt, off = gpu_chain_proof(u, bits, 0, int(pos[0]), L, xs, xe)
    rf, rc, ro = ref_counts(bits, 0, xs, xe)
    assert fp == 0 and fc == rf == 1  # (the last split starts one off a record)
    assert np.array_equal(cnt, rc) and np.array_equal(off, ro)
    fp, fc, cnt, off = gpu_chain_proof(u, bits, 0, int(pos[0]), L, xs[:5], xe[:5])
    assert (fp, fc) == (0, 0) and np.array_equal(off, ref_counts(bits, 0, xs[:5], xe[:5])[2])


@pytest.mark.parametrize("i", range(len(LADDER)))
def test_one_extra_bit_inside_a_hop(i, ladder_chain):
    """One false-positive bit at every offset class of one hop: the proof fails; the same bit outside [X0, X1) does
    not fail it."""
    pos, L, hops, u, bits = ladder_chain
    p, q = hops[i]
    for x in inside_classes(p, q):
        b = bits.copy()
        b[x] = True
        assert not ref_proof(u, L, b, 0, int(pos[0]), L)
        assert gpu_chain_proof(u, b, 0, int(pos[0]), L)[0] == 1, (LADDER[i], x - p, q - x)
        # X1 on the extra bit, one past it, and on p + 1; X0 one past the extra bit
        for X0, X1 in ((int(pos[0]), x), (int(pos[0]), x + 1), (int(pos[0]), p + 1), (x + 1, L), (x, L)):
            want = ref_proof(u, L, b, 0, X0, X1)
            assert gpu_chain_proof(u, b, 0, X0, X1)[0] == (not want), (LADDER[i], x - p, X0, X1)


@pytest.mark.parametrize("i", range(len(LADDER)))
def test_one_broken_record(i, ladder_chain):
    """The hop's source record with its bit cleared, its target's bit cleared, block_size off by one either way,
    negative, and past L."""
    pos, L, hops, u, bits = ladder_chain
    p, q = hops[i]
    X0 = int(pos[0])
    for what in ("clear_q", "bs+1", "bs-1", "negative", "past_L", "clear_p"):
        uu, b = u.copy(), bits.copy()
        if what == "clear_q":
            b[q] = False
        elif what == "clear_p":
            b[p] = False
        else:
            put_bs(uu, p, {"bs+1": q - p - 3, "bs-1": q - p - 5, "negative": -(q - p), "past_L": L - p - 3}[what])
        want = ref_proof(uu, L, b, 0, X0, L)
        assert not want or (what == "clear_p" and p == X0) or (what == "bs-1" and q - p == 4), (LADDER[i], what)
        assert gpu_chain_proof(uu, b, 0, X0, L)[0] == (not want), (LADDER[i], what)
        # a range that ends on the record leaves it out; one that ends behind it takes it in
        for X1 in (p, p + 1, q, q + 1):
            if X1 > X0:
                want = ref_proof(uu, L, b, 0, X0, X1)
                assert gpu_chain_proof(uu, b, 0, X0, X1)[0] == (not want), (LADDER[i], what, X1 - p)


RANDOM = [(6000, 1), (70_000, 2), (300_000, 3)]


@pytest.fixture(scope="module")
def random_chains():
    out = {}
    for n, seed in RANDOM:
        pos, L = random_chain(n, seed)
        out[n] = (pos, L) + write_chain(pos, L)
    return out


@pytest.mark.parametrize("n", [n for n, _ in RANDOM])
@pytest.mark.parametrize("xa", [0, 64])
def test_random_chain_ranges_and_splits(n, xa, random_chains):
    """A clean chain: the proof holds for X0 / X1 on a set bit, one off it and mid-word; splits of one record, of a few
    words, of more than 256 words (k_split_offsets' loop) and of more than 2048 (the popcount's 8-deep loop)."""
    pos, L, u, bits = random_chains[n]
    rng = np.random.default_rng(n)
    b = bits[xa:]
    first = int(pos[pos >= xa][0])
    for X0, X1 in ((first, L), (first + 1, L), (first, int(pos[-1])), (first, int(pos[-1]) + 1), (first + 33, L - 33),
                   (int(pos[len(pos) // 2]), int(pos[len(pos) // 2 + 1])), (int(pos[7]), int(pos[7]) + 1)):
        assert ref_proof(u, L, b, xa, X0, X1)
        assert gpu_chain_proof(u, b, xa, X0, X1)[0] == 0, (X0, X1)
    cuts = np.sort(rng.choice(pos[pos >= xa], size=min(40, pos.size - 2), replace=False))
    xs = [first] + cuts.tolist() + [-1, int(cuts[3]), int(cuts[5]), first]
    xe = cuts.tolist() + [L] + [L, int(cuts[3]), int(cuts[4]), L]
    fp, fc, cnt, off = gpu_chain_proof(u, b, xa, first, L, xs, xe)
    rf, rc, ro = ref_counts(b, xa, xs, xe)
    assert (fp, fc, rf) == (0, 0, 0)
    assert np.array_equal(cnt, rc) and np.array_equal(off, ro)
    # chain ends off the records: xe one past a record takes it in; xs one past a record raises the flag
    xs2, xe2 = [first, int(cuts[2])], [int(cuts[2]) + 1, int(cuts[9]) + 63]
    fp, fc, cnt, off = gpu_chain_proof(u, b, xa, first, L, xs2, xe2)
    rf, rc, ro = ref_counts(b, xa, xs2, xe2)
    assert fc == rf == 0 and np.array_equal(cnt, rc) and np.array_equal(off, ro)
    assert gpu_chain_proof(u, b, xa, first, L, [int(cuts[2]) + 1], [L])[1] == 1


@pytest.mark.parametrize("what", ["extra", "clear", "bs+1", "bs-1", "negative", "past_L"])
def test_random_chain_one_mutation(what, random_chains):
    pos, L, u, bits = random_chains[70_000]
    rng = np.random.default_rng(len(what))
    X0 = int(pos[0])
    for i in rng.choice(np.arange(1, pos.size - 1), size=10, replace=False).tolist():
        p, q = int(pos[i]), int(pos[i + 1])
        uu, b = u.copy(), bits.copy()
        if what == "extra":
            if q - p < 6:
                continue
            b[int(rng.integers(p + 1, q))] = True
        elif what == "clear":
            b[p] = False
        else:
            put_bs(uu, p, {"bs+1": q - p - 3, "bs-1": q - p - 5, "negative": -5, "past_L": L - p}[what])
        want = ref_proof(uu, L, b, 0, X0, L)
        assert not want or (what == "bs-1" and q - p == 4)
        assert gpu_chain_proof(uu, b, 0, X0, L)[0] == (not want), (what, i)
        assert gpu_chain_proof(uu, b, 0, X0, p)[0] == 0 and gpu_chain_proof(uu, b, 0, q, L)[0] == 0, (what, i)


def test_stream_end(random_chains):
    """The last record: its hop ends on L (holds), one past L, and its block_size lies in the stream's last bytes."""
    pos, L, u, bits = random_chains[6000]
    X0, last = int(pos[0]), int(pos[-1])
    assert gpu_chain_proof(u, bits, 0, X0, L)[0] == 0
    for Lc in (L - 1, last + 4, last + 3, last + 1):  # a shorter stream under the same bitmap
        want = ref_proof(u[:Lc], Lc, bits[:Lc], 0, X0, Lc)
        assert not want
        assert gpu_chain_proof(u[:Lc], bits[:Lc], 0, X0, Lc, L=Lc)[0] == 1, Lc


# ---- the list path ------------------------------------------------------------------------------------------------------
LIST_NS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 262_145]


@pytest.fixture(scope="module")
def lists():
    out = {}
    for n in LIST_NS:
        rng = np.random.default_rng(n)
        plist = 130 + np.cumsum(rng.integers(4, 12, size=n)).astype(np.int64)
        L = int(plist[-1]) + 200 if n else 1000
        bits = np.zeros(L, bool)
        bits[plist] = True
        out[n] = (plist, L, bits)
    return out


def list_splits(plist, L, rng):
    """xs on a list entry and off one, xe on an entry and one past it, xs = -1, xs >= xe, the whole range."""
    n = len(plist)
    xs, xe = [-1, 500, 64], [L, 500, L]
    if n:
        idx = np.unique(np.concatenate([[0, n - 1, n // 2], rng.integers(0, n, 12)]))
        for i in idx.tolist():
            j = min(n - 1, i + int(rng.integers(0, max(2, n // 3))))
            xs += [int(plist[i]), int(plist[i]), int(plist[i]) + 1, int(plist[i]) - 1]
            xe += [int(plist[j]), int(plist[j]) + 1, L, int(plist[j]) + 1]
    return xs, xe


@pytest.mark.parametrize("n", LIST_NS)
@pytest.mark.parametrize("failed_fallbacks", [0, 3])
def test_list_counts(n, failed_fallbacks, lists):
    """exact[2] == 0: the counts are the list's (two searches per split); else the bitmap's.  A bitmap that holds
    bits the list lacks tells the two apart."""
    plist, L, bits = lists[n]
    rng = np.random.default_rng(n + 1)
    xs, xe = list_splits(plist, L, rng)
    u = np.zeros(L, np.uint8)
    exact = [7, 0, failed_fallbacks]
    for extra in (False, True):
        b = bits.copy()
        if extra:
            b[[65, 127, L - 3]] = True
            if n:
                b[int(plist[n // 2]) + 2] = True
        fp, fc, cnt, off = gpu_chain_proof(u, b, 0, 64, L, xs, xe, plist, exact)
        rf, rc, ro = ref_counts(b, 0, xs, xe, plist if failed_fallbacks == 0 else None)
        assert fc == rf
        assert np.array_equal(cnt, rc), np.flatnonzero(cnt != rc)[:5]
        if not extra or failed_fallbacks:  # the offsets are the bitmap's: comparable when the counts are too
            assert np.array_equal(off, ro)
        assert fp == (0 if failed_fallbacks == 0 else int(not ref_proof(u, L, b, 0, 64, L)))


@pytest.mark.parametrize("exact,runs", [((5, 0, 0), False), ((0, 0, 0), False), ((0, 1, 0), True), ((0, 0, 1), True),
                                        (None, True)])
def test_proof_skipped_on_exact_counters(exact, runs, ladder_chain):
    """No missing link and no failed fallback: the proof is skipped whatever the bitmap holds; either counter non-zero,
    or no counters at all, and it runs."""
    pos, L, hops, u, bits = ladder_chain
    b = bits.copy()
    p, q = hops[len(hops) // 2]
    b[(p + q) // 2] = True
    assert not ref_proof(u, L, b, 0, int(pos[0]), L)
    plist = None if exact is None else pos
    assert gpu_chain_proof(u, b, 0, int(pos[0]), L, [int(pos[0])], [L], plist, exact)[0] == int(runs)
    assert gpu_chain_proof(u, bits, 0, int(pos[0]), L, [int(pos[0])], [L], plist, exact)[0] == 0
