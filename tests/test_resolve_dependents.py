"""k_inflate_resolve's dependent pass on hand-built token streams: files of small BGZF blocks written token by token
(deflate_writer, bgzf_writer) so that matches read what earlier matches of the same resolver step wrote — chains,
self-overlapping runs, sources straddling the step's base, more than 64 dependent bytes, the ring's wrap and mirror,
ISIZE cutting a dependent, a too-far distance next to dependents — each compared byte for byte with zlib.

steps() restates the resolver's step cutting (two tokens per lane, 64 lanes, a step's words start within 1024 bytes
of its base), so the CPU test can check that every group really has the dependents it is named for."""
import functools
import zlib

import numpy as np
import pytest

import bgzf_writer
import deflate_writer as dw
from test_inflate_streams import EOF_BLOCK, bgzf_block, gpu_result, oracle_result

SPAN, LANES = 1024, 64


def steps(tokens, isize=None):
    """[(base B, [(mO, d, Le) of each dependent])] for every resolver step of one block's tokens."""
    flat = []  # the 16-bit words: ("l", byte) | ("L", length) | ("d", distance)
    for t in tokens:
        flat += [("l", t)] if isinstance(t, int) else [("L", t[0]), ("d", t[1])]
    ae = sum(1 if k == "l" else v if k == "L" else 0 for k, v in flat)
    ae = ae if isize is None else min(ae, isize)
    flat += [("p", 0)] * (2 * LANES + 2)
    B, tp, out = 0, 0, []
    while B < ae:
        acc, deps, last_b_len, E = 0, [], False, B
        for i in range(LANES):
            a, b, n = flat[tp + 2 * i], flat[tp + 2 * i + 1], flat[tp + 2 * i + 2]
            O = B + acc
            if not (acc < SPAN and O < ae):
                break
            nl = (a[0] == "l") + (b[0] == "l")
            Lm = a[1] if a[0] == "L" else b[1] if b[0] == "L" else 0
            d = b[1] if a[0] == "L" else n[1]
            last_b_len = b[0] == "L"
            if Lm:
                mO = O + (nl if b[0] == "L" else 0)
                Le = min(Lm, ae - mO)
                if Le > 0 and d <= mO and mO - d + min(Le, d) > B:
                    deps.append((mO, d, Le))
            acc += nl + Lm
            E = min(ae, B + acc)
            nt = i + 1
        assert E > B
        out.append((B, deps))
        B, tp = E, tp + 2 * nt + (1 if last_b_len else 0)
    return out


def depth(deps):
    """The longest chain of hops through dependents' outputs that any dependent byte's source makes."""
    best = 0
    for mO, d, Le in deps:
        for j in range(Le):
            s, n = mO - d + j % d, 0
            for qO, qd, qL in reversed(deps):
                if qO <= s < qO + qL:
                    s, n = qO - qd + (s - qO) % qd, n + 1
            best = max(best, n)
    return best


def mod_hops(deps):
    """Hops that land in a dependent's output at or past its distance (the sweep's division)."""
    n = 0
    for mO, d, Le in deps:
        for j in range(Le):
            s = mO - d + j % d
            for qO, qd, qL in reversed(deps):
                if qO <= s < qO + qL:
                    n += s - qO >= qd
                    s = qO - qd + (s - qO) % qd
    return n


def block(tokens, isize=None, fixed=False):
    """(BGZF block, the bytes zlib inflates its payload to, cut at isize)"""
    w = dw.BitWriter()
    if fixed:
        dw.fixed(w, tokens, True)
    else:
        lit, dist = dw.lens_for(tokens)
        dw.dynamic(w, tokens, True, lit, dist)
    p = w.tobytes()
    z = zlib.decompressobj(-15)
    want = z.decompress(p) if isize is None else z.decompress(p, isize)
    assert isize is not None or (z.eof and want == dw.expand(tokens))
    return bgzf_block(p, len(want)), want


def lits(r, n):
    return [int(x) for x in r.integers(0, 256, n)]


def g_chains(r):
    """depth 1..6: each match reads exactly the previous match's output; the first reads literals of its own step"""
    out = []
    for dep in range(1, 7):
        for L in (3, 5, 16, 17, 40):
            for pre in (128, 127):
                out.append(lits(r, pre) + lits(r, L) + [(L, L)] * (dep + 1) + lits(r, 3))
    return out


def g_depth64(r):
    """a step of 64 matches with L = d = 3, each reading the one before: after 129 literals every lane of the second
    step holds a match and the first one reads that step's literal (64 dependents, 63 hops); after 126..128 and 131
    literals (the other token alignments) one or two fewer"""
    return [lits(r, pre) + [(3, 3)] * 64 + lits(r, 2) for pre in (129, 128, 127, 126, 131)]


def g_straddle(r):
    """the first step is [0, 128); then matches whose source begins before 128 and ends after it"""
    out = []
    for k in (1, 2, 3, 7):          # literals of the second step before the match
        for L in (3, 4, 9, 30, 258):
            for back in (1, 2, 5, 100):  # the source starts `back` bytes before the base
                d = k + back
                if min(L, d) <= back:  # (the source would end at or before the base)
                    continue
                out.append(lits(r, 128) + lits(r, k) + [(L, d), (5, 4), (7, L + 5)] + lits(r, 2))
    return out


def g_overlap(r):
    """self-overlapping runs, source start before the base or inside the step, then readers from inside the run"""
    out = []
    for d in range(1, 21):
        for L in sorted({3, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 17, 64, 65, 258}):
            if L < 3:
                continue
            for k in (d // 2, 30 + d):  # literals of the step before the run: fewer than d, or more
                out.append(lits(r, 128) + lits(r, k) + [(L, d), (5, L // 2 + 1), (9, L + 4)] + lits(r, 1) +
                           [(6, 10 + L // 3)])
    return out


def g_wide(r):
    """more than 64 dependent bytes in a step: three (258, 1) runs and readers of them"""
    return [lits(r, 128) + lits(r, 1) + [(258, 1)] * 3 + [(100, 400), (258, 300), (3, 1)] + lits(r, 3),
            lits(r, 127) + lits(r, 2) + [(258, 2), (258, 1), (258, 3), (70, 600), (65, 64), (64, 65)],
            lits(r, 128) + lits(r, 9) + [(64, 9), (65, 64), (63, 65), (1 + 64, 1)]]


def dense(r, n_out, max_d=8):
    """match-heavy tokens: short matches at short distances, so nearly every match is a dependent"""
    toks, out = lits(r, 4), 4
    while out < n_out:
        if r.random() < 0.15:
            toks.append(int(r.integers(0, 256)))
            out += 1
        else:
            L = int(r.integers(3, 259)) if r.random() < 0.03 else int(r.integers(3, 13))
            toks.append((L, int(r.integers(1, min(out, max_d) + 1))))
            out += L
    return toks


RING_OFFSETS = (0, 1, 31, 32, 4064, 4095)


def g_random(r, n=1000):
    """match-heavy random streams: distances 1..40, lengths 3..258"""
    out = []
    for _ in range(n):
        toks, o = lits(r, int(r.integers(1, 6))), 0
        o = len(toks)
        for _ in range(int(r.integers(5, 70))):
            if r.random() < 0.2:
                toks.append(int(r.integers(0, 256)))
                o += 1
            else:
                L = int(r.integers(3, 259)) if r.random() < 0.3 else int(r.integers(3, 20))
                toks.append((L, int(r.integers(1, min(o, 40) + 1))))
                o += L
        out.append(toks)
    return out


GROUPS = {"chains": g_chains, "depth64": g_depth64, "straddle": g_straddle, "overlap": g_overlap, "wide": g_wide,
          "random0": g_random, "random1": g_random, "random2": g_random}


@functools.lru_cache(maxsize=None)
def group_tokens(name):
    return GROUPS[name](np.random.default_rng(sorted(GROUPS).index(name) + 77))


@functools.lru_cache(maxsize=None)
def group_file(name):
    """(file bytes, [expected output of each block])"""
    made = [block(t, fixed=i % 2 == 0) for i, t in enumerate(group_tokens(name))]
    return b"".join(b for b, _ in made) + EOF_BLOCK, [w for _, w in made]


@functools.lru_cache(maxsize=None)
def ring_file():
    """Stored blocks in front of each dense block so that its first output byte falls on ring byte 0, 1, 31, 32, 4064
    and 4095; more than 8 KiB of output each, so the ring wraps twice under dependents."""
    r = np.random.default_rng(5)
    parts, wants, tested, at = [], [], [], 0
    for k in RING_OFFSETS:
        pad = (k - at) % 4096 or 4096
        filler = bytes(r.integers(0, 256, pad, dtype=np.uint8))
        parts.append(bgzf_writer.stored_block(filler))
        wants.append(filler)
        at += pad
        assert at % 4096 == k
        toks = dense(r, 8192 + 700)
        b, w = block(toks)
        parts.append(b)
        wants.append(w)
        tested.append((at, toks))
        at += len(w)
    return b"".join(parts) + EOF_BLOCK, wants, tested


@functools.lru_cache(maxsize=None)
def isize_file():
    """ISIZE ends the block inside a dependent match: a chain link, a long run, a reader of the run"""
    r = np.random.default_rng(9)
    made = []
    for toks, cut in ((lits(r, 128) + lits(r, 5) + [(5, 5)] * 4, 3),
                      (lits(r, 128) + lits(r, 2) + [(258, 2), (40, 7)], 11),
                      (lits(r, 128) + lits(r, 2) + [(258, 2), (40, 7)], 40 + 100),
                      (lits(r, 129) + [(3, 3)] * 64, 1)):
        n = len(dw.expand(toks)) - cut
        made.append((toks, n) + block(toks, isize=n))
    return b"".join(m[2] for m in made) + EOF_BLOCK, made


def toofar_tokens():
    r = np.random.default_rng(11)
    return lits(r, 128) + lits(r, 4) + [(4, 4), (6, 3), (5, 200), (4, 4), (9, 2)] + lits(r, 2)


def compare(data, wants):
    kind, got = gpu_result(data)
    assert kind == "ok", got
    at = 0
    for i, w in enumerate(wants):
        assert got[at:at + len(w)] == w, "block %d of %d (output offset %d)" % (i, len(wants), at)
        at += len(w)
    assert len(got) == at


def test_groups_have_their_dependents():
    """The files are what they are named for (steps() restates the resolver's step cutting): chains of every depth
    1..6, a step of 63 or more chained dependents, sources straddling base 128, hops that land past a run's first
    period, steps with more than 64 dependent bytes, dependents whose bytes and whose sources fall on ring bytes
    0..31 at every tested block offset, an ISIZE inside a dependent, dependents next to the too-far distance."""
    by_depth = {max(depth(d) for _, d in steps(t)) for t in group_tokens("chains")}
    assert by_depth >= set(range(1, 7)), by_depth
    d64 = [max((len(d), depth(d)) for _, d in steps(t)) for t in group_tokens("depth64")]
    assert d64[0] == (64, 63) and all(n >= 62 and h >= 61 for n, h in d64), d64
    for t in group_tokens("straddle"):
        B, deps = steps(t)[1]
        assert B == 128 and any(mO - d < 128 < mO - d + min(Le, d) for mO, d, Le in deps), t[128:]
    n_mod = 0  # blocks where a reader's source lands in a dependent run past the run's first period
    for t in group_tokens("overlap"):
        B, deps = steps(t)[1]
        assert B == 128 and len(deps) >= 3
        n_mod += mod_hops(deps) > 0
    assert n_mod >= 100, n_mod
    for t in group_tokens("wide"):
        assert max(sum(Le for _, _, Le in d) for _, d in steps(t)) > 64
    _, _, tested = ring_file()
    for uoff, toks in tested:
        dst, src = set(), set()
        for _, deps in steps(toks):
            for mO, d, Le in deps:
                dst.update((uoff + p) % 4096 for p in range(mO, mO + Le))
                src.update((uoff + p) % 4096 for p in range(mO - d, mO - d + min(Le, d)))
        # (every mirrored byte is written by a dependent; sources are the first min(Le, d) bytes only, so sparser)
        assert set(range(32)) <= dst and len(set(range(32)) & src) >= 8, uoff % 4096
    for toks, n, _, want in isize_file()[1]:
        last = steps(toks, isize=n)[-1][1][-1]
        full = {m[0]: m[2] for _, d in steps(toks) for m in d}
        assert len(want) == n and last[0] + last[2] == n and last[2] < full[last[0]]
    st = steps(toofar_tokens())  # (steps() leaves the too-far match out, as the kernel does)
    assert len(st[1][1]) == 4
    deps = [len(d) for name in ("random0", "random1", "random2") for t in group_tokens(name) for _, d in steps(t)]
    assert len(deps) >= 3000 and sum(deps) > 30000


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_dependent_shapes(name):
    compare(*group_file(name))


@pytest.mark.gpu
def test_ring_wrap_and_mirror():
    data, wants, _ = ring_file()
    compare(data, wants)


@pytest.mark.gpu
def test_isize_cuts_a_dependent():
    data, made = isize_file()
    compare(data, [m[3] for m in made])


@pytest.mark.gpu
def test_too_far_distance_among_dependents():
    """A distance reaching before the block's first byte in a step that also has dependents: the block goes to the
    exact decoder, which stops where zlib raises "invalid distance too far back"; the blocks around it do not change
    that."""
    r = np.random.default_rng(12)
    good = block(dense(r, 600))[0]
    w = dw.BitWriter()
    toks = toofar_tokens()
    dw.fixed(w, toks, True)
    with pytest.raises(zlib.error, match="too far back"):
        zlib.decompressobj(-15).decompress(w.tobytes())
    data = good + bgzf_block(w.tobytes(), 128 + 4 + 4 + 6 + 5 + 4 + 9 + 2) + good + EOF_BLOCK
    got = gpu_result(data)
    # (the library reports a data error as the reference does: by the bytes zlib had written when it stopped, here
    # the 142 in front of the too-far match)
    assert got == ("error", "Expected 162 decompressed bytes, found 142"), got
    assert got == oracle_result(data)
