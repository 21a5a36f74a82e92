"""Inflate on legal DEFLATE that zlib's encoder never writes (and on the invalid streams next to it): BGZF files built
bit by bit with tests/deflate_writer.py, checked against the oracle's zlib inflate (Inflater.inflate(buf, 0, ISIZE),
bgzf/src/main/scala/org/hammerlab/bgzf/block/Stream.scala:31-71) and, for the decoder path, against the rule of
k_inflate_wave: a payload goes to the exact per-lane decoder (inflate_fallbacks) when it holds a stored block after
Huffman output, an incomplete or empty code set, an invalid header or symbol, a stream that ends before ISIZE or goes
on past it, or a distance too far back; everything else (complete codes only, no stored block, the final block ending
exactly at ISIZE) must stay on the wave decoder — zlib's ENOUGH bound (852 / 592 entries at root 9) says that no
complete code overflows its 340 / 80 sub-table entries.

Every stream is first pinned on the CPU (no gpu mark): zlib returns expand(tokens) for the valid ones and raises the
expected message for the invalid ones, and the oracle agrees.

Three things that differ from a first guess, all pinned by the CPU tests below:
  * HCLEN = 4 admits only the symbols 16, 17, 18 and 0, so every length is 0 and the end-of-block code is missing:
    it is an invalid header here; HCLEN = 5 adds length 8 alone, with which no distance code can be complete (the
    exact path); a single distance code (HDIST = 1) is never complete either.
  * zlib decodes on after the output is full until a symbol needs room: an invalid literal/length or distance code,
    an invalid block header or an end-of-block symbol right after byte ISIZE is still seen (the oracle then reports
    "Expected N decompressed bytes, found N"), while a literal, a complete match or the input's end there is not an
    error.
  * inflate_fallbacks() cannot be read after a failed inflate, so the files that must fail assert the error alone.
"""
import functools
import hashlib
import json
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_writer as dw
from deflate_writer import BitWriter, EOF_BLOCK, bgzf_block
from test_inflate_streams import gpu_result, oracle_result, stored_chain

GOLDEN_DEFLATE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate")

# err: None = inflates to `want` (len(want) == isize); "" = the stream ends before isize bytes (zlib raises nothing);
# else the zlib message.  exact: the payload is outside the wave decoder's common case.
Case = namedtuple("Case", "name payload isize want exact err")


def ok(name, payload, want, exact=False, isize=None):
    isize = len(want) if isize is None else isize
    return Case(name, bytes(payload), isize, bytes(want[:isize]), exact, None)


def bad(name, payload, isize, err):
    return Case(name, bytes(payload), isize, None, True, err)


def rand_tokens(r, n_out, alphabet, start=0, p_match=0.3, max_len=40, max_dist=32768, min_dist=1):
    """Literals from `alphabet` and valid matches producing exactly n_out bytes, `start` bytes of history before them."""
    toks, out = [], start
    end = start + n_out
    while out < end:
        if out >= min_dist and end - out >= 3 and r.random() < p_match:
            ln = int(r.integers(3, min(max_len, end - out) + 1))
            toks.append((ln, int(r.integers(min_dist, min(out, max_dist) + 1))))
            out += ln
        else:
            toks.append(int(alphabet[int(r.integers(len(alphabet)))]))
            out += 1
    return toks


def dyn(tokens, final=True, w=None, lens=None, **kw):
    """One dynamic block of the tokens in complete codes made for them; returns the writer."""
    w = w or BitWriter()
    lit, dist = lens or dw.lens_for(tokens, alt258=kw.get("alt258", False))
    dw.dynamic(w, tokens, final, lit, dist, **kw)
    return w


BASE_ALPHA = np.frombuffer(b"ACGTN#+5?EJ=!:0123456789", np.uint8)


def base_tokens(seed=1, n=700):
    return rand_tokens(np.random.default_rng(seed), n, BASE_ALPHA)


def chain_lens(symbols, n):
    """Lengths 1, 2, ..., k - 1, k - 1 over the k given symbols (a complete code; k = 16 gives 1..14, 15, 15)."""
    lens = [0] * n
    k = len(symbols)
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, k - 1)
    return lens


def batch_walk(syms, cl_lens):
    """The header parser's walk over the code-length symbols, 64 bit offsets at a time: offsets advance by each
    symbol's code + extra bits, a batch ends at the first symbol starting at or past offset 64 (which opens the
    next).  Returns the batches as lists of indices into syms."""
    batches, i = [], 0
    while i < len(syms):
        o, cur = 0, []
        while o < 64 and i < len(syms):
            cur.append(i)
            o += dw.cl_symbol_bits(syms[i], cl_lens)
            i += 1
        batches.append(cur)
    return batches


def is16(s):
    return not isinstance(s, int) and s[0] == 16


def repeat_spans(syms):
    """(symbol, first index, end index) of every code-length symbol over the HLIT + HDIST lengths."""
    n, out = 0, []
    for s in syms:
        rep = 1 if isinstance(s, int) else dw.CL_REP_BASE[s[0]] + s[1]
        out.append((s, n, n + rep))
        n += rep
    return out


# ---- headers, valid ---------------------------------------------------------------------------------------------
def zero_runs_with_16(lens, first):
    """Explicit code-length symbols in which every long zero run is opened by `first` (17 or 18, its shortest form)
    and carried on by a 16 — a 16 that repeats a zero, which no zlib header holds."""
    base = {17: 3, 18: 11}[first]
    out, i = [], 0
    while i < len(lens):
        run = 0
        while i + run < len(lens) and lens[i + run] == 0:
            run += 1
        if run >= base + 3:
            k = min(run - base, 6)
            out += [(first, 0), (16, k - 3)]
            i += base + k
        else:
            out.append(lens[i])
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def headers_valid():
    cases = []
    toks = base_tokens()
    want = dw.expand(toks)
    lit, dist = dw.lens_for(toks)
    for style in ("plain", "zlib", "max"):
        cases.append(ok("cl_style_" + style, dyn(toks, cl_style=style).tobytes(), want))
    # HCLEN 18 (the last code-length-code length sent is symbol 1's) and 19 (symbol 15's); code-length codes of 7 bits
    lit15 = chain_lens([65, 67, 71, 84, 78, 35, 43, 53, 63, 69, 74, 61, 33, 58, 48, 256], 257)
    t15 = rand_tokens(np.random.default_rng(2), 400, np.array([65, 67, 71, 84, 78, 35, 43], np.uint8), p_match=0)
    d15 = [1, 2, 3, 3]
    for hclen, (ll, dl, tk) in ((18, (lit, [1, 1], rand_tokens(np.random.default_rng(3), 300, BASE_ALPHA, max_dist=2))),
                                (19, (lit15, d15, t15))):
        if hclen == 18:
            ll, _ = dw.lens_for(tk)
        syms = dw.cl_symbols(ll, dl, "zlib")
        freqs = [0] * 19
        for s in syms:
            freqs[s if isinstance(s, int) else s[0]] += 1
        # a skewed code: lengths up to 7 for the rare symbols
        used = sorted((s for s in range(19) if freqs[s]), key=lambda s: -freqs[s])
        cl = dw.limited_lengths([(1 << (2 * (len(used) - used.index(s))) if s in used else 0) for s in range(19)], 7)
        w = BitWriter()
        dw.dynamic(w, tk, True, ll, dl, cl_lens=cl, cl_style="zlib")
        need = 18 if hclen == 18 else 19
        got_hclen = max([4] + [i + 1 for i in range(19) if cl[dw.CL_ORDER[i]]])
        assert got_hclen == need and (hclen == 18 or max(cl) == 7), (got_hclen, cl)
        cases.append(ok("hclen_%d" % hclen, w.tobytes(), dw.expand(tk)))
    # HLIT 257 with HDIST 2 (the fewest distance codes a complete set can have); HLIT 286 with HDIST 30
    tk = rand_tokens(np.random.default_rng(4), 300, BASE_ALPHA, p_match=0)  # (HLIT 257: no length symbol)
    l257, d2 = dw.lens_for(tk)
    assert len(l257) == 257 and len(d2) == 2
    cases.append(ok("hlit257_hdist2", dyn(tk, lens=(l257, d2)).tobytes(), dw.expand(tk)))
    l286, d30 = dw.lens_for(toks, n_lit=286, n_dist=30, extra_lit=[285], extra_dist=[29])
    assert len(l286) == 286 and len(d30) == 30 and l286[285] and d30[29]
    for style in ("plain", "max"):
        cases.append(ok("hlit286_hdist30_" + style, dyn(toks, lens=(l286, d30), cl_style=style).tobytes(), want))
    # a 16 right after a 17 / an 18: it repeats a zero
    lz, dz = dw.lens_for(toks, n_lit=286, n_dist=30)
    for first in (17, 18):
        syms = zero_runs_with_16(lz + dz, first)
        assert any(is16(b) and not isinstance(a, int) and a[0] == first for a, b in zip(syms, syms[1:]))
        cases.append(ok("16_after_%d" % first, dyn(toks, lens=(lz, dz), cl_style="explicit", cl_syms=syms).tobytes(),
                        want))
    # chains of consecutive 16s longer than 64 bits of header: 255 literals and the end-of-block code all 8 bits
    tk = [int(b) for b in np.random.default_rng(5).integers(0, 255, 600)]
    l8 = [8] * 255 + [0] + [8]
    w = BitWriter()
    syms, cl = dw.dynamic(w, tk, True, l8, [1, 1], cl_lens=PHASE_CL, cl_style="max")  # (a 16: 2 + 2 bits)
    runs, cur = [], 0
    for s in syms + [0]:
        cur = cur + dw.cl_symbol_bits(s, cl) if is16(s) else (runs.append(cur) or 0)
    assert max(runs) > 128, runs
    cases.append(ok("16_chain", w.tobytes(), dw.expand(tk)))
    # one repeat crossing from the literal/length lengths into the distance lengths: a 16, a 17 and an 18
    for name, sel in (("16", 16), ("17", 17), ("18", 18)):
        if sel == 16:  # the last literal/length lengths (symbols 257..264) and the 16 distance lengths all 4
            tk2 = rand_tokens(np.random.default_rng(6), 400, BASE_ALPHA, max_len=10, max_dist=192)
            fl = [0] * 265
            for s in [t for t in tk2 if isinstance(t, int)] + [256]:
                fl[s] += 1
            ll = [x + 1 if x else 0 for x in dw.limited_lengths(fl, 14)]  # half of the code space
            ll[257:265] = [4] * 8                                          # the other half
            dl = [4] * 16
        else:  # zeros: the unused length symbols at the top, the unused short distances at the bottom
            n_zero = 4 if sel == 17 else 12
            tk2 = rand_tokens(np.random.default_rng(6), 400, BASE_ALPHA, max_dist=300, min_dist=dw.DIST_BASE[n_zero])
            top = max(dw.token_symbols(tk2)[0]) + 1
            ll, dl = dw.lens_for(tk2, n_lit=top + 3 if sel == 17 else 286, extra_dist=[n_zero])
            assert ll[top - 1] and not any(ll[top:]) and not any(dl[:n_zero]) and dl[n_zero]
        w = BitWriter()
        syms, _ = dw.dynamic(w, tk2, True, ll, dl, cl_style="max")
        cross = [s for s, a, b in repeat_spans(syms) if a < len(ll) < b]
        assert len(cross) == 1 and cross[0][0] == sel, (sel, cross)
        cases.append(ok("cross_hlit_" + name, w.tobytes(), dw.expand(tk2)))
    return cases


PHASE_CL = [0] * 19
for _s, _l in ((8, 1), (16, 2), (0, 3), (1, 3)):
    PHASE_CL[_s] = _l


def phase_syms(k):
    """k one-bit code-length symbols (length 8), then x = 8 and 16s repeating it up to literal 254; literal 255 unused,
    the end-of-block code 8 bits; two 1-bit distance codes."""
    syms = [8] * k + [8]
    n = k + 1
    while n < 255:
        rep = min(6, 255 - n)
        if rep < 3:
            syms += [8] * rep
        else:
            syms.append((16, rep - 3))
        n += rep
    return syms + [0, 8, 1, 1]


@functools.lru_cache(maxsize=None)
def header_phase():
    """A 16 as the first code-length symbol of a 64-bit batch of the header parser (its `prev` carry), at every phase."""
    cases = []
    tk = [int(b) for b in np.random.default_rng(7).integers(0, 255, 200)]  # (HLIT 257: literals only)
    want = dw.expand(tk)
    lit = [8] * 255 + [0, 8]
    opens, after_literal = [], []
    for k in range(64):
        syms = phase_syms(k)
        assert [b - a for _, a, b in repeat_spans(syms)] and repeat_spans(syms)[-1][2] == 259
        w = BitWriter()
        dw.dynamic(w, tk, True, lit, [1, 1], cl_lens=PHASE_CL, cl_style="explicit", cl_syms=syms)
        cases.append(ok("phase_%d" % k, w.tobytes(), want))
        for b in batch_walk(syms, PHASE_CL)[1:]:
            if is16(syms[b[0]]):
                opens.append(k)
                if isinstance(syms[b[0] - 1], int):
                    after_literal.append(k)
    # the coverage condition: a 16 opens a batch (the symbol before it lies in the previous batch: the carry), both
    # after another 16 (the carried value is itself a repeated one) and right after the literal length x
    assert opens and after_literal and set(opens) - set(after_literal), (opens, after_literal)
    return cases


# ---- headers, invalid ---------------------------------------------------------------------------------------------
def _hdr(lit, dist, pad=8, **kw):
    w = BitWriter()
    dw.dynamic(w, [], True, lit, dist, end=False, **kw)
    return w.tobytes() + b"\x00" * pad


@functools.lru_cache(maxsize=None)
def headers_invalid():
    toks = base_tokens(8, 300)
    lit, dist = dw.lens_for(toks)
    n = 300
    cl_all = dw.limited_lengths([3] * 19, 7)
    plain = list(lit) + list(dist)
    cases = [
        bad("16_first", _hdr(lit, dist, cl_lens=cl_all, cl_style="explicit", cl_syms=[(16, 0)] + plain[3:]), n,
            "invalid bit length repeat"),
        bad("repeat_overrun", _hdr(lit, dist, cl_lens=cl_all, cl_style="explicit", cl_syms=plain[:-2] + [(18, 0)]), n,
            "invalid bit length repeat"),
        bad("repeat_overrun_16", _hdr(lit, dist, cl_lens=cl_all, cl_style="explicit", cl_syms=plain[:-2] + [(16, 0)]),
            n, "invalid bit length repeat"),
    ]
    for f in (30, 31):
        cases.append(bad("hlit_field_%d" % f, _hdr(lit + [0] * (257 + f - len(lit)), dist, cl_lens=cl_all), n,
                         "too many length or distance symbols"))
        cases.append(bad("hdist_field_%d" % f, _hdr(lit, dist + [0] * (f + 1 - len(dist)), cl_lens=cl_all), n,
                         "too many length or distance symbols"))
    inc = [0] * 19
    inc[0], inc[8], inc[7] = 1, 2, 3  # 1/2 + 1/4 + 1/8 < 1
    one = [0] * 19
    one[0] = 1
    over = [0] * 19
    over[0], over[8], over[7] = 1, 1, 1
    for name, cl in (("cl_incomplete", inc), ("cl_single_1bit", one), ("cl_oversubscribed", over)):
        cases.append(bad(name, _hdr(lit, dist, cl_lens=cl, cl_style="explicit", cl_syms=[]), n,
                         "invalid code lengths set"))
    # HCLEN 4: only 16, 17, 18 and 0 have code-length codes, so all 258 lengths are zeros
    cl4 = [0] * 19
    cl4[18], cl4[0] = 1, 1
    w = BitWriter()
    dw.dynamic(w, [], True, [0] * 257, [0], cl_lens=cl4, cl_style="explicit", cl_syms=[(18, 127), (18, 109)], hclen=4,
               end=False)
    cases.append(bad("hclen_4", w.tobytes() + bytes(8), n, "invalid code -- missing end-of-block"))
    lo = list(lit)
    lo[[s for s in range(256) if lit[s] > 1][0]] -= 1  # one code shortened: over-subscribed
    cases.append(bad("lit_oversubscribed", _hdr(lo, dist), n, "invalid literal/lengths set"))
    li = list(lit)
    li[[s for s in range(256) if lit[s]][0]] += 1  # one code lengthened: incomplete, more than one code
    cases.append(bad("lit_incomplete", _hdr(li, dist), n, "invalid literal/lengths set"))
    ln = list(lit)
    ln[[s for s in range(256) if not lit[s]][0]] = lit[256]
    ln[256] = 0  # the same complete code without an end-of-block code
    cases.append(bad("no_end_of_block", _hdr(ln, dist), n, "invalid code -- missing end-of-block"))
    cases.append(bad("dist_oversubscribed", _hdr(lit, [1, 1, 1]), n, "invalid distances set"))
    cases.append(bad("dist_incomplete", _hdr(lit, [1, 2]), n, "invalid distances set"))
    return cases


# ---- accepted oddities ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oddities():
    r = np.random.default_rng(9)
    lits = [int(b) for b in BASE_ALPHA[r.integers(0, len(BASE_ALPHA), 500)]]
    lit, _ = dw.lens_for(lits + [(5, 1), (258, 1), (3, 1)])
    codes = dw.canonical_codes(lit)
    cases = [ok("one_dist_code_unused", dyn(lits, lens=(lit, [1])).tobytes(), bytes(lits), exact=True)]
    tk = lits + [(5, 1), 65, (258, 1), (3, 1)] + lits[:50]
    cases.append(ok("one_dist_code_used", dyn(tk, lens=(lit, [1])).tobytes(), dw.expand(tk), exact=True))
    w = BitWriter()
    dw.dynamic(w, lits, True, lit, [1], end=False)
    w.code(*codes[259])
    w.code(1, 1)  # the unassigned half of the 1-bit distance code
    w.put(0, 32)
    cases.append(bad("one_dist_code_unassigned", w.tobytes(), 600, "invalid distance code"))
    cases.append(ok("no_dist_code_literals", dyn(lits, lens=(lit, [0])).tobytes(), bytes(lits), exact=True))
    w = BitWriter()
    dw.dynamic(w, lits, True, lit, [0], end=False)
    w.code(*codes[259])
    w.put(0, 32)
    cases.append(bad("no_dist_code_length", w.tobytes(), 600, "invalid distance code"))
    # HCLEN 5: the code-length symbols 0 and 8 only (every code 8 bits), hence no distance code
    l8 = [8] * 255 + [0, 8]
    cl5 = [0] * 19
    cl5[0], cl5[8] = 1, 1
    b255 = [b % 255 for b in lits]
    w = BitWriter()
    dw.dynamic(w, b255, True, l8, [0], cl_lens=cl5, cl_style="plain")
    cases.append(ok("hclen_5", w.tobytes(), bytes(b255), exact=True))
    # an empty dynamic block whose literal/length code is a single 1-bit end-of-block code: first, last
    eob_only = [0] * 256 + [1]
    w = BitWriter()
    dw.dynamic(w, [], False, eob_only, [0])
    dyn(lits, w=w)
    cases.append(ok("empty_block_first", w.tobytes(), bytes(lits), exact=True))
    w = dyn(lits, final=False)
    dw.dynamic(w, [], True, eob_only, [0])
    cases.append(ok("empty_block_last", w.tobytes(), bytes(lits), exact=True))
    return cases


# ---- tables ---------------------------------------------------------------------------------------------------------
# code-length counts (lengths 1..15) of the complete codes with the largest sub-table totals at a 9-bit root, found
# by a dynamic program over (length, symbols left, codes left): they reach zlib's ENOUGH bounds exactly
MAX_SUB_LIT = [0, 3, 0, 0, 0, 0, 0, 0, 0, 233, 45, 1, 1, 1, 2]   # 286 symbols, 340 sub-table entries
MAX_SUB_DIST = [0, 3, 1, 1, 1, 1, 0, 0, 0, 13, 5, 1, 1, 1, 2]    # 30 symbols, 80 sub-table entries


def mostly_15_counts(n):
    """Counts per length (1..15) of a complete code over exactly n symbols with as many 15-bit codes as possible: the
    rest of the code space as the fewest shorter codes, the smallest of them halved until the symbols are used up."""
    n15 = max(k for k in range(2, n, 2) if bin(32768 - k).count("1") <= n - k)
    terms = [i for i in range(15) if (32768 - n15) >> i & 1]  # log2 of each short code's share, in 2^-15 units
    while len(terms) < n - n15:
        t = min(x for x in terms if x > 0)
        terms.remove(t)
        terms += [t - 1, t - 1]
    return [terms.count(15 - l) + (n15 if l == 15 else 0) for l in range(1, 16)]


def lens_from_counts(counts, order):
    """Assign the lengths (counts[l - 1] codes of l bits) to the symbols in `order`, shortest first."""
    seq = [l + 1 for l, c in enumerate(counts) for _ in range(c)]
    lens = [0] * len(order)
    for s, l in zip(order, seq):
        lens[s] = l
    return lens


@functools.lru_cache(maxsize=None)
def far_tokens():
    """> 32 KiB of output, then every length code and every distance code with its extra bits all-zero and all-one,
    the first of the distance-32768 matches exactly 32768 bytes in.  Every literal/length and distance symbol occurs."""
    r = np.random.default_rng(10)
    toks = [int(b) for b in r.permutation(256)]
    toks += rand_tokens(r, 32768 - 256, np.arange(256), start=256, p_match=0.6, max_len=258)
    assert len(dw.expand(toks)) == 32768
    toks.append((3, 32768))
    for k in range(30):
        for d in {dw.DIST_BASE[k], dw.DIST_BASE[k] + (1 << dw.DIST_EXTRA[k]) - 1}:
            toks.append((3 + k, d))
    for k in range(29):
        for ln in {dw.LEN_BASE[k], dw.LEN_BASE[k] + (1 << dw.LEN_EXTRA[k]) - 1}:
            toks.append((ln, int(r.integers(1, 32769))))
    return toks


@functools.lru_cache(maxsize=None)
def tables():
    cases = []
    r = np.random.default_rng(11)
    # lengths 1, 2, ..., 14, 15, 15 for both alphabets
    lsyms = [65, 67, 71, 84, 78, 35, 43, 53, 63, 69, 74, 256, 257, 260, 270, 285]
    lit = chain_lens(lsyms, 286)
    dist = chain_lens(list(range(16)), 16)
    assert sorted(x for x in lit if x) == sorted(x for x in dist if x) == list(range(1, 15)) + [15, 15]
    tk = [int(b) for b in r.choice([s for s in lsyms if s < 256], 400)]
    for ln in (3, 6, 24, 258):
        for d in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256):
            tk.append((ln, d))
            tk.append(int(r.choice([65, 67, 74])))
    assert set(dw.token_symbols(tk)[1]) == set(range(16))
    cases.append(ok("chain_1_to_15", dyn(tk, lens=(lit, dist)).tobytes(), dw.expand(tk)))
    # the largest sub-table totals: the long codes go to the symbols far_tokens uses least
    ft = far_tokens()
    ls, ds = dw.token_symbols(ft)
    fl = np.bincount(ls + [256], minlength=286)
    fd = np.bincount(ds, minlength=30)
    assert fl.min() > 0 and fd.min() > 0  # every symbol of both alphabets is on the path
    lit = lens_from_counts(MAX_SUB_LIT, [int(s) for s in np.argsort(-fl, kind="stable")])
    dist = lens_from_counts(MAX_SUB_DIST, [int(s) for s in np.argsort(-fd, kind="stable")])
    assert dw.kraft(lit) == dw.kraft(dist) == 1 << 15
    assert dw.subtable_total(lit) == 340 and dw.subtable_total(dist) == 80  # == kLitSub, kDistSub: the ENOUGH bounds
    cases.append(ok("max_subtables", dyn(ft, lens=(lit, dist), cl_style="max").tobytes(), dw.expand(ft)))
    # every used symbol 15 bits, except the few short ones that complete the code
    lit = lens_from_counts(mostly_15_counts(286), [int(s) for s in np.argsort(-fl, kind="stable")])
    dist = lens_from_counts(mostly_15_counts(30), [int(s) for s in np.argsort(-fd, kind="stable")])
    assert dw.kraft(lit) == dw.kraft(dist) == 1 << 15 and min(lit) > 0 and min(dist) > 0
    assert lit.count(15) >= 270 and dist.count(15) >= 16
    assert dw.subtable_total(lit) <= 340 and dw.subtable_total(dist) <= 80
    cases.append(ok("all_15_bits", dyn(ft, lens=(lit, dist)).tobytes(), dw.expand(ft)))
    return cases


def segment_bits(left_bits, final):
    """k_inflate_wave's round sizing: the bits each of the 64 lanes takes per round of a DEFLATE block whose data
    runs for left_bits to the payload's end (a non-final block's rounds are sized to 93 % of that)."""
    left = left_bits if final else left_bits * 930 // 1000
    nr = -(-left // (64 * 544))
    return min(544, max(32, (-(-left // (64 * nr)) + 31) & ~31)) if nr > 0 else 544


@functools.lru_cache(maxsize=None)
def dense_symbols():
    """Segments holding hundreds of symbols: a literal and the end-of-block code of 1 bit each, and 2-bit codes."""
    cases = []
    one = [0] * 257
    one[65] = one[256] = 1
    for name, n in (("1bit_60000", 60000), ("1bit_544_per_segment", 64 * 544 - 40)):
        w = BitWriter()
        dw.dynamic(w, [65] * n, True, one, [1, 1])
        hdr = w.nbits - n - 1
        seg = segment_bits(8 * len(w.tobytes()) - hdr, True)
        assert seg >= 480 and (n == 60000 or seg == 544), seg  # symbols per lane segment (1 bit each)
        cases.append(ok(name, w.tobytes(), b"A" * n))
    two = [0] * 257
    two[65] = two[67] = two[71] = two[256] = 2
    tk = [int(b) for b in np.random.default_rng(12).choice([65, 67, 71], 60000)]
    w = BitWriter()
    dw.dynamic(w, tk, True, two, [1, 1])
    assert segment_bits(2 * 60000, True) // 2 >= 224
    cases.append(ok("2bit_60000", w.tobytes(), bytes(tk)))
    return cases


# ---- data symbols ---------------------------------------------------------------------------------------------------
def both(name, tokens, alt258=False):
    want = dw.expand(tokens)
    w = BitWriter()
    dw.fixed(w, tokens, True, alt258=alt258)
    return [ok(name + "_fixed", w.tobytes(), want), ok(name + "_dynamic", dyn(tokens, alt258=alt258).tobytes(), want)]


@functools.lru_cache(maxsize=None)
def data_symbols():
    r = np.random.default_rng(13)
    ft = far_tokens()
    # the coverage condition, counted from the token list: every length and distance code at both extra-bit extremes
    # (symbol 284's all-one extra is length 258: only the 284 + 31 spelling writes it)
    lens_seen = {dw.length_symbol(t[0], alt)[:2] for t in ft if not isinstance(t, int) for alt in (False, True)}
    dist_seen = {dw.distance_symbol(t[1])[:2] for t in ft if not isinstance(t, int)}
    for k in range(29):
        assert {(257 + k, 0), (257 + k, (1 << dw.LEN_EXTRA[k]) - 1)} <= lens_seen, k
    for k in range(30):
        assert {(k, 0), (k, (1 << dw.DIST_EXTRA[k]) - 1)} <= dist_seen, k
    out = 0
    for i, t in enumerate(ft):
        if t == (3, 32768):
            assert out == 32768  # distance 32768 from exactly 32768 bytes in
            break
        out += 1 if isinstance(t, int) else t[0]
    cases = both("every_code", ft) + both("every_code_284", ft, alt258=True)
    # length 258 as symbol 284 + 31 extra
    tk = [65, 66, 67] + [(258, 1), (258, 3), 68, (258, 2), (257, 1), (258, 259)] * 8
    assert 285 not in dw.token_symbols(tk, alt258=True)[0] and dw.length_symbol(258, True) == (284, 31, 5)
    cases += both("len258_as_284", tk, alt258=True)
    # length-3 matches at every distance 24577..32768
    tk = rand_tokens(r, 32768, np.arange(256), p_match=0.7, max_len=258)
    tk += [(3, int(d)) for d in r.permutation(np.arange(24577, 32769))]
    cases += both("len3_far", tk)
    # overlapping copies: distances 1..16 x lengths {3, 4, 15, 16, 17, 257, 258}
    tk = [int(b) for b in r.integers(0, 256, 16)]
    for d in range(1, 17):
        for ln in (3, 4, 15, 16, 17, 257, 258):
            tk += [(ln, d), int(r.integers(0, 256))]
    cases += both("overlap", tk)
    return cases


@functools.lru_cache(maxsize=None)
def widest_symbols():
    """Back-to-back 48-bit matches (15-bit length code + 5 extra, 15-bit distance code + 13 extra) starting at every
    bit phase of a dword: 0..31 one-bit literals in front of them."""
    lit = chain_lens([65, 256, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 283, 284], 286)
    dist = chain_lens(list(range(14, 30)), 30)
    assert lit[65] == 1 and lit[284] == lit[283] == 15 and dist[29] == dist[28] == 15
    r = np.random.default_rng(14)
    head = [65] * 200 + [(257, 129 + i % 64) for i in range(130)]
    n0 = len(dw.expand(head))
    assert n0 >= 32768
    cases = []
    for k in range(32):
        tk = head + [65] * k
        for i in range(40):
            ln = (195, 226, 227, 257)[i % 4] if i % 3 else int(r.integers(195, 258))
            d = (16385, 24576, 24577, 32768)[i % 4] if i % 5 else int(r.integers(16385, 32769))
            tk.append((ln, d))
        assert all(dw.LEN_EXTRA[dw.length_symbol(t[0])[0] - 257] == 5 and dw.DIST_EXTRA[dw.distance_symbol(t[1])[0]] == 13
                   for t in tk[-40:])
        cases.append(ok("phase_%d" % k, dyn(tk, lens=(lit, dist)).tobytes(), dw.expand(tk)))
    return cases


@functools.lru_cache(maxsize=None)
def data_invalid():
    cases = []
    lits = [int(b) for b in np.random.default_rng(15).integers(0, 144, 300)]
    n = len(lits)
    for name, tok, msg in (("lit_286", ("sym", 286), "invalid literal/length code"),
                           ("lit_287", ("sym", 287), "invalid literal/length code"),
                           ("dist_30", ("rawdist", 3, 30, 0), "invalid distance code"),
                           ("dist_31", ("rawdist", 258, 31, 0), "invalid distance code")):
        w = BitWriter()
        dw.fixed(w, lits + [tok] + lits, True)
        cases.append(bad(name, w.tobytes(), 2 * n, msg))
        # the same symbol right after byte ISIZE: zlib decodes it before it looks for room, and reports it
        cases.append(bad(name + "_at_isize", w.tobytes(), n, msg))
        # ... and one literal further on, where zlib stops for room and never sees it
        w = BitWriter()
        dw.fixed(w, lits + [65, tok] + lits, True)
        cases.append(ok(name + "_past_isize", w.tobytes(), bytes(lits), exact=True))
    # a match reaching one byte before the payload's first output byte, from a dynamic block
    tk = lits + [(4, n + 1)] + lits
    w = BitWriter()
    lit, dist = dw.lens_for(tk)
    dw.dynamic(w, tk, True, lit, dist)
    cases.append(bad("too_far_back_dynamic", w.tobytes(), 2 * n + 4, "invalid distance too far back"))
    tk = lits + [(4, n)] + lits  # (exactly to the first byte: valid)
    cases.append(ok("back_to_first_byte", dyn(tk).tobytes(), dw.expand(tk)))
    return cases


# ---- block structure ------------------------------------------------------------------------------------------------
FIRST_SHARES = (0.01, 0.5, 0.93, 0.999)


def split_payload(tokens, share):
    """A non-final dynamic block with the first n1 tokens and a final block with the rest, n1 chosen so that the
    first block is `share` of the payload's bits; returns (payload, achieved share)."""
    n1 = int(len(tokens) * share)
    for _ in range(12):
        w = dyn(tokens[:n1], final=False)
        b1 = w.nbits
        rest = tokens[n1:]
        if share > 0.99:
            dw.fixed(w, rest, True)  # (a dynamic header alone would be more than the 0.1 % left)
        else:
            lit, dist = dw.lens_for(rest)
            dw.dynamic(w, rest, True, lit, dist)
        p = w.tobytes()
        got = b1 / (8 * len(p))
        if abs(got - share) < 0.002 or (share > 0.99 and abs(got - share) < 0.0005):
            break
        n1 = max(1, min(len(tokens) - 1, int(round(n1 * share / got))))
    return p, got


@functools.lru_cache(maxsize=None)
def block_structure():
    r = np.random.default_rng(16)
    cases = []
    big = [int(b) for b in BASE_ALPHA[r.integers(0, len(BASE_ALPHA), 65280)]]
    cases.append(ok("one_block_65280_literals", dyn(big).tobytes(), bytes(big)))
    # 200 tiny dynamic blocks (matches reach back into the earlier blocks' output)
    w, alltk = BitWriter(), []
    for i in range(200):
        tk = rand_tokens(r, int(r.integers(15, 40)), BASE_ALPHA, start=len(dw.expand(alltk)) if i % 20 == 0 else 0,
                         max_len=6)
        tk = [t if isinstance(t, int) or t[1] <= 15 * i + 1 else 65 for t in tk] if i % 20 else tk
        dyn(tk, final=i == 199, w=w)
        alltk += tk
    cases.append(ok("200_tiny_blocks", w.tobytes(), dw.expand(alltk)))
    # 100 empty fixed blocks, then data
    w = BitWriter()
    for _ in range(100):
        dw.fixed(w, [], False)
    tk = base_tokens(17, 2000)
    dyn(tk, w=w)
    cases.append(ok("100_empty_fixed_then_data", w.tobytes(), dw.expand(tk)))
    # fixed, dynamic and empty blocks interleaved
    w, alltk = BitWriter(), []
    for i in range(30):
        tk = [] if i % 3 == 2 else rand_tokens(r, int(r.integers(1, 900)), BASE_ALPHA, start=len(dw.expand(alltk)))
        if (i + i // 3) % 2:
            dw.fixed(w, tk, i == 29)
        else:
            dyn(tk, final=i == 29, w=w)
        alltk += tk
    cases.append(ok("interleaved", w.tobytes(), dw.expand(alltk)))
    # a non-final first block of 1 %, 50 %, 93 % and 99.9 % of the payload's bits
    tk = rand_tokens(r, 65280, BASE_ALPHA, p_match=0.15, max_len=12)
    for share in FIRST_SHARES:
        p, got = split_payload(tk, share)
        assert abs(got - share) < 0.01 and (share < 0.99 or 0.998 < got < 1), (share, got)  # within a point
        cases.append(ok("first_block_%g" % share, p, dw.expand(tk)))
    # Huffman, then stored, then Huffman again (the exact decoder)
    a, c = base_tokens(18, 500), base_tokens(19, 500)
    raw = r.integers(0, 256, 777, dtype=np.uint8).tobytes()
    w = dyn(a, final=False)
    dw.stored(w, raw, False)
    dyn(c, w=w)
    cases.append(ok("huffman_stored_huffman", w.tobytes(), dw.expand(a) + raw + dw.expand(c), exact=True))
    # trailing garbage after the final block
    cases.append(ok("trailing_garbage", dyn(a).tobytes() + bytes(r.integers(0, 256, 37, dtype=np.uint8)), dw.expand(a)))
    return cases


# ---- ISIZE semantics ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def isize_semantics():
    cases = []
    tk = base_tokens(20, 900)
    tk = tk if isinstance(tk[-1], int) else tk + [65]  # (the last byte a literal: ISIZE - 1 stops in front of it)
    want = dw.expand(tk)
    p = dyn(tk).tobytes()
    cases.append(ok("isize_minus_1", p, want, exact=True, isize=len(want) - 1))
    cases.append(bad("isize_plus_1", p, len(want) + 1, ""))
    # a payload cut in the middle of a 48-bit symbol
    lit = chain_lens([65, 256, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 283, 284], 286)
    dist = chain_lens(list(range(14, 30)), 30)
    head = [65] * 200 + [(257, 129)] * 130
    w = BitWriter()
    dw.dynamic(w, head + [66] * 5, True, lit, dist, end=False)
    cut = w.nbits + 24
    dw.put_tokens(w, [(257, 32768), 65], dw.canonical_codes(lit), dw.canonical_codes(dist))
    assert w.nbits - cut > 24
    full = dw.expand(head + [66] * 5 + [(257, 32768), 65])
    cases.append(bad("cut_mid_symbol", w.tobytes()[:cut // 8], len(full), ""))
    # the final block ends exactly at ISIZE and the bytes after it look like a non-final dynamic header
    nxt = dyn(tk[:50], final=False).tobytes()
    cases.append(ok("final_then_header", dyn(tk).tobytes() + nxt, want))
    # a non-final block ends exactly at ISIZE: an empty final block follows (the stream ends there) ...
    w = dyn(tk, final=False)
    dw.fixed(w, [], True)
    cases.append(ok("nonfinal_at_isize_empty_final", w.tobytes(), want))
    # ... or more data (the stream runs past ISIZE: zlib stops at the next block's first literal) ...
    w = dyn(tk, final=False)
    dyn([65] + tk[:100], w=w)
    cases.append(ok("nonfinal_at_isize_more_data", w.tobytes(), want, exact=True))
    # ... or an invalid block type, which zlib reads before it looks for room
    w = dyn(tk, final=False)
    w.put(0, 1)
    w.put(3, 2)
    w.put(0, 32)
    cases.append(bad("nonfinal_at_isize_bad_type", w.tobytes(), len(want), "invalid block type"))
    return cases


@functools.lru_cache(maxsize=None)
def after_isize():
    """What follows byte ISIZE: zlib decodes on until a symbol needs room, so invalid input right there is an error
    (ISIZE bytes found) and anything that merely wants to write is not."""
    lits = [int(b) for b in np.random.default_rng(23).integers(0, 144, 300)]
    n = len(lits)
    bad_sym = ("sym", 286)

    def fx(tokens, final=True, w=None, end=True):
        w = w or BitWriter()
        dw.fixed(w, tokens, final, end=end)
        return w

    cases = []
    # a match after the last byte: complete, so zlib stops for room (even one that reaches too far back) ...
    cases.append(ok("match_after", fx(lits + [(3, 1), bad_sym]).tobytes(), bytes(lits), exact=True))
    cases.append(ok("far_match_after", fx(lits + [(3, 32768), bad_sym]).tobytes(), bytes(lits), exact=True))
    # ... the last byte written by a match that ends exactly there, or is cut short there (still pending: zlib stops)
    tk = lits + [(10, 7)]
    cases.append(bad("match_ends_at_isize", fx(tk + [bad_sym]).tobytes(), n + 10, "invalid literal/length code"))
    cases.append(ok("match_cut_at_isize", fx(tk + [bad_sym]).tobytes(), dw.expand(tk), exact=True, isize=n + 9))
    # the input ends right after the block that wrote byte ISIZE (no final block)
    cases.append(ok("input_ends", fx(lits, final=False).tobytes(), bytes(lits), exact=True))
    b0 = fx(lits, end=False).nbits  # (1..8 bits of a 9-bit literal code follow the last byte's symbol)
    cases.append(ok("input_ends_mid_symbol", fx(lits + [200], end=False).tobytes()[:b0 // 8 + 1], bytes(lits),
                    exact=True))
    # end-of-block symbols and headers after byte ISIZE, then: stored data, a bad stored header, a bad dynamic header
    w = fx(lits, final=False)
    dw.fixed(w, [], False)
    dw.stored(w, b"xyz", True)
    cases.append(ok("then_stored_data", w.tobytes(), bytes(lits), exact=True))
    w = fx(lits, final=False)
    dw.stored(w, b"", False)
    dw.stored(w, b"", False)
    dw.fixed(w, [], True)
    cases.append(ok("then_empty_stored_to_the_end", w.tobytes(), bytes(lits), exact=True))
    w = fx(lits, final=False)
    dw.stored(w, b"", False)
    p = bytearray(w.tobytes())
    p[-1] ^= 1  # NLEN
    cases.append(bad("then_bad_stored_lengths", bytes(p) + bytes(4), n, "invalid stored block lengths"))
    w = fx(lits, final=False)
    lit, dist = dw.lens_for(lits)
    dw.dynamic(w, [], True, lit, dist, cl_lens=dw.limited_lengths([3] * 19, 7), cl_style="explicit",
               cl_syms=[(16, 0)] + (list(lit) + list(dist))[3:], end=False)
    cases.append(bad("then_bad_dynamic_header", w.tobytes() + bytes(8), n, "invalid bit length repeat"))
    w = fx(lits, final=False)
    dyn([], final=False, w=w)
    dw.fixed(w, [bad_sym], True)
    cases.append(bad("then_blocks_then_bad_symbol", w.tobytes(), n, "invalid literal/length code"))
    # a stored block after Huffman output that ends exactly at ISIZE, then an invalid block type; or with data left
    w = fx(lits[:100], final=False)
    dw.stored(w, bytes(lits[100:]), False)
    w.put(3 << 1, 3)
    w.put(0, 32)
    cases.append(bad("stored_ends_at_isize_bad_type", w.tobytes(), n, "invalid block type"))
    cases.append(ok("stored_cut_at_isize", w.tobytes(), bytes(lits), exact=True, isize=n - 1))
    return cases


GROUPS = {f.__name__: f for f in (after_isize, headers_valid, header_phase, headers_invalid, oddities, tables, dense_symbols,
                                  data_symbols, widest_symbols, data_invalid, block_structure, isize_semantics)}


def good_payload():
    tk = base_tokens(21, 300)
    return dyn(tk).tobytes(), len(dw.expand(tk))


def group_files(name):
    """(file name, BGZF bytes, payloads on the exact path or None for a file that must fail): the group's valid
    fast-path payloads in one file, its valid exact-path payloads in another, and one file per failing payload (a good
    payload on each side of it)."""
    cases = GROUPS[name]()
    files = []
    for exact in (False, True):
        sel = [c for c in cases if c.err is None and c.exact == exact]
        if sel:
            data = b"".join(bgzf_block(c.payload, c.isize) for c in sel) + EOF_BLOCK
            files.append(("exact" if exact else "fast", data, len(sel) if exact else 0))
    g, gn = good_payload()
    for c in cases:
        if c.err is not None:
            files.append((c.name, bgzf_block(g, gn) + bgzf_block(c.payload, c.isize) + bgzf_block(g, gn) + EOF_BLOCK,
                          None))
    return files


@pytest.mark.parametrize("group", GROUPS)
def test_streams_against_zlib_and_oracle(group):
    """The writer's streams pinned on the CPU: zlib inflates each valid one to expand(tokens) (stopping at ISIZE) and
    raises the expected message for each invalid one; the oracle agrees on the files the GPU tests use."""
    cases = GROUPS[group]()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.payload) <= 65000 and 0 < c.isize <= 65280, c.name
        d = zlib.decompressobj(-15)
        if c.err is None:
            assert len(c.want) == c.isize and d.decompress(c.payload, c.isize) == c.want, c.name
        elif c.err == "":
            assert len(d.decompress(c.payload, c.isize)) < c.isize, c.name
        else:
            with pytest.raises(zlib.error, match=re.escape(c.err)):
                d.decompress(c.payload, c.isize)
    by_name = {c.name: c for c in cases}
    for fname, data, exact in group_files(group):
        kind, out = oracle_result(data)
        assert len(data) < 4 << 20
        if exact is None:
            c = by_name[fname]
            assert kind == "error" and out.startswith("Expected %d decompressed bytes, found " % c.isize), (fname, out)
        else:
            want = b"".join(c.want for c in cases if c.err is None and c.exact == (fname == "exact"))
            assert kind == "ok" and out == want, fname


def test_writer_primitives():
    """put is LSB-first and code MSB-first; limited_lengths gives complete codes within the limit; a stream written
    with zlib's own choices inflates."""
    w = BitWriter()
    w.put(0b101, 3)
    w.code(0b110, 3)
    w.put(0x1ff, 9)
    assert w.nbits == 15 and w.bits == [1, 0, 1, 1, 1, 0] + [1] * 9 and w.tobytes() == bytes([0xdd, 0x7f])
    r = np.random.default_rng(0)
    for max_len in (3, 7, 15):
        for n in (2, 3, 8, 19, 30, 286):
            if n > (1 << max_len):
                continue
            for _ in range(20):
                f = [int(x) for x in r.integers(0, 1000, n) * (r.random(n) < 0.7)]
                f[0] += 1
                f[n - 1] += 1
                lens = dw.limited_lengths(f, max_len)
                assert dw.kraft(lens, max_len) == 1 << max_len and max(lens) <= max_len
                assert all((l > 0) == (x > 0) for l, x in zip(lens, f))
            lens = dw.limited_lengths([1 << min(i, 40) for i in range(n)], max_len)  # Huffman's depth far past max_len
            assert dw.kraft(lens, max_len) == 1 << max_len and max(lens) <= max_len
    assert dw.limited_lengths([0, 7, 0], 7) == [1, 1, 0]
    assert dw.canonical_codes([2, 1, 3, 3]) == {1: (0, 1), 0: (2, 2), 2: (6, 3), 3: (7, 3)}  # RFC 1951 3.2.2
    assert dw.subtable_total([1, 2, 3] + [10] * 128, root=9) == 128 and dw.subtable_total(dw.FIXED_LIT_LENS) == 0
    tk = base_tokens(22, 5000)
    for style in ("plain", "zlib", "max"):
        assert zlib.decompress(dyn(tk, cl_style=style).tobytes(), -15) == dw.expand(tk)
    w = BitWriter()
    dw.stored(w, b"abc", False)
    dw.fixed(w, [(3, 3), 100], True)
    assert zlib.decompress(w.tobytes(), -15) == b"abcabcd"
    assert dw.expand([1, 2, (5, 2), (3, 1)]) == bytes([1, 2, 1, 2, 1, 2, 1, 1, 1, 1])
    assert dw.walk_blocks(w.tobytes()) == [("stored", 3), ("fixed", 4)]
    by_name = {c.name: c for c in block_structure()}
    assert dw.walk_blocks(by_name["huffman_stored_huffman"].payload) == [("dynamic", 500), ("stored", 777), ("dynamic", 500)]
    assert [k for k, _ in dw.walk_blocks(by_name["100_empty_fixed_then_data"].payload)] == ["fixed"] * 100 + ["dynamic"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_foreign_streams(group):
    """Bytes (or the error) equal to the oracle's on every file of the group, and the decoder path: no fallback on a
    fast-path file, one per payload on an exact-path file."""
    import sbam
    wrong = []
    for fname, data, exact in group_files(group):
        want = oracle_result(data)
        got = gpu_result(data)
        if got != want:
            wrong.append((fname, got[0], got[1] if got[0] == "error" else len(got[1]), want[0],
                          want[1] if want[0] == "error" else len(want[1])))
        elif exact is not None:
            g = sbam.BamFile(data, inflate=False)
            try:
                g.inflate()
                n = g.inflate_fallbacks()
            finally:
                g.close()
            print(group, fname, "fallbacks", n, "expected", exact)
            if n != exact:
                wrong.append((fname, "fallbacks", n, "expected", exact))
    assert not wrong, wrong


# ---- the libdeflate-written corpus ----------------------------------------------------------------------------------
def corpus_manifest():
    with open(os.path.join(GOLDEN_DEFLATE, "corpus.json")) as f:
        return json.load(f)


def corpus_bytes(name):
    with open(os.path.join(GOLDEN_DEFLATE, name), "rb") as f:
        return f.read()


def bgzf_payloads(data):
    """(payload, ISIZE) of every block of a BGZF file written by bgzf_block."""
    out, pos = [], 0
    while pos < len(data):
        bsize = int.from_bytes(data[pos + 16:pos + 18], "little") + 1
        out.append((data[pos + 18:pos + bsize - 8], int.from_bytes(data[pos + bsize - 4:pos + bsize], "little")))
        pos += bsize
    return out


def corpus_exact_payloads(data):
    """The payloads of a corpus file that k_inflate_wave hands to the exact decoder: those with a stored block that
    are not stored blocks only (libdeflate level 12 writes the far-repeat buffer's random stretch as a stored block
    between two dynamic ones — a shape worth keeping; every other payload here is dynamic blocks alone)."""
    n = 0
    for p, isize in bgzf_payloads(data):
        if isize:
            kinds = [k for k, _ in dw.walk_blocks(p)]
            assert stored_chain(p) == (set(kinds) == {"stored"}) and (((p[0] >> 1) & 3) == 0) == (kinds[0] == "stored")
            n += "stored" in kinds and not stored_chain(p)
    return n


def test_corpus_oracle_and_regeneration():
    """The oracle inflates each committed libdeflate-written file to the recorded SHA-256; where libdeflate can be
    loaded, the generator writes the committed bytes again."""
    man = corpus_manifest()
    assert sorted(man) == ["libdeflate_l%d.bgzf" % l for l in (1, 12, 6, 9)]
    total = 0
    for name, rec in man.items():
        data = corpus_bytes(name)
        total += len(data)
        assert len(data) < 919482
        kind, out = oracle_result(data)
        assert kind == "ok" and hashlib.sha256(out).hexdigest() == rec["sha256"] and len(out) == rec["bytes"]
        assert len(bgzf_payloads(data)) - 1 == rec["blocks"]
        assert sum(n for _, n in dw.walk_blocks(bgzf_payloads(data)[0][0])) == 65280
        assert corpus_exact_payloads(data) == (1 if rec["level"] == 12 else 0)  # most files: no stored block at all
    assert total < 1500000
    import make_foreign_corpus as mk
    lib = mk.load_libdeflate()
    if lib is None:
        pytest.skip("libdeflate cannot be loaded: the committed files were checked, the regeneration was not")
    for name, rec in man.items():
        assert mk.build_file(lib, rec["level"]) == corpus_bytes(name), name


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 6, 9, 12])
def test_corpus_gpu(level):
    import sbam
    data = corpus_bytes("libdeflate_l%d.bgzf" % level)
    assert gpu_result(data) == oracle_result(data)
    exact = corpus_exact_payloads(data)  # 0 for every file without a stored block
    g = sbam.BamFile(data, inflate=False)
    try:
        g.inflate()
        assert g.inflate_fallbacks() == exact
    finally:
        g.close()
