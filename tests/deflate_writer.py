"""A bit-level DEFLATE (RFC 1951) writer for the tests: streams that no zlib encoder writes — forced header fields,
hand-chosen code lengths and code-length symbol sequences, incomplete and over-subscribed codes, length 258 as
symbol 284 + 31, invalid symbols — and expand(), a plain LZ77 expansion of the same tokens that serves as the
expected output independently of any inflater.

A token is an int (a literal byte), a (length, distance) pair, or one of the raw forms that only invalid streams
need: ("sym", s) writes literal/length symbol s with no extra bits (286 and 287 of the fixed code), and
("rawdist", length, dsym, extra) writes a length followed by distance symbol dsym and `extra` in 13 bits' worth of
that symbol's extra field (distance symbols 30 and 31 have none)."""
import heapq

import numpy as np

from test_inflate_streams import EOF_BLOCK, bgzf_block  # noqa: F401  (re-exported for the tests that build files)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL_REP_BASE = {16: 3, 17: 3, 18: 11}
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


class BitWriter:
    """Fields of up to 32 bits each, packed LSB-first into bytes by numpy."""

    def __init__(self):
        self._v = []
        self._n = []
        self.nbits = 0

    def put(self, v: int, n: int):  # n bits of v, LSB first (header fields, extra bits)
        assert 0 <= n <= 32 and 0 <= v < (1 << n)
        self._v.append(v)
        self._n.append(n)
        self.nbits += n

    def code(self, c: int, n: int):  # a Huffman code, MSB first
        assert 0 < n <= 32 and 0 <= c < (1 << n)
        self.put(int(format(c, "0%db" % n)[::-1], 2), n)

    def _bitarray(self) -> np.ndarray:
        v = np.asarray(self._v, dtype=np.uint64)[:, None]
        n = np.asarray(self._n, dtype=np.int64)[:, None]
        k = np.arange(32, dtype=np.uint64)[None, :]
        bits = ((v >> k) & np.uint64(1)).astype(np.uint8)
        return bits[k.astype(np.int64) < n]  # row-major: field order, LSB first within a field

    @property
    def bits(self):
        return self._bitarray().tolist()

    def tobytes(self) -> bytes:
        if not self._v:
            return b""
        return np.packbits(self._bitarray(), bitorder="little").tobytes()  # (zero padding to a whole byte)


def canonical_codes(lens):
    """symbol -> (code, length) of the canonical Huffman code with these lengths (RFC 1951 3.2.2); the code values
    are assigned whether or not the set is complete (an over-subscribed set gives codes that overflow their length:
    only its header is ever written)."""
    maxl = max(lens) if len(lens) else 0
    count = [0] * (maxl + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt = [0] * (maxl + 2)
    code = 0
    for l in range(1, maxl + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens, max_len=15) -> int:
    """Sum of 2^(max_len - l) over the used lengths: 1 << max_len for a complete code."""
    return sum(1 << (max_len - l) for l in lens if l)


def limited_lengths(freqs, max_len):
    """Code lengths (0 for unused symbols) of a complete prefix code with no length above max_len: Huffman's lengths,
    clamped, then the rarest short codes lengthened until the Kraft sum fits and the longest codes shortened until it
    is exactly 1.  A single used symbol gets a 1-bit code and so does one unused partner (a complete code needs two)."""
    n = len(freqs)
    used = [s for s in range(n) if freqs[s] > 0]
    lens = [0] * n
    if not used:
        return lens
    if len(used) == 1:
        partner = next(s for s in range(n) if s != used[0])
        lens[used[0]] = lens[partner] = 1
        return lens
    assert len(used) <= (1 << max_len)
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    tie = n
    while len(heap) > 1:
        fa, _, sa = heapq.heappop(heap)
        fb, _, sb = heapq.heappop(heap)
        for s in sa + sb:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tie, sa + sb))
        tie += 1
    for s in used:
        lens[s] = min(lens[s], max_len)
    full = 1 << max_len
    k = kraft(lens, max_len)
    by_rarity = sorted(used, key=lambda s: (freqs[s], s))
    while k > full:  # lengthen the rarest symbol that is still short of max_len, longest such code first
        s = max((s for s in by_rarity if lens[s] < max_len), key=lambda s: (lens[s], -freqs[s]))
        lens[s] += 1
        k -= 1 << (max_len - lens[s])
    while k < full:  # the gap is a multiple of the longest code's weight: shorten a longest code
        s = max(used, key=lambda s: (lens[s], freqs[s]))
        k += 1 << (max_len - lens[s])
        lens[s] -= 1
    assert k == full and all(0 < lens[s] <= max_len for s in used)
    return lens


def subtable_total(lens, root=9) -> int:
    """Entries of the second-level decode tables at a `root`-bit first level: one sub-table per root-bit prefix that
    has longer codes under it, sized by the longest of them."""
    size = {}
    for code, l in canonical_codes(lens).values():
        if l > root:
            p = code >> (l - root)
            size[p] = max(size.get(p, 0), 1 << (l - root))
    return sum(size.values())


def length_symbol(length: int, alt258: bool = False):
    """(symbol, extra value, extra bits) of a match length; alt258: 258 as symbol 284 with extra 31."""
    assert 3 <= length <= 258
    if length == 258:
        return (284, 31, 5) if alt258 else (285, 0, 0)
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def distance_symbol(dist: int):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k], DIST_EXTRA[k]


def token_symbols(tokens, alt258=False):
    """The (lit/len symbols, distance symbols) the tokens use, as two lists (for frequencies and coverage counts)."""
    ll, dd = [], []
    for t in tokens:
        if isinstance(t, int):
            ll.append(t)
        elif t[0] == "sym":
            ll.append(t[1])
        elif t[0] == "rawdist":
            ll.append(length_symbol(t[1], alt258)[0])
            dd.append(t[2])
        else:
            ll.append(length_symbol(t[0], alt258)[0])
            dd.append(distance_symbol(t[1])[0])
    return ll, dd


def expand(tokens, history: bytes = b"") -> bytes:
    """Plain LZ77 expansion (byte by byte, so overlapping copies repeat) of literal and (length, distance) tokens;
    `history` is output that earlier blocks of the same stream produced."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert isinstance(length, int) and 1 <= dist <= len(out), "not expandable: %r" % (t,)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


def put_tokens(w: BitWriter, tokens, lit_codes, dist_codes, alt258=False, end=True):
    """The tokens, then the end-of-block symbol, in the given codes (symbol -> (code, length))."""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit_codes[t])
        elif t[0] == "sym":
            w.code(*lit_codes[t[1]])
        else:
            raw = t[0] == "rawdist"
            s, xv, xb = length_symbol(t[1] if raw else t[0], alt258)
            w.code(*lit_codes[s])
            w.put(xv, xb)
            if raw:
                ds, dxv, dxb = t[2], t[3], (DIST_EXTRA[t[2]] if t[2] < 30 else 0)
            else:
                ds, dxv, dxb = distance_symbol(t[1])
            w.code(*dist_codes[ds])
            w.put(dxv, dxb)
    if end:
        w.code(*lit_codes[256])


def stored(w: BitWriter, data: bytes, final: bool):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.put(0, -w.nbits % 8)
    w.put(len(data), 16)
    w.put(len(data) ^ 0xffff, 16)
    for b in data:
        w.put(b, 8)


def fixed(w: BitWriter, tokens, final: bool, alt258=False, end=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS), alt258, end)


def _rle_max(seq):
    """Greedy longest runs over one sequence of lengths: 18 x 138 / 17 x 10 for zeros, value then 16 x 6."""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]
        run = 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, n - 11))
                run -= n
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [0] * run
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, n - 3))
                run -= n
            out += [v] * run
    return out


def cl_symbols(lit_lens, dist_lens, style):
    """The code-length symbol sequence of HLIT + HDIST lengths: ints 0-15, or (16 | 17 | 18, extra value)."""
    if style == "plain":
        return list(lit_lens) + list(dist_lens)
    if style == "max":  # one sequence: a run may cross from the literal/length lengths into the distance lengths
        return _rle_max(list(lit_lens) + list(dist_lens))
    if style == "zlib":  # the two trees run-length coded separately, as zlib's send_tree does
        return _rle_max(list(lit_lens)) + _rle_max(list(dist_lens))
    raise ValueError(style)


def cl_symbol_bits(sym, cl_lens) -> int:
    """Header bits of one code-length symbol (its code plus its extra bits)."""
    s = sym if isinstance(sym, int) else sym[0]
    return cl_lens[s] + CL_EXTRA.get(s, 0)


def dynamic(w: BitWriter, tokens, final: bool, lit_lens, dist_lens, cl_lens=None, cl_style="zlib", cl_syms=None,
            hlit=None, hdist=None, hclen=None, alt258=False, end=True):
    """One dynamic-Huffman block.  lit_lens / dist_lens are the code lengths to declare (HLIT = len(lit_lens) - 257
    and HDIST = len(dist_lens) - 1 unless forced: 287 / 288 and 31 / 32 entries give the field values 30 / 31 that
    zlib rejects).  cl_style "plain" | "zlib" | "max" run-length codes them; "explicit" writes cl_syms as given.
    cl_lens: the 19 code-length-code lengths (default: a complete code of at most 7 bits for the symbols used).
    The tokens are written in the canonical codes of lit_lens / dist_lens."""
    if cl_style == "explicit":
        syms = list(cl_syms)
    else:
        syms = cl_symbols(lit_lens, dist_lens, cl_style)
    if cl_lens is None:
        freqs = [0] * 19
        for s in syms:
            freqs[s if isinstance(s, int) else s[0]] += 1
        cl_lens = limited_lengths(freqs, 7)
    assert len(cl_lens) == 19 and max(cl_lens) <= 7
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    hlit_f = len(lit_lens) - 257 if hlit is None else hlit
    hdist_f = len(dist_lens) - 1 if hdist is None else hdist
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit_f, 5)
    w.put(hdist_f, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl_codes = canonical_codes(cl_lens)
    for s in syms:
        if isinstance(s, int):
            w.code(*cl_codes[s])
        else:
            w.code(*cl_codes[s[0]])
            w.put(s[1], CL_EXTRA[s[0]])
    put_tokens(w, tokens, canonical_codes(lit_lens), canonical_codes(dist_lens), alt258, end)
    return syms, cl_lens


def lens_for(tokens, n_lit=None, n_dist=None, max_len=15, alt258=False, extra_lit=(), extra_dist=()):
    """Complete literal/length and distance code lengths for these tokens (plus end of block and any extra symbols
    to include), trimmed to the highest used symbol or padded to n_lit / n_dist entries."""
    ll, dd = token_symbols(tokens, alt258)
    fl, fd = [0] * 286, [0] * 30
    for s in list(ll) + [256] + list(extra_lit):
        fl[s] += 1
    for s in list(dd) + list(extra_dist):
        fd[s] += 1
    if not any(fd):
        fd[0] = 1  # (limited_lengths then adds a partner: two 1-bit distance codes, a complete set)
    lit, dist = limited_lengths(fl, max_len), limited_lengths(fd, max_len)
    nl = n_lit or max(257, max(s for s in range(286) if lit[s]) + 1)
    nd = n_dist or max(s for s in range(30) if dist[s]) + 1
    assert not any(lit[nl:]) and not any(dist[nd:])
    return lit[:nl], dist[:nd]


def walk_blocks(payload: bytes):
    """A plain bit-by-bit reader of a valid raw DEFLATE stream: the list of its blocks as ("stored" | "fixed" |
    "dynamic", output bytes of the block), for telling on the CPU which blocks an encoder chose."""
    pos = 0  # bit position

    def peek(n):  # n <= 16 bits at pos, LSB first (zeros past the payload)
        return (int.from_bytes(payload[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    def get(n):
        nonlocal pos
        v = peek(n)
        pos += n
        return v

    def table(lens):
        return {(l, c): s for s, (c, l) in canonical_codes(lens).items()}

    def sym(t):
        nonlocal pos
        w, c = peek(15), 0
        for l in range(1, 16):
            c = (c << 1) | ((w >> (l - 1)) & 1)
            if (l, c) in t:
                pos += l
                return t[(l, c)]
        raise ValueError("no such code")

    blocks = []
    while True:
        final, btype = get(1), get(2)
        if btype == 0:
            pos += -pos % 8
            n = get(16)
            pos += 16 + 8 * n
            blocks.append(("stored", n))
        else:
            assert btype in (1, 2)
            lit, dist = FIXED_LIT_LENS, FIXED_DIST_LENS
            if btype == 2:
                hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = get(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = sym(ct)
                    lens += [s] if s < 16 else [lens[-1] if s == 16 else 0] * (CL_REP_BASE[s] + get(CL_EXTRA[s]))
                lit, dist = lens[:hlit], lens[hlit:hlit + hdist]
            lt, dt, n = table(lit), table(dist), 0
            while True:
                s = sym(lt)
                if s == 256:
                    break
                if s < 256:
                    n += 1
                else:
                    n += LEN_BASE[s - 257] + get(LEN_EXTRA[s - 257])
                    get(DIST_EXTRA[sym(dt)])
            blocks.append(("fixed" if btype == 1 else "dynamic", n))
        if final:
            return blocks
