"""The dynamic-Huffman half of csrc/sbam_deflate_core.h on the CPU: a stand-alone C++ program (ASan/UBSan) runs the
length-limited code builder on histograms and emits whole dynamic blocks from token lists with the core's functions;
Python judges the lengths (limit, Kraft sum, cost against an unlimited Huffman code) and zlib inflates the streams.
Also htsjdk-rewrite's --huffman argument errors."""
import gzip
import heapq
import os
import subprocess
import zlib

import pytest

from conftest import ROOT, fixture_bytes

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "sbam_deflate_core.h"
using namespace sbam_deflate;

struct Sink {  // LSB-first bit appender
  std::vector<uint8_t> out;
  int64_t nbits = 0;
  void put(uint32_t v, int n) {
    for (int i = 0; i < n; i++, nbits++) {
      if ((nbits & 7) == 0) out.push_back(0);
      out[nbits >> 3] |= (uint8_t)(((v >> i) & 1u) << (nbits & 7));
    }
  }
};

// every buffer at its documented size on the heap, so that ASan sees an access one past it
static std::vector<uint8_t> build(const std::vector<uint32_t> &count, int limit) {
  const int n = (int)count.size();
  std::unique_ptr<uint32_t[]> c(new uint32_t[n]), keys(new uint32_t[n]), work(new uint32_t[n + 16]);
  std::unique_ptr<uint8_t[]> len(new uint8_t[n]);
  std::memcpy(c.get(), count.data(), 4 * (size_t)n);
  build_lengths(c.get(), n, limit, len.get(), keys.get(), work.get());
  return std::vector<uint8_t>(len.get(), len.get() + n);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16], name[64];
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "B")) {  // B limit n counts... -> B lengths...
      int limit, n;
      if (std::fscanf(f, "%d %d", &limit, &n) != 2) return 3;
      std::vector<uint32_t> count(n);
      for (int i = 0; i < n; i++)
        if (std::fscanf(f, "%u", &count[i]) != 1) return 3;
      const std::vector<uint8_t> a = build(count, limit), b = build(count, limit);
      if (a != b) return 10;
      std::printf("B");
      for (uint8_t l : a) std::printf(" %d", (int)l);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "S")) {  // S name ntok, then "L v" / "M len dist" -> S name form bytes ... hex
      int ntok;
      if (std::fscanf(f, "%63s %d", name, &ntok) != 2) return 3;
      std::vector<int> kind(ntok), x(ntok), y(ntok);
      std::vector<uint32_t> lc(kLitSymbols, 0), dc(kDistSymbols, 0);
      int64_t n_bytes = 0;
      for (int i = 0; i < ntok; i++) {
        char k[4];
        if (std::fscanf(f, "%3s %d", k, &x[i]) != 2) return 3;
        kind[i] = k[0] == 'M';
        if (kind[i]) {
          if (std::fscanf(f, "%d", &y[i]) != 1) return 3;
          int s, e, c;
          uint32_t v;
          length_code(x[i], &s, &e, &v);
          distance_code(y[i], &c, &e, &v);
          lc[s]++, dc[c]++;
          n_bytes += x[i];
        } else {
          lc[x[i]]++;
          n_bytes++;
        }
      }
      lc[kEobSymbol] = 1;
      const std::vector<uint8_t> ll = build(lc, kMaxCodeBits), dl = build(dc, kMaxCodeBits);
      std::vector<Code> lcode(kLitSymbols), dcode(kDistSymbols);
      std::vector<uint32_t> keys(kClSymbols), work(kClSymbols + 16), next(kMaxCodeBits + 2);
      assign_codes(ll.data(), kLitSymbols, lcode.data(), next.data());
      assign_codes(dl.data(), kDistSymbols, dcode.data(), next.data());
      HeaderPlan plan;
      header_plan(ll.data(), dl.data(), &plan, keys.data(), work.data());
      if (plan.bits > kMaxHeaderBits) return 15;
      Sink s;
      write_header(&plan, ll.data(), dl.data(), s);
      const int64_t header_written = s.nbits;
      for (int i = 0; i < ntok; i++) {
        if (kind[i]) {
          const Token a = dyn_length(lcode.data(), x[i]), b = dyn_distance(dcode.data(), y[i]);
          if (a.n > kMaxHalfTokenBits || b.n > kMaxHalfTokenBits) return 11;
          s.put(a.bits, a.n);
          s.put(b.bits, b.n);
        } else {
          const Token a = dyn_symbol(lcode.data(), x[i]);
          s.put(a.bits, a.n);
        }
      }
      const Token e = dyn_symbol(lcode.data(), kEobSymbol);
      s.put(e.bits, e.n);
      const int64_t dyn_body = body_bits(lc.data(), dc.data(), ll.data(), dl.data(), 0, 1);
      const int64_t fixed_body = body_bits(lc.data(), dc.data(), nullptr, nullptr, 0, 1);
      int64_t lanes = 0;  // the same sum the way a wave takes it
      for (int lane = 0; lane < 64; lane++) lanes += body_bits(lc.data(), dc.data(), ll.data(), dl.data(), lane, 64);
      if (lanes != dyn_body) return 12;
      if (s.nbits != header_written + dyn_body) return 13;
      int bytes;
      const int form = choose_form((int)n_bytes, fixed_body, plan.bits, dyn_body, &bytes);
      std::printf("S %s %d %d %d %lld %lld %lld %d %d %d ", name, form, bytes, plan.bits, (long long)header_written,
                  (long long)dyn_body, (long long)fixed_body, plan.hlit, plan.hdist, plan.hclen);
      for (uint8_t b : s.out) std::printf("%02x", b);
      std::printf("\n");
    } else {
      return 4;
    }
  }
  // the permuted order of RFC 1951 section 3.2.7
  static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; i++)
    if (cl_order(i) != order[i]) return 20;
  // extra bits per symbol against length_code / distance_code
  for (int len = 3; len <= 258; len++) {
    int s, e;
    uint32_t v;
    length_code(len, &s, &e, &v);
    if (length_extra_bits(s) != e) return 21;
  }
  for (int d = 1; d <= 32768; d++) {
    int c, e;
    uint32_t v;
    distance_code(d, &c, &e, &v);
    if (distance_extra_bits(c) != e) return 22;
  }
  for (int s = 0; s < 288 && s < kLitSymbols; s++)
    if (fixed_lit_length(s) != fixed_symbol(s).n || fixed_lit_code(s).bits != fixed_symbol(s).bits) return 23;
  return 0;
}
"""

LIT, DIST, CL = 286, 30, 19
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
             258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class HostProgram:
    """The compiled program; run(commands) -> its output lines."""

    def __init__(self, directory):
        self.dir = directory
        src = directory / "deflate_dynamic.cpp"
        src.write_text(PROGRAM)
        self.exe = directory / "deflate_dynamic"
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o",
                        str(self.exe), str(src)], check=True)
        self.calls = 0

    def run(self, commands):
        self.calls += 1
        path = self.dir / f"commands{self.calls}.txt"
        path.write_text("\n".join(commands) + "\n")
        p = subprocess.run([str(self.exe), str(path)], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()

    def build_lengths(self, counts, limit):
        (ln,) = self.run([f"B {limit} {len(counts)} " + " ".join(str(int(c)) for c in counts)])
        return [int(v) for v in ln.split()[1:]]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostProgram(tmp_path_factory.mktemp("deflate_dynamic_host"))


def code_symbols(counts):
    """The symbols that get a code: the counted ones, and when fewer than two are, the lowest-numbered others."""
    used = [s for s, c in enumerate(counts) if c]
    for s in (0, 1):
        if len(used) < 2 and s not in used:
            used.append(s)
    return sorted(used)


def huffman(counts):
    """(cost, depth) of an unlimited Huffman code over code_symbols(counts), the shallowest of the optimal ones
    (between equal weights the node with the smaller depth below it merges first)."""
    heap = [(int(counts[s]), 0, s) for s in code_symbols(counts)]
    heapq.heapify(heap)
    cost, tick = 0, len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick))
        tick += 1
    return cost, heap[0][1]


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _steep(k):
    """Counts that leave a Huffman code no choice: each is larger than the sum of the two before it, so the tree is a
    chain k - 1 deep (Fibonacci counts tie at every merge, and the shallowest optimal tree over them is half as deep)."""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2] + 1)
    return f[:k]


def _spread(values, n, seed):
    import numpy as np
    out = [0] * n
    for s, v in zip(np.random.default_rng(seed).permutation(n)[:len(values)].tolist(), values):
        out[s] = v
    return out


def _histograms():
    import numpy as np
    rng = np.random.default_rng(1951)
    u = gzip.decompress(fixture_bytes("5k.bam"))[:65498]
    real = np.bincount(np.frombuffer(u, np.uint8), minlength=LIT).tolist()
    real[256] = 1
    one_dist = [0] * DIST
    one_dist[7] = 1234
    h = {
        "uniform_lit": (15, [7] * LIT), "uniform_dist": (15, [3] * DIST), "uniform_cl": (7, [5] * CL),
        "one_symbol": (15, [0] * 256 + [1] + [0] * 29), "one_symbol_0": (15, [9] + [0] * (LIT - 1)),
        "one_symbol_1": (7, [0, 4] + [0] * (CL - 2)),
        "two_symbols": (15, [0] * 65 + [1000] + [0] * 190 + [1] + [0] * 29),
        "fib25_lit": (15, _spread(_fib(25), LIT, 25)), "fib12_cl": (7, _spread(_fib(12), CL, 12)),
        "fib30_dist": (15, _spread(_fib(30), DIST, 30)), "fib19_cl": (7, _fib(19)),
        "steep20_lit": (15, _spread(_steep(20), LIT, 20)), "steep10_cl": (7, _spread(_steep(10), CL, 10)),
        "all286": (15, (rng.integers(1, 3000, LIT)).tolist()),
        "all286_skewed": (15, [1 + (65498 >> (s % 17)) for s in range(LIT)]),
        "no_distance": (15, [0] * DIST), "one_distance": (15, one_dist),
        "real_5k_literals": (15, real),
    }
    for i in range(12):  # random counts, sparse and dense, small and large
        n, limit = ((LIT, 15), (DIST, 15), (CL, 7))[i % 3]
        c = rng.integers(0, [4, 60, 70000, 3][i % 4], n) * (rng.random(n) < (0.3, 0.9)[i % 2])
        h[f"random{i}"] = (limit, c.astype(int).tolist())
    return h


def test_code_builder(host):
    """Per histogram: lengths within the limit, Kraft sum exactly 1, no code for an uncounted symbol outside the forced
    pair, the unlimited Huffman cost whenever that code fits the limit and never less, and (in the program) two runs
    alike.  The Fibonacci histograms pass the limits: 25 counts are 24 bits deep, 12 are 11."""
    hs = _histograms()
    names = sorted(hs)
    lines = host.run([f"B {hs[k][0]} {len(hs[k][1])} " + " ".join(map(str, hs[k][1])) for k in names])
    assert len(lines) == len(names)
    deep = set()
    for name, ln in zip(names, lines):
        limit, counts = hs[name]
        lens = [int(v) for v in ln.split()[1:]]
        assert len(lens) == len(counts), name
        assert max(lens) <= limit, name
        syms = code_symbols(counts)
        assert [s for s, l in enumerate(lens) if l] == syms, name
        assert sum(2 ** (limit - l) for l in lens if l) == 2 ** limit, name
        cost, depth = huffman(counts)
        mine = sum(c * l for c, l in zip(counts, lens))
        if depth <= limit:
            assert mine == cost, (name, mine, cost)
        else:
            deep.add(name)
            assert mine >= cost, (name, mine, cost)
    assert {"fib25_lit", "fib12_cl", "fib30_dist", "fib19_cl", "steep20_lit", "steep10_cl"} <= deep
    assert lines[names.index("no_distance")].split()[1:4] == ["1", "1", "0"]
    assert [int(v) for v in lines[names.index("one_distance")].split()[1:]] == [1] + [0] * 6 + [1] + [0] * 22


# ---- whole streams -----------------------------------------------------------------------------------------------
class Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def symbol(self, table):
        code, n = 0, 0
        while (n, code) not in table:
            code = (code << 1) | self.take(1)
            n += 1
            assert n <= 15
        return table[(n, code)]


def _canonical(lens):
    table, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    return table


def parse_dynamic(payload):
    """A BTYPE = 10, BFINAL = 1 block read independently of the library: HLIT, HDIST, HCLEN, the three length arrays,
    the header's bit count, the code-length symbols used and the tokens ("L", v) / ("M", length, distance)."""
    b = Bits(payload)
    assert b.take(1) == 1 and b.take(2) == 2
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * CL
    for i in range(hclen):
        cl[_CL_ORDER[i]] = b.take(3)
    ct, seq, cl_used = _canonical(cl), [], []
    while len(seq) < hlit + hdist:
        s = b.symbol(ct)
        cl_used.append(s)
        if s < 16:
            seq.append(s)
        elif s == 16:
            seq += [seq[-1]] * (3 + b.take(2))
        elif s == 17:
            seq += [0] * (3 + b.take(3))
        else:
            seq += [0] * (11 + b.take(7))
    assert len(seq) == hlit + hdist
    lit, dist = seq[:hlit] + [0] * (LIT - hlit), seq[hlit:] + [0] * (DIST - hdist)
    header_bits = b.pos
    lt, dt, tokens = _canonical(lit), _canonical(dist), []
    while True:
        s = b.symbol(lt)
        if s == 256:
            break
        if s < 256:
            tokens.append(("L", s))
        else:
            ln = _LEN_BASE[s - 257] + b.take(_LEN_EXTRA[s - 257])
            d = b.symbol(dt)
            tokens.append(("M", ln, _DIST_BASE[d] + b.take(_DIST_EXTRA[d])))
    assert (b.pos + 7) // 8 == len(payload)
    return {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl": cl, "lit": lit, "dist": dist,
            "header_bits": header_bits, "cl_used": cl_used, "tokens": tokens}


def token_counts(tokens):
    """The two histograms of a token list, the end of block counted once."""
    lc, dc = [0] * LIT, [0] * DIST
    for t in tokens:
        if t[0] == "L":
            lc[t[1]] += 1
        else:
            lc[257 + max(i for i, v in enumerate(_LEN_BASE) if v <= t[1])] += 1
            dc[max(i for i, v in enumerate(_DIST_BASE) if v <= t[2])] += 1
    lc[256] = 1
    return lc, dc


def _replay(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            _, ln, dist = t
            assert 1 <= dist <= len(out)
            for _ in range(ln):
                out.append(out[-dist])
    return bytes(out)


def _streams():
    import numpy as np
    rng = np.random.default_rng(258)
    noise = [("L", int(v)) for v in rng.integers(0, 256, 32768)]
    s = {}
    s["len_d1"] = [("L", 0x41)] + [t for n in range(3, 259) for t in (("M", n, 1), ("L", (n * 7) & 255))]
    s["len_d32768"] = noise + [("M", n, 32768) for n in range(3, 259)]
    s["dist_bounds"] = noise + [t for c in range(30) for t in
                                (("M", 3 + c, _DIST_BASE[c]), ("M", 258 - c, (_DIST_BASE + [32769])[c + 1] - 1))]
    s["literals"] = [("L", v) for v in (0, 143, 144, 255)]
    s["literal_only"] = [("L", int(v)) for v in rng.integers(0, 256, 3000) // 7 * 7]
    s["match_only"] = [("L", 9)] + [("M", 258, 1)] * 200
    s["match_only_pure"] = [("L", 9), ("M", 3, 1)]
    s["one_literal"] = [("L", 200)]
    s["steep_literals"] = [("L", v) for v, k in enumerate(_steep(20)) for _ in range(k)]  # 20 bits deep unlimited
    return s


def test_dynamic_streams_inflate(host):
    """Every match length at distances 1 and 32768, both ends of all 30 distance codes, literals 0 / 143 / 144 / 255,
    literal-only, match-only and one-literal blocks, and literals with counts that make a chain (the 15-bit limit at work):
    header and body from the core's functions inflate (zlib, a bare stream that ends exactly at its end) to the bytes
    the tokens mean; the header's computed bit count is the bits written, which an independent parse of the header
    confirms; the parsed lengths are the builder's for the parsed tokens' histograms."""
    streams = _streams()
    names = sorted(streams)
    cmds = []
    for k in names:
        cmds.append(f"S {k} {len(streams[k])}")
        cmds += [" ".join(map(str, t)) for t in streams[k]]
    lines = host.run(cmds)
    assert len(lines) == len(names)
    for name, ln in zip(names, lines):
        w = ln.split()
        assert w[1] == name
        form, nbytes, plan_bits, written, dyn_body, fixed_body = (int(v) for v in w[2:8])
        raw = bytes.fromhex(w[11])
        d = zlib.decompressobj(-15)
        out = d.decompress(raw)
        want = _replay(streams[name])
        assert d.eof and d.unused_data == b"" and out == want, name
        assert plan_bits == written and len(raw) == (written + dyn_body + 7) // 8, name
        p = parse_dynamic(raw)
        assert p["tokens"] == streams[name] and p["header_bits"] == plan_bits, name
        assert (p["hlit"], p["hdist"], p["hclen"]) == tuple(int(v) for v in w[8:11]), name
        lc, dc = token_counts(streams[name])
        assert p["lit"] == host.build_lengths(lc, 15) and p["dist"] == host.build_lengths(dc, 15), name
        sizes = [len(want) + 5, (3 + fixed_body + 7) // 8, len(raw)]
        assert nbytes == min(sizes) and form == sizes.index(min(sizes)), (name, sizes, form)
        if name in ("literal_only", "literals", "one_literal"):
            assert p["dist"][:2] == [1, 1] and p["hdist"] == 2, name  # no distance code used: the pair of two
    assert max(parse_dynamic(bytes.fromhex(lines[names.index("steep_literals")].split()[11]))["lit"]) == 15
    # all three run-length symbols where they apply: repeats of a length among 256 literals in use, and between
    # literals 0 and 143 a run of 142 zeros (138 by an 18, 4 by a 17)
    assert 16 in parse_dynamic(bytes.fromhex(lines[names.index("len_d1")].split()[11]))["cl_used"]
    assert {17, 18} <= set(parse_dynamic(bytes.fromhex(lines[names.index("literals")].split()[11]))["cl_used"])


# ---- CLI -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["htsjdk-rewrite", "--huffman", "static", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--huffman", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--level", "0", "--huffman", "dynamic", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--level", "2", "--huffman", "dynamic", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--level", "2", "--huffman", "fixed", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--level", "2", "in.bam", "out.bam"],
])
def test_rewrite_huffman_argument_errors(argv, capsys):
    """--huffman takes fixed or dynamic; dynamic with --level 0 and --level 2 with either are argument errors before
    anything is opened (in.bam does not exist)."""
    from sbam import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(argv)
    assert ei.value.code == 2
    assert "usage:" in capsys.readouterr().err


def test_huffman_flag_is_exported():
    import sbam
    assert sbam.SBAM_WRITE_DYNAMIC == 0x100
    src = open(os.path.join(ROOT, "include", "sbam.h")).read()
    assert "#define SBAM_WRITE_DYNAMIC 0x100" in src
