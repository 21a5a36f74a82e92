"""The BAM writer's DEFLATE tables on the CPU: csrc/sbam_deflate_core.h drives a small C++ program that emits
fixed-Huffman and stored streams straight from the core's tables, and zlib inflates them; plus htsjdk-rewrite's range
parser and argument errors."""
import os
import subprocess
import zlib

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sbam_deflate_core.h"
using namespace sbam_deflate;

struct Stream {  // LSB-first bit appender + the token list it was built from
  std::vector<uint8_t> out;
  int64_t nbits = 0, token_bits = 0;
  std::string toks;
  void put(uint32_t v, int n) {
    for (int i = 0; i < n; i++, nbits++) {
      if ((nbits & 7) == 0) out.push_back(0);
      out[nbits >> 3] |= (uint8_t)(((v >> i) & 1u) << (nbits & 7));
    }
  }
  void begin() { put(kHeaderValue, kHeaderBits); }
  void lit(uint32_t v) {
    const Token t = encode_literal(v);
    if (t.n != bits_literal(v)) std::exit(10);
    put(t.bits, t.n);
    token_bits += t.n;
    toks += "L " + std::to_string(v) + "\n";
  }
  void match(int len, int dist) {
    const Token t = encode_match(len, dist);
    if (t.n != bits_match(len, dist) || t.n > 31) std::exit(11);
    put(t.bits, t.n);
    token_bits += t.n;
    toks += "M " + std::to_string(len) + " " + std::to_string(dist) + "\n";
  }
  void end(const char *name) {
    put(0, kEobBits);
    if ((int64_t)out.size() != fixed_bytes(token_bits)) std::exit(12);
    std::printf("STREAM %s %lld ", name, (long long)token_bits);
    for (uint8_t b : out) std::printf("%02x", b);
    std::printf("\n%sEND\n", toks.c_str());
  }
};

static uint32_t rnd(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 24; }

int main() {
  // RFC 1951 section 3.2.5: first distance of each of the 30 codes
  static const int dbase[31] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
                                1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577, 32769};
  uint32_t seed = 12345;
  {  // every length at distance 1
    Stream s;
    s.begin();
    s.lit(0x41);
    for (int len = 3; len <= 258; len++) {
      s.match(len, 1);
      s.lit((uint32_t)(len * 7) & 255u);
    }
    s.end("len_d1");
  }
  {  // every length at distance 32768
    Stream s;
    s.begin();
    for (int i = 0; i < 32768; i++) s.lit(rnd(seed));
    for (int len = 3; len <= 258; len++) s.match(len, 32768);
    s.end("len_d32768");
  }
  {  // both ends of every distance code
    Stream s;
    s.begin();
    for (int i = 0; i < 32768; i++) s.lit(rnd(seed));
    for (int c = 0; c < 30; c++) {
      const int lo = dbase[c], hi = dbase[c + 1] - 1;
      int code, eb;
      uint32_t ex;
      distance_code(lo, &code, &eb, &ex);
      if (code != c || ex != 0) return 20;
      distance_code(hi, &code, &eb, &ex);
      if (code != c || ex != (1u << eb) - 1u) return 21;
      s.match(3 + c, lo);
      s.match(258 - c, hi);
    }
    s.end("dist_bounds");
  }
  {  // the literals at the edges of the 8- and 9-bit ranges, and the end-of-block code alone
    Stream s;
    s.begin();
    for (uint32_t v : {0u, 143u, 144u, 255u}) s.lit(v);
    s.end("literals");
    Stream e;
    e.begin();
    e.end("empty");
  }
  for (uint32_t n : {0u, 1u, 65498u}) {  // stored headers
    uint8_t h[kStoredHeader];
    stored_header(n, h);
    std::printf("STORED %u ", n);
    for (uint8_t b : h) std::printf("%02x", b);
    std::printf("\n");
  }
  // the hash stays inside the table
  for (uint32_t v : {0u, 1u, 0xffffffffu, 0x80000000u, 0x12345678u})
    if (hash4(v) >= (1u << kHashBits)) return 30;
  return 0;
}
"""

# RFC 1951 section 3.2.5, written out independently of the header under test
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
             258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def _token_bits(tok):
    if tok[0] == "L":
        return 8 if tok[1] < 144 else 9
    _, ln, dist = tok
    lc = max(i for i, b in enumerate(_LEN_BASE) if b <= ln)
    dc = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
    return (7 if 257 + lc < 280 else 8) + _LEN_EXTRA[lc] + 5 + _DIST_EXTRA[dc]


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


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_host")
    src = d / "deflate_emit.cpp"
    src.write_text(PROGRAM)
    exe = d / "deflate_emit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr)
    streams, stored, cur = {}, {}, None
    for ln in p.stdout.splitlines():
        w = ln.split()
        if w[0] == "STREAM":
            cur = {"bits": int(w[2]), "data": bytes.fromhex(w[3]), "tokens": []}
            streams[w[1]] = cur
        elif w[0] == "STORED":
            stored[int(w[1])] = bytes.fromhex(w[2])
        elif w[0] != "END":
            cur["tokens"].append((w[0],) + tuple(int(x) for x in w[1:]))
    return streams, stored


def _inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    assert d.eof and d.unused_data == b""
    return out


def test_fixed_streams_inflate(program_output):
    """Every length 3..258 at distance 1 and at 32768, both ends of all 30 distance codes, literals 0, 143, 144 and
    255 and the end-of-block code, emitted from the core's tables: zlib inflates each stream to the bytes its tokens
    mean, and the core's bit count of every token (checked against the emitted length in the program) sums to what
    RFC 1951's tables give."""
    streams, _ = program_output
    assert sorted(streams) == ["dist_bounds", "empty", "len_d1", "len_d32768", "literals"]
    for name, s in streams.items():
        assert _inflate(s["data"]) == _replay(s["tokens"]), name
        assert s["bits"] == sum(_token_bits(t) for t in s["tokens"]), name
        assert len(s["data"]) == (3 + s["bits"] + 7 + 7) // 8, name
    lens = {t[1] for t in streams["len_d1"]["tokens"] if t[0] == "M"}
    assert lens == set(range(3, 259)) and {t[2] for t in streams["len_d1"]["tokens"] if t[0] == "M"} == {1}
    far = [t for t in streams["len_d32768"]["tokens"] if t[0] == "M"]
    assert {t[1] for t in far} == set(range(3, 259)) and {t[2] for t in far} == {32768}
    dists = [t[2] for t in streams["dist_bounds"]["tokens"] if t[0] == "M"]
    assert dists == [d for c in range(30) for d in (_DIST_BASE[c], (_DIST_BASE + [32769])[c + 1] - 1)]
    assert [t[1] for t in streams["literals"]["tokens"]] == [0, 143, 144, 255]
    assert streams["empty"]["tokens"] == [] and _inflate(streams["empty"]["data"]) == b""


def test_stored_headers_inflate(program_output):
    """The stored-block header for n = 0, 1 and 65498 followed by n bytes is a complete DEFLATE stream."""
    _, stored = program_output
    assert sorted(stored) == [0, 1, 65498]
    for n, h in stored.items():
        body = bytes((i * 31 + 7) & 255 for i in range(n))
        assert len(h) == 5 and _inflate(h + body) == body


def test_read_range_parser():
    """-r as the reference's IntRanges reads it: lo-hi half-open, a single index, comma-separated; malformed,
    descending or overlapping ranges are argument errors."""
    import argparse
    from sbam.cli import parse_read_ranges
    assert parse_read_ranges("100-1000") == [(100, 1000)]
    assert parse_read_ranges("5") == [(5, 6)]
    assert parse_read_ranges("0-10, 20,30-40") == [(0, 10), (20, 21), (30, 40)]
    assert parse_read_ranges("7-7") == [(7, 7)]
    for bad in ("", "a-b", "10-5", "1-", "-5", "0-10,5-20", "3,3", "1.5", "10k"):
        with pytest.raises(argparse.ArgumentTypeError):
            parse_read_ranges(bad)


@pytest.mark.parametrize("argv", [
    ["htsjdk-rewrite", "-r", "10-5", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "-r", "0-10,5-20", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--level", "2", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--block-bytes", "0", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "--block-bytes", "65499", "in.bam", "out.bam"],
    ["htsjdk-rewrite", "in.bam"],
])
def test_rewrite_argument_errors(argv, capsys):
    """htsjdk-rewrite refuses bad ranges, levels, block sizes and a missing OUT before it opens anything."""
    from sbam import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(argv)
    assert ei.value.code == 2
    assert "usage:" in capsys.readouterr().err
