"""The resolver's dependent pass on the CPU: csrc/sbam_resolve_core.h drives a small C++ program that replays one
resolver step the way k_inflate_resolve does it — literals and independent matches first, then every dependent byte
from the position its collapsed source reaches after one descending sweep — and deflate_writer.expand() of the same
tokens is the expected output."""
import os
import subprocess

import pytest

from conftest import ROOT
from deflate_writer import expand

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sbam_resolve_core.h"
using namespace sbam_resolve;

static uint32_t seed = 2024;
static uint32_t rnd(uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; }

struct M { int mO, d, Le; };

int main() {
  // collapsed source of every byte of the longest match, every distance 1..300 (mO = d: the source is [0, d))
  for (int d = 1; d <= 300; d++) {
    std::printf("COLLAPSE %d", d);
    for (int j = 0; j < kMaxMatch; j++) {
      const int s = collapsed_source(d, d, j);
      if (period_offset(j, d) != j % d) return 10;
      std::printf(" %d", s);
    }
    std::printf("\n");
  }
  // one resolver step over random tokens: P literals before the step's base B, then up to 64 words
  long deps = 0, hops = 0, modhops = 0, collapsed = 0, maxdepth = 0;
  for (int c = 0; c < 600; c++) {
    std::vector<int> buf;          // output bytes, -1 = not written yet
    std::vector<M> ind, dep;
    const int P = c < 8 ? c : (int)rnd(300), B = P;
    std::printf("STEP %d\n", c);
    for (int i = 0; i < P; i++) { buf.push_back((int)rnd(256)); std::printf("L %d\n", buf.back()); }
    const int words = 1 + (int)rnd(64), style = (int)rnd(4);
    for (int w = 0; w < words; w++) {
      const int O = (int)buf.size();
      if (O == 0 || rnd(100) < (style == 0 ? 50u : 15u)) {
        buf.push_back((int)rnd(256));
        std::printf("L %d\n", buf.back());
        continue;
      }
      int L = rnd(4) == 0 ? 3 + (int)rnd(256) : 3 + (int)rnd(12);
      int d = style == 3 ? 1 + (int)rnd((uint32_t)O) : 1 + (int)rnd((uint32_t)(O < 40 ? O : 40));
      if (style == 2 && !dep.empty() && rnd(2)) {  // read exactly the previous match's output
        d = dep.back().Le;
        L = d;
      }
      std::printf("M %d %d\n", L, d);
      const int srcEnd = O - d + (L < d ? L : d);
      (srcEnd <= B ? ind : dep).push_back({O, d, L});
      buf.resize(O + L, -1);
    }
    // pass 1: independents copy from final bytes (their source lies below B)
    for (const M &m : ind)
      for (int j = 0; j < m.Le; j++) {
        const int s = collapsed_source(m.mO, m.d, j);
        if (s >= B || buf[s] < 0) return 20;
        buf[m.mO + j] = buf[s];
      }
    // pass 2: every dependent byte on its own, from the state pass 1 left (no byte of pass 2 is read)
    const int n = (int)dep.size();
    std::vector<int> mO(n), d(n), Le(n), got;
    for (int k = 0; k < n; k++) { mO[k] = dep[k].mO; d[k] = dep[k].d; Le[k] = dep[k].Le; }
    deps += n;
    for (int k = 0; k < n; k++)
      for (int j = 0; j < Le[k]; j++) {
        int s = collapsed_source(mO[k], d[k], j), depth = 0;
        collapsed += j >= d[k];
        if (s < mO[k] - d[k] || s >= mO[k]) return 21;
        // hop by hop (what sweep() does), counting
        for (int q = n - 1; q >= 0; q--) {
          if (hop_hits(s, mO[q], Le[q])) { hops++; depth++; modhops += s - mO[q] >= d[q]; }
          s = sweep_hop(s, mO[q], d[q], Le[q]);
        }
        if (s != sweep(collapsed_source(mO[k], d[k], j), mO.data(), d.data(), Le.data(), n)) return 22;
        if (s < 0 || s <= B - kMaxMatch) return 23;             // stays near
        for (int q = 0; q < n; q++) if (hop_hits(s, mO[q], Le[q])) return 24;  // outside every dependent's output
        if (buf[s] < 0) return 25;                              // a literal, an independent's byte or earlier output
        if (depth > maxdepth) maxdepth = depth;
        got.push_back(buf[s]);
      }
    size_t g = 0;
    for (int k = 0; k < n; k++) for (int j = 0; j < Le[k]; j++) buf[mO[k] + j] = got[g++];
    std::printf("OUT ");
    for (int v : buf) { if (v < 0) return 26; std::printf("%02x", v); }
    std::printf("\n");
  }
  std::printf("COUNTS %ld %ld %ld %ld %ld\n", deps, hops, modhops, collapsed, maxdepth);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("resolve_core_host")
    src = d / "resolve_replay.cpp"
    src.write_text(PROGRAM)
    exe = d / "resolve_replay"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    collapse, steps, counts, cur = {}, [], None, None
    for ln in p.stdout.splitlines():
        w = ln.split()
        if w[0] == "COLLAPSE":
            collapse[int(w[1])] = [int(x) for x in w[2:]]
        elif w[0] == "STEP":
            cur = {"tokens": [], "out": None}
            steps.append(cur)
        elif w[0] == "L":
            cur["tokens"].append(int(w[1]))
        elif w[0] == "M":
            cur["tokens"].append((int(w[1]), int(w[2])))
        elif w[0] == "OUT":
            cur["out"] = bytes.fromhex(w[1]) if len(w) > 1 else b""
        elif w[0] == "COUNTS":
            counts = [int(x) for x in w[1:]]
    return collapse, steps, counts


def test_collapsed_source_every_distance(program_output):
    """Byte j of a (258, d) match equals the byte at its collapsed source, which lies in the d bytes before the
    match: every d in 1..300, every j in 0..257, against expand()."""
    collapse, _, _ = program_output
    assert sorted(collapse) == list(range(1, 301))
    for d, pos in collapse.items():
        out = expand([(i * 131 + d * 7) & 255 for i in range(d)] + [(258, d)])
        assert len(pos) == 258
        for j, s in enumerate(pos):
            assert 0 <= s < d and s == j % d, (d, j, s)
            assert out[s] == out[d + j], (d, j, s)


def test_sweep_random_dependent_sets(program_output):
    """600 random resolver steps (0..299 bytes before the base, up to 64 words, short and long matches, distances
    within 40 and up to the whole output, chains reading exactly the previous match): literals and independents
    first, then every dependent byte from where one descending sweep ends — equal to expand() of the same tokens.
    The program itself checks that the sweep ends outside every dependent's output, above base - 258, on a byte
    already written.  The sets are not vacuous: thousands of dependents, hops through a mod, chains several deep."""
    _, steps, counts = program_output
    assert len(steps) == 600
    for i, s in enumerate(steps):
        assert s["out"] == expand(s["tokens"]), i
    deps, hops, modhops, collapsed, maxdepth = counts
    assert deps > 5000 and hops > 20000 and modhops > 500 and collapsed > 5000 and maxdepth >= 6, counts
