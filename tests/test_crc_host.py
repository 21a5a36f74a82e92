"""The CRC32 check's arithmetic and report text on the CPU: csrc/sbam_crc_core.h replayed lane by lane by a small C++
program against zlib.crc32, and the check-crc report lines."""
import os
import subprocess
import zlib

import numpy as np

from conftest import ROOT

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097,
           16383, 16384, 16385, 65279, 65280, 65535, 65536]
FRONT = 32  # bytes in front of a block in the program's buffer (non-zero: the head mask must hide them)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sbam_crc_core.h"
// argv: data file, then lengths.  For every length and every start alignment 0..15 the block is the file's bytes
// [a, a + len) placed at offset FRONT + a of a 16-byte aligned buffer whose other bytes are 0xA5; the kernel's
// decomposition runs with the 64 lanes in a loop.  Prints "len align crc".
int main(int argc, char **argv) {
  using namespace sbam_crc;
  std::vector<uint32_t> tab(kTabWords);
  for (int i = 0; i < kTabWords; i++) tab[i] = table_word((uint32_t)i);
  FILE *fh = std::fopen(argv[1], "rb");
  if (!fh) return 2;
  std::vector<uint8_t> data(1 << 17);
  const size_t got = std::fread(data.data(), 1, data.size(), fh);
  std::fclose(fh);
  const size_t cap = FRONT + 16 + 65536 + 4096;
  uint8_t *buf = static_cast<uint8_t *>(std::aligned_alloc(16, cap));
  for (int k = 2; k < argc; k++) {
    const int32_t n = std::atoi(argv[k]);
    for (int a = 0; a < 16; a++) {
      if ((size_t)(a + n) > got) return 3;
      std::memset(buf, 0xA5, cap);
      const int64_t uo = FRONT + a;
      std::memcpy(buf + uo, data.data() + a, (size_t)n);
      uint32_t terms = 0;
      for (int lane = 0; lane < 64; lane++) terms ^= lane_term(tab.data(), buf, uo, n, lane);
      std::printf("%d %d %u\n", n, a, finish(tab.data(), terms, n));
    }
  }
  std::printf("0 0 %u\n", finish(tab.data(), 0u, 0));
  std::free(buf);
  return 0;
}
""".replace("FRONT", str(FRONT))


def test_core_matches_zlib(tmp_path):
    """The kernel's decomposition (rows of 64 pieces of 16 bytes, positioned table folds, the cut last piece, the
    shifts as multiplications by powers of x) over every length at which the code takes another path and every start
    alignment, for random bytes, all 0x00 and all 0xFF; built with the address and undefined-behaviour sanitizers."""
    src = tmp_path / "crc_replay.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "crc_replay"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    rng = np.random.default_rng(0xC4C32)
    fills = {"random": rng.integers(0, 256, 1 << 17, dtype=np.uint8).tobytes(), "zeros": bytes(1 << 17),
             "ones": b"\xff" * (1 << 17)}
    for name, data in fills.items():
        path = tmp_path / (name + ".bin")
        path.write_bytes(data)
        p = subprocess.run([str(exe), str(path)] + [str(n) for n in LENGTHS], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        rows = [tuple(map(int, ln.split())) for ln in p.stdout.splitlines()]
        assert len(rows) == 16 * len(LENGTHS) + 1
        for n, a, got in rows:
            assert got == zlib.crc32(data[a:a + n]), (name, n, a)
    assert zlib.crc32(b"\0") != zlib.crc32(b"\0\0")  # what a dropped init term would confuse


def test_check_crc_lines():
    """The check-crc report: the count line, then all-match or the mismatches, cut at the limit with an ellipsis."""
    from sbam.cli import check_crc_lines
    assert check_crc_lines(26, 1687319, [], 10) == ["26 blocks, 1687319 uncompressed bytes checked",
                                                    "All CRC32s match"]
    bad = [(0, 0x12345678, 0x9abcdef0), (26169, 0, 0xffffffff), (52000, 1, 2)]
    assert check_crc_lines(40, 4000, bad[:2], 2) == [
        "40 blocks, 4000 uncompressed bytes checked",
        "2 of 40 blocks with a CRC32 mismatch:",
        "\t0: footer 12345678, computed 9abcdef0",
        "\t26169: footer 00000000, computed ffffffff"]
    assert check_crc_lines(40, 4000, bad, 2) == [
        "40 blocks, 4000 uncompressed bytes checked",
        "3 of 40 blocks with a CRC32 mismatch:",
        "\t0: footer 12345678, computed 9abcdef0",
        "\t26169: footer 00000000, computed ffffffff",
        "\t…"]
