"""The coordinate sort's host side: the key of csrc/sbam_sort_core.h replayed by a small C++ program against a numpy
restatement, sam.header_with_sort_order, and the ctypes mirrors of sbam_sort_totals and sbam_write_order against the
header as a C compiler lays it out."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

I32_MIN, I32_MAX = -2**31, 2**31 - 1
REF_IDS = [I32_MIN, -2, -1, 0, 1, 255, 256, I32_MAX]
POSITIONS = [I32_MIN, -1, 0, 1, 2**24 - 1, 2**24, I32_MAX]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "sbam_sort_core.h"
// argv: ref_id pos pairs.  Prints "ref_id pos key d0 .. d7" (the key and its eight digits, least significant first).
int main(int argc, char **argv) {
  static_assert(sbam_sort::key(-1, -1) == 0xffffffff7fffffffull, "no coordinate: last reference, first position");
  static_assert(sbam_sort::kDigits == 256 && sbam_sort::kMaxPasses == 8, "bytes of a 64-bit key");
  for (int k = 1; k + 1 < argc; k += 2) {
    const int32_t r = (int32_t)std::atoll(argv[k]), p = (int32_t)std::atoll(argv[k + 1]);
    const uint64_t key = sbam_sort::key(r, p);
    std::printf("%d %d %llu", r, p, (unsigned long long)key);
    for (int b = 0; b < sbam_sort::kMaxPasses; b++) std::printf(" %u", sbam_sort::digit(key, b));
    std::printf("\n");
  }
  return 0;
}
"""


def numpy_keys(ref_id, pos) -> np.ndarray:
    """The issue's definition, restated: (uint64)(uint32) ref_id << 32 | (uint32)(pos ^ 0x80000000)."""
    r = np.asarray(ref_id, np.int32).view(np.uint32).astype(np.uint64)
    p = (np.asarray(pos, np.int32).view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return (r << np.uint64(32)) | p


def test_key_matches_restatement_and_python_order(tmp_path):
    """Every (ref_id, pos) of the edge grid: the header's key (built with the address and undefined-behaviour
    sanitizers) equals the numpy restatement, its digits are its bytes, and sorting by it as an unsigned word is Python's
    sort of (ref_id mod 2^32, pos)."""
    src = tmp_path / "sort_key.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "sort_key"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    pairs = [(r, p) for r in REF_IDS for p in POSITIONS]
    p = subprocess.run([str(exe)] + [str(v) for pair in pairs for v in pair], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = [[int(v) for v in ln.split()] for ln in p.stdout.splitlines()]
    assert [(r[0], r[1]) for r in rows] == pairs
    got = np.asarray([r[2] for r in rows], np.uint64)
    want = numpy_keys([a for a, _ in pairs], [b for _, b in pairs])
    assert np.array_equal(got, want)
    for r in rows:
        assert r[3:] == list(int(r[2]).to_bytes(8, "little"))
    assert len(set(got.tolist())) == len(pairs)  # (distinct pairs, distinct keys)
    by_key = [pairs[i] for i in np.argsort(got, kind="stable").tolist()]
    assert by_key == sorted(pairs, key=lambda rp: (rp[0] % 2**32, rp[1]))
    assert by_key[-1][0] == -1 and by_key[0] == (0, I32_MIN)  # no coordinate last; the smallest position first


# ---- header_with_sort_order --------------------------------------------------------------------------------------
def _header(text: bytes, refs=((b"chr1", 1000), (b"chrM", 16571)), pad: int = 0) -> bytes:
    body = text + b"\0" * pad
    out = b"BAM\x01" + struct.pack("<i", len(body)) + body + struct.pack("<i", len(refs))
    for name, n in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", n)
    return out


def _split(h: bytes):
    (lt,) = struct.unpack_from("<i", h, 4)
    return h[8:8 + lt], h[8 + lt:]


SQ = b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrM\tLN:16571\n"


@pytest.mark.parametrize("text, want", [
    (b"@HD\tVN:1.5\tSO:unsorted\n" + SQ, b"@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    (b"@HD\tVN:1.5\n" + SQ, b"@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    (b"@HD\tVN:1.6\tSO:queryname\tGO:none\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\tGO:none\n" + SQ),
    (b"@HD\tVN:1.6", b"@HD\tVN:1.6\tSO:coordinate"),  # no newline behind the only line
    (SQ, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    (b"", b"@HD\tVN:1.6\tSO:coordinate\n"),
    (b"@CO\t@HD\tSO:unsorted\n", b"@HD\tVN:1.6\tSO:coordinate\n@CO\t@HD\tSO:unsorted\n"),  # @HD counts on line 1 only
])
def test_header_with_sort_order(text, want):
    """@HD with SO (at the end, in the middle), without SO, without @HD, an empty text: the text is the expected one,
    l_text is its length, and the references follow byte for byte; the same with NUL padding behind the text, which is
    dropped."""
    from sbam import sam
    for pad in (0, 1, 7):
        h = _header(text, pad=pad)
        out = sam.header_with_sort_order(h, "coordinate")
        got_text, refs = _split(out)
        assert got_text == want
        assert out[:4] == b"BAM\x01" and struct.unpack_from("<i", out, 4)[0] == len(want)
        assert refs == _split(h)[1] and len(out) == 8 + len(want) + len(refs)
        assert sam.header_with_sort_order(out, "coordinate") == out  # (already so: unchanged)
    assert _split(sam.header_with_sort_order(_header(b"@HD\tVN:1.6\tSO:coordinate\n"), "unsorted"))[0] == \
        b"@HD\tVN:1.6\tSO:unsorted\n"
    no_refs = sam.header_with_sort_order(_header(b"", refs=()), "coordinate")
    assert no_refs == b"BAM\x01" + struct.pack("<i", 25) + b"@HD\tVN:1.6\tSO:coordinate\n" + struct.pack("<i", 0)


def test_header_with_sort_order_rejects_what_is_no_header():
    from sbam import sam
    for bad in (b"", b"BAM\x01", b"BAN\x01" + bytes(8), b"BAM\x01" + struct.pack("<i", 100) + bytes(8),
                b"BAM\x01" + struct.pack("<i", -1) + bytes(8)):
        with pytest.raises(ValueError):
            sam.header_with_sort_order(bad, "coordinate")


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_sort_struct_layouts_follow_the_header(tmp_path):
    """sizeof / offsetof of sbam_sort_totals and sbam_write_order as a C compiler lays out include/sbam.h, against the
    ctypes mirrors; the new entry points are exported with signatures."""
    import sbam
    mirrors = {"sbam_sort_totals": sbam._SortTotals, "sbam_write_order": sbam._WriteOrder}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{ROOT}/include/sbam.h"', "int main(void) {"]
    for t, cls in mirrors.items():
        lines.append(f'  printf("{t} sizeof %zu\\n", sizeof({t}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{t} {f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()
    seen = set()
    for ln in out:
        t, f, *v = ln.split()
        cls = mirrors[t]
        if f == "sizeof":
            assert int(v[0]) == ctypes.sizeof(cls), t
        else:
            assert (int(v[0]), int(v[1])) == (getattr(cls, f).offset, getattr(cls, f).size), (t, f)
        seen.add((t, f))
    assert len(seen) == sum(len(c._fields_) + 1 for c in mirrors.values())
    assert ctypes.sizeof(sbam._SortTotals) == 24 and ctypes.sizeof(sbam._WriteOrder) == 24
    assert {"sbam_sort_records", "sbam_get_sort_order", "sbam_sort_order_device", "sbam_sort_tile_keys",
            "sbam_test_sort_keys", "sbam_write_bam_ordered"} <= set(sbam.EXPORTS)
    tile = sbam.load_library().sbam_sort_tile_keys()
    assert tile % 256 == 0 and 256 <= tile <= 8192
