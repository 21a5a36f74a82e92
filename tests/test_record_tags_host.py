"""The rules of sbam_load_record_tags on the CPU: sbam.sam.find_tags (the host statement of the rules) against the
reference's SAM text of 2.bam and 5k.bam and on hand-written tag bytes; csrc/sbam_tag_core.h replayed by a small C++
program (the lane's walk and the wave's walk, the 64 lanes of the NUL search in a loop) against find_tags' walk; and
the layout of the three new ABI structs.  The hand-written tag lists are shared with tests/test_record_tags.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_sam_text import decoded, golden_sam

# the 17 tag names that occur in 2.bam and 5k.bam, and one that does not
QUERY18 = ["X0", "X1", "BD", "MD", "PG", "RG", "XG", "BI", "AM", "NM", "SM", "XM", "XO", "MQ", "OQ", "XT", "XA", "ZZ"]
LONG = 1024  # sbam_tag_long_aux_bytes(): csrc/sbam_tag_core.h kLongAuxBytes (the GPU test asserts the export)


# ---- hand-written tag lists ------------------------------------------------------------------------------------------
def z(tag: bytes, text: bytes, t: bytes = b"Z") -> bytes:
    return tag + t + text + b"\0"


def arr(tag: bytes, sub: bytes, fmt: str, *vals) -> bytes:
    return tag + b"B" + sub + struct.pack("<i", len(vals)) + struct.pack(f"<{len(vals)}{fmt}", *vals)


def filler(n: int, tag: bytes = b"ZL") -> bytes:
    """A Z tag of exactly n bytes (n >= 4)."""
    return z(tag, b"f" * (n - 4))


HAND_QUERY = ["NM", "Nm", "MN", "N0", "XZ", "XH", "XE", "Xc", "XC", "Xs", "XS", "Xi", "XI", "Xf", "Xg", "Xh", "XA", "Bc",
              "BC", "Bs", "BS", "Bi", "BI", "Bf", "B0", "ZL", "ZN", "ZB", "AS", "RG", "MD", "ZZ"]
_SEVENTEEN = [b"T%c" % (65 + i) + b"C" + bytes([i]) for i in range(16)]  # sixteen other tags


def hand_lists(T: int = LONG):
    """(label, tag bytes) of every well-formed hand-written case."""
    every = (b"XAAQ" + b"Xcc" + struct.pack("<b", -128) + b"XCC" + struct.pack("<B", 255) +
             b"Xss" + struct.pack("<h", -32768) + b"XSS" + struct.pack("<H", 65535) +
             b"Xii" + struct.pack("<i", -2 ** 31) + b"XII" + struct.pack("<I", 0xFFFFFFFF) +
             b"Xff" + struct.pack("<f", -0.0) + b"Xgf" + struct.pack("<I", 0x7fc00001) + b"Xhf" + struct.pack("<f", 1e10) +
             z(b"XH", b"1AE301", b"H") + z(b"XE", b"") + arr(b"Bc", b"c", "b", -128, 127) + arr(b"BC", b"C", "B", 0, 255) +
             arr(b"Bs", b"s", "h", -32768, 32767, 5) + arr(b"BS", b"S", "H", 65535) + arr(b"Bi", b"i", "i", -2 ** 31) +
             arr(b"BI", b"I", "I", 0xFFFFFFFF, 1) + arr(b"Bf", b"f", "f", 0.25, -2.5) + arr(b"B0", b"c", "b"))
    out = [("none", b""), ("single", b"NMC\x07"), ("every type", every),
           ("first of 17", b"NMC\x01" + b"".join(_SEVENTEEN)), ("last of 17", b"".join(_SEVENTEEN) + b"NMC\x02"),
           ("middle of 17", b"".join(_SEVENTEEN[:8]) + b"NMC\x03" + b"".join(_SEVENTEEN[8:])),
           ("absent from 16", b"".join(_SEVENTEEN)),
           ("duplicated", b"NMC\x01" + z(b"RG", b"first") + b"NMC\x02" + z(b"RG", b"second")),
           ("one character apart", b"NmC\x01" + b"MNC\x02" + b"N0C\x03" + b"NMC\x04"),
           ("Z that spells a header", z(b"XZ", b"abNMC\x07cd") + b"NMC\x09"),
           ("B:C that spells a header", arr(b"BC", b"C", "B", *b"NMi\x01\x02\x03\x04") + b"NMC\x0a")]
    for n in (T - 1, T, T + 1):
        out.append((f"{n} tag bytes", b"ASC\x05" + filler(n - 8) + b"NMC\x06"))
    for d in (63, 64, 65, 255, 256, 257):
        # (the long path: more than T tag bytes; the NUL of ZN sits d bytes from its value's start)
        out.append((f"NUL at {d}", b"ASC\x01" + z(b"ZN", b"n" * d) + arr(b"ZB", b"C", "B", *([7] * T)) + b"NMs\x39\x30"))
    return out


def big_lists():
    """The two values larger than any LDS stage, each with a queried scalar behind it."""
    rng = np.random.default_rng(70000)
    text = rng.integers(33, 127, 70000, dtype=np.uint8).tobytes()
    elems = rng.integers(0, 65536, 100000, dtype=np.uint16)
    return [("70 000-character Z", b"ASC\x02" + z(b"MD", text) + b"NMi" + struct.pack("<i", -70000)),
            ("100 000-element B:S", b"ASC\x03" + b"ZBBS" + struct.pack("<i", elems.size) + elems.tobytes() + b"NMC\x0b")]


def malformed_lists(T: int = LONG):
    """(label, tag bytes) of every malformed kind, each once for a lane's walk and once (behind more than T well-formed
    bytes) for a wave's."""
    kinds = [("two bytes left for a header", b"NMC\x07" + b"XY"),
             ("unknown type", b"NMC\x07" + b"XYq\x01"),
             ("scalar past the end", b"NMC\x07" + b"XYi\x01\x02"),
             ("Z without a NUL", b"NMC\x07" + b"XYZabc"),
             ("B header cut", b"NMC\x07" + b"XYBc\x01\x00"),
             ("B with an unknown subtype", b"NMC\x07" + b"XYBx" + struct.pack("<i", 1) + b"\x00"),
             ("B with a negative count", b"NMC\x07" + b"XYBc" + struct.pack("<i", -1)),
             ("B elements past the end", b"NMC\x07" + b"XYBs" + struct.pack("<i", 3) + b"\x00" * 4)]
    return kinds + [(k + ", long", filler(T + 10) + v) for k, v in kinds]


def walked(aux: bytes):
    """([(name, type, sub, rel, len, value)] of the tags in front of the first malformed one, well-formed?)"""
    from sbam import sam
    out = []
    try:
        for name, t, st, rel, v, raw in sam._walk_tags(aux):
            n = len(raw) if t in "ZHB" else sam._SCALAR_WIDTH[t]
            out.append((name[0] | name[1] << 8, ord(t), ord(st) if st else 0, rel, n, v & (2 ** 64 - 1)))
    except ValueError:
        return out, False
    return out, True


# ---- find_tags against the reference's SAM text --------------------------------------------------------------------
def golden_table(name: str):
    """Per record of tests/golden/sam/<name>.sam.gz: the read name, then `type:value` or `*` per QUERY18 entry."""
    _, lines = golden_sam(name)
    rows = []
    for ln in lines:
        cols = ln.split("\t")
        tags = {}
        for c in cols[11:]:
            tags.setdefault(c[:2], c[3:])
        rows.append([cols[0]] + [tags.get(t, "*") for t in QUERY18])
    return rows


def aux_of(fields, k: int) -> bytes:
    return fields.aux[int(fields.aux_off[k]):int(fields.aux_off[k + 1])].tobytes()


@pytest.mark.parametrize("name,xa", [("2", 1257), ("5k", 2004)])
def test_find_tags_renders_the_reference_sam(name, xa, oracle_files):
    from sbam import sam
    o, offs, fields, _, _ = decoded(name + ".bam", oracle_files)
    want = golden_table(name)
    assert len(want) == len(offs)
    present = np.zeros(len(QUERY18), np.int64)
    for k in range(len(offs)):
        aux = aux_of(fields, k)
        got = sam.find_tags(aux, QUERY18)
        row = ["*" if g is None else sam.tag_value_text(g[0], g[1], g[3], g[4]) for g in got]
        assert row == want[k][1:], (k, want[k][0])
        for j, g in enumerate(got):
            if g is not None:
                present[j] += 1
                t, _, rel, v, raw = g
                assert aux[rel - 3:rel - 1].decode() == QUERY18[j] and (not raw or aux[rel:rel + len(raw)] == raw)
    want_present = [sum(r[1 + j] != "*" for r in want) for j in range(len(QUERY18))]
    assert present.tolist() == want_present
    assert present[QUERY18.index("XA")] == xa and present[QUERY18.index("ZZ")] == 0
    assert all(p > 0 for p in present[:-1]), "a queried tag name does not occur"


def test_find_tags_on_hand_written_lists():
    from sbam import sam
    got = dict(zip(HAND_QUERY, sam.find_tags(dict(hand_lists())["every type"], HAND_QUERY)))
    assert got["Xc"][:4] == ("c", "", 7, -128) and got["XC"][3] == 255 and got["Xs"][3] == -32768
    assert got["XS"][3] == 65535 and got["Xi"][3] == -2 ** 31 and got["XI"][3] == 0xFFFFFFFF
    assert got["Xf"][3] == 0x80000000 and got["Xg"][3] == 0x7fc00001
    assert got["Xh"][3] == struct.unpack("<I", struct.pack("<f", 1e10))[0]
    assert got["XA"][:4] == ("A", "", 3, ord("Q")) and got["XH"][0] == "H" and got["XH"][4] == b"1AE301"
    assert got["XE"][3] == 0 and got["XE"][4] == b"" and got["B0"][1:] == ("c", got["B0"][2], 0, b"")
    assert got["Bs"][1] == "s" and got["Bs"][3] == 3 and got["Bs"][4] == struct.pack("<3h", -32768, 32767, 5)
    assert got["NM"] is None and got["ZZ"] is None
    texts = [None if g is None else sam.tag_value_text(g[0], g[1], g[3], g[4]) for g in got.values()]
    assert "f:-0.0" in texts and "f:nan" in texts and "B:I,4294967295,1" in texts
    assert "f:" + sam._float_text(1e10) in texts and "A:Q" in texts and "Z:" in texts and "i:4294967295" in texts
    by = {k: dict(zip(HAND_QUERY, sam.find_tags(v, HAND_QUERY))) for k, v in hand_lists() + big_lists()}
    assert [by[k]["NM"][3] for k in ("first of 17", "last of 17", "middle of 17")] == [1, 2, 3]
    assert by["absent from 16"]["NM"] is None and by["none"]["NM"] is None
    assert by["duplicated"]["NM"][3] == 1 and by["duplicated"]["RG"][4] == b"first"
    assert [by["one character apart"][t][3] for t in ("Nm", "MN", "N0", "NM")] == [1, 2, 3, 4]
    assert by["Z that spells a header"]["NM"][3] == 9 and by["B:C that spells a header"]["NM"][3] == 10
    for n in (LONG - 1, LONG, LONG + 1):
        assert len(dict(hand_lists())[f"{n} tag bytes"]) == n and by[f"{n} tag bytes"]["NM"][3] == 6
    for d in (63, 64, 65, 255, 256, 257):
        g = by[f"NUL at {d}"]
        assert g["ZN"][3] == d and g["NM"][3] == 12345 and len(dict(hand_lists())[f"NUL at {d}"]) > LONG
    assert by["70 000-character Z"]["MD"][3] == 70000 and by["70 000-character Z"]["NM"][3] == -70000
    assert by["100 000-element B:S"]["ZB"][3] == 100000 and by["100 000-element B:S"]["NM"][3] == 11
    for label, aux in malformed_lists():
        with pytest.raises(ValueError):
            sam.find_tags(aux, ["ZZ"])
        with pytest.raises(ValueError):
            sam.tag_texts(aux)


# ---- the core header, replayed ---------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "sbam_tag_core.h"
// argv[1]: cases as (int32 n, int32 align, n bytes)*.  A case's tag bytes are placed at offset 8 + align of a
// 4-byte aligned buffer filled with 0x00 (so a NUL search that looked outside [from, end) would find one), as a
// record's lie at any alignment in the stream.  Each case is walked twice: as a lane walks it (bytes one at a time)
// and as a wave does (the header by one lane; the NUL search in steps of 64 lanes x one aligned dword).  Prints
// "<case> <L|W> ok|bad" after one line "key type sub rel len value" per tag.
int main(int argc, char **argv) {
  using namespace sbam_tag;
  FILE *fh = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
  if (!fh) return 2;
  int32_t hd[2];
  for (int id = 0; std::fread(hd, 4, 2, fh) == 2; id++) {
    const int32_t n = hd[0], align = hd[1];
    std::vector<uint32_t> store((size_t)(n + 8 + align + 3) / 4 + 2, 0u);
    uint8_t *buf = reinterpret_cast<uint8_t *>(store.data()) + 8 + align;
    if (n && std::fread(buf, 1, (size_t)n, fh) != (size_t)n) return 3;
    const int64_t x = 8 + align;  // the tag bytes' offset in the "stream"
    auto hdr = [&](int32_t p, int32_t cnt) {
      uint64_t h = 0;
      for (int i = 0; i < cnt; i++) h |= (uint64_t)buf[p + i] << (8 * i);
      return h;
    };
    auto lane_nul = [&](int32_t from, int32_t end) {
      for (int32_t e = from; e < end; e++)
        if (buf[e] == 0) return e;
      return (int32_t)-1;
    };
    auto wave_nul = [&](int32_t from, int32_t end) {
      for (int32_t q = nul_first_step(x, from); q < end; q += kNulStepBytes) {
        for (int lane = 0; lane < 64; lane++) {  // the ballot: the lowest lane with a hit
          const int32_t q0 = q + 4 * lane;
          uint32_t w = 0xffffffffu;
          if (q0 < end) std::memcpy(&w, buf + q0, 4);
          const int32_t hit = lane_first_nul(w, q0, from, end);
          if (hit >= 0) return hit;
        }
      }
      return (int32_t)-1;
    };
    auto on = [&](const Cell &c) {
      std::printf("%u %u %u %d %d %llu\n", c.key, c.type, c.sub, c.rel, c.len, (unsigned long long)c.value);
    };
    std::printf("%d L %s\n", id, walk(hdr, lane_nul, n, on) ? "ok" : "bad");
    std::printf("%d W %s\n", id, walk(hdr, wave_nul, n, on) ? "ok" : "bad");
  }
  std::fclose(fh);
  std::printf("long %d\n", kLongAuxBytes);
  return 0;
}
"""


def random_list(rng) -> bytes:
    out = b""
    for _ in range(int(rng.integers(0, 12))):
        tag = bytes(rng.choice(list(b"ABNMXZab"), 2).tolist())
        t = "AcCsSiIfZHB"[int(rng.integers(0, 11))]
        if t in "ZH":
            n = int(rng.choice([0, 1, 3, 17, 62, 63, 64, 65, 200, 255, 256, 257, 600]))
            out += z(tag, rng.integers(1, 256, n, dtype=np.uint8).tobytes(), t.encode())
        elif t == "B":
            st = "cCsSiIf"[int(rng.integers(0, 7))]
            w = {"c": 1, "C": 1, "s": 2, "S": 2}.get(st, 4)
            n = int(rng.integers(0, 40))
            out += tag + b"B" + st.encode() + struct.pack("<i", n) + rng.integers(0, 256, n * w, dtype=np.uint8).tobytes()
        else:
            w = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2}.get(t, 4)
            out += tag + t.encode() + rng.integers(0, 256, w, dtype=np.uint8).tobytes()
    return out


def test_core_replays_lane_and_wave_walks(tmp_path):
    """csrc/sbam_tag_core.h under the address and undefined-behaviour sanitizers: the hand-written lists (well-formed
    and malformed) at all four alignments, and 3000 random lists, each whole, cut at a random byte, and with one
    byte changed, walked as a lane and as a wave walk them, against find_tags' walk."""
    src, exe, data = tmp_path / "tag_replay.cpp", tmp_path / "tag_replay", tmp_path / "cases.bin"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    cases = []
    for _, aux in hand_lists() + malformed_lists() + big_lists()[:1]:
        cases += [(aux, a) for a in range(4)]
    rng = np.random.default_rng(0x7A65)
    for _ in range(3000):
        aux = random_list(rng)
        cases.append((aux, int(rng.integers(0, 4))))
        if aux:
            cases.append((aux[:int(rng.integers(0, len(aux)))], int(rng.integers(0, 4))))
            b = bytearray(aux)
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            cases.append((bytes(b), int(rng.integers(0, 4))))
    data.write_bytes(b"".join(struct.pack("<ii", len(aux), a) + aux for aux, a in cases))
    p = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines.pop() == f"long {LONG}"
    it = iter(lines)
    n_bad = 0
    for i, (aux, _) in enumerate(cases):
        want, ok = walked(aux)
        n_bad += not ok
        for mode in "LW":
            for w in want:
                assert tuple(map(int, next(it).split())) == w, (i, mode, aux[:64])
            assert next(it) == f"{i} {mode} {'ok' if ok else 'bad'}", (i, mode, aux[:64])
    assert next(it, None) is None
    assert n_bad > 1000 and len(cases) - n_bad > 3000


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_tag_struct_layouts_follow_the_header(tmp_path):
    """sizeof / offsetof of sbam_tag_query, sbam_record_tags and sbam_record_tag_totals as a C compiler lays out
    include/sbam.h, against the ctypes mirrors."""
    import sbam
    mirrors = {"sbam_tag_query": sbam._TagQuery, "sbam_record_tags": sbam._RecordTags,
               "sbam_record_tag_totals": sbam._RecordTagTotals}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{ROOT}/include/sbam.h"', "int main(void) {",
             '  printf("max %d\\n", SBAM_MAX_TAGS);']
    for t, cls in mirrors.items():
        lines.append(f'  printf("{t} sizeof %zu\\n", sizeof({t}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{t} {f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == f"max {sbam.MAX_TAGS}" == "max 32"
    seen = set()
    for ln in out[1:]:
        t, f, *v = ln.split()
        cls = mirrors[t]
        if f == "sizeof":
            assert int(v[0]) == ctypes.sizeof(cls), t
        else:
            assert (int(v[0]), int(v[1])) == (getattr(cls, f).offset, getattr(cls, f).size), (t, f)
        seen.add((t, f))
    assert len(seen) == sum(len(c._fields_) + 1 for c in mirrors.values())
    assert ctypes.sizeof(sbam._TagQuery) == 4 and ctypes.sizeof(sbam._RecordTags) == 32 + 2 * 8 * 32
    assert {"sbam_load_record_tags", "sbam_get_record_tags", "sbam_record_tags_device",
            "sbam_tag_long_aux_bytes"} <= set(sbam.EXPORTS)
    assert sbam.load_library().sbam_tag_long_aux_bytes() == LONG
