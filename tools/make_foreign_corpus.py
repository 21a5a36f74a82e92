#!/usr/bin/env python3
"""Writes tests/golden/deflate/libdeflate_l{1,6,9,12}.bgzf and corpus.json: BGZF files whose payloads come from
libdeflate (the encoder behind most htslib builds) instead of zlib, for tests/test_inflate_foreign.py.  The inputs are
deterministic: consecutive 65280-byte chunks of the inflated tests/fixtures/2.bam and 5k.bam, and a few of
test_inflate_streams.sample_inputs(0).  libdeflate is looked up on this machine only; the tests read the committed
files and need no libdeflate.

    python tools/make_foreign_corpus.py          # rewrite the files
"""
import ctypes
import ctypes.util
import glob
import hashlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "deflate")
LEVELS = (1, 6, 9, 12)
CHUNK = 65280
BAM_CHUNKS = {"2.bam": 4, "5k.bam": 4}
SAMPLES = (1, 3, 15, 16, 17)  # of sample_inputs(0): the dist-1 run, periods 3 and 200, read-name text, far repeats


def load_libdeflate():
    """The libdeflate shared library, or None when this machine has none."""
    names = [ctypes.util.find_library("deflate")]
    names += sorted(glob.glob(os.path.join(sys.prefix, "lib", "libdeflate.so*")))
    for n in names:
        if not n:
            continue
        try:
            lib = ctypes.CDLL(n)
        except OSError:
            continue
        lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
        lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
        lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
        lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                                    ctypes.c_size_t]
        lib.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t
        lib.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
        return lib
    return None


def inflate_bgzf(data: bytes) -> bytes:
    out, pos = [], 0
    while pos < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[pos:]))
        pos = len(data) - len(d.unused_data)
    return b"".join(out)


def inputs():
    from test_inflate_streams import sample_inputs
    res = []
    for name, n in BAM_CHUNKS.items():
        with open(os.path.join(ROOT, "tests", "fixtures", name), "rb") as f:
            u = inflate_bgzf(f.read())
        assert len(u) >= n * CHUNK
        res += [u[i * CHUNK:(i + 1) * CHUNK] for i in range(n)]
    s = sample_inputs(0)
    return res + [s[i] for i in SAMPLES]


def build_file(lib, level: int) -> bytes:
    from test_inflate_streams import EOF_BLOCK, bgzf_block
    c = lib.libdeflate_alloc_compressor(level)
    assert c
    blocks = []
    for x in inputs():
        buf = ctypes.create_string_buffer(lib.libdeflate_deflate_compress_bound(c, len(x)))
        n = lib.libdeflate_deflate_compress(c, x, len(x), buf, len(buf))
        assert n and zlib.decompress(buf.raw[:n], -15) == x
        blocks.append(bgzf_block(buf.raw[:n], len(x)))
    lib.libdeflate_free_compressor(c)
    return b"".join(blocks) + EOF_BLOCK


def main():
    lib = load_libdeflate()
    if lib is None:
        sys.exit("libdeflate is not on this machine")
    os.makedirs(OUT, exist_ok=True)
    raw = b"".join(inputs())
    man = {}
    for level in LEVELS:
        name = "libdeflate_l%d.bgzf" % level
        data = build_file(lib, level)
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        man[name] = {"level": level, "blocks": len(inputs()), "bytes": len(raw),
                     "sha256": hashlib.sha256(raw).hexdigest(), "file_bytes": len(data)}
        print(name, len(data), "bytes")
    with open(os.path.join(OUT, "corpus.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
