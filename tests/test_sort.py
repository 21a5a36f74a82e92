"""The coordinate sort on the GPU (sbam_sort_records, sbam_test_sort_keys) and the ordered writer
(sbam_write_bam_ordered).  Every comparison is exact: the order is the stable argsort of the 64-bit keys, restated here
in numpy from the record columns; an ordered write inflates to the header plus the records concatenated in that order
on the host."""
import ctypes
import gzip
import hashlib
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import record_stream_writer as rsw
from conftest import FIXTURES, ROOT, fixture_bytes
from test_write_bam import BB, check_bgzf

pytestmark = pytest.mark.gpu

SPLIT = 100000
SCAN_BLOCK = 1024  # elements one workgroup of launch_exclusive_scan covers (tests/test_scan.py)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def tile() -> int:
    import sbam
    return sbam.load_library().sbam_sort_tile_keys()


def numpy_keys(ref_id, pos) -> np.ndarray:
    r = np.asarray(ref_id, np.int32).view(np.uint32).astype(np.uint64)
    p = (np.asarray(pos, np.int32).view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return (r << np.uint64(32)) | p


def expected_passes(keys: np.ndarray) -> int:
    """No key below its predecessor: none.  Else one pass per byte that is not the same in every key."""
    if keys.size < 2 or not bool((keys[1:] < keys[:-1]).any()):
        return 0
    b = keys.view(np.uint8).reshape(-1, 8)
    return int((b != b[0]).any(axis=0).sum())


def sort_keys(keys: np.ndarray):
    """sbam_test_sort_keys -> (order, passes)."""
    import sbam
    L = sbam.load_library()
    keys = np.ascontiguousarray(keys, np.uint64)
    order = np.full(keys.size, -1, np.int64)
    passes = ctypes.c_int32(-1)
    rc = L.sbam_test_sort_keys(0, keys.ctypes.data if keys.size else None, keys.size,
                               order.ctypes.data if keys.size else None, ctypes.byref(passes))
    assert rc == sbam.SBAM_OK, rc
    return order, passes.value


# ---- 1. raw keys -------------------------------------------------------------------------------------------------
KINDS = ["random", "equal", "ascending_ties", "descending", "alternating"] + [f"byte{b}" for b in range(8)] + \
    ["bytes0and7", "first_tile_one_bucket", "digits_00_ff"]
BASE = 0x1122334455667788


def make_keys(kind: str, n: int, T: int) -> np.ndarray:
    rng = np.random.default_rng([n, KINDS.index(kind)])
    i = np.arange(n, dtype=np.uint64)
    if kind == "random":
        return rng.integers(0, 2**64, n, dtype=np.uint64)
    if kind == "equal":
        return np.full(n, BASE, np.uint64)
    if kind == "ascending_ties":
        return np.sort(rng.integers(0, max(n // 8, 1), n, dtype=np.uint64))
    if kind == "descending":
        return (np.uint64(1 << 40) + np.uint64(n) - i).astype(np.uint64)
    if kind == "alternating":
        return np.where(i % np.uint64(2) == 0, np.uint64(BASE + (1 << 33)), np.uint64(BASE)).astype(np.uint64)
    if kind.startswith("byte") and kind[4:].isdigit():  # digits n-1, n-2, ... mod 256 in byte b, the others constant
        b = int(kind[4:])
        d = (np.uint64(n) - np.uint64(1) - i) % np.uint64(256) if n else i
        return (np.uint64(BASE & ~(0xff << 8 * b)) | (d << np.uint64(8 * b))).astype(np.uint64)
    if kind == "bytes0and7":
        d0 = (i * np.uint64(7)) % np.uint64(256)
        d7 = (np.uint64(n) - np.uint64(1) - i) % np.uint64(256) if n else i
        return (np.uint64(BASE & 0x00ffffffffffff00) | d0 | (d7 << np.uint64(56))).astype(np.uint64)
    if kind == "first_tile_one_bucket":
        k = rng.integers(0, 2**64, n, dtype=np.uint64)
        k[:T] = np.uint64(0x8080808080808080)
        return k
    assert kind == "digits_00_ff"
    return (rng.integers(0, 2, (n, 8), dtype=np.uint8) * np.uint8(0xff)).view(np.uint64).reshape(n)


def sizes(T: int):
    big = SCAN_BLOCK * T + 1  # more tiles than one workgroup of the scan covers
    assert big <= 1 << 22
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T, 3 * T + 17, big]


@pytest.mark.parametrize("kind", KINDS)
def test_raw_keys_against_numpy_stable_argsort(kind):
    """Every size at which a wave, a row, a tile or the scan's workgroup fills up, for every kind of key: the order is
    numpy's stable argsort, and the passes are the bytes that vary (none for an input already in order)."""
    T = tile()
    for n in sizes(T):
        keys = make_keys(kind, n, T)
        order, passes = sort_keys(keys)
        assert np.array_equal(order, np.argsort(keys, kind="stable")), (kind, n)
        assert passes == expected_passes(keys), (kind, n, passes)
        if kind in ("equal", "ascending_ties"):
            assert passes == 0 and np.array_equal(order, np.arange(n)), (kind, n)
        if n >= 2 and kind.startswith("byte") and kind[4:].isdigit():
            assert passes == 1, (kind, n)
        if n >= 2 and kind == "bytes0and7":
            assert passes == 2, (kind, n)
        if n >= 64 and kind == "random":
            assert passes == 8, n


def test_same_input_twice_same_order():
    T = tile()
    for n in (3 * T + 17, SCAN_BLOCK * T + 1):
        for kind in ("random", "digits_00_ff", "alternating"):
            keys = make_keys(kind, n, T)
            a, pa = sort_keys(keys)
            b, pb = sort_keys(keys)
            assert np.array_equal(a, b) and pa == pb, (kind, n)


# ---- hand-built stream -------------------------------------------------------------------------------------------
CONTIGS = (1000, 5000, 70000, (1 << 24) + 5)


def bgzf(u: bytes, piece: int = 60000) -> bytes:
    out = b""
    for o in range(0, len(u), piece):
        c = u[o:o + piece]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        d = co.compress(c) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(d) + 25) + d
        out += struct.pack("<II", zlib.crc32(c), len(c))
    return out + EOF_BLOCK


def hand_records(n: int):
    """n short unmapped-flag records on four references and on none, seeded: ref_id in [-1, 4) with the -1 records
    scattered; pos from a small set per reference (so duplicates abound) that holds -1, 0 and the contig's length."""
    rng = np.random.default_rng(0x50A7)
    ref = rng.integers(-1, 4, n)
    recs = []
    for i in range(n):
        r = int(ref[i])
        top = CONTIGS[r] if r >= 0 else 50
        choices = [-1, 0, 1, 7, 7, top // 2, top - 1, top, int(rng.integers(0, top + 1))]
        recs.append(rsw.record(ref_id=r, pos=int(choices[int(rng.integers(0, len(choices)))]), name=b"r%d" % i))
    return recs


@pytest.fixture(scope="module")
def hand():
    import sbam
    T = tile()
    recs = hand_records(3 * T + 17)
    head = rsw.header(CONTIGS)
    with sbam.BamFile(bgzf(head + b"".join(recs)), path="hand.bam") as f:
        _, cols = f.load_records(32 << 20, columns=("offset", "block_size", "ref_id", "pos"))
        assert f.n_loaded == len(recs)
        yield f, cols, recs, head


def err_code(f) -> int:
    return f.L.sbam_last_error(f.ctx).contents.code


# ---- 2. sbam_sort_records ----------------------------------------------------------------------------------------
def test_sort_records_on_hand_built_stream(hand):
    import sbam
    f, cols, recs, _ = hand
    N, T = len(recs), tile()
    keys = numpy_keys(cols["ref_id"], cols["pos"])
    assert (cols["ref_id"] == -1).sum() > 100 and (cols["pos"] == -1).sum() > 100 and (cols["pos"] == 0).sum() > 100
    assert any(int((cols["pos"][cols["ref_id"] == r] == CONTIGS[r]).sum()) > 0 for r in range(4))
    want = np.argsort(keys, kind="stable")
    t = f.sort_records()
    assert t == {"n_records": N, "n_out_of_order": int((keys[1:] < keys[:-1]).sum()), "passes": expected_passes(keys)}
    assert t["n_out_of_order"] > N // 4 and 1 <= t["passes"] <= 8
    assert np.array_equal(f.sort_order(), want)
    assert cols["ref_id"][want[-1]] == -1 and cols["ref_id"][want[0]] == 0 and cols["pos"][want[0]] == -1
    for i0, n in ((0, 0), (0, 1), (T - 1, 2), (T, T + 1), (N - 5, 5), (N, 0)):
        assert np.array_equal(f.sort_order(i0, n), want[i0:i0 + n]), (i0, n)
    with pytest.raises(sbam.SbamError):
        f.sort_order(N - 1, 2)
    assert err_code(f) == sbam.ERR_ARG
    assert f.kernel_ms("sort") > 0 and 0 < f.kernel_ms("sort_keys") <= f.kernel_ms("sort")
    assert f.sort_records() == t and np.array_equal(f.sort_order(), want)  # (again: the same)


# ---- 3. ordered write --------------------------------------------------------------------------------------------
def starts_of(head_len: int, recs) -> np.ndarray:
    sizes_ = np.asarray([len(r) for r in recs], np.int64)
    return head_len + np.concatenate([[0], np.cumsum(sizes_)[:-1]]) if sizes_.size else np.zeros(0, np.int64)


def check_written(f, r, head: bytes, recs):
    """The output inflates to head + recs; the totals and written_records() say so."""
    want = head + b"".join(recs)
    check_bgzf(r["bytes"], want)
    assert r["n_records"] == len(recs) and r["ubytes"] == len(want) and r["header_bytes"] == len(head)
    st, _, _ = f.written_blocks()
    bp, bo = f.written_records()
    assert np.array_equal(np.searchsorted(st, bp) * BB + bo, starts_of(len(head), recs))


@pytest.mark.parametrize("level, huffman", [(0, "fixed"), (1, "fixed"), (1, "dynamic")])
def test_ordered_write_explicit_shuffle(hand, level, huffman):
    """order = a seeded shuffle (numpy, uploaded): the records come out in that sequence; ranges and keep select by
    loaded index and leave the sequence alone."""
    f, cols, recs, head = hand
    N = len(recs)
    perm = np.random.default_rng(3).permutation(N).astype(np.int64)
    r = f.write_bam(order=perm, level=level, huffman=huffman)
    check_written(f, r, head, [recs[i] for i in perm.tolist()])
    ranges = [(5, 900), (900, 901), (N - 2000, N - 3)]
    keep = np.random.default_rng(4).integers(0, 3, N) > 0
    mask = np.zeros(N, bool)
    for lo, hi in ranges:
        mask[lo:hi] = True
    mask &= keep
    assert 0 < mask.sum() < N
    r = f.write_bam(order=perm, ranges=ranges, keep=keep, level=level, huffman=huffman)
    check_written(f, r, head, [recs[i] for i in perm.tolist() if mask[i]])
    r = f.write_bam(order=perm, ranges=[(7, 7)], level=level, huffman=huffman)
    check_written(f, r, head, [])


@pytest.mark.parametrize("level, huffman", [(0, "fixed"), (1, "fixed"), (1, "dynamic")])
def test_null_order_is_the_last_sort(hand, level, huffman):
    f, cols, recs, head = hand
    f.sort_records()
    order = f.sort_order()
    a = f.write_bam(order="sorted", level=level, huffman=huffman)
    check_written(f, a, head, [recs[i] for i in order.tolist()])
    b = f.write_bam(order=order, level=level, huffman=huffman)
    assert a["bytes"] == b["bytes"]
    plain = f.write_bam(level=level, huffman=huffman)  # the unordered writer, on the same context
    check_written(f, plain, head, recs)
    assert plain["bytes"] == f.write_bam(order=np.arange(len(recs)), level=level, huffman=huffman)["bytes"]


_TENSOR_CHILD = """
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
import sbam
with sbam.BamFile(open(sys.argv[1], "rb").read()) as f:
    f.load_records(int(sys.argv[3]), columns=None)
    perm = np.random.default_rng(11).permutation(f.n_loaded).astype(np.int64)
    order = torch.from_numpy(perm).to("cuda:0")
    assert order.is_cuda and order.dtype == torch.int64
    f.write_bam(sys.argv[2], order=order)
"""


def test_order_device_tensor(tmp_path):
    """order as a torch int64 tensor on the device: its pointer goes to the kernel as it is, and the file is the one the
    same shuffle gives as a numpy array.  (A child process that initialises torch first, as for keep.)"""
    import sbam
    out = tmp_path / "shuffled.bam"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "spark-bam_amd"))
    p = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, os.path.join(FIXTURES, "5k.bam"), str(out), str(SPLIT)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with sbam.BamFile(fixture_bytes("5k.bam"), path="5k.bam") as f:
        f.load_records(SPLIT, columns=None)
        perm = np.random.default_rng(11).permutation(f.n_loaded).astype(np.int64)
        assert f.write_bam(order=perm)["bytes"] == out.read_bytes()


def test_plain_write_keeps_the_parents_bytes():
    """sbam_write_bam after a sort and an ordered write on the same context: records 100-1000 of 2.bam at levels 0 and
    1 without the EOF block have the SHA-256 the golden file records for the inflated 2.100-1000.bam."""
    import sbam
    with open(os.path.join(ROOT, "tests", "golden", "write_level1_digests.json")) as fh:
        gold = json.load(fh)["digests"]
    with sbam.BamFile(fixture_bytes("2.bam"), path="2.bam") as f:
        f.load_records(SPLIT, columns=None)
        f.sort_records()
        f.write_bam(order="sorted")
        for level in (0, 1):
            got = f.write_bam(ranges=[(100, 1000)], level=level, with_eof=False)["bytes"]
            assert hashlib.sha256(got).hexdigest() == gold[f"level{level}:2.100-1000.bam:bb0:noeof"], level


# ---- 4. round trip -----------------------------------------------------------------------------------------------
def split_stream(u: bytes):
    """(header bytes, [record bytes]) of an inflated BAM."""
    i32 = lambda x: struct.unpack_from("<i", u, x)[0]  # noqa: E731
    x = 12 + i32(4)
    for _ in range(i32(8 + i32(4))):
        x += 8 + i32(x)
    head, recs = u[:x], []
    while x < len(u):
        n = 4 + i32(x)
        recs.append(u[x:x + n])
        x += n
    assert x == len(u)
    return head, recs


def record_keys(recs) -> np.ndarray:
    a = np.asarray([struct.unpack_from("<ii", r, 4) for r in recs], np.int64).reshape(-1, 2)
    return numpy_keys(a[:, 0].astype(np.int32), a[:, 1].astype(np.int32))


def shuffled(name: str, seed: int):
    """(bytes of the fixture with its records in a seeded shuffle, those records in that sequence, the header)."""
    import sbam
    head, recs = split_stream(gzip.decompress(fixture_bytes(name)))
    with sbam.BamFile(fixture_bytes(name), path=name) as f:
        f.load_records(SPLIT, columns=None)
        assert f.n_loaded == len(recs)
        perm = np.random.default_rng(seed).permutation(len(recs)).astype(np.int64)
        data = f.write_bam(order=perm)["bytes"]
    mixed = [recs[i] for i in perm.tolist()]
    assert gzip.decompress(data) == head + b"".join(mixed)
    return data, mixed, head


def check_sorted_file(out: bytes, mixed, head: bytes):
    """`out` holds the records of `mixed` in the host's stable coordinate order behind `head` with SO:coordinate, passes
    the CRC check, counts no unsorted record and indexes without complaint.  Returns its .bai bytes."""
    import sbam
    from sbam import sam
    keys = record_keys(mixed)
    assert bool((keys[1:] < keys[:-1]).any())
    want = [mixed[i] for i in np.argsort(keys, kind="stable").tolist()]
    got_head, got = split_stream(gzip.decompress(out))
    assert got == want
    assert sorted(got) == sorted(mixed)
    assert got_head == sam.header_with_sort_order(head, "coordinate")
    (lt,) = struct.unpack_from("<i", got_head, 4)
    assert b"SO:coordinate" in got_head[8:8 + lt].split(b"\n")[0]
    with sbam.BamFile(out, path="sorted.bam") as h:
        assert h.check_crc()["n_bad"] == 0
        idx = h.build_index(SPLIT)
        assert idx["n_unsorted"] == 0 and idx["n_records"] == len(mixed)
        return h.build_bai(SPLIT, require_sorted=True)


@pytest.mark.parametrize("name", ["5k.bam", "2.bam"])
def test_round_trip(name):
    import sbam
    from sbam import sam
    data, mixed, head = shuffled(name, 20)
    with sbam.BamFile(data, path="shuffled.bam") as g:
        g.load_records(SPLIT, columns=None)
        with pytest.raises(sbam.SbamError, match="unsorted positions"):
            g.build_bai(SPLIT, require_sorted=True)
        t = g.sort_records()
        keys = record_keys(mixed)
        assert t["n_out_of_order"] == int((keys[1:] < keys[:-1]).sum()) > 0 and t["passes"] == expected_passes(keys)
        out = g.write_bam(order="sorted", header=sam.header_with_sort_order(g.header_bytes(), "coordinate"))["bytes"]
    assert len(check_sorted_file(out, mixed, head)) > 8


# ---- 5. state and arguments --------------------------------------------------------------------------------------
def test_state():
    """Sort, or an ordered write without an order, before load_records / before a sort: SBAM_ERR_STATE.  reset, load and
    a second load_records drop the order; fields, an index and a write do not."""
    import sbam
    data = fixture_bytes("2.bam")
    with sbam.BamFile(data, path="2.bam") as f:
        for call in (f.sort_records, f.sort_order, lambda: f.write_bam(order="sorted")):
            with pytest.raises(sbam.SbamError):
                call()
            assert err_code(f) == sbam.ERR_STATE
        f.load_records(SPLIT, columns=None)
        for call in (f.sort_order, lambda: f.write_bam(order="sorted")):
            with pytest.raises(sbam.SbamError):
                call()
            assert err_code(f) == sbam.ERR_STATE
        for redo in (lambda: (f.reset(), f.run()), lambda: (f.load(data), f.run()), lambda: None):
            f.sort_records()
            order = f.sort_order()
            f.load_record_fields(0, 10)
            f.build_index(SPLIT)
            f.write_bam()
            assert np.array_equal(f.sort_order(), order)
            redo()
            f.load_records(SPLIT, columns=None)
            for call in (f.sort_order, lambda: f.write_bam(order="sorted")):
                with pytest.raises(sbam.SbamError):
                    call()
                assert err_code(f) == sbam.ERR_STATE


def test_arguments(hand):
    import sbam
    f, cols, recs, head = hand
    N = len(recs)
    perm = np.random.default_rng(5).permutation(N).astype(np.int64)
    for at, v in ((5, N), (N - 1, -1), (0, 1 << 40)):
        assert f.write_bam()["n_records"] == N
        bad = perm.copy()
        bad[at] = v
        with pytest.raises(sbam.SbamError):
            f.write_bam(order=bad)
        assert err_code(f) == sbam.ERR_ARG
        assert f.L.sbam_get_written(f.ctx, None, 0) == sbam.ERR_STATE  # the previous file is gone, as after any failure
    with pytest.raises(ValueError):
        f.write_bam(order=perm[:-1])
    for kw in ({"header": head, "with_header": False}, {"header": b"BAN\x01" + head[4:]}, {"header": head + b"\0"},
               {"header": head[:-1]}, {"header": head[:8]}):
        with pytest.raises(sbam.SbamError):
            f.write_bam(order=perm, **kw)
        assert err_code(f) == sbam.ERR_ARG, kw
    # a header of another length, and no order beside it: the loaded order behind the new header
    other = rsw.header(CONTIGS, text=b"@HD\tVN:1.6\tSO:unsorted\n@CO\tsomething longer than before\n")
    check_written(f, f.write_bam(header=other), other, recs)
    check_written(f, f.write_bam(header=other, order=perm), other, [recs[i] for i in perm.tolist()])
    # a repeated entry is written twice
    twice = perm.copy()
    twice[1] = twice[0]
    check_written(f, f.write_bam(order=twice), head, [recs[i] for i in twice.tolist()])


# ---- 6. CLI ------------------------------------------------------------------------------------------------------
def test_cli_sort_index(tmp_path, capsys):
    from sbam import bai, cli
    data, mixed, head = shuffled("2.bam", 21)
    src, out = tmp_path / "shuffled.bam", tmp_path / "sorted.bam"
    src.write_bytes(data)
    assert cli.main(["sort", "--index", "-o", str(out), str(src)]) == 0
    want_bai = check_sorted_file(out.read_bytes(), mixed, head)
    got_bai = (tmp_path / "sorted.bam.bai").read_bytes()
    assert got_bai == want_bai
    n_ref = struct.unpack_from("<i", head, 8 + struct.unpack_from("<i", head, 4)[0])[0]
    assert len(bai.parse_bai(got_bai)) == n_ref
    keys = record_keys(mixed)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith(f"{len(mixed)} records, {int((keys[1:] < keys[:-1]).sum())} out of order before the sort, "
                           f"{expected_passes(keys)} passes, ")
