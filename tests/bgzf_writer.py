"""A BGZF (SAM spec 4.1) member writer for the tests: blocks whose sizes, header lengths and file offsets are chosen by
the test instead of by an encoder, so that headers land on exact offsets (scan-chunk and workgroup-step edges), blocks
are small enough to overflow the scan's per-chunk slots, XLEN differs from htsjdk's 6, blocks are empty without being
the EOF marker, and header-shaped byte patterns sit inside payloads.

Every member carries the real CRC32 and ISIZE of its payload.  A stored member holds one stored DEFLATE block (RFC 1951
3.2.4: BFINAL = 1, BTYPE = 00, LEN, NLEN, the bytes), so its payload bytes appear verbatim in the file, 23 + len(extra)
bytes after the member's start."""
import struct
import zlib

import numpy as np

MAGIC = b"\x1f\x8b\x08\x04"
STORED_OVERHEAD = 31  # 18-byte header + 5-byte stored-block header + 8-byte footer
MAX_STORED = 65536 - STORED_OVERHEAD  # BSIZE - 1 is a uint16


def _member(deflate: bytes, payload: bytes, extra: bytes = b"") -> bytes:
    xlen = 6 + len(extra)
    bsize = 12 + xlen + len(deflate) + 8
    assert bsize <= 65536, bsize
    hdr = MAGIC + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", xlen) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return hdr + extra + deflate + struct.pack("<II", zlib.crc32(payload), len(payload))


def stored_block(payload: bytes, extra: bytes = b"") -> bytes:
    """One member of 31 + len(extra) + len(payload) bytes holding `payload` as a single stored DEFLATE block;
    XLEN = 6 + len(extra), with `extra` (further subfields) after the BC subfield."""
    payload = bytes(payload)
    n = len(payload)
    assert n <= MAX_STORED - len(extra)
    return _member(b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + payload, payload, extra)


def deflated_block(payload: bytes, level: int = 6, extra: bytes = b"") -> bytes:
    payload = bytes(payload)
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return _member(co.compress(payload) + co.flush(), payload, extra)


def eof_marker() -> bytes:
    """The 28-byte empty block every BGZF writer ends a file with (a 2-byte deflate payload: what MetadataStream
    stops at)."""
    return _member(b"\x03\x00", b"")


def fake_header(bsize_minus_1: int, xlen: int = 6) -> bytes:
    """The 18 bytes of a BGZF header with this BSIZE - 1, to plant inside a payload."""
    return MAGIC + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", xlen) + b"BC" + struct.pack("<HH", 2, bsize_minus_1)


def candidates(blob) -> np.ndarray:
    """Positions q of every header match (Header.make's seven checked bytes: 0-3 = 1f 8b 08 04 and 12-14 = 'B' 'C' 02)
    with q + 18 <= len(blob), ascending."""
    d = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob
    n = d.size - 17
    if n <= 0:
        return np.zeros(0, np.int64)
    hit = np.ones(n, bool)
    for k, v in ((0, 0x1f), (1, 0x8b), (2, 0x08), (3, 0x04), (12, 0x42), (13, 0x43), (14, 0x02)):
        hit &= d[k:k + n] == v
    return np.flatnonzero(hit).astype(np.int64)


def stored_file(u: bytes, payload: int, starts=(), marker: bool = True, total=None) -> bytes:
    """`u` as stored members of `payload` bytes each, except that members are shortened so that one starts at each
    file offset in `starts` (ascending, at least 2 * (payload + 31) apart), and, with `total`, the last payload is cut so
    that the whole file (EOF marker included when `marker`) is exactly `total` bytes long (`u` must be long enough)."""
    out, at, x = [], 0, 0
    todo = sorted(starts)
    tail = len(eof_marker()) if marker else 0
    while x < len(u):
        n = min(payload, len(u) - x)
        goal = todo[0] if todo else (total - tail if total is not None else None)
        if goal is not None and goal - at < 2 * (payload + STORED_OVERHEAD):
            gap = goal - at  # one member if it fits, else two of about half each
            n = gap - STORED_OVERHEAD if gap <= payload + STORED_OVERHEAD else gap // 2 - STORED_OVERHEAD
            assert 0 <= n <= len(u) - x, (goal, at, n)
        b = stored_block(u[x:x + n])
        out.append(b)
        at += len(b)
        x += n
        if todo and at == todo[0]:
            todo.pop(0)
        elif not todo and total is not None and at == total - tail:
            break
    assert not todo, todo
    if marker:
        out.append(eof_marker())
    blob = b"".join(out)
    assert total is None or len(blob) == total, (len(blob), total)
    return blob
