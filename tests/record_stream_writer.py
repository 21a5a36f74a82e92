"""An uncompressed BAM stream writer for the tests (SAM spec 4.2): records whose every field, length and block_size
is chosen by the test instead of by an encoder, so that the stream can hold what no BAM writer emits.

A *decoy* is a record-shaped run of bytes inside a true record's aux tail.  The checker, which looks at every stream
offset, may call it a record start; RecordStream, which walks from record to record by block_size alone, never visits
it.  A decoy's block_size is free, so its hop (offset + 4 + block_size) can land on the next true record (the checker
then follows the true chain and the call survives any reads_to_check), a few bytes off it, on another decoy, on or past
the stream's end, or inside the decoy itself.

`Stream` returns, beside the bytes, the offsets of the true records, of the decoys and of each decoy's hop target, so
a test can put any of them on an exact offset (`fill_to`) and look its bit up in the oracle's answer."""
import struct

FIXED = 36  # block_size + the 32 fixed bytes
TINY = 38   # an unmapped record named "r": no CIGAR, l_seq = 0, no aux


def header(contig_lengths=(1000,), text: bytes = b"@HD\tVN:1.6\n") -> bytes:
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contig_lengths))
    for i, n in enumerate(contig_lengths):
        name = b"c%d\x00" % i
        out += struct.pack("<i", len(name)) + name + struct.pack("<i", n)
    return out


def filler(n: int) -> bytes:
    """n aux bytes that no record check passes over: one Z tag of 'A's (a refID of 0x41414141 is past any contig
    table), or zeros when too short for a tag."""
    return b"XAZ" + b"A" * (n - 4) + b"\x00" if n >= 4 else b"\x00" * n


def record(ref_id: int = -1, pos: int = -1, name: bytes = b"r", mapq: int = 0, bin_: int = 4680, flag: int = 4,
           cigar=(), seq: bytes = b"", qual: bytes = b"", l_seq=None, next_ref_id: int = -1, next_pos: int = -1,
           tlen: int = 0, aux: bytes = b"", block_size=None, l_read_name=None, n_cigar_op=None,
           raw_name=None) -> bytes:
    """One record.  `name` is written with its NUL (`raw_name`, when given, replaces both: the name field's bytes as
    they stand, with or without a NUL); `cigar` holds raw uint32 ops (len << 4 | op); `seq` the packed bases; l_seq,
    l_read_name, n_cigar_op and block_size default to what the bytes say and can each be overridden."""
    nm = name + b"\x00" if raw_name is None else bytes(raw_name)
    lrn = len(nm) if l_read_name is None else l_read_name
    nc = len(cigar) if n_cigar_op is None else n_cigar_op
    ls = len(qual) if l_seq is None else l_seq
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, lrn, mapq, bin_, nc, flag, ls, next_ref_id, next_pos, tlen)
    body += nm + b"".join(struct.pack("<I", op) for op in cigar) + seq + qual + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def _i32(v: int) -> int:
    return (v + 2**31) % 2**32 - 2**31


def implied_size(l_read_name: int, n_cigar_op: int, l_seq: int) -> int:
    """The least block_size full/Checker.scala:68-71 accepts: 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq
    in Java Int arithmetic (every sum wraps at 32 bits, '/' truncates toward zero)."""
    t = _i32(l_seq + 1)
    half = -(-t // 2) if t < 0 else t // 2
    return _i32(32 + l_read_name + 4 * n_cigar_op + _i32(half + l_seq))


def sized(n: int, **kw) -> bytes:
    """A true record of exactly n >= 38 bytes: the tiny record with n - 38 aux bytes of filler."""
    assert n >= TINY, n
    r = record(aux=filler(n - TINY), **kw)
    assert len(r) == n
    return r


class Stream:
    """The stream under construction.  records / decoys / targets are stream offsets; targets[i] is where decoys[i]
    hops to."""

    def __init__(self, contig_lengths=(1000,)):
        self.contig_lengths = tuple(contig_lengths)
        self.u = bytearray(header(contig_lengths))
        self.header_end = len(self.u)
        self.records, self.decoys, self.targets = [], [], []
        self._late = []  # (decoy index, delta): hops resolved against the final length

    def __len__(self):
        return len(self.u)

    def add(self, rec: bytes) -> int:
        """Append a true record (any bytes whose block_size spans them); returns its offset."""
        x = len(self.u)
        self.records.append(x)
        self.u += rec
        return x

    def junk(self, raw: bytes) -> int:
        """Append bytes that are no record (a tail)."""
        x = len(self.u)
        self.u += raw
        return x

    def tiny(self, n: int = 1, **kw):
        for _ in range(n):
            self.add(record(**kw))

    def fill_to(self, x: int, big: int = 0):
        """True records up to exactly offset x (at least 38 bytes away, or already there): `big`-byte records while
        they fit (0: tiny ones), the last one sized to end on x."""
        gap = x - len(self.u)
        assert gap == 0 or gap >= TINY, (x, len(self.u))
        step = max(big, TINY)
        while x - len(self.u) >= step + TINY:
            self.add(sized(step))
        if x > len(self.u):
            self.add(sized(x - len(self.u)))
        assert len(self.u) == x

    def host(self, decoy=None, at: int = 0, pad: int = 0, hop="next", n_decoys: int = 1, **kw):
        """A true record whose aux tail is `at` filler bytes, n_decoys decoys back to back and `pad` filler bytes.
        decoy: the decoy's bytes (default: the tiny record); its block_size is rewritten for the hop:
          "next"        the next true record (the host's end)           ("next", d): d bytes past it
          "chain"       the following decoy of this host, the last one to the host's end
          ("abs", x)    stream offset x                                 ("end", d): d bytes past the final length
          ("self", b)   block_size b as given (a hop inside the decoy)
        Returns (host offset, [decoy offsets])."""
        d = record() if decoy is None else bytes(decoy)
        h = len(self.u)
        first = h + TINY + at
        end = first + n_decoys * len(d) + pad
        self.add(record(aux=filler(at) + d * n_decoys + filler(pad), **kw))
        assert len(self.u) == end
        at_ = []
        for k in range(n_decoys):
            x = first + k * len(d)
            kind, arg = hop if isinstance(hop, tuple) else (hop, 0)
            if kind == "next":
                t = end + arg
            elif kind == "chain":
                t = x + len(d) if k + 1 < n_decoys else end
            elif kind == "abs":
                t = arg
            elif kind == "self":
                t = x + 4 + arg
            elif kind == "end":
                t = None
                self._late.append((len(self.decoys), arg))
            else:
                raise ValueError(hop)
            self.decoys.append(x)
            self.targets.append(t)
            if t is not None:
                self._patch(x, t)
            at_.append(x)
        return h, at_

    def _patch(self, x: int, target: int):
        self.u[x:x + 4] = struct.pack("<i", target - x - 4)

    def finish(self):
        """(bytes, {"records", "decoys", "targets", "header_end", "L"})."""
        L = len(self.u)
        for i, d in self._late:
            self.targets[i] = L + d
            self._patch(self.decoys[i], L + d)
        self._late = []
        return bytes(self.u), {"records": list(self.records), "decoys": list(self.decoys),
                               "targets": list(self.targets), "header_end": self.header_end, "L": L}
