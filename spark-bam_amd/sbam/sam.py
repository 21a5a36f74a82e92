"""SAM text of decoded records: the eleven mandatory columns plus tags, as htsjdk (SAMTextWriter) and samtools print
them, from the fixed-field columns of `BamFile.load_records` and the CSR columns of `BamFile.load_record_fields`.

Pinned by the reference's 2.sam / 5k.sam (the SAM text of 2.bam / 5k.bam that LoadSAMTest compares loadSam against
loadBam with): tests/test_sam_text.py.  Rules (SAM spec §1.4, §1.5, §4.2):

* POS and PNEXT are the stored 0-based values + 1; RNAME is `*` for ref_id < 0; RNEXT is `*` for next_ref_id < 0, `=`
  when it equals a non-negative ref_id, else the contig's name;
* CIGAR is `*` for 0 ops, letters `MIDNSHP=X`; SEQ is `*` for l_seq = 0; QUAL is `*` for l_seq = 0 or a first byte
  of 0xFF, else byte + 33;
* tags keep file order; the integer types c C s S i I all print as `i`; A, Z and H print as stored; B prints as
  `B:<t>,v,v…`; f prints in Python's shortest round-trip form.  No reference fixture has an `f` or a `B` tag: the
  text of those two is parity unpinned.

`find_tags` states the rules of `BamFile.load_record_tags` (sbam_load_record_tags) for one record's tag bytes, and
`tag_value_text` renders one decoded tag; `tag_texts` is built from the same walk and the same formatting.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Sequence

import numpy as np

CIGAR_OPS = "MIDNSHP=X"
_INT_TAGS = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4)}


def _float_text(v: float) -> str:
    """repr's shortest round-trip form, for the float32 the tag holds (1.5, 3.0, 0.1, 1e+10)."""
    return str(np.float32(v))


def _array_text(st: str, raw: bytes) -> str:
    """`B:<t>,v,v…` of a B array's element bytes."""
    if st == "f":
        vals = [_float_text(v) for v in struct.unpack(f"<{len(raw) // 4}f", raw)]
    else:
        fmt, w = _INT_TAGS[st]
        vals = [str(v) for v in struct.unpack(f"<{len(raw) // w}{fmt[1]}", raw)]
    return f"B:{st}" + "".join("," + v for v in vals)


def tag_value_text(type_: str, sub: str, value: int, raw: bytes = b"") -> str:
    """`t:value` of one decoded tag as SAM prints it (`i:3`, `Z:grp1`, `A:U`, `f:1.5`, `B:c,1,2,3`), from what
    find_tags and the columns of load_record_tags give: the stored type, a B array's subtype, the value column's
    entry, and the value's bytes (needed for Z, H and B)."""
    if type_ in _INT_TAGS:
        return f"i:{int(value)}"
    if type_ == "A":
        return f"A:{chr(int(value))}"
    if type_ == "f":
        return "f:" + _float_text(struct.unpack("<f", struct.pack("<I", int(value) & 0xffffffff))[0])
    if type_ in "ZH":
        return f"{type_}:{bytes(raw).decode('latin-1')}"
    if type_ == "B":
        return _array_text(sub, bytes(raw))
    raise ValueError(f"unknown tag type {type_!r}")


_SCALAR_WIDTH = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _walk_tags(aux: bytes):
    """(name, type, sub, rel, value, raw) of every tag of one record's raw tag bytes (SAM spec §4.2.4), in file order;
    ValueError for a malformed list.  `rel` is the offset of the value's first byte (B: of its first element), `value`
    what the value column of sbam_load_record_tags holds, `raw` the bytes of a Z, H or B value (else empty)."""
    p, n = 0, len(aux)
    while p < n:
        if n - p < 3:
            raise ValueError(f"truncated tag header at byte {p} of {n}")
        name, t = aux[p:p + 2], chr(aux[p + 2])
        left = n - p
        if t in _SCALAR_WIDTH:
            w = _SCALAR_WIDTH[t]
            if 3 + w > left:
                raise ValueError(f"value of tag at byte {p} runs past the record's end")
            raw4 = aux[p + 3:p + 3 + w]
            if t in _INT_TAGS:
                v = struct.unpack(_INT_TAGS[t][0], raw4)[0]
            else:  # A: the byte; f: the 32 IEEE bits
                v = int.from_bytes(raw4, "little")
            yield name, t, "", p + 3, v, b""
            p += 3 + w
        elif t in "ZH":
            e = aux.find(b"\0", p + 3)
            if e < 0:
                raise ValueError(f"{t} value at byte {p} has no NUL before the record's end")
            yield name, t, "", p + 3, e - p - 3, aux[p + 3:e]
            p = e + 1
        elif t == "B":
            if left < 8:
                raise ValueError(f"B header at byte {p} runs past the record's end")
            st = chr(aux[p + 3])
            cnt = struct.unpack_from("<i", aux, p + 4)[0]
            if st not in _SCALAR_WIDTH or st == "A":
                raise ValueError(f"unknown B subtype {st!r} at byte {p}")
            w = _SCALAR_WIDTH[st]
            if cnt < 0 or 8 + cnt * w > left:
                raise ValueError(f"B array at byte {p}: count {cnt} is negative or runs past the record's end")
            yield name, t, st, p + 8, cnt, aux[p + 8:p + 8 + cnt * w]
            p += 8 + cnt * w
        else:
            raise ValueError(f"unknown tag type {t!r} at byte {p}")


def find_tags(aux: bytes, tags) -> list:
    """The host statement of sbam_load_record_tags' rules for one record: per queried two-character tag name, None
    when the record has no such tag, else (type, sub, rel, value, raw_bytes) of its first occurrence.  The whole list
    is walked whatever is queried; ValueError for every malformed case (fewer than 3 bytes for a header, an unknown
    type, a value past the end, a Z or H without a NUL, a B with an unknown subtype, a negative count or elements
    past the end).  The tests' oracle; not on the data path."""
    want = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in tags]
    first = {}
    for name, t, st, rel, v, raw in _walk_tags(bytes(aux)):
        first.setdefault(name, (t, st, rel, v, raw))
    return [first.get(w) for w in want]


def tag_texts(aux: bytes) -> List[str]:
    """`TG:t:value` for each tag of one record's raw tag bytes (SAM spec §4.2.4), in file order."""
    return [f"{name.decode('latin-1')}:{tag_value_text(t, st, v, raw)}" for name, t, st, _, v, raw in _walk_tags(aux)]


def cigar_text(ops: np.ndarray) -> str:
    if ops.size == 0:
        return "*"
    return "".join(f"{int(op) >> 4}{CIGAR_OPS[int(op) & 15]}" for op in ops)


def sam_lines(columns: Dict[str, np.ndarray], fields, contig_names: Sequence[str]) -> List[str]:
    """One SAM line (no newline) per record of a batch.  `columns`: the batch's fixed-field columns (ref_id, pos,
    bin_mq_nl, flag_nc, next_ref_id, next_pos, tlen: `load_records` columns sliced to the batch); `fields`: the
    batch's RecordFields with all five data columns; `contig_names`: the header's reference names."""
    n = int(fields.n)
    no, co, so, ao = (np.asarray(getattr(fields, k)).tolist() for k in ("name_off", "cigar_off", "seq_off", "aux_off"))
    names = np.asarray(fields.name, np.uint8).tobytes()
    seqs = np.asarray(fields.seq, np.uint8).tobytes()
    quals = np.asarray(fields.qual, np.uint8)
    qtext = ((quals.astype(np.uint16) + 33) & 0xff).astype(np.uint8).tobytes()
    auxs = np.asarray(fields.aux, np.uint8).tobytes()
    cig = np.asarray(fields.cigar, np.uint32)
    ref, pos, bmn, fnc, nref, npos, tlen = (np.asarray(columns[k]).tolist() for k in (
        "ref_id", "pos", "bin_mq_nl", "flag_nc", "next_ref_id", "next_pos", "tlen"))
    if len(ref) != n:
        raise ValueError(f"{len(ref)} fixed-field rows for {n} records")

    def contig(i):
        return contig_names[i] if 0 <= i < len(contig_names) else "*"

    out = []
    for k in range(n):
        s0, s1 = so[k], so[k + 1]
        rnext = "*" if nref[k] < 0 else "=" if nref[k] == ref[k] else contig(nref[k])
        qual = "*" if s1 == s0 or quals[s0] == 0xff else qtext[s0:s1].decode("latin-1")
        cols = [names[no[k]:no[k + 1]].decode("latin-1"), str(fnc[k] >> 16), contig(ref[k]), str(pos[k] + 1),
                str((bmn[k] >> 8) & 0xff), cigar_text(cig[co[k]:co[k + 1]]), rnext, str(npos[k] + 1), str(tlen[k]),
                seqs[s0:s1].decode("latin-1") if s1 > s0 else "*", qual]
        cols += tag_texts(auxs[ao[k]:ao[k + 1]])
        out.append("\t".join(cols))
    return out


def header_with_sort_order(header_bytes: bytes, order: str = "coordinate") -> bytes:
    """A complete BAM header (magic, l_text, text, n_ref, the references) with `SO:<order>` on its `@HD` line (SAM spec
    §1.3), as htsjdk's SAMFileHeader.setSortOrder and `samtools sort` leave it: the `SO:` field of an `@HD` first line
    is replaced, or `\\tSO:<order>` appended to it; a text without `@HD` gets `@HD\\tVN:1.6\\tSO:<order>\\n` in front.
    Trailing NUL padding of the text is dropped, l_text follows, and the reference list is kept byte for byte.  Host
    only."""
    h = bytes(header_bytes)
    if len(h) < 12 or h[:4] != b"BAM\x01":
        raise ValueError("not a BAM header: no magic")
    (l_text,) = struct.unpack_from("<i", h, 4)
    if l_text < 0 or 8 + l_text + 4 > len(h):
        raise ValueError("not a BAM header: l_text runs past its end")
    text, refs = h[8:8 + l_text].rstrip(b"\0"), h[8 + l_text:]
    so = b"SO:" + order.encode("ascii")
    if text.startswith(b"@HD\t") or text.split(b"\n", 1)[0] == b"@HD":
        line, nl, rest = text.partition(b"\n")
        fields = line.split(b"\t")
        if any(f.startswith(b"SO:") for f in fields[1:]):
            fields = [fields[0]] + [so if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            fields.append(so)
        text = b"\t".join(fields) + nl + rest
    else:
        text = b"@HD\tVN:1.6\t" + so + b"\n" + text
    return h[:4] + struct.pack("<i", len(text)) + text + refs
