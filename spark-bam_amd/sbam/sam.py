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


def tag_texts(aux: bytes) -> List[str]:
    """`TG:t:value` for each tag of one record's raw tag bytes (SAM spec §4.2.4), in file order."""
    out, p, n = [], 0, len(aux)
    while p < n:
        if p + 3 > n:
            raise ValueError(f"truncated tag at byte {p} of {n}")
        tag, t = aux[p:p + 2].decode("latin-1"), chr(aux[p + 2])
        p += 3
        if t in _INT_TAGS:
            fmt, w = _INT_TAGS[t]
            out.append(f"{tag}:i:{struct.unpack_from(fmt, aux, p)[0]}")
            p += w
        elif t == "A":
            out.append(f"{tag}:A:{chr(aux[p])}")
            p += 1
        elif t == "f":
            out.append(f"{tag}:f:{_float_text(struct.unpack_from('<f', aux, p)[0])}")
            p += 4
        elif t in "ZH":
            e = aux.index(b"\0", p)
            out.append(f"{tag}:{t}:{aux[p:e].decode('latin-1')}")
            p = e + 1
        elif t == "B":
            st = chr(aux[p])
            cnt = struct.unpack_from("<i", aux, p + 1)[0]
            p += 5
            if st == "f":
                vals = [_float_text(v) for v in struct.unpack_from(f"<{cnt}f", aux, p)]
                w = 4
            elif st in _INT_TAGS:
                fmt, w = _INT_TAGS[st]
                vals = [str(v) for v in struct.unpack_from(f"<{cnt}{fmt[1]}", aux, p)]
            else:
                raise ValueError(f"unknown B subtype {st!r} in tag {tag}")
            out.append(f"{tag}:B:{st}" + "".join("," + v for v in vals))
            p += cnt * w
        else:
            raise ValueError(f"unknown tag type {t!r} in tag {tag}")
    return out


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
