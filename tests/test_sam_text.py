"""SAM text of decoded records (sbam.sam) against the reference's own SAM files, without a GPU.

tests/golden/sam/2.sam.gz and 5k.sam.gz are the reference's test_bams 2.sam and 5k.sam (gzip -9 -n): the SAM text of
2.bam and 5k.bam, which LoadSAMTest requires loadSam to read into the same records as loadBam.  A reference decoder
written here (plain struct and numpy over the oracle's inflated stream, walking block_size) produces the arrays
`BamFile.load_record_fields` returns; `sam.sam_lines` over them must equal the goldens' record lines verbatim.  That pins
the formatter and the goldens, and gives tests/test_record_fields.py its expected arrays (ref_fields / ref_columns).
Hand-made arrays cover what the fixtures lack: every `*` case and every tag type."""
import gzip
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, fixture_bytes

BASES = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
DATA_COLUMNS = ("name", "cigar", "seq", "qual", "aux")
OFFSET_COLUMNS = ("name_off", "cigar_off", "seq_off", "aux_off")


def record_chain(u: np.ndarray, x0: int, L: int):
    """Record offsets from x0 walking block_size (RecordStream.scala:27-41)."""
    b, xs, x = u[:L].tobytes(), [], x0
    while x + 4 <= L:
        xs.append(x)
        x += 4 + struct.unpack_from("<i", b, x)[0]
    return xs


def ref_fields(u: np.ndarray, offs) -> SimpleNamespace:
    """The CSR columns of the records at `offs` (SAM spec §4.2), as load_record_fields lays them out."""
    b = u.tobytes()
    parts = {k: [] for k in DATA_COLUMNS}
    for x in offs:
        bs, = struct.unpack_from("<i", b, x)
        lrn = b[x + 12]
        nc, = struct.unpack_from("<H", b, x + 16)
        ls, = struct.unpack_from("<i", b, x + 20)
        p = x + 36
        parts["name"].append(np.frombuffer(b, np.uint8, max(lrn - 1, 0), p))
        p += lrn
        parts["cigar"].append(np.frombuffer(b[p:p + 4 * nc], "<u4"))
        p += 4 * nc
        packed = np.frombuffer(b, np.uint8, (ls + 1) // 2, p)
        nib = np.empty(2 * packed.size, np.uint8)
        nib[0::2], nib[1::2] = packed >> 4, packed & 15
        parts["seq"].append(BASES[nib[:ls]])
        p += (ls + 1) // 2
        parts["qual"].append(np.frombuffer(b, np.uint8, ls, p))
        p += ls
        assert p <= x + 4 + bs, f"record at {x} overruns its block_size"
        parts["aux"].append(np.frombuffer(b, np.uint8, x + 4 + bs - p, p))
    out = SimpleNamespace(i0=0, n=len(offs))
    for k, dt in (("name", np.uint8), ("cigar", np.uint32), ("seq", np.uint8), ("qual", np.uint8), ("aux", np.uint8)):
        setattr(out, k, np.concatenate(parts[k]).astype(dt) if parts[k] else np.zeros(0, dt))
        if k != "qual":
            off = np.zeros(len(offs) + 1, np.int64)
            off[1:] = np.cumsum([a.size for a in parts[k]])
            setattr(out, k + "_off", off)
    return out


def ref_columns(u: np.ndarray, offs) -> dict:
    """The fixed-field columns sam_lines reads, as load_records lays them out."""
    b = u.tobytes()
    rows = [struct.unpack_from("<iiIIiiii", b, x + 4) for x in offs]
    names = ("ref_id", "pos", "bin_mq_nl", "flag_nc", "l_seq", "next_ref_id", "next_pos", "tlen")
    dts = (np.int32, np.int32, np.uint32, np.uint32, np.int32, np.int32, np.int32, np.int32)
    return {k: np.array([r[i] for r in rows], dt) for i, (k, dt) in enumerate(zip(names, dts))}


def slice_fields(f, i0: int, n: int) -> SimpleNamespace:
    """Records [i0, i0 + n) of a set of CSR columns, offsets rebased to 0."""
    out = SimpleNamespace(i0=i0, n=n)
    for k in DATA_COLUMNS:
        off = getattr(f, "seq_off" if k == "qual" else k + "_off")
        setattr(out, k, getattr(f, k)[off[i0]:off[i0 + n]])
        if k != "qual":
            setattr(out, k + "_off", off[i0:i0 + n + 1] - off[i0])
    return out


def stream_header(u: np.ndarray):
    """(header text, contig names, offset of the first record) of an inflated BAM stream."""
    b = u.tobytes()
    assert b[:4] == b"BAM\x01"
    lt, = struct.unpack_from("<i", b, 4)
    text, p = b[8:8 + lt], 8 + lt
    n, = struct.unpack_from("<i", b, p)
    p += 4
    names = []
    for _ in range(n):
        ln, = struct.unpack_from("<i", b, p)
        names.append(b[p + 4:p + 4 + ln - 1].decode("latin-1"))
        p += 4 + ln + 4
    return text.rstrip(b"\0").decode("latin-1"), names, p


def golden_sam(name: str):
    """(header lines, record lines) of tests/golden/sam/<name>.sam.gz"""
    with gzip.open(os.path.join(GOLDEN, "sam", name + ".sam.gz"), "rt", encoding="latin-1", newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return [ln for ln in lines if ln.startswith("@")], [ln for ln in lines if not ln.startswith("@")]


_DECODED = {}


def decoded(name: str, oracle_files):
    """(oracle file, record offsets, ref_fields, ref_columns, contig names) of a fixture, computed once."""
    if name not in _DECODED:
        o = oracle_files(name)
        _, names, first = stream_header(o.u)
        assert first == int(o.header_end)
        offs = record_chain(o.u, first, o.L)
        _DECODED[name] = (o, offs, ref_fields(o.u, offs), ref_columns(o.u, offs), names)
    return _DECODED[name]


@pytest.mark.parametrize("name,count", [("2", 2500), ("5k", 4910)])
def test_sam_lines_equal_the_reference_sam(name, count, oracle_files):
    from sbam import sam
    o, offs, fields, cols, names = decoded(name + ".bam", oracle_files)
    hdr, want = golden_sam(name)
    assert len(want) == count == len(offs)
    got = sam.sam_lines(cols, fields, names)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, f"{len(bad)} lines differ, first {bad[0]}:\n{got[bad[0]]}\n{want[bad[0]]}"
    assert len(got) == len(want)


@pytest.mark.parametrize("name", ["2", "5k"])
def test_header_text_equals_the_reference_sam(name, oracle_files):
    """The BAM's stored header text is the goldens' @ lines (what `view -h` prints first)."""
    o = oracle_files(name + ".bam")
    text, _, _ = stream_header(o.u)
    hdr, _ = golden_sam(name)
    assert text.rstrip("\n").split("\n") == hdr


def test_slice_fields_rebases_offsets(oracle_files):
    o, offs, fields, cols, names = decoded("2.bam", oracle_files)
    part = slice_fields(fields, 100, 7)
    again = ref_fields(o.u, offs[100:107])
    for k in DATA_COLUMNS + OFFSET_COLUMNS:
        assert np.array_equal(getattr(part, k), getattr(again, k)), k


def _one(name=b"r", ops=(), seq=b"", qual=b"", aux=b"", ref_id=0, pos=99, mapq=30, flag=0, next_ref_id=-1,
         next_pos=-1, tlen=0):
    """Hand-made arrays of one record: (columns, fields)."""
    f = SimpleNamespace(i0=0, n=1, name=np.frombuffer(name, np.uint8), name_off=np.array([0, len(name)]),
                        cigar=np.array(ops, np.uint32), cigar_off=np.array([0, len(ops)]),
                        seq=np.frombuffer(seq, np.uint8), qual=np.frombuffer(qual, np.uint8),
                        seq_off=np.array([0, len(seq)]), aux=np.frombuffer(aux, np.uint8),
                        aux_off=np.array([0, len(aux)]))
    c = {"ref_id": np.array([ref_id], np.int32), "pos": np.array([pos], np.int32),
         "bin_mq_nl": np.array([(4680 << 16) | (mapq << 8) | (len(name) + 1)], np.uint32),
         "flag_nc": np.array([(flag << 16) | len(ops)], np.uint32), "l_seq": np.array([len(seq)], np.int32),
         "next_ref_id": np.array([next_ref_id], np.int32), "next_pos": np.array([next_pos], np.int32),
         "tlen": np.array([tlen], np.int32)}
    return c, f


CONTIGS = ["chr1", "chr2"]


def _line(**kw):
    from sbam import sam
    c, f = _one(**kw)
    (ln,) = sam.sam_lines(c, f, CONTIGS)
    return ln.split("\t")


def test_star_cases():
    # unmapped, no CIGAR, no bases: RNAME, CIGAR, RNEXT, SEQ and QUAL are all `*`, POS and PNEXT 0
    assert _line(ref_id=-1, pos=-1, mapq=0, flag=4) == ["r", "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]
    # bases without qualities: a run of 0xFF prints `*`
    assert _line(ops=[(3 << 4) | 0], seq=b"ACG", qual=b"\xff\xff\xff")[9:11] == ["ACG", "*"]
    # qualities are byte + 33
    assert _line(ops=[(3 << 4) | 0], seq=b"ACG", qual=bytes([0, 30, 60]))[9:11] == ["ACG", "!?]"]
    # RNEXT: `=` for the same contig, the name for another; PNEXT and TLEN as stored (+1 / signed)
    assert _line(next_ref_id=0, next_pos=199, tlen=-120)[6:9] == ["=", "200", "-120"]
    assert _line(next_ref_id=1, next_pos=4)[6:8] == ["chr2", "5"]
    assert _line(ref_id=1, pos=0)[2:4] == ["chr2", "1"]


def test_cigar_letters():
    ops = [(k + 1) << 4 | k for k in range(9)]
    assert _line(ops=ops)[5] == "1M2I3D4N5S6H7P8=9X"
    assert _line(ops=[(268435455 << 4) | 0])[5] == "268435455M"


def test_every_tag_type():
    aux = (b"XAAQ" + b"Xcc" + struct.pack("<b", -5) + b"XCC" + struct.pack("<B", 250) +
           b"Xss" + struct.pack("<h", -30000) + b"XSS" + struct.pack("<H", 60000) +
           b"Xii" + struct.pack("<i", -2000000000) + b"XII" + struct.pack("<I", 4000000000) +
           b"Xff" + struct.pack("<f", 1.5) + b"XZZhello world\0" + b"XHH1AE301\0" + b"XEZ\0" +
           b"BcBc" + struct.pack("<i2b", 2, -1, 2) + b"BCBC" + struct.pack("<i2B", 2, 1, 255) +
           b"BsBs" + struct.pack("<i2h", 2, -300, 300) + b"BSBS" + struct.pack("<i1H", 1, 65535) +
           b"BiBi" + struct.pack("<i1i", 1, -70000) + b"BIBI" + struct.pack("<i1I", 1, 3000000000) +
           b"BfBf" + struct.pack("<i2f", 2, 0.25, -2.5) + b"B0Bc" + struct.pack("<i", 0))
    assert _line(aux=aux)[11:] == [
        "XA:A:Q", "Xc:i:-5", "XC:i:250", "Xs:i:-30000", "XS:i:60000", "Xi:i:-2000000000", "XI:i:4000000000",
        "Xf:f:1.5", "XZ:Z:hello world", "XH:H:1AE301", "XE:Z:", "Bc:B:c,-1,2", "BC:B:C,1,255", "Bs:B:s,-300,300",
        "BS:B:S,65535", "Bi:B:i,-70000", "BI:B:I,3000000000", "Bf:B:f,0.25,-2.5", "B0:B:c"]


def test_two_records_keep_their_own_slices():
    from sbam import sam
    f = SimpleNamespace(i0=0, n=2, name=np.frombuffer(b"ab", np.uint8), name_off=np.array([0, 0, 2]),
                        cigar=np.array([(2 << 4) | 0], np.uint32), cigar_off=np.array([0, 0, 1]),
                        seq=np.frombuffer(b"GT", np.uint8), qual=np.array([1, 2], np.uint8),
                        seq_off=np.array([0, 0, 2]), aux=np.frombuffer(b"NMC\x03", np.uint8),
                        aux_off=np.array([0, 0, 4]))
    z = np.zeros(2, np.int32)
    c = {"ref_id": z - 1, "pos": z - 1, "bin_mq_nl": np.array([1, 3], np.uint32),
         "flag_nc": np.array([4 << 16, (4 << 16) | 1], np.uint32), "l_seq": np.array([0, 2], np.int32),
         "next_ref_id": z - 1, "next_pos": z - 1, "tlen": z}
    assert sam.sam_lines(c, f, CONTIGS) == ["\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*", "ab\t4\t*\t0\t0\t2M\t*\t0\t0\tGT\t\"#\tNM:i:3"]
