"""sbam — host-side mirror of spark-bam's split/check/decode API over the MI355X C-ABI (libsbam.so).

Names, argument meaning and error behaviour follow the reference:

* ``Pos`` / ``Split``                         bgzf/.../Pos.scala:12-41, check/.../bam/spark/Split.scala:9-13
* ``BamFile.find_block_start``                bgzf/.../block/FindBlockStart.scala:8-36
* ``BamFile.find_record_start``               check/.../bam/spark/FindRecordStart.scala:11-63
* ``BamFile.eager_checker`` / ``full_checker``  check/.../check/{eager,full}/Checker.scala (Checker[Call].apply)
* ``BamFile.load_splits_and_reads`` etc.      load/.../spark/load/CanLoadBam.scala:173-382
* exceptions ``HeaderParseException``, ``HeaderSearchFailedException``, ``NoReadFoundException``,
  ``InflateException`` carry the reference's message text.

Everything computes on the GPU through ``libsbam.so``; there is no CPU fallback: importing this module
without the built library raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBAM_LIB", os.path.join(_HERE, "..", "build", "libsbam.so"))

SBAM_OK = 0
ERR_HEADER_PARSE, ERR_HEADER_SEARCH, ERR_INFLATE, ERR_NO_READ_FOUND, ERR_NOT_BAM, ERR_ARG, ERR_HIP, ERR_STATE, \
    ERR_HALO = range(1, 10)
ERR_RECORD = 10
ERR_CRC = 11
SBAM_WRITE_DYNAMIC = 0x100  # ORed into the writer's level 1: per block the smallest of stored, fixed and dynamic Huffman

FLAG_NAMES = [  # check/src/main/scala/org/hammerlab/bam/check/full/error/Flags.scala:201-223
    "tooFewFixedBlockBytes", "negativeReadIdx", "tooLargeReadIdx", "negativeReadPos", "tooLargeReadPos",
    "negativeNextReadIdx", "tooLargeNextReadIdx", "negativeNextReadPos", "tooLargeNextReadPos",
    "tooFewBytesForReadName", "nonNullTerminatedReadName", "nonASCIIReadName", "noReadName", "emptyReadName",
    "tooFewBytesForCigarOps", "invalidCigarOp", "emptyMappedCigar", "emptyMappedSeq",
    "tooFewRemainingBytesImplied",
]
WORD_SUCCESS = 0x80000000
WORD_HALO = 0x00800000

# Defaults (bgzf/.../block/package.scala:20-21, check/.../check/package.scala:17-18,28-29)
BGZF_BLOCKS_TO_CHECK = 5
READS_TO_CHECK = 10
MAX_READ_SIZE = 10_000_000
# Hadoop's local FileSystem block size (fs.local.block.size default): what a split size falls back to when
# -m/--max-split-size is unset (check/.../args/SplitSize.scala:10-17: "default to underlying FileSystem's value").
LOCAL_FS_BLOCK_SIZE = 32 << 20


def effective_split_size(max_split_size: Optional[int] = None, fs_block_size: int = LOCAL_FS_BLOCK_SIZE) -> int:
    """The split size Hadoop's FileInputFormat uses: computeSplitSize(blockSize, minSize=1, maxSize) =
    max(1, min(maxSize, blockSize)), with maxSize = the FS block size when -m is unset (SplitSize.scala:10-17).
    The FS-block cap comes from Hadoop, outside the reference tree: parity unpinned (no golden splits a file into
    pieces larger than 32 MiB)."""
    m = fs_block_size if max_split_size is None else int(max_split_size)
    return max(1, min(m, fs_block_size))


class SbamError(Exception):
    code = 0


class HeaderParseException(SbamError):
    code = ERR_HEADER_PARSE


class HeaderSearchFailedException(SbamError):
    code = ERR_HEADER_SEARCH


class InflateException(IOError, SbamError):
    code = ERR_INFLATE


class NoReadFoundException(SbamError):
    code = ERR_NO_READ_FOUND


class HaloException(SbamError):
    code = ERR_HALO


class RecordFieldsException(SbamError):
    """A record whose variable-length fields overrun its block_size (sbam_load_record_fields) or whose tag list is
    malformed (sbam_load_record_tags); `position` is the record's stream offset."""
    code = ERR_RECORD
    position = None


class CrcException(IOError, SbamError):
    """A BGZF block whose inflated bytes do not have the CRC32 its footer stores (verify_crc): `position` is the
    block's file offset, `expected` the stored value, `actual` the computed one."""
    code = ERR_CRC
    position = expected = actual = None


_EXC = {c.code: c for c in (HeaderParseException, HeaderSearchFailedException, InflateException,
                            NoReadFoundException, HaloException, RecordFieldsException, CrcException)}


class _Pos(ctypes.Structure):
    _fields_ = [("block_pos", ctypes.c_int64), ("offset", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _Split(ctypes.Structure):
    _fields_ = [("start", _Pos), ("end", _Pos)]


class _Error(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("idx", ctypes.c_int32), ("actual", ctypes.c_int64),
                ("expected", ctypes.c_int64), ("position", ctypes.c_int64), ("message", ctypes.c_char * 512)]


class _Counts(ctypes.Structure):
    _fields_ = [("totals", ctypes.c_int64 * 19), ("counts", ctypes.c_int64 * (21 * 19)), ("positions", ctypes.c_int64 * 21),
                ("reads_before_error", ctypes.c_int64 * (21 * 128)), ("pair_hist", ctypes.c_int64 * (19 * 19)),
                ("n_positions", ctypes.c_int64), ("n_success", ctypes.c_int64),
                ("n_too_few_fixed", ctypes.c_int64), ("n_halo", ctypes.c_int64)]


class _SplitArgs(ctypes.Structure):
    _fields_ = [("split_size", ctypes.c_int64), ("bgzf_blocks_to_check", ctypes.c_int32),
                ("reads_to_check", ctypes.c_int32), ("max_read_size", ctypes.c_int32),
                ("use_success_bitmap", ctypes.c_int32)]


class _RecordColumns(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("offset", "block_pos", "block_off", "block_size", "ref_id", "pos",
                                               "bin_mq_nl", "flag_nc", "l_seq", "next_ref_id", "next_pos", "tlen")]


RECORD_COLUMNS = {"offset": np.int64, "block_pos": np.int64, "block_off": np.int32, "block_size": np.int32,
                  "ref_id": np.int32, "pos": np.int32, "bin_mq_nl": np.uint32, "flag_nc": np.uint32,
                  "l_seq": np.int32, "next_ref_id": np.int32, "next_pos": np.int32, "tlen": np.int32}


class _RecordFields(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("name_off", "name", "cigar_off", "cigar", "seq_off", "seq", "qual",
                                               "aux_off", "aux")]


class _RecordFieldTotals(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("name_bytes", "cigar_ops", "seq_bases", "aux_bytes")]


MAX_TAGS = 32  # SBAM_MAX_TAGS


class _TagQuery(ctypes.Structure):
    _fields_ = [("tag", ctypes.c_char * 2), ("want_bytes", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class _RecordTags(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("type", "sub", "rel", "value")] + \
        [("bytes_off", ctypes.c_void_p * MAX_TAGS), ("bytes", ctypes.c_void_p * MAX_TAGS)]


class _RecordTagTotals(ctypes.Structure):
    _fields_ = [("present", ctypes.c_int64 * MAX_TAGS), ("bytes", ctypes.c_int64 * MAX_TAGS)]


class _IndexTotals(ctypes.Structure):
    _fields_ = [("n_ref", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
        [(n, ctypes.c_int64) for n in ("n_runs", "n_intv_total", "n_no_coor", "n_unsorted", "n_records")]


class _CrcTotals(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("n_blocks", "n_bad", "first_bad", "bytes")]


class _WriteArgs(ctypes.Structure):
    _fields_ = [("range_lo", ctypes.c_void_p), ("range_hi", ctypes.c_void_p), ("n_ranges", ctypes.c_int64),
                ("keep_device", ctypes.c_void_p), ("level", ctypes.c_int32), ("block_bytes", ctypes.c_int32),
                ("with_header", ctypes.c_int32), ("with_eof", ctypes.c_int32)]


class _WriteTotals(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("n_records", "header_bytes", "ubytes", "n_blocks", "n_stored_blocks",
                                              "comp_bytes")]


class _SortTotals(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_int64), ("n_out_of_order", ctypes.c_int64), ("passes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class _WriteOrder(ctypes.Structure):
    _fields_ = [("order_device", ctypes.c_void_p), ("header", ctypes.c_void_p), ("header_bytes", ctypes.c_int64)]


WRITE_BLOCK_BYTES = 65498  # htsjdk's uncompressed bytes per BGZF block


# sbam_load_record_fields' mask bits, the data column's dtype, its offsets column and its total
FIELD_BITS = {"name": 1, "cigar": 2, "seq": 4, "qual": 8, "aux": 16}
_FIELD_LAYOUT = {"name": (np.uint8, "name_off", "name_bytes"), "cigar": (np.uint32, "cigar_off", "cigar_ops"),
                 "seq": (np.uint8, "seq_off", "seq_bases"), "qual": (np.uint8, "seq_off", "seq_bases"),
                 "aux": (np.uint8, "aux_off", "aux_bytes")}


@dataclass
class RecordFields:
    """CSR columns of records [i0, i0 + n) (sbam_load_record_fields): `*_off` are int64[n + 1]; a data column that
    was not selected (or everything, with host=False) is None."""
    i0: int
    n: int
    totals: dict
    name_off: Optional[np.ndarray] = None
    name: Optional[np.ndarray] = None
    cigar_off: Optional[np.ndarray] = None
    cigar: Optional[np.ndarray] = None
    seq_off: Optional[np.ndarray] = None
    seq: Optional[np.ndarray] = None
    qual: Optional[np.ndarray] = None
    aux_off: Optional[np.ndarray] = None
    aux: Optional[np.ndarray] = None


@dataclass
class RecordTags:
    """Typed tags of records [i0, i0 + n) (sbam_load_record_tags): `type`, `sub`, `rel`, `value` are [len(tags), n]
    arrays (None with host=False); `bytes_off[tag]` (int64[n + 1]) and `bytes[tag]` (uint8) exist for the tags of
    `bytes_for`; `totals[tag]` = {"present", "bytes"}."""
    i0: int
    n: int
    tags: tuple
    totals: dict
    type: Optional[np.ndarray] = None
    sub: Optional[np.ndarray] = None
    rel: Optional[np.ndarray] = None
    value: Optional[np.ndarray] = None
    bytes_off: Optional[dict] = None
    bytes: Optional[dict] = None

    def floats(self, tag: str) -> np.ndarray:
        """The float32 view of the low 32 bits of a tag's values (meaningful where its type is `f`)."""
        return (self.value[self.tags.index(tag)] & 0xffffffff).astype(np.uint32).view(np.float32)

    def texts(self, tag: str) -> list:
        """A tag's value bytes per record (`bytes`), None where the record has no such tag; needs `bytes_for`."""
        j, off, data = self.tags.index(tag), self.bytes_off[tag].tolist(), self.bytes[tag].tobytes()
        return [data[off[k]:off[k + 1]] if t else None for k, t in enumerate(self.type[j].tolist())]


_vp, _i64, _i32, _P = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER
_SIGNATURES = {  # (restype, argtypes) of every symbol include/sbam.h declares
    "sbam_open": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _i64, _i64, _P(_vp)]),
    "sbam_close": (None, [_vp]),
    "sbam_last_error": (_P(_Error), [_vp]),
    "sbam_set_path": (ctypes.c_int, [_vp, ctypes.c_char_p]),
    "sbam_reset": (ctypes.c_int, [_vp]),
    "sbam_version": (ctypes.c_char_p, []),
    "sbam_find_block_starts": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "sbam_scan_blocks": (ctypes.c_int, [_vp, _P(_i64)]),
    "sbam_scan_path": (ctypes.c_int, [_vp, _P(_i32), _P(_i32), _P(_i64)]),
    "sbam_follow_segment_bytes": (ctypes.c_int, []),
    "sbam_get_blocks": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64]),
    "sbam_inflate": (ctypes.c_int, [_vp, _P(_i64)]),
    "sbam_inflate_fallbacks": (ctypes.c_int, [_vp, _P(_i64)]),
    "sbam_check_crc": (ctypes.c_int, [_vp, _i64, _i64, _P(_CrcTotals)]),
    "sbam_get_block_crcs": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "sbam_set_verify_crc": (ctypes.c_int, [_vp, _i32]),
    "sbam_read_uncompressed": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "sbam_pos_to_offset": (ctypes.c_int, [_vp, _Pos, _P(_i64)]),
    "sbam_offset_to_pos": (ctypes.c_int, [_vp, _i64, _P(_Pos)]),
    "sbam_header": (ctypes.c_int, [_vp, _P(_i32), _vp, _i32, _P(_Pos)]),
    "sbam_set_contig_lengths": (ctypes.c_int, [_vp, _i32, _vp]),
    "sbam_check_eager": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp]),
    "sbam_check_full_words": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp]),
    "sbam_check_full_counts": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _P(_Counts), _vp]),
    "sbam_find_record_start": (ctypes.c_int, [_vp, _i64, _i32, _i32, _P(_i32), _P(_Pos), _P(_i32)]),
    "sbam_file_splits": (ctypes.c_int, [_i64, _i64, _vp, _vp, _i64, _P(_i64)]),
    "sbam_split_records": (ctypes.c_int, [_vp, _P(_SplitArgs), _i64, _i64, _vp, _vp, _vp]),
    "sbam_compute_splits": (ctypes.c_int, [_vp, _P(_SplitArgs), _vp, _i64, _P(_i64)]),
    "sbam_record_offsets": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _P(_i64)]),
    "sbam_load": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64]),
    "sbam_reserve": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64]),
    "sbam_record_spans": (ctypes.c_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "sbam_load_records": (ctypes.c_int, [_vp, _P(_SplitArgs), _i64, _i64, _vp, _P(_i64)]),
    "sbam_records_path": (ctypes.c_int, [_vp, _P(_i32), _P(_i32), _P(_i64), _P(_i64)]),
    "sbam_get_record_columns": (ctypes.c_int, [_vp, _i64, _i64, _P(_RecordColumns)]),
    "sbam_record_columns_device": (ctypes.c_int, [_vp, _P(_RecordColumns), _P(_i64)]),
    "sbam_load_record_fields": (ctypes.c_int, [_vp, _i64, _i64, ctypes.c_uint32, _P(_RecordFieldTotals)]),
    "sbam_get_record_fields": (ctypes.c_int, [_vp, _P(_RecordFields)]),
    "sbam_record_fields_device": (ctypes.c_int, [_vp, _P(_RecordFields), _P(_i64), _P(_i64)]),
    "sbam_load_record_tags": (ctypes.c_int, [_vp, _i64, _i64, _P(_TagQuery), _i32, _P(_RecordTagTotals)]),
    "sbam_get_record_tags": (ctypes.c_int, [_vp, _P(_RecordTags)]),
    "sbam_record_tags_device": (ctypes.c_int, [_vp, _P(_RecordTags), _P(_i64), _P(_i64), _P(_i32)]),
    "sbam_tag_long_aux_bytes": (ctypes.c_int, []),
    "sbam_build_index": (ctypes.c_int, [_vp, _P(_IndexTotals)]),
    "sbam_get_index_runs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "sbam_get_index_refs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sbam_bai_assemble": (ctypes.c_int, [_i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64,
                                         _P(_i64)]),
    "sbam_write_bai": (ctypes.c_int, [_vp, _vp, _i64, _P(_i64)]),
    "sbam_index_long_cigar_ops": (ctypes.c_int, []),
    "sbam_write_bam": (ctypes.c_int, [_vp, _P(_WriteArgs), _P(_WriteTotals)]),
    "sbam_write_bam_ordered": (ctypes.c_int, [_vp, _P(_WriteArgs), _P(_WriteOrder), _P(_WriteTotals)]),
    "sbam_sort_records": (ctypes.c_int, [_vp, _P(_SortTotals)]),
    "sbam_get_sort_order": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "sbam_sort_order_device": (ctypes.c_int, [_vp, _P(_vp), _P(_i64)]),
    "sbam_sort_tile_keys": (ctypes.c_int, []),
    "sbam_test_sort_keys": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _vp, _P(_i32)]),
    "sbam_get_written": (ctypes.c_int, [_vp, _vp, _i64]),
    "sbam_written_device": (ctypes.c_int, [_vp, _P(_vp), _P(_i64)]),
    "sbam_get_written_blocks": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "sbam_get_written_records": (ctypes.c_int, [_vp, _vp, _vp]),
    "sbam_test_deflate": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _P(_i64), _P(_i64)]),
    "sbam_test_exclusive_scan": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _i32, _vp]),
    "sbam_test_scan_sums_int": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _vp]),
    "sbam_test_chain_proof": (ctypes.c_int, [ctypes.c_int, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp,
                                             _i64, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "sbam_last_kernel_ms": (ctypes.c_double, [_vp, ctypes.c_char_p]),
}
EXPORTS = list(_SIGNATURES)

_lib = None


def source_digest() -> str:
    """Digest of the kernel and C-ABI sources libsbam.so is built from: ties committed profiles (PMC traffic) to
    the kernel build they were measured on."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "..", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(csrc, name), "rb") as fh:
                h.update(name.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def load_library(path: str = LIB_PATH):
    """Load libsbam.so; raises (no fallback) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"libsbam.so not built at {path}: run `make -C spark-bam_amd` (no CPU fallback exists)")
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


@dataclass(frozen=True, order=True)
class Pos:
    """Virtual position (bgzf/src/main/scala/org/hammerlab/bgzf/Pos.scala:12-41)."""
    block_pos: int
    offset: int

    def __str__(self):
        return f"{self.block_pos}:{self.offset}"

    def to_htsjdk(self) -> int:
        return (self.block_pos << 16) | self.offset

    @staticmethod
    def from_htsjdk(v: int) -> "Pos":
        return Pos(v >> 16, v & 0xFFFF)

    def minus(self, other: "Pos", ratio: float = 3.0) -> float:
        """Pos.- with EstimatedCompressionRatio (Pos.scala:17-22)."""
        return float(max(0, self.block_pos - other.block_pos + int((self.offset - other.offset) / ratio)))


@dataclass(frozen=True)
class Split:
    """check/src/main/scala/org/hammerlab/bam/spark/Split.scala:9-13."""
    start: Pos
    end: Pos

    def length(self, ratio: float = 3.0) -> float:
        return self.end.minus(self.start, ratio)

    def __str__(self):
        return f"{self.start}-{self.end}"


@dataclass
class IndexRefs:
    """Linear index and per-reference metadata of a built index (sbam_get_index_refs): reference r's 16 kb windows
    are ioffset[intv_off[r]:intv_off[r + 1]]; the totals are sbam_build_index's."""
    intv_off: np.ndarray
    ioffset: np.ndarray
    off_beg: np.ndarray
    off_end: np.ndarray
    n_mapped: np.ndarray
    n_unmapped: np.ndarray
    n_no_coor: int
    n_unsorted: int
    n_records: int


def bai_assemble(n_ref: int, runs, intv_off, ioffset, off_beg, off_end, n_mapped, n_unmapped, n_no_coor: int) -> bytes:
    """sbam_bai_assemble (host only, no GPU): runs = (ref int32, bin uint32, beg uint64, end uint64) in file order,
    the linear index (UINT64_MAX = untouched window) and the per-reference metadata -> .bai bytes."""
    L = load_library()
    ref, bn, beg, end = (np.ascontiguousarray(a, t) for a, t in zip(runs, (np.int32, np.uint32, np.uint64, np.uint64)))
    io, ob, oe = (np.ascontiguousarray(a, np.uint64) for a in (ioffset, off_beg, off_end))
    iv, nm, nu = (np.ascontiguousarray(a, np.int64) for a in (intv_off, n_mapped, n_unmapped))
    args = (int(n_ref), ref.size, _ptr(ref), _ptr(bn), _ptr(beg), _ptr(end), _ptr(iv), _ptr(io), _ptr(ob), _ptr(oe),
            _ptr(nm), _ptr(nu), int(n_no_coor))
    n = ctypes.c_int64(-1)
    rc = L.sbam_bai_assemble(*args, None, 0, ctypes.byref(n))
    if n.value < 0:
        raise SbamError(f"sbam_bai_assemble: invalid arguments ({rc})")
    out = np.zeros(n.value, np.uint8)
    rc = L.sbam_bai_assemble(*args, _ptr(out), out.size, ctypes.byref(n))
    if rc != SBAM_OK:
        raise SbamError(f"sbam_bai_assemble: {rc}")
    return out.tobytes()


def _pos(p: _Pos) -> Pos:
    return Pos(int(p.block_pos), int(p.offset))


@dataclass
class Counts:
    """full-check reductions (check/.../full/error/Counts.scala; FullCheck.scala:141-191)."""
    totals: np.ndarray  # [19] per flag over every counted position ("Total error counts")
    by_key: np.ndarray  # [21, 19]: keys 1-2 always; every key when computed with by_key=True
    positions: np.ndarray  # [21]
    reads_before_error: np.ndarray  # [21, 128]
    pair_hist: np.ndarray  # [19, 19]
    n_positions: int
    n_success: int
    n_too_few_fixed: int

    # the packed int64 vector (what ranks all_reduce, and what tests/golden/bench_digests.json pins): fields in this order
    LAYOUT = (("totals", (19,)), ("by_key", (21, 19)), ("positions", (21,)), ("reads_before_error", (21, 128)),
              ("pair_hist", (19, 19)), ("n_success", ()), ("n_too_few_fixed", ()), ("n_positions", ()))

    def total_error_counts(self) -> dict:
        t = self.totals
        return {FLAG_NAMES[i]: int(t[i]) for i in range(19)}

    def pack(self) -> np.ndarray:
        return np.concatenate([np.asarray(getattr(self, name), np.int64).ravel() for name, _ in self.LAYOUT])

    @classmethod
    def unpack(cls, v: np.ndarray) -> "Counts":
        out, o = {}, 0
        for name, shape in cls.LAYOUT:
            n = int(np.prod(shape, dtype=np.int64))
            out[name] = v[o:o + n].reshape(shape) if shape else int(v[o])
            o += n
        return cls(**out)

    @classmethod
    def zero(cls) -> "Counts":
        return cls.unpack(np.zeros(N_COUNT_WORDS, np.int64))

    def __add__(self, other: "Counts") -> "Counts":
        return Counts(**{name: getattr(self, name) + getattr(other, name) for name, _ in self.LAYOUT})


N_COUNT_WORDS = sum(int(np.prod(shape, dtype=np.int64)) for _, shape in Counts.LAYOUT)


def n_hadoop_splits(file_size: int, split_size: int) -> int:
    """len(hadoop_splits(...)) without building the list (a 10 GB file has ~5000 splits)."""
    n = ctypes.c_int64(0)
    load_library().sbam_file_splits(file_size, split_size, None, None, 0, ctypes.byref(n))
    return int(n.value)


def hadoop_splits(file_size: int, split_size: int):
    """FileInputFormat split rule (through libsbam.sbam_file_splits)."""
    L = load_library()
    n = ctypes.c_int64(0)
    L.sbam_file_splits(file_size, split_size, None, None, 0, ctypes.byref(n))
    s = np.zeros(n.value, np.int64)
    e = np.zeros(n.value, np.int64)
    L.sbam_file_splits(file_size, split_size, _ptr(s), _ptr(e), n.value, ctypes.byref(n))
    return list(zip(s.tolist(), e.tolist()))


class BamFile:
    """One BAM file (or a shard of one) resident on one GPU — the per-task channel of the reference
    (load/.../spark/load/Channels.scala:15-26) with the hot path behind it."""

    def __init__(self, data, device: int = 0, base_offset: int = 0, file_size: Optional[int] = None,
                 path: str = "<bytes>", inflate: bool = True, contig_lengths: Optional[Sequence[int]] = None,
                 verify_crc: bool = False):
        self.L = load_library()
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        self._buf = np.ascontiguousarray(buf)
        self.path = path
        self.base_offset = base_offset
        self.file_size = int(file_size if file_size is not None else base_offset + self._buf.size)
        self.ctx = ctypes.c_void_p()
        rc = self.L.sbam_open(device, _ptr(self._buf), self._buf.size, base_offset, self.file_size,
                              ctypes.byref(self.ctx))
        self._check(rc)
        self._check(self.L.sbam_set_path(self.ctx, str(path).encode()))
        self._crc = None  # (b0, b1) of the last check_crc
        self.verify_crc = False
        if verify_crc:
            self.set_verify_crc(True)
        self.n_blocks = self._scan()
        self.uncompressed_size = None
        self.n_ref = None
        self.contig_lengths = None
        self.header_end = None
        self.n_loaded = 0  # records of the last load_records still on the device
        self._index = None  # totals of the last build_index
        self._written = None  # totals of the last write_bam
        self.device = device
        if inflate:
            self.inflate()
            if contig_lengths is not None:
                self.set_contig_lengths(contig_lengths)
            elif base_offset == 0:
                self.header()

    # ---- plumbing
    def _check(self, rc):
        if rc == SBAM_OK:
            return
        e = self.L.sbam_last_error(self.ctx).contents if self.ctx else None
        msg = e.message.decode() if e else f"sbam error {rc}"
        exc = _EXC.get(rc, SbamError)(msg)
        if rc == ERR_CRC and e:
            exc.position, exc.expected, exc.actual = int(e.position), int(e.expected), int(e.actual)
        if rc == ERR_RECORD and e:
            exc.position = int(e.position)
        raise exc

    def close(self):
        if self.ctx:
            self.L.sbam_close(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, data, base_offset: int = 0, file_size: Optional[int] = None):
        """sbam_load: make another byte range resident in this context (allocations kept, stages dropped).
        `data` (numpy uint8, possibly a view of pinned host memory) must stay alive while loading."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        self._buf = np.ascontiguousarray(buf)
        file_size = int(file_size if file_size is not None else base_offset + self._buf.size)
        # the context drops its contig lengths when the range may hold a different header (sbam_load)
        drop = base_offset == 0 or file_size != self.file_size
        self.base_offset = base_offset
        self.file_size = file_size
        self._check(self.L.sbam_load(self.ctx, _ptr(self._buf), self._buf.size, base_offset, self.file_size))
        if drop:
            self.n_ref = self.contig_lengths = self.header_end = None
        self.n_blocks = None
        self.uncompressed_size = None
        self.n_loaded = 0
        self._crc = None

    def reserve(self, comp_bytes: int, n_blocks: int, ubytes: int, n_records: int = 0):
        """sbam_reserve: size the device buffers for windows up to these sizes, so no later load reallocates.  A
        buffer that grows drops the context's stages (their device data is gone).  The context is then asked what
        survived (a query of a dropped stage is ERR_STATE), and exactly what this object had before is run again
        from the resident bytes: the block scan if it had one, inflate if it had a stream.  Checker results, splits
        and loaded records are not redone."""
        had_scan, had_stream = self.n_blocks is not None, self.uncompressed_size is not None
        self._check(self.L.sbam_reserve(self.ctx, int(comp_bytes), int(n_blocks), int(ubytes), int(n_records)))
        if had_scan and self.L.sbam_get_blocks(self.ctx, None, None, None, None, 0) == ERR_STATE:
            self.n_loaded = 0
            self.n_blocks = self._scan()
        if had_stream and self.L.sbam_read_uncompressed(self.ctx, 0, 0, None) == ERR_STATE:
            self.inflate()

    @property
    def loads_to_eof(self) -> bool:
        """Whether the resident bytes reach the end of the file (else a scan past them is a halo miss)."""
        return self.base_offset + self._buf.size >= self.file_size

    def reset(self):
        """Drop derived stages (keeps the resident compressed bytes and allocations)."""
        self._check(self.L.sbam_reset(self.ctx))
        self.n_blocks = None
        self.uncompressed_size = None
        self.n_loaded = 0
        self._crc = None

    def run(self, contig_lengths: Optional[Sequence[int]] = None):
        """Scan → inflate → header/contig lengths from the resident compressed bytes."""
        self.n_blocks = self._scan()
        self.inflate()
        if contig_lengths is not None:
            self.set_contig_lengths(contig_lengths)
        elif self.base_offset == 0:
            self.header()

    def kernel_ms(self, name: str) -> float:
        return float(self.L.sbam_last_kernel_ms(self.ctx, name.encode()))

    # ---- BGZF
    def _scan(self) -> int:
        n = ctypes.c_int64(0)
        self._check(self.L.sbam_scan_blocks(self.ctx, ctypes.byref(n)))
        return n.value

    def scan_path(self) -> dict:
        """What the last block scan did (sbam_scan_path): `followed` the headers' BSIZE hops to the table, `fell_back`
        to the byte scan after trying that; `segments` followed (0: not tried)."""
        a, b, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._check(self.L.sbam_scan_path(self.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return {"followed": bool(a.value), "fell_back": bool(b.value), "segments": int(n.value)}

    def blocks(self):
        """(start, compressedSize, uncompressedSize, uncompressedOffset) arrays (IndexBlocks.scala:40-44)."""
        n = self.n_blocks
        st, cs, us, uo = (np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64))
        self._check(self.L.sbam_get_blocks(self.ctx, _ptr(st), _ptr(cs), _ptr(us), _ptr(uo), n))
        return st, cs, us, uo

    def find_block_starts(self, starts: Sequence[int], bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK):
        q = np.asarray(starts, np.int64)
        out = np.zeros(q.size, np.int64)
        self._check(self.L.sbam_find_block_starts(self.ctx, _ptr(q), q.size, bgzf_blocks_to_check, _ptr(out)))
        return out

    def find_block_start(self, start: int, bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK) -> int:
        """FindBlockStart.apply (FindBlockStart.scala:8-36)."""
        return int(self.find_block_starts([start], bgzf_blocks_to_check)[0])

    def inflate(self) -> int:
        n = ctypes.c_int64(0)
        self._crc = None
        self.n_loaded = 0  # (a new stream: the context drops what was made from the old one)
        self._index = self._written = None
        self._check(self.L.sbam_inflate(self.ctx, ctypes.byref(n)))
        if self.verify_crc and self.n_blocks is not None:  # (the context checked the whole table)
            self._crc = (0, int(self.n_blocks))
        self.uncompressed_size = n.value
        return n.value

    def inflate_fallbacks(self) -> int:
        """Blocks the last inflate decoded on the exact per-lane path instead of the wave-parallel one."""
        n = ctypes.c_int64(0)
        self._check(self.L.sbam_inflate_fallbacks(self.ctx, ctypes.byref(n)))
        return n.value

    # ---- block CRC32 check
    def set_verify_crc(self, on: bool = True):
        """sbam_set_verify_crc: every later inflate checks each block's CRC32 against its footer and raises
        CrcException on the first mismatch (htslib's bgzf check; htsjdk's setCheckCrcs).  Sticky across reset and
        load; off by default."""
        self._check(self.L.sbam_set_verify_crc(self.ctx, 1 if on else 0))
        self.verify_crc = bool(on)

    def check_crc(self, b0: int = 0, b1: Optional[int] = None) -> dict:
        """sbam_check_crc over blocks [b0, b1) of the table (b1=None: through the last): the totals (n_blocks, n_bad,
        first_bad, bytes) plus `bad`, the mismatching blocks' table indices (int64), and `bad_offsets`, their file
        offsets."""
        t = _CrcTotals()
        self._crc = None
        self._check(self.L.sbam_check_crc(self.ctx, int(b0), -1 if b1 is None else int(b1), ctypes.byref(t)))
        out = {k: int(getattr(t, k)) for k, _ in _CrcTotals._fields_}
        self._crc = (int(b0), int(b0) + out["n_blocks"])
        if out["n_bad"]:
            computed, stored = self.block_crcs()
            bad = int(b0) + np.flatnonzero(computed != stored).astype(np.int64)
        else:
            bad = np.zeros(0, np.int64)
        out["bad"] = bad
        out["bad_offsets"] = self.blocks()[0][bad] if bad.size else np.zeros(0, np.int64)
        return out

    def block_crcs(self, b0: Optional[int] = None, n: Optional[int] = None):
        """(computed, stored) CRC32s as uint32 arrays for blocks [b0, b0 + n) of the last check_crc (default: the
        range it checked; after an inflate with verify_crc, the whole table).  Blocks it did not check: SbamError."""
        if b0 is None:
            b0 = self._crc[0] if self._crc else 0
        if n is None:
            n = (self._crc[1] if self._crc else (self.n_blocks or 0)) - b0
        computed, stored = np.zeros(max(n, 0), np.uint32), np.zeros(max(n, 0), np.uint32)
        self._check(self.L.sbam_get_block_crcs(self.ctx, int(b0), int(n), _ptr(computed), _ptr(stored)))
        return computed, stored

    def read_uncompressed(self, off: int, length: int) -> bytes:
        out = np.zeros(length, np.uint8)
        self._check(self.L.sbam_read_uncompressed(self.ctx, off, length, _ptr(out)))
        return out.tobytes()

    def offset_of(self, pos: Pos) -> int:
        o = ctypes.c_int64(0)
        self._check(self.L.sbam_pos_to_offset(self.ctx, _Pos(pos.block_pos, pos.offset, 0), ctypes.byref(o)))
        return o.value

    def pos_of(self, off: int) -> Pos:
        p = _Pos()
        self._check(self.L.sbam_offset_to_pos(self.ctx, off, ctypes.byref(p)))
        return _pos(p)

    # ---- header
    def header(self):
        n = ctypes.c_int32(0)
        lens = np.zeros(1 << 16, np.int64)
        end = _Pos()
        self._check(self.L.sbam_header(self.ctx, ctypes.byref(n), _ptr(lens), lens.size, ctypes.byref(end)))
        self.n_ref = n.value
        self.contig_lengths = lens[: n.value].copy()
        self.header_end = _pos(end)
        return self.n_ref, self.contig_lengths, self.header_end

    def header_bytes(self) -> bytes:
        """The file's BAM header as it lies in the stream: magic through the last reference (what write_bam puts first,
        and what sam.header_with_sort_order rewrites)."""
        if self.header_end is None:
            self.header()
        return self.read_uncompressed(0, self.offset_of(self.header_end))

    def set_contig_lengths(self, lens: Sequence[int]):
        a = np.asarray(lens, np.int64)
        self._check(self.L.sbam_set_contig_lengths(self.ctx, a.size, _ptr(a)))
        self.n_ref, self.contig_lengths = int(a.size), a.copy()

    # ---- checkers
    def check_eager(self, x0: int = 0, x1: Optional[int] = None, reads_to_check: int = READS_TO_CHECK) -> np.ndarray:
        """eager.Checker at every offset of [x0, x1) → bool array."""
        x1 = self.uncompressed_size if x1 is None else x1
        words = np.zeros((x1 - x0 + 63) // 64 + 1, np.uint64)
        self._check(self.L.sbam_check_eager(self.ctx, x0, x1, reads_to_check, _ptr(words)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        return bits[: x1 - x0].astype(bool)

    def check_eager_device(self, x0: int = 0, x1: Optional[int] = None,
                           reads_to_check: int = READS_TO_CHECK) -> None:
        """check_eager leaving the success bitmap on the device (the split computation reads it there)."""
        x1 = self.uncompressed_size if x1 is None else x1
        self._check(self.L.sbam_check_eager(self.ctx, x0, x1, reads_to_check, None))

    def check_full_words(self, x0: int = 0, x1: Optional[int] = None,
                         reads_to_check: int = READS_TO_CHECK) -> np.ndarray:
        """full.Checker result words (sbam.h layout) for every offset of [x0, x1)."""
        x1 = self.uncompressed_size if x1 is None else x1
        out = np.zeros(max(x1 - x0, 1), np.uint32)
        self._check(self.L.sbam_check_full_words(self.ctx, x0, x1, reads_to_check, _ptr(out)))
        return out[: x1 - x0]

    def check_full_counts(self, x0: int = 0, x1: Optional[int] = None, reads_to_check: int = READS_TO_CHECK,
                          want_bitmap: bool = False, by_key: bool = False):
        x1 = self.uncompressed_size if x1 is None else x1
        c = _Counts()
        bm = np.zeros((x1 - x0 + 63) // 64 + 1, np.uint64) if want_bitmap else None
        self._check(self.L.sbam_check_full_counts(self.ctx, x0, x1, reads_to_check, 1 if by_key else 0,
                                                  ctypes.byref(c), _ptr(bm)))
        counts = Counts(np.ctypeslib.as_array(c.totals).copy(),
                        np.ctypeslib.as_array(c.counts).reshape(21, 19).copy(),
                        np.ctypeslib.as_array(c.positions).copy(),
                        np.ctypeslib.as_array(c.reads_before_error).reshape(21, 128).copy(),
                        np.ctypeslib.as_array(c.pair_hist).reshape(19, 19).copy(),
                        int(c.n_positions), int(c.n_success), int(c.n_too_few_fixed))
        if want_bitmap:
            bits = np.unpackbits(bm.view(np.uint8), bitorder="little")[: x1 - x0].astype(bool)
            return counts, bits
        return counts

    def eager_checker(self, reads_to_check: int = READS_TO_CHECK):
        """Checker[Boolean] (check/.../check/Checker.scala:7-9) backed by a bulk GPU bitmap, the
        indexed.Checker precedent (check/.../check/indexed/Checker.scala:12-27)."""
        bits = self.check_eager(0, self.uncompressed_size, reads_to_check)
        return lambda pos: bool(bits[self.offset_of(pos)])

    def full_checker(self, reads_to_check: int = READS_TO_CHECK):
        words = self.check_full_words(0, self.uncompressed_size, reads_to_check)
        return lambda pos: int(words[self.offset_of(pos)])

    def find_record_start_with_delta(self, block_start: int, reads_to_check: int = READS_TO_CHECK,
                                     max_read_size: int = MAX_READ_SIZE):
        """FindRecordStart.withDelta from Pos(block_start, 0): (Pos, delta) or None."""
        found, p, d = ctypes.c_int32(0), _Pos(), ctypes.c_int32(0)
        self._check(self.L.sbam_find_record_start(self.ctx, block_start, reads_to_check, max_read_size,
                                                  ctypes.byref(found), ctypes.byref(p), ctypes.byref(d)))
        return (_pos(p), d.value) if found.value else None

    def find_record_start(self, block_start: int, reads_to_check: int = READS_TO_CHECK,
                          max_read_size: int = MAX_READ_SIZE) -> Pos:
        """FindRecordStart.apply: raises NoReadFoundException on None (FindRecordStart.scala:11-28)."""
        r = self.find_record_start_with_delta(block_start, reads_to_check, max_read_size)
        if r is None:
            raise NoReadFoundException(
                f"Failed to find a valid read-start in {max_read_size} attempts in {self.path} from {block_start}")
        return r[0]

    # ---- splits / records (CanLoadBam)
    def _args(self, split_size, bgzf_blocks_to_check, reads_to_check, max_read_size, use_bitmap):
        return _SplitArgs(split_size, bgzf_blocks_to_check, reads_to_check, max_read_size, 1 if use_bitmap else 0)

    def split_records(self, split_size: int, first: int = 0, count: Optional[int] = None,
                      bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK, reads_to_check: int = READS_TO_CHECK,
                      max_read_size: int = MAX_READ_SIZE, use_success_bitmap: bool = False):
        """Per Hadoop split: (first record Pos, non-empty?, record count)."""
        bp, off, nonempty, n = self.split_records_arrays(split_size, first, count, bgzf_blocks_to_check,
                                                         reads_to_check, max_read_size, use_success_bitmap)
        return [(Pos(int(bp[i]), int(off[i])), bool(nonempty[i]), int(n[i])) for i in range(bp.size)]

    def split_records_arrays(self, split_size: int, first: int = 0, count: Optional[int] = None,
                             bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK, reads_to_check: int = READS_TO_CHECK,
                             max_read_size: int = MAX_READ_SIZE, use_success_bitmap: bool = False):
        """split_records as arrays (first record block_pos, offset, non-empty, record count): no per-split
        Python objects (a 10 GB file has ~5000 splits)."""
        ns = n_hadoop_splits(self.file_size, split_size)
        count = ns - first if count is None else count
        fp = np.zeros(max(count, 1), dtype=[("block_pos", "<i8"), ("offset", "<i4"), ("reserved", "<i4")])
        fd = np.zeros(max(count, 1), np.int32)
        nr = np.zeros(max(count, 1), np.int64)
        a = self._args(split_size, bgzf_blocks_to_check, reads_to_check, max_read_size, use_success_bitmap)
        self._check(self.L.sbam_split_records(self.ctx, ctypes.byref(a), first, count, fp.ctypes.data,
                                              _ptr(fd), _ptr(nr)))
        return (fp["block_pos"][:count].copy(), fp["offset"][:count].astype(np.int64), fd[:count] != 0,
                nr[:count].copy())

    def partition_sizes(self, split_size: int, **kw) -> List[int]:
        """records.partitionSizes of sc.loadReads / loadBam (LoadBAMTest.scala:24-45)."""
        return [n for (_, _, n) in self.split_records(split_size, **kw)]

    def compute_splits(self, split_size: int, bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK,
                       reads_to_check: int = READS_TO_CHECK, max_read_size: int = MAX_READ_SIZE,
                       use_success_bitmap: bool = False) -> List[Split]:
        """loadSplitsAndReads(...).splits (CanLoadBam.scala:245-279)."""
        a = self._args(split_size, bgzf_blocks_to_check, reads_to_check, max_read_size, use_success_bitmap)
        cap = n_hadoop_splits(self.file_size, split_size) + 1
        out = (_Split * cap)()
        n = ctypes.c_int64(0)
        self._check(self.L.sbam_compute_splits(self.ctx, ctypes.byref(a), ctypes.addressof(out), cap,
                                               ctypes.byref(n)))
        return [Split(_pos(out[i].start), _pos(out[i].end)) for i in range(n.value)]

    def record_offsets(self, x0: int, x_end: int) -> np.ndarray:
        cap = max((x_end - x0) // 36 + 2, 2)
        out = np.zeros(cap, np.int64)
        n = ctypes.c_int64(0)
        self._check(self.L.sbam_record_offsets(self.ctx, x0, x_end, _ptr(out), cap, ctypes.byref(n)))
        return out[: n.value]

    def load_records(self, split_size: int, first: int = 0, count: Optional[int] = None,
                     bgzf_blocks_to_check: int = BGZF_BLOCKS_TO_CHECK, reads_to_check: int = READS_TO_CHECK,
                     max_read_size: int = MAX_READ_SIZE, use_success_bitmap: bool = False,
                     columns: Optional[Sequence[str]] = tuple(RECORD_COLUMNS)):
        """Records of Hadoop splits [first, first+count) decoded on the GPU (sbam_load_records): returns
        (partition sizes, {column: ndarray}) with the records of all those splits concatenated in split order.
        `columns=None` leaves the columns on the device (count only)."""
        ns = n_hadoop_splits(self.file_size, split_size)
        count = ns - first if count is None else count
        sizes = np.zeros(max(count, 1), np.int64)
        n = ctypes.c_int64(0)
        a = self._args(split_size, bgzf_blocks_to_check, reads_to_check, max_read_size, use_success_bitmap)
        self._check(self.L.sbam_load_records(self.ctx, ctypes.byref(a), first, count, _ptr(sizes), ctypes.byref(n)))
        sizes = sizes[:count]
        self.n_loaded = int(n.value)
        if columns is None:
            return sizes, {}
        cols = {k: np.zeros(n.value, RECORD_COLUMNS[k]) for k in columns}
        rc = _RecordColumns(**{k: v.ctypes.data for k, v in cols.items()})
        self._check(self.L.sbam_get_record_columns(self.ctx, 0, n.value, ctypes.byref(rc)))
        return sizes, cols

    def records_path(self) -> dict:
        """What the last split_records / compute_splits / load_records did (sbam_records_path): `tried` the success
        bitmap, `proved` the chains equal to it; `missing_links` / `failed_fallbacks` of the list-form chain pass
        behind that bitmap (-1: no such bitmap, or a later check ran first)."""
        t, p, m, f = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(-1), ctypes.c_int64(-1)
        self._check(self.L.sbam_records_path(self.ctx, ctypes.byref(t), ctypes.byref(p), ctypes.byref(m),
                                             ctypes.byref(f)))
        return {"tried": bool(t.value), "proved": bool(p.value), "missing_links": int(m.value),
                "failed_fallbacks": int(f.value)}

    def load_record_fields(self, i0: int = 0, n: Optional[int] = None,
                           fields: Sequence[str] = ("name", "cigar", "seq", "qual", "aux"), host: bool = True):
        """Names, CIGARs, bases, qualities and tags of records [i0, i0 + n) of the last load_records, decoded on the
        GPU into CSR columns (sbam_load_record_fields: what htsjdk's BAMRecordCodec.decode gives loadReads' SAMRecords,
        CanLoadBam.scala:221-241).  `n=None`: through the last loaded record.  Returns a RecordFields with the numpy
        columns; with host=False it holds only the totals and the columns stay on the device
        (sbam_record_fields_device)."""
        if n is None:
            n = max(self.n_loaded - i0, 0)
        mask = 0
        for f in fields:
            if f not in FIELD_BITS:
                raise ValueError(f"unknown field {f!r}")
            mask |= FIELD_BITS[f]
        tot = _RecordFieldTotals()
        self._check(self.L.sbam_load_record_fields(self.ctx, int(i0), int(n), mask, ctypes.byref(tot)))
        totals = {k: int(getattr(tot, k)) for k, _ in _RecordFieldTotals._fields_}
        out = RecordFields(int(i0), int(n), totals)
        if not host:
            return out
        ptrs = {}
        for name in ("name_off", "cigar_off", "seq_off", "aux_off"):
            a = np.zeros(n + 1, np.int64)
            setattr(out, name, a)
            ptrs[name] = a.ctypes.data
        for f in fields:
            dt, _, tk = _FIELD_LAYOUT[f]
            a = np.zeros(totals[tk], dt)
            setattr(out, f, a)
            ptrs[f] = a.ctypes.data if a.size else None
        rf = _RecordFields(**ptrs)
        self._check(self.L.sbam_get_record_fields(self.ctx, ctypes.byref(rf)))
        return out

    def load_record_tags(self, tags: Sequence[str], i0: int = 0, n: Optional[int] = None,
                         bytes_for: Sequence[str] = (), host: bool = True) -> RecordTags:
        """The tags named in `tags` of records [i0, i0 + n) of the last load_records as typed columns, decoded on the
        GPU from the inflated stream (sbam_load_record_tags: htsjdk's SAMRecord.getAttribute over loadReads' records,
        CanLoadBam.scala:221-241; SAM spec §4.2.4).  `bytes_for`: the tags whose value bytes (Z and H characters, B
        elements) are wanted as CSR columns.  `n=None`: through the last loaded record.  With host=False only the
        totals are filled and the columns stay on the device (sbam_record_tags_device)."""
        tags = tuple(tags)
        if n is None:
            n = max(self.n_loaded - i0, 0)
        for t in list(tags) + list(bytes_for):
            if not isinstance(t, str) or len(t.encode("latin-1", "replace")) != 2:
                raise ValueError(f"not a two-character tag name: {t!r}")
        if not set(bytes_for) <= set(tags):
            raise ValueError(f"bytes_for names tags that are not queried: {sorted(set(bytes_for) - set(tags))}")
        q = (_TagQuery * max(len(tags), 1))()
        for j, t in enumerate(tags):
            q[j].tag = t.encode("latin-1", "replace")
            q[j].want_bytes = 1 if t in bytes_for else 0
        tot = _RecordTagTotals()
        self._check(self.L.sbam_load_record_tags(self.ctx, int(i0), int(n), q, len(tags), ctypes.byref(tot)))
        totals = {t: {"present": int(tot.present[j]), "bytes": int(tot.bytes[j])} for j, t in enumerate(tags)}
        out = RecordTags(int(i0), int(n), tags, totals)
        if not host:
            return out
        shape = (len(tags), n)
        out.type, out.sub = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        out.rel, out.value = np.zeros(shape, np.int32), np.zeros(shape, np.int64)
        out.bytes_off, out.bytes = {}, {}
        rt = _RecordTags(type=out.type.ctypes.data, sub=out.sub.ctypes.data, rel=out.rel.ctypes.data,
                         value=out.value.ctypes.data)
        for j, t in enumerate(tags):
            if t in bytes_for:
                out.bytes_off[t] = np.zeros(n + 1, np.int64)
                out.bytes[t] = np.zeros(totals[t]["bytes"], np.uint8)
                rt.bytes_off[j] = out.bytes_off[t].ctypes.data
                rt.bytes[j] = out.bytes[t].ctypes.data if out.bytes[t].size else None
        self._check(self.L.sbam_get_record_tags(self.ctx, ctypes.byref(rt)))
        return out

    # ---- BAI writer
    def build_index(self, split_size: int = LOCAL_FS_BLOCK_SIZE, use_success_bitmap: bool = False) -> dict:
        """sbam_build_index over the whole file's records; they are loaded first (load_records over every split of
        `split_size`) when the context does not hold them.  Returns the totals."""
        t = _IndexTotals()
        rc = self.L.sbam_build_index(self.ctx, ctypes.byref(t))
        if rc == ERR_STATE and self.base_offset == 0 and self.file_size == self._buf.size \
                and self.uncompressed_size is not None:
            self.load_records(split_size, use_success_bitmap=use_success_bitmap, columns=None)
            rc = self.L.sbam_build_index(self.ctx, ctypes.byref(t))
        self._check(rc)
        self._index = {k: int(getattr(t, k)) for k, _ in _IndexTotals._fields_ if k != "reserved"}
        return self._index

    def index_runs(self):
        """The raw runs of the last build_index / build_bai in file order: (ref int32, bin uint32, beg uint64,
        end uint64), one entry per maximal stretch of records with the same (ref_id, bin)."""
        if self._index is None:
            raise SbamError("build_index has not run")
        n = self._index["n_runs"]
        ref, bn, beg, end = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._check(self.L.sbam_get_index_runs(self.ctx, _ptr(ref), _ptr(bn), _ptr(beg), _ptr(end)))
        return ref, bn, beg, end

    def index_refs(self) -> IndexRefs:
        """The linear index (after the fill) and the per-reference metadata of the last build_index / build_bai."""
        if self._index is None:
            raise SbamError("build_index has not run")
        t = self._index
        nr = t["n_ref"]
        iv, io = np.zeros(nr + 1, np.int64), np.zeros(t["n_intv_total"], np.uint64)
        ob, oe, nm, nu = np.zeros(nr, np.uint64), np.zeros(nr, np.uint64), np.zeros(nr, np.int64), np.zeros(nr, np.int64)
        self._check(self.L.sbam_get_index_refs(self.ctx, _ptr(iv), _ptr(io), _ptr(ob), _ptr(oe), _ptr(nm), _ptr(nu)))
        return IndexRefs(iv, io, ob, oe, nm, nu, t["n_no_coor"], t["n_unsorted"], t["n_records"])

    def build_bai(self, split_size: int = LOCAL_FS_BLOCK_SIZE, require_sorted: bool = True,
                  use_success_bitmap: bool = False) -> bytes:
        """The file's .bai bytes (SAM spec §5.2), built on the GPU from the decoded record columns (sbam_build_index,
        sbam_write_bai).  A file whose records are not in coordinate order raises SbamError("unsorted positions")
        unless require_sorted is False (the index is defined for any order; readers assume a sorted file)."""
        t = self.build_index(split_size, use_success_bitmap)
        if require_sorted and t["n_unsorted"] > 0:
            raise SbamError("unsorted positions")
        n = ctypes.c_int64(0)
        if self.L.sbam_write_bai(self.ctx, None, 0, ctypes.byref(n)) == ERR_STATE:
            self._check(ERR_STATE)
        out = np.zeros(n.value, np.uint8)
        self._check(self.L.sbam_write_bai(self.ctx, _ptr(out), out.size, ctypes.byref(n)))
        return out.tobytes()

    # ---- coordinate sort
    def sort_records(self) -> dict:
        """sbam_sort_records: the stable coordinate order of the loaded records ((uint32) ref_id, then pos; ties in
        loaded order), on the GPU.  Returns the totals: n_records, n_out_of_order (before the sort), passes."""
        t = _SortTotals()
        self._check(self.L.sbam_sort_records(self.ctx, ctypes.byref(t)))
        return {k: int(getattr(t, k)) for k, _ in _SortTotals._fields_ if k != "reserved"}

    def sort_order(self, i0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Entries [i0, i0 + n) of the last sort_records' order (int64): order[k] = loaded index of the k-th record."""
        if n is None:
            p, total = ctypes.c_void_p(), ctypes.c_int64(0)
            self._check(self.L.sbam_sort_order_device(self.ctx, ctypes.byref(p), ctypes.byref(total)))
            n = total.value - i0
        out = np.zeros(max(n, 0), np.int64)
        self._check(self.L.sbam_get_sort_order(self.ctx, i0, n, _ptr(out)))
        return out

    # ---- BAM writer
    def _upload(self, a: np.ndarray) -> int:
        """A device copy of a host array, allocated through the HIP runtime libsbam.so is linked to (dlsym through the
        library's handle reaches its dependencies): the pointer is then valid in the library's kernels whichever
        runtime torch brought along, and no torch is needed.  The caller frees it with hipFree."""
        L = self.L
        L.hipSetDevice.argtypes, L.hipMalloc.argtypes = [ctypes.c_int], [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        L.hipFree.argtypes = [ctypes.c_void_p]
        p = ctypes.c_void_p()
        if L.hipSetDevice(self.device) or L.hipMalloc(ctypes.byref(p), max(a.nbytes, 1)):
            raise SbamError("hipMalloc failed")
        if a.nbytes and L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1):  # hipMemcpyHostToDevice
            L.hipFree(p)
            raise SbamError("hipMemcpy failed")
        return p.value

    def write_bam(self, path: Optional[str] = None, ranges: Optional[Sequence[Tuple[int, int]]] = None, keep=None,
                  level: int = 1, block_bytes: int = WRITE_BLOCK_BYTES, with_header: bool = True,
                  with_eof: bool = True, huffman: str = "fixed", order=None, header: Optional[bytes] = None):
        """The records of the last load_records back into BGZF bytes on the GPU (sbam_write_bam; htsjdk-rewrite,
        HTSJDKRewrite.scala:21-91): the BAM header, then the records inside `ranges` (record-index pairs [lo, hi),
        ascending and disjoint; None: all) whose `keep` byte is nonzero (a torch bool / uint8 tensor on this device, or
        a numpy array, which is uploaded; None: all), cut every `block_bytes`, deflated at `level` (0 stored, 1 LZ77 +
        Huffman codes: `huffman` = "fixed", or "dynamic" for per block the smallest of stored, fixed and dynamic,
        level | SBAM_WRITE_DYNAMIC) and framed.  `order` (sbam_write_bam_ordered): "sorted" writes them in the order of
        the last sort_records; an int64 torch tensor on this device or a numpy array (uploaded) of n_loaded entries
        writes loaded record order[k] k-th (ranges and keep still select by loaded index; a repeated entry is written
        twice).  `header`: the bytes of a complete BAM header written instead of the file's (sam.header_with_sort_order).
        Returns the totals as a dict; the file bytes go to `path`, or with
        path=None into the dict as "bytes"."""
        if huffman not in ("fixed", "dynamic"):
            raise ValueError(f"huffman is 'fixed' or 'dynamic', not {huffman!r}")
        if huffman == "dynamic":
            if int(level) == 0:
                raise ValueError("huffman='dynamic' needs level 1: level 0 writes stored blocks only")
            level = int(level) | SBAM_WRITE_DYNAMIC
        ranges = [] if ranges is None else [(int(a), int(b)) for a, b in ranges]
        lo = np.asarray([a for a, _ in ranges], np.int64)
        hi = np.asarray([b for _, b in ranges], np.int64)
        keep_ptr, staged = None, None
        if keep is not None:
            if int(np.prod(keep.shape)) != self.n_loaded:
                raise ValueError(f"keep has {int(np.prod(keep.shape))} entries for {self.n_loaded} loaded records")
            if isinstance(keep, np.ndarray):
                staged = keep_ptr = self._upload(np.ascontiguousarray(keep).astype(np.uint8))
            else:
                import torch
                if not keep.is_cuda or keep.device.index != self.device or keep.element_size() != 1:
                    raise ValueError("keep: a bool / uint8 tensor on this BamFile's device, or a numpy array")
                keep = keep.contiguous()
                torch.cuda.synchronize(keep.device)
                keep_ptr = keep.data_ptr()
        ordered = order is not None or header is not None
        order_ptr, staged_order = None, None
        if order is not None and not (isinstance(order, str) and order == "sorted"):
            if isinstance(order, str):
                raise ValueError(f"order is 'sorted', a tensor or an array, not {order!r}")
            if int(np.prod(order.shape)) != self.n_loaded:
                raise ValueError(f"order has {int(np.prod(order.shape))} entries for {self.n_loaded} loaded records")
            if isinstance(order, np.ndarray):
                staged_order = order_ptr = self._upload(np.ascontiguousarray(order).astype(np.int64))
            else:
                import torch
                if not order.is_cuda or order.device.index != self.device or order.dtype != torch.int64:
                    raise ValueError("order: an int64 tensor on this BamFile's device, or a numpy array")
                order = order.contiguous()
                torch.cuda.synchronize(order.device)
                order_ptr = order.data_ptr()
        elif order is None and ordered:  # a header alone: the loaded order
            staged_order = order_ptr = self._upload(np.arange(self.n_loaded, dtype=np.int64))
        hbuf = np.frombuffer(bytes(header), np.uint8) if header is not None else None
        o = _WriteOrder(order_ptr, _ptr(hbuf) if hbuf is not None and hbuf.size else None,
                        hbuf.size if hbuf is not None else 0)
        a = _WriteArgs(_ptr(lo) if lo.size else None, _ptr(hi) if hi.size else None, lo.size,
                       keep_ptr if self.n_loaded else None, int(level), int(block_bytes), 1 if with_header else 0,
                       1 if with_eof else 0)
        t = _WriteTotals()
        try:
            if ordered:
                rc = self.L.sbam_write_bam_ordered(self.ctx, ctypes.byref(a), ctypes.byref(o), ctypes.byref(t))
            else:
                rc = self.L.sbam_write_bam(self.ctx, ctypes.byref(a), ctypes.byref(t))
        finally:
            for q in (staged, staged_order):
                if q:
                    self.L.hipFree(ctypes.c_void_p(q))
        self._check(rc)
        out = {k: int(getattr(t, k)) for k, _ in _WriteTotals._fields_}
        self._written = out
        data = np.zeros(out["comp_bytes"], np.uint8)
        self._check(self.L.sbam_get_written(self.ctx, _ptr(data), data.size))
        if path is None:
            out = dict(out, bytes=data.tobytes())
        else:
            with open(path, "wb") as fh:
                fh.write(data.tobytes())
        return out

    def written_blocks(self):
        """(start, csize, usize) of the data blocks of the last write_bam (sbam_get_written_blocks: the new file's
        .blocks sidecar, HTSJDKRewrite.scala:78-83)."""
        n = self._written["n_blocks"] if self._written else 0
        st, cs, us = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self.L.sbam_get_written_blocks(self.ctx, _ptr(st), _ptr(cs), _ptr(us)))
        return st, cs, us

    def written_records(self):
        """(block_pos, offset) of every record the last write_bam wrote, in the new file (sbam_get_written_records:
        its .records sidecar, HTSJDKRewrite.scala:85-90)."""
        n = self._written["n_records"] if self._written else 0
        bp, bo = np.zeros(n, np.int64), np.zeros(n, np.int32)
        self._check(self.L.sbam_get_written_records(self.ctx, _ptr(bp), _ptr(bo)))
        return bp, bo

    def record_spans(self, offsets: np.ndarray):
        """(ref_id, start, end) of the records at `offsets`: [getStart - 1, getEnd) as CanLoadBam.region uses it
        (unmapped: end 0)."""
        offs = np.ascontiguousarray(offsets, np.int64)
        n = offs.size
        r, a, b = (np.zeros(n, np.int32) for _ in range(3))
        self._check(self.L.sbam_record_spans(self.ctx, _ptr(offs), n, _ptr(r), _ptr(a), _ptr(b)))
        return r, a, b

    def _vpos_offset(self, v: int) -> int:
        """Stream offset of an htsjdk virtual offset (block << 16 | offset); an address at or behind the end of the
        last block (the EOF marker) maps to the stream end, any other address that starts no block is an error."""
        st, cs, us, uo = self.blocks()
        b, o = v >> 16, v & 0xffff
        i = int(np.searchsorted(st, b))
        if i < st.size and int(st[i]) == b:
            return int(uo[i]) + min(o, int(us[i]))
        if i >= st.size and (st.size == 0 or b >= int(st[-1]) + int(cs[-1])):
            return self.uncompressed_size
        raise SbamError(f"no BGZF block at {b}")

    def load_bam_intervals(self, bai: Optional[bytes] = None, loci: str = "", split_size: int = 32 << 20, ratio: float = 3.0):
        """sc.loadBamIntervals (CanLoadBam.scala:59-138): the BAI chunks overlapping `loci` (htsjdk getFileSpan,
        sbam.bai), grouped into partitions by estimated size (cappedCostGroups), and per chunk the records from
        chunk.start while Pos < chunk.end whose [getStart - 1, getEnd) intersects the loci.  Record chains and
        reference spans run on the GPU (sbam_record_offsets, sbam_record_spans).  Returns (chunks, partitions):
        partitions = per partition, the record stream offsets kept, in file order.  (The MaxSplitSize default of
        32 MiB is hammerlab's, outside the reference tree: parity unpinned.)  `bai=None`: the index is built here
        (build_bai), so a file without a sidecar index works."""
        from sbam import bai as B
        from sbam.cli import header_names
        if bai is None:
            bai = self.build_bai()
        refs = B.parse_bai(bai)
        names = header_names(self)
        q = []
        for contig, a, e in B.parse_loci(loci):
            ri = names.index(contig) if contig in names else -1
            q.append((ri, a + 1, e if e is not None else 0))  # toHtsJDKIntervals: 1-based closed
        chunks = B.file_span(refs, q)
        groups = B.capped_cost_groups([c.size(ratio) for c in chunks], float(split_size))
        want = [(names.index(c) if c in names else -2, a, e) for c, a, e in B.parse_loci(loci)]
        parts = []
        for g in groups:
            kept = []
            for ci in g:
                c = chunks[ci]
                offs = self.record_offsets(self._vpos_offset(c.start), self._vpos_offset(c.end))
                if offs.size == 0:
                    continue
                ri, st, en = self.record_spans(offs)
                m = np.zeros(offs.size, bool)
                for r, a, e in want:
                    m |= (ri == r) & (st < (e if e is not None else 1 << 31)) & (en > a)
                kept.append(offs[m])
            parts.append(np.concatenate(kept) if kept else np.zeros(0, np.int64))
        return chunks, parts

    def load_reads_and_positions(self, split_size: int, **kw):
        """loadReadsAndPositions: per partition, list of (Pos, record bytes) (CanLoadBam.scala:281-334).  Record
        offsets and Pos come from sbam_load_records; each partition's bytes are one contiguous stream slice."""
        sizes, c = self.load_records(split_size, columns=("offset", "block_pos", "block_off", "block_size"), **kw)
        parts, i = [], 0
        for n in sizes.tolist():
            recs = []
            if n:
                off, bs = c["offset"][i:i + n], c["block_size"][i:i + n]
                x0, x1 = int(off[0]), int(off[-1]) + 4 + int(bs[-1])
                raw = self.read_uncompressed(x0, x1 - x0)
                for j in range(n):
                    o = int(off[j]) - x0
                    recs.append((Pos(int(c["block_pos"][i + j]), int(c["block_off"][i + j])), raw[o:o + 4 + int(bs[j])]))
            parts.append(recs)
            i += n
        return parts

    def load_reads(self, split_size: int, **kw):
        """sc.loadReads (CanLoadBam.scala:348-352): per partition, list of record bytes."""
        return [[r for (_, r) in p] for p in self.load_reads_and_positions(split_size, **kw)]


def read_name(record: bytes) -> str:
    """read_name field of a BAM record (bytes starting at block_size)."""
    lrn = record[12]
    return record[36:36 + lrn - 1].decode()
