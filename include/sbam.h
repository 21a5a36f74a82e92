/*
 * sbam.h — C ABI of the MI355X-native spark-bam hot path (libsbam.so).
 *
 * Plain C types only (fixed-width ints, caller-owned host buffers, opaque handle), so a JVM
 * binding (JDK 22 Panama downcalls, or a JNI shim) or ctypes can call it directly; INTEGRATION.md
 * shows the reference-side binding for each entry point.  Every entry point names the reference
 * interface it replaces (paths relative to the spark-bam repository root).
 *
 * Threading / ownership (mirrors the reference's per-Spark-task channels, Channels.scala:15-26,
 * CallPartition.scala:35-37): one handle per task/file-shard, reentrant per handle, no global
 * mutable state, device memory owned by the handle and freed by sbam_close().  Errors are int
 * status codes plus a per-handle error record whose message text equals the reference exception's.
 */
#ifndef SBAM_H
#define SBAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------------- */
#define SBAM_OK 0
#define SBAM_ERR_HEADER_PARSE 1   /* HeaderParseException        bgzf/.../block/HeaderParseException.scala:6-11 */
#define SBAM_ERR_HEADER_SEARCH 2  /* HeaderSearchFailedException bgzf/.../block/FindBlockStart.scala:31-35;
                                     error.position = start, error.actual = positionsAttempted              */
#define SBAM_ERR_INFLATE 3        /* IOException "Expected N decompressed bytes, found M" Stream.scala:52-54 */
#define SBAM_ERR_NO_READ_FOUND 4  /* NoReadFoundException        check/.../bam/spark/FindRecordStart.scala:66-71;
                                     error.position = start, error.expected = maxReadSize                   */
#define SBAM_ERR_NOT_BAM 5        /* require(magic == "BAM\1")   check/.../bam/header/Header.scala:44-46      */
#define SBAM_ERR_ARG 6            /* invalid argument / capacity too small                                  */
#define SBAM_ERR_HIP 7            /* HIP runtime failure (device, allocation, launch)                       */
#define SBAM_ERR_STATE 8          /* stage called out of order (e.g. check before inflate)                  */
#define SBAM_ERR_HALO 9           /* a check needed bytes past a shard's loaded range (grow the halo)       */
#define SBAM_ERR_RECORD 10        /* variable-length fields overrun block_size, or (sbam_build_index) a record no
                                     BAI can index; error.position = record offset                          */
#define SBAM_ERR_CRC 11           /* a block's inflated bytes do not have the CRC32 its footer stores; error.position =
                                     the block's file offset, error.expected = stored, error.actual = computed */

typedef struct sbam_ctx sbam_ctx;

/* Virtual position: Pos(blockPos, offset), bgzf/src/main/scala/org/hammerlab/bgzf/Pos.scala:12 */
typedef struct {
  int64_t block_pos;
  int32_t offset;
  int32_t reserved;
} sbam_pos;

/* Split(start, end), check/src/main/scala/org/hammerlab/bam/spark/Split.scala:9-13 */
typedef struct {
  sbam_pos start;
  sbam_pos end;
} sbam_split;

typedef struct {
  int32_t code;      /* SBAM_ERR_* */
  int32_t idx;       /* HeaderParseException idx */
  int64_t actual;    /* HeaderParseException actual / inflate "found" */
  int64_t expected;  /* HeaderParseException expected / inflate "expected" */
  int64_t position;  /* compressed (or split-start) offset the error refers to */
  char message[512]; /* reference exception message text */
} sbam_error;

/* full-check reductions (check/.../full/error/Counts.scala:8-130; cli/.../full/FullCheck.scala:141-191).
 * Results equal to Flags.TooFewFixedBlockBytes (flag 0 alone, readsBeforeError 0) are dropped (counted in
 * n_too_few_fixed); every other Flags result is keyed by numNonZeroFields = popcount(flags) +
 * (readsBeforeError > 0). Flag index order = Flags.scala:201-223 bitset order. */
#define SBAM_NUM_FLAGS 19
#define SBAM_NUM_KEYS 21
#define SBAM_MAX_READS_TO_CHECK 127
typedef struct {
  int64_t totals[SBAM_NUM_FLAGS];                           /* per flag, all keys ("Total error counts") */
  int64_t counts[SBAM_NUM_KEYS][SBAM_NUM_FLAGS];            /* per key, per flag: keys 1-2 always, all with by_key */
  int64_t positions[SBAM_NUM_KEYS];                         /* positions per key */
  int64_t reads_before_error[SBAM_NUM_KEYS][SBAM_MAX_READS_TO_CHECK + 1];
  int64_t pair_hist[SBAM_NUM_FLAGS][SBAM_NUM_FLAGS];        /* key-2 positions by (flag i < flag j) */
  int64_t n_positions;                                      /* positions checked */
  int64_t n_success;                                        /* positions whose call is true */
  int64_t n_too_few_fixed;                                  /* dropped TooFewFixedBlockBytes results */
  int64_t n_halo;                                           /* positions that needed bytes past the shard */
} sbam_counts;

/* Per-position result word of the full checker (full/Checker.scala:22-184):
 * bits 0..18 = Flags bits, bits 24..30 = readsBeforeError (or Success.readsParsed), bit 31 = Success. */
#define SBAM_WORD_SUCCESS 0x80000000u
#define SBAM_WORD_HALO 0x00800000u /* bit 23: result unknown, chain left the shard's loaded bytes */

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Open a BAM file (or a shard of one) on a GPU: copies `len` compressed bytes that sit at file offset
 * `base_offset` of a file of `file_size` bytes into HBM.  For a whole file pass base_offset 0 and
 * file_size == len.  Replaces Channels(path) (load/.../spark/load/Channels.scala:15-26). */
int sbam_open(int device, const uint8_t *data, int64_t len, int64_t base_offset, int64_t file_size,
              sbam_ctx **out);
void sbam_close(sbam_ctx *ctx);
/* Replace the resident compressed bytes of an open context with another byte range (of the same or another
 * file) and drop every derived stage, keeping the device allocations: the streaming form of sbam_open for
 * inputs larger than HBM, one byte-range window after another (a Spark task re-opening its channel at the
 * next split range).  `data` may be pinned host memory; the copy is on the context's stream, so a second
 * context can load the next window while this one computes.  Contig lengths persist only for a later window
 * of the same file (base_offset > 0 and the same file_size); otherwise sbam_header / sbam_set_contig_lengths
 * must run again before a check. */
int sbam_load(sbam_ctx *ctx, const uint8_t *data, int64_t len, int64_t base_offset, int64_t file_size);
/* Size a context's device buffers for windows of up to comp_bytes compressed bytes, n_blocks BGZF blocks,
 * ubytes uncompressed bytes and n_records records (0: leave the record-sized buffers alone), so that no later
 * sbam_load / stage reallocates: the buffers are grow-only, and growing one is a hipFree + hipMalloc of up to
 * tens of GB that synchronises the device (a streamed Spark task whose next split range is larger than any
 * before it).  Allocates nothing that is already large enough.  The resident compressed bytes and contig lengths
 * are kept; when any stage buffer grows on a context that has already run a stage, every derived stage is
 * dropped (as sbam_reset) and later queries re-run them.  (No reference counterpart: the JVM channel has no
 * device memory; CanLoadBam.scala:281-334 re-opens a channel per split.) */
int sbam_reserve(sbam_ctx *ctx, int64_t comp_bytes, int64_t n_blocks, int64_t ubytes, int64_t n_records);
const sbam_error *sbam_last_error(const sbam_ctx *ctx);
/* The path (Path.toString) that exception messages name, as the reference's HeaderSearchFailedException /
 * NoReadFoundException format it (HeaderSearchFailedException.scala:7-12, FindRecordStart.scala:66-71);
 * default "<bytes>". */
int sbam_set_path(sbam_ctx *ctx, const char *path);
/* Drop every derived stage (block table, stream, bitmap) but keep the compressed bytes and the device
 * allocations, so the pipeline can be re-run from the resident input without allocating (bench). */
int sbam_reset(sbam_ctx *ctx);
const char *sbam_version(void);

/* ---- BGZF layer -------------------------------------------------------------------------------- */

/* FindBlockStart.apply for a batch of split starts (bgzf/.../block/FindBlockStart.scala:8-36).
 * out[i] = first start[i]+pos, pos < 65536, at which `blocks_to_check` BGZF headers chain. */
int sbam_find_block_starts(sbam_ctx *ctx, const int64_t *starts, int64_t n, int32_t blocks_to_check, int64_t *out);

/* MetadataStream from the shard's first block (offset 0 of a whole file; FindBlockStart(base_offset)
 * of a shard) to the end of the stream (MetadataStream.scala:23-54): builds the device block table.
 * *n_blocks receives the block count. */
int sbam_scan_blocks(sbam_ctx *ctx, int64_t *n_blocks);

/* Which way the last sbam_scan_blocks took to its table (read-only; no reference counterpart):
 *   *followed   1 when the table came from following the headers' BSIZE hops in parallel segments;
 *   *fell_back  1 when that was tried and not accepted (a segment's speculative entry was not on the chain, a parse
 *               failure, more blocks in a segment than its slots), and the byte scan built the table instead;
 *   *segments   the segments followed (0 when following was not tried: a candidate list already existed, or
 *               SBAM_SCAN_FOLLOW=0 in the environment).
 * All 0 before a scan.  Any pointer may be NULL. */
int sbam_scan_path(sbam_ctx *ctx, int32_t *followed, int32_t *fell_back, int64_t *segments);
/* Bytes per segment of that path (a build constant; tests place headers at segment edges). */
int sbam_follow_segment_bytes(void);

/* Copy the block table (IndexBlocks format: start, compressedSize, uncompressedSize;
 * bgzf/.../index/IndexBlocks.scala:40-44) plus each block's offset in the uncompressed stream. */
int sbam_get_blocks(sbam_ctx *ctx, int64_t *start, int32_t *csize, int32_t *usize, int64_t *uoff, int64_t cap);

/* Inflate every block of the table into the device-resident uncompressed stream
 * (Stream.scala:31-71 with Inflater(nowrap=true)); *uncompressed_size receives its length. */
int sbam_inflate(sbam_ctx *ctx, int64_t *uncompressed_size);

/* Blocks the last sbam_inflate handed from the wave-parallel decoder to the exact per-lane one (stored or
 * invalid blocks, incomplete codes, streams that end before ISIZE or run past it); for parity tests and profiles. */
int sbam_inflate_fallbacks(sbam_ctx *ctx, int64_t *n);

/* ---- BGZF block CRC32 check -------------------------------------------------------------------------- */

typedef struct {
  int64_t n_blocks;  /* blocks checked */
  int64_t n_bad;     /* blocks whose computed CRC32 differs from the footer's */
  int64_t first_bad; /* table index of the first of them, -1: none */
  int64_t bytes;     /* uncompressed bytes of the checked blocks */
} sbam_crc_totals;

/* CRC32 (IEEE, as zlib's crc32) of the inflated bytes of blocks [b0, b1) of the table, computed on the GPU from the
 * resident stream and compared with the value each block's footer stores; b1 < 0: through the last block.  The
 * reference has no counterpart: Stream.scala:49-54 enforces ISIZE and never reads the CRC.  The behaviour mirrored is
 * htslib's bgzf reader, which checks every block it inflates (`bgzip -t`), and htsjdk's setCheckCrcs.  A checker:
 * SBAM_OK when it ran, whether or not blocks mismatch (*totals says).  SBAM_ERR_STATE before a successful
 * sbam_inflate and after sbam_reset, sbam_load or a sbam_reserve that dropped the stages (the results belong to the
 * stream stage and go with it; sbam_reserve does not size their buffers); SBAM_ERR_ARG for a range outside the table;
 * b0 == b1 is valid and gives zero totals. */
int sbam_check_crc(sbam_ctx *ctx, int64_t b0, int64_t b1, sbam_crc_totals *totals);

/* Copy the computed and stored CRC32s of blocks [b0, b0 + n) from the last sbam_check_crc (either pointer may be
 * NULL).  Blocks outside the range it checked, or no check since the stream was made: SBAM_ERR_STATE.  (No reference
 * counterpart, as above: Stream.scala:49-54; htslib's bgzf check compares the same two values per block.) */
int sbam_get_block_crcs(sbam_ctx *ctx, int64_t b0, int64_t n, uint32_t *computed, uint32_t *stored);

/* on != 0: every later sbam_inflate checks the whole table after a successful inflate and fails with SBAM_ERR_CRC
 * ("CRC32 mismatch in block at <file offset>: footer <%08x>, computed <%08x>") on the first block that mismatches,
 * leaving the stream stage unset as after SBAM_ERR_INFLATE.  Sticky across sbam_reset and sbam_load; default off.
 * (No reference counterpart: Stream.scala:49-54 never reads the CRC; this is htslib's bgzf check, htsjdk's
 * setCheckCrcs(true).) */
int sbam_set_verify_crc(sbam_ctx *ctx, int32_t on);

/* Copy uncompressed bytes [off, off+len) of the stream to the host. */
int sbam_read_uncompressed(sbam_ctx *ctx, int64_t off, int64_t len, uint8_t *out);

/* Pos <-> flat uncompressed offset (UncompressedBytes.scala:17-19,65-78). */
int sbam_pos_to_offset(sbam_ctx *ctx, sbam_pos pos, int64_t *offset);
int sbam_offset_to_pos(sbam_ctx *ctx, int64_t offset, sbam_pos *pos);

/* ---- BAM header (check/.../bam/header/Header.scala:26-60; ContigLengths.scala:33-55) ---------- */

/* n_ref and contig lengths (cap entries), end_pos = Header.endPos.  Must follow sbam_inflate on a
 * whole file; a shard takes them from sbam_set_contig_lengths (the broadcast in CanLoadBam.scala:179-180).
 * Any int64 length is valid: the checkers compare refPos > length as the reference does on a Long
 * (PosChecker.scala:59), also for lengths below 0 or above INT32_MAX. */
int sbam_header(sbam_ctx *ctx, int32_t *n_ref, int64_t *lengths, int32_t cap, sbam_pos *end_pos);
int sbam_set_contig_lengths(sbam_ctx *ctx, int32_t n_ref, const int64_t *lengths);

/* ---- record-boundary checkers --------------------------------------------------------------- */

/* Shards.  A context opened with base_offset + len < file_size holds a stream that ends (at L) before the file does.
 * There every function below answers what the whole file would answer, or HALO: a position, search or chain that
 * needed a byte at or past L (a record's fixed bytes, name or CIGAR ops, or a hop offset + 4 + block_size > L) is
 * unknown, never decided from the bytes at hand.  HALO is SBAM_WORD_HALO in the words, n_halo / SBAM_ERR_HALO from the
 * counts (the other fields are the reductions over the decided positions), and SBAM_ERR_HALO from the record search
 * and the split functions.  The caller loads a longer range and asks again; no other error asks for that. */

/* eager.Checker at every uncompressed offset in [x0, x1) (check/.../check/eager/Checker.scala:24-126):
 * bit i of bitmap (LSB-first within uint64 words) = call at x0+i.  bitmap may be NULL (device-only).
 * On a shard the bit of an unknown position is 0, like a failure's, and the call still returns SBAM_OK; the context
 * remembers the smallest unknown position and lets the bitmap stand for [x0, that position) only, so that
 * sbam_find_record_start and the split functions decide the rest themselves (and answer HALO there). */
int sbam_check_eager(sbam_ctx *ctx, int64_t x0, int64_t x1, int32_t reads_to_check, uint64_t *bitmap);

/* full.Checker result words for [x0, x1) (check/.../check/full/Checker.scala:22-184). */
int sbam_check_full_words(sbam_ctx *ctx, int64_t x0, int64_t x1, int32_t reads_to_check, uint32_t *words);

/* full.Checker over [x0, x1) reduced to full-check Counts + success bitmap (device-resident; copied
 * to success_bitmap when non-NULL).  Replaces the per-position RDD + reduceByKey of FullCheck.scala:117-191.
 * by_key = 0 fills what the full-check report prints (totals, keys 1-2 per flag, positions per key, close-call
 * pairs, readsBeforeError); by_key = 1 also fills counts[k][f] for every key (negativesByNumNonzeroFields). */
int sbam_check_full_counts(sbam_ctx *ctx, int64_t x0, int64_t x1, int32_t reads_to_check, int32_t by_key,
                           sbam_counts *counts, uint64_t *success_bitmap);

/* FindRecordStart.withDelta (check/.../bam/spark/FindRecordStart.scala:30-63) from Pos(block_start, 0):
 * *found = 0 means None.  On a shard: the first position, in order, that is Success or unknown decides; unknown, or
 * reaching the stream's end with attempts left, is SBAM_ERR_HALO. */
int sbam_find_record_start(sbam_ctx *ctx, int64_t block_start, int32_t reads_to_check, int32_t max_read_size,
                           int32_t *found, sbam_pos *pos, int32_t *delta);

/* ---- splits and records (load/.../spark/load/CanLoadBam.scala:173-334) ----------------------- */

typedef struct {
  int64_t split_size;         /* MaxSplitSize (hadoop FileSplits max split size)  */
  int32_t bgzf_blocks_to_check; /* default 5  (bgzf/.../block/package.scala:20-21) */
  int32_t reads_to_check;     /* default 10 (check/.../check/package.scala:17-18)  */
  int32_t max_read_size;      /* default 10_000_000 (check/.../check/package.scala:28-29) */
  int32_t use_success_bitmap; /* 1: reuse the bitmap of a preceding sbam_check_full_counts over the stream */
} sbam_split_args;

/* Hadoop FileSplits of the whole file (FileInputFormat rule, SPLIT_SLOP 1.1): n_out splits [start, end). */
int sbam_file_splits(int64_t file_size, int64_t split_size, int64_t *starts, int64_t *ends, int64_t cap,
                     int64_t *n_out);

/* For Hadoop splits [first, first+count) of the file: FindBlockStart → FindRecordStart → record chain
 * with Pos < (end, 0).  Writes each split's first-record position (found[i]=0 when the split is empty or
 * past the shard) and record count (= the partition size of loadReads / loadReadsAndPositions).
 * On a shard SBAM_ERR_HALO when a first-record search or a chain needed bytes past the stream's end, or when no
 * loaded block starts at or past a split's end and the loaded blocks end before it. */
int sbam_split_records(sbam_ctx *ctx, const sbam_split_args *args, int64_t first, int64_t count, sbam_pos *first_pos,
                       int32_t *found, int64_t *n_records);

/* loadSplitsAndReads' splits for the whole file (CanLoadBam.scala:245-279): first positions of the non-empty
 * partitions paired by sliding2(Pos(fileSize, 0)). */
int sbam_compute_splits(sbam_ctx *ctx, const sbam_split_args *args, sbam_split *splits, int64_t cap, int64_t *n_out);

/* Record chain from flat offset x0 while offset < x_end (RecordStream.scala:27-41): record start offsets
 * (cap entries) and *n_out records; record bytes are stream[off, off+4+block_size). */
int sbam_record_offsets(sbam_ctx *ctx, int64_t x0, int64_t x_end, int64_t *offsets, int64_t cap, int64_t *n_out);

/* Reference spans of the records at the n stream offsets (loadBamIntervals' region filter, CanLoadBam.scala:
 * 107-135, 423-431): ref_id, start = POS (0-based) and end = POS + the CIGAR's reference length (M/D/N/=/X),
 * i.e. [getStart - 1, getEnd); unmapped records (flag 4) get end = 0, htsjdk's getAlignmentEnd. */
int sbam_record_spans(sbam_ctx *ctx, const int64_t *offsets, int64_t n, int32_t *ref_id, int32_t *start, int32_t *end);

/* ---- record decode: loadReads / loadReadsAndPositions (CanLoadBam.scala:221-241, 281-334) ------------- */

/* Per-record columns: the record's flat stream offset, its Pos, and the BAM fixed fields (SAM spec §4.2, the
 * part htsjdk BAMRecordCodec.decode reads eagerly: RecordStream.scala:16-33).  Record bytes are
 * stream[offset, offset + 4 + block_size) (sbam_read_uncompressed).  Any pointer may be NULL (not copied). */
typedef struct {
  int64_t *offset;
  int64_t *block_pos;   /* Pos.blockPos */
  int32_t *block_off;   /* Pos.offset   */
  int32_t *block_size;
  int32_t *ref_id;
  int32_t *pos;
  uint32_t *bin_mq_nl;  /* bin << 16 | MAPQ << 8 | l_read_name */
  uint32_t *flag_nc;    /* FLAG << 16 | n_cigar_op */
  int32_t *l_seq;
  int32_t *next_ref_id;
  int32_t *next_pos;
  int32_t *tlen;
} sbam_record_columns;

/* Records of Hadoop splits [first, first+count) — the partitions of loadReadsAndPositions, in split order —
 * decoded into device-resident columns owned by ctx (valid until the next load, reset or close).
 * split_counts[count] (may be NULL) receives the partition sizes, *n_records their sum.  With
 * use_success_bitmap and a preceding full check over the range, the chains are proven equal to the checker's
 * success bitmap and listed in parallel; otherwise (or when the proof fails) each split's chain is walked. */
int sbam_load_records(sbam_ctx *ctx, const sbam_split_args *args, int64_t first, int64_t count, int64_t *split_counts,
                      int64_t *n_records);

/* Which way the last sbam_split_records / sbam_compute_splits / sbam_load_records took to its record counts
 * (read-only; no reference counterpart: RecordStream only ever walks):
 *   *tried             1 when a success bitmap covered the splits and use_success_bitmap asked for it;
 *   *proved            1 when the chain proof held and the counts (and record lists) came from the bitmap, 0 when the
 *                      chains were walked;
 *   *missing_links,    the list-form chain pass's counters for the check that left that bitmap: PASS0 positions whose
 *   *failed_fallbacks  hop is not the next PASS0 position, and fallback walks that failed.  -1 when the bitmap was not
 *                      tried or not list-form, or when a later check ran before this call asked for them.
 * Any pointer may be NULL. */
int sbam_records_path(sbam_ctx *ctx, int32_t *tried, int32_t *proved, int64_t *missing_links,
                      int64_t *failed_fallbacks);

/* Copy records [i0, i0+n) of the last sbam_load_records into caller-owned host columns. */
int sbam_get_record_columns(sbam_ctx *ctx, int64_t i0, int64_t n, const sbam_record_columns *out);

/* Device pointers of the last sbam_load_records' columns (for in-process GPU consumers; no copy). */
int sbam_record_columns_device(sbam_ctx *ctx, sbam_record_columns *dev, int64_t *n_records);

/* ---- variable-length fields: the rest of the SAMRecord (SAM spec §4.2) ------------------------------------ */

/* Field mask of sbam_load_record_fields. */
#define SBAM_FIELD_NAME 1u
#define SBAM_FIELD_CIGAR 2u
#define SBAM_FIELD_SEQ 4u
#define SBAM_FIELD_QUAL 8u
#define SBAM_FIELD_AUX 16u

/* CSR columns of a batch of n records: every *_off has n + 1 int64 entries (exclusive prefix sums, [n] = total).
 *   name   read_name bytes without the trailing NUL (l_read_name - 1; 0 when l_read_name <= 1)   name_off
 *   cigar  the raw uint32 ops (len << 4 | op)                                                    cigar_off (in ops)
 *   seq    one ASCII byte per base, "=ACMGRSVTWYHKDBN"[nibble], high nibble first                 seq_off
 *   qual   the raw phred bytes (0xFF kept as is)                                                 seq_off (shared)
 *   aux    the raw tag bytes from the end of qual to offset + 4 + block_size                     aux_off */
typedef struct {
  int64_t *name_off;
  uint8_t *name;
  int64_t *cigar_off;
  uint32_t *cigar;
  int64_t *seq_off;
  uint8_t *seq;
  uint8_t *qual;
  int64_t *aux_off;
  uint8_t *aux;
} sbam_record_fields;

typedef struct {
  int64_t name_bytes;
  int64_t cigar_ops;
  int64_t seq_bases;
  int64_t aux_bytes;
} sbam_record_field_totals;

/* Decode the variable-length fields selected by `fields` (SBAM_FIELD_*) of records [i0, i0 + n) of the last
 * sbam_load_records into device columns owned by ctx (a grow-only arena; valid until the next call, load, reset or
 * close): what htsjdk BAMRecordCodec.decode reads behind RecordStream.scala:16-33 (SAM spec §4.2: read_name, cigar,
 * seq, qual, tags), for the SAMRecords of loadReads (CanLoadBam.scala:221-241, 348-352).  The batch bounds the memory:
 * the decoded columns of a whole file are about 1.3x its uncompressed size.  All four offset columns are always
 * produced; *totals (may be NULL) receives their last entries.  A record whose l_seq is negative, whose fields need
 * more than block_size bytes, or that ends past the stream is SBAM_ERR_RECORD with error.position = its stream
 * offset (the first such record of the batch; nothing is decoded).  SBAM_ERR_STATE without loaded records,
 * SBAM_ERR_ARG for a range outside them or an empty or unknown mask; n = 0 is SBAM_OK with zero totals. */
int sbam_load_record_fields(sbam_ctx *ctx, int64_t i0, int64_t n, uint32_t fields, sbam_record_field_totals *totals);

/* Copy the columns of the last sbam_load_record_fields into caller-owned host buffers sized from its totals (the
 * SAMRecord accessors getReadName / getCigar / getReadBases / getBaseQualities / getAttributes of BAMRecordCodec.decode,
 * SAM spec §4.2).  NULL members are not copied; a data member of a field that was not selected is SBAM_ERR_ARG. */
int sbam_get_record_fields(sbam_ctx *ctx, const sbam_record_fields *out);

/* Device pointers of the last sbam_load_record_fields' columns and its batch (for in-process GPU consumers; no copy;
 * the device-side form of BAMRecordCodec.decode's variable-length part, SAM spec §4.2).  The data pointer of a field
 * that was not selected is NULL. */
int sbam_record_fields_device(sbam_ctx *ctx, sbam_record_fields *dev, int64_t *i0, int64_t *n);

/* ---- typed tags: SAMRecord.getAttribute (SAM spec §4.2.4) -------------------------------------------------- */

#define SBAM_MAX_TAGS 32

/* One entry of a tag query: the two-character name, and whether the value's bytes are wanted as a CSR column. */
typedef struct {
  char tag[2];
  uint8_t want_bytes;
  uint8_t reserved;
} sbam_tag_query;

/* Columns of a batch of n records and a query of n_tags entries, tag-major: entry j, record k at index j * n + k.
 *   type   the stored type byte, one of A c C s S i I f Z H B; 0 when the record has no such tag
 *   sub    a B array's element type; 0 otherwise
 *   rel    offset of the value's first byte inside the record's tag bytes (sbam_load_record_fields' aux column:
 *          aux[aux_off[k] + rel]); Z and H: the first character; B: the first element, behind subtype and count;
 *          -1 when absent
 *   value  c s i sign-extended, C S I zero-extended, A the byte, f the 32 IEEE bits zero-extended, Z and H the length
 *          in bytes without the NUL, B the element count; 0 when absent
 * and for every entry j with want_bytes a CSR column: bytes_off[j] (n + 1 int64, exclusive prefix sums) and bytes[j],
 * holding a Z or H value's characters without the NUL, a B array's raw little-endian element bytes, and nothing for
 * scalar types and absent tags.  Entries of bytes_off / bytes whose query entry has no want_bytes (or j >= n_tags)
 * are NULL. */
typedef struct {
  uint8_t *type;
  uint8_t *sub;
  int32_t *rel;
  int64_t *value;
  int64_t *bytes_off[SBAM_MAX_TAGS];
  uint8_t *bytes[SBAM_MAX_TAGS];
} sbam_record_tags;

typedef struct {
  int64_t present[SBAM_MAX_TAGS]; /* records of the batch that have the tag */
  int64_t bytes[SBAM_MAX_TAGS];   /* the entry's CSR total (0 without want_bytes) */
} sbam_record_tag_totals;

/* Decode the tags named by q[0 .. n_tags) of records [i0, i0 + n) of the last sbam_load_records into device columns
 * owned by ctx: what htsjdk SAMRecord.getAttribute(tag) answers for the SAMRecords BAMRecordCodec.decode builds behind
 * RecordStream.scala:16-33, i.e. those of loadReads (CanLoadBam.scala:221-241); tag layout SAM spec §4.2.4.  The tag
 * bytes are read straight from the inflated stream; no sbam_load_record_fields is needed.  Rules:
 *   whole list   a record's whole tag list is always walked and validated, whatever is queried, so whether a batch is
 *                well-formed does not depend on the query;
 *   duplicates   the first occurrence of a tag in a record wins;
 *   malformed    SBAM_ERR_RECORD with error.position = the stream offset of the first such record of the batch, and
 *                nothing is produced, for: fewer than 3 bytes left for a tag header; an unknown type byte; a value
 *                that runs past the record's end; a Z or H value with no NUL before the record's end; a B array with
 *                an unknown subtype, a negative count, or elements past the end; and the structural failures
 *                sbam_load_record_fields reports (a negative l_seq, fields past block_size, a record past the stream);
 *   state        SBAM_ERR_STATE without loaded records;
 *   arguments    SBAM_ERR_ARG for a range outside the loaded records, n_tags outside 1..SBAM_MAX_TAGS, a tag that is
 *                not [A-Za-z][A-Za-z0-9], or the same tag twice in the query;
 *   empty batch  n = 0 is SBAM_OK with zero totals;
 *   lifetime     the columns live in buffers of their own (grow-only, sized by one rule) and stay valid until the next
 *                sbam_load_record_tags, load, reset or close; a later sbam_load_record_fields does not invalidate
 *                them, nor the reverse;
 *   timing       sbam_last_kernel_ms(ctx, "record_tags") is the device time of the call.
 * *totals (may be NULL) receives the per-entry counts. */
int sbam_load_record_tags(sbam_ctx *ctx, int64_t i0, int64_t n, const sbam_tag_query *q, int32_t n_tags,
                          sbam_record_tag_totals *totals);

/* Copy the columns of the last sbam_load_record_tags into caller-owned host buffers (type, sub, rel, value: n_tags * n
 * entries; bytes_off[j]: n + 1; bytes[j]: its total): the host form of SAMRecord.getAttribute over the batch
 * (BAMRecordCodec.decode behind RecordStream.scala:16-33; SAM spec §4.2.4).  NULL members are not copied; a bytes_off
 * or bytes member of an entry without want_bytes is SBAM_ERR_ARG. */
int sbam_get_record_tags(sbam_ctx *ctx, const sbam_record_tags *out);

/* Device pointers of the last sbam_load_record_tags' columns, its batch and its query size (for in-process GPU
 * consumers; no copy; the device-side form of SAMRecord.getAttribute, SAM spec §4.2.4, CanLoadBam.scala:221-241). */
int sbam_record_tags_device(sbam_ctx *ctx, sbam_record_tags *dev, int64_t *i0, int64_t *n, int32_t *n_tags);

/* Tag bytes above which sbam_load_record_tags walks one record with a whole wave (SAM spec §4.2.4; no reference
 * counterpart, htsjdk's BAMRecordCodec.decode is sequential): for tests that must reach that path. */
int sbam_tag_long_aux_bytes(void);

/* ---- BAI index writer (SAM spec §5.2, §5.3; the layout the reference reads in check/.../bam/index/Index.scala:53-90) -- */

/* The index is built from the record columns of the last sbam_load_records, in file order, by these rules (the usual
 * samtools/htslib writer's; pinned by the reference's 2.bam.bai and 5k.bam.bai):
 *   span    beg = max(pos, 0); end = pos + the CIGAR's reference length (M, D, N, =, X) for a mapped record (flag 4
 *           clear) with a positive one, else beg + 1; bin = reg2bin(beg, end) (14-bit minimum shift, 5 levels),
 *           computed, never the record's own bin field;
 *   run     a maximal stretch of consecutive records with ref_id >= 0 and the same (ref_id, bin): one chunk
 *           [virtual offset of its first record, virtual offset behind its last); a record with ref_id < 0 breaks a run;
 *   linear  ioffset[ref][w] = the smallest record start over the records touching 16 kb window w; an untouched window
 *           takes the next touched one's value (filled from the end);
 *   meta    per reference: smallest start, largest end, mapped and unmapped (flag 4) records; n_no_coor = records with
 *           ref_id < 0; n_unsorted = records whose ((uint32) ref_id, pos) is below their predecessor's.
 * The .bai bytes list a reference's bins in ascending bin number, the metadata pseudo-bin 37450 last (a reader must
 * not rely on an order: the reference's fixtures list theirs in hash-table order). */
typedef struct {
  int32_t n_ref;
  int32_t reserved;
  int64_t n_runs;        /* entries of sbam_get_index_runs */
  int64_t n_intv_total;  /* entries of sbam_get_index_refs' ioffset */
  int64_t n_no_coor;
  int64_t n_unsorted;
  int64_t n_records;
} sbam_index_totals;

/* Build the index of the whole file on the GPU (SAM spec §5.2; reader: check/.../bam/index/Index.scala:53-90).  Needs a
 * whole-file context (base_offset 0, file_size == len), known contig lengths, and a preceding sbam_load_records over
 * every split (first = 0 through the last; a file that ends behind its header needs none); else SBAM_ERR_STATE.
 * A record with ref_id >= n_ref, a reference end past 2^29, or CIGAR ops past its block_size or the stream end is
 * SBAM_ERR_RECORD with error.position = the stream offset of the first such record; nothing is produced.  The results
 * live on the device, owned by ctx (grow-only buffers sized by one rule; sbam_reserve serves streamed windows and does
 * not size them), until the next load, reset or close. */
int sbam_build_index(sbam_ctx *ctx, sbam_index_totals *totals);

/* The raw runs of the last sbam_build_index in file order, n_runs entries each (SAM spec §5.2 chunks before binning;
 * Index.scala:53-57 Chunk).  A NULL member is not copied. */
int sbam_get_index_runs(sbam_ctx *ctx, int32_t *ref, uint32_t *bin, uint64_t *beg, uint64_t *end);

/* The linear index after the fill and the per-reference metadata of the last sbam_build_index (SAM spec §5.2 ioffset
 * and the pseudo-bin 37450; Index.scala:60-90): intv_off has n_ref + 1 entries, reference r's windows are
 * ioffset[intv_off[r] .. intv_off[r + 1]); the other members have n_ref entries (off_beg of a reference without records
 * is UINT64_MAX).  A NULL member is not copied. */
int sbam_get_index_refs(sbam_ctx *ctx, int64_t *intv_off, uint64_t *ioffset, uint64_t *off_beg, uint64_t *off_end,
                        int64_t *n_mapped, int64_t *n_unmapped);

/* Runs, linear index and metadata -> .bai bytes (SAM spec §5.2; what Index.scala:60-90 parses).  Host only: no context,
 * no device.  Per reference: group the runs by bin in file order; for level 5 down to 1, every present bin in ascending
 * number (below level 5 its chunks sorted first) whose (last chunk's end >> 16) - (first chunk's beg >> 16) < 0x10000
 * and whose parent (bin - 1) >> 3 exists is appended to the parent and deleted; bin 0 is sorted; every bin's chunks are
 * coalesced in order (c joins the kept chunk m when m.end >> 16 >= c.beg >> 16); pseudo-bin 37450 holds
 * (off_beg, off_end) and (n_mapped, n_unmapped).  A reference with no records has n_bin = 0 and n_intv = 0.  ioffset
 * entries equal to UINT64_MAX count as untouched and are filled from the end.  *n_bytes receives the size; when cap is
 * smaller nothing is written and the result is SBAM_ERR_ARG. */
int sbam_bai_assemble(int32_t n_ref, int64_t n_runs, const int32_t *run_ref, const uint32_t *run_bin,
                      const uint64_t *run_beg, const uint64_t *run_end, const int64_t *intv_off,
                      const uint64_t *ioffset, const uint64_t *off_beg, const uint64_t *off_end,
                      const int64_t *n_mapped, const int64_t *n_unmapped, int64_t n_no_coor, uint8_t *out, int64_t cap,
                      int64_t *n_bytes);

/* sbam_bai_assemble over the last sbam_build_index (SAM spec §5.2; Index.scala:60-90 reads these bytes back): the file
 * a JVM caller stores beside the BAM as <name>.bam.bai.  cap too small: SBAM_ERR_ARG, *n_bytes = the size needed. */
int sbam_write_bai(sbam_ctx *ctx, uint8_t *out, int64_t cap, int64_t *n_bytes);

/* CIGAR ops above which sbam_build_index sums a record's reference length with a whole wave (SAM spec §4.2 n_cigar_op;
 * no reference counterpart, Index.scala:53-90 only reads): for tests that must reach that path. */
int sbam_index_long_cigar_ops(void);

/* ---- Coordinate sort of the loaded records (no reference counterpart: the reference never reorders records; the
 * behaviour mirrored is htsjdk's SAMFileWriterFactory with SortOrder.coordinate behind HTSJDKRewrite.scala:52-76, and
 * `samtools sort`) ------------------------------------------------------------------------------------------------
 * The key of loaded record r is the 64-bit unsigned word
 *   (uint64_t)(uint32_t)ref_id[r] << 32 | (uint32_t)(pos[r] ^ 0x80000000):
 * references ascend as unsigned, so ref_id == -1 (no coordinate) sorts last; within a reference pos ascends as signed,
 * so -1 sorts first.  Records with equal keys keep their loaded (file) order: the sort is stable, and the order a
 * function of the two columns alone.  This is the order sbam_build_index's n_unsorted tests and the one htsjdk and
 * samtools accept as SO:coordinate; it is not `samtools sort`'s tie order, which adds the strand bit.  Queryname and
 * tag orders, and merging sorted runs of a file larger than device memory, are not built. */
typedef struct {
  int64_t n_records;       /* records sorted (the loaded ones) */
  int64_t n_out_of_order;  /* before the sort: records whose key is below their predecessor's; 0: order = identity */
  int32_t passes;          /* radix passes that ran, 0..8 */
  int32_t reserved;
} sbam_sort_totals;

/* Sort the records of the last sbam_load_records by coordinate on the GPU (no reference counterpart; htsjdk
 * SortOrder.coordinate): an LSD radix sort of (key, index) pairs by bytes; a byte that is the same in every key costs no
 * pass, and an input already in order none at all.  SBAM_ERR_STATE without loaded records; no records is SBAM_OK;
 * 2^32 records or more: SBAM_ERR_ARG.  The order lives on the device, owned by ctx (grow-only buffers sized by one rule:
 * 32 bytes per record and 8 per 2048-key tile and digit; sbam_reserve serves streamed windows and does not size them),
 * until the next sbam_sort_records, sbam_load_records, load, reset or close; fields, tags, an index or a write do not
 * invalidate it.  sbam_last_kernel_ms: "sort_keys" (keys and histograms), "sort" (the whole call). */
int sbam_sort_records(sbam_ctx *ctx, sbam_sort_totals *totals);
/* Entries [i0, i0 + n) of the last sort's order into a host buffer: order[k] = loaded index of the k-th record in
 * coordinate order (no reference counterpart; what htsjdk's coordinate-sorting writer emits k-th). */
int sbam_get_sort_order(sbam_ctx *ctx, int64_t i0, int64_t n, int64_t *order);
/* The same column on the device, *n entries (no reference counterpart; for in-process GPU consumers; no copy). */
int sbam_sort_order_device(sbam_ctx *ctx, const int64_t **order, int64_t *n);
/* Keys per workgroup tile of the sort's passes, a build constant (no reference counterpart): for tests that must reach
 * the tile's edges and more tiles than one workgroup of the scan covers. */
int sbam_sort_tile_keys(void);

/* ---- BAM writer: records of the last sbam_load_records -> BGZF bytes on the device ------------------------------
 * htsjdk-rewrite (cli/src/main/scala/org/hammerlab/bam/rewrite/HTSJDKRewrite.scala:21-91): the BAM header, then the
 * selected records back to back, cut every block_bytes uncompressed bytes (htsjdk's 65498), each piece deflated and
 * framed as a BGZF block, the 28-byte EOF block last.  The uncompressed side equals the reference writer's byte for
 * byte; the compressed bytes are this library's own (level 0: stored blocks; level 1: LZ77 + the fixed Huffman code,
 * with a stored block wherever that would be smaller; level 1 | SBAM_WRITE_DYNAMIC: the same LZ77 tokens, and per block
 * the smallest of the stored form, the fixed code and a dynamic Huffman code built from the block's own counts, ties
 * to the earlier).  Deterministic: the output is a function of the input bytes and the arguments alone, whatever the
 * device's scheduling. */
#define SBAM_WRITE_DYNAMIC 0x100   /* OR into level 1: per block, the smallest of stored, fixed and dynamic Huffman */
typedef struct {
  const int64_t *range_lo;   /* host: record-index ranges [lo, hi) into the last sbam_load_records (HTSJDKRewrite.scala's */
  const int64_t *range_hi;   /* -r read-index ranges), ascending and disjoint                                         */
  int64_t n_ranges;          /* 0: every record                                                                       */
  const uint8_t *keep_device;/* optional device byte per loaded record; nonzero = keep; ANDed with the ranges         */
  int32_t level;             /* 0 stored, 1 LZ77 + fixed Huffman, 1 | SBAM_WRITE_DYNAMIC; anything else: SBAM_ERR_ARG */
  int32_t block_bytes;       /* uncompressed bytes per block, 1..65498; 0 = 65498                                     */
  int32_t with_header;       /* 1: the BAM header (stream bytes [0, header end)) goes first; needs a context that
                                starts at file offset 0 and has read its header (sbam_header)                         */
  int32_t with_eof;          /* 1: append the 28-byte EOF block                                                       */
} sbam_write_args;
typedef struct {
  int64_t n_records;        /* records written */
  int64_t header_bytes;     /* 0 without with_header */
  int64_t ubytes;           /* uncompressed bytes written: header_bytes + the records' 4 + block_size */
  int64_t n_blocks;         /* data blocks (the EOF block is not counted) */
  int64_t n_stored_blocks;  /* of them in the stored form */
  int64_t comp_bytes;       /* bytes of the file, the EOF block included */
} sbam_write_totals;

/* Write the selected records (HTSJDKRewrite.scala:52-76: header, then every read inside the ranges).  with_header = 0
 * and with_eof = 0 exist so that the outputs of a file's shards concatenate into one valid BAM.  SBAM_ERR_STATE: no
 * sbam_load_records has run, or with_header on a context that does not start at offset 0 (or whose header has not been
 * read); SBAM_ERR_ARG: ranges out of order, overlapping or past the loaded records, level not 0, 1 or
 * 1 | SBAM_WRITE_DYNAMIC, block_bytes outside 0..65498.  The file bytes, the block table and the records' positions
 * stay on the device, owned by ctx (grow-only buffers: the stream at its size; the file at its stored bound of
 * ubytes + 31 per block + 28, which no form of a block exceeds; the deflate slots at one batch of at most 4096 blocks,
 * block_bytes + 13 rounded up to 16 each; with SBAM_WRITE_DYNAMIC the token records, one per resident wavefront, at
 * most 1024, of two bytes per block byte + 2 rounded up to 16), until the next sbam_write_bam, load, reset or close. */
int sbam_write_bam(sbam_ctx *ctx, const sbam_write_args *args, sbam_write_totals *totals);
typedef struct {
  const int64_t *order_device; /* device, n_loaded entries: entry k of the output is loaded record order_device[k];
                                  NULL: the order of the last sbam_sort_records (SBAM_ERR_STATE when there is none) */
  const uint8_t *header;       /* host, optional: a complete BAM header (magic .. last reference) written instead of the
                                  stream's; only with with_header = 1, and then the context need not start at offset 0 */
  int64_t header_bytes;
} sbam_write_order;
/* sbam_write_bam with one indirection in its select step (no reference counterpart; htsjdk's SAMFileWriterFactory with
 * SortOrder.coordinate behind HTSJDKRewrite.scala:52-76, and `samtools sort`, when the order is a sort's).  args->range_*
 * and keep_device still index the loaded records: a record is written when its own index is selected, and the order
 * only decides the sequence.  ord == NULL: sbam_write_bam.  Checked before anything is written: every order_device entry
 * lies in [0, n_loaded), on the device, else SBAM_ERR_ARG (the previous written bytes are gone, as after any failed
 * write); a repeated entry is no error: that record is written twice.  The override header is checked on the host:
 * the magic, and l_text, n_ref and the names' lengths must add up to exactly header_bytes, else SBAM_ERR_ARG; so is a
 * header with with_header = 0, header_bytes without a header, or a header longer than the context's uncompressed
 * stream + 16368 bytes.  Totals, buffers and the getters below as for sbam_write_bam. */
int sbam_write_bam_ordered(sbam_ctx *ctx, const sbam_write_args *args, const sbam_write_order *ord,
                           sbam_write_totals *totals);
/* The file bytes of the last sbam_write_bam (what HTSJDKRewrite.scala:52-76 leaves at its output path); cap smaller
 * than comp_bytes: SBAM_ERR_ARG. */
int sbam_get_written(sbam_ctx *ctx, uint8_t *out, int64_t cap);
/* The same bytes on the device (HTSJDKRewrite.scala:52-76): *dev stays valid until the next write, load or close. */
int sbam_written_device(sbam_ctx *ctx, const uint8_t **dev, int64_t *n);
/* The written data blocks (HTSJDKRewrite.scala:78-83 -b, the .blocks sidecar's start, compressed size, uncompressed
 * size), n_blocks entries each.  A NULL member is not copied. */
int sbam_get_written_blocks(sbam_ctx *ctx, int64_t *start, int32_t *csize, int32_t *usize);
/* Pos of every written record in the new file (HTSJDKRewrite.scala:85-90 -i, the .records sidecar), n_records entries
 * each, in writing order. */
int sbam_get_written_records(sbam_ctx *ctx, int64_t *block_pos, int32_t *block_off);

/* ---- for tests: the writer's deflate and framing over arbitrary bytes (HTSJDKRewrite.scala:52-76's
 * BlockCompressedOutputStream half; no context: the call allocates its device buffers, runs on a stream of its own,
 * copies back and frees).  in[0, n) is cut every block_bytes (0 = 65498); out receives the BGZF bytes, *n_out their
 * count (cap too small: SBAM_ERR_ARG with *n_out set), *n_stored_blocks (may be NULL) the blocks in the stored form.
 * level as sbam_write_args.level: 0, 1 or 1 | SBAM_WRITE_DYNAMIC, else SBAM_ERR_ARG; the same bytes as sbam_write_bam
 * gives for the same stream, a function of in, block_bytes, level and with_eof alone; the buffers sized by the same
 * rule (the file ubytes + 31 per block + 28, slots and token records per batch). */
int sbam_test_deflate(int device, const uint8_t *in, int64_t n, int32_t block_bytes, int32_t level, int32_t with_eof,
                      uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_stored_blocks);

/* ---- for tests: the coordinate sort over arbitrary keys (no reference counterpart; no context: the call allocates
 * its device buffers, runs on a stream of its own, copies back and frees): order receives the stable order of the n
 * keys (order[k] = index of the k-th smallest, ties by index), *passes the radix passes that ran. */
int sbam_test_sort_keys(int device, const uint64_t *keys, int64_t n, int64_t *order, int32_t *passes);

/* ---- for tests: the library's prefix-sum primitives (no reference counterpart; no context: each call allocates its
 * device buffers, runs on a stream of its own, copies back and frees) ------------------------------------------- */
/* The in-place exclusive scan behind every offsets column (SAM spec §4.2's variable-length fields as CSR offsets):
 * in holds cols columns of n values; out receives cols columns of n + 1: the exclusive prefix sums and the total. */
int sbam_test_exclusive_scan(int device, const int64_t *in, int64_t n, int32_t cols, int64_t *out);
/* One workgroup's scan of n per-workgroup sums (the step between the passes of a device-wide scan; BGZF chunk counts,
 * MetadataStream.scala:23-54): out receives n exclusive prefix sums as int64 and, at [n], the total. */
int sbam_test_scan_sums_int(int device, const int32_t *in, int64_t n, int64_t *out);
/* The record-chain proof, the split popcounts and the split offsets (RecordStream.scala:27-41 read off a success
 * bitmap) on inputs of the caller's: a stream u of L bytes (copied with the library's zero pad behind it), a bitmap of
 * n_words words whose bit 0 is stream offset xa (a multiple of 64), the proof range [X0, X1) and n_splits chains
 * [xs[i], xe[i]) (xs < 0 or xs >= xe: an empty split), all inside the bitmap (else SBAM_ERR_ARG).  list / exact (both
 * or neither): an ascending PASS0 list of n_list offsets and the chain pass's three counter words.  fail[0] receives
 * the proof's flag, fail[1] the popcounts' (a split whose first offset is not a set bit); counts[n_splits] the record
 * counts, *n_offsets their sum, and offsets (cap entries) the set bits of every split at the exclusive scan of the
 * counts. */
int sbam_test_chain_proof(int device, const uint8_t *u, int64_t L, const uint64_t *bm, int64_t n_words, int64_t xa,
                          int64_t X0, int64_t X1, const int64_t *xs, const int64_t *xe, int64_t n_splits,
                          const int64_t *list, int64_t n_list, const uint64_t *exact, int32_t *fail, int64_t *counts,
                          int64_t *offsets, int64_t cap, int64_t *n_offsets);

/* ---- timing support for bench/profiling -------------------------------------------------------- */
/* Device time (ms, HIP events on the library's stream) of the most recent launch of a named kernel
 * family: "scan", "inflate", "check_full", "check_eager", "records", "load_records", "record_fields" (the gather of
 * sbam_load_record_fields; "record_field_sizes": its sizes and scan), "index" (sbam_build_index, from its first pass
 * through the linear index's fill), "crc" (the block CRC32 check), "record_tags" (sbam_load_record_tags: its walk and
 * scans, "record_tag_walk", plus the gather of its byte columns, "record_tag_bytes"), "write_select", "write_gather",
 * "write_deflate", "write_frame" (sbam_write_bam's stages; deflate and frame: of its last batch of blocks; the deflate
 * stage is one launch at every level, SBAM_WRITE_DYNAMIC's tokens, codes and emit included), "sort_keys" and "sort"
 * (sbam_sort_records: its keys and histograms; the whole call). Returns -1 if none. */
double sbam_last_kernel_ms(sbam_ctx *ctx, const char *kernel);

#ifdef __cplusplus
}
#endif
#endif /* SBAM_H */
