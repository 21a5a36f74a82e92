// sbam_internal.h — launch wrappers shared by the kernels (sbam_*.hip) and the C-ABI host
// layer (sbam_api.cpp).  Not part of the public ABI (include/sbam.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>

namespace sbam {

// One BGZF header candidate found by the byte scan (Header.make, bgzf/.../block/Header.scala:48-83).
struct Candidate {
  int64_t pos;    // offset in the loaded buffer
  int32_t hsize;  // 18 + XLEN - 6
  int32_t csize;  // BSIZE + 1
  int32_t isize;  // ISIZE (valid when flags & CAND_ISIZE)
  int32_t flags;  // CAND_*
};
enum : int32_t { CAND_ISIZE = 1, CAND_EMPTY = 2 };

// Device view of the BGZF block table (struct of arrays; offsets relative to the loaded buffer).
struct BlockTable {
  const int64_t *start;
  const int32_t *hsize;
  const int32_t *csize;
  const int32_t *usize;
  const int64_t *uoff;
  int64_t n;
};

// The decode -> resolve token pool.  Block b's u16 tokens live in its main region (1 B per uncompressed byte,
// tok_region in sbam_inflate.hip: room for (usize + 16) / 2 tokens) unless base[b] >= 0: then at arena + base[b],
// a region of 2 usize + 32 B taken from the arena by a block that needs more (the exact decoder's blocks, and
// blocks whose wave decode outgrows the main region: they move there).  arena_used counts every request, also
// those past arena_cap (the block then reports INF_OVERFLOW and the host grows the arena and inflates again).
struct TokPool {
  uint8_t *main;
  uint8_t *arena;
  int64_t arena_cap;
  unsigned long long *arena_used;
  int64_t *base;
};

// Stream under check: uncompressed bytes u[0, L) (+ zero pad), contig lengths, EOF semantics.
struct StreamView {
  const uint8_t *u;
  int64_t L;
  const int64_t *lens;  // contig lengths (device)
  int32_t nref;
  int32_t eof_real;  // 1: L is the file's end; 0: a shard, reads past L are HALO
};

struct CountsDev {  // mirrors sbam_counts (int64 fields) in device memory
  unsigned long long *counts;  // [21][19]
  unsigned long long *positions;  // [21]
  unsigned long long *rbe;  // [21][128]
  unsigned long long *pair;  // [19][19]
  unsigned long long *scalars;  // n_positions, n_success, n_too_few_fixed, n_halo
  unsigned long long *totals;   // [19] per-flag totals over every counted position
  // [ntiles][4]: the record-0 pass's PASS0 positions per tile and wave (set only for the full counts that are not
  // by-key, which then write every tile's; the chain pass's chunk counts come from these instead of a second read of the bitmap)
  int32_t *tile_pass0 = nullptr;
  // shards only (StreamView::eof_real == 0; nullptr on a whole file): the smallest position whose call is unknown
  // (HALO), ~0 if none.  Set for the eager check as well, whose other pointers are null: its bitmap says "false" at
  // such a position, so the bitmap covers the range only up to this one (set_bitmap).
  unsigned long long *first_halo = nullptr;
};

// Device columns of decoded records (sbam_records.hip); mirrors sbam_record_columns minus the offsets.
struct RecordColumnsDev {
  int64_t *block_pos;
  int32_t *block_off, *block_size, *ref_id, *pos;
  uint32_t *bin_mq_nl, *flag_nc;
  int32_t *l_seq, *next_ref_id, *next_pos, *tlen;
};

constexpr int kScanChunk = 1 << 20;  // bytes per workgroup in the BGZF candidate scan
constexpr int kScanSlots = 512;      // candidate slots per chunk in the one-pass scan (>= 2 KiB per block)
constexpr int kStreamPad = 16384;  // zero pad behind the uncompressed stream (>= checker LDS window)
constexpr int kCompPad = 256;  // zero pad behind the compressed bytes (bit-reader / input-ring lookahead)

// The block table by following BSIZE hops (sbam_bgzf.hip, section 2): bytes per segment (one wave each) and row slots
// per segment.  The rows share the scan's slot buffer (the scan runs only when the followed table is not accepted),
// so a segment divides a scan chunk and has the same 2 KiB per slot.
#ifndef SBAM_FOLLOW_SEG_LOG2
#define SBAM_FOLLOW_SEG_LOG2 18  // (the sweep: DESIGN.md, Measurement)
#endif
constexpr int kFollowSeg = 1 << SBAM_FOLLOW_SEG_LOG2;
constexpr int kFollowSlots = kFollowSeg / (kScanChunk / kScanSlots);
static_assert(kFollowSeg >= (128 << 10) && kScanChunk % kFollowSeg == 0, "a chain's exit lies in the next segment");
enum : int32_t { FOLLOW_STOP = 1, FOLLOW_PARSE = 2, FOLLOW_OVERFLOW = 4, FOLLOW_NOENTRY = 8 };
struct FollowSegs {  // per segment (sbam_layout.h: follow_segs)
  int64_t *entry, *exit;  // where its chain began (-1: no entry found) and the first position it did not take
  int32_t *rows, *kind;   // blocks on its chain (exact also past the slots); FOLLOW_* (0: left through its far edge)
  int32_t *cnt;           // rows the accepted table takes from it
  int64_t *off;           // their exclusive sums
};
inline int64_t follow_segments(int64_t D, int64_t start_rel) {
  const int64_t n = (D + kFollowSeg - 1) / kFollowSeg - start_rel / kFollowSeg;
  return n > 1 ? n : 1;
}
// follow + link + counts; verdict: two words (first unusable segment, first stopped segment; set here)
hipError_t launch_follow_blocks(const uint8_t *d, int64_t D, int64_t start_rel, int64_t nseg, FollowSegs fs,
                                Candidate *slots, int64_t *verdict, hipStream_t s);
hipError_t launch_follow_compact(const Candidate *slots, FollowSegs fs, int64_t nseg, Candidate *out, hipStream_t s);
// FindBlockStart without a candidate list, on the bytes themselves
hipError_t launch_find_block_starts_bytes(const uint8_t *d, int64_t D, const int64_t *starts, int64_t n,
                                          int32_t blocks_to_check, int64_t *out, hipStream_t s);
hipError_t launch_scan_slots(const uint8_t *d, int64_t D, int32_t *chunk_counts, int64_t nchunks, Candidate *slots,
                             int64_t *overflow, hipStream_t s);
hipError_t launch_scan_compact(const Candidate *slots, const int32_t *chunk_counts, const int64_t *chunk_offsets,
                               int64_t nchunks, Candidate *out, hipStream_t s);
hipError_t launch_scan_write(const uint8_t *d, int64_t D, const int64_t *chunk_offsets, int64_t nchunks,
                             Candidate *cands, hipStream_t s);
hipError_t launch_chain_verify(const Candidate *cands, int64_t ncand, int64_t first, int64_t D, int64_t *first_stop,
                               hipStream_t s);
hipError_t launch_find_block_starts(int64_t D, const Candidate *cands, int64_t ncand, const int64_t *starts, int64_t n,
                                    int32_t blocks_to_check, int64_t *out, hipStream_t s);
// (+ uoff[0..n]: the uncompressed offsets, computed on the device; wsum: (n + 255) / 256 int64 of scratch)
hipError_t launch_gather_blocks(const Candidate *cands, int64_t first, int64_t n, int64_t *start, int32_t *hsize,
                                int32_t *csize, int32_t *usize, int64_t *wsum, int64_t *uoff, hipStream_t s);
// Inflate (sbam_inflate.hip): entropy decode into per-block token regions (wave-parallel fast path, per-lane
// exact path for the blocks it hands over), then LZ77 resolve into `out`.  tok: inflate_token_bytes(L, nb) bytes;
// slow: nb int32; counters: 3 × u32 device scratch, reset by the decode launch.
inline size_t inflate_token_bytes(int64_t L, int64_t nb) {
  // main regions (+1 KiB: the resolver reads up to 2 x 64 + 1 tokens past a step's start)
  return (((size_t)L + 15) & ~(size_t)15) + 32 * (size_t)nb + 1024;
}
// default arena: 1/16 of the uncompressed bytes (the synthetic BAM needs none; stored blocks need 2 B per byte)
// (SBAM_ARENA_MB overrides it: tests of the arena's growth)
inline size_t inflate_arena_bytes(int64_t L) {
  const char *e = std::getenv("SBAM_ARENA_MB");
  if (e && *e) return (size_t)std::atoll(e) << 20;
  return (size_t)L / 16 + (1u << 20);
}
hipError_t launch_inflate_decode(const uint8_t *d, int64_t D, BlockTable bt, TokPool tok, uint8_t *out,
                                 int32_t *status, int32_t *found, int32_t *slow, unsigned int *counters,
                                 hipStream_t s);
// list (nlist blocks) or every block; blocks with a distance past their first byte are appended to redo[*nredo]
hipError_t launch_inflate_resolve(BlockTable bt, uint8_t *out, TokPool tok, const int32_t *found,
                                  const int32_t *list, int64_t nlist, int32_t *redo, unsigned int *nredo,
                                  hipStream_t s);
// the exact decoder over list[0 .. counters[2]) (the resolver's redo list)
hipError_t launch_inflate_redo(const uint8_t *d, int64_t D, BlockTable bt, TokPool tok, const int32_t *list,
                               unsigned int *counters, int32_t *status, int32_t *found, hipStream_t s);
// first_err = min block index with status != 0 (caller presets ~0)
hipError_t launch_first_error(const int32_t *status, int64_t n, unsigned long long *first_err, hipStream_t s);
hipError_t launch_lower_bound(const Candidate *c, int64_t n, int64_t q, int64_t *out, hipStream_t s);
// CRC32 of the inflated bytes of blocks [b0, b1) against the footers' (sbam_crc.hip): crc[b] computed, stored[b] the
// little-endian u32 at comp[start[b] + csize[b] - 8]; *n_bad += mismatches, *first_bad = min(*first_bad, their
// indices) (the caller presets 0 and ~0).  u: the stream of L bytes with its kStreamPad behind it.
hipError_t launch_block_crc(const uint8_t *comp, int64_t D, const uint8_t *u, int64_t L, BlockTable bt, int64_t b0,
                            int64_t b1, uint32_t *crc, uint32_t *stored, unsigned long long *n_bad,
                            unsigned long long *first_bad, hipStream_t s);
// Bitmaps cover [x0 & ~63, x1): bit (x - (x0 & ~63)) = call at x (0 for x < x0).
// *tiles_counted: whether cd.tile_pass0 now holds every tile's PASS0 count (it is set, and the run is not by-key)
hipError_t launch_check_full_counts(StreamView sv, int64_t x0, int64_t x1, int32_t R, int32_t by_key, CountsDev cd,
                                    unsigned long long *bitmap, hipStream_t s, bool *tiles_counted);
int64_t check_tiles(int64_t x0, int64_t x1);  // record-0 pass tiles of [x0, x1)
// (launch_check_full_counts runs the record-0 pass; launch_check_full_chains then resolves the PASS0 chains)
hipError_t launch_check_full_chains(StreamView sv, int64_t x0, int64_t x1, int32_t R, int32_t by_key, CountsDev cd,
                                    unsigned long long *bitmap, hipStream_t s);
// list-form chain pass (sbam_check.hip): scratch owned by the context
struct ChainScratch {
  int32_t *chunk_cnt;             // [nchunks]
  int64_t *chunk_off;             // [nchunks + 1]; [nchunks] = number of PASS0 positions
  int64_t *list;                  // PASS0 positions in order
  uint8_t *ok;                    // link bits
  int64_t *fb;                    // fallback positions
  unsigned long long *n_fb;       // fallback count
};
int64_t chain_list_chunks(int64_t x0, int64_t x1);
// tile_pass0 (or nullptr: count the bitmap): the record-0 pass's per-tile counts (CountsDev::tile_pass0)
hipError_t launch_chain_list_build(int64_t x0, int64_t x1, const unsigned long long *bitmap, const ChainScratch &cs,
                                   const int32_t *tile_pass0, hipStream_t s);
hipError_t launch_chain_list_run(StreamView sv, int64_t x0, int64_t x1, int32_t R, int32_t by_key, CountsDev cd,
                                 unsigned long long *bitmap, const ChainScratch &cs, hipStream_t s);
// (first_halo: CountsDev::first_halo, nullptr on a whole file)
hipError_t launch_check_eager_pass0(StreamView sv, int64_t x0, int64_t x1, int32_t R, unsigned long long *bitmap,
                                    unsigned long long *first_halo, hipStream_t s);
hipError_t launch_check_words(StreamView sv, int64_t x0, int64_t x1, int32_t R, uint32_t *words,
                              unsigned long long *bitmap, unsigned long long *first_halo, hipStream_t s);
hipError_t launch_find_record_starts(StreamView sv, const int64_t *x0, int64_t n, int32_t R, int64_t max_read_size,
                                     const unsigned long long *bitmap, int64_t bitmap_x0, int64_t bitmap_x1,
                                     int64_t *out, hipStream_t s);
hipError_t launch_record_counts(StreamView sv, const int64_t *x0, const int64_t *x_end, int64_t n, int64_t *counts,
                                hipStream_t s);
hipError_t launch_record_offsets(StreamView sv, int64_t x0, int64_t x_end, int64_t *offsets, int64_t cap,
                                 int64_t *n_out, hipStream_t s);
// Record chains of splits and record decode (sbam_records.hip).  Bitmaps as for the checker: bit (x - xa) = call
// at x, xa 64-aligned.  fail: i32 device flag, set to 1 when the chain is not the bitmap's set bits.
hipError_t launch_chain_proof(const uint8_t *u, int64_t L, const unsigned long long *bm, int64_t xa, int64_t X0,
                              int64_t X1, int32_t *fail, const unsigned long long *exact, hipStream_t s);
// (list, nlist, exact: the chain pass's PASS0 list and counters when the bitmap came from it, else nullptr)
hipError_t launch_split_popcounts(const unsigned long long *bm, int64_t xa, const int64_t *xs, const int64_t *xe,
                                  int64_t n, int64_t *counts, int32_t *fail, const int64_t *list, int64_t nlist,
                                  const unsigned long long *exact, hipStream_t s);
hipError_t launch_split_offsets(const unsigned long long *bm, int64_t xa, const int64_t *xs, const int64_t *xe,
                                const int64_t *base, int64_t n, int64_t *out, hipStream_t s);
hipError_t launch_record_walk(const uint8_t *u, int64_t L, const int64_t *xs, const int64_t *xe, const int64_t *base,
                              int64_t n, int64_t *out, hipStream_t s);
hipError_t launch_record_spans(const uint8_t *u, int64_t L, const int64_t *offs, int64_t n, int32_t *ref_id,
                               int32_t *start, int32_t *end, hipStream_t s);
hipError_t launch_record_columns(const uint8_t *u, const int64_t *offs, int64_t n, const int64_t *bstart,
                                 const int64_t *buoff, const int32_t *busize, int64_t nblocks, int64_t file_base,
                                 RecordColumnsDev cols, hipStream_t s);
// Variable-length fields of decoded records as CSR columns (sbam_fields.hip).  All pointers address the batch's
// first record; L is the stream's length.
struct FieldSizesArgs {
  const int64_t *roff;
  const int32_t *block_size;
  const uint32_t *bin_mq_nl, *flag_nc;
  const int32_t *l_seq;
  int64_t n, L;
};
// lengths of record k's four CSR columns; a record that fails validation has none
struct FieldLens {
  int64_t v[4];  // name bytes, cigar ops, bases, aux bytes
  bool bad;
};
__device__ __forceinline__ FieldLens field_lens(const FieldSizesArgs &a, int64_t k) {
  FieldLens r;
  const int64_t bs = a.block_size[k], ls = a.l_seq[k];
  const int64_t lrn = a.bin_mq_nl[k] & 0xffu, nc = a.flag_nc[k] & 0xffffu;
  const int64_t need = 36 + lrn + 4 * nc + ((ls + 1) >> 1) + ls;
  r.bad = ls < 0 || need > 4 + bs || a.roff[k] + 4 + bs > a.L;
  r.v[0] = r.bad ? 0 : (lrn > 1 ? lrn - 1 : 0);
  r.v[1] = r.bad ? 0 : nc;
  r.v[2] = r.bad ? 0 : ls;
  r.v[3] = r.bad ? 0 : 4 + bs - need;
  return r;
}
struct FieldOffsets {  // n + 1 int64 each
  int64_t *name, *cigar, *seq, *aux;
};
struct FieldGatherArgs {
  const uint8_t *u;
  const int64_t *roff;
  const uint32_t *bin_mq_nl, *flag_nc;
  const int32_t *l_seq;
  const int64_t *off;  // the column's offsets, in units of 1 << sh bytes
  int64_t n;
  int32_t sh;
  int64_t total;       // output bytes
  uint8_t *out;        // 8-byte aligned, room for total rounded up to 8
  int64_t *tiles;      // scratch: 2 * field_gather_tiles(total) int64 (each tile's first and last record)
  const int64_t *src = nullptr;  // field 5 only: each record's source position in the stream
};
int64_t field_size_blocks(int64_t n);  // entries per length of launch_field_sizes' bsum scratch
int64_t field_gather_tiles(int64_t total);
// lengths, validation (first_bad = min failing record index of the batch, ~0 when none) and offsets; totals[4]
hipError_t launch_field_sizes(const FieldSizesArgs &a, int64_t *bsum, FieldOffsets off, unsigned long long *first_bad,
                              int64_t *totals, hipStream_t s);
// field: 0 name, 1 cigar, 2 seq (ASCII bases), 3 qual, 4 aux, 5 the bytes at a.src[r] (roff and the fixed-field
// columns are then not read)
hipError_t launch_field_gather(int field, const FieldGatherArgs &a, hipStream_t s);
// BAI index from the record columns (sbam_index.hip).  Records in file order; the block table as for
// launch_record_columns (+ csize: the address behind the last block is where the last record ends).
struct IndexArgs {
  const uint8_t *u;
  int64_t L;
  const int64_t *roff, *block_pos;
  const int32_t *block_off, *block_size, *ref_id, *pos;
  const uint32_t *bin_mq_nl, *flag_nc;
  int64_t n;
  int32_t nref;
  const int64_t *bstart, *buoff;
  const int32_t *bcsize, *busize;
  int64_t nblocks, file_base;
  int32_t *end_out;   // scratch columns, n each: the exclusive reference end and reg2bin(beg, end)
  uint32_t *bin_out;
};
struct IndexStats {  // device words, preset by the host
  unsigned long long *w;  // [0] first offending stream offset (~0), [1] n_no_coor, [2] n_unsorted, [3] n_runs
  unsigned long long *n_mapped, *n_unmapped, *off_beg /* ~0 */, *off_end, *n_intv;  // nref each
};
struct IndexRuns {  // n entries each
  int32_t *ref;
  uint32_t *bin;
  unsigned long long *beg, *end;
  int64_t n;
};
int64_t index_blocks(int64_t n);  // entries of the passes' heads scratch
int index_long_cigar_ops();       // a record with more CIGAR ops than this is summed by a whole wave
// spans, counters, and heads[] = exclusive sums of the run heads per workgroup (st.w[3] = n_runs)
hipError_t launch_index_pass1(const IndexArgs &a, IndexStats st, int64_t *heads, hipStream_t s);
// run scatter, linear index into ioffset (preset ~0; reference r's windows at [intv_off[r], intv_off[r + 1])) and
// its backward fill
hipError_t launch_index_pass2(const IndexArgs &a, const int64_t *heads, IndexRuns r, const int64_t *intv_off,
                              unsigned long long *ioffset, hipStream_t s);

// Typed tags of decoded records (sbam_tags.hip): the walk over records [0, n) of a batch, the scans of the byte
// columns' lengths, and (through launch_field_gather, field 5) their bytes.
struct TagWalkArgs {
  FieldSizesArgs rec;            // the batch's fixed-field columns
  const uint8_t *u;              // the stream (rec.L bytes and its pad)
  int32_t nq, nb;                // queried tags; byte columns
  uint16_t key[32];              // name[0] | name[1] << 8 per query entry
  int8_t bcol[32];               // the entry's byte column, -1: none
  unsigned long long filter;     // sbam_tag::filter_bit of every key
  uint8_t *type, *sub;           // nq * n each, tag-major
  int32_t *rel;
  int64_t *value;
  int64_t *off;                  // byte column b's lengths at off[b * ostride + k] (scanned in place afterwards)
  int64_t ostride;
  int64_t *src;                  // and its values' stream positions at src[b * n + k]
  unsigned long long *first_bad; // min index of a malformed record (preset ~0)
  unsigned long long *present;   // kTagPresentSlots x 32 counters (preset 0): entry j's count is the sum over slots
};
constexpr int kTagPresentSlots = 64;
int tag_long_aux_bytes();
hipError_t launch_tag_walk(const TagWalkArgs &a, hipStream_t s);

// Prefix sums (sbam_scan.hip).  Column c of `cols`: out[c * n + i] = the sum of in[c * n + j] over j < i, as int64,
// and totals[c] = the column's sum; one workgroup per column.  out may be in (int64).
hipError_t launch_scan_sums(const int32_t *in, int64_t *out, int64_t n, int32_t cols, int64_t *totals, hipStream_t s);
hipError_t launch_scan_sums(const int64_t *in, int64_t *out, int64_t n, int32_t cols, int64_t *totals, hipStream_t s);
// off[c * stride + k], k < n: values -> exclusive prefix sums in place, [n] = totals[c] = the column's sum.
// bsum: cols * exclusive_scan_blocks(n) int64 of scratch.
int64_t exclusive_scan_blocks(int64_t n);
hipError_t launch_exclusive_scan(int64_t *off, int64_t stride, int64_t n, int32_t cols, int64_t *bsum, int64_t *totals,
                                 hipStream_t s);

// Coordinate sort (sbam_sort.hip): a stable LSD radix sort of (key, index) pairs, 8-bit digits.  The tile is a build
// constant (sbam_sort_tile_keys): a multiple of 256, at most 8192.
#ifndef SBAM_SORT_TILE
#define SBAM_SORT_TILE 2048
#endif
constexpr int kSortTile = SBAM_SORT_TILE;
constexpr int kSortHistWords = 8 * 256 + 1;  // the eight digit histograms, then the out-of-order count
struct SortBufs {  // (sbam_layout.h: sort_bufs)
  uint64_t *keys[2];         // n each: ping and pong
  uint32_t *idx[2];          // n each (the kernels carry 32-bit indices: n < 2^32)
  int64_t *order;            // n: the result
  int64_t *cnt;              // 256 columns of sort_tiles(n) + 1: a pass's per-tile digit counts, scanned in place
  int64_t *bsum;             // 256 * exclusive_scan_blocks(sort_tiles(n)): the scan's scratch
  int64_t *totals, *dbase;   // 256: the columns' totals; 257: their exclusive sums (the buckets' bases) and the total
  unsigned long long *hist;  // kSortHistWords
};
int64_t sort_tiles(int64_t n);
// keys[0] (ref_id non-null: built from the columns; null: already there), and hist filled
hipError_t launch_sort_keys(const int32_t *ref_id, const int32_t *pos, int64_t n, const SortBufs &b, hipStream_t s);
// one pass by byte `pass` from keys[src], idx[src] to the other pair (first: idx[src] is the identity and not read;
// last: the indices go to order as int64, the keys nowhere)
hipError_t launch_sort_pass(const SortBufs &b, int64_t n, int pass, int src, bool first, bool last, hipStream_t s);
hipError_t launch_sort_identity(int64_t *order, int64_t n, hipStream_t s);
// *flag (an 8-byte word, read as int32) = 1 when an entry of order[0, n) lies outside [0, limit), else 0
hipError_t launch_order_check(const int64_t *order, int64_t n, int64_t limit, int32_t *flag, hipStream_t s);

// BAM writer (sbam_write.hip): select -> (launch_exclusive_scan, launch_field_gather field 5) -> deflate -> frame.
struct WriteSelectArgs {
  const int64_t *roff;           // the loaded records' stream offsets and block_size column, n each
  const int32_t *block_size;
  int64_t n, L;                  // (L: the stream's length)
  const int64_t *range_lo, *range_hi;  // device: record-index ranges [lo, hi), ascending and disjoint
  int64_t n_ranges;              // 0: every record
  const uint8_t *keep;           // device byte per record (nonzero: keep), or nullptr
  int64_t header_bytes;          // stream bytes [0, header_bytes) go first (entry 0 of the columns)
  int64_t *len, *cnt;            // n + 1 values each (room for n + 2: the scan adds the total): bytes and 0 / 1
  int64_t *src;                  // n + 1: each entry's source position in the stream
  const int64_t *order = nullptr;  // device, n entries: entry 1 + k is record order[k] (null: record k); ranges and
                                   // keep still index the loaded records
};
hipError_t launch_write_select(const WriteSelectArgs &a, hipStream_t s);
// Pos of the written records from the scanned columns (off, ord: n + 2 entries each) and the written block starts
hipError_t launch_written_records(const int64_t *off, const int64_t *ord, int64_t n, int32_t block_bytes,
                                  const int64_t *start, int64_t *block_pos, int32_t *block_off, hipStream_t s);
constexpr int kWritePad = 4096;  // readable bytes behind the writer's stream (the CRC's row lookahead, the matcher's
                                 // compare past a block's end); the stream is 16-byte aligned
// One batch of output blocks [b0, b0 + nb): block b holds stream bytes [b * block_bytes, ...) of wu[0, ubytes).
struct WriteBlocksArgs {
  const uint8_t *wu;
  int64_t ubytes;
  int32_t block_bytes;
  int64_t b0, nb;
  uint8_t *slots;        // block b0 + k's fixed-Huffman payload at slots + k * slot_stride (level 1)
  int64_t slot_stride;   // write_slot_stride(block_bytes): the stored bound, not 64 KiB
  int32_t *pay, *stored; // by block: payload bytes, 1 = stored form
  int64_t *tsz;          // by k: 18 + payload + 8; scanned in place (nb + 1 entries) between deflate and frame
  uint8_t *tokens;       // SBAM_WRITE_DYNAMIC: write_token_records(nb) records of token_stride bytes, one per workgroup
  int64_t token_stride;  // write_token_stride(block_bytes)
};
struct WriteFrameArgs {
  uint8_t *file;         // 8-byte aligned
  int64_t base;          // file offset of the batch's first block
  int32_t with_eof;      // the EOF block goes behind the batch
  int64_t *start;        // by block (+ the end offset behind the batch's last)
  int32_t *csize, *usize;
  unsigned long long *n_stored;  // += stored blocks
};
constexpr int32_t kWriteDynamic = 0x100;  // SBAM_WRITE_DYNAMIC of sbam.h, in the level word
int64_t write_slot_stride(int32_t block_bytes);
int64_t write_token_stride(int32_t block_bytes);
int64_t write_token_records(int64_t blocks);
hipError_t launch_write_deflate(const WriteBlocksArgs &a, int32_t level, hipStream_t s);
hipError_t launch_write_frame(const WriteBlocksArgs &a, const WriteFrameArgs &f, hipStream_t s);

}  // namespace sbam
