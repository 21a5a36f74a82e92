// sbam_layout.h — where every column lies in the arenas the host layer (sbam_api.cpp) carves: one function per arena,
// run once on a null cursor for the arena's size and once on the buffer for the pointers, so the size and the
// pointers cannot disagree.  sbam_reserve runs the same functions with its estimates.  Plain C++ (no HIP): counts
// that follow from a kernel's launch geometry (exclusive_scan_blocks, field_gather_tiles, ...) come in as numbers, and
// a layout whose columns are a launcher's argument struct (sbam_internal.h) fills that struct, named by the caller.
// Host-tested by tests/test_layout_host.py.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sbam.h"

namespace sbam_layout {

typedef unsigned long long u64;  // (the kernels' counter type)

// Carve cursor over an arena at `base` (null: sizes only, every column null).  A column starts at the next multiple of
// its alignment (the base is at least 256-B aligned), so columns taken with their element's size as alignment form one
// contiguous run behind the column before them: what one memset or one copy covers.
struct Carve {
  explicit Carve(void *base) : base_(static_cast<uint8_t *>(base)) {}
  template <class T>
  T *take(size_t n, size_t align = 256) {
    at_ = up(at_, align);
    T *p = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
    at_ += n * sizeof(T);
    return p;
  }
  int32_t *i32(size_t n, size_t a = 256) { return take<int32_t>(n, a); }
  int64_t *i64(size_t n, size_t a = 256) { return take<int64_t>(n, a); }
  u64 *w64(size_t n, size_t a = 256) { return take<u64>(n, a); }
  size_t bytes() const { return up(at_, 256); }  // the arena's size
  static size_t up(size_t b, size_t a = 256) { return (b + a - 1) & ~(a - 1); }
  uint8_t *base_;
  size_t at_ = 0;  // the end of the last column
};

// The followed block table's nseg segments, as R = FollowSegs
template <class R>
R follow_segs(Carve &k, size_t nseg) {
  return R{k.i64(nseg), k.i64(nseg), k.i32(nseg), k.i32(nseg), k.i32(nseg), k.i64(nseg)};
}

// loadReads' n records, as R = RecordColumnsDev
template <class R>
R record_cols(Carve &k, size_t n) {
  return R{k.i64(n), k.i32(n), k.i32(n), k.i32(n), k.i32(n), k.take<uint32_t>(n),
           k.take<uint32_t>(n), k.i32(n), k.i32(n), k.i32(n), k.i32(n)};
}

// The fields' offsets of n records: four CSR columns of n + 1, the sizes' scan scratch (nblk = field_size_blocks(n)),
// and one run of five words: the first bad record, then the four totals
struct FieldOffs { int64_t *off[4], *bsum, *first_bad, *totals; };
inline FieldOffs field_offs(Carve &k, size_t n, size_t nblk) {
  return {{k.i64(n + 1), k.i64(n + 1), k.i64(n + 1), k.i64(n + 1)}, k.i64(4 * nblk), k.i64(1), k.i64(4, 8)};
}

// A byte column (one of the fields' data, one tag's bytes): its bytes, padded to the gather's 8-byte stores, and behind
// them the gather's per-tile record ranges (tiles = field_gather_tiles(bytes))
struct ByteCol { uint8_t *data; int64_t *tiles; };
inline ByteCol byte_col(Carve &k, size_t bytes, size_t tiles) { return {k.take<uint8_t>(bytes + 8), k.i64(2 * tiles)}; }

// Typed tags of n records into wa = TagWalkArgs (nq queries, nb of them with a byte column): the four cell columns
template <class A>
void tag_cells(Carve &k, A &wa, size_t n) {
  const size_t cells = (size_t)wa.nq * n;
  wa.type = k.take<uint8_t>(cells), wa.sub = k.take<uint8_t>(cells), wa.rel = k.i32(cells), wa.value = k.i64(cells);
}
// and the byte columns' offset columns (n + 1 each, ostride entries apart), their values' source positions (n each),
// the scans' scratch (nblk = exclusive_scan_blocks(n) each), and one run of 1 + SBAM_MAX_TAGS + slots x SBAM_MAX_TAGS
// words: the first bad record, the byte totals, the present counters
struct TagScan { int64_t *bsum, *totals; };
constexpr size_t kTagTotalsAt = 1, kTagPresentAt = 1 + SBAM_MAX_TAGS;  // words into the run
template <class A>
TagScan tag_offs(Carve &k, A &wa, size_t n, size_t nblk, size_t slots) {
  wa.ostride = (int64_t)(Carve::up((n + 1) * 8) / 8);
  wa.off = k.i64((size_t)wa.nb * wa.ostride), wa.src = k.i64((size_t)wa.nb * n);
  int64_t *bsum = k.i64((size_t)wa.nb * nblk);
  wa.first_bad = k.w64(1);
  int64_t *totals = k.i64(SBAM_MAX_TAGS, 8);
  wa.present = k.w64(slots * SBAM_MAX_TAGS, 8);
  return {bsum, totals};
}

// The index's counter words as R = IndexStats, one run: four scalars, then five counters per reference
template <class R>
R index_words(Carve &k, size_t nref) {
  return R{k.w64(4), k.w64(nref, 8), k.w64(nref, 8), k.w64(nref, 8), k.w64(nref, 8), k.w64(nref, 8)};
}

// The coordinate sort of n keys as R = SortBufs: the order, the ping-pong keys and 32-bit indices, a pass's digit
// counts (256 columns of tiles + 1), the scan's scratch (nblk = exclusive_scan_blocks(tiles) per column), the 256
// totals, their 257 sums, and the histogram words (hist_words: eight histograms and the out-of-order count)
template <class R>
R sort_bufs(Carve &k, size_t n, size_t tiles, size_t nblk, size_t hist_words) {
  R r{};
  r.order = k.i64(n);
  r.keys[0] = k.take<uint64_t>(n), r.keys[1] = k.take<uint64_t>(n);
  r.idx[0] = k.take<uint32_t>(n), r.idx[1] = k.take<uint32_t>(n);
  r.cnt = k.i64(256 * (tiles + 1));
  r.bsum = k.i64(256 * nblk);
  r.totals = k.i64(256), r.dbase = k.i64(257);
  r.hist = k.w64(hist_words);
  return r;
}

// The writer's selection over n loaded records, one run: the length and the 0-1 column (n + 1 entries and the scan's
// total each, stride apart), each entry's source, the scan's scratch (nblk = exclusive_scan_blocks(n + 1) per column)
// and the two totals
struct WriteSel { int64_t *len, *cnt; size_t stride; int64_t *src, *bsum, *tot; };
inline WriteSel write_sel(Carve &k, size_t n, size_t nblk) {
  return {k.i64(n + 2), k.i64(n + 2, 8), n + 2, k.i64(n + 1, 8), k.i64(2 * nblk, 8), k.i64(2, 8)};
}

// The writer's blocks stage.  Per batch: the sizes (and the scan's total), the scan's scratch (nblk =
// exclusive_scan_blocks(batch)), the batch's bytes, the stored-block counter.  Per block of the file: four columns.
struct WriteSizes { int64_t *tsz, *bsum, *tot; u64 *n_stored; };
inline WriteSizes write_sizes(Carve &k, size_t batch, size_t nblk) {
  return {k.i64(batch + 1), k.i64(nblk, 8), k.i64(1, 8), k.w64(1, 8)};
}
struct WriteCols { int32_t *pay, *stored, *csize, *usize; };
inline WriteCols write_cols(Carve &k, size_t nb) { return {k.i32(nb), k.i32(nb, 4), k.i32(nb, 4), k.i32(nb, 4)}; }

// The full check's Counts as R = CountsDev, one run (on the device, and the host's copy of it): the groups of
// sbam_counts from `counts` to the four scalars in its order, then the totals
template <class R>
R count_words(Carve &k) {
  constexpr size_t K = SBAM_NUM_KEYS, F = SBAM_NUM_FLAGS, N = SBAM_MAX_READS_TO_CHECK + 1;
  return R{k.w64(K * F), k.w64(K, 8), k.w64(K * N, 8), k.w64(F * F, 8), k.w64(4, 8), k.w64(F, 8)};
}

}  // namespace sbam_layout
