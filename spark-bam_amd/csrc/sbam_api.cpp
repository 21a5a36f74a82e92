// sbam_api.cpp — C-ABI (include/sbam.h) over the HIP kernels: device memory, stage orchestration,
// Pos mapping, split assembly and error records.  Host code mirrors the reference's control flow:
//   Channels / FindBlockStart / FindRecordStart / loadReadsAndPositions / loadSplitsAndReads
//   (load/src/main/scala/org/hammerlab/bam/spark/load/CanLoadBam.scala:173-334),
//   full-check Counts folding (cli/src/main/scala/org/hammerlab/bam/check/full/FullCheck.scala:141-191).
#include "../../include/sbam.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sbam_deflate_core.h"
#include "sbam_internal.h"
#include "sbam_layout.h"
#include "sbam_tag_core.h"

using namespace sbam;
using namespace sbam_layout;

namespace {

#define HIPTRY(expr)                 \
  do {                               \
    hipError_t e_ = (expr);          \
    if (e_ != hipSuccess) return e_; \
  } while (0)

// SBAM_LOG_GROW=1: report every reallocation of an existing buffer (the streamed pipe's stalls)
bool log_grow() {
  static const bool on = [] {
    const char *e = std::getenv("SBAM_LOG_GROW");
    return e && *e && *e != '0';
  }();
  return on;
}

// Owned, grow-only device buffer: reused across sbam_reset() so a re-run allocates nothing; frees itself (with the
// owner's device current: sbam_close, or the entry point a local one lives in).
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p_) (void)hipFree(p_);
  }
  // Room for n elements (at least one).  An allocation that is large enough is kept; else a new one replaces it and
  // the contents are lost: *grew is then set (a buffer never allocated held no stage's data, and sets nothing).
  hipError_t ensure(size_t n, bool *grew = nullptr) {
    if (p_ && size_ >= n) return hipSuccess;
    const size_t m = std::max<size_t>(n, 1);
    if (p_ && log_grow()) std::fprintf(stderr, "[sbam] grow %zu -> %zu bytes\n", size_ * sizeof(T), m * sizeof(T));
    if (p_ && grew) *grew = true;
    if (p_) (void)hipFree(p_);  // (first: the two need not fit side by side)
    size_ = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), m * sizeof(T));
    if (e == hipSuccess) size_ = m;
    else p_ = nullptr;
    return e;
  }
  void swap(DevBuf &o) {
    std::swap(p_, o.p_);
    std::swap(size_, o.size_);
  }
  size_t size() const { return size_; }  // elements allocated
  T *get() const { return p_; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
  size_t size_ = 0;
};

// Token arena (TokPool): blocks whose tokens outgrow their main region.  The allocation has 1 KiB more than the
// usable bytes: the resolver's token lookahead.
struct TokArena {
  DevBuf<uint8_t> buf;
  size_t usable() const { return buf.size() ? buf.size() - 1024 : 0; }
  hipError_t ensure(size_t bytes, bool *grew = nullptr) { return buf.ensure(bytes + 1024, grew); }
};

// The BAM writer's blocks stage (sbam_write.hip): an uncompressed stream in, BGZF bytes and their block table out.
// Owned by a context (sbam_write_bam) or by a test call (sbam_test_deflate); writer_run fills it.
constexpr int64_t kWriteBatch = 4096;  // blocks deflated into the slots at a time (268 MB of stream at 65 498)
struct Writer {
  DevBuf<uint8_t> u;      // the stream (writer_ensure_stream)
  DevBuf<uint8_t> slots;  // one batch's Huffman payloads
  DevBuf<uint8_t> tokens; // SBAM_WRITE_DYNAMIC: one token record per workgroup of a batch's launch
  DevBuf<uint8_t> cols;   // by block: write_cols, carved into col
  DevBuf<int64_t> start;  // by block, + the end offset
  DevBuf<uint8_t> tsz;    // of a batch: write_sizes, carved into sz
  WriteCols col{}; WriteSizes sz{};  // (set by ensure_write_blocks)
  DevBuf<uint8_t> file;
  int64_t ubytes = -1, nb = 0, n_stored = 0, comp_bytes = 0;  // of the last run (ubytes: set by the owner, -1: none)
  int32_t block_bytes = 0;
};

// Host mirror of the scanned block table (relative offsets).  The fast scan's table comes back behind the GPU, into
// pinned staging: the stream's length on the main stream (ev[0]), the columns on copy_stream, beside the decoder,
// once the table is built (ev[2]; ev[1] when they have landed).  get() moves them into the vectors when the host
// first reads them (sbam_inflate: while the decoder runs); total() needs only the length.
struct BlockMirror {
  int64_t n = -1;  // blocks of the scanned table; -1: sbam_scan_blocks has not run
  std::vector<int64_t> start, uoff;  // (uoff: n + 1 entries, the last one the stream's length)
  std::vector<int32_t> csize, usize;
  uint8_t *stage = nullptr;  // pinned: length | start[n] | uoff[n + 1] | csize[n] | usize[n]
  size_t stage_bytes = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipStream_t copy_stream = nullptr;
  bool pending = false;  // the table is in staging (or on its way there), not yet in the vectors

  // No table.  Waits for a column copy nobody read: it reads the device columns and writes the staging that the
  // next table reuses, and must not land over that table later.
  hipError_t invalidate() {
    const hipError_t e = pending ? hipEventSynchronize(ev[1]) : hipSuccess;
    pending = false;
    n = -1;  // (the vectors keep their storage; fill() and get() replace their contents)
    return e;
  }
  // After a fast scan: queue the host's copy of the nb-block device table behind the work on s; not waited for.
  hipError_t start_copy(const int64_t *d_start, const int64_t *d_uoff, const int32_t *d_csize, const int32_t *d_usize,
                        int64_t nb, hipStream_t s) {
    const size_t need = 8 + (size_t)nb * 8 + (size_t)(nb + 1) * 8 + (size_t)nb * 8;
    if (stage_bytes < need) {
      HIPTRY(hipStreamSynchronize(s));  // (an earlier table's length copy may still target the old staging)
      if (stage) (void)hipHostFree(stage);
      stage = nullptr;
      stage_bytes = 0;
      HIPTRY(hipHostMalloc(reinterpret_cast<void **>(&stage), need + need / 8, hipHostMallocDefault));
      stage_bytes = need + need / 8;
    }
    for (hipEvent_t &e : ev)
      if (!e) HIPTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!copy_stream) HIPTRY(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    int64_t *st = reinterpret_cast<int64_t *>(stage + 8), *uo = st + nb;
    int32_t *cs = reinterpret_cast<int32_t *>(uo + nb + 1), *us = cs + nb;
    HIPTRY(hipMemcpyAsync(stage, d_uoff + nb, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipEventRecord(ev[0], s));
    HIPTRY(hipEventRecord(ev[2], s));
    HIPTRY(hipStreamWaitEvent(copy_stream, ev[2], 0));
    HIPTRY(hipMemcpyAsync(uo, d_uoff, (nb + 1) * 8, hipMemcpyDeviceToHost, copy_stream));
    if (nb) {
      HIPTRY(hipMemcpyAsync(st, d_start, nb * 8, hipMemcpyDeviceToHost, copy_stream));
      HIPTRY(hipMemcpyAsync(cs, d_csize, nb * 4, hipMemcpyDeviceToHost, copy_stream));
      HIPTRY(hipMemcpyAsync(us, d_usize, nb * 4, hipMemcpyDeviceToHost, copy_stream));
    }
    HIPTRY(hipEventRecord(ev[1], copy_stream));
    n = nb;
    pending = true;
    return hipSuccess;
  }
  // After the host walk: the table it built (uoff follows from usize).
  void fill(std::vector<int64_t> &&st, std::vector<int32_t> &&cs, std::vector<int32_t> &&us) {
    start = std::move(st);
    csize = std::move(cs);
    usize = std::move(us);
    n = (int64_t)start.size();
    uoff.resize(n + 1);
    int64_t acc = 0;
    for (int64_t b = 0; b < n; b++) {
      uoff[b] = acc;
      acc += (usize[b] < 0) ? 0 : usize[b];
    }
    uoff[n] = acc;
    pending = false;
  }
  // the scanned stream's uncompressed length (waits only for its own 8-byte copy)
  hipError_t total(int64_t *L) {
    if (pending) {
      HIPTRY(hipEventSynchronize(ev[0]));
      *L = *reinterpret_cast<const int64_t *>(stage);
    } else {
      *L = uoff[n];
    }
    return hipSuccess;
  }
  // the vectors, valid: waits for the columns and unpacks the staging once
  hipError_t get() {
    if (!pending) return hipSuccess;
    HIPTRY(hipEventSynchronize(ev[1]));
    const int64_t *st = reinterpret_cast<const int64_t *>(stage + 8), *uo = st + n;
    const int32_t *cs = reinterpret_cast<const int32_t *>(uo + n + 1), *us = cs + n;
    start.assign(st, st + n);
    uoff.assign(uo, uo + n + 1);
    csize.assign(cs, cs + n);
    usize.assign(us, us + n);
    pending = false;
    return hipSuccess;
  }
  // (sbam_close, both streams idle)
  void destroy() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stage) (void)hipHostFree(stage);
  }
};

// The context's small device scratch: one 8-byte word per use, so that no two uses share a word by accident.
//   scan_total, scan_overflow  scan_candidates (read back as one pair)
//   table_first, chain_stop    sbam_scan_blocks: the lower bound, and where the chain verify stopped
//   follow_bad, follow_stop,   follow_blocks: the link kernel's verdict and the accepted table's block count (read
//   follow_total               back as one triple)
//   inflate_error              first block whose status is not 0
//   record_count, proof_fail   sbam_record_offsets; split_counts (an int32 flag)
//   arena_used                 TokPool::arena_used
//   crc_bad, crc_first_bad     run_crc (written and read back as one pair)
//   order_bad                  sbam_write_bam_ordered: an entry of the caller's order outside the loaded records
//   first_halo                 the checkers on a shard: CountsDev::first_halo
struct Scratch {
  int64_t scan_total, scan_overflow, table_first, chain_stop, inflate_error, record_count, proof_fail, arena_used;
  int64_t crc_bad, crc_first_bad;
  int64_t follow_bad, follow_stop, follow_total;
  int64_t order_bad;
  int64_t first_halo;
};

}  // namespace

struct sbam_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t D = 0, base = 0, file_size = 0;
  DevBuf<uint8_t> d_comp;
  // candidates from the header scan
  DevBuf<Candidate> d_cand;
  int64_t ncand = -1;
  DevBuf<int32_t> d_cc;
  DevBuf<int64_t> d_coff;
  DevBuf<Candidate> d_slots;  // one-pass scan: kScanSlots per chunk; the followed table: kFollowSlots per segment
  // the followed table's segments (follow_segs), and what the last sbam_scan_blocks did (sbam_scan_path)
  DevBuf<uint8_t> d_fseg;
  int32_t sp_followed = 0, sp_fell_back = 0;
  int64_t sp_segments = 0;
  // per-call query scratch (split starts / answers): kept, since hipMalloc + hipFree per call cost ~0.5 ms of
  // host time each (a device-wide synchronisation) between the kernels of a step
  DevBuf<int64_t> d_qa, d_qb;
  // block table (relative offsets): device columns, and the host mirror that owns the scan's state (blk.n)
  DevBuf<int64_t> d_bstart, d_buoff;
  DevBuf<int32_t> d_bh, d_bc, d_bu;
  BlockMirror blk;
  // uncompressed stream
  DevBuf<uint8_t> d_u;
  int64_t L = -1;
  DevBuf<int32_t> d_status, d_found;
  // inflate scratch: token pages of the decode → resolve path
  DevBuf<uint8_t> d_pool;  // main token regions (inflate_token_bytes)
  TokArena arena;
  DevBuf<int64_t> d_tokbase;
  DevBuf<int32_t> d_slow;        // blocks the wave decoder hands to the exact per-lane decoder
  DevBuf<unsigned int> d_icnt;   // slow-path blocks, slow-path work, resolve work, stored-only blocks
  int64_t inflate_slow = -1;     // blocks the last sbam_inflate decoded on the exact per-lane path
  // CRC32 check of the stream's blocks (sbam_check_crc): computed and stored values by table index, and the range
  // [crc_b0, crc_b1) the last check filled (-1: none); they belong to the stream stage and go with it
  DevBuf<uint32_t> d_crc, d_crcst;
  int64_t crc_b0 = -1, crc_b1 = -1;
  bool verify_crc = false;  // sbam_set_verify_crc: sticky across reset and load
  // contig lengths
  int32_t nref = -1;
  DevBuf<int64_t> d_lens;
  std::vector<int64_t> h_lens;
  sbam_pos header_end{0, 0, 0};
  int64_t header_x = -1;  // stream offset of header_end (-1: the lengths came from sbam_set_contig_lengths)
  // success bitmap of the latest full/eager check, and what it covers (set_bitmap / drop_bitmap)
  DevBuf<unsigned long long> d_bitmap;
  int64_t bm_x0 = 0, bm_x1 = 0;
  int32_t bm_R = -1;
  bool bm_valid = false;
  bool bm_list = false;  // the bitmap came from the list-form chain pass: d_nfb[1..2] describe its links
  int64_t plist_n = 0;   // (and d_plist[0, plist_n) its PASS0 positions)
  // list-form chain pass scratch (launch_chain_list_*)
  DevBuf<int32_t> d_ccnt;
  DevBuf<int32_t> d_tcnt;  // record-0 pass: PASS0 positions per tile and wave (CountsDev::tile_pass0)
  DevBuf<int64_t> d_coff2, d_plist, d_pfb;
  DevBuf<uint8_t> d_pok;
  DevBuf<unsigned long long> d_nfb;
  // split chains: per-split first record / chain end / count / record base
  DevBuf<int64_t> d_sx, d_se, d_sn, d_sb;
  // what the last split_counts did (sbam_records_path): bitmap tried, proof held, and the list pass's link counters
  // (-1: not list-form), which stay in d_nfb until asked for (rp_fetch) or until the next check replaces them
  int32_t rp_tried = 0, rp_proved = 0;
  int64_t rp_missing = -1, rp_failed = -1;
  bool rp_fetch = false;
  // decoded records of the last sbam_load_records (offset column + RecordColumnsDev in one arena)
  DevBuf<int64_t> d_roff;
  DevBuf<uint8_t> d_rcols;
  RecordColumnsDev rcols{};
  int64_t n_loaded = -1;
  // variable-length fields of the last sbam_load_record_fields: offsets + scan scratch, and the data arena
  DevBuf<uint8_t> d_foff, d_fdata;
  sbam_record_fields fdev{};  // device pointers (data of unselected fields: null)
  int64_t f_i0 = 0, f_n = -1;
  sbam_record_field_totals f_tot{};
  // typed tags of the last sbam_load_record_tags: the four cell columns; the byte columns' offsets, source positions
  // and scan scratch; their bytes (tag_cells, tag_offs; ensure_byte_columns)
  DevBuf<uint8_t> d_tcell, d_toff, d_tdata;
  sbam_record_tags tdev{};  // device pointers (byte columns of entries without want_bytes: null)
  int64_t t_i0 = 0, t_n = -1;
  int32_t t_nq = 0;
  bool t_bytes[SBAM_MAX_TAGS] = {};  // which query entries have a byte column
  sbam_record_tag_totals t_tot{};
  // sbam_load_records covered every split of a whole file (what sbam_build_index needs)
  bool loaded_all = false;
  // BAI index of the last sbam_build_index: per-record scratch (end, bin), per-workgroup run heads, the counter
  // words (4 scalars + 5 per reference), the runs (ref, bin | beg | end) and the linear index with its offsets
  DevBuf<int32_t> d_iend;
  DevBuf<uint32_t> d_ibin;
  DevBuf<int64_t> d_iheads, d_iintv;
  DevBuf<uint8_t> d_istat;  // index_words
  DevBuf<unsigned long long> d_irun, d_ioff;
  DevBuf<int32_t> d_irunref;
  DevBuf<uint32_t> d_irunbin;
  bool idx_built = false;
  sbam_index_totals idx_tot{};
  IndexStats istat{};  // d_istat, carved (index_words)
  std::vector<int64_t> idx_intv;  // n_ref + 1 window offsets
  // coordinate order of the last sbam_sort_records: the order column with the sort's ping-pong buffers, counts and
  // histogram words in one arena (sort_bufs)
  DevBuf<uint8_t> d_sort;
  SortBufs sbuf{};
  bool sorted = false;
  sbam_sort_totals sort_tot{};
  // BAM of the last sbam_write_bam: the selection's columns (write_sel), the ranges, the gather's tiles, the blocks
  // stage, and the written records' Pos columns
  DevBuf<uint8_t> d_wsel;
  DevBuf<int64_t> d_wrange, d_wtiles, d_wrpos;
  DevBuf<int32_t> d_wroff;
  Writer w;
  sbam_write_totals w_tot{};
  // small device scratch
  DevBuf<int64_t> d_small;  // Scratch
  DevBuf<uint8_t> d_counts;  // count_words
  // timing
  std::map<std::string, std::pair<hipEvent_t, hipEvent_t>> ev;
  // sbam_load's copy pieces in flight (hipEventDisableTiming events, created on first use)
  hipEvent_t load_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  sbam_error err{};
  std::string path = "<bytes>";  // Path.toString in exception messages (sbam_set_path)
};

namespace {

int set_err(sbam_ctx *c, int code, const char *fmt, ...) {
  c->err.code = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(c->err.message, sizeof(c->err.message), fmt, ap);
  va_end(ap);
  return code;
}

#define HIPCHK(ctx, expr)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return set_err(ctx, SBAM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct Timer {  // HIP events around a launch family on the ctx stream (no context: nothing)
  sbam_ctx *c;
  std::pair<hipEvent_t, hipEvent_t> *e = nullptr;
  Timer(sbam_ctx *c_, const char *name) : c(c_) {
    if (!c) return;
    auto it = c->ev.find(name);
    if (it == c->ev.end()) {
      std::pair<hipEvent_t, hipEvent_t> p;
      (void)hipEventCreate(&p.first);
      (void)hipEventCreate(&p.second);
      it = c->ev.emplace(name, p).first;
    }
    e = &it->second;
    (void)hipEventRecord(e->first, c->stream);
  }
  ~Timer() { if (c) (void)hipEventRecord(e->second, c->stream); }
};

// a word of the small scratch, by name
#define SMALL(c, word) ((c)->d_small.get() + offsetof(Scratch, word) / 8)
#define USMALL(c, word) reinterpret_cast<unsigned long long *>(SMALL(c, word))

// An arena by its layout (sbam_layout.h): the null pass sizes the buffer, the second pass carves it.
template <class F>
hipError_t carve(DevBuf<uint8_t> &buf, bool *grew, F &&layout) {
  Carve size(nullptr);
  layout(size);
  HIPTRY(buf.ensure(size.bytes(), grew));
  Carve k(buf.get());
  layout(k);
  return hipSuccess;
}

StreamView view(sbam_ctx *c) {
  return StreamView{c->d_u, c->L, c->d_lens, c->nref, (c->base + c->D >= c->file_size) ? 1 : 0};
}

// ---- stage state -----------------------------------------------------------------------------------
// What a check left in d_bitmap; dropped by whatever changes the stream or the checker's inputs under it.
// first_halo: the smallest position of [x0, x1) whose call is unknown on a shard (-1: none).  Its bit and those of
// later unknown positions are clear like a failure's, so the bitmap counts as covering the range only below it: the
// consumers evaluate what lies behind themselves (k_find_record_starts, split_counts' walk), and those answer HALO.
void set_bitmap(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, bool list_form, int64_t first_halo = -1) {
  c->bm_x0 = x0 & ~(int64_t)63;
  c->bm_x1 = first_halo >= 0 && first_halo < x1 ? first_halo : x1;
  c->bm_R = R;
  c->bm_list = list_form;
  c->bm_valid = true;
}
void drop_bitmap(sbam_ctx *c) { c->bm_valid = c->bm_list = c->rp_fetch = false; }

// The stages a context can hold, in the order they are made: candidates -> table -> stream -> {crc, bitmap, records},
// records -> {fields, tags, index, written, sorted}.  (The table comes from the followed hops, or from the candidates; a
// context can hold one without the candidates, never a later stage without the table.)  A producer drops its own
// stage, and with it everything made from it, before it touches a buffer (drop_from), and sets its stage's validity
// field as its last step; nothing else clears one.
enum Stage { kCandidates, kTable, kStream, kCrc, kBitmap, kRecords, kFields, kTags, kIndex, kWritten, kSorted };
bool any_stage_ran(const sbam_ctx *c) { return c->ncand >= 0 || c->blk.n >= 0 || c->L >= 0 || c->n_loaded >= 0; }
// Returns the table mirror's invalidate() (a wait for a copy in flight), hipSuccess for every other stage.
hipError_t drop_from(sbam_ctx *c, Stage from) {
  const bool stream = from <= kStream, records = stream || from == kRecords;
  if (from == kCandidates) c->ncand = -1;
  const hipError_t e = from <= kTable ? c->blk.invalidate() : hipSuccess;
  if (from <= kTable) c->sp_followed = c->sp_fell_back = 0, c->sp_segments = 0;
  if (stream) c->L = c->inflate_slow = -1;
  if (stream || from == kCrc) c->crc_b0 = c->crc_b1 = -1;
  if (stream || from == kBitmap) drop_bitmap(c);
  if (records) c->n_loaded = -1, c->loaded_all = false;
  if (records || from == kFields) c->f_n = -1;
  if (records || from == kTags) c->t_n = -1;
  if (records || from == kIndex) c->idx_built = false;
  if (records || from == kWritten) c->w.ubytes = -1;
  if (records || from == kSorted) c->sorted = false;
  return e;
}

// ---- one size rule per stage ---------------------------------------------------------------------------
// Each stage sizes its buffers here from its natural sizes, and sbam_reserve calls the same functions with its
// estimates, so a reserved context's stages find every buffer large enough.  *grew: an existing buffer was replaced.
int64_t scan_chunks(int64_t comp_bytes) { return (comp_bytes + kScanChunk - 1) / kScanChunk; }
hipError_t ensure_scan(sbam_ctx *c, int64_t comp_bytes, bool *grew = nullptr) {
  const int64_t nchunks = scan_chunks(comp_bytes);
  HIPTRY(c->d_cc.ensure(nchunks, grew));
  HIPTRY(c->d_coff.ensure(nchunks, grew));
  return c->d_slots.ensure((size_t)nchunks * kScanSlots, grew);
}
// the followed table of comp_bytes: its segments' words, and their rows in the scan's slots
hipError_t ensure_follow(sbam_ctx *c, int64_t nseg, bool *grew = nullptr, FollowSegs *fs = nullptr) {
  HIPTRY(c->d_slots.ensure((size_t)nseg * kFollowSlots, grew));
  FollowSegs r;
  return carve(c->d_fseg, grew, [&](Carve &k) { (fs ? *fs : r) = follow_segs<FollowSegs>(k, (size_t)nseg); });
}
hipError_t ensure_table(sbam_ctx *c, int64_t nb, bool *grew = nullptr) {
  HIPTRY(c->d_bstart.ensure(nb + 1, grew));
  HIPTRY(c->d_bh.ensure(nb + 1, grew));
  HIPTRY(c->d_bc.ensure(nb + 1, grew));
  HIPTRY(c->d_bu.ensure(nb + 1, grew));
  return c->d_buoff.ensure(nb + 1 + (nb + 255) / 256, grew);  // (+ launch_gather_blocks' per-workgroup sums)
}
hipError_t ensure_inflate(sbam_ctx *c, int64_t L, int64_t nb, bool *grew = nullptr) {
  HIPTRY(c->d_u.ensure((size_t)L + kStreamPad, grew));
  HIPTRY(c->d_status.ensure(nb, grew));
  HIPTRY(c->d_found.ensure(nb, grew));
  // token pool (TokPool): main regions at 1 B per output byte, the arena for blocks that need more
  HIPTRY(c->d_pool.ensure(inflate_token_bytes(L, nb), grew));
  HIPTRY(c->arena.ensure(inflate_arena_bytes(L), grew));
  HIPTRY(c->d_tokbase.ensure(nb, grew));
  HIPTRY(c->d_slow.ensure(2 * nb, grew));  // (the exact decoder's list, then the stored-only list)
  return c->d_icnt.ensure(4);
}
// the CRC check's computed and stored values, one per block of the table
hipError_t ensure_crc(sbam_ctx *c, int64_t nb, bool *grew = nullptr) {
  HIPTRY(c->d_crc.ensure((size_t)nb, grew));
  return c->d_crcst.ensure((size_t)nb, grew);
}
// bitmap words covering [x0 & ~63, x1)
hipError_t ensure_bitmap(sbam_ctx *c, int64_t x0, int64_t x1, bool *grew = nullptr) {
  return c->d_bitmap.ensure((size_t)((x1 - (x0 & ~(int64_t)63) + 63) / 64) + 1, grew);
}
// (the full check: the bitmap and the record-0 pass's per-tile counts; + 8: an unaligned x0 may add a tile)
hipError_t ensure_check(sbam_ctx *c, int64_t x0, int64_t x1, bool *grew = nullptr) {
  HIPTRY(ensure_bitmap(c, x0, x1, grew));
  return c->d_tcnt.ensure((size_t)(4 * check_tiles(x0, x1) + 8), grew);
}
hipError_t ensure_chain_list(sbam_ctx *c, size_t n, bool *grew = nullptr) {
  HIPTRY(c->d_plist.ensure(n, grew));
  HIPTRY(c->d_pfb.ensure(n, grew));
  HIPTRY(c->d_pok.ensure(n, grew));
  return c->d_nfb.ensure(3);
}
// loadReads' N records: the offset column, and record_cols in one arena, carved into *cols
hipError_t ensure_record_columns(sbam_ctx *c, size_t N, bool *grew = nullptr, RecordColumnsDev *cols = nullptr) {
  HIPTRY(c->d_roff.ensure(N, grew));
  RecordColumnsDev r;
  return carve(c->d_rcols, grew, [&](Carve &k) { (cols ? *cols : r) = record_cols<RecordColumnsDev>(k, N); });
}
// byte columns of bytes[i] bytes (< 0: none) with their gather tiles (byte_col): the fields' data, the tags' bytes
hipError_t ensure_byte_columns(DevBuf<uint8_t> &buf, int ncol, const int64_t *bytes, ByteCol *o, bool *grew = nullptr) {
  return carve(buf, grew, [&](Carve &k) {
    for (int i = 0; i < ncol; i++)
      if (bytes[i] >= 0) o[i] = byte_col(k, (size_t)bytes[i], (size_t)field_gather_tiles(bytes[i]));
  });
}

// the index's per-record scratch and run heads for N records
hipError_t ensure_index(sbam_ctx *c, size_t N, bool *grew = nullptr) {
  HIPTRY(c->d_iend.ensure(N, grew));
  HIPTRY(c->d_ibin.ensure(N, grew));
  return c->d_iheads.ensure((size_t)index_blocks((int64_t)N) + 1, grew);
}

// the coordinate sort of N records (sort_bufs), carved into *b; sbam_reserve serves streamed windows and does not size
// it (as for the index)
hipError_t ensure_sort(DevBuf<uint8_t> &buf, size_t N, SortBufs *b, bool *grew = nullptr) {
  const int64_t tiles = sort_tiles((int64_t)N);
  return carve(buf, grew, [&](Carve &k) {
    *b = sort_bufs<SortBufs>(k, N, (size_t)tiles, (size_t)exclusive_scan_blocks(tiles), kSortHistWords);
  });
}

// The sort of n keys, b.keys[0] built from the columns (ref_id non-null) or already there: the histograms decide which
// passes run (none when no key is below its predecessor: the identity), and b.order receives the stable order.
// tc: the context whose timer records the keys stage (nullptr: none).  Synchronises s once, for the histograms.
hipError_t sort_run(const SortBufs &b, const int32_t *ref_id, const int32_t *pos, int64_t n, hipStream_t s, sbam_ctx *tc,
                    int64_t *out_of_order, int32_t *passes) {
  std::vector<unsigned long long> h(kSortHistWords, 0);
  {
    Timer t(tc, "sort_keys");
    HIPTRY(launch_sort_keys(ref_id, pos, n, b, s));
  }
  HIPTRY(hipMemcpyAsync(h.data(), b.hist, h.size() * 8, hipMemcpyDeviceToHost, s));
  HIPTRY(hipStreamSynchronize(s));
  *out_of_order = (int64_t)h[kSortHistWords - 1];
  int run[8], np = 0;
  for (int p = 0; p < 8 && *out_of_order; p++) {
    bool constant = false;  // one bin holds every key: the pass would move nothing
    for (int d = 0; d < 256; d++) constant |= h[p * 256 + d] == (unsigned long long)n;
    if (!constant) run[np++] = p;
  }
  *passes = np;
  if (!np) return launch_sort_identity(b.order, n, s);
  for (int j = 0; j < np; j++) HIPTRY(launch_sort_pass(b, n, run[j], j & 1, j == 0, j == np - 1, s));
  return hipSuccess;
}

// The BAM writer.  Its scratch is bounded by the batch, its results by what they hold:
//   w.u      the stream, rounded up to the gather's 8-byte stores, + kWritePad
//   w.slots  min(blocks, kWriteBatch) slots of write_slot_stride(block_bytes) bytes (the stored bound + 8, not 64 KiB),
//            + 16: only level 1 uses them
//   w.tokens write_token_records(batch) records of write_token_stride(block_bytes) bytes (a 16-bit entry per block
//            byte and one for the end of block), one per workgroup of k_deflate_dynamic's grid (at most 1024), not per
//            block: a wave is done with its record when its block is written.  Only SBAM_WRITE_DYNAMIC uses them;
//            a batch's slots and records stay below 403 MB (268 + 134 at 65 498 bytes per block)
//   w.cols   write_cols; w.start one int64 per block + 1
//   w.tsz    write_sizes of kWriteBatch blocks
//   w.file   the stored bound: ubytes + 31 per block (18 + 5 + 8) + 28; a Huffman block is never larger
bool write_level_ok(int32_t level) { return level == 0 || level == 1 || level == (1 | SBAM_WRITE_DYNAMIC); }
static_assert(kWriteDynamic == SBAM_WRITE_DYNAMIC, "the flag the kernels' launcher tests is the ABI's");
int64_t write_blocks(int64_t ubytes, int32_t block_bytes) { return (ubytes + block_bytes - 1) / block_bytes; }
hipError_t ensure_write_stream(Writer &w, int64_t ubytes) {
  return w.u.ensure((((size_t)ubytes + 7) & ~(size_t)7) + kWritePad);
}
hipError_t ensure_write_blocks(Writer &w, int64_t ubytes, int32_t block_bytes, int32_t level) {
  const int64_t nb = write_blocks(ubytes, block_bytes), batch = std::min(nb, kWriteBatch);
  if (level) HIPTRY(w.slots.ensure((size_t)(batch * write_slot_stride(block_bytes) + 16)));
  if (level & SBAM_WRITE_DYNAMIC)
    HIPTRY(w.tokens.ensure((size_t)(write_token_records(batch) * write_token_stride(block_bytes))));
  HIPTRY(carve(w.cols, nullptr, [&](Carve &k) { w.col = write_cols(k, (size_t)nb); }));
  HIPTRY(w.start.ensure((size_t)(nb + 1)));
  HIPTRY(carve(w.tsz, nullptr,
               [&](Carve &k) { w.sz = write_sizes(k, kWriteBatch, exclusive_scan_blocks(kWriteBatch)); }));
  return w.file.ensure((size_t)(ubytes + 31 * nb + 28));
}

// Deflate and frame w.u[0, ubytes) into w.file, a batch of blocks at a time; the host reads each batch's size (8 bytes)
// to place the next.  tc: the context whose timers record the stages (nullptr: none).
hipError_t writer_run(Writer &w, hipStream_t s, sbam_ctx *tc, int64_t ubytes, int32_t block_bytes, int32_t level,
                      bool with_eof) {
  HIPTRY(ensure_write_blocks(w, ubytes, block_bytes, level));
  const int64_t nb = write_blocks(ubytes, block_bytes);
  HIPTRY(hipMemsetAsync(w.sz.n_stored, 0, 8, s));
  int64_t base = 0, b0 = 0;
  do {
    const int64_t k = std::min(kWriteBatch, nb - b0);
    const WriteBlocksArgs a{w.u, ubytes, block_bytes, b0, k, w.slots, write_slot_stride(block_bytes), w.col.pay, w.col.stored,
                            w.sz.tsz, w.tokens, write_token_stride(block_bytes)};
    {
      Timer t(tc, "write_deflate");
      HIPTRY(launch_write_deflate(a, level, s));
    }
    {
      Timer t(tc, "write_frame");
      HIPTRY(launch_exclusive_scan(w.sz.tsz, k + 1, k, 1, w.sz.bsum, w.sz.tot, s));
      const WriteFrameArgs f{w.file, base, (with_eof && b0 + k >= nb) ? 1 : 0, w.start, w.col.csize, w.col.usize, w.sz.n_stored};
      HIPTRY(launch_write_frame(a, f, s));
    }
    int64_t bytes = 0;
    HIPTRY(hipMemcpyAsync(&bytes, w.sz.tot, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    base += bytes;
    b0 += k;
  } while (b0 < nb);
  unsigned long long ns = 0;
  HIPTRY(hipMemcpy(&ns, w.sz.n_stored, 8, hipMemcpyDeviceToHost));
  w.nb = nb;
  w.n_stored = (int64_t)ns;
  w.comp_bytes = base + (with_eof ? 28 : 0);
  w.block_bytes = block_bytes;
  return hipSuccess;
}

// Header.make details at relative offset q (for HeaderParseException).
int header_parse_error(sbam_ctx *c, int64_t q) {
  uint8_t h[18] = {0};
  const int64_t n = std::min<int64_t>(18, c->D - q);
  if (n > 0) (void)hipMemcpy(h, c->d_comp + q, (size_t)n, hipMemcpyDeviceToHost);
  static const int idxs[7] = {0, 1, 2, 3, 12, 13, 14};
  static const int exps[7] = {31, 139, 8, 4, 66, 67, 2};
  for (int j = 0; j < 7; j++)
    if (h[idxs[j]] != (uint8_t)exps[j]) {
      c->err.idx = idxs[j];
      c->err.actual = (int8_t)h[idxs[j]];
      c->err.expected = (int8_t)(uint8_t)exps[j];
      c->err.position = c->base + q;
      return set_err(c, SBAM_ERR_HEADER_PARSE, "Position %d: %d != %d", idxs[j], (int)(int8_t)h[idxs[j]],
                     (int)(int8_t)(uint8_t)exps[j]);
    }
  return set_err(c, SBAM_ERR_HEADER_PARSE, "header parse failure at %lld", (long long)(c->base + q));
}

// NoReadFoundException(path, start, maxReadSize) (FindRecordStart.scala:11-28, 66-71)
int no_read_found(sbam_ctx *c, int64_t start, int32_t max_read_size) {
  c->err.position = start;
  c->err.expected = max_read_size;
  return set_err(c, SBAM_ERR_NO_READ_FOUND, "Failed to find a valid read-start in %d attempts in %s from %lld",
                 max_read_size, c->path.c_str(), (long long)start);
}

// SBAM_ERR_RECORD for loaded record i, with its stream offset (the fields' and the tags' first bad record)
int bad_record(sbam_ctx *c, int64_t i, const char *what) {
  int64_t x = -1;
  HIPCHK(c, hipMemcpy(&x, c->d_roff + i, 8, hipMemcpyDeviceToHost));
  c->err.position = x;
  return set_err(c, SBAM_ERR_RECORD, "record %lld at %lld: %s", (long long)i, (long long)x, what);
}

// a scanned block table, with its host copy in c->blk's vectors
int ensure_blocks(sbam_ctx *c) {
  if (c->blk.n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_scan_blocks has not run");
  HIPCHK(c, c->blk.get());
  return SBAM_OK;
}
int ensure_stream(sbam_ctx *c) {
  if (c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_inflate has not run");
  if (c->nref < 0) return set_err(c, SBAM_ERR_STATE, "contig lengths unknown (sbam_header / sbam_set_contig_lengths)");
  return ensure_blocks(c);
}

// block index whose (relative) start == q, or -1
int64_t block_at(const sbam_ctx *c, int64_t q) {
  const std::vector<int64_t> &st = c->blk.start;
  auto it = std::lower_bound(st.begin(), st.end(), q);
  if (it == st.end() || *it != q) return -1;
  return it - st.begin();
}
sbam_pos pos_of(const sbam_ctx *c, int64_t x, int64_t *hint = nullptr) {
  // last block with uoff <= x and usize > 0 containing x; x at a block end normalises to (next, 0).  hint: the block
  // of the previous (smaller) query — the search gallops from it (split starts ascend: 4767 full binary searches
  // over a 3 MB table were 0.2 ms of host time per 10 GB step)
  const BlockMirror &t = c->blk;
  int64_t lo = 0, hi = t.n;
  if (hint && *hint >= 0 && *hint < t.n && t.uoff[*hint] <= x) {
    int64_t step = 1;
    lo = *hint;
    while (lo + step < t.n && t.uoff[lo + step] <= x) {
      lo += step;
      step *= 2;
    }
    hi = std::min(lo + step, t.n);
  }
  auto it = std::upper_bound(t.uoff.begin() + lo, t.uoff.begin() + hi, x);
  int64_t b = (it - t.uoff.begin()) - 1;
  if (hint && b >= 0) *hint = b;
  while (b >= 0 && b < t.n && x >= t.uoff[b] + t.usize[b]) b++;
  if (b < 0 || b >= t.n) {
    const int64_t endp = t.n > 0 ? t.start[t.n - 1] + t.csize[t.n - 1] : 0;
    return sbam_pos{c->base + endp, 0, 0};
  }
  return sbam_pos{c->base + t.start[b], (int32_t)(x - t.uoff[b]), 0};
}

}  // namespace

extern "C" {

const char *sbam_version(void) { return "sbam-mi355x 0.1 (gfx950)"; }

int sbam_open(int device, const uint8_t *data, int64_t len, int64_t base_offset, int64_t file_size, sbam_ctx **out) {
  if (!out || (!data && len > 0) || len < 0 || base_offset < 0 || file_size < base_offset + len) return SBAM_ERR_ARG;
  sbam_ctx *c = new sbam_ctx();
  *out = c;
  c->device = device;
  c->D = len;
  c->base = base_offset;
  c->file_size = file_size;
  HIPCHK(c, hipSetDevice(device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(c, c->d_comp.ensure((size_t)len + kCompPad));
  HIPCHK(c, hipMemsetAsync(c->d_comp + len, 0, kCompPad, c->stream));
  if (len) HIPCHK(c, hipMemcpyAsync(c->d_comp, data, (size_t)len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, c->d_small.ensure(sizeof(Scratch) / 8));
  HIPCHK(c, carve(c->d_counts, nullptr, count_words<CountsDev>));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

void sbam_close(sbam_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->blk.copy_stream) (void)hipStreamSynchronize(c->blk.copy_stream);
  for (auto &kv : c->ev) {
    (void)hipEventDestroy(kv.second.first);
    (void)hipEventDestroy(kv.second.second);
  }
  for (hipEvent_t e : c->load_ev)
    if (e) (void)hipEventDestroy(e);
  c->blk.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // (the device buffers free themselves: this context's device is current, its streams were idle)
}

const sbam_error *sbam_last_error(const sbam_ctx *c) { return c ? &c->err : nullptr; }

int sbam_set_path(sbam_ctx *c, const char *path) {
  if (!c || !path) return SBAM_ERR_ARG;
  c->path = path;
  return SBAM_OK;
}

int sbam_load(sbam_ctx *c, const uint8_t *data, int64_t len, int64_t base_offset, int64_t file_size) {
  if (!c || (!data && len > 0) || len < 0 || base_offset < 0 || file_size < base_offset + len) return SBAM_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the previous window's work is done with d_comp
  HIPCHK(c, c->d_comp.ensure((size_t)len + kCompPad));
  HIPCHK(c, hipMemsetAsync(c->d_comp + len, 0, kCompPad, c->stream));
  // in 8 MiB pieces with at most kInFlight queued: a multi-GB copy queued whole would hold the copy engine, and the
  // small copies of another context's kernels running meanwhile (results, tables) would wait behind it
  // (tools/e2e_probe.py: a window's compute 56 -> 98 ms while the next window's 2.5 GB copy ran); a few pieces in
  // flight keep the engine busy without a host round trip between pieces
  constexpr int64_t kPiece = 8ll << 20;
  constexpr int kInFlight = 3;
  for (hipEvent_t &e : c->load_ev)
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int64_t k = 0;
  for (int64_t o = 0; o < len; o += kPiece, k++) {
    if (k >= kInFlight) HIPCHK(c, hipEventSynchronize(c->load_ev[(k - kInFlight) % 4]));
    const int64_t n = std::min(kPiece, len - o);
    HIPCHK(c, hipMemcpyAsync(c->d_comp + o, data + o, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->load_ev[k % 4], c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // another file (or a range from its start): its contig lengths must come from sbam_header /
  // sbam_set_contig_lengths again; a later window of the same file keeps them
  if (base_offset == 0 || file_size != c->file_size) c->nref = -1;
  c->D = len;
  c->base = base_offset;
  c->file_size = file_size;
  return sbam_reset(c);
}

int sbam_reserve(sbam_ctx *c, int64_t comp_bytes, int64_t n_blocks, int64_t ubytes, int64_t n_records) {
  if (!c || comp_bytes < 0 || n_blocks < 0 || ubytes < 0 || n_records < 0) return SBAM_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->blk.copy_stream) HIPCHK(c, hipStreamSynchronize(c->blk.copy_stream));
  if ((size_t)comp_bytes + kCompPad > c->d_comp.size()) {  // keep the resident bytes (sbam_load replaces them anyway)
    DevBuf<uint8_t> p;
    HIPCHK(c, p.ensure((size_t)comp_bytes + kCompPad));
    if (c->D + kCompPad > 0) HIPCHK(c, hipMemcpy(p, c->d_comp, (size_t)c->D + kCompPad, hipMemcpyDeviceToDevice));
    c->d_comp.swap(p);
  }
  // Any stage buffer that grows is a fresh allocation whose contents are gone, so a context that has already run a
  // stage drops its stages (sbam_reset) when one grows: a later query re-runs them instead of reading uninitialised
  // device memory.  The resident compressed bytes and the contig lengths are kept.
  bool grew = false;
  HIPCHK(c, ensure_scan(c, comp_bytes, &grew));
  HIPCHK(c, ensure_follow(c, follow_segments(comp_bytes, 0), &grew));
  // candidates: every block's header plus the rare false positives inside payloads
  HIPCHK(c, c->d_cand.ensure((size_t)(n_blocks + n_blocks / 8 + 1024), &grew));
  HIPCHK(c, ensure_table(c, n_blocks, &grew));
  HIPCHK(c, ensure_inflate(c, ubytes, n_blocks, &grew));
  HIPCHK(c, ensure_check(c, 0, ubytes, &grew));
  if (n_records > 0) {  // the chain pass's PASS0 list (about one entry per record) and loadReads' columns
    const size_t n = (size_t)(n_records + n_records / 8 + 4096);
    HIPCHK(c, ensure_chain_list(c, n, &grew));
    HIPCHK(c, ensure_record_columns(c, n, &grew));
  }
  if (grew && any_stage_ran(c)) return sbam_reset(c);
  return SBAM_OK;
}

int sbam_reset(sbam_ctx *c) {
  if (!c) return SBAM_ERR_ARG;
  const hipError_t e = drop_from(c, kCandidates);
  c->err = sbam_error{};
  HIPCHK(c, e);
  return SBAM_OK;
}

double sbam_last_kernel_ms(sbam_ctx *c, const char *kernel) {
  if (!std::strcmp(kernel, "record_tags")) {  // two spans with the host's look at the totals between them
    const double walk = sbam_last_kernel_ms(c, "record_tag_walk"), bytes = sbam_last_kernel_ms(c, "record_tag_bytes");
    return walk < 0 ? -1.0 : walk + (bytes < 0 ? 0.0 : bytes);
  }
  auto it = c->ev.find(kernel);
  if (it == c->ev.end()) return -1.0;
  (void)hipEventSynchronize(it->second.second);
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, it->second.first, it->second.second) != hipSuccess) return -1.0;
  return ms;
}

// ---- candidates (scan) ---------------------------------------------------------------------------
static int scan_candidates(sbam_ctx *c) {
  if (c->ncand >= 0) return SBAM_OK;
  Timer t(c, "scan");
  const int64_t nchunks = scan_chunks(c->D);
  HIPCHK(c, ensure_scan(c, c->D));
  // one pass into per-chunk slots (+ counts, exact even past the slots)
  HIPCHK(c, launch_scan_slots(c->d_comp, c->D, c->d_cc, nchunks, c->d_slots, SMALL(c, scan_overflow), c->stream));
  HIPCHK(c, launch_scan_sums(c->d_cc, c->d_coff, nchunks, 1, SMALL(c, scan_total), c->stream));
  int64_t tot_ovf[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(tot_ovf, SMALL(c, scan_total), 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t total = tot_ovf[0];
  HIPCHK(c, c->d_cand.ensure(total));
  if (tot_ovf[1] == 0) {
    HIPCHK(c, launch_scan_compact(c->d_slots, c->d_cc, c->d_coff, nchunks, c->d_cand, c->stream));
  } else {  // a chunk with more than kScanSlots candidates (blocks under 2 KiB): the exact second pass
    HIPCHK(c, launch_scan_write(c->d_comp, c->D, c->d_coff, nchunks, c->d_cand, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ncand = total;
  return SBAM_OK;
}

// ---- the table without candidates (follow) -----------------------------------------------------------
// SBAM_SCAN_FOLLOW=0: build every table from the byte scan (tests and A/B runs of the two paths)
static bool follow_enabled() {
  const char *e = std::getenv("SBAM_SCAN_FOLLOW");
  return !(e && *e == '0');
}

// The block table from start_rel by following the BSIZE hops in parallel segments.  *nb: its blocks, with the device
// columns built and the host's copy queued as after the fast chain; -1 when the segments' chains do not join up into
// one accepted table (sp_fell_back is set, nothing else is changed, and the caller runs the byte scan).
static int follow_blocks(sbam_ctx *c, int64_t start_rel, int64_t *nb) {
  const int64_t nseg = follow_segments(c->D, start_rel);
  FollowSegs fs;
  unsigned long long v[3] = {0, 0, 0};  // first unusable segment, first stopped segment, rows up to the stop
  {
    Timer t(c, "scan");
    HIPCHK(c, ensure_follow(c, nseg, nullptr, &fs));
    HIPCHK(c, launch_follow_blocks(c->d_comp, c->D, start_rel, nseg, fs, c->d_slots, SMALL(c, follow_bad), c->stream));
    HIPCHK(c, launch_scan_sums(fs.cnt, fs.off, nseg, 1, SMALL(c, follow_total), c->stream));
    HIPCHK(c, hipMemcpyAsync(v, SMALL(c, follow_bad), sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the one round trip: the table's size)
  }
  c->sp_segments = nseg;
  if (!(v[1] < v[0])) {  // no stop before the first segment that cannot be used
    c->sp_fell_back = 1;
    *nb = -1;
    return SBAM_OK;
  }
  const int64_t n = (int64_t)v[2];
  Timer t(c, "chain");
  HIPCHK(c, c->d_cand.ensure((size_t)n));  // (no candidate list lives there: ncand < 0)
  HIPCHK(c, ensure_table(c, n));
  HIPCHK(c, launch_follow_compact(c->d_slots, fs, nseg, c->d_cand, c->stream));
  HIPCHK(c, launch_gather_blocks(c->d_cand, 0, n, c->d_bstart, c->d_bh, c->d_bc, c->d_bu, c->d_buoff + n + 1,
                                 c->d_buoff, c->stream));
  HIPCHK(c, c->blk.start_copy(c->d_bstart, c->d_buoff, c->d_bc, c->d_bu, n, c->stream));
  c->sp_followed = 1;
  *nb = n;
  return SBAM_OK;
}

int sbam_follow_segment_bytes(void) { return kFollowSeg; }

int sbam_scan_path(sbam_ctx *c, int32_t *followed, int32_t *fell_back, int64_t *segments) {
  if (!c) return SBAM_ERR_ARG;
  if (followed) *followed = c->sp_followed;
  if (fell_back) *fell_back = c->sp_fell_back;
  if (segments) *segments = c->sp_segments;
  return SBAM_OK;
}

int sbam_find_block_starts(sbam_ctx *c, const int64_t *starts, int64_t n, int32_t nchk, int64_t *out) {
  if (!c || (!starts && n) || (!out && n) || nchk < 0) return SBAM_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int64_t> rel(n);
  for (int64_t i = 0; i < n; i++) {
    rel[i] = starts[i] - c->base;
    if (rel[i] < 0 || rel[i] > c->D) return set_err(c, SBAM_ERR_ARG, "split start %lld outside loaded bytes", (long long)starts[i]);
  }
  HIPCHK(c, c->d_qa.ensure((size_t)n));
  HIPCHK(c, c->d_qb.ensure((size_t)n));
  int64_t *d_q = c->d_qa, *d_o = c->d_qb;
  HIPCHK(c, hipMemcpyAsync(d_q, rel.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  if (c->ncand >= 0)  // a candidate list exists: search it
    HIPCHK(c, launch_find_block_starts(c->D, c->d_cand, c->ncand, d_q, n, nchk, d_o, c->stream));
  else  // none (the table was followed, or nothing has run): the same rules on the bytes behind each start
    HIPCHK(c, launch_find_block_starts_bytes(c->d_comp, c->D, d_q, n, nchk, d_o, c->stream));
  HIPCHK(c, hipMemcpyAsync(out, d_o, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; i++) {
    if (out[i] < 0) {
      // HeaderSearchFailedException(path, start, positionsAttempted = MAX_BLOCK_SIZE) (FindBlockStart.scala:16-35)
      c->err.position = starts[i];
      c->err.actual = 65536;
      return set_err(c, SBAM_ERR_HEADER_SEARCH, "%s: failed to find BGZF header in %d bytes from %lld",
                     c->path.c_str(), 65536, (long long)starts[i]);
    }
    out[i] += c->base;
  }
  return SBAM_OK;
}

int sbam_scan_blocks(sbam_ctx *c, int64_t *n_blocks) {
  if (!c) return SBAM_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kTable));  // (no table, and nothing made from one, until this scan has built one)
  int rc = SBAM_OK;
  int64_t start_rel = 0;
  if (c->base > 0) {  // a shard starts at the first block at/after its first byte
    int64_t s = c->base, o = 0;
    rc = sbam_find_block_starts(c, &s, 1, 5, &o);
    if (rc) return rc;
    start_rel = o - c->base;
  }
  if (c->ncand < 0 && follow_enabled()) {  // no candidate list yet: the table needs none
    int64_t nb = -1;
    rc = follow_blocks(c, start_rel, &nb);
    if (rc) return rc;
    if (nb >= 0) {
      if (n_blocks) *n_blocks = nb;
      return SBAM_OK;
    }
  }
  // today's exact path, from the start: the candidates of every byte offset, then their chain
  rc = scan_candidates(c);
  if (rc) return rc;
  Timer t(c, "chain");
  int64_t first = 0;
  HIPCHK(c, launch_lower_bound(c->d_cand, c->ncand, start_rel, SMALL(c, table_first), c->stream));
  HIPCHK(c, hipMemcpyAsync(&first, SMALL(c, table_first), sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int64_t nb = 0;
  bool fast = true;
  if (start_rel + 18 > c->D) {
    nb = 0;  // EOF before the first header: empty stream
  } else {
    Candidate c0{};
    if (first < c->ncand) HIPCHK(c, hipMemcpy(&c0, c->d_cand + first, sizeof(Candidate), hipMemcpyDeviceToHost));
    if (first >= c->ncand || c0.pos != start_rel) return header_parse_error(c, start_rel);
    const unsigned long long none = ~0ull;
    HIPCHK(c, hipMemcpyAsync(SMALL(c, chain_stop), &none, sizeof(none), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_chain_verify(c->d_cand, c->ncand, first, c->D, SMALL(c, chain_stop), c->stream));
    unsigned long long stop = 0;
    HIPCHK(c, hipMemcpyAsync(&stop, SMALL(c, chain_stop), sizeof(stop), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t si = (int64_t)(stop >> 2);
    const int code = (int)(stop & 3);
    if (code == 1) nb = si - first;
    else if (code == 2) nb = si - first + 1;
    else fast = false;  // a candidate that is not the next header: walk exactly on the host
  }
  if (fast) {
    // columns and offsets built on the device; the host's copy is queued behind them, not waited for
    HIPCHK(c, ensure_table(c, nb));
    HIPCHK(c, launch_gather_blocks(c->d_cand, first, nb, c->d_bstart, c->d_bh, c->d_bc, c->d_bu, c->d_buoff + nb + 1,
                                   c->d_buoff, c->stream));
    HIPCHK(c, c->blk.start_copy(c->d_bstart, c->d_buoff, c->d_bc, c->d_bu, nb, c->stream));
  } else {
    std::vector<Candidate> hc(c->ncand);
    HIPCHK(c, hipMemcpy(hc.data(), c->d_cand, c->ncand * sizeof(Candidate), hipMemcpyDeviceToHost));
    int64_t q = start_rel, i = first;
    std::vector<int64_t> st;
    std::vector<int32_t> hs, cs, us;
    for (;;) {  // MetadataStream._advance, exactly (MetadataStream.scala:23-54)
      if (q + 18 > c->D) break;
      while (i < c->ncand && hc[i].pos < q) i++;
      if (i >= c->ncand || hc[i].pos != q) return header_parse_error(c, q);
      const Candidate &k = hc[i];
      if (!(k.flags & CAND_ISIZE) || (k.flags & CAND_EMPTY)) break;
      st.push_back(k.pos);
      cs.push_back(k.csize);
      us.push_back(k.isize);
      hs.push_back(k.hsize);
      q += k.csize;
    }
    nb = (int64_t)st.size();
    HIPCHK(c, ensure_table(c, nb));
    HIPCHK(c, hipMemcpy(c->d_bstart, st.data(), nb * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bh, hs.data(), nb * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bc, cs.data(), nb * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bu, us.data(), nb * 4, hipMemcpyHostToDevice));
    BlockMirror &t = c->blk;
    t.fill(std::move(st), std::move(cs), std::move(us));
    HIPCHK(c, hipMemcpyAsync(c->d_buoff, t.uoff.data(), (nb + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n_blocks) *n_blocks = nb;
  return SBAM_OK;
}

int sbam_get_blocks(sbam_ctx *c, int64_t *start, int32_t *csize, int32_t *usize, int64_t *uoff, int64_t cap) {
  if (!c) return SBAM_ERR_ARG;
  int rc = ensure_blocks(c);
  if (rc) return rc;
  const BlockMirror &t = c->blk;
  if (cap < t.n) return set_err(c, SBAM_ERR_ARG, "capacity %lld < %lld blocks", (long long)cap, (long long)t.n);
  for (int64_t b = 0; b < t.n; b++) {
    if (start) start[b] = c->base + t.start[b];
    if (csize) csize[b] = t.csize[b];
    if (usize) usize[b] = t.usize[b];
    if (uoff) uoff[b] = t.uoff[b];
  }
  return SBAM_OK;
}

static int run_crc(sbam_ctx *c, int64_t L, int64_t b0, int64_t b1, unsigned long long bad[2]);

int sbam_inflate(sbam_ctx *c, int64_t *usz) {
  if (!c) return SBAM_ERR_ARG;
  if (c->blk.n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_scan_blocks has not run");
  HIPCHK(c, hipSetDevice(c->device));
  int64_t L = 0;
  HIPCHK(c, c->blk.total(&L));  // (the table's host copy is picked up below, while the decoder runs)
  const int64_t nb = c->blk.n;
  HIPCHK(c, drop_from(c, kStream));  // (no stream, and nothing made from one, until this call has decoded one)
  HIPCHK(c, ensure_inflate(c, L, nb));
  HIPCHK(c, hipMemsetAsync(c->d_u + L, 0, kStreamPad, c->stream));
  int32_t *d_status = c->d_status, *d_found = c->d_found;
  const unsigned long long none = ~0ull;
  BlockTable bt{c->d_bstart, c->d_bh, c->d_bc, c->d_bu, c->d_buoff, nb};
  unsigned long long *d_used = USMALL(c, arena_used), *d_ferr = USMALL(c, inflate_error);
  unsigned long long ferr = 0;
  unsigned int cnt3[3] = {0, 0, 0};  // slow-path blocks, -, blocks the resolver handed back
  for (;;) {
    const TokPool tp{c->d_pool, c->arena.buf, (int64_t)c->arena.usable(), d_used, c->d_tokbase};
    HIPCHK(c, hipMemsetAsync(c->d_tokbase, 0xff, nb * sizeof(int64_t), c->stream));  // every block: main region
    HIPCHK(c, hipMemsetAsync(d_used, 0, sizeof(unsigned long long), c->stream));
    {
      Timer t(c, "inflate");
      {
        Timer t1(c, "inflate_decode");
        HIPCHK(c, launch_inflate_decode(c->d_comp, c->D, bt, tp, c->d_u, d_status, d_found, c->d_slow, c->d_icnt, c->stream));
      }
      Timer t2(c, "inflate_resolve");
      // (the slow list is consumed by now: the resolver's redo list reuses d_slow, its count is d_icnt[2])
      HIPCHK(c, launch_inflate_resolve(bt, c->d_u, tp, d_found, nullptr, 0, c->d_slow, c->d_icnt + 2, c->stream));
    }
    // the table's host copy, while the kernels run (before the copies of the results below: copies into pageable
    // memory wait for the stream)
    HIPCHK(c, c->blk.get());
    HIPCHK(c, hipMemcpyAsync(d_ferr, &none, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_first_error(d_status, nb, d_ferr, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ferr, d_ferr, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt3, c->d_icnt, 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cnt3[2] > 0) {  // a distance past its block's start ("invalid distance too far back"): the exact decoder
      HIPCHK(c, launch_inflate_redo(c->d_comp, c->D, bt, tp, c->d_slow, c->d_icnt, d_status, d_found, c->stream));
      HIPCHK(c, launch_inflate_resolve(bt, c->d_u, tp, d_found, c->d_slow, cnt3[2], nullptr, nullptr, c->stream));
      HIPCHK(c, hipMemcpyAsync(d_ferr, &none, 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, launch_first_error(d_status, nb, d_ferr, c->stream));
      HIPCHK(c, hipMemcpyAsync(&ferr, d_ferr, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (ferr == ~0ull) break;
    int32_t st = 0;
    unsigned long long used = 0;
    HIPCHK(c, hipMemcpy(&st, d_status + ferr, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&used, d_used, 8, hipMemcpyDeviceToHost));
    if (st != 3 /* INF_OVERFLOW */ || used <= c->arena.usable()) break;
    // the arena was too small for the blocks that needed it (used counts every request): grow it, inflate again
    if (log_grow()) std::fprintf(stderr, "[sbam] token arena %zu -> %llu bytes\n", c->arena.usable(), used);
    HIPCHK(c, c->arena.ensure((size_t)used + (used >> 3)));
  }
  if (ferr != ~0ull) {
    int32_t found = 0;
    HIPCHK(c, hipMemcpy(&found, d_found + ferr, 4, hipMemcpyDeviceToHost));
    c->err.position = c->base + c->blk.start[ferr];
    c->err.expected = c->blk.usize[ferr];
    c->err.actual = found;
    return set_err(c, SBAM_ERR_INFLATE, "Expected %d decompressed bytes, found %d", c->blk.usize[ferr], found);
  }
  if (c->verify_crc) {  // htslib's bgzf check: every block's inflated bytes against its footer, before the stream is set
    unsigned long long bad[2];
    const int rc = run_crc(c, L, 0, nb, bad);
    if (rc) return rc;
    if (bad[0]) {
      const int64_t b = (int64_t)bad[1];
      uint32_t got = 0, want = 0;
      HIPCHK(c, hipMemcpy(&got, c->d_crc + b, 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&want, c->d_crcst + b, 4, hipMemcpyDeviceToHost));
      c->err.position = c->base + c->blk.start[b];
      c->err.expected = want;
      c->err.actual = got;
      return set_err(c, SBAM_ERR_CRC, "CRC32 mismatch in block at %lld: footer %08x, computed %08x",
                     (long long)c->err.position, want, got);
    }
    c->crc_b0 = 0;
    c->crc_b1 = nb;
  }
  c->inflate_slow = cnt3[0] + cnt3[2];
  c->L = L;
  if (usz) *usz = L;
  return SBAM_OK;
}

// ---- CRC32 check ------------------------------------------------------------------------------------
// blocks [b0, b1) of the table against their footers, over the stream of L bytes in d_u; bad[0] = mismatches,
// bad[1] = the first one's table index (~0: none)
static int run_crc(sbam_ctx *c, int64_t L, int64_t b0, int64_t b1, unsigned long long bad[2]) {
  const int64_t nb = c->blk.n;
  HIPCHK(c, ensure_crc(c, nb));
  unsigned long long *d_bad = USMALL(c, crc_bad);  // (and crc_first_bad behind it)
  bad[0] = 0;
  bad[1] = ~0ull;
  HIPCHK(c, hipMemcpyAsync(d_bad, bad, 16, hipMemcpyHostToDevice, c->stream));
  {
    Timer t(c, "crc");
    const BlockTable bt{c->d_bstart, c->d_bh, c->d_bc, c->d_bu, c->d_buoff, nb};
    HIPCHK(c, launch_block_crc(c->d_comp, c->D, c->d_u, L, bt, b0, b1, c->d_crc, c->d_crcst, d_bad, d_bad + 1,
                               c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(bad, d_bad, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_set_verify_crc(sbam_ctx *c, int32_t on) {
  if (!c) return SBAM_ERR_ARG;
  c->verify_crc = on != 0;
  return SBAM_OK;
}

int sbam_check_crc(sbam_ctx *c, int64_t b0, int64_t b1, sbam_crc_totals *totals) {
  if (!c) return SBAM_ERR_ARG;
  if (c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_inflate has not run");
  int rc = ensure_blocks(c);
  if (rc) return rc;
  const int64_t nb = c->blk.n;
  if (b1 < 0) b1 = nb;
  if (b0 < 0 || b0 > b1 || b1 > nb)
    return set_err(c, SBAM_ERR_ARG, "blocks [%lld, %lld) outside the table of %lld", (long long)b0, (long long)b1,
                   (long long)nb);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kCrc));
  unsigned long long bad[2];
  rc = run_crc(c, c->L, b0, b1, bad);
  if (rc) return rc;
  c->crc_b0 = b0;
  c->crc_b1 = b1;
  if (totals) {
    totals->n_blocks = b1 - b0;
    totals->n_bad = (int64_t)bad[0];
    totals->first_bad = bad[1] == ~0ull ? -1 : (int64_t)bad[1];
    totals->bytes = c->blk.uoff[b1] - c->blk.uoff[b0];
  }
  return SBAM_OK;
}

int sbam_get_block_crcs(sbam_ctx *c, int64_t b0, int64_t n, uint32_t *computed, uint32_t *stored) {
  if (!c || b0 < 0 || n < 0) return SBAM_ERR_ARG;
  if (c->L < 0 || c->crc_b0 < 0) return set_err(c, SBAM_ERR_STATE, "sbam_check_crc has not run");
  if (b0 < c->crc_b0 || b0 + n > c->crc_b1)
    return set_err(c, SBAM_ERR_STATE, "blocks [%lld, %lld) outside the checked range [%lld, %lld)", (long long)b0,
                   (long long)(b0 + n), (long long)c->crc_b0, (long long)c->crc_b1);
  HIPCHK(c, hipSetDevice(c->device));
  if (n && computed) HIPCHK(c, hipMemcpy(computed, c->d_crc + b0, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (n && stored) HIPCHK(c, hipMemcpy(stored, c->d_crcst + b0, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

int sbam_inflate_fallbacks(sbam_ctx *c, int64_t *n) {
  if (!c || !n) return SBAM_ERR_ARG;
  if (c->L < 0 || c->inflate_slow < 0) return set_err(c, SBAM_ERR_STATE, "sbam_inflate has not run");
  *n = c->inflate_slow;
  return SBAM_OK;
}

int sbam_read_uncompressed(sbam_ctx *c, int64_t off, int64_t len, uint8_t *out) {
  if (!c || off < 0 || len < 0) return SBAM_ERR_ARG;
  if (c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_inflate has not run");
  if (off + len > c->L) return set_err(c, SBAM_ERR_ARG, "range past the stream end");
  HIPCHK(c, hipSetDevice(c->device));
  if (len) HIPCHK(c, hipMemcpy(out, c->d_u + off, (size_t)len, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

int sbam_pos_to_offset(sbam_ctx *c, sbam_pos p, int64_t *off) {
  if (!c || !off) return SBAM_ERR_ARG;
  int rc = ensure_blocks(c);
  if (rc) return rc;
  const int64_t b = block_at(c, p.block_pos - c->base);
  if (b < 0 || p.offset < 0 || p.offset > c->blk.usize[b]) return set_err(c, SBAM_ERR_ARG, "no block at %lld", (long long)p.block_pos);
  *off = c->blk.uoff[b] + p.offset;
  return SBAM_OK;
}

int sbam_offset_to_pos(sbam_ctx *c, int64_t off, sbam_pos *p) {
  if (!c || !p) return SBAM_ERR_ARG;
  int rc = ensure_blocks(c);
  if (rc) return rc;
  *p = pos_of(c, off);
  return SBAM_OK;
}

// ---- BAM header -----------------------------------------------------------------------------------
int sbam_set_contig_lengths(sbam_ctx *c, int32_t n_ref, const int64_t *lengths) {
  if (!c || n_ref < 0 || (n_ref && !lengths)) return SBAM_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_lens.ensure((size_t)n_ref));
  // The device table holds the lengths clamped to [-2, INT32_MAX] (h_lens keeps the caller's values).  The kernels
  // ask only refPos > length for an int32 refPos >= -1 (refPos < -1 is decided before the length is looked at,
  // PosChecker.scala:43-63), which the clamp leaves unchanged for every int64 length, and the record-0 kernels keep
  // the table as int32 in LDS.
  std::vector<int64_t> clamped(lengths, lengths + n_ref);
  for (int64_t &v : clamped) v = v < -2 ? -2 : v > INT32_MAX ? INT32_MAX : v;
  if (n_ref) HIPCHK(c, hipMemcpyAsync(c->d_lens, clamped.data(), n_ref * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->h_lens.assign(lengths, lengths + n_ref);
  c->nref = n_ref;
  c->header_x = -1;
  drop_bitmap(c);
  return SBAM_OK;
}

int sbam_header(sbam_ctx *c, int32_t *n_ref, int64_t *lengths, int32_t cap, sbam_pos *end_pos) {
  if (!c) return SBAM_ERR_ARG;
  if (c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_inflate has not run");
  if (c->base != 0) return set_err(c, SBAM_ERR_STATE, "header lives in the file's first block (shard: sbam_set_contig_lengths)");
  if (int rc = ensure_blocks(c)) return rc;
  auto rd = [&](int64_t off, int64_t n, void *dst) -> bool {
    if (off < 0 || off + n > c->L) return false;
    return hipMemcpy(dst, c->d_u + off, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
  };
  char magic[4];
  if (!rd(0, 4, magic) || memcmp(magic, "BAM\1", 4) != 0)
    return set_err(c, SBAM_ERR_NOT_BAM, "requirement failed");
  int32_t l_text = 0, nr = 0;
  if (!rd(4, 4, &l_text)) return set_err(c, SBAM_ERR_NOT_BAM, "truncated header");
  int64_t x = 8 + (int64_t)l_text;
  if (!rd(x, 4, &nr)) return set_err(c, SBAM_ERR_NOT_BAM, "truncated header");
  x += 4;
  std::vector<int64_t> lens;
  for (int32_t i = 0; i < nr; i++) {
    int32_t l_name = 0, l_ref = 0;
    if (!rd(x, 4, &l_name)) return set_err(c, SBAM_ERR_NOT_BAM, "truncated header");
    x += 4 + (int64_t)l_name;
    if (!rd(x, 4, &l_ref)) return set_err(c, SBAM_ERR_NOT_BAM, "truncated header");
    x += 4;
    lens.push_back(l_ref);
  }
  int rc = sbam_set_contig_lengths(c, nr, lens.data());
  if (rc) return rc;
  c->header_end = pos_of(c, x);
  c->header_x = x;
  if (n_ref) *n_ref = nr;
  if (lengths)
    for (int32_t i = 0; i < nr && i < cap; i++) lengths[i] = lens[i];
  if (end_pos) *end_pos = c->header_end;
  return SBAM_OK;
}

// Copy a device bitmap covering [x0 & ~63, x1) out as bits relative to x0.
static int copy_bitmap_out(sbam_ctx *c, int64_t x0, int64_t x1, uint64_t *out) {
  const int64_t x0a = x0 & ~(int64_t)63, sh = x0 - x0a;
  const size_t nwa = (size_t)((x1 - x0a + 63) / 64), nw = (size_t)((x1 - x0 + 63) / 64);
  if (!nw) return SBAM_OK;
  if (!sh) {
    HIPCHK(c, hipMemcpyAsync(out, c->d_bitmap, nw * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SBAM_OK;
  }
  std::vector<uint64_t> t(nwa + 1, 0);
  HIPCHK(c, hipMemcpyAsync(t.data(), c->d_bitmap, nwa * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < nw; i++) out[i] = (t[i] >> sh) | (t[i + 1] << (64 - sh));
  const int64_t tail = (x1 - x0) & 63;
  if (tail) out[nw - 1] &= (1ull << tail) - 1;
  return SBAM_OK;
}

// ---- checkers ------------------------------------------------------------------------------------
static int check_range_args(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R) {
  int rc = ensure_stream(c);
  if (rc) return rc;
  if (x0 < 0 || x1 < x0 || x1 > c->L) return set_err(c, SBAM_ERR_ARG, "range [%lld, %lld) outside stream of %lld", (long long)x0, (long long)x1, (long long)c->L);
  if (R < 0 || R > SBAM_MAX_READS_TO_CHECK) return set_err(c, SBAM_ERR_ARG, "reads_to_check %d out of range", R);
  return SBAM_OK;
}

static hipError_t run_chains(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, int32_t by_key, CountsDev cd,
                             bool *list_form, const int32_t *tile_pass0 = nullptr);

// CountsDev::first_halo for a check of this context: the scratch word set to "none" on a shard, nullptr on a whole file.
static hipError_t first_halo_begin(sbam_ctx *c, unsigned long long **out) {
  *out = nullptr;
  if (view(c).eof_real) return hipSuccess;
  *out = USMALL(c, first_halo);
  return hipMemsetAsync(*out, 0xff, 8, c->stream);
}
// ... and its value once the check has run (-1: none); the caller synchronises the stream before it reads *out.
static hipError_t first_halo_fetch(sbam_ctx *c, const unsigned long long *d, int64_t *out) {
  *out = -1;
  return d ? hipMemcpyAsync(out, d, 8, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

int sbam_check_eager(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, uint64_t *bitmap) {
  if (!c) return SBAM_ERR_ARG;
  int rc = check_range_args(c, x0, x1, R);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kBitmap));
  HIPCHK(c, ensure_bitmap(c, x0, x1));
  bool list_form = false;
  CountsDev cd{};
  int64_t first_halo = -1;
  HIPCHK(c, first_halo_begin(c, &cd.first_halo));
  {
    Timer t(c, "check_eager");
    {
      Timer t0(c, "check_eager_pass0");
      HIPCHK(c, launch_check_eager_pass0(view(c), x0, x1, R, c->d_bitmap, cd.first_halo, c->stream));
    }
    HIPCHK(c, run_chains(c, x0, x1, R, 0, cd, &list_form));
  }
  HIPCHK(c, first_halo_fetch(c, cd.first_halo, &first_halo));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (bitmap) {
    int rc2 = copy_bitmap_out(c, x0, x1, bitmap);
    if (rc2) return rc2;
  }
  set_bitmap(c, x0, x1, R, list_form, first_halo);
  return SBAM_OK;
}

int sbam_check_full_words(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, uint32_t *words) {
  if (!c || !words) return SBAM_ERR_ARG;
  int rc = check_range_args(c, x0, x1, R);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kBitmap));
  DevBuf<uint32_t> d_w;  // (per-call: one word per position)
  HIPCHK(c, d_w.ensure(x1 - x0));
  HIPCHK(c, ensure_bitmap(c, x0, x1));
  unsigned long long *d_fh = nullptr;
  int64_t first_halo = -1;
  HIPCHK(c, first_halo_begin(c, &d_fh));
  {
    Timer t(c, "check_words");
    HIPCHK(c, launch_check_words(view(c), x0, x1, R, d_w, c->d_bitmap, d_fh, c->stream));
  }
  if (x1 > x0) HIPCHK(c, hipMemcpyAsync(words, d_w, (x1 - x0) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, first_halo_fetch(c, d_fh, &first_halo));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  set_bitmap(c, x0, x1, R, false, first_halo);
  return SBAM_OK;
}

// Chain pass after a record-0 pass: the list form (launch_chain_list_*) when the PASS0 positions fit its
// scratch (a position list of up to 1/32 of the range), else the per-chunk k_chains walk.  *list_form: which one
// built the bitmap (for set_bitmap).
static hipError_t run_chains(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, int32_t by_key, CountsDev cd,
                             bool *list_form, const int32_t *tile_pass0) {
  const int64_t nch = chain_list_chunks(x0, x1);
  const int64_t cap = (x1 - x0) / 32 + 4096;
  HIPTRY(c->d_ccnt.ensure((size_t)std::max<int64_t>(nch, 1)));
  HIPTRY(c->d_coff2.ensure((size_t)nch + 1));
  ChainScratch cs{c->d_ccnt, c->d_coff2, nullptr, nullptr, nullptr, nullptr};
  HIPTRY(launch_chain_list_build(x0, x1, c->d_bitmap, cs, tile_pass0, c->stream));
  int64_t total = 0;
  HIPTRY(hipMemcpyAsync(&total, c->d_coff2 + nch, 8, hipMemcpyDeviceToHost, c->stream));
  HIPTRY(hipStreamSynchronize(c->stream));
  *list_form = total <= cap;
  if (!*list_form) return launch_check_full_chains(view(c), x0, x1, R, by_key, cd, c->d_bitmap, c->stream);
  HIPTRY(ensure_chain_list(c, (size_t)std::max<int64_t>(total, 1)));
  cs.list = c->d_plist;
  cs.ok = c->d_pok;
  cs.fb = c->d_pfb;
  cs.n_fb = c->d_nfb;
  c->plist_n = total;
  return launch_chain_list_run(view(c), x0, x1, R, by_key, cd, c->d_bitmap, cs, c->stream);
}

int sbam_check_full_counts(sbam_ctx *c, int64_t x0, int64_t x1, int32_t R, int32_t by_key, sbam_counts *out,
                           uint64_t *bitmap) {
  if (!c || !out) return SBAM_ERR_ARG;
  int rc = check_range_args(c, x0, x1, R);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kBitmap));
  HIPCHK(c, ensure_check(c, x0, x1));
  Carve k(c->d_counts.get());
  CountsDev cd = count_words<CountsDev>(k);
  cd.tile_pass0 = c->d_tcnt;
  const size_t words = cd.totals + SBAM_NUM_FLAGS - cd.counts;  // (one run)
  HIPCHK(c, hipMemsetAsync(cd.counts, 0, words * 8, c->stream));
  int64_t first_halo = -1;
  HIPCHK(c, first_halo_begin(c, &cd.first_halo));
  bool tiles = false, list_form = false;
  {
    Timer t(c, "check_full");
    {
      Timer t0(c, "check_pass0");
      HIPCHK(c, launch_check_full_counts(view(c), x0, x1, R, by_key, cd, c->d_bitmap, c->stream, &tiles));
    }
    Timer t1(c, "check_chains");
    HIPCHK(c, run_chains(c, x0, x1, R, by_key, cd, &list_form, tiles ? c->d_tcnt.get() : nullptr));
  }
  std::vector<unsigned long long> hw(words);
  HIPCHK(c, hipMemcpyAsync(hw.data(), cd.counts, words * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, first_halo_fetch(c, cd.first_halo, &first_halo));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (bitmap) {
    int rc2 = copy_bitmap_out(c, x0, x1, bitmap);
    if (rc2) return rc2;
  }
  // the host's copy has the device's layout
  memset(out, 0, sizeof(*out));
  Carve hk(hw.data());
  const CountsDev h = count_words<CountsDev>(hk);
  std::memcpy(out->counts, h.counts, sizeof(out->counts));
  std::memcpy(out->positions, h.positions, sizeof(out->positions));
  std::memcpy(out->reads_before_error, h.rbe, sizeof(out->reads_before_error));
  std::memcpy(out->pair_hist, h.pair, sizeof(out->pair_hist));
  std::memcpy(out->totals, h.totals, sizeof(out->totals));
  out->n_positions = x1 - x0;
  out->n_success = (int64_t)h.scalars[1];
  out->n_too_few_fixed = (int64_t)h.scalars[2];
  out->n_halo = (int64_t)h.scalars[3];
  set_bitmap(c, x0, x1, R, list_form, first_halo);
  if (out->n_halo) {
    c->err.actual = out->n_halo;
    return set_err(c, SBAM_ERR_HALO, "%lld positions need bytes past the shard", (long long)out->n_halo);
  }
  return SBAM_OK;
}

static int find_record_starts(sbam_ctx *c, const std::vector<int64_t> &x0, int32_t R, int64_t mrs, bool use_bm,
                              std::vector<int64_t> &out) {
  const int64_t n = (int64_t)x0.size();
  out.assign(n, -1);
  if (!n) return SBAM_OK;
  HIPCHK(c, c->d_qa.ensure((size_t)n));
  HIPCHK(c, c->d_qb.ensure((size_t)n));
  int64_t *d_x = c->d_qa, *d_o = c->d_qb;
  HIPCHK(c, hipMemcpyAsync(d_x, x0.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  const bool bm = use_bm && c->bm_valid && c->bm_R == R;
  {
    Timer t(c, "find_record");
    HIPCHK(c, launch_find_record_starts(view(c), d_x, n, R, mrs, bm ? c->d_bitmap.get() : nullptr, c->bm_x0, c->bm_x1, d_o,
                                        c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(out.data(), d_o, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_find_record_start(sbam_ctx *c, int64_t block_start, int32_t R, int32_t mrs, int32_t *found, sbam_pos *pos,
                           int32_t *delta) {
  if (!c || !found) return SBAM_ERR_ARG;
  int rc = ensure_stream(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  *found = 0;
  const int64_t b = block_at(c, block_start - c->base);
  if (b < 0) return SBAM_OK;  // EOF-marker block / past the stream: the uncompressed stream is empty → None
  std::vector<int64_t> x0{c->blk.uoff[b]}, out;
  rc = find_record_starts(c, x0, R, mrs, true, out);
  if (rc) return rc;
  if (out[0] == -2) return set_err(c, SBAM_ERR_HALO, "record search left the shard");
  if (out[0] < 0) return SBAM_OK;
  *found = 1;
  if (pos) *pos = pos_of(c, out[0]);
  if (delta) *delta = (int32_t)(out[0] - x0[0]);
  return SBAM_OK;
}

// ---- splits ----------------------------------------------------------------------------------------
int sbam_file_splits(int64_t file_size, int64_t split_size, int64_t *starts, int64_t *ends, int64_t cap, int64_t *n_out) {
  if (split_size <= 0 || file_size < 0 || !n_out) return SBAM_ERR_ARG;
  // FileInputFormat.getSplits: while (bytesRemaining / splitSize > SPLIT_SLOP) emit; then the remainder.
  int64_t n = 0, off = 0, rem = file_size;
  while ((double)rem / (double)split_size > 1.1) {
    if (n < cap && starts) { starts[n] = off; ends[n] = off + split_size; }
    n++;
    off += split_size;
    rem -= split_size;
  }
  if (rem > 0) {
    if (n < cap && starts) { starts[n] = off; ends[n] = file_size; }
    n++;
  }
  *n_out = n;
  return SBAM_OK;
}

// FindBlockStart → FindRecordStart for Hadoop splits [first, first+count): first-record offsets xs and chain
// ends xe = offset of Pos(split end, 0) (CanLoadBam.scala:195-241).
static int split_starts(sbam_ctx *c, const sbam_split_args *a, int64_t first, int64_t count, std::vector<int64_t> &xs,
                        std::vector<int64_t> &xe) {
  int64_t ns = 0;
  sbam_file_splits(c->file_size, a->split_size, nullptr, nullptr, 0, &ns);
  if (first + count > ns) return set_err(c, SBAM_ERR_ARG, "split range past %lld splits", (long long)ns);
  std::vector<int64_t> st(ns), en(ns);
  sbam_file_splits(c->file_size, a->split_size, st.data(), en.data(), ns, &ns);
  std::vector<int64_t> q(st.begin() + first, st.begin() + first + count), bs(count);
  int rc = sbam_find_block_starts(c, q.data(), count, a->bgzf_blocks_to_check, bs.data());
  if (rc) return rc;
  std::vector<int64_t> x0(count);
  xe.assign(count, 0);
  // block_at / x_end_of for every split: the queries ascend, so each search gallops from the previous answer
  // (10 240 independent binary searches over the host block table took ~1 ms of host time per 10 GB step)
  const std::vector<int64_t> &bst = c->blk.start, &buo = c->blk.uoff;
  const int64_t nbh = (int64_t)bst.size();
  auto first_ge = [&](int64_t from, int64_t q) {  // first index >= from with bst[index] >= q
    int64_t lo = from, step = 1, hi = from;
    while (hi < nbh && bst[hi] < q) {
      lo = hi + 1;
      hi += step;
      step *= 2;
    }
    return (int64_t)(std::lower_bound(bst.begin() + lo, bst.begin() + std::min(hi, nbh), q) - bst.begin());
  };
  int64_t ib = 0, ie = 0;
  for (int64_t i = 0; i < count; i++) {
    const int64_t qb = bs[i] - c->base, qe = en[first + i] - c->base;
    const bool sorted = i == 0 || (bs[i] >= bs[i - 1] && en[first + i] >= en[first + i - 1]);
    ib = first_ge(sorted ? ib : 0, qb);
    ie = first_ge(sorted ? ie : 0, qe);
    const int64_t b = (ib < nbh && bst[ib] == qb) ? ib : -1;  // block_at
    if (b < 0) {  // FindRecordStart on the EOF marker: empty stream → None → NoReadFoundException
      return no_read_found(c, bs[i], a->max_read_size);
    }
    x0[i] = buo[b];
    // On a shard the first block at or past the split's end may lie behind the loaded blocks; only when they end at or
    // past the split's end is it the block that follows them, whose Pos(start, 0) is the stream's end.
    if (ie >= nbh && !view(c).eof_real && (nbh == 0 || bst[nbh - 1] + c->blk.csize[nbh - 1] < qe))
      return set_err(c, SBAM_ERR_HALO, "the block at the split's end lies past the shard");
    xe[i] = ie < nbh ? buo[ie] : c->L;  // flat offset of Pos(first block starting at or past the end, 0)
  }
  rc = find_record_starts(c, x0, a->reads_to_check, a->max_read_size, a->use_success_bitmap != 0, xs);
  if (rc) return rc;
  for (int64_t i = 0; i < count; i++) {
    if (xs[i] == -2) return set_err(c, SBAM_ERR_HALO, "record search left the shard");
    if (xs[i] < 0) {
      return no_read_found(c, bs[i], a->max_read_size);
    }
  }
  return SBAM_OK;
}

// Record counts of the chains [xs[i], xe[i]) (RecordStream.scala:27-41).  With try_bitmap and a success bitmap
// covering them, the chains are proven equal to the bitmap's set bits (sbam_records.hip) and counted by
// popcount; else (or if the proof fails) each chain is walked.  Leaves xs/xe on the device (d_sx, d_se).
static int split_counts(sbam_ctx *c, bool try_bitmap, const std::vector<int64_t> &xs, const std::vector<int64_t> &xe,
                        std::vector<int64_t> &cnt, bool *proved) {
  const int64_t n = (int64_t)xs.size();
  *proved = false;
  cnt.assign(n, 0);
  c->rp_tried = c->rp_proved = 0;
  c->rp_missing = c->rp_failed = -1;
  c->rp_fetch = false;
  if (!n) return SBAM_OK;
  HIPCHK(c, c->d_sx.ensure(n));
  HIPCHK(c, c->d_se.ensure(n));
  HIPCHK(c, c->d_sn.ensure(n));
  HIPCHK(c, hipMemcpyAsync(c->d_sx, xs.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_se, xe.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  const int64_t X0 = *std::min_element(xs.begin(), xs.end());
  const int64_t X1 = *std::max_element(xe.begin(), xe.end());
  Timer t(c, "records");
  if (try_bitmap && c->bm_valid && X0 >= c->bm_x0 && X1 <= c->bm_x1) {
    int32_t *d_fail = reinterpret_cast<int32_t *>(SMALL(c, proof_fail));
    const int64_t xa = c->bm_x0 & ~(int64_t)63;
    HIPCHK(c, hipMemsetAsync(d_fail, 0, 4, c->stream));
    // SBAM_FORCE_PROOF=1 (measurement): run the proof even when the list pass found every link, as a bitmap with one
    // false-positive PASS0 site anywhere in the range would (bench.py's loadReads line reports both)
    const char *fp = std::getenv("SBAM_FORCE_PROOF");
    const bool force = fp && *fp && *fp != '0';
    HIPCHK(c, launch_chain_proof(c->d_u, c->L, c->d_bitmap, xa, X0, X1, d_fail,
                                 (c->bm_list && !force) ? c->d_nfb.get() : nullptr, c->stream));
    HIPCHK(c, launch_split_popcounts(c->d_bitmap, xa, c->d_sx, c->d_se, n, c->d_sn, d_fail, c->d_plist, c->plist_n,
                                     c->bm_list ? c->d_nfb.get() : nullptr, c->stream));
    int32_t fail = 1;
    HIPCHK(c, hipMemcpyAsync(&fail, d_fail, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt.data(), c->d_sn, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rp_tried = 1;
    c->rp_fetch = c->bm_list;
    if (!fail) {
      c->rp_proved = 1;
      *proved = true;
      return SBAM_OK;
    }
  }
  HIPCHK(c, launch_record_counts(view(c), c->d_sx, c->d_se, n, c->d_sn, c->stream));
  HIPCHK(c, hipMemcpyAsync(cnt.data(), c->d_sn, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; i++) {
    if (cnt[i] == -2) return set_err(c, SBAM_ERR_HALO, "record chain left the shard");
    if (cnt[i] < 0) return set_err(c, SBAM_ERR_INFLATE, "UnexpectedEOF in record stream");
  }
  return SBAM_OK;
}

int sbam_split_records(sbam_ctx *c, const sbam_split_args *a, int64_t first, int64_t count, sbam_pos *first_pos,
                       int32_t *found, int64_t *n_records) {
  if (!c || !a || first < 0 || count < 0) return SBAM_ERR_ARG;
  int rc = ensure_stream(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int64_t> xs, xe, cnt;
  rc = split_starts(c, a, first, count, xs, xe);
  if (rc) return rc;
  bool proved = false;
  rc = split_counts(c, a->use_success_bitmap != 0, xs, xe, cnt, &proved);
  if (rc) return rc;
  int64_t hint = 0;
  for (int64_t i = 0; i < count; i++) {
    if (first_pos) first_pos[i] = pos_of(c, xs[i], &hint);
    if (found) found[i] = cnt[i] > 0;
    if (n_records) n_records[i] = cnt[i];
  }
  return SBAM_OK;
}

int sbam_compute_splits(sbam_ctx *c, const sbam_split_args *a, sbam_split *splits, int64_t cap, int64_t *n_out) {
  if (!c || !a || !n_out) return SBAM_ERR_ARG;
  int64_t ns = 0;
  sbam_file_splits(c->file_size, a->split_size, nullptr, nullptr, 0, &ns);
  std::vector<sbam_pos> fp(ns);
  std::vector<int32_t> fd(ns);
  int rc = sbam_split_records(c, a, 0, ns, fp.data(), fd.data(), nullptr);
  if (rc) return rc;
  std::vector<sbam_pos> firsts;
  for (int64_t i = 0; i < ns; i++)
    if (fd[i]) firsts.push_back(fp[i]);
  const int64_t n = (int64_t)firsts.size();
  *n_out = n;
  if (cap < n) return set_err(c, SBAM_ERR_ARG, "capacity %lld < %lld splits", (long long)cap, (long long)n);
  for (int64_t i = 0; i < n; i++) {
    splits[i].start = firsts[i];
    splits[i].end = (i + 1 < n) ? firsts[i + 1] : sbam_pos{c->file_size, 0, 0};
  }
  return SBAM_OK;
}

int sbam_record_offsets(sbam_ctx *c, int64_t x0, int64_t x_end, int64_t *offsets, int64_t cap, int64_t *n_out) {
  if (!c || !n_out || x0 < 0) return SBAM_ERR_ARG;
  int rc = ensure_stream(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int64_t> d_o;  // (per-call)
  HIPCHK(c, d_o.ensure(cap));
  HIPCHK(c, launch_record_offsets(view(c), x0, std::min(x_end, c->L), d_o, cap, SMALL(c, record_count), c->stream));
  int64_t n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, SMALL(c, record_count), 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n < 0) n = -(n + 3);
  if (offsets && n) HIPCHK(c, hipMemcpy(offsets, d_o, std::min(n, cap) * 8, hipMemcpyDeviceToHost));
  *n_out = n;
  return SBAM_OK;
}

int sbam_record_spans(sbam_ctx *c, const int64_t *offsets, int64_t n, int32_t *ref_id, int32_t *start, int32_t *end) {
  if (!c || n < 0 || (n && (!offsets || !ref_id || !start || !end))) return SBAM_ERR_ARG;
  if (n == 0) return SBAM_OK;
  int rc = ensure_stream(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int64_t> d_o;  // (per-call)
  DevBuf<int32_t> d_r;
  HIPCHK(c, d_o.ensure(n));
  HIPCHK(c, d_r.ensure(3 * n));
  HIPCHK(c, hipMemcpyAsync(d_o, offsets, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_record_spans(c->d_u, c->L, d_o, n, d_r, d_r + n, d_r + 2 * n, c->stream));
  HIPCHK(c, hipMemcpyAsync(ref_id, d_r, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(start, d_r + n, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(end, d_r + 2 * n, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

// ---- record decode ---------------------------------------------------------------------------------------
int sbam_load_records(sbam_ctx *c, const sbam_split_args *a, int64_t first, int64_t count, int64_t *split_counts_out,
                      int64_t *n_records) {
  if (!c || !a || first < 0 || count < 0) return SBAM_ERR_ARG;
  int rc = ensure_stream(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kRecords));
  std::vector<int64_t> xs, xe, cnt;
  rc = split_starts(c, a, first, count, xs, xe);
  if (rc) return rc;
  bool proved = false;
  rc = split_counts(c, a->use_success_bitmap != 0, xs, xe, cnt, &proved);
  if (rc) return rc;
  std::vector<int64_t> base(count + 1, 0);
  for (int64_t i = 0; i < count; i++) base[i + 1] = base[i] + cnt[i];
  const int64_t N = base[count];
  HIPCHK(c, c->d_sb.ensure(count + 1));
  HIPCHK(c, ensure_record_columns(c, N, nullptr, &c->rcols));
  HIPCHK(c, hipMemcpyAsync(c->d_sb, base.data(), (count + 1) * 8, hipMemcpyHostToDevice, c->stream));
  {
    Timer t(c, "load_records");
    if (proved)
      HIPCHK(c, launch_split_offsets(c->d_bitmap, c->bm_x0 & ~(int64_t)63, c->d_sx, c->d_se, c->d_sb, count, c->d_roff,
                                     c->stream));
    else
      HIPCHK(c, launch_record_walk(c->d_u, c->L, c->d_sx, c->d_se, c->d_sb, count, c->d_roff, c->stream));
    HIPCHK(c, launch_record_columns(c->d_u, c->d_roff, N, c->d_bstart, c->d_buoff, c->d_bu, c->blk.n, c->base,
                                    c->rcols, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->n_loaded = N;
  {
    int64_t ns = 0;
    sbam_file_splits(c->file_size, a->split_size, nullptr, nullptr, 0, &ns);
    c->loaded_all = c->base == 0 && c->file_size == c->D && first == 0 && count == ns;
  }
  if (split_counts_out)
    for (int64_t i = 0; i < count; i++) split_counts_out[i] = cnt[i];
  if (n_records) *n_records = N;
  return SBAM_OK;
}

int sbam_records_path(sbam_ctx *c, int32_t *tried, int32_t *proved, int64_t *missing_links,
                      int64_t *failed_fallbacks) {
  if (!c) return SBAM_ERR_ARG;
  if (c->rp_fetch) {  // the counters of the check whose bitmap that call used are still in d_nfb
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(h, c->d_nfb, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rp_missing = (int64_t)h[1];
    c->rp_failed = (int64_t)h[2];
    c->rp_fetch = false;
  }
  if (tried) *tried = c->rp_tried;
  if (proved) *proved = c->rp_proved;
  if (missing_links) *missing_links = c->rp_missing;
  if (failed_fallbacks) *failed_fallbacks = c->rp_failed;
  return SBAM_OK;
}

int sbam_get_record_columns(sbam_ctx *c, int64_t i0, int64_t n, const sbam_record_columns *o) {
  if (!c || !o || i0 < 0 || n < 0) return SBAM_ERR_ARG;
  if (c->n_loaded < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  if (i0 + n > c->n_loaded)
    return set_err(c, SBAM_ERR_ARG, "records [%lld, %lld) past %lld loaded", (long long)i0, (long long)(i0 + n),
                   (long long)c->n_loaded);
  if (!n) return SBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const RecordColumnsDev &k = c->rcols;
  struct { void *dst; const void *src; size_t w; } cp[] = {
      {o->offset, c->d_roff, 8}, {o->block_pos, k.block_pos, 8}, {o->block_off, k.block_off, 4},
      {o->block_size, k.block_size, 4}, {o->ref_id, k.ref_id, 4}, {o->pos, k.pos, 4},
      {o->bin_mq_nl, k.bin_mq_nl, 4}, {o->flag_nc, k.flag_nc, 4}, {o->l_seq, k.l_seq, 4},
      {o->next_ref_id, k.next_ref_id, 4}, {o->next_pos, k.next_pos, 4}, {o->tlen, k.tlen, 4}};
  for (auto &e : cp)
    if (e.dst)
      HIPCHK(c, hipMemcpyAsync(e.dst, static_cast<const uint8_t *>(e.src) + i0 * e.w, n * e.w, hipMemcpyDeviceToHost,
                               c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_record_columns_device(sbam_ctx *c, sbam_record_columns *d, int64_t *n_records) {
  if (!c || !d) return SBAM_ERR_ARG;
  if (c->n_loaded < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  const RecordColumnsDev &k = c->rcols;
  *d = sbam_record_columns{c->d_roff, k.block_pos, k.block_off, k.block_size, k.ref_id, k.pos,
                           k.bin_mq_nl, k.flag_nc, k.l_seq, k.next_ref_id, k.next_pos, k.tlen};
  if (n_records) *n_records = c->n_loaded;
  return SBAM_OK;
}

// ---- variable-length fields (SAM spec §4.2; htsjdk BAMRecordCodec.decode behind RecordStream.scala:16-33) ----
int sbam_load_record_fields(sbam_ctx *c, int64_t i0, int64_t n, uint32_t fields, sbam_record_field_totals *totals) {
  if (!c) return SBAM_ERR_ARG;
  if (c->n_loaded < 0 || c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  constexpr uint32_t kAll = SBAM_FIELD_NAME | SBAM_FIELD_CIGAR | SBAM_FIELD_SEQ | SBAM_FIELD_QUAL | SBAM_FIELD_AUX;
  if (i0 < 0 || n < 0 || i0 + n > c->n_loaded)
    return set_err(c, SBAM_ERR_ARG, "records [%lld, %lld) outside the %lld loaded", (long long)i0, (long long)(i0 + n),
                   (long long)c->n_loaded);
  if (fields == 0 || (fields & ~kAll)) return set_err(c, SBAM_ERR_ARG, "field mask 0x%x", (unsigned)fields);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kFields));
  c->fdev = sbam_record_fields{};
  c->f_tot = sbam_record_field_totals{};
  if (totals) *totals = c->f_tot;
  if (n == 0) {
    c->f_i0 = i0;
    c->f_n = 0;
    return SBAM_OK;
  }
  FieldOffs o;
  HIPCHK(c, carve(c->d_foff, nullptr, [&](Carve &k) { o = field_offs(k, (size_t)n, (size_t)field_size_blocks(n)); }));
  const RecordColumnsDev &k = c->rcols;
  const FieldSizesArgs sa{c->d_roff + i0, k.block_size + i0, k.bin_mq_nl + i0, k.flag_nc + i0, k.l_seq + i0, n, c->L};
  {
    Timer t(c, "record_field_sizes");
    HIPCHK(c, launch_field_sizes(sa, o.bsum, FieldOffsets{o.off[0], o.off[1], o.off[2], o.off[3]},
                                 reinterpret_cast<unsigned long long *>(o.first_bad), o.totals, c->stream));
  }
  int64_t h[5];  // the first bad record and the four totals: one run
  HIPCHK(c, hipMemcpyAsync(h, o.first_bad, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // (the gather is not launched: it reads only records that passed)
  if (h[0] != -1) return bad_record(c, i0 + h[0], "variable-length fields overrun block_size");
  const sbam_record_field_totals tot{h[1], h[2], h[3], h[4]};
  // data arena: the selected columns
  const struct { uint32_t bit; int64_t bytes; int off; int sh; } col[5] = {
      {SBAM_FIELD_NAME, tot.name_bytes, 0, 0}, {SBAM_FIELD_CIGAR, 4 * tot.cigar_ops, 1, 2},
      {SBAM_FIELD_SEQ, tot.seq_bases, 2, 0},   {SBAM_FIELD_QUAL, tot.seq_bases, 2, 0},
      {SBAM_FIELD_AUX, tot.aux_bytes, 3, 0}};
  int64_t col_bytes[5];
  for (int f = 0; f < 5; f++) col_bytes[f] = (fields & col[f].bit) ? col[f].bytes : -1;
  ByteCol d[5] = {};
  HIPCHK(c, ensure_byte_columns(c->d_fdata, 5, col_bytes, d));
  {
    Timer t(c, "record_fields");
    for (int f = 0; f < 5; f++) {
      if (!d[f].data) continue;
      const FieldGatherArgs ga{c->d_u, sa.roff,   sa.bin_mq_nl, sa.flag_nc, sa.l_seq, o.off[col[f].off],
                               n,      col[f].sh, col[f].bytes, d[f].data,    d[f].tiles};
      HIPCHK(c, launch_field_gather(f, ga, c->stream));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->fdev = sbam_record_fields{o.off[0], d[0].data, o.off[1], reinterpret_cast<uint32_t *>(d[1].data), o.off[2], d[2].data,
                               d[3].data, o.off[3], d[4].data};
  c->f_tot = tot;
  c->f_i0 = i0;
  c->f_n = n;
  if (totals) *totals = tot;
  return SBAM_OK;
}

int sbam_get_record_fields(sbam_ctx *c, const sbam_record_fields *o) {
  if (!c || !o) return SBAM_ERR_ARG;
  if (c->f_n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_record_fields has not run");
  if (c->f_n == 0) {  // an empty batch: each offset column is its single 0
    for (int64_t *p : {o->name_off, o->cigar_off, o->seq_off, o->aux_off})
      if (p) *p = 0;
    return SBAM_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const sbam_record_fields &d = c->fdev;
  const size_t no = (size_t)(c->f_n + 1) * 8;
  const struct { void *dst; const void *src; size_t bytes; bool offs; } cp[] = {
      {o->name_off, d.name_off, no, true},   {o->name, d.name, (size_t)c->f_tot.name_bytes, false},
      {o->cigar_off, d.cigar_off, no, true}, {o->cigar, d.cigar, (size_t)c->f_tot.cigar_ops * 4, false},
      {o->seq_off, d.seq_off, no, true},     {o->seq, d.seq, (size_t)c->f_tot.seq_bases, false},
      {o->qual, d.qual, (size_t)c->f_tot.seq_bases, false},
      {o->aux_off, d.aux_off, no, true},     {o->aux, d.aux, (size_t)c->f_tot.aux_bytes, false}};
  for (auto &e : cp)
    if (e.dst && !e.src) return set_err(c, SBAM_ERR_ARG, "a requested field was not selected by sbam_load_record_fields");
  for (auto &e : cp)
    if (e.dst && e.bytes) HIPCHK(c, hipMemcpyAsync(e.dst, e.src, e.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_record_fields_device(sbam_ctx *c, sbam_record_fields *d, int64_t *i0, int64_t *n) {
  if (!c || !d) return SBAM_ERR_ARG;
  if (c->f_n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_record_fields has not run");
  *d = c->fdev;
  if (i0) *i0 = c->f_i0;
  if (n) *n = c->f_n;
  return SBAM_OK;
}

// ---- typed tags (SAM spec §4.2.4; htsjdk SAMRecord.getAttribute over BAMRecordCodec.decode's records) -------------
int sbam_tag_long_aux_bytes(void) { return tag_long_aux_bytes(); }

int sbam_load_record_tags(sbam_ctx *c, int64_t i0, int64_t n, const sbam_tag_query *q, int32_t n_tags,
                          sbam_record_tag_totals *totals) {
  if (!c) return SBAM_ERR_ARG;
  if (c->n_loaded < 0 || c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  if (i0 < 0 || n < 0 || i0 + n > c->n_loaded)
    return set_err(c, SBAM_ERR_ARG, "records [%lld, %lld) outside the %lld loaded", (long long)i0, (long long)(i0 + n),
                   (long long)c->n_loaded);
  if (!q || n_tags < 1 || n_tags > SBAM_MAX_TAGS) return set_err(c, SBAM_ERR_ARG, "%d tags in the query", (int)n_tags);
  TagWalkArgs wa{};
  int nb = 0;
  for (int j = 0; j < n_tags; j++) {
    const unsigned char a = (unsigned char)q[j].tag[0], b = (unsigned char)q[j].tag[1];
    const bool alpha = (a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z');
    const bool alnum = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || (b >= '0' && b <= '9');
    if (!alpha || !alnum)
      return set_err(c, SBAM_ERR_ARG, "query entry %d is not a tag name [A-Za-z][A-Za-z0-9]", j);
    wa.key[j] = (uint16_t)(a | (b << 8));
    for (int i = 0; i < j; i++)
      if (wa.key[i] == wa.key[j]) return set_err(c, SBAM_ERR_ARG, "tag %c%c twice in the query", a, b);
    wa.bcol[j] = q[j].want_bytes ? (int8_t)nb++ : (int8_t)-1;
    wa.filter |= 1ull << sbam_tag::filter_bit(wa.key[j]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kTags));
  c->tdev = sbam_record_tags{};
  c->t_tot = sbam_record_tag_totals{};
  if (totals) *totals = c->t_tot;
  c->t_nq = n_tags;
  for (int j = 0; j < SBAM_MAX_TAGS; j++) c->t_bytes[j] = j < n_tags && wa.bcol[j] >= 0;
  if (n == 0) {
    c->t_i0 = i0;
    c->t_n = 0;
    return SBAM_OK;
  }
  const RecordColumnsDev &k = c->rcols;
  wa.rec = FieldSizesArgs{c->d_roff + i0, k.block_size + i0, k.bin_mq_nl + i0, k.flag_nc + i0, k.l_seq + i0, n, c->L};
  wa.u = c->d_u;
  wa.nq = n_tags;
  wa.nb = nb;
  TagScan o;
  HIPCHK(c, carve(c->d_tcell, nullptr, [&](Carve &k) { tag_cells(k, wa, (size_t)n); }));
  HIPCHK(c, carve(c->d_toff, nullptr,
                  [&](Carve &k) { o = tag_offs(k, wa, n, exclusive_scan_blocks(n), kTagPresentSlots); }));
  const size_t small_words = kTagPresentAt + kTagPresentSlots * SBAM_MAX_TAGS;  // (the run at wa.first_bad)
  {
    Timer t(c, "record_tag_walk");
    HIPCHK(c, hipMemsetAsync(wa.first_bad, 0, small_words * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(wa.first_bad, 0xff, 8, c->stream));
    HIPCHK(c, launch_tag_walk(wa, c->stream));
    HIPCHK(c, launch_exclusive_scan(wa.off, wa.ostride, n, nb, o.bsum, o.totals, c->stream));
  }
  std::vector<int64_t> h(small_words);
  HIPCHK(c, hipMemcpyAsync(h.data(), wa.first_bad, small_words * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // (nothing is produced; the gather is not launched)
  if (h[0] != -1)
    return bad_record(c, i0 + h[0], "malformed tag list, or variable-length fields overrun block_size");
  sbam_record_tag_totals tot{};
  int64_t col_bytes[SBAM_MAX_TAGS];
  for (int j = 0; j < n_tags; j++) {
    for (int s = 0; s < kTagPresentSlots; s++) tot.present[j] += h[kTagPresentAt + s * SBAM_MAX_TAGS + j];
    if (wa.bcol[j] >= 0) tot.bytes[j] = col_bytes[wa.bcol[j]] = h[kTagTotalsAt + wa.bcol[j]];
  }
  ByteCol d[SBAM_MAX_TAGS] = {};
  HIPCHK(c, ensure_byte_columns(c->d_tdata, nb, col_bytes, d));
  sbam_record_tags dev{wa.type, wa.sub, wa.rel, wa.value, {}, {}};
  {
    Timer t(c, "record_tag_bytes");
    for (int j = 0; j < n_tags; j++) {
      const int b = wa.bcol[j];
      if (b < 0) continue;
      dev.bytes_off[j] = wa.off + b * wa.ostride;
      dev.bytes[j] = d[b].data;
      FieldGatherArgs ga{c->d_u, nullptr, nullptr, nullptr, nullptr, dev.bytes_off[j], n, 0, col_bytes[b], dev.bytes[j],
                         d[b].tiles};
      ga.src = wa.src + b * n;
      HIPCHK(c, launch_field_gather(5, ga, c->stream));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tdev = dev;
  c->t_tot = tot;
  c->t_i0 = i0;
  c->t_n = n;
  if (totals) *totals = tot;
  return SBAM_OK;
}

int sbam_get_record_tags(sbam_ctx *c, const sbam_record_tags *o) {
  if (!c || !o) return SBAM_ERR_ARG;
  if (c->t_n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_record_tags has not run");
  for (int j = 0; j < SBAM_MAX_TAGS; j++)
    if ((o->bytes_off[j] || o->bytes[j]) && !c->t_bytes[j])
      return set_err(c, SBAM_ERR_ARG, "the bytes of query entry %d were not asked of sbam_load_record_tags", j);
  if (c->t_n == 0) {  // an empty batch: each offset column is its single 0
    for (int j = 0; j < SBAM_MAX_TAGS; j++)
      if (o->bytes_off[j]) *o->bytes_off[j] = 0;
    return SBAM_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const sbam_record_tags &d = c->tdev;
  const size_t cells = (size_t)c->t_nq * (size_t)c->t_n;
  auto copy = [&](void *dst, const void *src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIPCHK(c, copy(o->type, d.type, cells));
  HIPCHK(c, copy(o->sub, d.sub, cells));
  HIPCHK(c, copy(o->rel, d.rel, cells * 4));
  HIPCHK(c, copy(o->value, d.value, cells * 8));
  for (int j = 0; j < c->t_nq; j++) {
    HIPCHK(c, copy(o->bytes_off[j], d.bytes_off[j], (size_t)(c->t_n + 1) * 8));
    HIPCHK(c, copy(o->bytes[j], d.bytes[j], (size_t)c->t_tot.bytes[j]));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_record_tags_device(sbam_ctx *c, sbam_record_tags *d, int64_t *i0, int64_t *n, int32_t *n_tags) {
  if (!c || !d) return SBAM_ERR_ARG;
  if (c->t_n < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_record_tags has not run");
  *d = c->t_n ? c->tdev : sbam_record_tags{};  // (an empty batch has no columns)
  if (i0) *i0 = c->t_i0;
  if (n) *n = c->t_n;
  if (n_tags) *n_tags = c->t_nq;
  return SBAM_OK;
}

// ---- BAI index writer (SAM spec §5.2, §5.3; read back by check/.../bam/index/Index.scala:53-90) ------------------
int sbam_index_long_cigar_ops(void) { return index_long_cigar_ops(); }

int sbam_build_index(sbam_ctx *c, sbam_index_totals *totals) {
  if (!c) return SBAM_ERR_ARG;
  if (c->base != 0 || c->file_size != c->D)
    return set_err(c, SBAM_ERR_STATE, "sbam_build_index needs a whole-file context");
  // (a file that ends behind its header has no record for sbam_load_records to find: its index needs no load)
  const bool no_records = c->L >= 0 && c->nref >= 0 && c->header_x == c->L;
  if (c->L < 0 || c->nref < 0 || (!no_records && (c->n_loaded < 0 || !c->loaded_all)))
    return set_err(c, SBAM_ERR_STATE, "sbam_build_index needs sbam_load_records over every split of the file");
  if (int rc = ensure_blocks(c)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kIndex));
  const int64_t N = no_records ? 0 : c->n_loaded;
  const int32_t nref = c->nref;
  HIPCHK(c, ensure_index(c, (size_t)N));
  IndexStats &st = c->istat;
  HIPCHK(c, carve(c->d_istat, nullptr, [&](Carve &k) { st = index_words<IndexStats>(k, (size_t)nref); }));
  HIPCHK(c, c->d_iintv.ensure((size_t)nref + 1));
  const size_t nstat = st.n_intv + nref - st.w;  // (one run)
  const RecordColumnsDev &k = c->rcols;
  const IndexArgs ia{c->d_u,  c->L,        c->d_roff, k.block_pos, k.block_off, k.block_size, k.ref_id,
                     k.pos,   k.bin_mq_nl, k.flag_nc, N,           nref,        c->d_bstart,  c->d_buoff,
                     c->d_bc, c->d_bu,     c->blk.n,  c->base,     c->d_iend,   c->d_ibin};
  std::vector<unsigned long long> hs(nstat, 0);
  {
    Timer t(c, "index");
    HIPCHK(c, hipMemsetAsync(st.w, 0, nstat * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(st.w, 0xff, 8, c->stream));
    if (nref) HIPCHK(c, hipMemsetAsync(st.off_beg, 0xff, (size_t)nref * 8, c->stream));
    HIPCHK(c, launch_index_pass1(ia, st, c->d_iheads, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs.data(), st.w, nstat * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hs[0] != ~0ull) {
      c->err.position = (int64_t)hs[0];
      return set_err(c, SBAM_ERR_RECORD, "record at %lld: ref_id, reference end or CIGAR outside what a BAI can index",
                     (long long)hs[0]);
    }
    const int64_t n_runs = (int64_t)hs[3];
    c->idx_intv.assign((size_t)nref + 1, 0);
    for (int32_t r = 0; r < nref; r++) c->idx_intv[r + 1] = c->idx_intv[r] + (int64_t)hs[st.n_intv - st.w + r];
    const int64_t n_intv = c->idx_intv[nref];
    HIPCHK(c, c->d_irunref.ensure((size_t)n_runs));
    HIPCHK(c, c->d_irunbin.ensure((size_t)n_runs));
    HIPCHK(c, c->d_irun.ensure(2 * (size_t)n_runs));
    HIPCHK(c, c->d_ioff.ensure((size_t)n_intv));
    HIPCHK(c, hipMemcpyAsync(c->d_iintv, c->idx_intv.data(), ((size_t)nref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_intv) HIPCHK(c, hipMemsetAsync(c->d_ioff, 0xff, (size_t)n_intv * 8, c->stream));
    const IndexRuns runs{c->d_irunref, c->d_irunbin, c->d_irun, c->d_irun + n_runs, n_runs};
    HIPCHK(c, launch_index_pass2(ia, c->d_iheads, runs, c->d_iintv, c->d_ioff, c->stream));
    c->idx_tot = sbam_index_totals{nref, 0, n_runs, n_intv, (int64_t)hs[1], (int64_t)hs[2], N};
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->idx_built = true;
  if (totals) *totals = c->idx_tot;
  return SBAM_OK;
}

int sbam_get_index_runs(sbam_ctx *c, int32_t *ref, uint32_t *bin, uint64_t *beg, uint64_t *end) {
  if (!c) return SBAM_ERR_ARG;
  if (!c->idx_built) return set_err(c, SBAM_ERR_STATE, "sbam_build_index has not run");
  const size_t n = (size_t)c->idx_tot.n_runs;
  if (!n) return SBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (ref) HIPCHK(c, hipMemcpyAsync(ref, c->d_irunref, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (bin) HIPCHK(c, hipMemcpyAsync(bin, c->d_irunbin, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (beg) HIPCHK(c, hipMemcpyAsync(beg, c->d_irun, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (end) HIPCHK(c, hipMemcpyAsync(end, c->d_irun + n, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_get_index_refs(sbam_ctx *c, int64_t *intv_off, uint64_t *ioffset, uint64_t *off_beg, uint64_t *off_end,
                        int64_t *n_mapped, int64_t *n_unmapped) {
  if (!c) return SBAM_ERR_ARG;
  if (!c->idx_built) return set_err(c, SBAM_ERR_STATE, "sbam_build_index has not run");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nref = (size_t)c->idx_tot.n_ref, nb = nref * 8;
  if (intv_off) std::copy(c->idx_intv.begin(), c->idx_intv.end(), intv_off);
  if (ioffset && c->idx_tot.n_intv_total)
    HIPCHK(c, hipMemcpyAsync(ioffset, c->d_ioff, (size_t)c->idx_tot.n_intv_total * 8, hipMemcpyDeviceToHost, c->stream));
  if (nref) {
    if (n_mapped) HIPCHK(c, hipMemcpyAsync(n_mapped, c->istat.n_mapped, nb, hipMemcpyDeviceToHost, c->stream));
    if (n_unmapped) HIPCHK(c, hipMemcpyAsync(n_unmapped, c->istat.n_unmapped, nb, hipMemcpyDeviceToHost, c->stream));
    if (off_beg) HIPCHK(c, hipMemcpyAsync(off_beg, c->istat.off_beg, nb, hipMemcpyDeviceToHost, c->stream));
    if (off_end) HIPCHK(c, hipMemcpyAsync(off_end, c->istat.off_end, nb, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBAM_OK;
}

int sbam_bai_assemble(int32_t n_ref, int64_t n_runs, const int32_t *run_ref, const uint32_t *run_bin,
                      const uint64_t *run_beg, const uint64_t *run_end, const int64_t *intv_off,
                      const uint64_t *ioffset, const uint64_t *off_beg, const uint64_t *off_end,
                      const int64_t *n_mapped, const int64_t *n_unmapped, int64_t n_no_coor, uint8_t *out, int64_t cap,
                      int64_t *n_bytes) {
  constexpr uint32_t kMetaBin = 37450, kMaxBin = 37449;
  if (n_ref < 0 || n_runs < 0 || !n_bytes || cap < 0 || (cap && !out)) return SBAM_ERR_ARG;
  if (n_runs && (!run_ref || !run_bin || !run_beg || !run_end)) return SBAM_ERR_ARG;
  if (n_ref && (!intv_off || !off_beg || !off_end || !n_mapped || !n_unmapped)) return SBAM_ERR_ARG;
  typedef std::pair<uint64_t, uint64_t> Chunk;  // (beg, end): sorts by beg, then end
  std::vector<std::map<uint32_t, std::vector<Chunk>>> bins((size_t)n_ref);
  for (int64_t k = 0; k < n_runs; k++) {  // 1. the runs by bin, in file order
    if (run_ref[k] < 0 || run_ref[k] >= n_ref || run_bin[k] >= kMaxBin) return SBAM_ERR_ARG;
    bins[run_ref[k]][run_bin[k]].push_back(Chunk(run_beg[k], run_end[k]));
  }
  for (int32_t r = 0; r < n_ref; r++) {
    if (intv_off[r + 1] < intv_off[r] || (intv_off[r + 1] > intv_off[r] && !ioffset)) return SBAM_ERR_ARG;
    auto &B = bins[r];
    for (int l = 5; l >= 1; l--) {  // 2. small bins move into their parents, leaves first
      const uint32_t lo = ((1u << (3 * l)) - 1) / 7, hi = ((1u << (3 * l + 3)) - 1) / 7;
      std::vector<uint32_t> present;
      for (auto it = B.lower_bound(lo); it != B.end() && it->first < hi; ++it) present.push_back(it->first);
      for (uint32_t b : present) {
        std::vector<Chunk> &cs = B[b];
        if (l < 5) std::sort(cs.begin(), cs.end());
        auto parent = B.find((b - 1) >> 3);
        if ((cs.back().second >> 16) - (cs.front().first >> 16) < 0x10000 && parent != B.end()) {
          parent->second.insert(parent->second.end(), cs.begin(), cs.end());
          B.erase(b);
        }
      }
    }
    auto b0 = B.find(0);  // 3.
    if (b0 != B.end()) std::sort(b0->second.begin(), b0->second.end());
    for (auto &kv : B) {  // 4. coalesce in order
      std::vector<Chunk> &cs = kv.second;
      size_t m = 0;
      for (size_t k = 1; k < cs.size(); k++) {
        if ((cs[m].second >> 16) >= (cs[k].first >> 16)) cs[m].second = std::max(cs[m].second, cs[k].second);
        else cs[++m] = cs[k];
      }
      cs.resize(m + 1);
    }
  }
  // the size, then the bytes
  int64_t need = 8 + 8;
  for (int32_t r = 0; r < n_ref; r++) {
    need += 8;  // n_bin, n_intv
    if (n_mapped[r] + n_unmapped[r] == 0 && bins[r].empty()) continue;
    for (auto &kv : bins[r]) need += 8 + 16 * (int64_t)kv.second.size();
    need += 8 + 32 + 8 * (intv_off[r + 1] - intv_off[r]);
  }
  *n_bytes = need;
  if (cap < need) return SBAM_ERR_ARG;
  uint8_t *p = out;
  auto put32 = [&](uint32_t v) { std::memcpy(p, &v, 4); p += 4; };
  auto put64 = [&](uint64_t v) { std::memcpy(p, &v, 8); p += 8; };
  std::memcpy(p, "BAI\1", 4);
  p += 4;
  put32((uint32_t)n_ref);
  for (int32_t r = 0; r < n_ref; r++) {
    if (n_mapped[r] + n_unmapped[r] == 0 && bins[r].empty()) {
      put32(0);
      put32(0);
      continue;
    }
    put32((uint32_t)bins[r].size() + 1);
    for (auto &kv : bins[r]) {  // ascending bin number
      put32(kv.first);
      put32((uint32_t)kv.second.size());
      for (const Chunk &ch : kv.second) {
        put64(ch.first);
        put64(ch.second);
      }
    }
    put32(kMetaBin);  // 5. the metadata pseudo-bin, last
    put32(2);
    put64(off_beg[r]);
    put64(off_end[r]);
    put64((uint64_t)n_mapped[r]);
    put64((uint64_t)n_unmapped[r]);
    const int64_t ni = intv_off[r + 1] - intv_off[r];
    put32((uint32_t)ni);
    uint8_t *io = p;
    uint64_t next = ~0ull;  // an untouched window takes the next touched one's value
    for (int64_t wdw = ni - 1; wdw >= 0; wdw--) {
      const uint64_t v = ioffset[intv_off[r] + wdw];
      if (v != ~0ull) next = v;
      std::memcpy(io + 8 * wdw, &next, 8);
    }
    p += 8 * ni;
  }
  put64((uint64_t)n_no_coor);
  return SBAM_OK;
}

int sbam_write_bai(sbam_ctx *c, uint8_t *out, int64_t cap, int64_t *n_bytes) {
  if (!c || !n_bytes || cap < 0 || (cap && !out)) return SBAM_ERR_ARG;
  if (!c->idx_built) return set_err(c, SBAM_ERR_STATE, "sbam_build_index has not run");
  const sbam_index_totals &t = c->idx_tot;
  std::vector<int32_t> ref((size_t)t.n_runs);
  std::vector<uint32_t> bin((size_t)t.n_runs);
  std::vector<uint64_t> beg((size_t)t.n_runs), end((size_t)t.n_runs), ioff((size_t)t.n_intv_total);
  const size_t nr = (size_t)t.n_ref;
  std::vector<uint64_t> ob(nr), oe(nr);
  std::vector<int64_t> nm(nr), nu(nr);
  if (int rc = sbam_get_index_runs(c, ref.data(), bin.data(), beg.data(), end.data())) return rc;
  if (int rc = sbam_get_index_refs(c, nullptr, ioff.data(), ob.data(), oe.data(), nm.data(), nu.data())) return rc;
  const int rc = sbam_bai_assemble(t.n_ref, t.n_runs, ref.data(), bin.data(), beg.data(), end.data(),
                                   c->idx_intv.data(), ioff.data(), ob.data(), oe.data(), nm.data(), nu.data(),
                                   t.n_no_coor, out, cap, n_bytes);
  if (rc) return set_err(c, rc, "sbam_write_bai: %lld bytes needed, capacity %lld", (long long)*n_bytes, (long long)cap);
  return SBAM_OK;
}

// ---- coordinate sort (no reference counterpart; htsjdk SortOrder.coordinate, sbam_sort_core.h) --------------------
int sbam_sort_tile_keys(void) { return kSortTile; }

int sbam_sort_records(sbam_ctx *c, sbam_sort_totals *totals) {
  if (!c) return SBAM_ERR_ARG;
  if (c->n_loaded < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  const int64_t N = c->n_loaded;
  if (N >= (1ll << 32)) return set_err(c, SBAM_ERR_ARG, "%lld records: the sort carries 32-bit indices", (long long)N);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kSorted));
  HIPCHK(c, ensure_sort(c->d_sort, (size_t)N, &c->sbuf));
  int64_t below = 0;
  int32_t passes = 0;
  {
    Timer t(c, "sort");
    HIPCHK(c, sort_run(c->sbuf, c->rcols.ref_id, c->rcols.pos, N, c->stream, c, &below, &passes));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sort_tot = sbam_sort_totals{N, below, passes, 0};
  c->sorted = true;
  if (totals) *totals = c->sort_tot;
  return SBAM_OK;
}

int sbam_get_sort_order(sbam_ctx *c, int64_t i0, int64_t n, int64_t *order) {
  if (!c || i0 < 0 || n < 0 || (n && !order)) return SBAM_ERR_ARG;
  if (!c->sorted) return set_err(c, SBAM_ERR_STATE, "sbam_sort_records has not run");
  if (i0 + n > c->sort_tot.n_records)
    return set_err(c, SBAM_ERR_ARG, "entries [%lld, %lld) past %lld sorted", (long long)i0, (long long)(i0 + n),
                   (long long)c->sort_tot.n_records);
  if (!n) return SBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(order, c->sbuf.order + i0, (size_t)n * 8, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

int sbam_sort_order_device(sbam_ctx *c, const int64_t **order, int64_t *n) {
  if (!c || !order || !n) return SBAM_ERR_ARG;
  if (!c->sorted) return set_err(c, SBAM_ERR_STATE, "sbam_sort_records has not run");
  *order = c->sbuf.order;
  *n = c->sort_tot.n_records;
  return SBAM_OK;
}

// ---- BAM writer (htsjdk-rewrite, cli/.../bam/rewrite/HTSJDKRewrite.scala:21-91) ---------------------------------
// A complete BAM header (SAM spec §4.2: magic, l_text, text, n_ref, then l_name, name, l_ref per reference) of exactly
// n bytes?
static bool bam_header_adds_up(const uint8_t *h, int64_t n) {
  auto i32 = [&](int64_t at) { int32_t v; std::memcpy(&v, h + at, 4); return v; };
  if (!h || n < 12 || std::memcmp(h, "BAM\1", 4) != 0) return false;
  const int64_t l_text = i32(4);
  if (l_text < 0 || 8 + l_text + 4 > n) return false;
  int64_t at = 8 + l_text;
  const int64_t n_ref = i32(at);
  at += 4;
  if (n_ref < 0) return false;
  for (int64_t r = 0; r < n_ref; r++) {
    if (at + 4 > n) return false;
    const int64_t l_name = i32(at);
    if (l_name < 0 || at + 4 + l_name + 4 > n) return false;
    at += 4 + l_name + 4;
  }
  return at == n;
}

// sbam_write_bam (ord null) and sbam_write_bam_ordered: one writer, the order one indirection in its select step
static int write_bam(sbam_ctx *c, const sbam_write_args *a, const sbam_write_order *ord, sbam_write_totals *totals) {
  if (!c || !a) return SBAM_ERR_ARG;
  if (c->n_loaded < 0 || c->L < 0) return set_err(c, SBAM_ERR_STATE, "sbam_load_records has not run");
  const int64_t N = c->n_loaded;
  const int32_t bb = a->block_bytes == 0 ? sbam_deflate::kMaxBlockBytes : a->block_bytes;
  if (bb < 1 || bb > sbam_deflate::kMaxBlockBytes)
    return set_err(c, SBAM_ERR_ARG, "block_bytes %d outside 1..%d", (int)a->block_bytes, sbam_deflate::kMaxBlockBytes);
  if (!write_level_ok(a->level))
    return set_err(c, SBAM_ERR_ARG, "level 0x%x: 0 (stored), 1 (fixed Huffman) or 1 | SBAM_WRITE_DYNAMIC = 0x%x (per block the "
                   "smallest of stored, fixed and dynamic Huffman)", (unsigned)a->level, 1 | SBAM_WRITE_DYNAMIC);
  if (a->n_ranges < 0 || (a->n_ranges && (!a->range_lo || !a->range_hi))) return set_err(c, SBAM_ERR_ARG, "ranges missing");
  for (int64_t r = 0; r < a->n_ranges; r++) {
    const int64_t lo = a->range_lo[r], hi = a->range_hi[r];
    if (lo < 0 || hi < lo || hi > N || (r && lo < a->range_hi[r - 1]))
      return set_err(c, SBAM_ERR_ARG, "range %lld [%lld, %lld): out of order or outside the %lld loaded records",
                     (long long)r, (long long)lo, (long long)hi, (long long)N);
  }
  const uint8_t *header = ord ? ord->header : nullptr;
  if (ord && !header && ord->header_bytes != 0) return set_err(c, SBAM_ERR_ARG, "header_bytes without a header");
  if (header) {
    if (!a->with_header) return set_err(c, SBAM_ERR_ARG, "a header override needs with_header = 1");
    if (!bam_header_adds_up(header, ord->header_bytes))
      return set_err(c, SBAM_ERR_ARG, "header override: not a BAM header of exactly %lld bytes (magic, l_text, n_ref, names)",
                     (long long)ord->header_bytes);
    // (the gather copies entry 0 from the stream's first bytes before the override replaces them: they must be readable)
    if (ord->header_bytes + 16 > c->L + kStreamPad)
      return set_err(c, SBAM_ERR_ARG, "header override of %lld bytes: at most %lld (the stream's length + %d)",
                     (long long)ord->header_bytes, (long long)(c->L + kStreamPad - 16), kStreamPad - 16);
  } else if (a->with_header && (c->base != 0 || c->header_x < 0)) {
    return set_err(c, SBAM_ERR_STATE, "with_header needs a context that starts at file offset 0 and has read its header");
  }
  const int64_t *order = ord ? ord->order_device : nullptr;
  if (ord && !order) {
    if (!c->sorted) return set_err(c, SBAM_ERR_STATE, "sbam_sort_records has not run (and no order_device given)");
    order = c->sbuf.order;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, drop_from(c, kWritten));
  if (ord && ord->order_device) {  // the caller's entries, checked on the device before anything is written
    int32_t bad = 0;
    HIPCHK(c, launch_order_check(order, N, N, reinterpret_cast<int32_t *>(SMALL(c, order_bad)), c->stream));
    HIPCHK(c, hipMemcpyAsync(&bad, SMALL(c, order_bad), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return set_err(c, SBAM_ERR_ARG, "order_device: an entry outside the %lld loaded records", (long long)N);
  }
  const int64_t header_bytes = header ? ord->header_bytes : a->with_header ? c->header_x : 0;
  WriteSel sl;
  HIPCHK(c, carve(c->d_wsel, nullptr, [&](Carve &k) { sl = write_sel(k, N, exclusive_scan_blocks(N + 1)); }));
  HIPCHK(c, c->d_wrange.ensure((size_t)(2 * a->n_ranges)));
  if (a->n_ranges) {
    HIPCHK(c, hipMemcpyAsync(c->d_wrange, a->range_lo, (size_t)a->n_ranges * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_wrange + a->n_ranges, a->range_hi, (size_t)a->n_ranges * 8, hipMemcpyHostToDevice,
                             c->stream));
  }
  {
    Timer t(c, "write_select");
    const WriteSelectArgs sa{c->d_roff, c->rcols.block_size, N, c->L, c->d_wrange, c->d_wrange + a->n_ranges,
                             a->n_ranges, a->keep_device, header_bytes, sl.len, sl.cnt, sl.src, order};
    HIPCHK(c, launch_write_select(sa, c->stream));
    HIPCHK(c, launch_exclusive_scan(sl.len, (int64_t)sl.stride, N + 1, 2, sl.bsum, sl.tot, c->stream));
  }
  int64_t h[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h, sl.tot, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t ubytes = h[0], n_records = h[1];
  HIPCHK(c, ensure_write_stream(c->w, ubytes));
  HIPCHK(c, c->d_wtiles.ensure((size_t)(2 * field_gather_tiles(ubytes))));
  {
    Timer t(c, "write_gather");
    // every entry is a "field" at src[i] of len[i] bytes: sbam_fields.hip's gather, divided over output bytes
    const FieldGatherArgs ga{c->d_u, nullptr, nullptr, nullptr, nullptr, sl.len,       N + 1,
                             0,      ubytes,  c->w.u,  c->d_wtiles, sl.src};
    HIPCHK(c, launch_field_gather(5, ga, c->stream));
    if (header) HIPCHK(c, hipMemcpyAsync(c->w.u, header, (size_t)header_bytes, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, writer_run(c->w, c->stream, c, ubytes, bb, a->level, a->with_eof != 0));
  HIPCHK(c, c->d_wrpos.ensure((size_t)n_records));
  HIPCHK(c, c->d_wroff.ensure((size_t)n_records));
  HIPCHK(c, launch_written_records(sl.len, sl.cnt, N, bb, c->w.start, c->d_wrpos, c->d_wroff, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->w_tot = sbam_write_totals{n_records, header_bytes, ubytes, c->w.nb, c->w.n_stored, c->w.comp_bytes};
  c->w.ubytes = ubytes;
  if (totals) *totals = c->w_tot;
  return SBAM_OK;
}

int sbam_write_bam(sbam_ctx *c, const sbam_write_args *a, sbam_write_totals *totals) {
  return write_bam(c, a, nullptr, totals);
}

int sbam_write_bam_ordered(sbam_ctx *c, const sbam_write_args *a, const sbam_write_order *ord,
                           sbam_write_totals *totals) {
  return write_bam(c, a, ord, totals);
}

int sbam_get_written(sbam_ctx *c, uint8_t *out, int64_t cap) {
  if (!c || (!out && cap > 0)) return SBAM_ERR_ARG;
  if (c->w.ubytes < 0) return set_err(c, SBAM_ERR_STATE, "sbam_write_bam has not run");
  if (cap < c->w.comp_bytes)
    return set_err(c, SBAM_ERR_ARG, "sbam_get_written: %lld bytes needed, capacity %lld", (long long)c->w.comp_bytes,
                   (long long)cap);
  HIPCHK(c, hipSetDevice(c->device));
  if (c->w.comp_bytes) HIPCHK(c, hipMemcpy(out, c->w.file, (size_t)c->w.comp_bytes, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

int sbam_written_device(sbam_ctx *c, const uint8_t **dev, int64_t *n) {
  if (!c || !dev || !n) return SBAM_ERR_ARG;
  if (c->w.ubytes < 0) return set_err(c, SBAM_ERR_STATE, "sbam_write_bam has not run");
  *dev = c->w.file;
  *n = c->w.comp_bytes;
  return SBAM_OK;
}

int sbam_get_written_blocks(sbam_ctx *c, int64_t *start, int32_t *csize, int32_t *usize) {
  if (!c) return SBAM_ERR_ARG;
  if (c->w.ubytes < 0) return set_err(c, SBAM_ERR_STATE, "sbam_write_bam has not run");
  const size_t nb = (size_t)c->w.nb;
  if (!nb) return SBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const WriteCols &col = c->w.col;
  if (start) HIPCHK(c, hipMemcpy(start, c->w.start, nb * 8, hipMemcpyDeviceToHost));
  if (csize) HIPCHK(c, hipMemcpy(csize, col.csize, nb * 4, hipMemcpyDeviceToHost));
  if (usize) HIPCHK(c, hipMemcpy(usize, col.usize, nb * 4, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

int sbam_get_written_records(sbam_ctx *c, int64_t *block_pos, int32_t *block_off) {
  if (!c) return SBAM_ERR_ARG;
  if (c->w.ubytes < 0) return set_err(c, SBAM_ERR_STATE, "sbam_write_bam has not run");
  const size_t n = (size_t)c->w_tot.n_records;
  if (!n) return SBAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (block_pos) HIPCHK(c, hipMemcpy(block_pos, c->d_wrpos, n * 8, hipMemcpyDeviceToHost));
  if (block_off) HIPCHK(c, hipMemcpy(block_off, c->d_wroff, n * 4, hipMemcpyDeviceToHost));
  return SBAM_OK;
}

// ---- test support: the scan launchers on buffers and a stream of their own (no context) -------------------------
namespace {
struct ScanTest {  // a device, a stream and one allocation, released on every path
  hipStream_t stream = nullptr;
  uint8_t *buf = nullptr;
  hipError_t open(int device, size_t bytes) {
    HIPTRY(hipSetDevice(device));
    HIPTRY(hipStreamCreate(&stream));
    return hipMalloc(reinterpret_cast<void **>(&buf), bytes ? bytes : 8);
  }
  ~ScanTest() {
    if (buf) (void)hipFree(buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
}  // namespace

int sbam_test_exclusive_scan(int device, const int64_t *in, int64_t n, int32_t cols, int64_t *out) {
  if (n < 0 || cols < 1 || !out || (n && !in)) return SBAM_ERR_ARG;
  const size_t N = (size_t)n, C = (size_t)cols, stride = N + 1, nblk = (size_t)exclusive_scan_blocks(n);
  ScanTest t;
  if (t.open(device, (C * stride + C * nblk + C) * 8) != hipSuccess) return SBAM_ERR_HIP;
  int64_t *off = reinterpret_cast<int64_t *>(t.buf), *bsum = off + C * stride, *totals = bsum + C * nblk;
  std::vector<int64_t> tot(C);
  hipError_t e = hipMemsetAsync(t.buf, 0xff, (C * stride + C * nblk + C) * 8, t.stream);
  if (e == hipSuccess && n)
    e = hipMemcpy2DAsync(off, stride * 8, in, N * 8, N * 8, C, hipMemcpyHostToDevice, t.stream);
  if (e == hipSuccess) e = launch_exclusive_scan(off, (int64_t)stride, n, cols, bsum, totals, t.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, off, C * stride * 8, hipMemcpyDeviceToHost, t.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(tot.data(), totals, C * 8, hipMemcpyDeviceToHost, t.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t.stream);
  if (e != hipSuccess) return SBAM_ERR_HIP;
  for (size_t c = 0; c < C; c++)  // the totals pointer and the column's last entry are one number
    if (tot[c] != out[c * stride + N]) return SBAM_ERR_STATE;
  return SBAM_OK;
}

int sbam_test_scan_sums_int(int device, const int32_t *in, int64_t n, int64_t *out) {
  if (n < 0 || !out || (n && !in)) return SBAM_ERR_ARG;
  const size_t N = (size_t)n, in_bytes = (N * 4 + 7) & ~(size_t)7;
  ScanTest t;
  if (t.open(device, in_bytes + (N + 1) * 8) != hipSuccess) return SBAM_ERR_HIP;
  const int32_t *d_in = reinterpret_cast<const int32_t *>(t.buf);
  int64_t *d_out = reinterpret_cast<int64_t *>(t.buf + in_bytes);
  hipError_t e = hipMemsetAsync(d_out, 0xff, (N + 1) * 8, t.stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(t.buf, in, N * 4, hipMemcpyHostToDevice, t.stream);
  if (e == hipSuccess) e = launch_scan_sums(d_in, d_out, n, 1, d_out + n, t.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (N + 1) * 8, hipMemcpyDeviceToHost, t.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t.stream);
  return e == hipSuccess ? SBAM_OK : SBAM_ERR_HIP;
}

// The sort (sort_run: keys' histograms, the passes they leave, the order) over the caller's keys, on buffers and a
// stream of the call's own.
int sbam_test_sort_keys(int device, const uint64_t *keys, int64_t n, int64_t *order, int32_t *passes) {
  if (n < 0 || n >= (1ll << 32) || !passes || (n && (!keys || !order))) return SBAM_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return SBAM_ERR_HIP;
  DevBuf<uint8_t> buf;  // (freed on every path, with this device current)
  SortBufs b{};
  hipStream_t s = nullptr;
  if (hipStreamCreate(&s) != hipSuccess) return SBAM_ERR_HIP;
  int64_t below = 0;
  hipError_t e = ensure_sort(buf, (size_t)n, &b);
  if (e == hipSuccess && n) e = hipMemcpyAsync(b.keys[0], keys, (size_t)n * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = sort_run(b, nullptr, nullptr, n, s, nullptr, &below, passes);
  if (e == hipSuccess && n) e = hipMemcpyAsync(order, b.order, (size_t)n * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  return e == hipSuccess ? SBAM_OK : SBAM_ERR_HIP;
}

// The three record kernels behind split_counts / sbam_load_records' proven path, on a stream, a bitmap and splits
// of the caller's.  Every index a kernel may form from its arguments is checked here first: the bitmap covers
// [xa, xa + 64 n_words), [X0, X1) and every split lie inside it, and the stream gets the library's zero pad.
int sbam_test_chain_proof(int device, const uint8_t *u, int64_t L, const uint64_t *bm, int64_t n_words, int64_t xa,
                          int64_t X0, int64_t X1, const int64_t *xs, const int64_t *xe, int64_t n_splits,
                          const int64_t *list, int64_t n_list, const uint64_t *exact, int32_t *fail, int64_t *counts,
                          int64_t *offsets, int64_t cap, int64_t *n_offsets) {
  if (L < 0 || n_words < 1 || n_splits < 0 || n_list < 0 || cap < 0 || !bm || !fail || !n_offsets) return SBAM_ERR_ARG;
  if ((L && !u) || (n_splits && (!xs || !xe || !counts)) || (cap && !offsets)) return SBAM_ERR_ARG;
  if ((list != nullptr) != (exact != nullptr) || (n_list && !list)) return SBAM_ERR_ARG;
  const int64_t xb = xa + 64 * n_words;
  if (xa < 0 || (xa & 63) || X0 < xa || X1 > xb) return SBAM_ERR_ARG;
  const size_t S = (size_t)n_splits;
  int64_t worst = 0;  // most offsets k_split_offsets can write for one split: the set bits of its range
  for (size_t i = 0; i < S; i++) {
    if (xs[i] < 0 || xs[i] >= xe[i]) continue;
    if (xs[i] < xa || xe[i] > xb) return SBAM_ERR_ARG;
    int64_t pc = 0;
    for (int64_t w = (xs[i] - xa) >> 6; w <= (xe[i] - 1 - xa) >> 6; w++) pc += __builtin_popcountll(bm[w]);
    worst = std::max(worst, pc);
  }
  for (int64_t i = 1; i < n_list; i++)
    if (list[i] < list[i - 1]) return SBAM_ERR_ARG;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t nblk = (size_t)exclusive_scan_blocks(n_splits);
  const size_t o_u = 0, o_bm = o_u + up((size_t)L + kStreamPad), o_xs = o_bm + up((size_t)n_words * 8),
               o_xe = o_xs + up(S * 8 + 8), o_cnt = o_xe + up(S * 8 + 8), o_base = o_cnt + up(S * 8 + 8),
               o_bsum = o_base + up((S + 1) * 8), o_tot = o_bsum + up(nblk * 8 + 8), o_list = o_tot + 256,
               o_exact = o_list + up((size_t)n_list * 8 + 8), o_fail = o_exact + 256, o_end = o_fail + 256;
  ScanTest t;
  if (t.open(device, o_end) != hipSuccess) return SBAM_ERR_HIP;
  uint8_t *d_u = t.buf + o_u;
  auto *d_bm = reinterpret_cast<unsigned long long *>(t.buf + o_bm);
  auto *d_xs = reinterpret_cast<int64_t *>(t.buf + o_xs), *d_xe = reinterpret_cast<int64_t *>(t.buf + o_xe);
  auto *d_cnt = reinterpret_cast<int64_t *>(t.buf + o_cnt), *d_base = reinterpret_cast<int64_t *>(t.buf + o_base);
  auto *d_bsum = reinterpret_cast<int64_t *>(t.buf + o_bsum), *d_tot = reinterpret_cast<int64_t *>(t.buf + o_tot);
  auto *d_list = reinterpret_cast<int64_t *>(t.buf + o_list);
  auto *d_exact = reinterpret_cast<unsigned long long *>(t.buf + o_exact);
  auto *d_fail = reinterpret_cast<int32_t *>(t.buf + o_fail);
  hipStream_t s = t.stream;
#define T_(expr) do { if ((expr) != hipSuccess) return SBAM_ERR_HIP; } while (0)
  T_(hipMemsetAsync(t.buf, 0, o_end, s));
  if (L) T_(hipMemcpyAsync(d_u, u, (size_t)L, hipMemcpyHostToDevice, s));
  T_(hipMemcpyAsync(d_bm, bm, (size_t)n_words * 8, hipMemcpyHostToDevice, s));
  if (S) {
    T_(hipMemcpyAsync(d_xs, xs, S * 8, hipMemcpyHostToDevice, s));
    T_(hipMemcpyAsync(d_xe, xe, S * 8, hipMemcpyHostToDevice, s));
    T_(hipMemsetAsync(d_cnt, 0xff, S * 8, s));
  }
  if (n_list) T_(hipMemcpyAsync(d_list, list, (size_t)n_list * 8, hipMemcpyHostToDevice, s));
  if (exact) T_(hipMemcpyAsync(d_exact, exact, 24, hipMemcpyHostToDevice, s));
  // fail[0]: the proof; fail[1]: a split whose first record is not a set bit (one word in split_counts)
  T_(launch_chain_proof(d_u, L, d_bm, xa, X0, X1, d_fail, exact ? d_exact : nullptr, s));
  T_(launch_split_popcounts(d_bm, xa, d_xs, d_xe, n_splits, d_cnt, d_fail + 1, list ? d_list : nullptr, n_list,
                            exact ? d_exact : nullptr, s));
  T_(hipMemcpyAsync(fail, d_fail, 8, hipMemcpyDeviceToHost, s));
  if (S) T_(hipMemcpyAsync(counts, d_cnt, S * 8, hipMemcpyDeviceToHost, s));
  T_(hipStreamSynchronize(s));
  int64_t total = 0;
  for (size_t i = 0; i < S; i++) {
    if (counts[i] < 0) return SBAM_ERR_STATE;
    total += counts[i];
  }
  *n_offsets = total;
  if (!S) return SBAM_OK;
  // bases = the exclusive scan of the counts, as sbam_load_records takes them; room for the counts' total plus one
  // split's set bits, so a count that disagrees with the bitmap still writes inside the buffer
  T_(hipMemcpyAsync(d_base, d_cnt, S * 8, hipMemcpyDeviceToDevice, s));
  T_(launch_exclusive_scan(d_base, (int64_t)S + 1, n_splits, 1, d_bsum, d_tot, s));
  int64_t *d_out = nullptr;
  const size_t n_out = (size_t)(total + worst + 1);
  T_(hipMalloc(reinterpret_cast<void **>(&d_out), n_out * 8));
  hipError_t e = hipMemsetAsync(d_out, 0xff, n_out * 8, s);
  if (e == hipSuccess) e = launch_split_offsets(d_bm, xa, d_xs, d_xe, d_base, n_splits, d_out, s);
  int64_t dev_total = -1;
  if (e == hipSuccess) e = hipMemcpyAsync(&dev_total, d_tot, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && std::min(total, cap) > 0)
    e = hipMemcpyAsync(offsets, d_out, (size_t)std::min(total, cap) * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d_out);
#undef T_
  if (e != hipSuccess) return SBAM_ERR_HIP;
  return dev_total == total ? SBAM_OK : SBAM_ERR_STATE;
}

// The writer's blocks stage (writer_run: deflate, scan, frame) over the caller's bytes, with the library's pad behind
// them, on a Writer and a stream of the call's own.
int sbam_test_deflate(int device, const uint8_t *in, int64_t n, int32_t block_bytes, int32_t level, int32_t with_eof,
                      uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_stored_blocks) {
  if (n < 0 || cap < 0 || !n_out || (n && !in) || (cap && !out)) return SBAM_ERR_ARG;
  const int32_t bb = block_bytes == 0 ? sbam_deflate::kMaxBlockBytes : block_bytes;
  if (bb < 1 || bb > sbam_deflate::kMaxBlockBytes || !write_level_ok(level)) return SBAM_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return SBAM_ERR_HIP;
  Writer w;  // (freed on every path, with this device current)
  hipStream_t s = nullptr;
  if (hipStreamCreate(&s) != hipSuccess) return SBAM_ERR_HIP;
  hipError_t e = ensure_write_stream(w, n);
  if (e == hipSuccess) e = hipMemsetAsync(w.u, 0, w.u.size(), s);
  if (e == hipSuccess && n) e = hipMemcpyAsync(w.u, in, (size_t)n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = writer_run(w, s, nullptr, n, bb, level, with_eof != 0);
  int rc = e == hipSuccess ? SBAM_OK : SBAM_ERR_HIP;
  if (rc == SBAM_OK) {
    *n_out = w.comp_bytes;
    if (n_stored_blocks) *n_stored_blocks = w.n_stored;
    if (cap < w.comp_bytes) rc = SBAM_ERR_ARG;
    else if (w.comp_bytes && hipMemcpy(out, w.file, (size_t)w.comp_bytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = SBAM_ERR_HIP;
  }
  (void)hipStreamDestroy(s);
  return rc;
}

}  // extern "C"
