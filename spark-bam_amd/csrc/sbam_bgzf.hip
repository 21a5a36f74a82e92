// sbam_bgzf.hip — hand-written CDNA4 (gfx950) kernels for the BGZF layer of the spark-bam hot path.
//
//  * BGZF block-header scan   (Header.make bgzf/.../block/Header.scala:48-83, MetadataStream.scala:23-54,
//                              FindBlockStart.scala:8-36)
//  The inflate kernels live in sbam_inflate.hip, the record-boundary checker and record chain in sbam_check.hip.
//
// All byte/integer work: no MFMA (no dense contraction).  Design notes and rooflines: DESIGN.md.
#include "sbam_device.h"
#include "sbam_internal.h"

namespace sbam {

// ================================================================================================
// 1. BGZF header scan
// ================================================================================================
constexpr int kScanThreads = 256;
constexpr int kScanWide = 32;  // positions per thread and iteration of k_scan_slots_wide
constexpr int kScanStep = kScanThreads * 16;  // bytes per workgroup iteration

// 16 candidate bits for positions q0..q0+15 given the 32 bytes at q0 (w[0..7] little-endian words).
// Header.make checks bytes 0-3 = 1f 8b 08 04 and 12,13,14 = 'B','C',2 (byte 15 unchecked).
SB_DEV uint32_t header_bits16(const uint32_t w[8], int64_t q0, int64_t D) {
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int wi = i >> 2, o = i & 3;
    const uint32_t m = __builtin_amdgcn_alignbyte(w[wi + 1], w[wi], o);
    const uint32_t bc = __builtin_amdgcn_alignbyte(w[wi + 4], w[wi + 3], o) & 0x00ffffffu;
    const bool hit = (m == 0x04088b1fu) && (bc == 0x00024342u) && (q0 + i + 18 <= D);
    bits |= hit ? (1u << i) : 0u;
  }
  return bits;
}

SB_DEV void load32(const uint8_t *d, int64_t q0, uint32_t w[8]) {
  const uint4 a = *reinterpret_cast<const uint4 *>(d + q0);
  const uint4 b = *reinterpret_cast<const uint4 *>(d + q0 + 16);
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

SB_DEV void fill_candidate(const uint8_t *d, int64_t D, int64_t q, Candidate &c) {
  const int32_t xlen = (int32_t)d[q + 10] | ((int32_t)d[q + 11] << 8);
  const int32_t hs = 18 + xlen - 6;
  const int32_t cs = ((int32_t)d[q + 16] | ((int32_t)d[q + 17] << 8)) + 1;
  int32_t fl = 0, isz = 0;
  if (q + cs <= D) {
    const int64_t e = q + cs - 4;
    isz = (int32_t)((uint32_t)d[e] | ((uint32_t)d[e + 1] << 8) | ((uint32_t)d[e + 2] << 16) |
                    ((uint32_t)d[e + 3] << 24));
    fl |= CAND_ISIZE;
  }
  if (cs - hs - 8 == 2) fl |= CAND_EMPTY;
  c.pos = q;
  c.hsize = hs;
  c.csize = cs;
  c.isize = isz;
  c.flags = fl;
}

// Second pass: write candidates in file order at chunk_offsets[chunk] + rank.
__global__ __launch_bounds__(kScanThreads) void k_scan_write(const uint8_t *__restrict__ d, int64_t D,
                                                              const int64_t *__restrict__ chunk_off,
                                                              Candidate *__restrict__ out) {
  const int64_t cbase = (int64_t)blockIdx.x * kScanChunk;
  const int64_t cend = min(cbase + (int64_t)kScanChunk, D);
  __shared__ int s_any;
  __shared__ int s_wsum[kScanThreads / 64];
  int64_t run = chunk_off[blockIdx.x];
  for (int64_t it = cbase; it < cend; it += kScanStep) {
    const int64_t q0 = it + threadIdx.x * 16;
    uint32_t bits = 0;
    if (q0 < cend) {
      uint32_t w[8];
      load32(d, q0, w);
      bits = header_bits16(w, q0, D);
      if (q0 + 16 > cend) bits &= (1u << (cend - q0)) - 1u;
    }
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    if (bits) s_any = 1;
    __syncthreads();
    if (s_any) {  // rare: ordered rank = wave prefix + preceding waves
      const int c = __popc(bits);
      const int incl = wave_incl_scan(c);
      if (lane_id() == 63) s_wsum[threadIdx.x >> 6] = incl;
      __syncthreads();
      int before = incl - c;
      for (int wv = 0; wv < (int)(threadIdx.x >> 6); wv++) before += s_wsum[wv];
      int64_t slot = run + before;
      while (bits) {
        const int i = __ffs(bits) - 1;
        bits &= bits - 1;
        fill_candidate(d, D, q0 + i, out[slot++]);
      }
      run += s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    }
    __syncthreads();
  }
}

// One-pass form (round 3): the candidates of chunk b written to its kScanSlots fixed slots, its count to
// chunk_counts[b] (slots past kScanSlots are not written; *overflow is set and the caller runs k_scan_write with the
// exact offsets instead), then k_scan_compact moves the slots into file order — the compressed bytes are read once
// instead of twice (a count pass + k_scan_write).  Round 4: P positions per thread and iteration (P + 16 B loaded as
// 16-B pieces, the next one's prefetched while this one's candidates are ranked), and one barrier per iteration
// without candidates (an "any candidate" flag in three rotating LDS words: the one for iteration i + 1 is cleared
// before iteration i's barrier, after every read of it in iteration i - 2).  Scan at 10 GB with P = 16 / 32 / 64:
// 2.51 / 2.14 / 2.20 ms; 16 positions with three barriers per iteration (round 3): 2.83.
template <int P>
SB_DEV void load_wide(const uint8_t *d, int64_t q0, uint32_t w[P / 4 + 4]) {
#pragma unroll
  for (int k = 0; k < P / 16 + 1; k++) {
    const uint4 a = *reinterpret_cast<const uint4 *>(d + q0 + 16 * k);
    w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w;
  }
}
template <int P>
__global__ __launch_bounds__(kScanThreads) void k_scan_slots_wide(const uint8_t *__restrict__ d, int64_t D,
                                                                   int32_t *__restrict__ chunk_counts,
                                                                   Candidate *__restrict__ slots,
                                                                   unsigned long long *__restrict__ overflow) {
  constexpr int kW = P / 4 + 4, kScanWideStep = kScanThreads * P;  // words per thread, bytes per iteration
  static_assert(P % 16 == 0 && P <= 64 && kScanChunk % kScanWideStep == 0 && kCompPad >= P + 16, "wide scan");
  const int64_t cbase = (int64_t)blockIdx.x * kScanChunk;
  const int64_t cend = min(cbase + (int64_t)kScanChunk, D);
  __shared__ int s_any[3];
  __shared__ int s_wsum[kScanThreads / 64];
  if (threadIdx.x < 3) s_any[threadIdx.x] = 0;
  __syncthreads();
  Candidate *out = slots + (int64_t)blockIdx.x * kScanSlots;
  int run = 0, ph = 0;
  uint32_t wn[kW];
  if (cbase + threadIdx.x * P < cend) load_wide<P>(d, cbase + threadIdx.x * P, wn);
  for (int64_t it = cbase; it < cend; it += kScanWideStep) {
    const int64_t q0 = it + threadIdx.x * P;
    uint32_t w[kW];
#pragma unroll
    for (int k = 0; k < kW; k++) w[k] = wn[k];
    if (q0 + kScanWideStep < cend) load_wide<P>(d, q0 + kScanWideStep, wn);
    uint64_t bits = 0;
    if (q0 < cend) {
#pragma unroll
      for (int i = 0; i < P; i++) {
        const int wi = i >> 2, o = i & 3;
        const uint32_t m = __builtin_amdgcn_alignbyte(w[wi + 1], w[wi], o);
        const uint32_t bc = __builtin_amdgcn_alignbyte(w[wi + 4], w[wi + 3], o) & 0x00ffffffu;
        bits |= (m == 0x04088b1fu && bc == 0x00024342u) ? (1ull << i) : 0ull;
      }
      // Header.make needs 18 bytes; the chunk owns positions below cend
      const int64_t lim = min(cend - q0, D - 18 + 1 - q0);
      if (lim < P) bits &= lim > 0 ? (1ull << lim) - 1ull : 0ull;
    }
    const int nx = ph == 2 ? 0 : ph + 1;
    if (threadIdx.x == 0) s_any[nx] = 0;
    if (bits) s_any[ph] = 1;
    __syncthreads();
    const bool any = s_any[ph] != 0;
    ph = nx;
    if (any) {  // rare: ordered rank = wave prefix + preceding waves
      const int c = __popcll(bits);
      const int incl = wave_incl_scan(c);
      if (lane_id() == 63) s_wsum[threadIdx.x >> 6] = incl;
      __syncthreads();
      int slot = run + incl - c;
      for (int wv = 0; wv < (int)(threadIdx.x >> 6); wv++) slot += s_wsum[wv];
      while (bits) {
        const int i = __ffsll((unsigned long long)bits) - 1;
        bits &= bits - 1;
        if (slot < kScanSlots) fill_candidate(d, D, q0 + i, out[slot]);
        slot++;
      }
      run += s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    }
  }
  if (threadIdx.x == 0) {
    chunk_counts[blockIdx.x] = run;
    if (run > kScanSlots) atomicOr(overflow, 1ull);
  }
}

// slots -> file order: slot j of chunk b goes to chunk_off[b] + j (j < chunk_counts[b] <= kScanSlots)
__global__ void k_scan_compact(const Candidate *__restrict__ slots, const int32_t *__restrict__ cnt,
                               const int64_t *__restrict__ off, int64_t nchunks, Candidate *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b = i / kScanSlots;
  const int j = (int)(i % kScanSlots);
  if (b < nchunks && j < cnt[b]) out[off[b] + j] = slots[i];
}

// MetadataStream chain test: per candidate i (>= first), code 0 = the next header sits at cands[i+1];
// 1 = stop before emitting i (ISIZE past EOF, or empty block); 2 = emit i then EOF inside the next header;
// 3 = next header not at cands[i+1] (false positive in between, or corruption: host walks exactly).
__global__ void k_chain_verify(const Candidate *__restrict__ c, int64_t n, int64_t first, int64_t D,
                               unsigned long long *__restrict__ first_stop) {
  const int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Candidate ci = c[i];
  unsigned code;
  if (!(ci.flags & CAND_ISIZE) || (ci.flags & CAND_EMPTY)) {
    code = 1;
  } else {
    const int64_t nx = ci.pos + ci.csize;
    if (nx + 18 > D) code = 2;
    else if (i + 1 < n && c[i + 1].pos == nx) code = 0;
    else code = 3;
  }
  if (code) atomicMin(first_stop, (unsigned long long)(i * 4 + code));
}

SB_DEV int64_t cand_lower_bound(const Candidate *c, int64_t lo, int64_t hi, int64_t q) {
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (c[m].pos < q) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// FindBlockStart.apply for a batch of split starts (one thread per start).
__global__ void k_find_block_starts(const Candidate *__restrict__ c, int64_t n, int64_t D,
                                    const int64_t *__restrict__ starts, int64_t nq, int32_t nchk,
                                    int64_t *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const int64_t s = starts[t];
  if (nchk == 0) {  // take(0) parses no header, so the first probe is accepted (FindBlockStart.scala:19-24)
    out[t] = s;
    return;
  }
  const int64_t lim = s + 65536;  // Block.MAX_BLOCK_SIZE probes
  int64_t best = -1;
  const int64_t qe = max(s, D - 17);  // q + 18 > D: EOF while reading the first header → accepted
  for (int64_t j = cand_lower_bound(c, 0, n, s); j < n && c[j].pos < lim && c[j].pos < qe; j++) {
    int64_t cp = c[j].pos, idx = j;
    bool ok = true;
    for (int k = 0; k < nchk; k++) {
      if (cp + 18 > D) break;
      if (idx < 0) { ok = false; break; }
      const Candidate cc = c[idx];
      if (cp + cc.csize > D) break;
      if (cc.csize - cc.hsize - 8 == 2) break;
      cp += cc.csize;
      const int64_t nj = cand_lower_bound(c, idx + 1, n, cp);
      idx = (nj < n && c[nj].pos == cp) ? nj : -1;
    }
    if (ok) { best = c[j].pos; break; }
  }
  if (best < 0 && qe < lim) best = qe;
  out[t] = best;  // -1: HeaderSearchFailedException
}

__global__ void k_lower_bound(const Candidate *__restrict__ c, int64_t n, int64_t q, int64_t *__restrict__ out) {
  *out = cand_lower_bound(c, 0, n, q);
}

// The block table's columns from the verified chain, plus each workgroup's sum of uncompressed sizes for
// k_block_uoff (a negative isize counts 0, as MetadataStream's offsets do).
__global__ __launch_bounds__(256) void k_gather_blocks(const Candidate *__restrict__ c, int64_t first, int64_t n,
                                                       int64_t *__restrict__ st, int32_t *__restrict__ hs,
                                                       int32_t *__restrict__ cs, int32_t *__restrict__ us,
                                                       int64_t *__restrict__ wsum) {
  __shared__ int64_t s[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t u = 0;
  if (i < n) {
    const Candidate ci = c[first + i];
    st[i] = ci.pos;
    hs[i] = ci.hsize;
    cs[i] = ci.csize;
    us[i] = ci.isize;
    u = ci.isize < 0 ? 0 : ci.isize;
  }
  u = wave_sum(u);
  if (lane_id() == 0) s[threadIdx.x >> 6] = u;
  __syncthreads();
  if (threadIdx.x == 0) wsum[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// Uncompressed offsets uoff[0..n] (exclusive prefix of the sizes; uoff[n] = the stream's length): each workgroup adds
// up the sums of the workgroups before it (n / 256 of them at most, from L2), then scans its own 256 blocks.
__global__ __launch_bounds__(256) void k_block_uoff(const int32_t *__restrict__ us, int64_t n,
                                                    const int64_t *__restrict__ wsum, int64_t *__restrict__ uoff) {
  __shared__ int64_t s[4], ws[4];
  const int t = threadIdx.x;
  int64_t b = 0;
  for (int64_t k = t; k < (int64_t)blockIdx.x; k += 256) b += wsum[k];
  b = wave_sum(b);
  if (lane_id() == 0) s[t >> 6] = b;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  const int64_t v = i < n ? (us[i] < 0 ? 0 : us[i]) : 0;
  int64_t total;
  const int64_t x = block_incl_scan<int64_t, 256>(v, total, ws);  // (its barriers publish s too)
  const int64_t base = s[0] + s[1] + s[2] + s[3];
  if (i < n) uoff[i] = base + x - v;
  if (i == n - 1) uoff[n] = base + x;
}

// ================================================================================================
// 2. The block table by following BSIZE hops (no pass over the bytes)
// ================================================================================================
// MetadataStream reads one header, adds BSIZE + 1 and reads the next: 18 + 4 bytes per block, not the block.  One such
// chain is serial, so the loaded bytes are cut into segments of kFollowSeg bytes and one wave follows each: segment 0
// from the table's first block, segment g > 0 from the first header pattern at or after g * kFollowSeg whose successor
// holds the pattern too (a speculative entry).  k_follow_link then accepts the table only when every segment's exit
// is the next one's entry up to the first stop; otherwise the byte scan above runs instead (a false header in a
// payload that sits first behind a segment's edge costs exactly that).  No wave waits for another.

// The header at q (q <= D) and the four bytes before it, which are the previous block's ISIZE: 28 bytes from the
// aligned dword at or before q - 4, all inside [0, D + kCompPad).
struct HeaderAt {
  uint32_t magic, bc, xlen, bsize, prev_isize;
  SB_DEV bool pattern() const { return magic == 0x04088b1fu && bc == 0x00024342u; }  // Header.make's seven bytes
  SB_DEV int32_t hsize() const { return 18 + (int32_t)xlen - 6; }
  SB_DEV int32_t csize() const { return (int32_t)bsize + 1; }
  SB_DEV bool empty() const { return csize() - hsize() - 8 == 2; }
};
SB_DEV HeaderAt header_at(const uint8_t *d, int64_t q) {
  const int64_t base = (q >= 4 ? q - 4 : 0) & ~(int64_t)3;
  const uint32_t sh = (uint32_t)(q - base);  // 0..7; below 4 only for q < 4 (no block before it)
  const uint32_t *p = reinterpret_cast<const uint32_t *>(d + base);
  uint32_t w[7], v[6];
#pragma unroll
  for (int k = 0; k < 7; k++) w[k] = p[k];
#pragma unroll
  for (int k = 0; k < 6; k++) v[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh & 3);
  const bool hi = sh >= 4;
  HeaderAt h;
  h.prev_isize = v[0];
  h.magic = hi ? v[1] : v[0];
  h.xlen = (hi ? v[3] : v[2]) >> 16;
  h.bc = (hi ? v[4] : v[3]) & 0x00ffffffu;
  h.bsize = (hi ? v[5] : v[4]) & 0xffffu;
  return h;
}

// First p in [lo, hi) (hi <= D - 17) that holds the header pattern and that accept(p) takes, in file order; -1: none.
// The whole wave calls it with the same arguments: 1 KiB per load instruction (each lane its 16 positions' 32 bytes),
// four of them in flight; accept runs wave-uniform on the rare hits.  hi - lo <= 64 KiB + 16: at most 17 iterations.
template <class F>
SB_DEV int64_t wave_first_header(const uint8_t *d, int64_t D, int64_t lo, int64_t hi, F accept) {
  constexpr int kInFlight = 4;
  for (int64_t base = lo & ~(int64_t)15; base < hi; base += kInFlight * 1024) {
    uint32_t w[kInFlight][8];
#pragma unroll
    for (int k = 0; k < kInFlight; k++) {
      const int64_t q0 = base + k * 1024 + lane_id() * 16;
      if (q0 < hi) load32(d, q0, w[k]);
    }
#pragma unroll
    for (int k = 0; k < kInFlight; k++) {
      const int64_t q0 = base + k * 1024 + lane_id() * 16;
      uint32_t bits = 0;
      if (q0 < hi) {
        bits = header_bits16(w[k], q0, D);
        if (q0 < lo) bits &= ~0u << (lo - q0);
        if (q0 + 16 > hi) bits &= (1u << (hi - q0)) - 1u;
      }
      for (unsigned long long any = __ballot(bits != 0); any; any = __ballot(bits != 0)) {
        const int l = __ffsll(any) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bits, l, 64);
        const int i = __ffs(b) - 1;
        const int64_t p = base + k * 1024 + l * 16 + i;
        if (accept(p)) return p;
        if (lane_id() == l) bits &= bits - 1;
      }
    }
  }
  return -1;
}

// One wave per segment.  Rows go to the segment's kFollowSlots fixed slots (a row past them is counted, not written,
// and sets FOLLOW_OVERFLOW); a row's isize arrives with the next header's load, four bytes before it.
__global__ __launch_bounds__(256) void k_follow_blocks(const uint8_t *__restrict__ d, int64_t D, int64_t start_rel,
                                                        int64_t nseg, FollowSegs fs, Candidate *__restrict__ slots) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nseg) return;
  const int64_t g = start_rel / kFollowSeg + w;  // (the table's first block may lie past segment 0 of the bytes)
  const int64_t seg_end = (g + 1) * (int64_t)kFollowSeg;
  Candidate *out = slots + w * kFollowSlots;
  int64_t q = start_rel;
  if (w > 0) {
    const int64_t lo = g * (int64_t)kFollowSeg;
    q = wave_first_header(d, D, lo, min(lo + 65536, D - 17), [&](int64_t p) {
      const HeaderAt h = header_at(d, p);
      const int64_t nx = p + h.csize();
      if (nx > D || h.empty() || nx + 18 > D) return true;  // the chain stops here: MetadataStream's rules
      return header_at(d, nx).pattern();
    });
  }
  const int64_t entry = q;
  int32_t n = 0, kind = q < 0 ? FOLLOW_NOENTRY : 0;
  // q grows by csize >= 1 per hop and ends the loop at seg_end: at most kFollowSeg + 1 hops
  while (q >= 0) {
    const HeaderAt h = header_at(d, q);  // (q <= D)
    if (n > 0 && n <= kFollowSlots && lane_id() == 0) out[n - 1].isize = (int32_t)h.prev_isize;
    if (q + 18 > D) { kind |= FOLLOW_STOP; break; }  // EOF inside the next header
    if (q >= seg_end) break;
    if (!h.pattern()) { kind |= FOLLOW_PARSE; break; }
    if (q + h.csize() > D || h.empty()) { kind |= FOLLOW_STOP; break; }  // stop before emitting
    if (n < kFollowSlots) {
      if (lane_id() == 0) {
        out[n].pos = q;
        out[n].hsize = h.hsize();
        out[n].csize = h.csize();
        out[n].flags = CAND_ISIZE;
      }
    } else {
      kind |= FOLLOW_OVERFLOW;
    }
    n++;
    q += h.csize();
  }
  if (lane_id() == 0) {
    fs.entry[w] = entry;
    fs.exit[w] = q;
    fs.rows[w] = n;
    fs.kind[w] = kind;
  }
}

// verdict[0] = first segment the table cannot be taken from (parse failure, overflow, no entry, or an exit that is
// not the next segment's entry), verdict[1] = first segment whose chain stopped; both preset ~0.
__global__ void k_follow_link(FollowSegs fs, int64_t nseg, unsigned long long *__restrict__ verdict) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nseg) return;
  const int32_t kind = fs.kind[w];
  const bool stop = (kind & FOLLOW_STOP) != 0;
  bool bad = (kind & (FOLLOW_PARSE | FOLLOW_OVERFLOW | FOLLOW_NOENTRY)) != 0;
  if (!stop && !bad) bad = w + 1 >= nseg || fs.entry[w + 1] != fs.exit[w];
  if (bad) atomicMin(verdict, (unsigned long long)w);
  if (stop) atomicMin(verdict + 1, (unsigned long long)w);
}
// The accepted table's rows per segment (those up to the stop; none when the table is not accepted).
__global__ void k_follow_counts(FollowSegs fs, int64_t nseg, const unsigned long long *__restrict__ verdict) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nseg) return;
  const unsigned long long bad = verdict[0], stop = verdict[1];
  fs.cnt[w] = (stop < bad && (unsigned long long)w <= stop) ? fs.rows[w] : 0;
}
// slots -> file order, as k_scan_compact: row j of segment w goes to off[w] + j
__global__ void k_follow_compact(const Candidate *__restrict__ slots, FollowSegs fs, int64_t nseg,
                                 Candidate *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t w = i / kFollowSlots;
  const int j = (int)(i % kFollowSlots);
  if (w < nseg && j < fs.cnt[w]) out[fs.off[w] + j] = slots[i];
}

// FindBlockStart.apply without a candidate list: one wave per start.  k_find_block_starts' rules, with "a candidate
// at cp" read as "the header test holds on the bytes at cp".
__global__ __launch_bounds__(256) void k_find_block_starts_bytes(const uint8_t *__restrict__ d, int64_t D,
                                                                  const int64_t *__restrict__ starts, int64_t nq,
                                                                  int32_t nchk, int64_t *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= nq) return;
  const int64_t s = starts[t];
  int64_t best = s;  // nchk == 0: take(0) parses no header, so the first probe is accepted
  if (nchk > 0) {
    const int64_t lim = s + 65536;     // Block.MAX_BLOCK_SIZE probes
    const int64_t qe = max(s, D - 17);  // q + 18 > D: EOF while reading the first header → accepted
    best = wave_first_header(d, D, s, min(lim, qe), [&](int64_t p) {
      int64_t cp = p;
      for (int k = 0; k < nchk; k++) {
        if (cp + 18 > D) break;
        const HeaderAt h = header_at(d, cp);
        if (!h.pattern()) return false;
        if (cp + h.csize() > D || h.empty()) break;
        cp += h.csize();
      }
      return true;
    });
    if (best < 0 && qe < lim) best = qe;
  }
  if (lane_id() == 0) out[t] = best;  // -1: HeaderSearchFailedException
}

// ================================================================================================
// launch wrappers
// ================================================================================================

hipError_t launch_scan_write(const uint8_t *d, int64_t D, const int64_t *off, int64_t nchunks, Candidate *c,
                             hipStream_t s) {
  if (nchunks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_write, dim3((unsigned)nchunks), dim3(kScanThreads), 0, s, d, D, off, c);
  return hipGetLastError();
}
hipError_t launch_scan_slots(const uint8_t *d, int64_t D, int32_t *cc, int64_t nchunks, Candidate *slots,
                             int64_t *overflow, hipStream_t s) {
  (void)hipMemsetAsync(overflow, 0, sizeof(int64_t), s);
  if (nchunks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_slots_wide<kScanWide>, dim3((unsigned)nchunks), dim3(kScanThreads), 0, s, d, D, cc,
                     slots, reinterpret_cast<unsigned long long *>(overflow));
  return hipGetLastError();
}
hipError_t launch_scan_compact(const Candidate *slots, const int32_t *cc, const int64_t *off, int64_t nchunks,
                               Candidate *out, hipStream_t s) {
  const int64_t n = nchunks * kScanSlots;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slots, cc, off, nchunks,
                     out);
  return hipGetLastError();
}
hipError_t launch_chain_verify(const Candidate *c, int64_t n, int64_t first, int64_t D, int64_t *first_stop,
                               hipStream_t s) {
  if (n - first <= 0) return hipSuccess;
  const int64_t m = n - first;
  hipLaunchKernelGGL(k_chain_verify, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, c, n, first, D,
                     reinterpret_cast<unsigned long long *>(first_stop));
  return hipGetLastError();
}
hipError_t launch_find_block_starts(int64_t D, const Candidate *c, int64_t ncand, const int64_t *st, int64_t n,
                                    int32_t nchk, int64_t *out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_find_block_starts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, ncand, D, st, n,
                     nchk, out);
  return hipGetLastError();
}
hipError_t launch_follow_blocks(const uint8_t *d, int64_t D, int64_t start_rel, int64_t nseg, FollowSegs fs,
                                Candidate *slots, int64_t *verdict, hipStream_t s) {
  unsigned long long *v = reinterpret_cast<unsigned long long *>(verdict);
  (void)hipMemsetAsync(v, 0xff, 2 * sizeof(*v), s);
  const unsigned nwg = (unsigned)((nseg + 255) / 256);
  hipLaunchKernelGGL(k_follow_blocks, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, s, d, D, start_rel, nseg, fs,
                     slots);
  hipLaunchKernelGGL(k_follow_link, dim3(nwg), dim3(256), 0, s, fs, nseg, v);
  hipLaunchKernelGGL(k_follow_counts, dim3(nwg), dim3(256), 0, s, fs, nseg, v);
  return hipGetLastError();
}
hipError_t launch_follow_compact(const Candidate *slots, FollowSegs fs, int64_t nseg, Candidate *out, hipStream_t s) {
  const int64_t n = nseg * kFollowSlots;
  hipLaunchKernelGGL(k_follow_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slots, fs, nseg, out);
  return hipGetLastError();
}
hipError_t launch_find_block_starts_bytes(const uint8_t *d, int64_t D, const int64_t *st, int64_t n, int32_t nchk,
                                          int64_t *out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_find_block_starts_bytes, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, d, D, st, n, nchk,
                     out);
  return hipGetLastError();
}
hipError_t launch_lower_bound(const Candidate *c, int64_t n, int64_t q, int64_t *out, hipStream_t s) {
  hipLaunchKernelGGL(k_lower_bound, dim3(1), dim3(1), 0, s, c, n, q, out);
  return hipGetLastError();
}
hipError_t launch_gather_blocks(const Candidate *c, int64_t first, int64_t n, int64_t *st, int32_t *hs, int32_t *cs,
                                int32_t *us, int64_t *wsum, int64_t *uoff, hipStream_t s) {
  if (n == 0) return hipMemsetAsync(uoff, 0, sizeof(int64_t), s);
  const unsigned nwg = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_gather_blocks, dim3(nwg), dim3(256), 0, s, c, first, n, st, hs, cs, us, wsum);
  hipLaunchKernelGGL(k_block_uoff, dim3(nwg), dim3(256), 0, s, us, n, wsum, uoff);
  return hipGetLastError();
}
}  // namespace sbam
