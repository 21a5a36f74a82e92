// sbam_fields.hip — the variable-length half of a BAM record as device columns (gfx950).
//
// Reference: htsjdk BAMRecordCodec.decode behind RecordStream (check/src/main/scala/org/hammerlab/bam/iterator/
// RecordStream.scala:16-33) hands loadReads' callers SAMRecords with name, CIGAR, bases, qualities and tags
// (CanLoadBam.scala:221-241, 348-352; record layout: SAM spec §4.2).  Here records [i0, i0 + n) of the last
// sbam_load_records become CSR columns: int64 offsets (n + 1 entries, exclusive prefix sums) plus packed data.
//
//   sizes    one thread per record reads the fixed-field columns (coalesced; the stream is not touched), computes
//            the four lengths and validates them against block_size and the stream end; the first bad record index
//            is reduced to the host, which then launches no gather.
//   scan     per-workgroup sums, launch_scan_sums over the four columns of sums, per-workgroup offsets (int64).
//   gather   work is divided over OUTPUT bytes: a workgroup owns an 8 KiB tile of one column; the records that
//            intersect it come from a binary search in the offsets (one thread per tile, ahead of the gather),
//            their offsets and field positions are staged in LDS when they fit, and every lane builds 8 output
//            bytes from the one or more records they fall in.  Source bytes sit at any alignment:
//            three aligned dword loads plus alignbyte give the 8 bytes at a position (the stream buffer is 4-byte
//            aligned and padded past L).  Bases: 8 output bytes come from 4-5 packed bytes; the nibble parity is
//            that of the base index inside the record, not of the output address.  A 400 000-base record and a
//            1-base one cost the same per output byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbam_device.h"
#include "sbam_internal.h"

namespace sbam {

int64_t field_gather_tiles(int64_t total);

namespace {

constexpr int kSizeThreads = 1024;   // records per workgroup in the sizes / offsets kernels
constexpr int kGatherThreads = 256;
constexpr int kLaneBytes = 8;        // output bytes per lane and step
constexpr int kStepBytes = kGatherThreads * kLaneBytes;  // 2 KiB of one output column per workgroup step
// steps per tile: 8 KiB tiles; 4 KiB for the cigar column, so that a tile of one-op records (4 bytes each) still
// fits the LDS stage
constexpr int field_steps(int field) { return field == 1 ? 2 : 4; }
constexpr int kStageCap = 1040;      // a tile's records kept in LDS (more: searched in global memory)

// bsum[f * nblk + b] = workgroup b's sum of length f; *first_bad = min index of a record that fails validation
__global__ void __launch_bounds__(kSizeThreads) k_field_sums(FieldSizesArgs a, int64_t nblk, int64_t *__restrict__ bsum,
                                                             unsigned long long *__restrict__ first_bad) {
  __shared__ int64_t ws[kSizeThreads / 64][4];
  const int64_t k = (int64_t)blockIdx.x * kSizeThreads + threadIdx.x;
  FieldLens r{{0, 0, 0, 0}, false};
  if (k < a.n) r = field_lens(a, k);
  if (r.bad) atomicMin(first_bad, (unsigned long long)k);
  int64_t incl[4], total[4];
  block_incl_scan<int64_t, 4, kSizeThreads>(r.v, incl, total, ws);
  if (threadIdx.x < 4) bsum[threadIdx.x * nblk + blockIdx.x] = total[threadIdx.x];
}

// off[f][k] = exclusive prefix sum of length f over the batch's records, off[f][n] = its total
__global__ void __launch_bounds__(kSizeThreads) k_field_offsets(FieldSizesArgs a, int64_t nblk,
                                                                const int64_t *__restrict__ bsum, FieldOffsets off) {
  __shared__ int64_t ws[kSizeThreads / 64][4];
  const int64_t k = (int64_t)blockIdx.x * kSizeThreads + threadIdx.x;
  FieldLens r{{0, 0, 0, 0}, false};
  if (k < a.n) r = field_lens(a, k);
  int64_t incl[4], total[4];
  block_incl_scan<int64_t, 4, kSizeThreads>(r.v, incl, total, ws);
  if (k >= a.n) return;
  int64_t *o[4] = {off.name, off.cigar, off.seq, off.aux};
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const int64_t e = bsum[f * nblk + blockIdx.x] + incl[f];
    o[f][k] = e - r.v[f];
    if (k == a.n - 1) o[f][a.n] = e;
  }
}

// four 4-bit base codes (code j in bits 4j..4j+3) -> four ASCII bytes of "=ACMGRSVTWYHKDBN": the table is four
// constant dwords; one byte-permute indexes each half with the codes' low three bits, bit 3 selects the half
SB_DEV uint32_t bases4(uint32_t h) {
  uint32_t s = (h | (h << 8)) & 0x00ff00ffu;
  s = (s | (s << 4)) & 0x0f0f0f0fu;
  const uint32_t sel = s & 0x07070707u;
  const uint32_t lo = __builtin_amdgcn_perm(0x56535247u /* GRSV */, 0x4d43413du /* =ACM */, sel);
  const uint32_t hi = __builtin_amdgcn_perm(0x4e42444bu /* KDBN */, 0x48595754u /* TWYH */, sel);
  const uint32_t m = ((s >> 3) & 0x01010101u) * 0xffu;
  return (lo & ~m) | (hi & m);
}

// ASCII of the 8 bases from base index b of the packed sequence at x (high nibble first)
SB_DEV uint64_t bases8(const uint8_t *u, int64_t x, int64_t b) {
  const uint64_t v = load8(u, x + (b >> 1));
  // nibbles in base order: swap the two of each byte, then drop the first when b is odd
  uint64_t t = ((v & 0x0f0f0f0f0f0f0f0full) << 4) | ((v >> 4) & 0x0f0f0f0f0f0f0f0full);
  t >>= 4 * (uint32_t)(b & 1);
  const uint32_t h = (uint32_t)t;
  return (uint64_t)bases4(h & 0xffffu) | ((uint64_t)bases4(h >> 16) << 32);
}

enum : int { F_NAME = 0, F_CIGAR = 1, F_SEQ = 2, F_QUAL = 3, F_AUX = 4, F_AT = 5 };

// stream offset of record r's field F (SAM spec §4.2: 36 fixed bytes, read_name, cigar, seq, qual, tags); F_AT: the
// position column a.src gives (a tag's value, sbam_tags.hip)
template <int F>
SB_DEV int64_t field_start(const FieldGatherArgs &a, int64_t r) {
  if (F == F_AT) return a.src[r];
  int64_t x = a.roff[r] + 36;
  if (F == F_NAME) return x;
  x += a.bin_mq_nl[r] & 0xffu;
  if (F == F_CIGAR) return x;
  x += 4 * (int64_t)(a.flag_nc[r] & 0xffffu);
  if (F == F_SEQ) return x;
  const int64_t ls = a.l_seq[r];
  x += (ls + 1) >> 1;
  if (F == F_QUAL) return x;
  return x + ls;
}

// the last r in [lo, hi] with off(r) <= q (off(lo) <= q holds)
template <class Get>
SB_DEV int64_t owner(Get get, int64_t lo, int64_t hi, int64_t q) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (get(mid) <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One thread per tile: the records that own the tile's first and last byte.  (Found here, ahead of the gather, the
// ~log2(n) dependent loads of a search overlap across tiles instead of opening every gather workgroup.)
__global__ void __launch_bounds__(kGatherThreads) k_field_tiles(const int64_t *__restrict__ goff, int64_t n, int sh,
                                                                int64_t total, int64_t tiles, int64_t tile_bytes,
                                                                int64_t *__restrict__ first, int64_t *__restrict__ last) {
  const int64_t b = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x;
  if (b >= tiles) return;
  const int64_t t0 = b * tile_bytes;
  const int64_t t1 = t0 + tile_bytes < total ? t0 + tile_bytes : total;
  auto gget = [&](int64_t r) { return goff[r] << sh; };
  const int64_t f = owner(gget, 0, n - 1, t0);
  first[b] = f;
  last[b] = owner(gget, f, n - 1, t1 - 1);
}

// One workgroup per tile (8 KiB; cigar 4 KiB) of column F's output bytes [0, a.total).  a.off holds the column's
// offsets in units of 1 << a.sh bytes (cigar ops: 4 bytes); a.tiles the tiles' first and last records
// (k_field_tiles).  The offsets and the field's stream positions of the tile's records are staged in LDS by
// coalesced loads when they fit.
template <int F>
__global__ void __launch_bounds__(kGatherThreads) k_field_gather(FieldGatherArgs a, int64_t tiles) {
  __shared__ int64_t soff[kStageCap + 1];
  __shared__ int64_t ssrc[kStageCap];
  constexpr int kTileBytes = field_steps(F) * kStepBytes;
  const int64_t t0 = (int64_t)blockIdx.x * kTileBytes;
  const int64_t t1 = t0 + kTileBytes < a.total ? t0 + kTileBytes : a.total;
  if (t0 >= t1) return;
  const int sh = a.sh;
  const int64_t *__restrict__ goff = a.off;
  const int64_t r_lo = a.tiles[blockIdx.x], r_hi = a.tiles[tiles + blockIdx.x];
  const int64_t cnt = r_hi - r_lo + 2;  // offsets r_lo .. r_hi + 1
  const bool staged = cnt <= kStageCap + 1;
  if (staged) {
    for (int64_t i = threadIdx.x; i < cnt; i += kGatherThreads) {
      soff[i] = goff[r_lo + i] << sh;
      if (i < cnt - 1) ssrc[i] = field_start<F>(a, r_lo + i);
    }
    __syncthreads();
  }
  auto get = [&](int64_t r) { return staged ? soff[r - r_lo] : goff[r] << sh; };
  for (int it = 0; it < field_steps(F); it++) {
    const int64_t p = t0 + ((int64_t)it * kGatherThreads + threadIdx.x) * kLaneBytes;
    if (p >= t1) break;
    const int64_t pe = p + kLaneBytes < t1 ? p + kLaneBytes : t1;
    uint64_t out = 0;
    int64_t q = p;
    int64_t r = owner(get, r_lo, r_hi, q);
    for (;;) {
      // q lies in record r: its bytes from q on go to out's bytes q - p and up; what runs past the record's end
      // (bytes inside the padded stream) is overwritten by the next record's or cleared below
      const int64_t rs = get(r), re = get(r + 1);
      const int64_t x = staged ? ssrc[r - r_lo] : field_start<F>(a, r);
      const uint64_t v = F == F_SEQ ? bases8(a.u, x, q - rs) : load8(a.u, x + (q - rs));
      const uint32_t s8 = 8 * (uint32_t)(q - p);
      out = s8 ? (out & ((1ull << s8) - 1ull)) | (v << s8) : v;
      if (re >= pe) break;
      q = re;
      r++;  // the next record with a byte at q: usually r + 1, else past the empty ones
      if (get(r + 1) <= q) r = owner(get, r, r_hi, q);
    }
    if (pe - p < kLaneBytes) out &= (1ull << (8 * (uint32_t)(pe - p))) - 1ull;
    *reinterpret_cast<uint64_t *>(a.out + p) = out;
  }
}

template <int F>
hipError_t gather(const FieldGatherArgs &a, hipStream_t s) {
  constexpr int64_t kTileBytes = field_steps(F) * kStepBytes;
  const int64_t tiles = (a.total + kTileBytes - 1) / kTileBytes;
  hipLaunchKernelGGL(k_field_tiles, dim3((unsigned)((tiles + kGatherThreads - 1) / kGatherThreads)),
                     dim3(kGatherThreads), 0, s, a.off, a.n, a.sh, a.total, tiles, kTileBytes, a.tiles,
                     a.tiles + tiles);
  hipLaunchKernelGGL(k_field_gather<F>, dim3((unsigned)tiles), dim3(kGatherThreads), 0, s, a, tiles);
  return hipGetLastError();
}

}  // namespace

// (an upper bound for every column: the smallest tile)
int64_t field_gather_tiles(int64_t total) { return (total + 2 * kStepBytes - 1) / (2 * kStepBytes); }
int64_t field_size_blocks(int64_t n) { return (n + kSizeThreads - 1) / kSizeThreads; }

hipError_t launch_field_sizes(const FieldSizesArgs &a, int64_t *bsum, FieldOffsets off, unsigned long long *first_bad,
                              int64_t *totals, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int64_t nblk = field_size_blocks(a.n);
  hipError_t e = hipMemsetAsync(first_bad, 0xff, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_field_sums, dim3((unsigned)nblk), dim3(kSizeThreads), 0, s, a, nblk, bsum, first_bad);
  e = launch_scan_sums(bsum, bsum, nblk, 4, totals, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_field_offsets, dim3((unsigned)nblk), dim3(kSizeThreads), 0, s, a, nblk, bsum, off);
  return hipGetLastError();
}

hipError_t launch_field_gather(int field, const FieldGatherArgs &a, hipStream_t s) {
  if (a.n <= 0 || a.total <= 0) return hipSuccess;
  switch (field) {
    case F_NAME: return gather<F_NAME>(a, s);
    case F_CIGAR: return gather<F_CIGAR>(a, s);
    case F_SEQ: return gather<F_SEQ>(a, s);
    case F_QUAL: return gather<F_QUAL>(a, s);
    case F_AUX: return gather<F_AUX>(a, s);
    case F_AT: return gather<F_AT>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace sbam
