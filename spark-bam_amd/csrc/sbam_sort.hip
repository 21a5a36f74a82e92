// sbam_sort.hip — the stable coordinate sort of the loaded records (gfx950, wave64): an LSD radix sort of
// (key, record index) pairs by 8-bit digits, at most eight passes.  The key and the order it defines: sbam_sort_core.h.
//
// No reference counterpart: the reference never reorders records.  The behaviour mirrored is htsjdk's
// SAMFileWriterFactory with SortOrder.coordinate (behind cli/.../bam/rewrite/HTSJDKRewrite.scala:52-76) and
// `samtools sort` without its strand tie-break.
//
//   keys     one thread per record builds the key from ref_id / pos (or takes a caller's key: the test entry), counts
//            the records whose key is below their predecessor's (one atomic per wave) and adds every byte of the key to
//            eight 256-bin histograms: LDS counters per workgroup, then one global atomic per non-empty bin.  The host
//            reads the 2049 words back: no record out of order -> the order is the identity and no pass runs; a digit
//            with one bin holding every key -> that pass would move nothing and is skipped (n_ref <= 256 and
//            positions below 2^24 leave four of the eight).
//   count    per pass, one workgroup per tile of kSortTile keys: the tile's 256 digit counts, written digit-major
//            (column d over the tiles), so that launch_exclusive_scan over the 256 columns gives every (digit, tile)
//            its offset inside the digit's bucket, and launch_scan_sums over the 256 totals every bucket its base.
//   scatter  one workgroup per tile, four waves, each owning a contiguous quarter of the tile and walking it in rows
//            of 64 keys in order.  A lane's peers (the lanes of its row with its digit) come from eight ballots; its
//            rank among them is popcount(peers & lanes_below); the row's first peer adds the row's count to the
//            wave's LDS counter of that digit after every peer has read it.  So a key's place is
//              bucket base + (digit, tile) offset + earlier waves' counts + earlier rows' count + rank in the row,
//            every term a count, none an arrival order: equal digits keep their input order, and the whole sort is
//            stable and deterministic.  The first pass takes the record index from the key's position instead of
//            reading it, the last writes the int64 order column and no keys.
//
// Bounds.  keys reads 8 B per record (two columns) and writes 8; a pass reads the keys twice (count, scatter) and the
// 4-byte indices once and writes both: 32 B per key, all streaming but the scatter's stores, which land in 256 runs
// per tile of 8 keys on average (64 B of keys, 32 B of indices).  DESIGN.md §Sort has the measured rates.
#include "sbam_device.h"
#include "sbam_internal.h"
#include "sbam_sort_core.h"

namespace sbam {

namespace {

namespace S = sbam_sort;
typedef unsigned long long u64;

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortRows = kSortTile / kSortThreads;  // rows of 64 keys per wave
constexpr int kHistBlocks = 2048;                    // workgroups of the keys kernel (grid-stride beyond)
static_assert(kSortTile % kSortThreads == 0 && kSortRows >= 1 && kSortRows <= 32, "whole rows per wave");
static_assert(S::kDigits == kSortThreads, "one thread per digit writes the counts");

// counts[d] += the live lanes with digit d.  One LDS atomic per lane, or, when the whole wave holds one digit (a
// constant byte of the keys: the usual case for the high bytes), one for the wave.  Counts only: their order is free.
SB_DEV void count_digit(uint32_t *counts, uint32_t d, bool live, u64 live_mask) {
  if (!live_mask) return;
  const int first = __ffsll((long long)live_mask) - 1;
  const uint32_t d0 = (uint32_t)__shfl((int)d, first, 64);
  if (__ballot(live && d != d0) == 0) {
    if (lane_id() == first) atomicAdd(&counts[d0], (uint32_t)__popcll(live_mask));
  } else if (live) {
    atomicAdd(&counts[d], 1u);
  }
}

// keys[i] (COLS: built from the columns and stored), the out-of-order count and the eight histograms.
// hist: 8 x 256 words by (byte, bin), then the out-of-order count; preset 0.
template <bool COLS>
__global__ void __launch_bounds__(kSortThreads) k_sort_keys(const int32_t *__restrict__ ref_id,
                                                            const int32_t *__restrict__ pos, uint64_t *keys, int64_t n,
                                                            u64 *__restrict__ hist) {
  __shared__ uint32_t sh[S::kMaxPasses * S::kDigits];
  for (int i = threadIdx.x; i < S::kMaxPasses * S::kDigits; i += kSortThreads) sh[i] = 0;
  __syncthreads();
  int64_t below = 0;
  for (int64_t base = (int64_t)blockIdx.x * kSortThreads; base < n; base += (int64_t)gridDim.x * kSortThreads) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < n;
    uint64_t k = 0;
    if (live) {
      k = COLS ? S::key(ref_id[i], pos[i]) : keys[i];
      if (i > 0) below += k < (COLS ? S::key(ref_id[i - 1], pos[i - 1]) : keys[i - 1]);
    }
    if (COLS && live) keys[i] = k;
    const u64 lm = __ballot(live);
#pragma unroll
    for (int b = 0; b < S::kMaxPasses; b++) count_digit(sh + b * S::kDigits, S::digit(k, b), live, lm);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S::kMaxPasses * S::kDigits; i += kSortThreads)
    if (sh[i]) atomicAdd(hist + i, (u64)sh[i]);
  below = wave_sum(below);
  if (lane_id() == 0 && below) atomicAdd(hist + S::kMaxPasses * S::kDigits, (u64)below);
}

// cnt[d * stride + tile] = keys of the tile whose byte `pass` is d
__global__ void __launch_bounds__(kSortThreads) k_sort_count(const uint64_t *__restrict__ keys, int64_t n, int pass,
                                                             int64_t *__restrict__ cnt, int64_t stride) {
  __shared__ uint32_t sh[S::kDigits];
  sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * kSortTile;
#pragma unroll
  for (int r = 0; r < kSortRows; r++) {
    const int64_t i = t0 + r * kSortThreads + threadIdx.x;
    const bool live = i < n;
    const uint32_t d = live ? S::digit(keys[i], pass) : 0u;
    count_digit(sh, d, live, __ballot(live));
  }
  __syncthreads();
  cnt[(int64_t)threadIdx.x * stride + blockIdx.x] = sh[threadIdx.x];
}

// the live lanes of the row whose digit is this lane's
SB_DEV u64 digit_peers(uint32_t d, bool live) {
  u64 m = __ballot(live);
#pragma unroll
  for (int b = 0; b < S::kDigitBits; b++) {
    const bool bit = (d >> b) & 1u;
    const u64 bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// tile blockIdx.x of pass `pass`: toff[d * stride + tile] the tile's offset inside digit d's bucket, dbase[d] the
// bucket's base.  FIRST: the index of a key is its position (iin is not read); LAST: the indices go out as the int64
// order column and the keys are not written.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kSortThreads) k_sort_scatter(const uint64_t *__restrict__ kin,
                                                               const uint32_t *__restrict__ iin,
                                                               uint64_t *__restrict__ kout,
                                                               uint32_t *__restrict__ iout, int64_t *__restrict__ oout,
                                                               int64_t n, int pass, const int64_t *__restrict__ toff,
                                                               int64_t stride, const int64_t *__restrict__ dbase) {
  __shared__ uint32_t wcnt[kSortWaves][S::kDigits];  // per wave and digit: the count so far, then the wave's base
  __shared__ int64_t gbase[S::kDigits];              // the tile's first place in digit d's bucket
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  const u64 below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kSortWaves; k++) wcnt[k][threadIdx.x] = 0;
  gbase[threadIdx.x] = dbase[threadIdx.x] + toff[(int64_t)threadIdx.x * stride + blockIdx.x];
  __syncthreads();
  const int64_t w0 = (int64_t)blockIdx.x * kSortTile + (int64_t)w * (64 * kSortRows) + lane;
  uint64_t key[kSortRows];
  uint32_t rank[kSortRows];
#pragma unroll
  for (int r = 0; r < kSortRows; r++) {
    const int64_t i = w0 + r * 64;
    key[r] = i < n ? kin[i] : 0;
  }
  // rows in order: rank[r] = keys of this wave's earlier rows with the digit + the row's peers below this lane
#pragma unroll
  for (int r = 0; r < kSortRows; r++) {
    const bool live = w0 + r * 64 < n;
    const uint32_t d = S::digit(key[r], pass);
    const u64 peers = digit_peers(d, live);
    const uint32_t before = (uint32_t)__popcll(peers & below);
    const uint32_t seen = live ? wcnt[w][d] : 0u;
    rank[r] = seen + before;
    // every peer has read the counter (one load instruction for the wave, ahead of the store); the row's first peer
    // moves it on, and the next row reads it back from LDS
    __builtin_amdgcn_wave_barrier();
    if (live && before == 0) wcnt[w][d] = seen + (uint32_t)__popcll(peers);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __syncthreads();
  {  // thread d: the waves' counts of digit d -> their exclusive sums
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kSortWaves; k++) {
      const uint32_t c = wcnt[k][threadIdx.x];
      wcnt[k][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRows; r++) {
    const int64_t i = w0 + r * 64;
    if (i >= n) continue;
    const uint32_t d = S::digit(key[r], pass);
    const int64_t p = gbase[d] + wcnt[w][d] + rank[r];
    if ((uint64_t)p >= (uint64_t)n) continue;  // (cannot happen while count and scatter see the same keys)
    const uint32_t idx = FIRST ? (uint32_t)i : iin[i];
    if (LAST) {
      oout[p] = (int64_t)idx;
    } else {
      kout[p] = key[r];
      iout[p] = idx;
    }
  }
}

__global__ void __launch_bounds__(kSortThreads) k_sort_identity(int64_t *__restrict__ order, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kSortThreads + threadIdx.x;
  if (i < n) order[i] = i;
}

// flag |= 1 when an entry of order[0, n) lies outside [0, limit)
__global__ void __launch_bounds__(kSortThreads) k_order_check(const int64_t *__restrict__ order, int64_t n,
                                                              int64_t limit, int32_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * kSortThreads + threadIdx.x;
  const bool bad = i < n && (uint64_t)order[i] >= (uint64_t)limit;
  if (__ballot(bad) && lane_id() == 0) atomicOr(flag, 1);
}

}  // namespace

int64_t sort_tiles(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

hipError_t launch_sort_keys(const int32_t *ref_id, const int32_t *pos, int64_t n, const SortBufs &b, hipStream_t s) {
  hipError_t e = hipMemsetAsync(b.hist, 0, (size_t)kSortHistWords * 8, s);
  if (e != hipSuccess || n <= 0) return e;
  const int64_t blocks = (n + kSortThreads - 1) / kSortThreads;
  const dim3 grid((unsigned)(blocks < kHistBlocks ? blocks : kHistBlocks));
  if (ref_id)
    hipLaunchKernelGGL(k_sort_keys<true>, grid, dim3(kSortThreads), 0, s, ref_id, pos, b.keys[0], n, b.hist);
  else
    hipLaunchKernelGGL(k_sort_keys<false>, grid, dim3(kSortThreads), 0, s, ref_id, pos, b.keys[0], n, b.hist);
  return hipGetLastError();
}

hipError_t launch_sort_pass(const SortBufs &b, int64_t n, int pass, int src, bool first, bool last, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t tiles = sort_tiles(n), stride = tiles + 1;
  const dim3 grid((unsigned)tiles), block(kSortThreads);
  hipLaunchKernelGGL(k_sort_count, grid, block, 0, s, b.keys[src], n, pass, b.cnt, stride);
  hipError_t e = launch_exclusive_scan(b.cnt, stride, tiles, S::kDigits, b.bsum, b.totals, s);
  if (e != hipSuccess) return e;
  e = launch_scan_sums(b.totals, b.dbase, S::kDigits, 1, b.dbase + S::kDigits, s);
  if (e != hipSuccess) return e;
  const uint64_t *kin = b.keys[src];
  const uint32_t *iin = b.idx[src];
  uint64_t *kout = b.keys[src ^ 1];
  uint32_t *iout = b.idx[src ^ 1];
#define SBAM_SCATTER(F, L)                                                                                        \
  hipLaunchKernelGGL((k_sort_scatter<F, L>), grid, block, 0, s, kin, iin, kout, iout, b.order, n, pass, b.cnt, stride, \
                     b.dbase)
  if (first && last) SBAM_SCATTER(true, true);
  else if (first) SBAM_SCATTER(true, false);
  else if (last) SBAM_SCATTER(false, true);
  else SBAM_SCATTER(false, false);
#undef SBAM_SCATTER
  return hipGetLastError();
}

hipError_t launch_sort_identity(int64_t *order, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sort_identity, dim3((unsigned)((n + kSortThreads - 1) / kSortThreads)), dim3(kSortThreads), 0,
                     s, order, n);
  return hipGetLastError();
}

hipError_t launch_order_check(const int64_t *order, int64_t n, int64_t limit, int32_t *flag, hipStream_t s) {
  hipError_t e = hipMemsetAsync(flag, 0, 8, s);
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(k_order_check, dim3((unsigned)((n + kSortThreads - 1) / kSortThreads)), dim3(kSortThreads), 0, s,
                     order, n, limit, flag);
  return hipGetLastError();
}

}  // namespace sbam
