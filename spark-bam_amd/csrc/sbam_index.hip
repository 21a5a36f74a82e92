// sbam_index.hip — the BAI index (SAM spec §5.2, §5.3) from the decoded record columns (gfx950).
//
// Reference: the reference reads a .bai (check/src/main/scala/org/hammerlab/bam/index/Index.scala:53-90) and hands
// it to htsjdk for loadBamIntervals (CanLoadBam.scala:59-138); it writes none.  The writer's rules are the SAM
// spec's and the usual samtools/htslib indexer's, pinned by the reference's 2.bam.bai and 5k.bam.bai.
//
// Everything is data-parallel over the records of the last sbam_load_records, in file order:
//
//   spans    one lane per record: beg, end (the CIGAR's reference length: M, D, N, =, X) and reg2bin(beg, end) into two
//            scratch columns; a record with more than kLongCigar ops is summed by its whole wave.  A record whose
//            ref_id, end or CIGAR breaks the rules lowers the first-error word (its stream offset).
//   stats    one lane per record: run head (the (ref_id, bin) of record i - 1 differs), order violation, and the
//            per-reference counters, reduced inside the wave before any global atomic (a coordinate-sorted file has
//            one reference per wave almost everywhere); per-workgroup head counts for the compaction.
//   scan     launch_scan_sums: exclusive sums of the head counts, their total = n_runs.
//   runs     scan of the head flags inside the workgroup; a head scatters (ref, bin, vbeg), a tail its vend.
//   linear   one lane per record: atomicMin(vbeg) into every 16 kb window the record touches that record i - 1 does
//            not touch on the same reference (the predecessor's vbeg is smaller, so skipping is exact for any order
//            and leaves about one atomic per window); then one wave per reference fills untouched windows backwards.
//
// Virtual offsets: vbeg = block_pos << 16 | block_off of the record's columns; vend = the same Pos rule at
// offset + 4 + block_size, which is the next record's vbeg when that record starts there, else a search of the
// block table (launch_record_columns' rule: last block with uoff <= x, advanced past exhausted blocks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbam_device.h"
#include "sbam_internal.h"

namespace sbam {

namespace {

constexpr int kIndexThreads = 1024;  // records per workgroup (sixteen waves)
constexpr uint32_t kLongCigar = 16;  // ops above which a record's CIGAR is summed by the whole wave
constexpr int64_t kMaxEnd = 1ll << 29;
typedef unsigned long long u64;

// the little-endian dword at x from the two aligned dwords around it (the stream is 4-byte aligned and padded)
SB_DEV uint32_t rd_u32(const uint8_t *u, int64_t x) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(u + (x & ~(int64_t)3));
  return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(x & 3));
}

SB_DEV uint32_t op_ref_len(uint32_t op) {
  const uint32_t t = op & 0xfu;
  return (t == 0 || t == 2 || t == 3 || t == 7 || t == 8) ? op >> 4 : 0u;
}

// reg2bin with a 14-bit minimum shift and 5 levels (SAM spec §5.3); e = end - 1 may be negative (bin 0)
SB_DEV uint32_t reg2bin(int64_t beg, int64_t end) {
  const int64_t e = end - 1;
  if (beg >> 14 == e >> 14) return (uint32_t)(4681 + (beg >> 14));
  if (beg >> 17 == e >> 17) return (uint32_t)(585 + (beg >> 17));
  if (beg >> 20 == e >> 20) return (uint32_t)(73 + (beg >> 20));
  if (beg >> 23 == e >> 23) return (uint32_t)(9 + (beg >> 23));
  if (beg >> 26 == e >> 26) return (uint32_t)(1 + (beg >> 26));
  return 0;
}

SB_DEV u64 vbeg_of(const IndexArgs &a, int64_t i) {
  return ((u64)a.block_pos[i] << 16) | (u64)(uint32_t)a.block_off[i];
}

SB_DEV u64 vend_of(const IndexArgs &a, int64_t i) {
  const int64_t x = a.roff[i] + 4 + (int64_t)a.block_size[i];
  if (i + 1 < a.n && a.roff[i + 1] == x) return vbeg_of(a, i + 1);
  int64_t lo = 0, hi = a.nblocks;  // first block with uoff > x
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.buoff[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  int64_t b = lo - 1;
  if (b < 0) return (u64)a.file_base << 16;
  while (b < a.nblocks && x >= a.buoff[b] + a.busize[b]) b++;
  if (b >= a.nblocks)  // past the last data block: the address behind it (the EOF marker's)
    return (u64)(a.file_base + a.bstart[a.nblocks - 1] + a.bcsize[a.nblocks - 1]) << 16;
  return ((u64)(a.file_base + a.bstart[b]) << 16) | (u64)(x - a.buoff[b]);
}

SB_DEV int64_t beg_of(const IndexArgs &a, int64_t i) {
  const int64_t p = a.pos[i];
  return p < 0 ? 0 : p;
}

SB_DEV bool placed(const IndexArgs &a, int64_t i) { return (uint32_t)a.ref_id[i] < (uint32_t)a.nref; }

// spans: end_out[i], bin_out[i] of every record; a[0] of the stats words = first offending stream offset
__global__ void __launch_bounds__(kIndexThreads) k_index_spans(IndexArgs a, IndexStats st) {
  const int64_t i = (int64_t)blockIdx.x * kIndexThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < a.n;
  const int32_t ref = live ? a.ref_id[i] : -1;
  bool bad = live && ref >= a.nref;
  int64_t x = 0, cig = 0, rlen = 0;
  uint32_t nc = 0, flag = 0;
  bool walk = false;  // the CIGAR is read: a mapped record on a reference, its ops inside the record and the stream
  if (live && ref >= 0) {
    x = a.roff[i];
    const int64_t bs = a.block_size[i];
    const uint32_t fnc = a.flag_nc[i];
    nc = fnc & 0xffffu;
    flag = fnc >> 16;
    cig = x + 36 + (int64_t)(a.bin_mq_nl[i] & 0xffu);
    if (bs < 32 || cig + 4 * (int64_t)nc > x + 4 + bs || x + 4 + bs > a.L) bad = true;
    walk = !bad && !(flag & 4u) && nc > 0;
  }
  if (walk && nc <= kLongCigar)
    for (uint32_t k = 0; k < nc; k++) rlen += op_ref_len(rd_u32(a.u, cig + 4 * (int64_t)k));
  // long CIGARs: one record after another, 64 ops per step across the wave
  u64 m = __ballot(walk && nc > kLongCigar);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int64_t c0 = __shfl((long long)cig, src);
    const uint32_t n0 = (uint32_t)__shfl((int)nc, src);
    int64_t s = 0;
    for (uint32_t k = (uint32_t)lane; k < n0; k += 64) s += op_ref_len(rd_u32(a.u, c0 + 4 * (int64_t)k));
    s = wave_sum(s);
    if (lane == src) rlen = s;
  }
  if (!live) return;
  const int64_t p = a.pos[i];
  int64_t beg = p < 0 ? 0 : p;
  int64_t end = (walk && rlen > 0) ? p + rlen : beg + 1;
  if (ref >= 0 && end > kMaxEnd) bad = true;
  if (bad) {  // (the later passes still run before the host reads the error: keep their inputs in range)
    atomicMin(st.w, (u64)a.roff[i]);
    beg = beg < kMaxEnd ? beg : kMaxEnd - 1;
    end = beg + 1;
  }
  a.end_out[i] = (int32_t)end;
  a.bin_out[i] = reg2bin(beg, end);
}

// stats: the per-reference counters, the scalars, and heads[b] = run heads of workgroup b
__global__ void __launch_bounds__(kIndexThreads) k_index_stats(IndexArgs a, IndexStats st, int64_t *__restrict__ heads) {
  __shared__ int ws[kIndexThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kIndexThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < a.n;
  const int32_t ref = live ? a.ref_id[i] : INT32_MIN;
  const bool on_ref = live && placed(a, i);
  int head = 0, unsorted = 0;
  int64_t mapped = 0, unmapped = 0;
  u64 vb = ~0ull, ve = 0, nintv = 0;
  if (live && i > 0) {
    const uint32_t r0 = (uint32_t)a.ref_id[i - 1], r1 = (uint32_t)ref;
    unsorted = r1 < r0 || (r1 == r0 && a.pos[i] < a.pos[i - 1]);
  }
  if (on_ref) {
    head = i == 0 || a.ref_id[i - 1] != ref || a.bin_out[i - 1] != a.bin_out[i];
    const bool un = (a.flag_nc[i] >> 16) & 4u;
    mapped = !un;
    unmapped = un;
    vb = vbeg_of(a, i);
    ve = vend_of(a, i);
    const int64_t e = (int64_t)a.end_out[i] - 1;
    nintv = e >= 0 ? (u64)(e >> 14) + 1 : 0;
  }
  // lanes on the first lane's reference are reduced in the wave; the others (a reference boundary) go direct
  const int32_t ref0 = __shfl(ref, 0);
  const bool same = on_ref && ref == ref0;
  const int64_t sm = wave_sum(same ? mapped : 0), su = wave_sum(same ? unmapped : 0);
  const u64 mb = wave_min(same ? vb : ~0ull), me = wave_max(same ? ve : 0), mi = wave_max(same ? nintv : 0);
  const int64_t nocoor = wave_sum((int64_t)(live && ref < 0)), uns = wave_sum((int64_t)unsorted);
  if (lane == 0) {
    if ((uint32_t)ref0 < (uint32_t)a.nref && live) {
      if (sm) atomicAdd(st.n_mapped + ref0, (u64)sm);
      if (su) atomicAdd(st.n_unmapped + ref0, (u64)su);
      atomicMin(st.off_beg + ref0, mb);
      atomicMax(st.off_end + ref0, me);
      atomicMax(st.n_intv + ref0, mi);
    }
    if (nocoor) atomicAdd(st.w + 1, (u64)nocoor);
    if (uns) atomicAdd(st.w + 2, (u64)uns);
  }
  if (on_ref && !same) {
    atomicAdd((mapped ? st.n_mapped : st.n_unmapped) + ref, 1ull);
    atomicMin(st.off_beg + ref, vb);
    atomicMax(st.off_end + ref, ve);
    atomicMax(st.n_intv + ref, nintv);
  }
  int total;
  (void)block_incl_scan<int, kIndexThreads>(head, total, ws);
  if (threadIdx.x == 0) heads[blockIdx.x] = total;
}

// runs: run k = (ref, bin, vbeg of its head, vend of its tail); heads[] holds the exclusive sums
__global__ void __launch_bounds__(kIndexThreads) k_index_runs(IndexArgs a, const int64_t *__restrict__ heads,
                                                              IndexRuns r) {
  __shared__ int ws[kIndexThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kIndexThreads + threadIdx.x;
  const bool on_ref = i < a.n && placed(a, i);
  int head = 0, tail = 0;
  if (on_ref) {
    const int32_t ref = a.ref_id[i];
    const uint32_t bin = a.bin_out[i];
    head = i == 0 || a.ref_id[i - 1] != ref || a.bin_out[i - 1] != bin;
    tail = i + 1 == a.n || a.ref_id[i + 1] != ref || a.bin_out[i + 1] != bin;
  }
  int total;
  const int incl = block_incl_scan<int, kIndexThreads>(head, total, ws);
  if (!on_ref) return;
  const int64_t k = heads[blockIdx.x] + incl - 1;  // the run this record belongs to
  if (k < 0 || k >= r.n) return;
  if (head) {
    r.ref[k] = a.ref_id[i];
    r.bin[k] = a.bin_out[i];
    r.beg[k] = vbeg_of(a, i);
  }
  if (tail) r.end[k] = vend_of(a, i);
}

// linear: ioffset[intv_off[ref] + w] = min vbeg over the records that touch window w
__global__ void __launch_bounds__(256) k_index_linear(IndexArgs a, const int64_t *__restrict__ intv_off,
                                                      u64 *__restrict__ ioffset) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || !placed(a, i)) return;
  const int32_t ref = a.ref_id[i];
  const int64_t w0 = beg_of(a, i) >> 14, w1 = ((int64_t)a.end_out[i] - 1) >> 14;
  int64_t p0 = 1, p1 = 0;  // the predecessor's windows on this reference (none: empty)
  if (i > 0 && a.ref_id[i - 1] == ref) {
    p0 = beg_of(a, i - 1) >> 14;
    p1 = ((int64_t)a.end_out[i - 1] - 1) >> 14;
  }
  const int64_t base = intv_off[ref], cap = intv_off[ref + 1] - base;
  const u64 vb = vbeg_of(a, i);
  for (int64_t w = w0; w <= w1 && w < cap; w++) {
    if (w >= p0 && w <= p1) {  // covered by the predecessor, whose vbeg is smaller: skip to its last window
      w = p1;
      continue;
    }
    atomicMin(ioffset + base + w, vb);
  }
}

// fill: one wave per reference, from the last window down: an untouched window (~0) takes the next touched one
__global__ void __launch_bounds__(64) k_index_fill(const int64_t *__restrict__ intv_off, u64 *__restrict__ ioffset) {
  const int lane = threadIdx.x;
  const int64_t base = intv_off[blockIdx.x], n = intv_off[blockIdx.x + 1] - base;
  u64 *t = ioffset + base;
  u64 carry = ~0ull;
  for (int64_t b = ((n - 1) >> 6) << 6; n > 0 && b >= 0; b -= 64) {
    const int64_t w = b + lane;
    u64 v = w < n ? t[w] : ~0ull;
    for (int o = 1; o < 64; o <<= 1) {
      const u64 x = __shfl_down(v, o);
      if (lane + o < 64 && v == ~0ull) v = x;
    }
    if (v == ~0ull) v = carry;
    if (w < n) t[w] = v;
    carry = __shfl(v, 0);
  }
}

}  // namespace

int64_t index_blocks(int64_t n) { return (n + kIndexThreads - 1) / kIndexThreads; }
int index_long_cigar_ops() { return (int)kLongCigar; }

hipError_t launch_index_pass1(const IndexArgs &a, IndexStats st, int64_t *heads, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int64_t nblk = index_blocks(a.n);
  hipLaunchKernelGGL(k_index_spans, dim3((unsigned)nblk), dim3(kIndexThreads), 0, s, a, st);
  hipLaunchKernelGGL(k_index_stats, dim3((unsigned)nblk), dim3(kIndexThreads), 0, s, a, st, heads);
  return launch_scan_sums(heads, heads, nblk, 1, reinterpret_cast<int64_t *>(st.w + 3), s);
}

hipError_t launch_index_pass2(const IndexArgs &a, const int64_t *heads, IndexRuns r, const int64_t *intv_off,
                              unsigned long long *ioffset, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_index_runs, dim3((unsigned)index_blocks(a.n)), dim3(kIndexThreads), 0, s, a, heads, r);
  hipLaunchKernelGGL(k_index_linear, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, intv_off, ioffset);
  if (a.nref > 0) hipLaunchKernelGGL(k_index_fill, dim3((unsigned)a.nref), dim3(64), 0, s, intv_off, ioffset);
  return hipGetLastError();
}

}  // namespace sbam
