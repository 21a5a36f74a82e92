// sbam_tags.hip — selected tags of decoded records as typed device columns (gfx950).
//
// Reference: htsjdk SAMRecord.getAttribute(tag) over the records BAMRecordCodec.decode builds behind RecordStream
// (check/src/main/scala/org/hammerlab/bam/iterator/RecordStream.scala:16-33), i.e. what loadReads' callers ask their
// SAMRecords (CanLoadBam.scala:221-241); tag layout: SAM spec §4.2.4.  For records [i0, i0 + n) of the last
// sbam_load_records and a query of up to 32 tag names, four tag-major columns (type, sub, rel, value) and, per
// want_bytes entry, a CSR column of the value's bytes.
//
//   walk     a workgroup of 256 threads owns 256 consecutive records.  Every thread computes its record's tag range
//            from the fixed-field columns (field_lens: the stream is not touched) and the workgroup scans the ranges'
//            sizes.  In rounds, the next run of records whose tag bytes fit the 30 KiB LDS stage is copied there as
//            aligned dwords, the work divided over dwords (a record keeps its alignment mod 4), and then one
//            lane per record walks its list in LDS: sbam_tag::walk validates every tag and notes the header position
//            of the first occurrence of each queried name (uint16, in LDS); after the walk the lanes of a wave write
//            the cells of one query entry at a time, consecutive records to consecutive addresses.  `present` is
//            counted per workgroup in LDS and added to one of 64 global slots per entry, which the host sums.
//   long     a record with more than kLongAuxBytes tag bytes is not staged: after the rounds the workgroup's waves
//            take its long records in turn and walk them in global memory, lane 0 reading each header (8 bytes,
//            broadcast) and all 64 lanes searching a Z or H value's NUL 256 bytes a step with a ballot.
//   scan     the byte columns' lengths become exclusive int64 prefix sums in place (launch_exclusive_scan,
//            sbam_scan.hip), one grid row per column.
//   bytes    sbam_fields.hip's gather (work divided over output bytes) with each record's source position taken from
//            the column the walk wrote: record offset + tag start + rel.
//
// LDS per workgroup: 35 856 B static (the 30 KiB stage, 5 KiB of per-record ranges, the long-record list, the query
// and its counters) + 512 B per query entry (found positions): 4 workgroups (16 waves) per CU up to 9 entries, 3 from 10 to 32;
// 54 VGPRs, so registers do not limit it.  A lane's LDS reads are aligned dwords (three
// per header) and single bytes (NUL search) at record-dependent addresses: ds_read_b32 banking, (a / 4) mod 32 per
// 32-lane half; records start at arbitrary stage offsets, so conflicts are those of random addresses, not a stride's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbam_device.h"
#include "sbam_internal.h"
#include "sbam_tag_core.h"

namespace sbam {

namespace {

constexpr int kWalkThreads = 256;  // records per workgroup
constexpr int kWalkWaves = kWalkThreads / 64;
constexpr int kStageBytes = 30720;
static_assert(sbam_tag::kLongAuxBytes + 8 <= kStageBytes, "one short record must fit the stage");
static_assert(sbam_tag::kLongAuxBytes < 65536, "found positions are uint16");

// exclusive prefix sums of one int32 per thread over the workgroup into pre[0 .. kWalkThreads]
SB_DEV void walk_scan(int32_t v, int32_t *pre, int32_t *ws) {
  int32_t total;
  pre[threadIdx.x + 1] = block_incl_scan<int32_t, kWalkThreads>(v, total, ws);
  if (threadIdx.x == 0) pre[0] = 0;
  __syncthreads();
}

// the cell of query entry j of batch record k: absent, or the decoded tag c of a record whose tag bytes start at
// stream offset x
SB_DEV void write_cell(const TagWalkArgs &a, int j, int b, int64_t k, bool found, const sbam_tag::Cell &c, int64_t x) {
  const int64_t idx = (int64_t)j * a.rec.n + k;
  a.type[idx] = found ? (uint8_t)c.type : 0;
  a.sub[idx] = found ? (uint8_t)c.sub : 0;
  a.rel[idx] = found ? c.rel : -1;
  a.value[idx] = found ? c.value : 0;
  if (b >= 0) {
    a.off[b * a.ostride + k] = found && sbam_tag::has_bytes(c.type) ? c.len : 0;
    a.src[b * a.rec.n + k] = found ? x + c.rel : 0;
  }
}

// A long record (n tag bytes at stream offset x), walked by the whole wave; every value here is wave-uniform.
SB_DEV void wave_walk(const TagWalkArgs &a, const uint16_t *skey, const int8_t *sbcol, uint32_t *spresent, int64_t k,
                       int64_t x, int32_t n) {
  const int lane = threadIdx.x & 63;
  const uint8_t *__restrict__ g = a.u + x;
  auto hdr = [&](int32_t p, int32_t cnt) -> uint64_t {
    uint32_t lo = 0, hi = 0;
    if (lane == 0) {
      for (int i = 0; i < 4; i++) {
        if (i < cnt) lo |= (uint32_t)g[p + i] << (8 * i);
        if (4 + i < cnt) hi |= (uint32_t)g[p + 4 + i] << (8 * i);
      }
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    return (uint64_t)lo | ((uint64_t)hi << 32);
  };
  auto nul = [&](int32_t from, int32_t end) -> int32_t {
    for (int32_t q = sbam_tag::nul_first_step(x, from); q < end; q += sbam_tag::kNulStepBytes) {
      const int32_t q0 = q + 4 * lane;
      // (aligned in the stream; a dword that straddles the record's end lies inside the stream's pad)
      const uint32_t w = q0 < end ? *reinterpret_cast<const uint32_t *>(g + q0) : 0xffffffffu;
      const int32_t hit = sbam_tag::lane_first_nul(w, q0, from, end);
      const unsigned long long m = __ballot(hit >= 0);
      if (m) return __shfl(hit, __ffsll((long long)m) - 1);
    }
    return -1;
  };
  uint32_t seen = 0;
  const bool ok = sbam_tag::walk(hdr, nul, n, [&](const sbam_tag::Cell &c) {
    if (!((a.filter >> sbam_tag::filter_bit(c.key)) & 1ull)) return;
    for (int j = 0; j < a.nq; j++) {
      if (skey[j] != c.key || ((seen >> j) & 1u)) continue;
      seen |= 1u << j;
      if (lane == 0) {
        write_cell(a, j, sbcol[j], k, true, c, x);
        atomicAdd(&spresent[j], 1u);
      }
    }
  });
  if (!ok && lane == 0) atomicMin(a.first_bad, (unsigned long long)k);
  if (lane < a.nq && !((seen >> lane) & 1u)) write_cell(a, lane, sbcol[lane], k, false, sbam_tag::Cell{}, x);
}

__global__ void __launch_bounds__(kWalkThreads) k_tag_walk(TagWalkArgs a) {
  extern __shared__ uint16_t sfound[];  // [nq][kWalkThreads]: header position of the entry's first occurrence
  __shared__ uint32_t sstage[kStageBytes / 4 + 4];  // (+ the dwords a header read may take behind the last record)
  __shared__ int64_t sstart[kWalkThreads];          // stream offset of each record's tag bytes
  __shared__ int32_t slen[kWalkThreads];            // and their number
  __shared__ int32_t spre[kWalkThreads + 1];        // exclusive sums of the records' stage slots (bytes)
  __shared__ int32_t sws[kWalkWaves];
  __shared__ uint16_t slong[kWalkThreads];
  __shared__ int32_t snlong;
  __shared__ uint16_t skey[sbam_tag::kMaxTags];
  __shared__ int8_t sbcol[sbam_tag::kMaxTags];
  __shared__ uint32_t spresent[sbam_tag::kMaxTags];  // the workgroup's records that have each entry
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t k0 = (int64_t)blockIdx.x * kWalkThreads, k = k0 + tid;
  const int cnt = (int)(a.rec.n - k0 < kWalkThreads ? a.rec.n - k0 : kWalkThreads);
  if (tid < sbam_tag::kMaxTags) {
    skey[tid] = a.key[tid];
    sbcol[tid] = a.bcol[tid];
    spresent[tid] = 0;
  }
  if (tid == 0) snlong = 0;
  FieldLens r{{0, 0, 0, 0}, false};
  if (tid < cnt) r = field_lens(a.rec, k);
  if (r.bad) atomicMin(a.first_bad, (unsigned long long)k);
  const bool good = tid < cnt && !r.bad;
  const int32_t len = (int32_t)r.v[3];
  const int64_t x = good ? a.rec.roff[k] + 4 + a.rec.block_size[k] - len : 0;
  const bool lane_walks = good && len <= sbam_tag::kLongAuxBytes;
  const int32_t slot = lane_walks ? (int32_t)(((x & 3) + len + 3) & ~(int64_t)3) : 0;
  sstart[tid] = x;
  slen[tid] = len;
  __syncthreads();  // (snlong is 0)
  if (good && !lane_walks) slong[atomicAdd(&snlong, 1)] = (uint16_t)tid;
  walk_scan(slot, spre, sws);

  const uint8_t *stage8 = reinterpret_cast<const uint8_t *>(sstage);
  int base = 0;
  while (base < cnt) {
    // the records of this round: the longest run from `base` whose slots fit the stage (never empty: one slot does)
    const int32_t p0 = spre[base];
    const bool fits = tid >= base && tid < cnt && spre[tid + 1] - p0 <= kStageBytes;
    const int end = base + __syncthreads_count(fits);  // (also: the previous round's lanes are done with the stage)
    // the copy is divided over the round's dwords, not its records: a thread finds the record that owns its dword
    // in spre (the last one whose slot starts at or below it; empty slots are passed over).  (One record per wave and
    // step left 56 of 64 lanes idle on 27-byte lists and made every record a dependent trip to memory.)
    const int32_t round_dwords = (spre[end] - p0) >> 2;
#pragma unroll 4
    for (int32_t i = tid; i < round_dwords; i += kWalkThreads) {
      const int32_t o = p0 + 4 * i;
      int lo = base, hi = end - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (spre[mid] <= o) lo = mid;
        else hi = mid - 1;
      }
      const uint32_t *__restrict__ gw = reinterpret_cast<const uint32_t *>(a.u + (sstart[lo] & ~(int64_t)3));
      sstage[i] = gw[(o - spre[lo]) >> 2];
    }
    __syncthreads();
    if (fits && lane_walks) {
      const int32_t sb = spre[tid] - p0 + (int32_t)(x & 3);  // the record's first tag byte in the stage
      auto hdr = [&](int32_t p, int32_t) -> uint64_t {
        const uint32_t o = (uint32_t)(sb + p), s = o & 3u;
        const uint32_t *w = sstage + (o >> 2);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, s) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, s) << 32);
      };
      auto nul = [&](int32_t from, int32_t n) -> int32_t {
        for (int32_t e = from; e < n; e++)
          if (stage8[sb + e] == 0) return e;
        return -1;
      };
      uint32_t seen = 0;
      const bool ok = sbam_tag::walk(hdr, nul, len, [&](const sbam_tag::Cell &c) {
        if (!((a.filter >> sbam_tag::filter_bit(c.key)) & 1ull)) return;
        for (int j = 0; j < a.nq; j++) {
          if (skey[j] != c.key || ((seen >> j) & 1u)) continue;
          seen |= 1u << j;
          sfound[j * kWalkThreads + tid] = (uint16_t)c.pos;
        }
      });
      if (!ok) atomicMin(a.first_bad, (unsigned long long)k);
      // (a malformed record's cells are written too, from what was seen in front of the bad tag: the host discards
      // the batch)
      for (int j = 0; j < a.nq; j++) {
        const bool found = (seen >> j) & 1u;
        sbam_tag::Cell c{};
        if (found) c = sbam_tag::decode_at(hdr, nul, len, (int32_t)sfound[j * kWalkThreads + tid]);
        write_cell(a, j, sbcol[j], k, found, c, x);
        const unsigned long long m = __ballot(found);
        if (found && lane == __ffsll((long long)m) - 1) atomicAdd(&spresent[j], (uint32_t)__popcll(m));
      }
    }
    base = end;
  }
  __syncthreads();
  const int nlong = snlong;
  for (int i = wave; i < nlong; i += kWalkWaves) {
    const int t = slong[i];
    wave_walk(a, skey, sbcol, spresent, k0 + t, sstart[t], slen[t]);
  }
  // one global atomic per workgroup and entry, spread over kTagPresentSlots addresses per entry: one per wave on a
  // single address serialised in L2 and cost more than the walk
  __syncthreads();
  if (tid < a.nq && spresent[tid])
    atomicAdd(&a.present[(blockIdx.x % kTagPresentSlots) * sbam_tag::kMaxTags + tid], (unsigned long long)spresent[tid]);
}

}  // namespace

int tag_long_aux_bytes() { return sbam_tag::kLongAuxBytes; }

hipError_t launch_tag_walk(const TagWalkArgs &a, hipStream_t s) {
  if (a.rec.n <= 0) return hipSuccess;
  const int64_t nblk = (a.rec.n + kWalkThreads - 1) / kWalkThreads;
  hipLaunchKernelGGL(k_tag_walk, dim3((unsigned)nblk), dim3(kWalkThreads), (size_t)a.nq * kWalkThreads * sizeof(uint16_t),
                     s, a);
  return hipGetLastError();
}

}  // namespace sbam
