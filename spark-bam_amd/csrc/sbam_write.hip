// sbam_write.hip — the BAM writer's kernels: select, deflate and BGZF framing (gfx950, wave64).
//
// Reference: htsjdk-rewrite (cli/src/main/scala/org/hammerlab/bam/rewrite/HTSJDKRewrite.scala:21-91) sends records
// through htsjdk's SAMFileWriter, whose BlockCompressedOutputStream cuts the uncompressed stream (header, then the
// records back to back) every 65 498 bytes, deflates each piece and frames it as a BGZF block.  Here:
//
//   select   one thread per entry (loaded record k, or record order[k] of an ordered write): selected (inside a range,
//            and kept, both by the record's loaded index) -> its length 4 + block_size and a 1 into
//            two int64 columns, which launch_exclusive_scan turns into each record's offset in the output stream and
//            its ordinal among the written records.  Entry 0 of the columns is the BAM header, a pseudo-record at
//            stream offset 0.  The bytes are then copied by sbam_fields.hip's gather (field 5: work divided over
//            output bytes, so a 100-byte read and a 100 kB one cost the same per byte).
//   deflate  one wavefront (one workgroup) per output block.  Level 1 walks the block in rows of 64 positions, one per
//            lane: a lane hashes the four bytes at its position into a per-wave LDS table of 2^13 positions, takes the
//            entry as its candidate (entries left by earlier rows; the row's own positions enter the table after the
//            lookup, by an LDS atomic max, so two lanes of a row that meet in a bucket leave the larger position
//            whatever the order of their stores), extends it by 8-byte compares, and a ballot-driven greedy pass
//            picks the row's tokens in position order.  Token lengths come from sbam_deflate_core.h, a wave scan gives
//            every token its bit position, and the tokens are ORed into a 64-word LDS stage whose full words go out by
//            plain stores.  A block whose fixed-Huffman form would pass the stored size (n + 5 bytes) stops at that
//            bound and is marked stored: the kernel never writes past its slot.
//            Level 1 | SBAM_WRITE_DYNAMIC (k_deflate_dynamic) runs the same row walk and match search, but a row's
//            tokens go to a record in global memory (16-bit entries: a literal one, a match two) and into two LDS
//            histograms.  The wave then builds the literal/length and distance codes with sbam_deflate_core.h's
//            builder (the sort by rank across the lanes, the tree, the length limit and the canonical codes by lane 0
//            in the space the hash table no longer needs), plans the header, prices the stored, fixed and dynamic
//            forms from the histograms and emits the smallest: the header through the LDS stage, then the record in
//            rows of 64 entries, each looked up in the code tables in LDS (the fixed code loaded into the same tables
//            when that form wins).  The size is known before the first bit, so no block stops at the bound.
//   frame   one wavefront per block, eight per workgroup: CRC32 of the block's slice of the stream
//            (sbam_crc_core.h), the 18 header bytes with BSIZE, the payload from its slot (a stored block's bytes
//            straight from the stream), CRC32 and ISIZE; the wave behind the last block writes the EOF block.
//
// Bounds.  select and frame move every byte once (frame reads the stream for the CRC and, for a stored block, once
// more for the copy).  deflate is latency-bound inside a wave: per row one dependent chain of a stream load, an LDS
// lookup, the compare loop (divergent: the row waits for its longest match), a serial loop over the row's matches and
// three LDS round trips for the stage; the grid supplies the parallelism (one block per wave, four waves' tables per
// CU's 160 KB of LDS).  DESIGN.md §BAM writer has the measured rates.
#include "sbam_crc_core.h"
#include "sbam_deflate_core.h"
#include "sbam_device.h"
#include "sbam_internal.h"

namespace sbam {

namespace {

namespace D = sbam_deflate;

constexpr int kSelectThreads = 256;
constexpr int kTabEntries = 1 << D::kHashBits;
constexpr int kStageWords = 64;  // carry (< 32 bits) + 64 tokens x 31 bits = 2015 bits at most
constexpr int kFrameWaves = 8;

// the last range r with lo[r] <= i contains i?  (ranges ascending and disjoint)
SB_DEV bool in_ranges(const int64_t *__restrict__ lo, const int64_t *__restrict__ hi, int64_t nr, int64_t i) {
  if (nr == 0) return true;
  int64_t a = 0, b = nr;  // first range with lo > i
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (lo[m] <= i) a = m + 1;
    else b = m;
  }
  return a > 0 && i < hi[a - 1];
}

__global__ void __launch_bounds__(kSelectThreads) k_write_select(WriteSelectArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;  // entry: 0 the header, 1 + r record r
  if (i > a.n) return;
  int64_t len = a.header_bytes, cnt = 0, src = 0;
  if (i > 0) {
    int64_t r = i - 1;
    if (a.order) r = a.order[r];
    const bool known = (uint64_t)r < (uint64_t)a.n;  // (the host has checked a caller's order before this launch)
    r = known ? r : 0;
    const int32_t bs = a.block_size[r];
    src = a.roff[r];
    len = 4 + (int64_t)(bs < 0 ? 0 : bs);
    bool sel = known && in_ranges(a.range_lo, a.range_hi, a.n_ranges, r) && (!a.keep || a.keep[r] != 0);
    sel = sel && src >= 0 && src + len <= a.L;  // (every loaded record lies inside the stream)
    len = sel ? len : 0;
    cnt = sel ? 1 : 0;
  }
  a.len[i] = len;
  a.cnt[i] = cnt;
  a.src[i] = src;
}

// Pos of every written record: entry 1 + k of the scanned columns is the k-th entry's stream offset and ordinal
__global__ void __launch_bounds__(kSelectThreads) k_written_records(const int64_t *__restrict__ off,
                                                                    const int64_t *__restrict__ ord, int64_t n,
                                                                    int32_t block_bytes,
                                                                    const int64_t *__restrict__ start,
                                                                    int64_t *__restrict__ block_pos,
                                                                    int32_t *__restrict__ block_off) {
  const int64_t i = 1 + (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  if (i > n || ord[i + 1] == ord[i]) return;
  const int64_t x = off[i], b = x / block_bytes;
  block_pos[ord[i]] = start[b];
  block_off[ord[i]] = (int32_t)(x - b * block_bytes);
}

// geometry of block b: its first stream byte and its length
SB_DEV int block_len(const WriteBlocksArgs &a, int64_t b, int64_t *uo) {
  *uo = b * a.block_bytes;
  const int64_t left = a.ubytes - *uo;
  return (int)(left < a.block_bytes ? left : a.block_bytes);
}

// level 0: every block is stored
__global__ void __launch_bounds__(kSelectThreads) k_stored_sizes(WriteBlocksArgs a) {
  const int64_t k = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  if (k >= a.nb) return;
  int64_t uo;
  const int n = block_len(a, a.b0 + k, &uo);
  a.pay[a.b0 + k] = n + D::kStoredHeader;
  a.stored[a.b0 + k] = 1;
  a.tsz[k] = 26 + n + D::kStoredHeader;
}

// level 1: LZ77 + the fixed Huffman code; one wave per block, striding over the batch
__global__ void __launch_bounds__(64) k_deflate_fixed(WriteBlocksArgs a) {
  __shared__ uint32_t tab[kTabEntries];  // bucket -> 1 + the largest position seen with that hash (0: none)
  __shared__ uint32_t stage[kStageWords];
  const int lane = threadIdx.x;
  for (int64_t k = blockIdx.x; k < a.nb; k += gridDim.x) {
    int64_t uo;
    const int n = block_len(a, a.b0 + k, &uo);
    uint32_t *__restrict__ out = reinterpret_cast<uint32_t *>(a.slots + k * a.slot_stride);
    const int limit = n + D::kStoredHeader;  // bytes of the stored form: the Huffman form may not pass it
    __syncthreads();                         // (the previous block's last reads of the stage)
    for (int i = lane; i < kTabEntries; i += 64) tab[i] = 0;
    stage[lane] = lane == 0 ? D::kHeaderValue : 0u;
    __syncthreads();
    int carry = D::kHeaderBits;  // bits in the stage
    int wbase = 0;               // words already in the slot
    bool stored = false;
    int pos = 0;
    while (pos < n) {
      const int W = n - pos < 64 ? n - pos : 64;
      const int p = pos + lane;
      int len = 0, dist = 0;
      uint32_t h = 0, byte0 = 0;
      bool ins = false;
      if (lane < W) {
        const uint64_t v8 = load8(a.wu, uo + p);
        byte0 = (uint32_t)v8 & 255u;
        if (p + D::kMinMatch <= n) {
          ins = true;
          h = D::hash4((uint32_t)v8);
          const int c = (int)tab[h] - 1;
          if (c >= 0 && p - c <= D::kMaxDist) {
            const int ml = n - p < D::kMaxMatch ? n - p : D::kMaxMatch;
            int l = 0;
            while (l < ml) {
              const uint64_t x = load8(a.wu, uo + p + l) ^ load8(a.wu, uo + c + l);
              if (x) {
                l += __builtin_ctzll(x) >> 3;
                break;
              }
              l += 8;
            }
            l = l < ml ? l : ml;
            if (l >= D::kMinMatch) len = l, dist = p - c;
          }
        }
      }
      __syncthreads();  // every lane's lookup is ahead of the row's inserts
      if (ins) atomicMax(&tab[h], (uint32_t)(p + 1));
      // greedy selection in position order: literals up to the next lane with a match, then past that match
      const uint64_t mb = __ballot(len > 0);
      uint64_t tok = 0;
      int l = 0;
      while (l < W) {
        const uint64_t m = mb & (~0ull << l);
        if (!m) {
          tok |= ~0ull << l;
          break;
        }
        const int j = __builtin_ctzll(m);
        tok |= (~0ull << l) & ((2ull << j) - 1ull);
        l = j + __builtin_amdgcn_readlane(len, __builtin_amdgcn_readfirstlane(j));
      }
      const bool is_tok = lane < W && ((tok >> lane) & 1ull);
      int nbits = 0;
      uint32_t bits = 0;
      if (is_tok) {
        nbits = len ? D::bits_match(len, dist) : D::bits_literal(byte0);
        bits = (len ? D::encode_match(len, dist) : D::encode_literal(byte0)).bits;
      }
      const int incl = wave_incl_scan(nbits);
      const int total = carry + __builtin_amdgcn_readlane(incl, 63);
      if (nbits) {
        const int o = carry + incl - nbits, w = o >> 5, s = o & 31;
        atomicOr(&stage[w], bits << s);
        if (s + nbits > 32) atomicOr(&stage[w + 1], bits >> (32 - s));
      }
      __syncthreads();
      const int full = total >> 5;  // <= 62
      if ((wbase + full) * 4 > limit) {  // wave-uniform: the Huffman form has passed the stored size
        stored = true;
        break;
      }
      const uint32_t mine = stage[lane], keep = stage[full];
      if (lane < full) out[wbase + lane] = mine;
      __syncthreads();
      stage[lane] = lane == 0 ? keep : 0u;
      __syncthreads();
      wbase += full;
      carry = total & 31;
      pos += l > W ? l : W;
    }
    // the end-of-block code is seven zero bits: the stage already holds them
    const int bytes = (int)(((int64_t)wbase * 32 + carry + D::kEobBits + 7) >> 3);
    if (!stored && bytes > limit) stored = true;
    if (!stored) {
      const int words = (carry + D::kEobBits + 31) >> 5;  // 1 or 2; the slot has room for two past the limit
      if (lane < words) out[wbase + lane] = stage[lane];
    }
    if (lane == 0) {
      const int pay = stored ? limit : bytes;
      a.pay[a.b0 + k] = pay;
      a.stored[a.b0 + k] = stored ? 1 : 0;
      a.tsz[k] = 26 + pay;
    }
  }
}

// ---- level 1 | SBAM_WRITE_DYNAMIC: the same tokens, then per block the smallest of stored, fixed and dynamic --------
// A token record holds 16-bit entries, each one code plus its extra bits in the output (at most kMaxHalfTokenBits):
constexpr uint32_t kTokLength = 0x100;    // | length - 3: the first half of a match; its distance follows
constexpr uint32_t kTokEob = 0x200;       // the record's last entry
constexpr uint32_t kTokDistance = 0x8000; // | distance - 1
                                          // (below 0x100: a literal)
// the stage holds the header in one piece, and a carry with a row of 64 entries
constexpr int kDynStageWords = 160;
static_assert(kDynStageWords * 32 >= 31 + D::kMaxHeaderBits + 1, "the dynamic header does not fit the stage");
static_assert(kDynStageWords * 32 >= 31 + 64 * D::kMaxHalfTokenBits + 31, "a row of tokens does not fit the stage");
static_assert(D::kMaxHalfTokenBits <= 32, "a token half is ORed into at most two words");
constexpr int kCodeSymbols = D::kLitSymbols + D::kDistSymbols;
constexpr int kSortWork = 320;  // words of the table's space for the sorted keys; the builder's work space follows
static_assert(kSortWork >= D::kLitSymbols && 2 * kSortWork + 16 <= kTabEntries, "the code builder works in the table");

// sort_keys of sbam_deflate_core.h by the wave: every symbol of the code finds its rank among the (distinct) keys
SB_DEV int wave_sort_keys(const uint32_t *count, int n, uint32_t *keys, int lane) {
  int mine = 0;
  for (int s = lane; s < n; s += 64) mine += count[s] > 0;
  const int used = wave_sum(mine);
  const uint32_t c0 = count[0];
  mine = 0;
  for (int s = lane; s < n; s += 64) {
    const uint32_t cs = count[s];
    if (!D::in_code(cs, s, used, c0)) continue;
    const uint32_t k = D::sort_key(cs, s);
    int rank = 0;
    for (int t = 0; t < n; t++) rank += D::in_code(count[t], t, used, c0) && D::sort_key(count[t], t) < k;
    keys[rank] = k;
    mine++;
  }
  return wave_sum(mine);
}

// the stage's full words go to the slot, the partial word moves to the front; every lane's ORs are behind a barrier
SB_DEV void stage_flush(uint32_t *stage, uint32_t *__restrict__ out, int &wbase, int &carry, int total, int lane) {
  const int full = total >> 5;  // < kDynStageWords
  for (int i = lane; i < full; i += 64) out[wbase + i] = stage[i];
  const uint32_t keep = stage[full];
  __syncthreads();
  for (int i = lane; i <= full; i += 64) stage[i] = i == 0 ? keep : 0u;
  __syncthreads();
  wbase += full;
  carry = total & 31;
}

struct StageSink {  // lane 0 alone appends the header
  uint32_t *stage;
  int nbits;
  SB_DEV void put(uint32_t v, int n) {
    if (n == 0) return;
    const int w = nbits >> 5, s = nbits & 31;
    stage[w] |= v << s;
    if (s + n > 32) stage[w + 1] |= v >> (32 - s);
    nbits += n;
  }
};

__global__ void __launch_bounds__(64) k_deflate_dynamic(WriteBlocksArgs a) {
  __shared__ uint32_t tab[kTabEntries];  // as k_deflate_fixed's; after the token pass the code builder's work space
  __shared__ uint32_t stage[kDynStageWords];
  __shared__ uint32_t count[kCodeSymbols];  // literal/length symbols, then distance codes
  __shared__ D::Code code[kCodeSymbols];
  __shared__ uint8_t clen[kCodeSymbols + 4];
  __shared__ D::HeaderPlan plan;
  const int lane = threadIdx.x;
  uint16_t *tok = reinterpret_cast<uint16_t *>(a.tokens + (int64_t)blockIdx.x * a.token_stride);
  uint32_t *const lit_count = count, *const dist_count = count + D::kLitSymbols;
  uint8_t *const lit_len = clen, *const dist_len = clen + D::kLitSymbols;
  for (int64_t k = blockIdx.x; k < a.nb; k += gridDim.x) {
    int64_t uo;
    const int n = block_len(a, a.b0 + k, &uo);
    uint32_t *__restrict__ out = reinterpret_cast<uint32_t *>(a.slots + k * a.slot_stride);
    __syncthreads();  // (the previous block's last reads)
    for (int i = lane; i < kTabEntries; i += 64) tab[i] = 0;
    for (int i = lane; i < kDynStageWords; i += 64) stage[i] = 0;
    for (int i = lane; i < kCodeSymbols; i += 64) count[i] = i == D::kEobSymbol ? 1u : 0u;
    __syncthreads();
    // 1. tokens: k_deflate_fixed's row walk and match search; the row's tokens go to the record and the histograms
    int ntok = 0, pos = 0;
    while (pos < n) {
      const int W = n - pos < 64 ? n - pos : 64;
      const int p = pos + lane;
      int len = 0, dist = 0;
      uint32_t h = 0, byte0 = 0;
      bool ins = false;
      if (lane < W) {
        const uint64_t v8 = load8(a.wu, uo + p);
        byte0 = (uint32_t)v8 & 255u;
        if (p + D::kMinMatch <= n) {
          ins = true;
          h = D::hash4((uint32_t)v8);
          const int c = (int)tab[h] - 1;
          if (c >= 0 && p - c <= D::kMaxDist) {
            const int ml = n - p < D::kMaxMatch ? n - p : D::kMaxMatch;
            int l = 0;
            while (l < ml) {
              const uint64_t x = load8(a.wu, uo + p + l) ^ load8(a.wu, uo + c + l);
              if (x) {
                l += __builtin_ctzll(x) >> 3;
                break;
              }
              l += 8;
            }
            l = l < ml ? l : ml;
            if (l >= D::kMinMatch) len = l, dist = p - c;
          }
        }
      }
      __syncthreads();  // every lane's lookup is ahead of the row's inserts
      if (ins) atomicMax(&tab[h], (uint32_t)(p + 1));
      const uint64_t mb = __ballot(len > 0);
      uint64_t sel = 0;
      int l = 0;
      while (l < W) {
        const uint64_t m = mb & (~0ull << l);
        if (!m) {
          sel |= ~0ull << l;
          break;
        }
        const int j = __builtin_ctzll(m);
        sel |= (~0ull << l) & ((2ull << j) - 1ull);
        l = j + __builtin_amdgcn_readlane(len, __builtin_amdgcn_readfirstlane(j));
      }
      const bool is_tok = lane < W && ((sel >> lane) & 1ull);
      const int slots = is_tok ? (len ? 2 : 1) : 0;
      const int incl = wave_incl_scan(slots);
      if (is_tok) {
        const int o = ntok + incl - slots;  // < n: a literal covers one byte, a match's two entries at least four
        if (len) {
          int ls, le, dc, de;
          uint32_t x;
          D::length_code(len, &ls, &le, &x);
          D::distance_code(dist, &dc, &de, &x);
          tok[o] = (uint16_t)(kTokLength | (uint32_t)(len - 3));
          tok[o + 1] = (uint16_t)(kTokDistance | (uint32_t)(dist - 1));
          atomicAdd(&lit_count[ls], 1u);
          atomicAdd(&dist_count[dc], 1u);
        } else {
          tok[o] = (uint16_t)byte0;
          atomicAdd(&lit_count[byte0], 1u);
        }
      }
      ntok += __builtin_amdgcn_readlane(incl, 63);
      pos += l > W ? l : W;
      __syncthreads();  // the row's inserts are ahead of the next row's lookups
    }
    if (lane == 0) tok[ntok] = (uint16_t)kTokEob;
    ntok++;
    // 2. codes: the core's builder on the histograms, the sort by the wave, the rest by lane 0
    uint32_t *keys = tab, *work = tab + kSortWork;
    int m = wave_sort_keys(lit_count, D::kLitSymbols, keys, lane);
    __syncthreads();
    if (lane == 0) {
      D::lengths_from_sorted(keys, m, D::kLitSymbols, D::kMaxCodeBits, lit_len, work);
      D::assign_codes(lit_len, D::kLitSymbols, code, work);
    }
    __syncthreads();
    m = wave_sort_keys(dist_count, D::kDistSymbols, keys, lane);
    __syncthreads();
    if (lane == 0) {
      D::lengths_from_sorted(keys, m, D::kDistSymbols, D::kMaxCodeBits, dist_len, work);
      D::assign_codes(dist_len, D::kDistSymbols, code + D::kLitSymbols, work);
      D::header_plan(lit_len, dist_len, &plan, keys, work);
    }
    __syncthreads();
    // 3. choice, from the histograms alone
    const int64_t fixed_body = wave_sum(D::body_bits(lit_count, dist_count, nullptr, nullptr, lane, 64));
    const int64_t dyn_body = wave_sum(D::body_bits(lit_count, dist_count, lit_len, dist_len, lane, 64));
    int bytes;
    int form = D::choose_form(n, fixed_body, plan.bits, dyn_body, &bytes);  // (wave-uniform)
    // 4. emit: the header, then the record in rows of 64 entries through the codes in LDS
    int carry = 0, wbase = 0;
    if (form == 1) {  // the fixed code takes the dynamic one's place in the tables
      __syncthreads();
      for (int s = lane; s < kCodeSymbols; s += 64)
        code[s] = s < D::kLitSymbols ? D::fixed_lit_code(s) : D::fixed_dist_code(s - D::kLitSymbols);
      if (lane == 0) stage[0] = D::kHeaderValue;
      carry = D::kHeaderBits;
      __syncthreads();
    } else if (form == 2) {
      if (lane == 0) {
        StageSink sink{stage, 0};
        D::write_header(&plan, lit_len, dist_len, sink);
      }
      __syncthreads();
      stage_flush(stage, out, wbase, carry, plan.bits, lane);
    }
    for (int base = 0; form != 0 && base < ntok; base += 64) {
      int nbits = 0;
      uint32_t bits = 0;
      if (base + lane < ntok) {
        const uint32_t t = tok[base + lane];
        const D::Token e = t & kTokDistance ? D::dyn_distance(code + D::kLitSymbols, (int)(t & 0x7fffu) + 1)
                           : t & kTokLength ? D::dyn_length(code, (int)(t & 255u) + 3)
                                            : D::dyn_symbol(code, t == kTokEob ? D::kEobSymbol : (int)t);
        bits = e.bits;
        nbits = e.n;
      }
      const int incl = wave_incl_scan(nbits);
      const int total = carry + __builtin_amdgcn_readlane(incl, 63);
      if (nbits) {
        const int o = carry + incl - nbits, w = o >> 5, s = o & 31;
        atomicOr(&stage[w], bits << s);
        if (s + nbits > 32) atomicOr(&stage[w + 1], bits >> (32 - s));
      }
      __syncthreads();
      // The record's entries are the histograms' counts, taken in the same branch of the token pass, so the bits
      // written are the bits priced, `bytes` <= n + 4, and the last word ends inside the slot's n + 13.  An
      // invariant check, not a path any input takes: were the two ever to disagree, the block is stored instead,
      // and nothing goes past the slot.
      if (((int64_t)wbase * 32 + total + 7) >> 3 > bytes) {
        form = 0;
        bytes = n + D::kStoredHeader;
        break;
      }
      stage_flush(stage, out, wbase, carry, total, lane);
    }
    if (form != 0 && lane == 0 && carry) out[wbase] = stage[0];
    if (lane == 0) {
      a.pay[a.b0 + k] = bytes;
      a.stored[a.b0 + k] = form == 0 ? 1 : 0;
      a.tsz[k] = 26 + bytes;
    }
  }
}

// n bytes from sbase + so (sbase 4-byte aligned, readable 12 bytes past the source) to dst, by one wave: the head up
// to dst's 8-byte boundary and the tail by bytes, the body by 8-byte stores
SB_DEV void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ sbase, int64_t so, int n, int lane) {
  int head = (int)((8 - (reinterpret_cast<uintptr_t>(dst) & 7)) & 7);
  head = head < n ? head : n;
  if (lane < head) dst[lane] = sbase[so + lane];
  const int body = (n - head) >> 3;
  for (int i = lane; i < body; i += 64)
    *reinterpret_cast<uint64_t *>(dst + head + 8 * i) = load8(sbase, so + head + 8 * i);
  const int done = head + 8 * body;
  if (lane < n - done) dst[done + lane] = sbase[so + done + lane];
}

// byte i of the 28-byte BGZF EOF block; bytes 0..15 are also every block's header in front of BSIZE
SB_DEV uint8_t eof_byte(int i) {
  const uint64_t w = i < 8 ? 0x0000000004088b1full : i < 16 ? 0x000243420006ff00ull : i < 24 ? 0x000000000003001bull : 0ull;
  return (uint8_t)(w >> (8 * (i & 7)));
}

__global__ void __launch_bounds__(64 * kFrameWaves) k_frame(WriteBlocksArgs a, WriteFrameArgs f) {
  __shared__ uint32_t tab[sbam_crc::kTabWords];
  for (uint32_t i = threadIdx.x; i < (uint32_t)sbam_crc::kTabWords; i += blockDim.x) tab[i] = sbam_crc::table_word(i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t g = (int64_t)blockIdx.x * kFrameWaves; g <= a.nb; g += (int64_t)gridDim.x * kFrameWaves) {
    const int64_t k = g + wave;
    if (k > a.nb) continue;
    uint8_t *__restrict__ dst = f.file + f.base + a.tsz[k];
    if (k == a.nb) {  // behind the batch's last block
      if (f.with_eof && lane < 28) dst[lane] = eof_byte(lane);
      if (lane == 0) f.start[a.b0 + k] = f.base + a.tsz[k];
      continue;
    }
    const int64_t b = a.b0 + k;
    int64_t uo;
    const int n = block_len(a, b, &uo);
    const int pay = __builtin_amdgcn_readfirstlane(a.pay[b]);
    const bool stored = __builtin_amdgcn_readfirstlane(a.stored[b]) != 0;
    const int total = 26 + pay;
    uint32_t terms = sbam_crc::lane_term(tab, a.wu, uo, n, lane);
    for (int o = 32; o > 0; o >>= 1) terms ^= __shfl_xor(terms, o, 64);
    const uint32_t crc = sbam_crc::finish(tab, terms, n);
    if (lane < 16) dst[lane] = eof_byte(lane);
    if (lane == 16) dst[16] = (uint8_t)((total - 1) & 255);
    if (lane == 17) dst[17] = (uint8_t)((total - 1) >> 8);
    if (stored) {
      uint8_t sh[D::kStoredHeader];
      D::stored_header((uint32_t)n, sh);
#pragma unroll
      for (int i = 0; i < D::kStoredHeader; i++)
        if (lane == i) dst[18 + i] = sh[i];
      wave_copy(dst + 18 + D::kStoredHeader, a.wu, uo, n, lane);
    } else {
      wave_copy(dst + 18, a.slots, k * a.slot_stride, pay, lane);
    }
    if (lane < 4) dst[18 + pay + lane] = (uint8_t)(crc >> (8 * lane));
    else if (lane < 8) dst[18 + pay + lane] = (uint8_t)((uint32_t)n >> (8 * (lane - 4)));
    if (lane == 0) {
      f.start[b] = f.base + a.tsz[k];
      f.csize[b] = total;
      f.usize[b] = n;
      if (stored) atomicAdd(f.n_stored, 1ull);
    }
  }
}

}  // namespace

int64_t write_slot_stride(int32_t block_bytes) {
  return ((int64_t)block_bytes + D::kStoredHeader + 8 + 15) & ~(int64_t)15;
}

// 16-bit entries: at most one per byte (a literal one, a match of four bytes or more two) and the end of block
int64_t write_token_stride(int32_t block_bytes) { return (2 * ((int64_t)block_bytes + 1) + 15) & ~(int64_t)15; }
// k_deflate_dynamic's grid: 4 waves per CU (36 KiB of LDS each) x 256 CUs resident, every one with a record of its own
int64_t write_token_records(int64_t blocks) { return blocks < 1024 ? blocks : 1024; }

hipError_t launch_write_select(const WriteSelectArgs &a, hipStream_t s) {
  const int64_t grid = (a.n + 1 + kSelectThreads - 1) / kSelectThreads;
  hipLaunchKernelGGL(k_write_select, dim3((unsigned)grid), dim3(kSelectThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_written_records(const int64_t *off, const int64_t *ord, int64_t n, int32_t block_bytes,
                                  const int64_t *start, int64_t *block_pos, int32_t *block_off, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t grid = (n + kSelectThreads - 1) / kSelectThreads;
  hipLaunchKernelGGL(k_written_records, dim3((unsigned)grid), dim3(kSelectThreads), 0, s, off, ord, n, block_bytes,
                     start, block_pos, block_off);
  return hipGetLastError();
}

hipError_t launch_write_deflate(const WriteBlocksArgs &a, int32_t level, hipStream_t s) {
  if (a.nb <= 0) return hipSuccess;
  if (level == 0) {
    const int64_t grid = (a.nb + kSelectThreads - 1) / kSelectThreads;
    hipLaunchKernelGGL(k_stored_sizes, dim3((unsigned)grid), dim3(kSelectThreads), 0, s, a);
  } else if (level & kWriteDynamic) {
    const int64_t grid = write_token_records(a.nb);  // one token record per workgroup
    hipLaunchKernelGGL(k_deflate_dynamic, dim3((unsigned)grid), dim3(64), 0, s, a);
  } else {
    const int64_t grid = a.nb < 4096 ? a.nb : 4096;  // 4 waves per CU x 256 CUs resident, and the same again queued
    hipLaunchKernelGGL(k_deflate_fixed, dim3((unsigned)grid), dim3(64), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_write_frame(const WriteBlocksArgs &a, const WriteFrameArgs &f, hipStream_t s) {
  const int64_t groups = (a.nb + 1 + kFrameWaves - 1) / kFrameWaves;
  const int grid = (int)(groups < 1024 ? groups : 1024);
  hipLaunchKernelGGL(k_frame, dim3(grid), dim3(64 * kFrameWaves), 0, s, a, f);
  return hipGetLastError();
}

}  // namespace sbam
