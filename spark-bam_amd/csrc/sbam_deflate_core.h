// sbam_deflate_core.h — what the BAM writer's DEFLATE encoder (sbam_write.hip) knows without a GPU, host- and
// device-callable, so that a plain C++ program can emit streams from the same tables and hand them to zlib
// (tests/test_deflate_host.py).
//
// RFC 1951.  A block is stored (BTYPE = 00: five header bytes, then the bytes), one fixed-Huffman block (BTYPE = 01,
// BFINAL = 1) or one dynamic-Huffman block (BTYPE = 10: the second half of this file, tests/test_deflate_dynamic_host.py).
// The fixed code:
//   literal 0..143      8 bits  00110000 + v          literal 144..255    9 bits  110010000 + (v - 144)
//   symbol 256..279     7 bits  0000000 + (s - 256)   symbol 280..287     8 bits  11000000 + (s - 280)
//   distance code       5 bits, the code's number
// Huffman codes enter the stream from their most significant bit, everything else (header bits, extra bits) from the
// least significant: a token is assembled here as one little-endian bit string of at most 31 bits, the Huffman codes
// bit-reversed, so that a writer only shifts it to the stream's bit position and ORs it in.
//   literal v                   code(v)
//   match (length, distance)    code(length symbol) | length extra | code(distance symbol) | distance extra
// bits_literal / bits_match give a token's length without building it: the one function that both the pass that
// places tokens (a prefix sum of these lengths) and the pass that writes them rely on.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBAM_DEFL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBAM_DEFL_HD inline
#endif

namespace sbam_deflate {

constexpr int kMinMatch = 4;           // the hash covers four bytes; RFC 1951 would allow 3
constexpr int kMaxMatch = 258;
constexpr int kMaxDist = 32768;
constexpr int kMaxBlockBytes = 65498;  // htsjdk's BlockCompressedStreamConstants.DEFAULT_UNCOMPRESSED_BLOCK_SIZE
constexpr int kStoredHeader = 5;       // BFINAL | BTYPE, LEN, NLEN
constexpr int kHashBits = 13;
constexpr int kHeaderBits = 3;         // BFINAL = 1, BTYPE = 01
constexpr uint32_t kHeaderValue = 3u;  // (bit 0: BFINAL, bits 1-2: BTYPE, least significant first)
constexpr int kEobBits = 7;            // symbol 256: seven zero bits

struct Token {
  uint32_t bits;  // little-endian bit string
  int n;          // its length, <= 31
};

// floor(log2(v)), v > 0
SBAM_DEFL_HD int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }

// the low n bits of v in reverse order
SBAM_DEFL_HD uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// length 3..258 -> symbol 257..285, its extra-bit count and value (RFC 1951 §3.2.5)
SBAM_DEFL_HD void length_code(int len, int *sym, int *ebits, uint32_t *extra) {
  const uint32_t l = (uint32_t)(len - 3);
  if (len == kMaxMatch) {
    *sym = 285, *ebits = 0, *extra = 0;
  } else if (l < 8) {
    *sym = 257 + (int)l, *ebits = 0, *extra = 0;
  } else {
    const int e = ilog2(l) - 2;
    *sym = 261 + 4 * e + (int)((l >> e) & 3u);
    *ebits = e;
    *extra = l & ((1u << e) - 1u);
  }
}

// distance 1..32768 -> code 0..29, its extra-bit count and value
SBAM_DEFL_HD void distance_code(int dist, int *code, int *ebits, uint32_t *extra) {
  const uint32_t d = (uint32_t)(dist - 1);
  if (d < 4) {
    *code = (int)d, *ebits = 0, *extra = 0;
  } else {
    const int e = ilog2(d) - 1;
    *code = 2 * e + 2 + (int)((d >> e) & 1u);
    *ebits = e;
    *extra = d & ((1u << e) - 1u);
  }
}

// the fixed code of literal/length symbol 0..287, bit-reversed
SBAM_DEFL_HD Token fixed_symbol(int sym) {
  if (sym < 144) return Token{reverse_bits(0x30u + (uint32_t)sym, 8), 8};
  if (sym < 256) return Token{reverse_bits(0x190u + (uint32_t)(sym - 144), 9), 9};
  if (sym < 280) return Token{reverse_bits((uint32_t)(sym - 256), 7), 7};
  return Token{reverse_bits(0xC0u + (uint32_t)(sym - 280), 8), 8};
}

// bits of this token
SBAM_DEFL_HD int bits_literal(uint32_t v) { return v < 144 ? 8 : 9; }
SBAM_DEFL_HD int bits_match(int len, int dist) {
  int ls, le, dc, de;
  uint32_t x;
  length_code(len, &ls, &le, &x);
  distance_code(dist, &dc, &de, &x);
  return (ls < 280 ? 7 : 8) + le + 5 + de;
}

SBAM_DEFL_HD Token encode_literal(uint32_t v) { return fixed_symbol((int)v); }
SBAM_DEFL_HD Token encode_match(int len, int dist) {
  int ls, le, dc, de;
  uint32_t lx, dx;
  length_code(len, &ls, &le, &lx);
  distance_code(dist, &dc, &de, &dx);
  Token t = fixed_symbol(ls);
  t.bits |= lx << t.n;
  t.n += le;
  t.bits |= reverse_bits((uint32_t)dc, 5) << t.n;
  t.n += 5;
  t.bits |= dx << t.n;
  t.n += de;
  return t;
}

// the five bytes in front of a stored block of n bytes (n <= 65535), BFINAL = 1
SBAM_DEFL_HD void stored_header(uint32_t n, uint8_t out[kStoredHeader]) {
  out[0] = 1;
  out[1] = (uint8_t)(n & 255u);
  out[2] = (uint8_t)(n >> 8);
  out[3] = (uint8_t)(~n & 255u);
  out[4] = (uint8_t)((~n >> 8) & 255u);
}

// bucket of the four bytes v (little-endian) in a table of 1 << kHashBits entries
SBAM_DEFL_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// payload bytes of a block whose tokens take `token_bits` bits in the fixed-Huffman form
SBAM_DEFL_HD int64_t fixed_bytes(int64_t token_bits) { return (kHeaderBits + token_bits + kEobBits + 7) >> 3; }

// ---- dynamic Huffman blocks (BTYPE = 10) -------------------------------------------------------------------------
// A block's tokens are counted into two histograms (literal/length symbols 0..285, symbol 256 once; distance codes
// 0..29).  From them, in this order and before a bit is written:
//   build_lengths     length-limited code lengths (15 bits for the two alphabets, 7 for the code-length alphabet)
//   assign_codes      the canonical codes of RFC 1951 §3.2.2, bit-reversed, next to their lengths
//   header_plan       HLIT, HDIST, the run-length pass over the two length arrays, the code-length code, HCLEN and
//                     the header's bit count
//   body_bits         bits of the tokens (end of block included) under a set of lengths: the dynamic ones, or
//                     fixed_lit_length / kFixedDistBits for the fixed form
//   choose_form       the smallest of stored, fixed and dynamic, ties to the earlier
// and write_header emits the header through any sink with put(value, bits), by the same run-length pass.
// Everything is deterministic: ties between equal counts are broken by symbol number.
constexpr int kLitSymbols = 286;
constexpr int kDistSymbols = 30;
constexpr int kClSymbols = 19;
constexpr int kMaxCodeBits = 15;
constexpr int kMaxClBits = 7;
constexpr int kEobSymbol = 256;
constexpr int kFixedDistBits = 5;
constexpr int kKeySymBits = 9;  // sort key: count << 9 | symbol
// the longest dynamic header: 3 + 5 + 5 + 4, 19 x 3, and 316 lengths of 7 code bits + 7 extra bits at the most
constexpr int kMaxHeaderBits = 17 + 3 * kClSymbols + (kLitSymbols + kDistSymbols) * (kMaxClBits + 7);
// the longest token half of a dynamic block: a distance code and its extra bits (a length code takes 15 + 5)
constexpr int kMaxHalfTokenBits = kMaxCodeBits + 13;

struct Code {
  uint16_t bits;  // the code, bit-reversed: its first bit in the stream is bit 0
  uint16_t n;     // its length; 0: the symbol has no code
};

SBAM_DEFL_HD int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
SBAM_DEFL_HD int distance_extra_bits(int code) { return code < 4 ? 0 : (code - 2) >> 1; }
SBAM_DEFL_HD int fixed_lit_length(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
SBAM_DEFL_HD int cl_extra_bits(int sym) { return sym < 16 ? 0 : sym == 16 ? 2 : sym == 17 ? 3 : 7; }
// the code-length symbol whose length is the header's i-th (RFC 1951 §3.2.7):
// 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
SBAM_DEFL_HD int cl_order(int i) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                          6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// A symbol belongs to the code when it was counted, or when fewer than two were (`used` < 2) and it is one of the
// lowest-numbered uncounted ones that make up the pair: 0, and 1 when 0 was the counted one or none was.
SBAM_DEFL_HD bool in_code(uint32_t count, int sym, int used, uint32_t count0) {
  return count > 0 || (used < 2 && (sym == 0 || (sym == 1 && (used == 0 || count0 > 0))));
}
SBAM_DEFL_HD uint32_t sort_key(uint32_t count, int sym) { return (count << kKeySymBits) | (uint32_t)sym; }

// keys[0, m) = the sort keys of the code's symbols in ascending order (count, then symbol); returns m >= 2.
// (Keys are distinct, so any sort gives this order: the kernel ranks them in parallel.)
SBAM_DEFL_HD int sort_keys(const uint32_t *count, int n, uint32_t *keys) {
  int used = 0, m = 0;
  for (int s = 0; s < n; s++) used += count[s] > 0;
  for (int s = 0; s < n; s++) {
    if (!in_code(count[s], s, used, count[0])) continue;
    const uint32_t k = sort_key(count[s], s);
    int i = m++;
    for (; i > 0 && keys[i - 1] > k; i--) keys[i] = keys[i - 1];
    keys[i] = k;
  }
  return m;
}

// Code lengths of the m >= 2 symbols in keys (ascending) into len[0, n); every other symbol gets 0.  work: m + 16
// words.  Depths of a Huffman tree over the sorted counts, in place (Moffat and Katajainen; between equal weights a
// leaf goes before a merged node, which gives the shallowest of the optimal trees); depths past `limit` are cut to
// it and the Kraft sum is brought back to 1 one unit of 2^-limit at a time: a code of the limit's length leaves, the
// longest shorter code takes a second code beside it one bit down; the lengths then go to the symbols in sorted
// order, longest to rarest.  A tree within the limit is left as it is, so its cost is the Huffman cost.
SBAM_DEFL_HD void lengths_from_sorted(const uint32_t *keys, int m, int n, int limit, uint8_t *len, uint32_t *work) {
  uint32_t *A = work, *bl = work + m;
  for (int s = 0; s < n; s++) len[s] = 0;
  for (int i = 0; i < m; i++) A[i] = keys[i] >> kKeySymBits;
  for (int d = 0; d <= limit; d++) bl[d] = 0;
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < m - 1; next++) {
    if (leaf >= m || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= m || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  A[m - 2] = 0;
  for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
  int avbl = 1, used = 0, dpth = 0;
  root = m - 2;
  while (avbl > 0) {  // the nodes of this depth that are not internal are leaves: counted, not stored
    while (root >= 0 && (int)A[root] == dpth) used++, root--;
    for (; avbl > used; avbl--) bl[dpth < limit ? dpth : limit]++;
    avbl = 2 * used;
    dpth++;
    used = 0;
  }
  uint32_t kraft = 0;  // in units of 2^-limit
  for (int d = 1; d <= limit; d++) kraft += bl[d] << (limit - d);
  while (kraft > (1u << limit)) {
    bl[limit]--;
    for (int d = limit - 1; d > 0; d--)
      if (bl[d]) {
        bl[d]--;
        bl[d + 1] += 2;
        break;
      }
    kraft--;
  }
  int i = 0;
  for (int d = limit; d > 0; d--)
    for (uint32_t c = bl[d]; c > 0; c--) len[keys[i++] & ((1u << kKeySymBits) - 1u)] = (uint8_t)d;
}

// count[0, n) -> len[0, n), at most `limit` bits, Kraft sum 1.  keys: n words; work: n + 16 words.
SBAM_DEFL_HD void build_lengths(const uint32_t *count, int n, int limit, uint8_t *len, uint32_t *keys, uint32_t *work) {
  const int m = sort_keys(count, n, keys);
  lengths_from_sorted(keys, m, n, limit, len, work);
}

// canonical codes from lengths (RFC 1951 §3.2.2), bit-reversed as fixed_symbol's.  next: kMaxCodeBits + 2 words.
SBAM_DEFL_HD void assign_codes(const uint8_t *len, int n, Code *code, uint32_t *next) {
  for (int d = 0; d <= kMaxCodeBits + 1; d++) next[d] = 0;
  for (int s = 0; s < n; s++) next[len[s] + 1]++;
  next[1] = 0;  // (symbols without a code)
  for (int d = 2; d <= kMaxCodeBits; d++) next[d] = (next[d - 1] << 1) + (next[d] << 1);
  for (int s = 0; s < n; s++) {
    const int l = len[s];
    code[s] = Code{(uint16_t)(l ? reverse_bits(next[l]++, l) : 0u), (uint16_t)l};
  }
}

// The run-length pass over the header's length sequence, lit[0, nlit) then dist[0, ndist) as one: emit(symbol,
// extra bits, extra value) per code-length symbol.  A run of zeros goes out as 18s (11..138), then a 17 (3..10),
// then single zeros; a run of a nonzero length as the length itself, then 16s (3..6 repeats), then the rest singly.
template <class Emit>
SBAM_DEFL_HD void rle_pass(const uint8_t *lit, int nlit, const uint8_t *dist, int ndist, Emit &&emit) {
  const int total = nlit + ndist;
  int i = 0;
  while (i < total) {
    const int v = i < nlit ? lit[i] : dist[i - nlit];
    int run = 1;
    while (i + run < total && (i + run < nlit ? lit[i + run] : dist[i + run - nlit]) == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        emit(18, 7, (uint32_t)(r - 11));
        run -= r;
      }
      if (run >= 3) {
        emit(17, 3, (uint32_t)(run - 3));
        run = 0;
      }
    } else {
      emit(v, 0, 0u);
      run--;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        emit(16, 2, (uint32_t)(r - 3));
        run -= r;
      }
    }
    for (; run > 0; run--) emit(v, 0, 0u);
  }
}

struct HeaderPlan {
  int hlit, hdist, hclen;  // counts of lengths sent: 257..286, 1..30, 4..19
  int bits;                // of the whole header, BFINAL and BTYPE included
  uint32_t cl_count[kClSymbols];
  uint8_t cl_len[kClSymbols];
  Code cl_code[kClSymbols];
};

// Everything about the header that follows from the two length arrays.  keys: kClSymbols words; work: kClSymbols + 16.
SBAM_DEFL_HD void header_plan(const uint8_t *lit_len, const uint8_t *dist_len, HeaderPlan *p, uint32_t *keys,
                              uint32_t *work) {
  int hlit = kLitSymbols, hdist = kDistSymbols;
  while (hlit > 257 && lit_len[hlit - 1] == 0) hlit--;
  while (hdist > 1 && dist_len[hdist - 1] == 0) hdist--;
  p->hlit = hlit;
  p->hdist = hdist;
  uint32_t *cnt = p->cl_count;
  for (int s = 0; s < kClSymbols; s++) cnt[s] = 0;
  rle_pass(lit_len, hlit, dist_len, hdist, [cnt](int sym, int, uint32_t) { cnt[sym]++; });
  build_lengths(cnt, kClSymbols, kMaxClBits, p->cl_len, keys, work);
  assign_codes(p->cl_len, kClSymbols, p->cl_code, work);
  int hclen = kClSymbols;
  while (hclen > 4 && p->cl_len[cl_order(hclen - 1)] == 0) hclen--;
  p->hclen = hclen;
  int bits = 3 + 5 + 5 + 4 + 3 * hclen;
  for (int s = 0; s < kClSymbols; s++) bits += (int)cnt[s] * (p->cl_len[s] + cl_extra_bits(s));
  p->bits = bits;
}

// The header through sink.put(value, bits): values enter the stream from their least significant bit.
template <class Sink>
SBAM_DEFL_HD void write_header(const HeaderPlan *p, const uint8_t *lit_len, const uint8_t *dist_len, Sink &sink) {
  sink.put(1u | 2u << 1, 3);  // BFINAL = 1, BTYPE = 10
  sink.put((uint32_t)(p->hlit - 257), 5);
  sink.put((uint32_t)(p->hdist - 1), 5);
  sink.put((uint32_t)(p->hclen - 4), 4);
  for (int i = 0; i < p->hclen; i++) sink.put(p->cl_len[cl_order(i)], 3);
  const Code *cc = p->cl_code;
  rle_pass(lit_len, p->hlit, dist_len, p->hdist, [cc, &sink](int sym, int eb, uint32_t extra) {
    sink.put(cc[sym].bits, cc[sym].n);
    if (eb) sink.put(extra, eb);
  });
}

// Bits of a block's tokens, end of block included, under the lengths lit_len / dist_len, or under the fixed code when
// lit_len is null; over the symbols first, first + step, ... (0, 1: all of them; a wave sums lane, 64 and adds up).
SBAM_DEFL_HD int64_t body_bits(const uint32_t *lit_count, const uint32_t *dist_count, const uint8_t *lit_len,
                               const uint8_t *dist_len, int first, int step) {
  int64_t bits = 0;
  for (int s = first; s < kLitSymbols; s += step)
    bits += (int64_t)lit_count[s] * ((lit_len ? lit_len[s] : fixed_lit_length(s)) + length_extra_bits(s));
  for (int c = first; c < kDistSymbols; c += step)
    bits += (int64_t)dist_count[c] * ((lit_len ? dist_len[c] : kFixedDistBits) + distance_extra_bits(c));
  return bits;
}

// The block's form, 0 stored, 1 fixed, 2 dynamic, and its payload bytes: the smallest, ties to the earlier.
// fixed_body / dyn_body: body_bits (the end-of-block code is in them); dyn_header: HeaderPlan::bits.
SBAM_DEFL_HD int choose_form(int n, int64_t fixed_body, int64_t dyn_header, int64_t dyn_body, int *bytes) {
  const int64_t st = n + kStoredHeader, fx = (kHeaderBits + fixed_body + 7) >> 3, dy = (dyn_header + dyn_body + 7) >> 3;
  const int form = st <= fx && st <= dy ? 0 : fx <= dy ? 1 : 2;
  *bytes = (int)(form == 0 ? st : form == 1 ? fx : dy);
  return form;
}

// The halves of a dynamic block's tokens, at most kMaxHalfTokenBits each: a literal (or the end of block) is its
// code; a match is its length symbol's code and extra bits, then its distance code and extra bits.
SBAM_DEFL_HD Token dyn_symbol(const Code *lit, int sym) { return Token{lit[sym].bits, lit[sym].n}; }
SBAM_DEFL_HD Token dyn_length(const Code *lit, int len) {
  int ls, le;
  uint32_t lx;
  length_code(len, &ls, &le, &lx);
  return Token{(uint32_t)lit[ls].bits | lx << lit[ls].n, lit[ls].n + le};
}
SBAM_DEFL_HD Token dyn_distance(const Code *dist, int d) {
  int dc, de;
  uint32_t dx;
  distance_code(d, &dc, &de, &dx);
  return Token{(uint32_t)dist[dc].bits | dx << dist[dc].n, dist[dc].n + de};
}
// the fixed code laid out as a dynamic one's tables, for a writer that emits both forms from the same arrays
SBAM_DEFL_HD Code fixed_lit_code(int sym) {
  const Token t = fixed_symbol(sym);
  return Code{(uint16_t)t.bits, (uint16_t)t.n};
}
SBAM_DEFL_HD Code fixed_dist_code(int code) { return Code{(uint16_t)reverse_bits((uint32_t)code, 5), 5}; }

}  // namespace sbam_deflate

