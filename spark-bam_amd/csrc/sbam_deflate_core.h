// sbam_deflate_core.h — what the BAM writer's DEFLATE encoder (sbam_write.hip) knows without a GPU, host- and
// device-callable, so that a plain C++ program can emit streams from the same tables and hand them to zlib
// (tests/test_deflate_host.py).
//
// RFC 1951.  A block is either stored (BTYPE = 00: five header bytes, then the bytes) or one fixed-Huffman block
// (BTYPE = 01, BFINAL = 1).  The fixed code:
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

}  // namespace sbam_deflate
