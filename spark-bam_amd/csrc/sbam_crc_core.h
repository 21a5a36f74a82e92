// sbam_crc_core.h — the arithmetic of the BGZF block CRC32 check (sbam_crc.hip), host- and device-callable, so that
// a plain C++ program can replay the kernel's decomposition lane by lane (tests/test_crc_host.py).
//
// CRC-32 is the IEEE reflected form (polynomial 0xEDB88320, init and final xor 0xFFFFFFFF: zlib.crc32).  With
// raw(s, M) the register update without init or final xor, and shift(s, n) = s * x^(8n) mod P (n zero bytes):
//   raw(0, zeros ‖ M) = raw(0, M)                      leading zero bytes are free
//   raw(s, A ‖ B)     = shift(raw(s, A), |B|) ^ raw(0, B)
//   crc32(M)          = ~( shift(~0, |M|) ^ XOR_i shift(raw(0, piece_i), bytes behind piece_i) )
// A wave cuts a block into rows of 64 pieces of 16 bytes (16-byte aligned in the stream); lane l owns piece l of every
// row and folds its pieces into one accumulator, 16 table lookups per piece:
//   T[j][v] = raw state of byte v followed by j zero bytes           -> accumulator positioned at the piece's end
//   U[j][v] = the same followed by 1008 + j zero bytes               -> positioned at the lane's piece of the next row
// A lane uses U while it has a byte in the next row, T for its last whole piece, and T[0] byte by byte for a piece the
// block's end cuts.  Its accumulator is then less than 1024 bytes before the block's end; that shift, and the init
// term's (up to 65536 bytes), are bitwise multiplications by powers of x taken from three small tables.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBAM_CRC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBAM_CRC_HD inline
#endif

namespace sbam_crc {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kRowBytes = 1024;          // 64 lanes x 16 bytes
constexpr int kTabT = 0;                 // T[16][256]
constexpr int kTabU = 4096;              // U[16][256]
constexpr int kTabPow = 8192;            // x^(8 d): d < 32 | x^(8 32 d): d < 32 | x^(8 1024 d): d <= 64
constexpr int kPowWords = 32 + 32 + 65;
constexpr int kTabWords = kTabPow + kPowWords;

// a * b mod P; bit 31 is the coefficient of x^0 (the reflected register)
SBAM_CRC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// raw(0, one byte v)
SBAM_CRC_HD constexpr uint32_t byte_entry(uint32_t v) {
  for (int i = 0; i < 8; i++) v = (v >> 1) ^ (kPoly & (0u - (v & 1u)));
  return v;
}

struct Consts {
  uint32_t sh[32];          // x^(8 j), j < 16 (T); x^(8 (1008 + j)), j < 16 (U)
  uint32_t pw[kPowWords];   // the three power tables, as in the table image
};

constexpr Consts make_consts() {
  Consts c{};
  const uint32_t x8 = 0x00800000u;
  uint32_t *plo = c.pw, *pmid = c.pw + 32, *phi = c.pw + 64;
  plo[0] = 0x80000000u;
  for (int d = 1; d < 32; d++) plo[d] = mulmod(plo[d - 1], x8);
  const uint32_t x256 = mulmod(plo[31], x8);
  pmid[0] = 0x80000000u;
  for (int d = 1; d < 32; d++) pmid[d] = mulmod(pmid[d - 1], x256);
  const uint32_t x8192 = mulmod(pmid[31], x256);
  phi[0] = 0x80000000u;
  for (int d = 1; d <= 64; d++) phi[d] = mulmod(phi[d - 1], x8192);
  const uint32_t x1008 = mulmod(pmid[31], plo[16]);  // 1008 = 31 * 32 + 16 bytes
  for (int j = 0; j < 16; j++) {
    c.sh[j] = plo[j];
    c.sh[16 + j] = mulmod(x1008, plo[j]);
  }
  return c;
}

// word idx of the table image (kTabWords words: built once per workgroup into LDS, or by the host)
SBAM_CRC_HD uint32_t table_word(uint32_t idx) {
  constexpr Consts C = make_consts();
  if (idx >= (uint32_t)kTabPow) return C.pw[idx - kTabPow];
  return mulmod(byte_entry(idx & 255u), C.sh[idx >> 8]);
}

// x^(8 n) for n <= 65536 + 1023
SBAM_CRC_HD uint32_t xpow_bytes(const uint32_t *tab, uint32_t n) {
  const uint32_t *pw = tab + kTabPow;
  const uint32_t lo = mulmod(pw[n & 31u], pw[32 + ((n >> 5) & 31u)]);
  return (n >> 10) ? mulmod(lo, pw[64 + (n >> 10)]) : lo;
}

struct alignas(16) Piece {
  uint32_t w[4];
};

// 16 bytes into the accumulator (positioned at the piece's start); t = tab + kTabT or tab + kTabU
SBAM_CRC_HD uint32_t fold16(const uint32_t *t, uint32_t acc, const Piece &p) {
  const uint32_t a = p.w[0] ^ acc, b = p.w[1], c = p.w[2], d = p.w[3];
  return t[15 * 256 + (a & 255u)] ^ t[14 * 256 + ((a >> 8) & 255u)] ^ t[13 * 256 + ((a >> 16) & 255u)] ^
         t[12 * 256 + (a >> 24)] ^ t[11 * 256 + (b & 255u)] ^ t[10 * 256 + ((b >> 8) & 255u)] ^
         t[9 * 256 + ((b >> 16) & 255u)] ^ t[8 * 256 + (b >> 24)] ^ t[7 * 256 + (c & 255u)] ^
         t[6 * 256 + ((c >> 8) & 255u)] ^ t[5 * 256 + ((c >> 16) & 255u)] ^ t[4 * 256 + (c >> 24)] ^
         t[3 * 256 + (d & 255u)] ^ t[2 * 256 + ((d >> 8) & 255u)] ^ t[1 * 256 + ((d >> 16) & 255u)] ^ t[d >> 24];
}

// bytes [lo, hi) of the piece, one at a time (the piece the block's end cuts)
SBAM_CRC_HD uint32_t fold_bytes(const uint32_t *tab, uint32_t acc, const Piece &p, int lo, int hi) {
  for (int i = 0; i < 16; i++) {
    const uint32_t v = (p.w[i >> 2] >> (8 * (i & 3))) & 255u;
    if (i >= lo && i < hi) acc = tab[kTabT + ((acc ^ v) & 255u)] ^ (acc >> 8);
  }
  return acc;
}

// zero the first k bytes (k <= 16) of a piece: the bytes in front of the block
SBAM_CRC_HD void mask_head(Piece &p, int k) {
  for (int j = 0; j < 4; j++) {
    const int z = k - 4 * j;  // bytes of word j to clear
    if (z >= 4) p.w[j] = 0;
    else if (z > 0) p.w[j] &= ~0u << (8 * z);
  }
}

// One lane's share of block bytes u[uo, uo + n), n > 0: returns its accumulator shifted to the block's end, i.e. its
// term of the XOR over the wave.  u is 16-byte aligned and readable for 2 KiB + 16 B past the block's end.
SBAM_CRC_HD uint32_t lane_term(const uint32_t *tab, const uint8_t *u, int64_t uo, int32_t n, int lane) {
  const int64_t a0 = uo & ~(int64_t)15, E = uo + n;
  const int nrows = (int)((E - a0 + kRowBytes - 1) / kRowBytes);
  int64_t q = a0 + 16 * lane;
  uint32_t acc = 0, dist = 0;
  Piece next = *reinterpret_cast<const Piece *>(u + q);
  for (int r = 0; r < nrows; r++, q += kRowBytes) {
    Piece p = next;
    if (r + 1 < nrows) next = *reinterpret_cast<const Piece *>(u + q + kRowBytes);
    const int64_t rem = E - q;  // block bytes from the piece's start on
    if (rem >= 16) {
      if (r == 0 && q < uo) mask_head(p, (int)(uo - q < 16 ? uo - q : 16));
      const bool more = rem > kRowBytes;  // the lane has a byte in the next row
      acc = fold16(tab + (more ? kTabU : kTabT), acc, p);
      if (!more) dist = (uint32_t)(rem - 16);
    } else if (rem > 0) {
      acc = fold_bytes(tab, acc, p, (r == 0 && q < uo) ? (int)(uo - q) : 0, (int)rem);
      dist = 0;
    }
  }
  return mulmod(acc, xpow_bytes(tab, dist));
}

// XOR of the 64 lane terms -> the block's CRC32
SBAM_CRC_HD uint32_t finish(const uint32_t *tab, uint32_t terms, int32_t n) {
  return ~(mulmod(0xFFFFFFFFu, xpow_bytes(tab, (uint32_t)n)) ^ terms);
}

}  // namespace sbam_crc
