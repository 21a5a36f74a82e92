// sbam_tag_core.h — the arithmetic of one step of a BAM tag-list walk (sbam_tags.hip), host- and device-callable, so
// that a plain C++ program can replay what a lane and what a wave of the kernel do (tests/test_record_tags_host.py).
//
// A record's tag bytes (SAM spec §4.2.4) are a list without an index: two name bytes, a type byte, then a value whose
// length depends on the type:
//   A c C        1 byte          s S     2 bytes          i I f     4 bytes
//   Z H          characters up to and including a NUL
//   B            a subtype byte (c C s S i I f), an int32 count, count elements of the subtype's width
// decode_at() reads the header at one position and says where the value lies, how long it is and where the next
// header starts, or that the list is malformed there.  Its two accesses to the bytes are functors: hdr(p, cnt) gives
// the cnt <= 8 bytes at p as a little-endian word, nul(from, n) the index of the first NUL in [from, n) or -1.  A lane
// of the kernel reads both from its LDS stage; a wave reads the header with one lane and searches the NUL with all 64
// (lane_first_nul per lane, the lowest lane with a hit wins).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBAM_TAG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBAM_TAG_HD inline
#endif

namespace sbam_tag {

constexpr int kMaxTags = 32;        // SBAM_MAX_TAGS
constexpr int kLongAuxBytes = 1024; // a record with more tag bytes is walked by a whole wave
constexpr int kNulStepBytes = 256;  // bytes one step of the wave's NUL search covers: 64 lanes x one aligned dword

// bytes of a scalar value of this type; 0: not a scalar type
SBAM_TAG_HD int scalar_width(uint32_t t) {
  switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
  }
  return 0;
}
// bytes of one element of a B array of this subtype; 0: unknown subtype
SBAM_TAG_HD int elem_width(uint32_t t) { return t == 'A' ? 0 : scalar_width(t); }

// the value column's entry of a scalar: raw = the value's bytes, little-endian, with whatever follows them above
SBAM_TAG_HD int64_t scalar_value(uint32_t type, uint32_t raw) {
  switch (type) {
    case 'c': return (int8_t)raw;
    case 'A': case 'C': return raw & 0xffu;
    case 's': return (int16_t)raw;
    case 'S': return raw & 0xffffu;
    case 'i': return (int32_t)raw;
  }
  return raw;  // I, f: 32 bits, zero-extended
}

struct Head {
  int32_t val_off;  // the value's first byte, from the header's: 3, or 8 behind a B's subtype and count
  int32_t val_len;  // its bytes; -1: NUL-terminated (Z, H)
  bool bad;
};

// One step: a header with `left` bytes from its first byte to the record's end; sub and count are the bytes behind
// the type, read only for a B with left >= 8.
SBAM_TAG_HD Head head(uint32_t type, uint32_t sub, int32_t count, int64_t left) {
  Head h{3, 0, true};
  if (left < 3) return h;
  const int w = scalar_width(type);
  if (w) {
    h.val_len = w;
    h.bad = 3 + w > left;
  } else if (type == 'Z' || type == 'H') {
    h.val_len = -1;
    h.bad = false;
  } else if (type == 'B') {
    const int ew = elem_width(sub);
    if (left < 8 || ew == 0 || count < 0 || 8 + (int64_t)count * ew > left) return h;
    h.val_off = 8;
    h.val_len = count * ew;
    h.bad = false;
  }
  return h;
}

struct Cell {
  uint32_t key;   // name[0] | name[1] << 8
  uint32_t type, sub;
  int32_t pos;    // the header's first byte
  int32_t rel;    // the value's first byte
  int32_t len;    // the value's bytes (Z, H: without the NUL)
  int32_t next;   // the next header
  int64_t value;  // the value column's entry
  bool bad;
};

SBAM_TAG_HD uint32_t tag_key(uint32_t c0, uint32_t c1) { return (c0 & 0xffu) | ((c1 & 0xffu) << 8); }
// bit of a 64-bit filter over the queried names: a name whose bit is clear is in no query
SBAM_TAG_HD uint32_t filter_bit(uint32_t key) { return (key ^ (key >> 5) ^ (key >> 10)) & 63u; }
// whether a type's value has bytes for a want_bytes column
SBAM_TAG_HD bool has_bytes(uint32_t type) { return type == 'Z' || type == 'H' || type == 'B'; }

// the tag whose header starts at byte p of a record's n tag bytes
template <class Hdr, class Nul>
SBAM_TAG_HD Cell decode_at(Hdr hdr, Nul nul, int32_t n, int32_t p) {
  Cell c{};
  c.bad = true;
  c.pos = p;
  const int32_t left = n - p;
  if (left < 3) return c;
  const uint64_t h = hdr(p, left < 8 ? left : 8);
  c.key = (uint32_t)h & 0xffffu;
  c.type = (uint32_t)(h >> 16) & 0xffu;
  const uint32_t sub = (uint32_t)(h >> 24) & 0xffu;
  const int32_t count = (int32_t)(uint32_t)(h >> 32);
  const Head hd = head(c.type, sub, count, left);
  if (hd.bad) return c;
  c.rel = p + hd.val_off;
  if (hd.val_len < 0) {
    const int32_t e = nul(c.rel, n);
    if (e < 0) return c;
    c.len = e - c.rel;
    c.next = e + 1;
    c.value = c.len;
  } else {
    c.len = hd.val_len;
    c.next = c.rel + c.len;
    if (c.type == 'B') {
      c.sub = sub;
      c.value = count;
    } else {
      c.value = scalar_value(c.type, (uint32_t)(h >> 24));
    }
  }
  c.bad = false;
  return c;
}

// The whole list: on(cell) for every tag in file order; false when the list is malformed (on() has then seen the
// tags in front of the bad one).
template <class Hdr, class Nul, class On>
SBAM_TAG_HD bool walk(Hdr hdr, Nul nul, int32_t n, On on) {
  int32_t p = 0;
  while (p < n) {
    const Cell c = decode_at(hdr, nul, n, p);
    if (c.bad) return false;
    on(c);
    p = c.next;
  }
  return true;
}

// One lane's share of a step of the wave's NUL search: w holds tag bytes [q0, q0 + 4) (q0 may be negative in the
// first step: the dword is aligned in the stream, not in the record); the index of its first zero byte inside
// [from, end), or -1.
SBAM_TAG_HD int32_t lane_first_nul(uint32_t w, int32_t q0, int32_t from, int32_t end) {
  for (int b = 0; b < 4; b++) {
    const int32_t q = q0 + b;
    if (q >= from && q < end && ((w >> (8 * b)) & 0xffu) == 0) return q;
  }
  return -1;
}
// first byte index (a multiple of 4 in the stream, so possibly up to 3 below `from`) of the search's first step, for
// tag bytes that start at stream offset x
SBAM_TAG_HD int32_t nul_first_step(int64_t x, int32_t from) { return (int32_t)(((x + from) & ~(int64_t)3) - x); }

}  // namespace sbam_tag
