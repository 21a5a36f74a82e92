// sbam_sort_core.h — the coordinate order's one definition (sbam_sort.hip), host- and device-callable, so that a plain
// C++ program can test the key against a restatement (tests/test_sort_host.py).
//
// The key of a record is the 64-bit unsigned word  (uint32) ref_id << 32 | (uint32) (pos ^ 0x80000000):
//   references ascend as unsigned, so ref_id == -1 (no coordinate) sorts last;
//   within a reference pos ascends as signed (the xor moves INT32_MIN to 0), so -1 sorts first.
// Records with equal keys keep their loaded order: the sort is stable and its result a function of the two columns
// alone.  This is the order sbam_build_index's n_unsorted tests and the one htsjdk and samtools accept as
// SO:coordinate; it is not `samtools sort`'s tie order, which adds the strand bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBAM_SORT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBAM_SORT_HD inline
#endif

namespace sbam_sort {

constexpr int kDigitBits = 8;                   // an LSD radix pass sorts by one byte of the key
constexpr int kDigits = 1 << kDigitBits;        // bins of a pass
constexpr int kMaxPasses = 64 / kDigitBits;     // bytes of a key

SBAM_SORT_HD constexpr uint64_t key(int32_t ref_id, int32_t pos) {
  return ((uint64_t)(uint32_t)ref_id << 32) | (uint64_t)((uint32_t)pos ^ 0x80000000u);
}

// byte `pass` of a key (0: the least significant)
SBAM_SORT_HD constexpr uint32_t digit(uint64_t k, int pass) { return (uint32_t)(k >> (kDigitBits * pass)) & (kDigits - 1); }

}  // namespace sbam_sort
