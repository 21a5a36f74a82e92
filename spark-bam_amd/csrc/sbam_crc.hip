// sbam_crc.hip — CRC32 of every BGZF block's inflated bytes against the value its footer stores (gfx950).
//
// The reference never reads the footer's CRC (Stream.scala:49-54 checks ISIZE only); htslib's bgzf reader verifies
// every block, htsjdk offers it (setCheckCrcs).  This kernel is that check on the device-resident stream.
//
// One wavefront per BGZF block, kCrcWaves waves per workgroup, the block index taken from the wave id so that
// neighbouring waves read neighbouring stream bytes; a workgroup builds the lookup tables in LDS once (from the
// polynomial: no global tables, no mutable global state) and then strides over the table.  The arithmetic — rows of
// 64 pieces of 16 bytes, each lane folding its pieces with 16 LDS lookups per piece, the shifts as multiplications by
// powers of x, an XOR reduction over the wave — is sbam_crc_core.h, shared with the host test.
//
// Bound: every stream byte is loaded once (16 B per lane, coalesced); per KiB and wave the LDS serves 16 ds_read_b32
// of random table words (bank = byte value mod 32, so about 3 to 4 distinct addresses meet on the busiest bank of a
// 32-lane group).  DESIGN.md §CRC check has the measured rate.
#include "sbam_crc_core.h"
#include "sbam_internal.h"

namespace sbam {

namespace {

constexpr int kCrcWaves = 8;  // waves (blocks in flight) per workgroup; the 33 KiB of tables allow 4 workgroups per CU

__global__ __launch_bounds__(64 * kCrcWaves) void block_crc_kernel(const uint8_t *__restrict__ comp, int64_t D,
                                                                   const uint8_t *__restrict__ u, int64_t L,
                                                                   BlockTable bt, int64_t b0, int64_t b1,
                                                                   uint32_t *__restrict__ crc,
                                                                   uint32_t *__restrict__ stored,
                                                                   unsigned long long *__restrict__ n_bad,
                                                                   unsigned long long *__restrict__ first_bad) {
  __shared__ uint32_t tab[sbam_crc::kTabWords];
  for (uint32_t i = threadIdx.x; i < (uint32_t)sbam_crc::kTabWords; i += blockDim.x) tab[i] = sbam_crc::table_word(i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t g = b0 + (int64_t)blockIdx.x * kCrcWaves; g < b1; g += (int64_t)gridDim.x * kCrcWaves) {
    const int64_t b = g + wave;
    if (b >= b1) continue;
    // wave-uniform block geometry
    const int32_t n = __builtin_amdgcn_readfirstlane(bt.usize[b]);
    const int64_t uo_ = bt.uoff[b];
    const int64_t uo = ((int64_t)__builtin_amdgcn_readfirstlane((int32_t)(uo_ >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)uo_);
    uint32_t terms = 0;
    const bool in_stream = n > 0 && uo >= 0 && uo + n <= L;  // (always, after a successful inflate)
    if (in_stream) terms = sbam_crc::lane_term(tab, u, uo, n, lane);
    for (int o = 32; o > 0; o >>= 1) terms ^= __shfl_xor(terms, o, 64);
    if (lane == 0) {
      const uint32_t c = in_stream ? sbam_crc::finish(tab, terms, n) : 0u;
      // the footer's CRC32 sits 8 bytes before the block's end: unaligned, read by bytes
      const int64_t f = bt.start[b] + bt.csize[b] - 8;
      uint32_t s = 0;
      if (f >= 0 && f + 4 <= D)
        s = (uint32_t)comp[f] | ((uint32_t)comp[f + 1] << 8) | ((uint32_t)comp[f + 2] << 16) | ((uint32_t)comp[f + 3] << 24);
      crc[b] = c;
      stored[b] = s;
      if (c != s) {
        atomicAdd(n_bad, 1ull);
        atomicMin(first_bad, (unsigned long long)b);
      }
    }
  }
}

}  // namespace

hipError_t launch_block_crc(const uint8_t *comp, int64_t D, const uint8_t *u, int64_t L, BlockTable bt, int64_t b0,
                            int64_t b1, uint32_t *crc, uint32_t *stored, unsigned long long *n_bad,
                            unsigned long long *first_bad, hipStream_t s) {
  if (b1 <= b0) return hipSuccess;
  const int64_t groups = (b1 - b0 + kCrcWaves - 1) / kCrcWaves;
  const int grid = (int)(groups < 1024 ? groups : 1024);  // 4 workgroups per CU x 256 CUs, striding over the table
  hipLaunchKernelGGL(block_crc_kernel, dim3(grid), dim3(64 * kCrcWaves), 0, s, comp, D, u, L, bt, b0, b1, crc, stored,
                     n_bad, first_bad);
  return hipGetLastError();
}

}  // namespace sbam
