// sbam_device.h — device-only helpers shared by the kernels (wave64, gfx950): wave reductions, the wave scan, and
// the one workgroup scan every prefix sum of the library is built from.  Included by the .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SB_DEV __device__ __forceinline__

namespace sbam {

SB_DEV int lane_id() { return __lane_id(); }

template <class T>
SB_DEV T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
SB_DEV uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
template <class T>
SB_DEV T wave_min(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
template <class T>
SB_DEV T wave_max(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// inclusive scan across the wave: lane l receives v of lanes 0 .. l
template <class T>
SB_DEV T wave_incl_scan(T v) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// the 8 bytes at u + x (u 4-byte aligned, x of any alignment) from the three aligned dwords around them; the buffer is
// readable for 12 bytes past x rounded down to 4
SB_DEV uint64_t load8(const uint8_t *u, int64_t x) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(u + (x & ~(int64_t)3));
  const uint32_t s = (uint32_t)(x & 3);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
  const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, s), hi = __builtin_amdgcn_alignbyte(w2, w1, s);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// Workgroup inclusive scan of K values per thread (THREADS = blockDim.x; thread order = threadIdx.x): incl[f] = the
// sum of v[f] over threads 0 .. threadIdx.x, total[f] = over all of them.  ws: THREADS / 64 rows of LDS scratch.
// Every thread of the workgroup calls it (two barriers).
//
// Barrier contract: the trailing barrier is part of the primitive.  When the call returns, every thread has read
// what it needs from ws, so ws may be reused at once, by the next call or for anything else; callers add no barrier
// for the scan's sake and rely on none beyond these two.
template <class T, int K, int THREADS>
SB_DEV void block_incl_scan(const T (&v)[K], T (&incl)[K], T (&total)[K], T (*ws)[K]) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves, one workgroup");
  constexpr int kWaves = THREADS / 64;
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int f = 0; f < K; f++) {
    incl[f] = wave_incl_scan(v[f]);
    if (lane == 63) ws[w][f] = incl[f];
  }
  __syncthreads();
  T before[K], tot[K];
#pragma unroll
  for (int f = 0; f < K; f++) before[f] = tot[f] = 0;
#pragma unroll 4  // (all of sixteen waves' rows in flight at once is 128 registers for four int64 columns)
  for (int k = 0; k < kWaves; k++) {
#pragma unroll
    for (int f = 0; f < K; f++) {
      const T x = ws[k][f];
      before[f] += k < w ? x : (T)0;
      tot[f] += x;
    }
  }
#pragma unroll
  for (int f = 0; f < K; f++) {
    incl[f] += before[f];
    total[f] = tot[f];
  }
  __syncthreads();
}

// the same for one value per thread: returns the inclusive sum; ws: THREADS / 64 entries
template <class T, int THREADS>
SB_DEV T block_incl_scan(T v, T &total, T *ws) {
  const T in[1] = {v};
  T incl[1], tot[1];
  block_incl_scan<T, 1, THREADS>(in, incl, tot, reinterpret_cast<T(*)[1]>(ws));
  total = tot[0];
  return incl[0];
}

}  // namespace sbam
