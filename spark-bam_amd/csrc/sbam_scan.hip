// sbam_scan.hip — the device-wide exclusive prefix sums every stage uses (gfx950), on sbam_device.h's workgroup scan.
//
//   launch_scan_sums       one workgroup per column turns n per-workgroup sums (int32 or int64) into int64 exclusive
//                          offsets plus the column's total.  Thread t owns the contiguous run [t·per, (t + 1)·per) of the
//                          sums: it adds up its run, one workgroup scan of the 1024 run sums gives every run its base,
//                          and the run is written out: two passes over n integers and two barriers, instead of
//                          n / 1024 barrier-separated rounds (311 -> ~20 us for the 206 K chunks of a 10 GB shard).
//   launch_exclusive_scan  int64 length columns -> exclusive offsets in place: per-workgroup sums, launch_scan_sums
//                          over them, per-workgroup offsets; one grid row per column.
#include "sbam_device.h"
#include "sbam_internal.h"

namespace sbam {

namespace {

constexpr int kScanThreads = 1024;
constexpr int kRunBatch = 8;  // elements of a run in flight

// column c = blockIdx.x: out[c * n + i] = sum of in[c * n + j], j < i; totals[c] = the column's sum.  out may be in
// (int64): every element is read into registers before it is written, and no thread touches another's run.
template <class In>
__global__ void __launch_bounds__(kScanThreads) k_scan_sums(const In *in, int64_t *out, int64_t n, int64_t *totals) {
  __shared__ int64_t ws[kScanThreads / 64];
  in += (int64_t)blockIdx.x * n;
  out += (int64_t)blockIdx.x * n;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t b = min((int64_t)threadIdx.x * per, n), e = min(b + per, n);
  int64_t sum = 0;
#pragma unroll 8
  for (int64_t i = b; i < e; i++) sum += in[i];
  int64_t total;
  int64_t run = block_incl_scan<int64_t, kScanThreads>(sum, total, ws) - sum;
  int64_t i = b;
  for (; i + kRunBatch <= e; i += kRunBatch) {
    int64_t v[kRunBatch];
#pragma unroll
    for (int k = 0; k < kRunBatch; k++) v[k] = in[i + k];
#pragma unroll
    for (int k = 0; k < kRunBatch; k++) {
      out[i + k] = run;
      run += v[k];
    }
  }
  for (; i < e; i++) {
    const int64_t v = in[i];
    out[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// grid (nblk, cols): bsum[c * nblk + blk] = the sum of column c over workgroup blk's elements
__global__ void __launch_bounds__(kScanThreads) k_scan_block_sums(const int64_t *__restrict__ off, int64_t stride,
                                                                  int64_t n, int64_t nblk, int64_t *__restrict__ bsum) {
  __shared__ int64_t ws[kScanThreads / 64];
  const int64_t k = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
  int64_t total;
  block_incl_scan<int64_t, kScanThreads>(k < n ? off[blockIdx.y * stride + k] : 0, total, ws);
  if (threadIdx.x == 0) bsum[blockIdx.y * nblk + blockIdx.x] = total;
}

// grid (nblk, cols): column c's values -> exclusive prefix sums in place, [n] = its total
__global__ void __launch_bounds__(kScanThreads) k_scan_offsets(int64_t *__restrict__ off, int64_t stride, int64_t n,
                                                               int64_t nblk, const int64_t *__restrict__ bsum) {
  __shared__ int64_t ws[kScanThreads / 64];
  const int64_t k = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
  int64_t *col = off + blockIdx.y * stride;
  const int64_t v = k < n ? col[k] : 0;
  int64_t total;
  const int64_t e = bsum[blockIdx.y * nblk + blockIdx.x] + block_incl_scan<int64_t, kScanThreads>(v, total, ws);
  if (k >= n) return;
  col[k] = e - v;
  if (k == n - 1) col[n] = e;
}

template <class In>
hipError_t scan_sums(const In *in, int64_t *out, int64_t n, int32_t cols, int64_t *totals, hipStream_t s) {
  if (cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scan_sums<In>, dim3((unsigned)cols), dim3(kScanThreads), 0, s, in, out, n < 0 ? 0 : n, totals);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scan_sums(const int32_t *in, int64_t *out, int64_t n, int32_t cols, int64_t *totals, hipStream_t s) {
  return scan_sums(in, out, n, cols, totals, s);
}
hipError_t launch_scan_sums(const int64_t *in, int64_t *out, int64_t n, int32_t cols, int64_t *totals, hipStream_t s) {
  return scan_sums(in, out, n, cols, totals, s);
}

int64_t exclusive_scan_blocks(int64_t n) { return (n + kScanThreads - 1) / kScanThreads; }

hipError_t launch_exclusive_scan(int64_t *off, int64_t stride, int64_t n, int32_t cols, int64_t *bsum, int64_t *totals,
                                 hipStream_t s) {
  if (n < 0 || cols <= 0) return hipSuccess;
  if (n == 0) {  // no element: every column's total, and its only offset, is 0
    hipError_t e = hipMemsetAsync(totals, 0, (size_t)cols * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    return hipMemset2DAsync(off, (size_t)stride * sizeof(int64_t), 0, sizeof(int64_t), (size_t)cols, s);
  }
  const int64_t nblk = exclusive_scan_blocks(n);
  const dim3 grid((unsigned)nblk, (unsigned)cols);
  hipLaunchKernelGGL(k_scan_block_sums, grid, dim3(kScanThreads), 0, s, off, stride, n, nblk, bsum);
  hipError_t e = launch_scan_sums(bsum, bsum, nblk, cols, totals, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scan_offsets, grid, dim3(kScanThreads), 0, s, off, stride, n, nblk, bsum);
  return hipGetLastError();
}

}  // namespace sbam
