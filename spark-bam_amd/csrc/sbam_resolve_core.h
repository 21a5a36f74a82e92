// sbam_resolve_core.h — the position arithmetic of the resolver's dependent pass (k_inflate_resolve, step 3c of
// sbam_inflate.hip), host- and device-callable, so that a plain C++ program can replay it on token lists
// (tests/test_resolve_core_host.py).
//
// A match (mO, d, Le) writes output positions [mO, mO + Le) from the bytes d positions back.  Within one resolver
// step the matches whose source reaches past the step's base are *dependents*: their bytes are produced one per
// lane, each lane finding the position that holds its byte's value outside every dependent's output:
//   collapsed source  byte j of a match is byte j mod d of its period, which starts at mO - d: a self-overlapping
//                     match (d < Le) never reads its own output;
//   sweep             dependents' outputs are disjoint and in position order, and a hop out of dependent k lands
//                     below mO_k, so it can only land in an earlier dependent: visiting the dependents once, last to
//                     first, follows a source chain of any depth to its end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBAM_RS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SBAM_RS_HD inline
#endif

namespace sbam_resolve {

constexpr int kMaxMatch = 258;  // RFC 1951: the longest match, so r below is < 258

// Offset r (0 <= r < Le) of a match's output, folded into the match's first period [0, d).  The division is only
// needed when r >= d: the kernel asks for it only when some lane of the wave is in that case.
SBAM_RS_HD int period_offset(int r, int d) { return r < d ? r : (int)((uint32_t)r % (uint32_t)d); }

// The position whose byte output byte j of match (mO, d) repeats: in [mO - d, mO).
SBAM_RS_HD int collapsed_source(int mO, int d, int j) { return mO - d + period_offset(j, d); }

// s inside dependent k's output [mO_k, mO_k + Le_k)?
SBAM_RS_HD bool hop_hits(int s, int mOk, int Lek) { return (uint32_t)(s - mOk) < (uint32_t)Lek; }

// One sweep visit: the position that holds the value of position s once dependent (mO_k, d_k, Le_k) is ruled out.
SBAM_RS_HD int sweep_hop(int s, int mOk, int dk, int Lek) {
  return hop_hits(s, mOk, Lek) ? collapsed_source(mOk, dk, s - mOk) : s;
}

// The whole descending sweep over n dependents in position order (the kernel walks a lane mask the same way).
SBAM_RS_HD int sweep(int s, const int *mO, const int *d, const int *Le, int n) {
  for (int k = n - 1; k >= 0; k--) s = sweep_hop(s, mO[k], d[k], Le[k]);
  return s;
}

}  // namespace sbam_resolve
