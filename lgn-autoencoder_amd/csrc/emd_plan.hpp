// lgn-autoencoder_amd/csrc/emd_plan.hpp -- what the hosts of the EMD kernels (emd.hip, emd_pairs.hip) plan with: the LDS of one
// wavefront, where the flow matrix lives, the workspace of the flows that do not fit LDS, and the pair numbering of the all-pairs
// kernel.  No device code of emd.hip depends on this file: its kernels carve their LDS by hand in the order emd_lds_doubles counts.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "../../include/lgn_amd.h"

namespace lgn {

constexpr int EMD_LDS_BUDGET = 64 * 1024;      // plan-time budget of one wave's LDS (no opt-in launch attribute below it)
constexpr int EMD_GLOBAL_WAVES = 2048;         // resident waves of the workspace path: 8 per CU

__host__ __device__ constexpr long long emd_lds_doubles(int n, int m, bool lds_flow) {
  return 5ll * (n + 1) + 8 + (lds_flow ? (long long)(n + 1) * (m + 1) : 0);
}
__host__ __device__ constexpr long long emd_lds_total(int n, int m, bool lds_flow) {
  return 8 * emd_lds_doubles(n, m, lds_flow) + 8ll * (n + 1);
}
inline bool emd_flow_in_lds(int N) { return emd_lds_total(N, N, true) <= EMD_LDS_BUDGET; }
inline long long emd_workspace(long long B, int N) {
  if (emd_flow_in_lds(N)) return 0;
  return (B < EMD_GLOBAL_WAVES ? B : EMD_GLOBAL_WAVES) * (long long)(N + 1) * (N + 1) * 8;
}

inline int emd_check_work(const char* who, long long B, int N, const void* work, long long work_bytes) {
  const long long need = emd_workspace(B, N);
  if (need == 0) return 0;
  LGN_CHECK_ARG(work, "%s: N = %d keeps the flow in a workspace: null work (lgn_emd_workspace_bytes: %lld bytes)", who, N, need);
  LGN_CHECK_ARG(work_bytes >= need, "%s: workspace of %lld bytes is too short (%lld needed)", who, work_bytes, need);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  return 0;
}

// ---- pair numbering of lgn_emd_pairs_f64 (include/lgn_amd.h) ------------------------------------------------------------------------
// FULL: p = i B1 + j.  ALIGNED: p = i = j.  UPPER: the pairs i < j of B events, row-major over the upper triangle: row i starts at
// emd_upper_row_start(i, B) and holds B - 1 - i pairs.
__host__ __device__ inline long long emd_pairs_count(int mode, int B0, int B1) {
  if (mode == LGN_EMD_PAIRS_FULL) return (long long)B0 * B1;
  if (mode == LGN_EMD_PAIRS_UPPER) return (long long)B0 * (B0 - 1) / 2;
  return B0;
}
__host__ __device__ inline unsigned long long emd_upper_row_start(unsigned long long i, unsigned long long B) {
  return i * (2 * B - i - 1) / 2;                 // (one of the two factors is even; below 2^63 for B < 2^31)
}
// p in [0, emd_pairs_count) -> (i, j).  The square root only seeds the row of UPPER; the two integer loops decide it.
__host__ __device__ inline void emd_pairs_decode(int mode, long long p, int B0, int B1, int& i, int& j) {
  if (mode == LGN_EMD_PAIRS_FULL) {
    i = (int)(p / B1), j = (int)(p % B1);
  } else if (mode == LGN_EMD_PAIRS_UPPER) {
    const unsigned long long B = (unsigned long long)B0, q = (unsigned long long)p;
    const double t = 2.0 * (double)B0 - 1.0;
    double disc = t * t - 8.0 * (double)p;
    disc = disc > 0.0 ? disc : 0.0;
    long long r = (long long)((t - sqrt(disc)) * 0.5);
    r = r < 0 ? 0 : (r > (long long)B0 - 2 ? (long long)B0 - 2 : r);
    while (r > 0 && emd_upper_row_start((unsigned long long)r, B) > q) --r;
    while (r < (long long)B0 - 2 && emd_upper_row_start((unsigned long long)r + 1, B) <= q) ++r;
    i = (int)r, j = (int)(r + 1 + (long long)(q - emd_upper_row_start((unsigned long long)r, B)));
  } else {
    i = j = (int)p;
  }
}

}  // namespace lgn
