// lgn-autoencoder_amd/csrc/lds.hpp -- dynamic LDS: one launch function, and the carve a kernel shares with its launcher.
//
// A layout is a __host__ __device__ struct built from the shape arguments the kernel sees: its constructor walks an LdsCarve, every
// member is the byte offset of a region, `bytes` is the total.  The kernel takes its pointers from it (lds_at<T>(smem_raw, L.region)),
// the launcher hands L.bytes to lds_launch; nobody else computes either.  (DESIGN section 4 says which kernels have one, and why the
// others still carve by hand.)
#pragma once
#include "common.hpp"
#include "../../include/lgn_amd.h"

namespace lgn {

struct LdsCarve {
  size_t off = 0;
  template <typename T>
  __host__ __device__ size_t take(size_t n) {       // n elements of T; returns the byte offset they start at
    const size_t o = off;
    off += n * sizeof(T);
    return o;
  }
};

template <typename T>
__device__ __forceinline__ T* lds_at(unsigned char* smem, size_t byte_off) { return reinterpret_cast<T*>(smem + byte_off); }

// The one way a kernel with `bytes` of dynamic LDS is launched: refuses what no CU holds, lifts the 64 KiB default, launches, checks.
// No cache: the attribute call is per launch (a host-side table write; a captured graph replays none of it).
template <typename... P, typename... A>
int lds_launch(void (*kernel)(P...), const char* what, dim3 grid, dim3 block, size_t bytes, hipStream_t stream, A&&... args) {
  LGN_CHECK_ARG(bytes <= LGN_LDS_LIMIT, "%s: needs %zu B of LDS (> %d)", what, bytes, LGN_LDS_LIMIT);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    LGN_CHECK_ARG(e == hipSuccess, "%s: cannot raise dynamic LDS to %zu B: %s", what, bytes, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kernel, grid, block, bytes, stream, args...);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // namespace lgn
