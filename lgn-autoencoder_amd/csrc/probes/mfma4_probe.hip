// The four-block fp64 matrix instruction v_mfma_f64_4x4x4_4b_f64 (__builtin_amdgcn_mfma_f64_4x4x4f64): D_b(4x4) += A_b(4x4) B_b(4x4),
// b = 0 .. 3, one double per lane for each of A, B, D.  Two questions before the chain CGMLP kernels use it for their padded last tile:
//   1. which lane holds which element of A, B and D (measured from one-hot A operands against B = 1 + lane);
//   2. what it costs: alone (one accumulator, two, four) and between 16x16x4 instructions that share its B operand (the layers' pattern).
//   hipcc --offload-arch=gfx950 -O3 -o mfma4_probe mfma4_probe.hip && ./mfma4_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double v4d __attribute__((ext_vector_type(4)));

// ---- 1. layout: for every lane la, A = (lane == la), B = 1 + lane; D[la][lane] names the B lane each D lane received
__global__ void layout(double* out) {
  const int lane = threadIdx.x;
  for (int la = 0; la < 64; ++la) {
    const double a = lane == la ? 1.0 : 0.0, b = 1.0 + lane;
    out[la * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0);
  }
}

// ---- 2. cost.  One wave per SIMD (256 threads, one workgroup per CU); shader cycles from clock64.
//   0: thin, one accumulator (dependent chain)        1: thin, two alternating accumulators       2: thin, four accumulators
//   3: full 16x16x4 only, two accumulators            4: full, full, thin sharing B (1 : 2)        5: full, thin sharing B (1 : 1)
//   6: full, thin, thin sharing B (two thin accumulators: a last tile of eight neurons)
constexpr int GROUPS = 24;
template <int VAR>
__global__ __launch_bounds__(256) void cost(double* out, long long* cyc, int rounds) {
  const int lane = threadIdx.x & 63;
  double a0 = 1e-3 * lane, a1 = 2e-3 * lane, a2 = 1e-3 * (lane & 3), b = 1.0 + 1e-3 * lane;
  v4d f0 = {0, 0, 0, 0}, f1 = {0, 0, 0, 0};
  double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  const long long c0 = clock64();
  for (int r = 0; r < rounds; ++r) {
#pragma unroll
    for (int s = 0; s < GROUPS; ++s) {
      if (VAR == 0) t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
      if (VAR == 1) {
        if (s & 1) t1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t1, 0, 0, 0);
        else t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
      }
      if (VAR == 2) {
        if ((s & 3) == 0) t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
        if ((s & 3) == 1) t1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t1, 0, 0, 0);
        if ((s & 3) == 2) t2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t2, 0, 0, 0);
        if ((s & 3) == 3) t3 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t3, 0, 0, 0);
      }
      if (VAR == 3) {
        if (s & 1) f1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, f1, 0, 0, 0);
        else f0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, f0, 0, 0, 0);
      }
      if (VAR == 4) {
        f0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, f0, 0, 0, 0);
        f1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, f1, 0, 0, 0);
        t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
      }
      if (VAR == 5) {
        f0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, f0, 0, 0, 0);
        t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
      }
      if (VAR == 6) {
        f0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, f0, 0, 0, 0);
        t0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t0, 0, 0, 0);
        t1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a2, b, t1, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // feed the results back like the layers do (keeps the compiler from hoisting anything)
    b = fmax(b, 1e-30 * (f0[0] + f1[1] + t0 + t1 + t2 + t3));
  }
  const long long c1 = clock64();
  out[blockIdx.x * blockDim.x + threadIdx.x] = f0[0] + f0[3] + f1[1] + t0 + t1 + t2 + t3 + b;
  if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = c1 - c0;
}

template <int VAR>
static double run(const char* what, int full, int thin, double* out, long long* cyc) {
  const int rounds = 2000;
  long long h = 0;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(cost<VAR>, dim3(256), dim3(256), 0, 0, out, cyc, rounds);
    hipDeviceSynchronize();
    hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost);
  }
  const double per_group = (double)h / ((double)rounds * GROUPS);
  printf("variant %d: %-58s %7.1f cycles per group of %d full + %d thin\n", VAR, what, per_group, full, thin);
  return per_group;
}

int main() {
  double* out; long long* cyc;
  hipMalloc(&out, 1 << 24); hipMalloc(&cyc, 8);
  // ---- layout
  static double h[64 * 64];
  hipLaunchKernelGGL(layout, dim3(1), dim3(64), 0, 0, out);
  hipDeviceSynchronize();
  hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost);
  printf("layout of v_mfma_f64_4x4x4_4b_f64: A = one-hot at lane la, B = 1 + lane; 'd<-b' = D lane d received B lane b\n");
  int bad = 0;
  for (int la = 0; la < 64; ++la) {
    printf("  A lane %2d:", la);
    int n = 0;
    for (int d = 0; d < 64; ++d) {
      const double v = h[la * 64 + d];
      if (v != 0.0) { printf(" %d<-%d", d, (int)v - 1); ++n; }
      // assumed: A lane la = (i = la & 3, block (la >> 2) & 3, k = la >> 4); B lane = (j = l & 3, block, k = l >> 4); D lane = (j = l & 3, block, i = l >> 4)
      const int i = la & 3, blk = (la >> 2) & 3, k = la >> 4;
      const double want = ((d >> 4) == i && ((d >> 2) & 3) == blk) ? 1.0 + 16 * k + 4 * blk + (d & 3) : 0.0;
      if (v != want) ++bad;
    }
    printf("%s\n", n == 4 ? "" : "   (not four lanes)");
  }
  printf("assumed mapping  A: i = l & 3, b = (l >> 2) & 3, k = l >> 4   B: j = l & 3, b = (l >> 2) & 3, k = l >> 4   D: j = l & 3, b = (l >> 2) & 3, i = l >> 4\n");
  printf("  -> %s (%d of 4096 entries differ)\n", bad == 0 ? "CONFIRMED" : "NOT what the instruction does", bad);
  // ---- cost
  printf("cost, one wave per SIMD, 256 workgroups of 256 threads, %d groups per round:\n", GROUPS);
  const double c0 = run<0>("thin, one accumulator (dependent chain)", 0, 1, out, cyc);
  const double c1 = run<1>("thin, two alternating accumulators", 0, 1, out, cyc);
  const double c2 = run<2>("thin, four accumulators", 0, 1, out, cyc);
  const double c3 = run<3>("full 16x16x4, two alternating accumulators", 1, 0, out, cyc);
  const double c4 = run<4>("full, full, thin sharing B (1 : 2, one thin accumulator)", 2, 1, out, cyc);
  const double c5 = run<5>("full, thin sharing B (1 : 1, one thin accumulator)", 1, 1, out, cyc);
  const double c6 = run<6>("full, thin, thin sharing B (two thin accumulators)", 1, 2, out, cyc);
  printf("cycles per thin instruction: chain %.1f | two accumulators %.1f | four %.1f | full instruction %.1f\n", c0, c1, c2, c3);
  printf("interleaved cost of a thin instruction (group - full instructions): 1:2 %.1f | 1:1 %.1f | 1 full + 2 thin %.1f each\n",
         c4 - 2 * c3, c5 - c3, (c6 - c3) / 2);
  return 0;
}
