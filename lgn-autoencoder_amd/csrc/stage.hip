// lgn-autoencoder_amd/csrc/stage.hip -- staging of a batch into a step's static input buffers in one launch, with the reference's
// per-jet --normalize (utils/normalize_p4.py, utils/train.py:281-297), and the de-normalisation of reconstruction and target that
// validate() / test.py collect.
//
// stage_batch_kernel: one wavefront per jet, four jets per workgroup, lanes stride the particles; a row is 32 B = two 16-byte
// vectors.  No LDS: the reductions (the jet's factor, the jet node of jet_features) run over wave shuffles.
//   pass 1   per-lane max_i |p_i^mu| (NaN kept, as torch.amax keeps it: fmax would drop it) and sum_i E_i in row order, then the
//            butterflies -> the jet's factor (+ 1e-16, added, not clamped: an all-zero jet has factor 1e-16 and stays zero)
//   pass 2   target = p / factor, p4_in = target * scale, mask (labels, else target[.., 0] != 0: the reference's encoder sees the
//            normalised batch), per-lane sums of p4_in in row order for the jet node
//   pass 3   (jet_features) the jet node, the scalar normsq4(sum over all N + 1 nodes) in column 0 of in_scalars, data['scalars']
// Jets b >= B (the all-masked padding jets of a short batch) are written as zeros in every output.
//
// Device-resident epochs: stage_gather_kernel is the same staging with each row's jet picked by index from a resident dataset at a
// cursor kept on the device, epoch_collect_kernel the bookkeeping behind the step (loss sum, step count, collected rows, cursor
// advance), epoch_reset_kernel their state's clear -- [gather | step | collect] is one linear graph, replayed once per batch.
// stage_gather_at_kernel and epoch_collect_planes_kernel are the two with a base row (a second plan of another batch size replayed
// behind the first: the short last batch of a training epoch) and with tensors of several planes, [planes][B][rd] (the latent); they
// run the device code of the first two -- stage_jet and gather_jet, LGN_COLLECT_RUN and collect_arrive.
//
// Contraction is off: p / f * scale, the products of normsq4 and the sums round one operation at a time, as torch's do.
#pragma clang fp contract(off)

#include <algorithm>

#include "common.hpp"
#include "../../include/lgn_amd.h"
#include "ops.hpp"
#include "wave_sum.hpp"

namespace lgn {
namespace {

constexpr double NORM_EPS = 1e-16;     // EPS of utils/normalize_p4.py
constexpr int STAGE_WAVES = 4;

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct StageArgs {
  const double* p4;          // [B][N][4]
  const uint8_t* labels;     // [B][N] or null
  const double* scalars;     // [B][Nn][K] or null (K == 0)
  int B, B_pad, N, method, jet, K;
  double scale;
  double* p4_in;             // [B_pad][Nn][4]   Nn = N + jet
  double* target;            // [B_pad][N][4]    (may be p4_in: scale == 1, no jet node)
  uint8_t* mask;             // [B_pad][Nn]
  double* in_scalars;        // [B_pad][Nn][jet + K] or null
  double* factor;            // [B_pad][4]
};

// One jet by one wavefront: batch row b of every output from jet `src` of the sources; src < 0 is a padding jet.  The body of both
// staging kernels -- they differ in where a row's jet comes from, nothing else.
__device__ __forceinline__ void stage_jet(const StageArgs& a, const long b, const long src_jet, const int lane) {
  const int N = a.N, Nn = N + a.jet, S = a.jet + a.K;
  dbl2* __restrict__ tg = reinterpret_cast<dbl2*>(a.target + (size_t)b * N * 4);
  dbl2* __restrict__ pin = reinterpret_cast<dbl2*>(a.p4_in + (size_t)b * Nn * 4);
  uint8_t* __restrict__ mk = a.mask + (size_t)b * Nn;
  double* __restrict__ sc = a.in_scalars ? a.in_scalars + (size_t)b * Nn * S : nullptr;
  const bool aliased = a.p4_in == a.target;
  const dbl2 zero2 = {0.0, 0.0};

  if (src_jet < 0) {                   // padding jet: zeros everywhere
    for (int i = lane; i < N; i += 64) { tg[2 * i] = zero2; tg[2 * i + 1] = zero2; }
    if (!aliased)
      for (int i = lane; i < Nn; i += 64) { pin[2 * i] = zero2; pin[2 * i + 1] = zero2; }
    for (int i = lane; i < Nn; i += 64) mk[i] = 0;
    if (sc)
      for (int e = lane; e < Nn * S; e += 64) sc[e] = 0.0;
    if (lane < 2) reinterpret_cast<dbl2*>(a.factor + (size_t)b * 4)[lane] = zero2;
    return;
  }

  const dbl2* __restrict__ src = reinterpret_cast<const dbl2*>(a.p4 + (size_t)src_jet * N * 4);
  // ---- pass 1: the factor
  double f[4] = {1.0, 1.0, 1.0, 1.0};
  if (a.method != LGN_NORM_NONE) {
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, e = 0.0;
    for (int i = lane; i < N; i += 64) {
      const dbl2 lo = src[2 * i], hi = src[2 * i + 1];
      m0 = nan_max(m0, fabs(lo.x)); m1 = nan_max(m1, fabs(lo.y));
      m2 = nan_max(m2, fabs(hi.x)); m3 = nan_max(m3, fabs(hi.y));
      e += lo.x;
    }
    if (a.method == LGN_NORM_JET_E) {
      const double v[8] = {e, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      double s[8];
      wave_allsum<8>(v, s, lane);
      f[0] = f[1] = f[2] = f[3] = s[0] + NORM_EPS;
    } else if (a.method == LGN_NORM_OVERALL_MAX) {
      const double m = wave_nan_max(nan_max(nan_max(m0, m1), nan_max(m2, m3)));
      f[0] = f[1] = f[2] = f[3] = m + NORM_EPS;
    } else {
      f[0] = wave_nan_max(m0) + NORM_EPS; f[1] = wave_nan_max(m1) + NORM_EPS;
      f[2] = wave_nan_max(m2) + NORM_EPS; f[3] = wave_nan_max(m3) + NORM_EPS;
    }
  }
  if (lane < 2) {
    const dbl2 fv = {lane ? f[2] : f[0], lane ? f[3] : f[1]};       // (no run-time index: the array stays in registers)
    reinterpret_cast<dbl2*>(a.factor + (size_t)b * 4)[lane] = fv;
  }

  // ---- pass 2: target, encoder input, mask; per-lane sums of the encoder input in row order
  const uint8_t* __restrict__ lab = a.labels ? a.labels + (size_t)src_jet * N : nullptr;
  double j[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < N; i += 64) {
    const dbl2 lo = src[2 * i], hi = src[2 * i + 1];
    const dbl2 tlo = {lo.x / f[0], lo.y / f[1]}, thi = {hi.x / f[2], hi.y / f[3]};
    const dbl2 qlo = {tlo.x * a.scale, tlo.y * a.scale}, qhi = {thi.x * a.scale, thi.y * a.scale};
    tg[2 * i] = tlo; tg[2 * i + 1] = thi;
    if (!aliased) { pin[2 * i] = qlo; pin[2 * i + 1] = qhi; }
    mk[i] = lab ? lab[i] : (uint8_t)(tlo.x != 0.0);
    j[0] += qlo.x; j[1] += qlo.y; j[2] += qhi.x; j[3] += qhi.y;
  }

  // ---- pass 3: jet node, jet-mass scalar, data['scalars']  (Encoder._prepare_input)
  if (a.jet) {
    double s[8];
    wave_allsum<8>(j, s, lane);
    if (lane < 2) {
      const dbl2 jv = {lane ? s[2] : s[0], lane ? s[3] : s[1]};
      pin[2 * N + lane] = jv;
    }
    if (lane == 0) mk[N] = 1;
    // normsq4 of the sum over ALL N + 1 nodes = particles + jet node: twice the jet (lgn_encoder.py:377-390), 2 E^2 - sum p^2
    const double t0 = s[0] + s[0], t1 = s[1] + s[1], t2 = s[2] + s[2], t3 = s[3] + s[3];
    const double q0 = t0 * t0, q1 = t1 * t1, q2 = t2 * t2, q3 = t3 * t3;
    const double mass = 2.0 * q0 - (((q0 + q1) + q2) + q3);
    for (int i = lane; i < Nn; i += 64) sc[(size_t)i * S] = mass;
  }
  if (a.K > 0) {
    const double* __restrict__ xs = a.scalars + (size_t)src_jet * Nn * a.K;
    for (int e = lane; e < Nn * a.K; e += 64) {
      const int i = e / a.K, k = e - i * a.K;
      sc[(size_t)i * S + a.jet + k] = xs[e];
    }
  }
}

__global__ __launch_bounds__(64 * STAGE_WAVES) void stage_batch_kernel(const StageArgs a) {
  const long b = (long)blockIdx.x * STAGE_WAVES + (threadIdx.x >> 6);
  if (b >= a.B_pad) return;            // whole waves leave; nothing below waits on the workgroup
  stage_jet(a, b, b < a.B ? b : -1, threadIdx.x & 63);
}

// The same staging with the jet of row b taken from a resident dataset: index[cursor * B_pad + b], the cursor read from the device
// (an epoch replays ONE graph: nothing of a step's position may be a kernel argument).  Rows at or behind `count` are padding jets;
// so is a row whose index lies outside [0, M) -- no address is formed from it -- and lane 0 then stores LGN_EPOCH_BAD_INDEX.
struct GatherArgs {
  const int* index;          // [count]
  const long long* cursor;   // [0]: batches done in this epoch
  long long count, M;
  int* status;
};

// The jet at position pos of the epoch's order (pos >= count: a padding jet), with the check of its index -- the lookup of both
// gather kernels.
__device__ __forceinline__ long gather_jet(const GatherArgs& g, const long long pos, const int lane) {
  long src_jet = -1;
  if (pos < g.count) {
    const long long j = g.index[pos];
    if (j >= 0 && j < g.M) src_jet = (long)j;
    else if (lane == 0) g.status[0] = LGN_EPOCH_BAD_INDEX;      // (every wave that stores, stores the same word)
  }
  return src_jet;
}

__global__ __launch_bounds__(64 * STAGE_WAVES) void stage_gather_kernel(const StageArgs a, const GatherArgs g) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * STAGE_WAVES + (threadIdx.x >> 6);
  if (b >= a.B_pad) return;
  const long long c = g.cursor[0];
  // (a cursor outside the epoch -- negative, or so large that the product would wrap -- stages padding jets only)
  const long long pos = (c >= 0 && c <= g.count / a.B_pad) ? c * a.B_pad + b : g.count;
  stage_jet(a, b, gather_jet(g, pos, lane), lane);
}

// The gather of a second plan of another batch size behind the first (the short last batch of a training epoch): position
// base + cursor * B_pad + b, 0 <= base <= count.  base = 0 is the kernel above.
__global__ __launch_bounds__(64 * STAGE_WAVES) void stage_gather_at_kernel(const StageArgs a, const GatherArgs g, const long long base) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * STAGE_WAVES + (threadIdx.x >> 6);
  if (b >= a.B_pad) return;
  const long long c = g.cursor[0];
  const long long pos = (c >= 0 && c <= (g.count - base) / a.B_pad) ? base + c * a.B_pad + b : g.count;
  stage_jet(a, b, gather_jet(g, pos, lane), lane);
}

// out[b][i][mu] = x[b][i][mu] * factor[b][mu] for reconstruction and target at once: one thread per row of each tensor
__global__ __launch_bounds__(BLOCK) void denormalize_kernel(const double* __restrict__ x0, const double* __restrict__ x1,
                                                            const double* __restrict__ factor, long rows, int N,
                                                            double* __restrict__ out0, double* __restrict__ out1) {
  const long r = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= rows) return;
  const dbl2* f = reinterpret_cast<const dbl2*>(factor + (r / N) * 4);
  const dbl2 flo = f[0], fhi = f[1];
  {
    const dbl2 lo = reinterpret_cast<const dbl2*>(x0)[2 * r], hi = reinterpret_cast<const dbl2*>(x0)[2 * r + 1];
    reinterpret_cast<dbl2*>(out0)[2 * r] = lo * flo;
    reinterpret_cast<dbl2*>(out0)[2 * r + 1] = hi * fhi;
  }
  if (x1) {
    const dbl2 lo = reinterpret_cast<const dbl2*>(x1)[2 * r], hi = reinterpret_cast<const dbl2*>(x1)[2 * r + 1];
    reinterpret_cast<dbl2*>(out1)[2 * r] = lo * flo;
    reinterpret_cast<dbl2*>(out1)[2 * r + 1] = hi * fhi;
  }
}

// The epoch's bookkeeping behind a step, in the step's graph: rows b < n_valid = min(B, count - cursor * B) of up to
// LGN_EPOCH_MAX_COLLECT static [B][rd] tensors go to [count][rd] epoch buffers at jet cursor * B + b -- rows are contiguous on both
// sides, so a tensor is ONE run of n_valid * rd doubles, moved as 16-byte vectors where both ends are aligned -- then the workgroup
// that arrives LAST (a ticket in cursor[1]; every thread of every workgroup has read the cursor by then) adds the step's loss to
// epoch[0], counts the step in epoch[1], clears the ticket and advances the cursor: one thread, one fp64 add per step, in step order.
struct CollectArgs {
  const double* loss;        // the step's loss (device scalar)
  double* epoch;             // [0] sum of the losses, [1] steps
  long long* cursor;         // [0] batches done, [1] arrival ticket (0 between launches)
  long long count;
  int B, n;
  const double* src[LGN_EPOCH_MAX_COLLECT];
  double* dst[LGN_EPOCH_MAX_COLLECT];
  int rd[LGN_EPOCH_MAX_COLLECT];
};

// One run of `total` doubles from s to d by the whole grid, 16-byte vectors where both ends are aligned: the copy of both collect
// kernels.  It is a macro, not a function: as an inlined function the same statements leave epoch_collect_kernel with another order
// of its scalar address arithmetic, and that kernel's code is to stay what it was, instruction for instruction.
#define LGN_COLLECT_RUN(s, d, total, tid, nth)                                                  \
  do {                                                                                          \
    if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {        \
      const dbl2* __restrict__ s2 = reinterpret_cast<const dbl2*>(s);                           \
      dbl2* __restrict__ d2 = reinterpret_cast<dbl2*>(d);                                       \
      for (long e = tid; e < total / 2; e += nth) d2[e] = s2[e];                                \
      if ((total & 1) && tid == 0) d[total - 1] = s[total - 1];                                 \
    } else {                                                                                    \
      for (long e = tid; e < total; e += nth) d[e] = s[e];                                      \
    }                                                                                           \
  } while (0)

// The arrival ticket of both collect kernels: the last workgroup to arrive books the step and advances the cursor from c.
__device__ __forceinline__ void collect_arrive(const CollectArgs& a, const long long c) {
  __syncthreads();                     // every thread of this workgroup has read the cursor
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(a.cursor + 1), 1ULL);
    if (t == gridDim.x - 1) {          // the last workgroup to arrive: nobody reads the cursor any more
      a.cursor[1] = 0;
      a.epoch[0] += a.loss[0];
      a.epoch[1] += 1.0;
      a.cursor[0] = c + 1;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void epoch_collect_kernel(const CollectArgs a) {
  const long long c = a.cursor[0];
  long long n_valid = 0;
  if (c >= 0 && c <= a.count / a.B) n_valid = a.count - c * a.B < a.B ? a.count - c * a.B : a.B;
  const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nth = (long)gridDim.x * BLOCK;
  for (int k = 0; k < a.n && n_valid > 0; ++k) {
    const double* __restrict__ s = a.src[k];
    double* __restrict__ d = a.dst[k] + c * a.B * a.rd[k];
    const long total = (long)n_valid * a.rd[k];
    LGN_COLLECT_RUN(s, d, total, tid, nth);
  }
  collect_arrive(a, c);
}

// The same bookkeeping for tensors whose batch axis is the SECOND one (the latent, [2][B][rd]) and for a second plan behind the
// first: source k is [planes[k]][B][rd], its destination [planes[k]][count][rd], a plane ONE run of n_valid * rd doubles at row
// row0 = base + cursor * B with n_valid = min(B, count - row0).  planes = 1 and base = 0 is the kernel above.
struct PlaneArgs {
  long long base;
  int planes[LGN_EPOCH_MAX_COLLECT];
};

__global__ __launch_bounds__(BLOCK) void epoch_collect_planes_kernel(const CollectArgs a, const PlaneArgs p) {
  const long long c = a.cursor[0];
  long long n_valid = 0, row0 = 0;
  if (c >= 0 && c <= (a.count - p.base) / a.B) {       // (so that row0 <= count, whatever the cursor holds)
    row0 = p.base + c * a.B;
    n_valid = a.count - row0 < a.B ? a.count - row0 : a.B;
  }
  const long tid = (long)blockIdx.x * BLOCK + threadIdx.x, nth = (long)gridDim.x * BLOCK;
  for (int k = 0; k < a.n && n_valid > 0; ++k)
    for (int q = 0; q < p.planes[k]; ++q) {
      const double* __restrict__ s = a.src[k] + (long long)q * a.B * a.rd[k];
      double* __restrict__ d = a.dst[k] + ((long long)q * a.count + row0) * a.rd[k];
      const long total = (long)n_valid * a.rd[k];
      LGN_COLLECT_RUN(s, d, total, tid, nth);
    }
  collect_arrive(a, c);
}

#undef LGN_COLLECT_RUN

__global__ void epoch_reset_kernel(long long* cursor, double* epoch, int* status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cursor[0] = 0; cursor[1] = 0;
    epoch[0] = 0.0; epoch[1] = 0.0;
    status[0] = 0;
  }
}

}  // namespace

int stage_batch(const double* p4, const uint8_t* labels, const double* scalars, int B, int B_pad, int N, int method, double scale,
                int jet_features, int K, double* p4_in, double* target, uint8_t* mask, double* in_scalars, double* factor,
                hipStream_t st) {
  const StageArgs a{p4, labels, scalars, B, B_pad, N, method, jet_features ? 1 : 0, K, scale, p4_in, target, mask, in_scalars, factor};
  stage_batch_kernel<<<cdiv(B_pad, STAGE_WAVES), 64 * STAGE_WAVES, 0, st>>>(a);
  LGN_CHECK_LAUNCH();
  return 0;
}

int denormalize(const double* x0, const double* x1, const double* factor, int B, int N, double* out0, double* out1, hipStream_t st) {
  const long rows = (long)B * N;
  denormalize_kernel<<<(unsigned)((rows + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>(x0, x1, factor, rows, N, out0, out1);
  LGN_CHECK_LAUNCH();
  return 0;
}

int stage_gather(const double* p4, const uint8_t* labels, const double* scalars, long long M, const int* index, long long count,
                 const long long* cursor, int B_pad, int N, int method, double scale, int jet_features, int K, double* p4_in,
                 double* target, uint8_t* mask, double* in_scalars, double* factor, int* status, hipStream_t st) {
  const StageArgs a{p4, labels, scalars, B_pad, B_pad, N, method, jet_features ? 1 : 0, K, scale, p4_in, target, mask, in_scalars, factor};
  const GatherArgs g{index, cursor, count, M, status};
  stage_gather_kernel<<<cdiv(B_pad, STAGE_WAVES), 64 * STAGE_WAVES, 0, st>>>(a, g);
  LGN_CHECK_LAUNCH();
  return 0;
}

int epoch_collect(const double* loss, double* epoch, long long* cursor, long long count, int B, int n, const double* const* src,
                  double* const* dst, const int* row_doubles, hipStream_t st) {
  CollectArgs a{loss, epoch, cursor, count, B, n, {}, {}, {}};
  long most = 0;
  for (int k = 0; k < n; ++k) {
    a.src[k] = src[k]; a.dst[k] = dst[k]; a.rd[k] = row_doubles[k];
    most = std::max(most, (long)B * row_doubles[k]);
  }
  // a thread moves about four 16-byte vectors of the largest tensor; a few workgroups saturate what a step's outputs need
  const long blocks = std::min<long>(std::max<long>((most / 2 + 4 * BLOCK - 1) / (4 * BLOCK), 1), 64);
  epoch_collect_kernel<<<(unsigned)blocks, BLOCK, 0, st>>>(a);
  LGN_CHECK_LAUNCH();
  return 0;
}

int stage_gather_at(const double* p4, const uint8_t* labels, const double* scalars, long long M, const int* index, long long count,
                    long long base, const long long* cursor, int B_pad, int N, int method, double scale, int jet_features, int K,
                    double* p4_in, double* target, uint8_t* mask, double* in_scalars, double* factor, int* status, hipStream_t st) {
  const StageArgs a{p4, labels, scalars, B_pad, B_pad, N, method, jet_features ? 1 : 0, K, scale, p4_in, target, mask, in_scalars, factor};
  const GatherArgs g{index, cursor, count, M, status};
  stage_gather_at_kernel<<<cdiv(B_pad, STAGE_WAVES), 64 * STAGE_WAVES, 0, st>>>(a, g, base);
  LGN_CHECK_LAUNCH();
  return 0;
}

int epoch_collect_planes(const double* loss, double* epoch, long long* cursor, long long count, long long base, int B, int n,
                         const double* const* src, double* const* dst, const int* row_doubles, const int* planes, hipStream_t st) {
  CollectArgs a{loss, epoch, cursor, count, B, n, {}, {}, {}};
  PlaneArgs p{base, {}};
  long most = 0;
  for (int k = 0; k < n; ++k) {
    a.src[k] = src[k]; a.dst[k] = dst[k]; a.rd[k] = row_doubles[k]; p.planes[k] = planes[k];
    most = std::max(most, (long)B * row_doubles[k] * planes[k]);
  }
  // (the grid of epoch_collect, sized by the largest tensor over all its planes)
  const long blocks = std::min<long>(std::max<long>((most / 2 + 4 * BLOCK - 1) / (4 * BLOCK), 1), 64);
  epoch_collect_planes_kernel<<<(unsigned)blocks, BLOCK, 0, st>>>(a, p);
  LGN_CHECK_LAUNCH();
  return 0;
}

int epoch_reset(long long* cursor, double* epoch, int* status, hipStream_t st) {
  epoch_reset_kernel<<<1, 64, 0, st>>>(cursor, epoch, status);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // namespace lgn
