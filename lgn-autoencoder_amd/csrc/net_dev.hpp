// lgn-autoencoder_amd/csrc/net_dev.hpp -- device code shared by net_kernels.hip (the O(N)-per-jet network ends) and the level
// kernels that carry one of those ends in their own launch: operand staging, block sums, and the decoder output + Chamfer
// loss of a jet (forward and backward), which is either a kernel of its own or the tail of the decoder's last level forward.
#pragma once
#include "common.hpp"

namespace lgn {

constexpr double NET_RSQRT2 = 0.70710678118654752440084436210484903928;

// gradient of cart_from_canon: G_c1 = h G_px - i h G_py, G_c3 = -h G_px - i h G_py
__device__ __forceinline__ void cart_from_canon_bwd(const cx<double> (&g)[4], cx<double> (&gc)[4]) {
  gc[0] = g[0];
  gc[1] = {(g[1].r + g[2].i) * NET_RSQRT2, (g[1].i - g[2].r) * NET_RSQRT2};
  gc[2] = g[3];
  gc[3] = {(-g[1].r + g[2].i) * NET_RSQRT2, (-g[1].i - g[2].r) * NET_RSQRT2};
}

// block-wide sum of one value per thread (BLOCK threads); result valid on thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = group_sum<64>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}
// One operand on its way to LDS: issue() puts the first U * BLOCK elements into registers (loads only), commit() stores them
// through put(element, value) and fetches whatever lies beyond that window (large jets) with a plain loop.  A kernel issues ALL
// its operands before it commits the first one, so their HBM round trips overlap.
template <int U>
struct StageRegs {
  double r[U];
  __device__ __forceinline__ void issue(const double* __restrict__ src, int total) {
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = total > 0 ? src[min((int)threadIdx.x + u * BLOCK, total - 1)] : 0.0;   // clamped: no branch per load
  }
  template <class Put>
  __device__ __forceinline__ void commit(const double* __restrict__ src, int total, Put put) const {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((int)threadIdx.x + u * BLOCK < total) put((int)threadIdx.x + u * BLOCK, r[u]);
    for (int e = threadIdx.x + U * BLOCK; e < total; e += BLOCK) put(e, src[e]);
  }
};
__device__ __forceinline__ cx<double> cart_from_canon_m(const double* c, int m) {
  if (m == 0) return {c[0], c[4]};
  if (m == 3) return {c[2], c[6]};
  if (m == 1) return {(c[1] - c[3]) * NET_RSQRT2, (c[5] - c[7]) * NET_RSQRT2};
  return {-(c[5] + c[7]) * NET_RSQRT2, (c[1] + c[3]) * NET_RSQRT2};
}

// Jet momenta of two padded particle sets, as the reference's jet-feature MSE sums them (x.sum(-2), y.sum(-2): every row,
// padding included, no mask): js[m] = sum_i x[i][m] (threads 0..3), js[4 + m] = sum_j y[j][m] (threads 4..7), in particle
// order.  The caller synchronises before reading js.
__device__ __forceinline__ void jet_sums(const double* x, int N, const double* y, int M, double* js) {
  const int tid = threadIdx.x;
  if (tid < 8) {
    const int m = tid & 3;
    double s = 0.0;
    if (tid < 4) for (int i = 0; i < N; ++i) s += x[i * 4 + m];
    else for (int j = 0; j < M; ++j) s += y[j * 4 + m];
    js[tid] = s;
  }
}

// get_real methods of the whole step (utils/utils.py:194-207; LGN_REAL_* of include/lgn_amd.h)
enum : int { REAL_SUM = 0, REAL_RE = 1, REAL_IM = 2, REAL_MEAN = 3, REAL_NORM = 4 };
constexpr double GET_REAL_NORM_EPS = 1e-16;

// ============================================================================================
// decoder output + get_real(., method) + Chamfer loss [+ jscale * sum_mu (sum_i x_i - sum_j t_j)_mu^2: the jet-feature term],
// forward and backward in one pass per jet.  method and jscale are uniform: the branches on them cost the 'sum' path a few
// scalar instructions
//   recon [2][B][N][4]; loss_part [B]; g_v [2][B][N][C][4]; part row per jet: dWo1 [2][C]
// LDS: x [N][4] | tg [N][4] | rmin [N] | cmin [N] | gx [N][4] | ycl [N][8] | vl [N*C][8] | tmp [N*C][2] | wol [2C] | rarg, carg [N] ints
//      | js [8] (jet momenta of x and the target)
// ============================================================================================
__host__ __device__ inline size_t dec_out_loss_bytes(int N, int C) {
  return sizeof(double) * ((size_t)N * 22 + (size_t)N * C * 10 + 2 * (size_t)C + 8) + sizeof(int) * 2 * (size_t)N;
}
// One workgroup of BLOCK threads per jet; lds = dec_out_loss_bytes(N, C) bytes of (dynamic) LDS.  A kernel of its own
// (dec_output_loss_kernel), or the tail of the decoder's last level forward (level_fwd2.hip: LevelArgs::loss_wo1).
// GRAD = false (evaluation step): recon receives get_real(., method) [B][N][4] instead of the two planes, loss_part the per-jet
// terms, and nothing else is written (g_v, part unused): the forward arithmetic is the same code, so recon and loss_part are the
// training step's bits.
template <bool GRAD = true>
__device__ __forceinline__ void dec_output_loss_body(int B, int N, int C, const double* __restrict__ v,
                                                     const double* __restrict__ wo1, const double* __restrict__ target,
                                                     double loss_scale, int method, double jscale, double* recon,
                                                     double* loss_part, double* g_v, double* part, unsigned char* smem_raw) {
  double* x = reinterpret_cast<double*>(smem_raw);       // [N][4] real reconstruction get_real(re, im)
  double* tg = x + N * 4;                                // [N][4] target
  double* rmin = tg + N * 4;                             // [N]
  double* cmin = rmin + N;                               // [N]
  double* gx = cmin + N;                                 // [N][4]
  double* ycl = gx + N * 4;                              // [N][8] canonical output (re[4] | im[4])
  double* vl = ycl + N * 8;                              // [N*C][8] the last level's vectors (re[4] | im[4])
  double* tmp = vl + N * C * 8;                          // [N*C][2]
  double* wol = tmp + N * C * 2;                         // [2C]
  int* rarg = reinterpret_cast<int*>(wol + 2 * C);       // [N]
  int* carg = rarg + N;                                  // [N]
  double* js = reinterpret_cast<double*>(carg + N);      // [8] jet momenta of x (0..3) and of the target (4..7)
  __shared__ double red[4];
  const int b = blockIdx.x;
  const size_t plp = (size_t)B * N * 4, pl = (size_t)B * N * C, j4 = (size_t)b * N * 4, jc = (size_t)b * N * C;
  {
    StageRegs<4> vr, vi;
    StageRegs<1> tr, wr;
    vr.issue(v + jc * 4, N * C * 4); vi.issue(v + (pl + jc) * 4, N * C * 4); tr.issue(target + j4, N * 4); wr.issue(wo1, 2 * C);
    vr.commit(v + jc * 4, N * C * 4, [&](int e, double q) { vl[(e >> 2) * 8 + (e & 3)] = q; });
    vi.commit(v + (pl + jc) * 4, N * C * 4, [&](int e, double q) { vl[(e >> 2) * 8 + 4 + (e & 3)] = q; });
    tr.commit(target + j4, N * 4, [&](int e, double q) { tg[e] = q; });
    wr.commit(wo1, 2 * C, [&](int e, double q) { wol[e] = q; });
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N * 4; e += BLOCK) {     // (node, component): mix_to_output on the (1,1) irrep
    const int n = e >> 2, m = e & 3;
    cx<double> yc = {0, 0};
#pragma unroll 4
    for (int c = 0; c < C; ++c)
      cfma(yc, cx<double>{wol[c], wol[C + c]}, cx<double>{vl[(n * C + c) * 8 + m], vl[(n * C + c) * 8 + 4 + m]});
    ycl[n * 8 + m] = yc.r;
    ycl[n * 8 + 4 + m] = yc.i;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N * 4; e += BLOCK) {
    const cx<double> pc = cart_from_canon_m(ycl + (e >> 2) * 8, e & 3);
    if (GRAD) {
      recon[j4 + e] = pc.r;
      recon[plp + j4 + e] = pc.i;
    }
    double xe;                                           // get_real(., method)
    if (method == REAL_SUM) xe = pc.r + pc.i;
    else if (method == REAL_RE) xe = pc.r;
    else if (method == REAL_IM) xe = pc.i;
    else if (method == REAL_MEAN) xe = (pc.r + pc.i) / 2;
    else xe = sqrt(pc.r * pc.r + pc.i * pc.i + GET_REAL_NORM_EPS);
    x[e] = xe;
    if (!GRAD) recon[j4 + e] = xe;
  }
  __syncthreads();
  if (jscale != 0.0) jet_sums(x, N, tg, N, js);          // (read after the block sum below: it synchronises)
  // squared Euclidean distances d(i,j) = |t_j - x_i|^2; row minima (over j) and column minima (over i), first occurrence:
  // four lanes per row / column scan a quarter of the range each, then meet on (distance, index)
  const int nq = (N + 3) / 4;
  for (int e = threadIdx.x; e < 8 * N; e += BLOCK) {
    const bool rowwise = (e >> 2) < N;
    const int a = rowwise ? e >> 2 : (e >> 2) - N, q = e & 3;
    double best = 0;
    int arg = 0x7fffffff;
#pragma unroll 4
    for (int o = q * nq; o < min(N, (q + 1) * nq); ++o) {
      const double* xi = x + (rowwise ? a : o) * 4;
      const double* tj = tg + (rowwise ? o : a) * 4;
      double d0 = tj[0] - xi[0], d1 = tj[1] - xi[1], d2 = tj[2] - xi[2], d3 = tj[3] - xi[3];
      double d = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
      if (arg == 0x7fffffff || d < best) { best = d; arg = o; }
    }
#pragma unroll
    for (int off = 2; off; off >>= 1) {
      const double ob = __shfl_xor(best, off, 4);
      const int oa = __shfl_xor(arg, off, 4);
      if (oa != 0x7fffffff && (arg == 0x7fffffff || ob < best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    if (q == 0) {
      if (rowwise) { rmin[a] = best; rarg[a] = arg; } else { cmin[a] = best; carg[a] = arg; }
    }
  }
  __syncthreads();
  double lsum = 0;
  for (int n = threadIdx.x; n < N; n += BLOCK) lsum += (rmin[n] + cmin[n]) * 0.5;
  lsum = block_sum(lsum, red);
  if (threadIdx.x == 0) {
    if (jscale != 0.0)
      for (int m = 0; m < 4; ++m) { const double dj = js[m] - js[4 + m]; lsum += dj * dj * jscale; }
    loss_part[b] = lsum;
  }
  if constexpr (!GRAD) return;
  // d loss / d x_i = (x_i - t_{j*(i)}) + sum_{j : i*(j) = i} (x_i - t_j)      (two lanes per (i, component): a half of the j range each)
  const int nh = (N + 1) / 2;
  for (int e = threadIdx.x; e < N * 8; e += BLOCK) {
    const int im = e >> 1, h = e & 1, i = im >> 2, m = im & 3;
    const double xi = x[im];
    double g = h ? 0.0 : xi - tg[rarg[i] * 4 + m];
#pragma unroll 5
    for (int j = h * nh; j < min(N, (h + 1) * nh); ++j) g += carg[j] == i ? xi - tg[j * 4 + m] : 0.0;
    g += __shfl_xor(g, 1, 2);
    if (jscale != 0.0) g += h ? 0.0 : 2.0 * jscale * (js[m] - js[4 + m]);
    if (h == 0) gx[im] = g * loss_scale;
  }
  __syncthreads();
  // back through get_real (the planes' gradients: gx, 0 / 0, gx / gx, gx / gx/2, gx/2 / gx re/x, gx im/x), rep_to_p and
  // mix_to_output; dWo1[c] = sum_n sum_m G_yc[n][m] conj(v[n][c][m])
  for (int e = threadIdx.x; e < N * C; e += BLOCK) {
    const int n = e / C, c = e - n * C;
    cx<double> g[4], gc[4], d = {0, 0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double q = gx[n * 4 + m];
      if (method == REAL_SUM) g[m] = {q, q};
      else if (method == REAL_RE) g[m] = {q, 0.0};
      else if (method == REAL_IM) g[m] = {0.0, q};
      else if (method == REAL_MEAN) g[m] = {q / 2, q / 2};
      else {                                             // re / im again from the canonical output, still in LDS
        const cx<double> pc = cart_from_canon_m(ycl + n * 8, m);
        const double r = q / x[n * 4 + m];
        g[m] = {r * pc.r, r * pc.i};
      }
    }
    cart_from_canon_bwd(g, gc);
    const cx<double> w = {wol[c], wol[C + c]};
    const size_t base = jc + e;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      cx<double> r = cmulc(gc[m], w);
      g_v[base * 4 + m] = r.r;
      g_v[pl * 4 + base * 4 + m] = r.i;
      cfmac(d, gc[m], cx<double>{vl[e * 8 + m], vl[e * 8 + 4 + m]});
    }
    tmp[e * 2] = d.r;
    tmp[e * 2 + 1] = d.i;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * C) {
    const int k = threadIdx.x / C, c = threadIdx.x - k * C;
    double acc = 0.0;
#pragma unroll 6
    for (int n = 0; n < N; ++n) acc += tmp[(n * C + c) * 2 + k];
    part[(size_t)b * 2 * C + k * C + c] = acc;
  }
}

// The output mix, get_real and their backward as stages of their own, for the per-jet loss kernels that are not Chamfer's
// (assign_loss.hip).  The same statements as in dec_output_loss_body above, which stays one piece: the level kernels that carry it as
// their tail keep their code and register counts.  THE TWO COPIES MUST CHANGE TOGETHER: the forward copy is pinned against the original by
// the bit-for-bit reconstruction test, the backward copy by the gradient tests of both losses against the same oracle.  The LDS blocks they work on (each caller carves its own layout around them):
struct DecOutLds {
  double *x, *tg, *gx, *ycl, *vl, *tmp, *wol;    // [N][4] get_real(re, im) | [N][4] target | [N][4] d loss / d x | [N][8] | [N*C][8] | [N*C][2] | [2C]
};
// mix_to_output on the last level's vectors -> Cartesian -> get_real(., method): stages v, the target and Wo1, leaves x and tg in LDS
// (synchronised).  GRAD: recon [2][B][N][4] receives the two planes; else recon [B][N][4] receives x.
template <bool GRAD>
__device__ __forceinline__ void dec_out_forward(int B, int N, int C, const double* __restrict__ v, const double* __restrict__ wo1,
                                                const double* __restrict__ target, int method, double* recon, const DecOutLds& s) {
  double *x = s.x, *tg = s.tg, *ycl = s.ycl, *vl = s.vl, *wol = s.wol;
  const int b = blockIdx.x;
  const size_t plp = (size_t)B * N * 4, pl = (size_t)B * N * C, j4 = (size_t)b * N * 4, jc = (size_t)b * N * C;
  {
    StageRegs<4> vr, vi;
    StageRegs<1> tr, wr;
    vr.issue(v + jc * 4, N * C * 4); vi.issue(v + (pl + jc) * 4, N * C * 4); tr.issue(target + j4, N * 4); wr.issue(wo1, 2 * C);
    vr.commit(v + jc * 4, N * C * 4, [&](int e, double q) { vl[(e >> 2) * 8 + (e & 3)] = q; });
    vi.commit(v + (pl + jc) * 4, N * C * 4, [&](int e, double q) { vl[(e >> 2) * 8 + 4 + (e & 3)] = q; });
    tr.commit(target + j4, N * 4, [&](int e, double q) { tg[e] = q; });
    wr.commit(wo1, 2 * C, [&](int e, double q) { wol[e] = q; });
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N * 4; e += BLOCK) {     // (node, component): mix_to_output on the (1,1) irrep
    const int n = e >> 2, m = e & 3;
    cx<double> yc = {0, 0};
#pragma unroll 4
    for (int c = 0; c < C; ++c)
      cfma(yc, cx<double>{wol[c], wol[C + c]}, cx<double>{vl[(n * C + c) * 8 + m], vl[(n * C + c) * 8 + 4 + m]});
    ycl[n * 8 + m] = yc.r;
    ycl[n * 8 + 4 + m] = yc.i;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N * 4; e += BLOCK) {
    const cx<double> pc = cart_from_canon_m(ycl + (e >> 2) * 8, e & 3);
    if (GRAD) {
      recon[j4 + e] = pc.r;
      recon[plp + j4 + e] = pc.i;
    }
    double xe;                                           // get_real(., method)
    if (method == REAL_SUM) xe = pc.r + pc.i;
    else if (method == REAL_RE) xe = pc.r;
    else if (method == REAL_IM) xe = pc.i;
    else if (method == REAL_MEAN) xe = (pc.r + pc.i) / 2;
    else xe = sqrt(pc.r * pc.r + pc.i * pc.i + GET_REAL_NORM_EPS);
    x[e] = xe;
    if (!GRAD) recon[j4 + e] = xe;
  }
  __syncthreads();
}
// gx [N][4] = d loss / d x (in LDS, synchronised) -> g_v [2][B][N][C][4] and the jet's dWo1 partial row [2][C].  ACC: both are added to
// what another loss stage of the same jet left there (the hybrid loss: Chamfer first, then the EMD stage of emd_loss.hip) -- a plain
// read-modify-write by the thread that owns the element, so the sum has one order.
template <bool ACC = false>
__device__ __forceinline__ void dec_out_backward(int B, int N, int C, int method, double* g_v, double* part, const DecOutLds& s) {
  double *x = s.x, *gx = s.gx, *ycl = s.ycl, *vl = s.vl, *tmp = s.tmp, *wol = s.wol;
  const int b = blockIdx.x;
  const size_t pl = (size_t)B * N * C, jc = (size_t)b * N * C;
  // back through get_real (the planes' gradients: gx, 0 / 0, gx / gx, gx / gx/2, gx/2 / gx re/x, gx im/x), rep_to_p and
  // mix_to_output; dWo1[c] = sum_n sum_m G_yc[n][m] conj(v[n][c][m])
  for (int e = threadIdx.x; e < N * C; e += BLOCK) {
    const int n = e / C, c = e - n * C;
    cx<double> g[4], gc[4], d = {0, 0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double q = gx[n * 4 + m];
      if (method == REAL_SUM) g[m] = {q, q};
      else if (method == REAL_RE) g[m] = {q, 0.0};
      else if (method == REAL_IM) g[m] = {0.0, q};
      else if (method == REAL_MEAN) g[m] = {q / 2, q / 2};
      else {                                             // re / im again from the canonical output, still in LDS
        const cx<double> pc = cart_from_canon_m(ycl + n * 8, m);
        const double r = q / x[n * 4 + m];
        g[m] = {r * pc.r, r * pc.i};
      }
    }
    cart_from_canon_bwd(g, gc);
    const cx<double> w = {wol[c], wol[C + c]};
    const size_t base = jc + e;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      cx<double> r = cmulc(gc[m], w);
      if constexpr (ACC) {
        const double o_r = g_v[base * 4 + m], o_i = g_v[pl * 4 + base * 4 + m];
        g_v[base * 4 + m] = o_r + r.r;
        g_v[pl * 4 + base * 4 + m] = o_i + r.i;
      } else {
        g_v[base * 4 + m] = r.r;
        g_v[pl * 4 + base * 4 + m] = r.i;
      }
      cfmac(d, gc[m], cx<double>{vl[e * 8 + m], vl[e * 8 + 4 + m]});
    }
    tmp[e * 2] = d.r;
    tmp[e * 2 + 1] = d.i;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * C) {
    const int k = threadIdx.x / C, c = threadIdx.x - k * C;
    double acc = 0.0;
#pragma unroll 6
    for (int n = 0; n < N; ++n) acc += tmp[(n * C + c) * 2 + k];
    if constexpr (ACC) part[(size_t)b * 2 * C + k * C + c] = part[(size_t)b * 2 * C + k * C + c] + acc;
    else part[(size_t)b * 2 * C + k * C + c] = acc;
  }
}

}  // namespace lgn
