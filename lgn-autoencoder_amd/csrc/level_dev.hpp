// lgn-autoencoder_amd/csrc/level_dev.hpp -- device helpers shared by the level forward/backward kernels.
#pragma once
#include "level.hpp"

namespace lgn {

// ---- LDS carve -------------------------------------------------------------------------
// All offsets are in units of T and are multiples of 2 (16-byte aligned for fp64 b128 reads).
template <int C, bool DEC>
struct Carve {
  static constexpr int R = 4 * C;                       // radial outputs per pair: [lin][2c+z]
  static constexpr int NS = node_stride(C);             // per-node scalars in the node tile
  static constexpr int PS = DEC ? 8 : 4;                // position scalars per node
  // radial parameter block
  static constexpr int RA = 0, RB = NB, RC = 2 * NB;    // a, b, c
  static constexpr int RW = 3 * NB;                     // Wt[k][R] (k-major)
  static constexpr int RBIAS = RW + NB * R;             // bias[R]
  static constexpr int RAD_SIZE = RBIAS + R;
  __host__ __device__ static constexpr int even(int x) { return (x + 1) & ~1; }
};

// Cooperative load of one jet's node features / positions / mask into LDS.
//   nd[j*NS + c*10 + {0: s_r, 1: s_i, 2..5: v_r[m], 6..9: v_i[m]}]
//   pj[j*PS + ...]  encoder: (E,px,py,pz); decoder: q_r[4], q_i[4] (complex canonical)
// Thread t takes item t of every array FIRST -- all its global loads are issued together (clamped addresses, no branches)
// and only then written to LDS: one memory round trip for a 30-particle jet instead of one per array (a loop "load, store"
// per array serialises the round trips: the stores of one loop wait for its loads before the next loop's loads are issued).
// Items beyond the first BLOCK of an array (N C > 256) take the plain loops.
template <typename T>
struct JetRegs {
  T s[2], v[8], p[2];
  uint8_t m;
};
template <typename T, int C, bool DEC>
__device__ __forceinline__ void load_jet_issue(const T* __restrict__ s_in, const T* __restrict__ v_in, const T* __restrict__ p,
                                               const uint8_t* __restrict__ mask, int B, int N, int b, JetRegs<T>& r) {
  const int tid = threadIdx.x;
  const size_t plane_s = (size_t)B * N * C, plane_p = (size_t)B * N * 4;
  const int e = tid < N * C ? tid : 0, ep = tid < N * 4 ? tid : 0, em = tid < N ? tid : 0;
  const T* s0 = s_in + (size_t)b * N * C;
  const T* v0 = v_in + (size_t)b * N * C * 4;
  const T* p0 = p + (size_t)b * N * 4;
  r.s[0] = s0[e];
  r.s[1] = s0[plane_s + e];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    r.v[m] = v0[e * 4 + m];
    r.v[4 + m] = v0[plane_s * 4 + e * 4 + m];
  }
  r.p[0] = p0[ep];
  r.p[1] = DEC ? p0[plane_p + ep] : T(0);
  r.m = DEC ? uint8_t(0) : mask[(size_t)b * N + em];
}
template <typename T, int C, bool DEC>
__device__ __forceinline__ void load_jet_commit(const T* __restrict__ s_in, const T* __restrict__ v_in, const T* __restrict__ p,
                                                const uint8_t* __restrict__ mask, int B, int N, int b, const JetRegs<T>& r,
                                                T* nd, T* pj, uint8_t* mk) {
  using L = Carve<C, DEC>;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const size_t plane_s = (size_t)B * N * C;
  if (tid < N * C) {
    const int j = tid / C, c = tid - j * C;
    T* d = nd + j * L::NS + c * 10;
    d[0] = r.s[0];
    d[1] = r.s[1];
#pragma unroll
    for (int m = 0; m < 8; ++m) d[2 + m] = r.v[m];
  }
  if (tid < N * 4) {
    if (DEC) {
      pj[(tid >> 2) * 8 + (tid & 3)] = r.p[0];
      pj[(tid >> 2) * 8 + 4 + (tid & 3)] = r.p[1];
    } else {
      pj[tid] = r.p[0];
    }
  }
  if (!DEC && tid < N) mk[tid] = r.m;
  // remainder (jets with more than BLOCK items per array; also the second half of a 512-thread workgroup's share)
  const T* s0 = s_in + (size_t)b * N * C;
  const T* v0 = v_in + (size_t)b * N * C * 4;
  for (int e = tid + nthr; e < N * C; e += nthr) {
    int j = e / C, c = e - j * C;
    T* d = nd + j * L::NS + c * 10;
    d[0] = s0[e];
    d[1] = s0[plane_s + e];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      d[2 + m] = v0[e * 4 + m];
      d[6 + m] = v0[plane_s * 4 + e * 4 + m];
    }
  }
  const T* p0 = p + (size_t)b * N * 4;
  if (DEC) {
    const size_t plane_p = (size_t)B * N * 4;
    for (int e = tid + nthr; e < N * 4; e += nthr) {
      pj[(e >> 2) * 8 + (e & 3)] = p0[e];
      pj[(e >> 2) * 8 + 4 + (e & 3)] = p0[plane_p + e];
    }
  } else {
    for (int e = tid + nthr; e < N * 4; e += nthr) pj[e] = p0[e];
    for (int e = tid + nthr; e < N; e += nthr) mk[e] = mask[(size_t)b * N + e];
  }
}
template <typename T, int C, bool DEC>
__device__ __forceinline__ void load_jet(const T* __restrict__ s_in, const T* __restrict__ v_in,
                                         const T* __restrict__ p, const uint8_t* __restrict__ mask, int B, int N,
                                         int b, T* nd, T* pj, uint8_t* mk) {
  JetRegs<T> r;
  load_jet_issue<T, C, DEC>(s_in, v_in, p, mask, B, N, b, r);
  load_jet_commit<T, C, DEC>(s_in, v_in, p, mask, B, N, b, r, nd, pj, mk);
}

// Geometry of one ordered pair (i, j): q = canonical(p_i - p_j); encoder also the signed norm + mask.
template <typename T, bool DEC>
struct PairGeom {
  cx<T> q[4];
  T nrm;
  bool on;   // edge unmasked (encoder); decoder edges are always "masked" (radial == bias)
};

template <typename T, bool DEC>
__device__ __forceinline__ PairGeom<T, DEC> pair_geom(const T* pi, const T* pjj, bool mi, bool mj) {
  PairGeom<T, DEC> g;
  if (DEC) {
#pragma unroll
    for (int m = 0; m < 4; ++m) g.q[m] = {pi[m] - pjj[m], pi[4 + m] - pjj[4 + m]};
    g.nrm = T(0);
    g.on = false;
  } else {
    T d0 = pi[0] - pjj[0], d1 = pi[1] - pjj[1], d2 = pi[2] - pjj[2], d3 = pi[3] - pjj[3];
    T nsq;
    g.nrm = signed_norm(d0, d1, d2, d3, nsq);
    g.on = mi && mj && (g.nrm != T(0));
    const T h = rsqrt2<T>();
    g.q[0] = {d0, T(0)};
    g.q[1] = {d1 * h, -d2 * h};
    g.q[2] = {d3, T(0)};
    g.q[3] = {-d1 * h, -d2 * h};
  }
  return g;
}

// <a, b> * 2 = a0 b0 + a1 b3 - a2 b2 + a3 b1  (the 1/2 of the CG coefficient is applied by the caller)
template <typename T>
__device__ __forceinline__ cx<T> bil2(const cx<T> (&a)[4], const cx<T> (&b)[4]) {
  cx<T> r = cmul(a[0], b[0]);
  cfma(r, a[1], b[3]);
  cx<T> t = cmul(a[2], b[2]);
  r.r -= t.r;
  r.i -= t.i;
  cfma(r, a[3], b[1]);
  return r;
}

// One row of the separable decoder aggregate (level_fwd2.hip: SEP), one channel of one node:
//   A4 = S e0            A1[m] = VS[m] e0            e0 = R0 (1 + i), R0 = b0 (1 + i)
//   A3 = R1 (<VS, p> - VP) / 2        A2[m] = R1 (p[m] S - SP[m])        R1 = b1 (1 + i)
// from the channel's jet sums sm = S | VS[4] | SP[4] | VP and the node's centred momentum pn = re[4] | im[4].  The forward computes the
// row and the backward computes it AGAIN instead of reading it back (LevelArgs::sep_sums), so the two must agree bit for bit, and the
// forward's s_out / v_out are pinned: every multiply-add is spelled out, as in tail_dev.hpp, in the form the forward compiled to when
// the products were written with * and + (which of a complex product's two terms went into the fused multiply-add differed from
// product to product: the imaginary parts below are not all the same shape on purpose).  NOS: no A3 / A4 (a3h, a4 unset).
struct SepRow {
  cx<double> a3h, a4, a1[4], a2[4];       // a3h = A3 with the CG coefficient 1/2 applied
};
template <bool NOS>
__device__ __forceinline__ SepRow dec_sep_row(const double* sm, const double* pn, double b0, double b1) {
#pragma clang fp contract(off)
  const cx<double> e0 = {b0 - b0, b0 + b0};
  const cx<double> S = {sm[0], sm[1]};
  cx<double> VS[4], pc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    VS[m] = {sm[2 + 2 * m], sm[3 + 2 * m]};
    pc[m] = {pn[m], pn[4 + m]};
  }
  SepRow o;
  if constexpr (!NOS) {
    o.a4.r = __builtin_fma(S.r, e0.r, -(S.i * e0.i));
    o.a4.i = __builtin_fma(S.r, e0.i, S.i * e0.r);
    cx<double> t, u;                                            // t = 2 <VS, p> (bil2), then - VP
    t.r = __builtin_fma(VS[0].r, pc[0].r, -(VS[0].i * pc[0].i));
    t.i = __builtin_fma(VS[0].i, pc[0].r, VS[0].r * pc[0].i);
    cfma(t, VS[1], pc[3]);
    u.r = __builtin_fma(VS[2].r, pc[2].r, -(VS[2].i * pc[2].i));
    u.i = __builtin_fma(VS[2].i, pc[2].r, VS[2].r * pc[2].i);
    t.r -= u.r;  t.i -= u.i;
    cfma(t, VS[3], pc[1]);
    t.r -= sm[18];  t.i -= sm[19];
    const double w = b1 * t.i;
    o.a3h.r = 0.5 * __builtin_fma(b1, t.r, -w);
    o.a3h.i = 0.5 * __builtin_fma(b1, t.r, w);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    o.a1[m].r = __builtin_fma(VS[m].r, e0.r, -(VS[m].i * e0.i));
    o.a1[m].i = __builtin_fma(VS[m].r, e0.i, VS[m].i * e0.r);
    cx<double> u;
    u.r = __builtin_fma(pc[m].r, S.r, -(pc[m].i * S.i));
    u.i = __builtin_fma(pc[m].r, S.i, pc[m].i * S.r);
    u.r -= sm[10 + 2 * m];  u.i -= sm[11 + 2 * m];
    const double w = b1 * u.i;
    o.a2[m].r = __builtin_fma(b1, u.r, -w);
    o.a2[m].i = __builtin_fma(b1, u.r, w);
  }
  return o;
}

// metric-permuted copy: tilde(x)[m] such that <a, b> = 1/2 sum_m a[m] * tilde(b)[m]
template <typename T>
__device__ __forceinline__ void metric_perm(const cx<T> (&x)[4], cx<T> (&y)[4]) {
  y[0] = x[0];
  y[1] = x[3];
  y[2] = {-x[2].r, -x[2].i};
  y[3] = x[1];
}

// Five reciprocals for the price of one: 1 / u_s from the reciprocal of the product (prefix products up, suffix products down).
// The five Lorentzian bells of a lane are 1 / (1 + c_s^2 |n|^2 + 1e-16), u_s >= 1 and far from overflow in the product; v_rcp_f64
// runs at a quarter of the fp64 rate and each refined reciprocal is 32 cycles of the datapath the pair sweeps are bound by:
// 5 x 32 -> 32 + 12 multiplies = 80 cycles per lane and tile.  Each result carries three or four roundings instead of one (a few
// 1e-16 relative).  A product that leaves the range (each u_s around 1e60: unnormalised momenta times a large c; or a NaN input)
// takes the five divisions one by one -- a branch no realistic jet enters; without it the overflow turned five values that
// should be ~0 into NaN (inf * 0 in the Newton step).
__device__ __forceinline__ void rcp5(const double (&u)[5], double (&r)[5]) {
  const double p1 = u[0] * u[1], p2 = p1 * u[2], p3 = p2 * u[3], p4 = p3 * u[4];
  if (__builtin_expect(!(p4 < 0x1p+1000), 0)) {
#pragma unroll
    for (int s = 0; s < 5; ++s) r[s] = 1.0 / u[s];
    return;
  }
  double t = __builtin_amdgcn_rcp(p4);
  double e = __builtin_fma(-p4, t, 1.0);
  t = __builtin_fma(t, e, t);
  e = __builtin_fma(-p4, t, 1.0);
  t = __builtin_fma(t, e, t);                  // 1 / (u0 u1 u2 u3 u4)
  r[4] = t * p3;  t *= u[4];                   // t = 1 / (u0 .. u3)
  r[3] = t * p2;  t *= u[3];
  r[2] = t * p1;  t *= u[2];                   // t = 1 / (u0 u1)
  r[1] = t * u[0];
  r[0] = t * u[1];
}

}  // namespace lgn
