// lgn-autoencoder_amd/csrc/pair_dev.hpp -- the pair sweep of the message-passing levels, each piece once.
//
// Mapping shared by every kernel that includes this: a wave owns a group of 4 particles and sweeps the other index in tiles of 4;
// lane = (pair slot pr = lane & 15, channel in group cg = lane >> 4); the radial Linear layers and the radial-parameter GEMM run on
// v_mfma_f64_16x16x4_f64.  The kernels keep their control flow (group ownership, chunking, pipelining, receiver split, barriers and
// stamps); what a pair, a tile or an epilogue computes is here:
//
//   RadLane / BellRow        per-lane constants of the radial network in matrix-core fragment form
//   enc_pair                 geometry of an encoder pair
//   radial_masked            the radial network of a tile, reciprocals by rcp5 under the EXEC mask      } two forms that differ in the
//   radial_select, rho_select  the same with fast_rcp, "+ 1e-16" and selects                            } last bits: see below
//   rad_b_rows, rad_a_rows, rad_gemm_step, rad_rows_store, rad_rows_sum
//                            the [4C x pairs] . [pairs x 42] radial-parameter GEMM: T1 | T2 | S | dB of one jet
//   AggGrad, SrcFeat, edge_P2, edge_V, enc_edge_rad
//                            the radial gradient of one encoder edge (pair, channel); what is NOT shared of the edge backward, and why
//   dec_bias_store, dec_bias_sum   the decoder's bias-gradient epilogue
//
// Everything a piece branches on is a template argument; none of them stamps.
#pragma once
#include "level_dev.hpp"

namespace lgn {

// ---- layouts and sizes ------------------------------------------------------------------------------------------------------
// One row of the gradient of the aggregate, per receiver: A3 | A4 (scalars, 2C each) | A1 | A2 (vectors, 8C each).  PAD doubles of
// row padding: level_bwd3 keeps the whole jet's rows in LDS and reads four nodes' rows at once -- rows of 20 C doubles put every
// second node of C = 4 on the same banks, + 2 does not; the rows that travel through global memory (g_ag) are unpadded.
template <int C, int PAD = 0>
struct GARow {
  static constexpr int A3 = 0, A4 = 2 * C, A1 = 4 * C, A2 = 12 * C, SIZE = 20 * C + PAD;
};

constexpr int PAIR_TS = 18;                                // padded row stride of the 16 x 16 transpose tiles (doubles)
// transpose tiles of one wave: NG tiles of dL/d rad (A operand) and three of basis columns (B operand) ...
__host__ __device__ constexpr int pair_tiles(int NG) { return (NG + 3) * 16 * PAIR_TS; }
// ... and what a wave needs of the region they live in: after the sweep it holds the wave's 64 x 12 NG accumulator rows
__host__ __device__ constexpr int pair_scratch(int NG) { return pair_tiles(NG) > 64 * NG * 12 ? pair_tiles(NG) : 64 * NG * 12; }

// ---- per-lane constants of the radial network -------------------------------------------------------------------------------
// Bells: basis function k = 4 s + cg of this lane, beta_k = a_k + b_k / (1 + c_k^2 |n|^2).  Linear: A fragments
// wf[g][s] = W'[r' = lane & 15][k = 4 s + cg] of channel group g (row r' = channel in group + 4 q, q = 2 lin + z) and the
// accumulator's initial value bias[g][q] of this lane's channel.  Decoder: the edge mask is identically zero, the radial values
// are the biases (both planes of a channel carry the same real bias), nothing else is loaded.
template <int C, bool DEC>
struct RadLane {
  static constexpr int NG = (C + 3) / 4;
  double ak[5], bk[5], ck2[5], wf[NG][5], bias[NG][4];
  __device__ __forceinline__ void load_bells(const double* ra, const double* rb, const double* rc, int lane) {
    const int cg = lane >> 4;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int k = 4 * s + cg;
      ak[s] = ra[k];
      bk[s] = rb[k];
      const double c = rc[k];
      ck2[s] = c * c;
    }
  }
  __device__ __forceinline__ void load(const double* ra, const double* rb, const double* rc, const double* w0, const double* b0,
                                       const double* w1, const double* b1, int lane) {
    const int cg = lane >> 4;
    if (!DEC) {
      load_bells(ra, rb, rc, lane);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int rr = lane & 15, q = rr >> 2, ch = 4 * g + (rr & 3);
        const double* w = (q >> 1) ? w1 : w0;
#pragma unroll
        for (int s = 0; s < 5; ++s) wf[g][s] = ch < C ? w[(2 * ch + (q & 1)) * NB + 4 * s + cg] : 0.0;
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int ch = 4 * g + cg;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double* bb = (q >> 1) ? b1 : b0;
        bias[g][q] = ch < C ? (DEC ? bb[ch] : bb[2 * ch + (q & 1)]) : 0.0;
      }
    }
  }
  // the bell constants as the radial evaluations read them (BellRow is the other source)
  __device__ __forceinline__ double a(int s) const { return ak[s]; }
  __device__ __forceinline__ double b(int s) const { return bk[s]; }
  __device__ __forceinline__ double c2(int s) const { return ck2[s]; }
};
// The 15 bell constants of a lane group as a row of LDS, a[5] | b[5] | c^2[5]: the symmetric large-jet sweep reads them per tile --
// in registers the second pass of its tiles below the diagonal spills into the hot loop.
struct BellRow {
  const double* row;
  __device__ __forceinline__ double a(int s) const { return row[s]; }
  __device__ __forceinline__ double b(int s) const { return row[5 + s]; }
  __device__ __forceinline__ double c2(int s) const { return row[10 + s]; }
};

// ---- geometry of an encoder pair --------------------------------------------------------------------------------------------
// d = p_i - p_j (real Cartesian momenta), an = |norm_sq| with norm_sq as the reference forms it (zonal_functions.py:142, 201-218),
// on = the pair is live (both particles real, inside the jet) and norm_sq != 0.  The canonical difference is
// q = [d0, a - ib, d3, -a - ib] with a = d1 / sqrt 2, b = d2 / sqrt 2: the edge products use (qd0, qd3, qa, qb), canonical() spells
// q out for the callers that multiply by it.
struct EncPair {
  double d0, d1, d2, d3, an;
  double qd0, qd3, qa, qb;
  bool on;
  __device__ __forceinline__ void canonical(cx<double> (&q)[4]) const {
    const double h = rsqrt2<double>();
    q[0] = {d0, 0.0};
    q[1] = {d1 * h, -d2 * h};
    q[2] = {d3, 0.0};
    q[3] = {-d1 * h, -d2 * h};
  }
};
__device__ __forceinline__ EncPair enc_pair(const double* pi, const double* pjj, bool ok, bool m1, bool m2) {
  EncPair p;
  p.d0 = pi[0] - pjj[0];  p.d1 = pi[1] - pjj[1];  p.d2 = pi[2] - pjj[2];  p.d3 = pi[3] - pjj[3];
  const double q0 = p.d0 * p.d0, q1 = p.d1 * p.d1, q2 = p.d2 * p.d2, q3 = p.d3 * p.d3;
  const double nsq = (2.0 * q0 - (((q0 + q1) + q2) + q3)) + 1e-16;
  p.an = fabs(nsq);                                          // (c * norm)^2 == c^2 |norm_sq|
  p.on = ok && m1 && m2 && (nsq != 0.0);
  const double h = rsqrt2<double>();
  p.qd0 = p.d0;  p.qd3 = p.d3;  p.qa = p.d1 * h;  p.qb = p.d2 * h;
  return p;
}

// ---- the radial network of a tile: R[g] = (R0r, R0i, R1r, R1i) of this lane's pair and channel 4 g + cg ---------------------------
// A masked pair keeps the Linear bias: the mask zeroes the basis, not the output (position_levels.py:144-149).
//
// TWO FORMS, which differ in the last bits of rho and beta and are not to be merged without re-recording every pinned hash:
//   radial_masked   1 / (1 + c^2 |n|^2) for the five bells at once by rcp5, inside an EXEC-masked block, without the reference's
//                   "+ 1e-16" (absorbed: the sum is >= 1); it also hands back rho for the B rows of the radial GEMM.
//                   level_bwd3, level_bwd_sweep_enc; level_fwd2's prep() is the same statements, spelled out there (the kernel
//                   says why) -- the training step at maxdim 2.
//   radial_select   one fast_rcp((1 + c^2 |n|^2) + 1e-16) per bell and a select per value; rho_select is its rho.
//                   The moments kernels of generic_moments.hip -- which serve maxdim 3 with N > 32 --, level_bwd_rad2 and
//                   moments_rad_reduce2 (rho only; the latter with columns, not pairs, on the lanes); level_bwd_nodes2 spells
//                   it out (the kernel says why).
template <int NG>
__device__ __forceinline__ void radial_bias(const double (&bias)[NG][4], v4d (&R)[NG]) {
#pragma unroll
  for (int g = 0; g < NG; ++g) R[g] = v4d{bias[g][0], bias[g][1], bias[g][2], bias[g][3]};
}
template <int NG, class K>
__device__ __forceinline__ void radial_masked(const K& k, const double (&wf)[NG][5], const double (&bias)[NG][4], double an, bool on,
                                              v4d (&R)[NG], double (&rho)[5]) {
  double beta[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 5; ++s) rho[s] = 0.0;
  if (on) {                                                  // (EXEC-masked block: no per-value selects)
#pragma unroll
    for (int s = 0; s < 5; ++s) beta[s] = 1.0 + k.c2(s) * an;
    rcp5(beta, rho);
#pragma unroll
    for (int s = 0; s < 5; ++s) beta[s] = __builtin_fma(k.b(s), rho[s], k.a(s));
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    R[g] = v4d{bias[g][0], bias[g][1], bias[g][2], bias[g][3]};
#pragma unroll
    for (int s = 0; s < 5; ++s) R[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf[g][s], beta[s], R[g], 0, 0, 0);
  }
}
__device__ __forceinline__ double rho_select(double c2, double an, bool on) {
  return on ? fast_rcp((1.0 + c2 * an) + 1e-16) : 0.0;
}
template <int NG, class K>
__device__ __forceinline__ void radial_select(const K& k, const double (&wf)[NG][5], const double (&bias)[NG][4], double an, bool on,
                                              v4d (&R)[NG]) {
  double beta[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const double u = (1.0 + k.c2(s) * an) + 1e-16;
    const double bv = __builtin_fma(k.b(s), fast_rcp(u), k.a(s));
    beta[s] = on ? bv : 0.0;
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    R[g] = v4d{bias[g][0], bias[g][1], bias[g][2], bias[g][3]};
#pragma unroll
    for (int s = 0; s < 5; ++s) R[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf[g][s], beta[s], R[g], 0, 0, 0);
  }
}

// ---- the radial-parameter GEMM ----------------------------------------------------------------------------------------------
//   T1[r][k] = sum_p G[p][r] on rho_k    T2[r][k] = sum_p G[p][r] on |n|^2 rho_k^2    S[r] = sum_p G[p][r] on    dB[r] = sum_p G[p][r]
// are one GEMM [r x pairs] . [pairs x 42 columns].  Both operands are produced pair-per-lane and turned into fragments by 16 x 16
// transposes through the wave's LDS tiles trw: NG tiles [pair][r' = cg + 4 q] of dL/d rad, then three tiles [pair][column]
//   [0, 16) rho_k, k < 16 | [16, 32) |n|^2 rho_k^2, k < 16 | 32..35 rho_16..19, 36..39 |n|^2 rho_16..19^2, 40 on, 41 one, 42..47 zero.
// B rows of this lane's pair: its five bells k = 4 s + cg; each of the four channel lanes of a pair fills two of columns 40..47.
__device__ __forceinline__ void rad_b_rows(double* xb, int pr, int cg, const double (&rho)[5], double an, bool on, bool ok) {
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const double x2 = an * rho[s] * rho[s];
    if (s < 4) {
      xb[pr * PAIR_TS + 4 * s + cg] = rho[s];
      xb[16 * PAIR_TS + pr * PAIR_TS + 4 * s + cg] = x2;
    } else {
      xb[32 * PAIR_TS + pr * PAIR_TS + cg] = rho[s];
      xb[32 * PAIR_TS + pr * PAIR_TS + 4 + cg] = x2;
    }
  }
  xb[32 * PAIR_TS + pr * PAIR_TS + 8 + 2 * cg] = cg == 0 ? (on ? 1.0 : 0.0) : 0.0;
  xb[32 * PAIR_TS + pr * PAIR_TS + 9 + 2 * cg] = cg == 0 ? (ok ? 1.0 : 0.0) : 0.0;
}
// A rows of one channel group: dL/d (R0r, R0i, R1r, R1i) of this lane's pair and channel into the group's tile ta
__device__ __forceinline__ void rad_a_rows(double* ta, int pr, int cg, double G0r, double G0i, double G1r, double G1i) {
  ta[pr * PAIR_TS + cg] = G0r;
  ta[pr * PAIR_TS + 4 + cg] = G0i;
  ta[pr * PAIR_TS + 8 + cg] = G1r;
  ta[pr * PAIR_TS + 12 + cg] = G1i;
}
// T[g][t][r' = cg + 4 q][col = pr] += sum over the tile's 16 pairs: A[i = r'][k = pair], B[k = pair][j = col], four pairs per
// instruction.  The wave's rows are visible to its own lanes before, and read by all of them before the next tile overwrites them.
template <int NG>
__device__ __forceinline__ void rad_gemm_step(const double* trw, int pr, int cg, v4d (&T)[NG][3]) {
  wave_sync();
  const double* xb = trw + NG * 16 * PAIR_TS;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int prow = 4 * s + cg;                             // pair held by this lane for k-step s
    double bv[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) bv[t] = xb[t * 16 * PAIR_TS + prow * PAIR_TS + pr];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const double av = trw[g * 16 * PAIR_TS + prow * PAIR_TS + pr];
#pragma unroll
      for (int t = 0; t < 3; ++t) T[g][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[t], T[g][t], 0, 0, 0);
    }
  }
  wave_sync();
}
// Epilogue, first half: every wave leaves its accumulators as a row of 12 NG doubles per lane in red (which may alias the transpose
// tiles: the caller's barrier stands before this); the caller's barrier follows.
template <int NG>
__device__ __forceinline__ void rad_rows_store(double* red, int wave, int lane, const v4d (&T)[NG][3]) {
  double* mine = red + (size_t)(wave * 64 + lane) * NG * 12;
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) mine[(g * 3 + t) * 4 + q] = T[g][t][q];
}
// Epilogue, second half: the sum over the waves in a FIXED form and the T1 | T2 | S | dB partial-row layout (row r = lin 2C + 2c + z).
//   Sequential   ((((0 + w0) + w1) + w2) + ...) over NWV waves                          level_bwd_sweep_enc
//   Pairwise     (w0 + w1) + (w2 + w3), with eight waves + ((w4 + w5) + (w6 + w7))      every other kernel
// NWV = 0: four or eight waves, known at run time only (nw; level_bwd_rad2).  DEAL: the 12 NG sums of a lane position are dealt to
// four calling waves by q == wq (level_bwd3: one wave doing all of them was 4 000 cycles of the kernel's tail); else one wave calls.
enum class WaveSum { Sequential, Pairwise };
template <int C, int NWV, WaveSum FORM, bool DEAL = false>
__device__ __forceinline__ void rad_rows_sum(const double* red, double* part, int lane, int wq = 0, int nw = NWV) {
  static_assert(FORM != WaveSum::Sequential || NWV > 0, "the sequential form needs the wave count at compile time");
  constexpr int NG = (C + 3) / 4, R = 4 * C;
  const int col = lane & 15, cg = lane >> 4;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int ch = 4 * g + cg;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (DEAL && q != wq) continue;
        const int e = (g * 3 + t) * 4 + q;
        double v;
        if constexpr (FORM == WaveSum::Sequential) {
          v = 0.0;
          for (int w = 0; w < NWV; ++w) v += red[(size_t)(w * 64 + lane) * NG * 12 + e];
        } else {
          v = (red[(size_t)(0 * 64 + lane) * NG * 12 + e] + red[(size_t)(1 * 64 + lane) * NG * 12 + e]) +
              (red[(size_t)(2 * 64 + lane) * NG * 12 + e] + red[(size_t)(3 * 64 + lane) * NG * 12 + e]);
          if (NWV ? NWV == 8 : nw == 8)
            v += (red[(size_t)(4 * 64 + lane) * NG * 12 + e] + red[(size_t)(5 * 64 + lane) * NG * 12 + e]) +
                 (red[(size_t)(6 * 64 + lane) * NG * 12 + e] + red[(size_t)(7 * 64 + lane) * NG * 12 + e]);
        }
        if (ch >= C) continue;
        const int r = (q >> 1) * 2 * C + 2 * ch + (q & 1);
        if (t == 0) part[r * NB + col] = v;                      // T1[r][k = col]
        else if (t == 1) part[R * NB + r * NB + col] = v;        // T2[r][k = col]
        else {
          if (col < 4) part[r * NB + 16 + col] = v;
          else if (col < 8) part[R * NB + r * NB + 16 + (col - 4)] = v;
          else if (col == 8) part[2 * R * NB + r] = v;           // S
          else if (col == 9) part[2 * R * NB + R + r] = v;       // dB
        }
      }
  }
}

// ---- backward of one encoder edge (pair, channel) ---------------------------------------------------------------------------
// NOT shared: the edge backward of the single-sweep kernels (level_bwd3, level_bwd_sweep_enc: gradient w.r.t. the source node, and
// the forward and reverse edge's gradient w.r.t. the pair's radial values).  The two are the same statements term for term, but
// stated as functions here they gave other last bits of the radial gradients (g_a, g_b, g_c, g_w1, g_b1; everything else equal):
// the complex products written with * and + are contracted into fused multiply-adds by the compiler, and which product it fuses
// depends on the code around them.  They also sit at the register limit (a first restatement spilled 30 - 150 registers in the
// symmetric forms; the figures of both are in profiles/r11_pair_dev.txt, section 2).  The two-sweep form below keeps its bits and is shared by level_bwd_rad2; level_bwd3's phase 2 is the text to
// read for the single-sweep form, and level_bwd_sweep_enc follows it.
//
// The upstream gradient of one receiver's aggregate, one channel: gA3 enters with its factor 1/2 everywhere.
struct AggGrad {
  cx<double> gA3, gA4, gA1[4], gA2[4];
};
// The source particle's features of one channel, with v[3] - v[1] and v[1] + v[3] for <v, q>.
struct SrcFeat {
  cx<double> s, v[4], dv, sv;
  __device__ __forceinline__ void diffs() {
    dv = {v[3].r - v[1].r, v[3].i - v[1].i};
    sv = {v[1].r + v[3].r, v[1].i + v[3].i};
  }
  // from a row [s2 | v_r[4] | v_i[4]]
  __device__ __forceinline__ void load(const double* n) {
    s = {n[0], n[1]};
#pragma unroll
    for (int m = 0; m < 4; ++m) v[m] = {n[2 + m], n[6 + m]};
    diffs();
  }
};
// With real momenta q = [d0, a - ib, d3, -a - ib] the edge e1[m] = R1 q[m] enters the radial gradient only through
//   P2 = sum_m gA2[m] conj(q[m])    and    V = <v, q> = v0 d0 - v2 d3 + a (v3 - v1) - ib (v1 + v3):
// 8 + 8 flops instead of four complex products each.
__device__ __forceinline__ cx<double> edge_P2(const cx<double> (&gA2)[4], const EncPair& p) {
  const cx<double> dg = {gA2[1].r - gA2[3].r, gA2[1].i - gA2[3].i}, sg = {gA2[1].r + gA2[3].r, gA2[1].i + gA2[3].i};
  cx<double> P2;
  P2.r = __builtin_fma(gA2[0].r, p.qd0, __builtin_fma(gA2[2].r, p.qd3, __builtin_fma(p.qa, dg.r, -p.qb * sg.i)));
  P2.i = __builtin_fma(gA2[0].i, p.qd0, __builtin_fma(gA2[2].i, p.qd3, __builtin_fma(p.qa, dg.i, p.qb * sg.r)));
  return P2;
}
__device__ __forceinline__ cx<double> edge_V(const cx<double> (&v)[4], const cx<double>& dv, const cx<double>& sv, const EncPair& p) {
  cx<double> V;
  V.r = __builtin_fma(v[0].r, p.qd0, __builtin_fma(-v[2].r, p.qd3, __builtin_fma(p.qa, dv.r, p.qb * sv.i)));
  V.i = __builtin_fma(v[0].i, p.qd0, __builtin_fma(-v[2].i, p.qd3, __builtin_fma(p.qa, dv.i, -p.qb * sv.r)));
  return V;
}
// Gradient w.r.t. the radial values of the pair i <- j, before the change of basis R0 -> e0:
//   ge0 = gA4 conj(s_j) + sum_m gA1[m] conj(v_j[m])      gR1 = sum_m ge1[m] conj(q[m]) = conj(s_j) P2 + gA3 conj(V)
__device__ __forceinline__ void enc_edge_rad(const AggGrad& u, const EncPair& p, const SrcFeat& x, cx<double>& ge0, cx<double>& gR1) {
  ge0 = cmulc(u.gA4, x.s);
#pragma unroll
  for (int m = 0; m < 4; ++m) cfmac(ge0, u.gA1[m], x.v[m]);
  gR1 = cmulc(edge_P2(u.gA2, p), x.s);
  cfmac(gR1, u.gA3, edge_V(x.v, x.dv, x.sv, p));
}

// ---- the decoder's bias-gradient epilogue -----------------------------------------------------------------------------------
// dB0 / dB1: this lane's sums of dL/d b0, dL/d b1 over its pairs, per channel group.  First half: sum over the 16 pair slots
// (butterfly), one row of 8 per (wave, group); the caller's barrier follows.  Second half: thread (lin, channel) adds the waves in
// index order.
template <int NG>
__device__ __forceinline__ void dec_bias_store(double* red, int wave, int pr, int cg, const double (&dB0)[NG], const double (&dB1)[NG]) {
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    double x0 = dB0[g], x1 = dB1[g];
    for (int m = 1; m < 16; m <<= 1) { x0 += shfl_xor(x0, m); x1 += shfl_xor(x1, m); }
    if (pr == 0) {
      red[(wave * NG + g) * 8 + cg] = x0;
      red[(wave * NG + g) * 8 + 4 + cg] = x1;
    }
  }
}
template <int C, int NWV>
__device__ __forceinline__ void dec_bias_sum(const double* red, double* part, int tid) {
  constexpr int NG = (C + 3) / 4;
  if (tid < 2 * C) {
    const int lin = tid / C, ch = tid - lin * C, g = ch >> 2, c4 = ch & 3;
    double s = 0;
    for (int w = 0; w < NWV; ++w) s += red[(w * NG + g) * 8 + lin * 4 + c4];
    part[tid] = s;
  }
}

}  // namespace lgn
