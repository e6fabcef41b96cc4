// lgn-autoencoder_amd/csrc/generic_moments.hip -- the N^2 part of a message-passing level for ARBITRARY node irreps
// (maxdim = 3: (0,0),(1,1),(2,0),(0,2),(2,2); reference lgn/cg_lib/cg_ops.py:135-298 with aggregate=True).
//
// The reference forms, per pair of irreps (r1 of the node, r2 of the edge), the Kronecker product
// node_j[r1] (x) edge_ij[r2], sums it over neighbours j FIRST and applies the Clebsch-Gordan matrix afterwards
// (cg_ops.py:287-297 then :195-204).  The neighbour sum therefore only ever needs the "moments"
//     U[i][c][q][0]     = sum_j X_j[c][q] * e0_ij[c]          (edge irrep (0,0),  e0 = R0 (1+1i))
//     U[i][c][q][1 + m] = sum_j X_j[c][q] * e1_ij[c][m]       (edge irrep (1,1),  e1 = R1 canonical(p_i - p_j))
// for every component q of the packed node feature vector X (Q = sum of the irrep dimensions).  These kernels
// compute the moments and their backward passes without any Clebsch-Gordan table; the (sparse, table driven)
// CG contraction is O(N) per jet and lives in generic_local.hip.  At maxdim = 2 (Q = 5) this reproduces the fused
// closed-form kernels, which the tests use as a cross-check.
//
// Mapping = level_fwd2 / level_bwd2: wave = 4 particles, tiles of 4 partners, lane = (pair slot, channel in group),
// radial Linear layers on v_mfma_f64_16x16x4_f64; the component axis q is processed in chunks of QC so that the
// accumulators stay in registers (the radial part is recomputed per chunk).
#include <stdlib.h>

#include "lds.hpp"
#include "pair_dev.hpp"
#include "ops.hpp"

namespace lgn {

namespace {
constexpr int QC = 5;      // components per sweep

// geometry + radial values of the ordered pair (i, j) held by this lane; returns R[g] = (R0r, R0i, R1r, R1i)
// (the select form of the radial network: pair_dev.hpp)
template <int C, bool DEC>
__device__ __forceinline__ void pair_radial(const RadLane<C, DEC>& rc, const double* pi, const double* pjj, bool ok, bool mi,
                                            bool mj, cx<double> (&q)[4], v4d (&R)[RadLane<C, DEC>::NG], double& an, bool& on) {
  if (DEC) {
#pragma unroll
    for (int m = 0; m < 4; ++m) q[m] = {pi[m] - pjj[m], pi[4 + m] - pjj[4 + m]};
    radial_bias(rc.bias, R);
    an = 0.0;
    on = false;
  } else {
    const EncPair ep = enc_pair(pi, pjj, ok, mi, mj);
    an = ep.an;
    on = ep.on;
    ep.canonical(q);
    radial_select(rc, rc.wf, rc.bias, an, on, R);
  }
}

// cooperative load of a jet's packed features X[2][B][N][C][Q] into LDS as xs[(j*C + c)*Q*2 + q*2 + z]
__device__ __forceinline__ void load_packed(const double* __restrict__ X, int B, int N, int C, int Q, int b, double* xs) {
  const size_t plane = (size_t)B * N * C * Q;
  const double* x0 = X + (size_t)b * N * C * Q;
  for (int e = threadIdx.x; e < N * C * Q; e += BLOCK) {
    xs[2 * e] = x0[e];
    xs[2 * e + 1] = x0[plane + e];
  }
}
template <bool DEC>
__device__ __forceinline__ void load_pos(const GenArgs& a, int b, double* pj, uint8_t* mk) {
  const int N = a.N, B = a.B;
  if (DEC) {
    const size_t plane_p = (size_t)B * N * 4;
    const double* p0 = a.p + (size_t)b * N * 4;
    for (int e = threadIdx.x; e < N * 4; e += BLOCK) {
      int j = e >> 2, m = e & 3;
      pj[j * 8 + m] = p0[e];
      pj[j * 8 + 4 + m] = p0[plane_p + e];
    }
  } else {
    const double* p0 = a.p + (size_t)b * N * 4;
    for (int e = threadIdx.x; e < N * 4; e += BLOCK) pj[e] = p0[e];
    for (int e = threadIdx.x; e < N; e += BLOCK) mk[e] = a.mask[(size_t)b * N + e];
  }
}
}  // namespace

// =========================================================================================================
// forward:  U[b][i][c][q][k][z]
// =========================================================================================================
// XL: the jet's packed features are staged in LDS (N C Q 16 bytes); XL = false (round 5: jets whose features do not fit -- 150
// particles at maxdim 3 are 288 KB -- used to be refused) reads them from global memory instead, every source row from L1 / L2.
template <int C, bool DEC, bool XL>
__global__ __launch_bounds__(BLOCK) void moments_fwd_kernel(GenArgs a) {
  constexpr int NG = (C + 3) / 4;
  constexpr int PS = DEC ? 8 : 4;
  const int N = a.N, B = a.B, Q = a.Q;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* xs = reinterpret_cast<double*>(smem_raw);           // N * C * Q * 2 (XL)
  double* pj = xs + (XL ? (size_t)N * C * Q * 2 : 0);         // N * PS
  uint8_t* mk = reinterpret_cast<uint8_t*>(pj + N * PS);
  const size_t xplane = (size_t)B * N * C * Q;
  if (XL) load_packed(a.X, B, N, C, Q, b, xs);
  load_pos<DEC>(a, b, pj, mk);
  RadLane<C, DEC> rc;
  rc.load(a.ra, a.rb, a.rc, a.w0, a.b0, a.w1, a.b1, lane);
  __syncthreads();

  const int pr = lane & 15, cg = lane >> 4, ti = pr >> 2, tj = pr & 3;
  const int ngroups = (N + 3) >> 2;
  for (int rg = wave; rg < ngroups; rg += 4) {
    const int i = rg * 4 + ti;
    const bool iok = i < N;
    const int ii = iok ? i : N - 1;
    double pi[PS];
#pragma unroll
    for (int m = 0; m < PS; ++m) pi[m] = pj[ii * PS + m];
    const bool mi = DEC ? false : (mk[ii] != 0);
    for (int q0 = 0; q0 < Q; q0 += QC) {
      cx<double> acc[NG][QC][5];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int x = 0; x < QC; ++x)
#pragma unroll
          for (int k = 0; k < 5; ++k) acc[g][x][k] = {0, 0};
      for (int j0 = 0; j0 < N; j0 += 4) {
        const int j = j0 + tj;
        const bool ok = iok && j < N;
        const int jj = j < N ? j : N - 1;
        cx<double> q[4];
        v4d R[NG];
        double an;
        bool on;
        pair_radial<C, DEC>(rc, pi, pj + jj * PS, ok, mi, DEC ? false : (mk[jj] != 0), q, R, an, on);
        if (ok) {
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const int ch = 4 * g + cg;
            if (ch < C) {
              const cx<double> R0 = {R[g][0], R[g][1]}, R1 = {R[g][2], R[g][3]};
              cx<double> e[5];
              e[0] = {R0.r - R0.i, R0.r + R0.i};
#pragma unroll
              for (int m = 0; m < 4; ++m) e[1 + m] = cmul(R1, q[m]);
              const double* xj = xs + ((size_t)jj * C + ch) * Q * 2;
              const double* xg = a.X + (((size_t)b * N + jj) * C + ch) * Q;
#pragma unroll
              for (int x = 0; x < QC; ++x) {
                if (q0 + x < Q) {
                  const cx<double> xv = XL ? cx<double>{xj[(q0 + x) * 2], xj[(q0 + x) * 2 + 1]} : cx<double>{xg[q0 + x], xg[xplane + q0 + x]};
#pragma unroll
                  for (int k = 0; k < 5; ++k) cfma(acc[g][x][k], xv, e[k]);
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int ch = 4 * g + cg;
#pragma unroll
        for (int x = 0; x < QC; ++x)
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            const double sr = quad_sum(acc[g][x][k].r), si = quad_sum(acc[g][x][k].i);
            if (tj == 0 && iok && ch < C && q0 + x < Q) {
              double* u = a.U + ((((size_t)b * N + i) * C + ch) * Q + q0 + x) * 10 + 2 * k;
              u[0] = sr;
              u[1] = si;
            }
          }
      }
    }
  }
}

// =========================================================================================================
// backward, j-centric:  gX[j][c][q] += sum_i sum_k gU[i][c][q][k] conj(e_k,ij[c])      (+ decoder d p_j)
// =========================================================================================================
template <int C, bool DEC>
__global__ __launch_bounds__(BLOCK) void moments_bwd_nodes_kernel(GenArgs a) {
  constexpr int NG = (C + 3) / 4;
  constexpr int PS = DEC ? 8 : 4;
  const int N = a.N, B = a.B, Q = a.Q;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* pj = reinterpret_cast<double*>(smem_raw);           // N * PS
  uint8_t* mk = reinterpret_cast<uint8_t*>(pj + N * PS);
  load_pos<DEC>(a, b, pj, mk);
  RadLane<C, DEC> rc;
  rc.load(a.ra, a.rb, a.rc, a.w0, a.b0, a.w1, a.b1, lane);
  __syncthreads();

  const int pr = lane & 15, cg = lane >> 4, tj = pr >> 2, ti = pr & 3;
  const size_t plane = (size_t)B * N * C * Q;
  const int ngroups = (N + 3) >> 2;
  for (int rg = wave; rg < ngroups; rg += 4) {
    const int j = rg * 4 + tj;
    const bool jok = j < N;
    const int jj = jok ? j : N - 1;
    double pme[PS];
#pragma unroll
    for (int m = 0; m < PS; ++m) pme[m] = pj[jj * PS + m];
    const bool mj = DEC ? false : (mk[jj] != 0);
    cx<double> Gq[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int q0 = 0; q0 < Q; q0 += QC) {
      cx<double> acc[NG][QC], xme[NG][QC];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int x = 0; x < QC; ++x) {
          acc[g][x] = {0, 0};
          xme[g][x] = {0, 0};
          const int ch = 4 * g + cg;
          if (DEC && ch < C && q0 + x < Q) {
            const size_t e = (((size_t)b * N + jj) * C + ch) * Q + q0 + x;
            xme[g][x] = {a.X[e], a.X[plane + e]};
          }
        }
      for (int i0 = 0; i0 < N; i0 += 4) {
        const int i = i0 + ti;
        const bool ok = jok && i < N;
        const int ii = i < N ? i : N - 1;
        cx<double> q[4];
        v4d R[NG];
        double an;
        bool on;
        pair_radial<C, DEC>(rc, pj + ii * PS, pme, ok, DEC ? false : (mk[ii] != 0), mj, q, R, an, on);
        if (ok) {
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const int ch = 4 * g + cg;
            if (ch < C) {
              const cx<double> R0 = {R[g][0], R[g][1]}, R1 = {R[g][2], R[g][3]};
              cx<double> e[5];
              e[0] = {R0.r - R0.i, R0.r + R0.i};
#pragma unroll
              for (int m = 0; m < 4; ++m) e[1 + m] = cmul(R1, q[m]);
              const double* gu = a.gU + (((size_t)b * N + ii) * C + ch) * Q * 10;
#pragma unroll
              for (int x = 0; x < QC; ++x) {
                if (q0 + x < Q) {
                  const double* gq = gu + (q0 + x) * 10;
#pragma unroll
                  for (int k = 0; k < 5; ++k) {
                    const cx<double> gv = {gq[2 * k], gq[2 * k + 1]};
                    cfmac(acc[g][x], gv, e[k]);
                    if (DEC && k > 0) {          // G_e1[m] += gU[q][1+m] conj(X_j[q]);  G_q[m] += G_e1[m] conj(R1)
                      cfmac(Gq[k - 1], cmulc(gv, xme[g][x]), R1);
                    }
                  }
                }
              }
            }
          }
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int ch = 4 * g + cg;
#pragma unroll
        for (int x = 0; x < QC; ++x) {
          const double sr = quad_sum(acc[g][x].r), si = quad_sum(acc[g][x].i);
          if (ti == 0 && jok && ch < C && q0 + x < Q) {
            const size_t e = (((size_t)b * N + j) * C + ch) * Q + q0 + x;
            a.gX[e] += sr;
            a.gX[plane + e] += si;
          }
        }
      }
    }
    if (DEC) {
      const size_t plp = (size_t)B * N * 4;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        double qr = quad_sum(Gq[m].r), qi = quad_sum(Gq[m].i);
        qr += shfl_xor(qr, 16);  qr += shfl_xor(qr, 32);
        qi += shfl_xor(qi, 16);  qi += shfl_xor(qi, 32);
        if (jok && ti == 0 && cg == 0) {
          a.g_p[((size_t)b * N + jj) * 4 + m] -= qr;
          a.g_p[plp + ((size_t)b * N + jj) * 4 + m] -= qi;
        }
      }
    }
  }
}

// =========================================================================================================
// backward, i-centric: radial parameter gradient sums (encoder: T1|T2|S|dB as in level_bwd2; decoder: bias sums)
// and the decoder's d p_i.   G_e_k[c] = sum_q gU[i][c][q][k] conj(X_j[c][q])
// =========================================================================================================
template <int C, bool DEC, bool XL>
__global__ __launch_bounds__(BLOCK) void moments_bwd_rad_kernel(GenArgs a) {
  constexpr int NG = (C + 3) / 4;
  constexpr int PS = DEC ? 8 : 4;
  const int N = a.N, B = a.B, Q = a.Q;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* xs = reinterpret_cast<double*>(smem_raw);           // N * C * Q * 2 (XL; else read from global memory, see moments_fwd_kernel)
  double* pj = xs + (XL ? (size_t)N * C * Q * 2 : 0);         // N * PS
  const size_t xplane = (size_t)B * N * C * Q;
  double* tr = pj + N * PS;                                   // 4 waves' transpose tiles (also the final reduction buffer)
  constexpr int TRSZ = 4 * pair_scratch(NG);
  uint8_t* mk = reinterpret_cast<uint8_t*>(tr + TRSZ);
  if (XL) load_packed(a.X, B, N, C, Q, b, xs);
  load_pos<DEC>(a, b, pj, mk);
  RadLane<C, DEC> rc;
  rc.load(a.ra, a.rb, a.rc, a.w0, a.b0, a.w1, a.b1, lane);
  __syncthreads();

  const int pr = lane & 15, cg = lane >> 4, ti = pr >> 2, tj = pr & 3;
  double* trw = tr + wave * pair_tiles(NG);
  v4d T[NG][3];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int t = 0; t < 3; ++t) T[g][t] = v4d{0, 0, 0, 0};
  double dB0[NG], dB1[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) dB0[g] = dB1[g] = 0.0;

  const int ngroups = (N + 3) >> 2;
  for (int rg = wave; rg < ngroups; rg += 4) {
    const int i = rg * 4 + ti;
    const bool iok = i < N;
    const int ii = iok ? i : N - 1;
    double pi[PS];
#pragma unroll
    for (int m = 0; m < PS; ++m) pi[m] = pj[ii * PS + m];
    const bool mi = DEC ? false : (mk[ii] != 0);
    cx<double> Gq[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int j0 = 0; j0 < N; j0 += 4) {
      const int j = j0 + tj;
      const bool ok = iok && j < N;
      const int jj = j < N ? j : N - 1;
      cx<double> q[4];
      v4d R[NG];
      double an;
      bool on;
      pair_radial<C, DEC>(rc, pi, pj + jj * PS, ok, mi, DEC ? false : (mk[jj] != 0), q, R, an, on);
      if (!DEC) {
        double rho[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) rho[s] = rho_select(rc.ck2[s], an, on);
        rad_b_rows(trw + NG * 16 * PAIR_TS, pr, cg, rho, an, on, ok);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int ch = 4 * g + cg;
        double G0r = 0, G0i = 0, G1r = 0, G1i = 0;
        if (ok && ch < C) {
          const double* xj = xs + ((size_t)jj * C + ch) * Q * 2;
          const double* xg = a.X + (((size_t)b * N + jj) * C + ch) * Q;
          const double* gu = a.gU + (((size_t)b * N + ii) * C + ch) * Q * 10;
          cx<double> ge[5] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
          for (int x = 0; x < Q; ++x) {
            const cx<double> xv = XL ? cx<double>{xj[2 * x], xj[2 * x + 1]} : cx<double>{xg[x], xg[xplane + x]};
#pragma unroll
            for (int k = 0; k < 5; ++k) cfmac(ge[k], cx<double>{gu[x * 10 + 2 * k], gu[x * 10 + 2 * k + 1]}, xv);
          }
          cx<double> gR1 = {0, 0};
          const cx<double> R1 = {R[g][2], R[g][3]};
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            cfmac(gR1, ge[1 + m], q[m]);
            if (DEC) cfmac(Gq[m], ge[1 + m], R1);
          }
          G0r = ge[0].r + ge[0].i;  G0i = ge[0].i - ge[0].r;
          G1r = gR1.r;  G1i = gR1.i;
        }
        if (DEC) {
          dB0[g] += G0r + G0i;          // R0 = b0 (1+i): d b0 = Re G_R0 + Im G_R0
          dB1[g] += G1r + G1i;
        } else {
          rad_a_rows(trw + g * 16 * PAIR_TS, pr, cg, G0r, G0i, G1r, G1i);
        }
      }
      if (!DEC) rad_gemm_step(trw, pr, cg, T);
    }
    if (DEC) {
      const size_t plp = (size_t)B * N * 4;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        double qr = quad_sum(Gq[m].r), qi = quad_sum(Gq[m].i);
        qr += shfl_xor(qr, 16);  qr += shfl_xor(qr, 32);
        qi += shfl_xor(qi, 16);  qi += shfl_xor(qi, 32);
        if (iok && tj == 0 && cg == 0) {
          a.g_p[((size_t)b * N + i) * 4 + m] += qr;
          a.g_p[plp + ((size_t)b * N + i) * 4 + m] += qi;
        }
      }
    }
  }

  __syncthreads();
  double* part = a.part_rad + (size_t)blockIdx.x * rad_partial_size(C, DEC);
  if (DEC) {
    dec_bias_store(tr, wave, pr, cg, dB0, dB1);
    __syncthreads();
    dec_bias_sum<C, 4>(tr, part, tid);
  } else {
    rad_rows_store(tr, wave, lane, T);
    __syncthreads();
    if (wave == 0) rad_rows_sum<C, 4, WaveSum::Pairwise>(tr, part, lane);
  }
}

// ---------------------------------------------------------------------------------------------------------
template <int C, bool DEC>
static int launch_moments(const GenArgs& a, int which, hipStream_t st) {
  constexpr int PS = DEC ? 8 : 4;
  constexpr int NG = (C + 3) / 4;
  const size_t xs = sizeof(double) * (size_t)a.N * C * a.Q * 2, pos = sizeof(double) * (size_t)a.N * PS + a.N + 16;
  if (which == 0) {
    const bool xl = xs + pos <= LGN_LDS_LIMIT;       // (jets whose features do not fit read them from global memory)
    auto k = xl ? moments_fwd_kernel<C, DEC, true> : moments_fwd_kernel<C, DEC, false>;
    return lds_launch(k, "moments_fwd", dim3(a.B), dim3(BLOCK), (xl ? xs : 0) + pos, st, a);
  }
  if (which == 1) return lds_launch(moments_bwd_nodes_kernel<C, DEC>, "moments_bwd_nodes", dim3(a.B), dim3(BLOCK), pos, st, a);
  constexpr int TRSZ = 4 * pair_scratch(NG);
  const bool xl = xs + pos + sizeof(double) * TRSZ <= LGN_LDS_LIMIT;
  auto k = xl ? moments_bwd_rad_kernel<C, DEC, true> : moments_bwd_rad_kernel<C, DEC, false>;
  return lds_launch(k, "moments_bwd_rad", dim3(a.B), dim3(BLOCK), (xl ? xs : 0) + pos + sizeof(double) * TRSZ, st, a);
}

bool moments2_fits(const GenArgs& a, int decoder);                                               // generic_moments2.hip
int moments2_dispatch(const GenArgs& a, int decoder, int which, double* Gbuf, hipStream_t st);

// which: 0 forward, 1 backward j-centric, 2 backward i-centric (one partial row per jet).
// Jets that fit in LDS take the channel-outermost kernels of generic_moments2.hip (the encoder's i-centric pass then needs
// a.gbuf, moments2_gbuf_doubles(B, N, C) doubles of scratch); LGN_AMD_MOMENTS_V1=1 keeps this file's kernels.
int moments_dispatch(const GenArgs& a, int decoder, int which, hipStream_t st) {
  LGN_CHECK_ARG(a.B > 0 && a.N > 0 && a.Q > 0, "moments: empty input (B=%d N=%d Q=%d)", a.B, a.N, a.Q);
  {
    const bool v1 = (a.flags & LVL_MOMENTS_V1) != 0;
    if (!v1 && moments2_fits(a, decoder) && (decoder || which != 2 || a.gbuf)) return moments2_dispatch(a, decoder, which, a.gbuf, st);
  }
  LGN_CHECK_ARG(!a.tb, "moments: the tile-blocked layout is implemented by the channel-outermost kernels only (N <= 32)");
#define LGN_CASE(CC) case CC: return decoder ? launch_moments<CC, true>(a, which, st) : launch_moments<CC, false>(a, which, st);
  switch (a.C) {
    LGN_CASE(1) LGN_CASE(2) LGN_CASE(3) LGN_CASE(4) LGN_CASE(5) LGN_CASE(6) LGN_CASE(7) LGN_CASE(8)
    default: set_error("moments: C=%d unsupported (1..8)", a.C); return -1;
  }
#undef LGN_CASE
}

}  // namespace lgn
