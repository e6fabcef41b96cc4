// lgn-autoencoder_amd/csrc/assign_loss.hip -- the assignment losses of a jet, forward and backward in one pass: the reference's
// HungarianMSELoss (utils/losses/hungarian_mse/hungarian_mse.py:46-84 with utils.py next to it) and nn.MSELoss (utils/train.py:460-462,
// the same loss with the identity assignment), as the last stage of the training / evaluation step (dec_output_assign_loss: output
// mix -> get_real -> loss -> gradient back into the last level's vectors) and on their own (module API: lgn/losses.py).
//
//   frames (p, q) of (x = get_real(recon), t = target), D columns:
//     0 abs Cartesian  (E, px, py, pz), D = 4                       1 abs polar (pt, eta, phi), D = 3, get_p_polar: eps under the root
//     2 relative polar (pt / Jpt, eta - Jeta, phi - Jphi), J = polar of the TARGET's summed momenta for both sides, phi not wrapped
//     3 relative Cartesian of frame 2: (pt cos phi, pt cos phi (sic), pt sinh eta)
//   col = scipy's linear_sum_assignment of |p_i - q_j| (lsap_wave; no gradient through it); loss_part = scale sum_r |p[col[r]] - q[r]|^2
//   (the reference pairs p[col[r]] with q[r]); d loss / d p[col[r]] = 2 scale (p[col[r]] - q[r]), then through the frame's Jacobian.
//
// One workgroup of BLOCK threads per jet.  Wave 0 solves the assignment; the other waves meanwhile compute the per-row Jacobians
// d frame / d (px, py, pz) of the reconstruction side, which do not depend on it.
//
// The headers of the output stage are included first: their code (the output mix, get_real) contracts as it does in the Chamfer
// step's kernels, so the reconstruction is that step's bit for bit.  lsap_wave.hpp then switches contraction off for the rest of
// the file: an FMA in a cost or a reduced cost changes which column wins an exact tie.
#include "lds.hpp"
#include "net_dev.hpp"
#include "net.hpp"
#include "lsap_wave.hpp"
#include "polar_dev.hpp"     // p_polar_loss

namespace lgn {
namespace {

constexpr double EPS = 1e-16;          // get_eps() of the reference in fp64
enum : int { FR_ABS_CART = 0, FR_ABS_POLAR = 1, FR_REL_POLAR = 2, FR_REL_CART = 3 };

__host__ __device__ inline int frame_of(int kind, int abs_coord, int polar_coord) {
  if (kind == LGN_LOSS_MSE) return FR_ABS_CART;
  return abs_coord ? (polar_coord ? FR_ABS_POLAR : FR_ABS_CART) : (polar_coord ? FR_REL_POLAR : FR_REL_CART);
}

// LDS of the loss proper, in doubles: P [4][N] | Q [4][N] | J [N][9] | u [N] | jet [4] | col [N] ints
__host__ __device__ inline size_t core_doubles(int N) { return (size_t)18 * N + 4 + ((size_t)N + 1) / 2; }

struct Polar { double pt, eta, phi; };
__device__ __forceinline__ Polar polar_of(double px, double py, double pz) {
  Polar r;
  p_polar_loss(px, py, pz, r.pt, r.eta, r.phi);
  return r;
}

// x [N][4], tg [N][4] staged in LDS (synchronised); GRAD: gx [N][4] = d loss_part / d x is left in LDS, synchronised on return.
// Writes loss_part[b], assignment[b][N] and status[b] (both nullable) and returns the status (the same value on every thread):
// bit 0 -- a cost is NaN or -inf, bit 8 -- the matrix is infeasible; loss_part is then NaN, gx zero and the assignment -1.
template <int K, bool GRAD>
__device__ __forceinline__ int assign_loss_core(int N, int kind, int frame, double scale, const double* x, const double* tg, double* gx,
                                                 double* ws, size_t b, double* loss_part, int* assignment, int* status) {
  double* P = ws;                        // [4][N] frame of the reconstruction, component-major
  double* Q = P + 4 * N;                 // [4][N] frame of the target
  double* J = Q + 4 * N;                 // [N][3][3] d frame_c / d (px, py, pz) of the reconstruction rows
  double* u = J + 9 * N;                 // [N] row duals of the solver
  double* jet = u + N;                   // [4] summed target momenta (px, py, pz)
  int* col = reinterpret_cast<int*>(jet + 4);    // [N]
  __shared__ double red[4];
  __shared__ int st_s;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const bool rel = frame >= FR_REL_POLAR;
  if (rel && tid < 3) {                  // target.sum(-2), rows in order
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < N; ++r) s = s + tg[r * 4 + 1 + tid];
    jet[tid] = s;
  }
  if (tid == 0) st_s = 0;
  if (rel) __syncthreads();
  for (int t = tid; t < 2 * N; t += BLOCK) {
    const int side = t >= N, r = t - side * N;
    const double* row = (side ? tg : x) + 4 * r;
    double* f = (side ? Q : P) + r;
    if (frame == FR_ABS_CART) {
      f[0] = row[0], f[N] = row[1], f[2 * N] = row[2], f[3 * N] = row[3];
    } else {
      Polar p = polar_of(row[1], row[2], row[3]);
      if (rel) {
        const Polar jp = polar_of(jet[0], jet[1], jet[2]);
        p.pt = p.pt / jp.pt;
        p.eta = p.eta - jp.eta;
        p.phi = p.phi - jp.phi;
      }
      if (frame == FR_REL_CART) {
        const double c = p.pt * cos(p.phi);
        f[0] = c, f[N] = c, f[2 * N] = p.pt * sinh(p.eta);      // get_p_cartesian: py = pt cos(phi) as the reference has it
      } else {
        f[0] = p.pt, f[N] = p.eta, f[2 * N] = p.phi;
      }
      f[3 * N] = 0.0;
    }
  }
  __syncthreads();
  if (w == 0) {
    if (kind == LGN_LOSS_HUNGARIAN) {
      StagedCost<K> cf;
      cf.P = P;
      cf.N = N;
      cf.lorentz = false;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
#pragma unroll
        for (int c = 0; c < 4; ++c) cf.q[k][c] = j < N ? Q[c * N + j] : 0.0;
      }
      bool bad = false;
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (lane + 64 * k < N) bad |= bad_cost(cf(i, k));
      }
      int st = __ballot(bad) ? 1 : 0;
      if (!st && lsap_wave<K>(cf, N, u, col) != 0) st = 1 << 8;
      if (lane == 0) st_s = st;
    } else {
      for (int r = lane; r < N; r += 64) col[r] = r;
    }
  } else if (GRAD && frame != FR_ABS_CART) {
    for (int r = tid - 64; r < N; r += BLOCK - 64) {
      const double px = x[4 * r + 1], py = x[4 * r + 2], pz = x[4 * r + 3];
      const Polar p = polar_of(px, py, pz);
      const double ipe = p.pt + EPS, z = pz / ipe, a = py + EPS, c = px + EPS, h = a * a + c * c;
      double dpt[3] = {px / p.pt, py / p.pt, 0.0};
      const double de = 1.0 / sqrt(z * z + 1.0), dz = -pz / (ipe * ipe);
      const double deta[3] = {de * (dz * dpt[0]), de * (dz * dpt[1]), de / ipe};
      const double dphi[3] = {-a / h, c / h, 0.0};
      double* Jr = J + 9 * r;
      if (rel) {
        const Polar jp = polar_of(jet[0], jet[1], jet[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) dpt[k] = dpt[k] / jp.pt;
        if (frame == FR_REL_CART) {
          const double ptr = p.pt / jp.pt, er = p.eta - jp.eta, pr = p.phi - jp.phi;
          const double cs = cos(pr), sn = sin(pr), sh = sinh(er), ch = cosh(er);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double d0 = cs * dpt[k] - (ptr * sn) * dphi[k];
            Jr[k] = d0;
            Jr[3 + k] = d0;
            Jr[6 + k] = sh * dpt[k] + (ptr * ch) * deta[k];
          }
          continue;
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Jr[k] = dpt[k];
        Jr[3 + k] = deta[k];
        Jr[6 + k] = dphi[k];
      }
    }
  }
  __syncthreads();
  const int st = st_s;
  double acc = 0.0;
  for (int r = tid; r < N; r += BLOCK) {
    const int s = st ? r : col[r];
    const double d0 = P[s] - Q[r], d1 = P[N + s] - Q[N + r], d2 = P[2 * N + s] - Q[2 * N + r], d3 = P[3 * N + s] - Q[3 * N + r];
    acc = acc + sq4(d0, d1, d2, d3);
    if (GRAD) {
      const double g0 = 2.0 * scale * d0, g1 = 2.0 * scale * d1, g2 = 2.0 * scale * d2, g3 = 2.0 * scale * d3;
      double* o = gx + 4 * s;              // col is a permutation: every row of gx is written exactly once
      if (st) {
        o[0] = o[1] = o[2] = o[3] = 0.0;
      } else if (frame == FR_ABS_CART) {
        o[0] = g0, o[1] = g1, o[2] = g2, o[3] = g3;
      } else {
        const double* Js = J + 9 * s;
        o[0] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[1 + k] = (g0 * Js[k] + g1 * Js[3 + k]) + g2 * Js[6 + k];
      }
    }
    if (assignment) assignment[b * N + r] = st ? -1 : s;
  }
  acc = block_sum(acc, red);               // (synchronises: gx is complete for the caller)
  if (tid == 0) {
    loss_part[b] = st ? NAN : acc * scale;
    if (status) status[b] = st;
  }
  return st;
}

// ---- the loss on its own: x, y [B][N][4] -> loss_part [B], gx [B][N][4] ------------------------------------------------------
template <int K>
__global__ __launch_bounds__(BLOCK) void hungarian_mse_kernel(int N, const double* __restrict__ x, const double* __restrict__ y, int kind,
                                                             int frame, double scale, double* __restrict__ loss_part,
                                                             double* __restrict__ gx_out, int* __restrict__ assignment,
                                                             int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* xs = reinterpret_cast<double*>(smem_raw);
  double* ts = xs + 4 * N;
  double* gx = ts + 4 * N;
  const size_t b = blockIdx.x, j4 = b * (size_t)N * 4;
  for (int e = threadIdx.x; e < 4 * N; e += BLOCK) {
    xs[e] = x[j4 + e];
    ts[e] = y[j4 + e];
  }
  __syncthreads();
  assign_loss_core<K, true>(N, kind, frame, scale, xs, ts, gx, gx + 4 * N, b, loss_part, assignment, status);
  for (int e = threadIdx.x; e < 4 * N; e += BLOCK) gx_out[j4 + e] = gx[e];
}

// ---- decoder output + get_real + assignment loss, forward and backward (GRAD) or forward only, as dec_output_loss_body is for Chamfer --
// LDS: x [N][4] | tg [N][4] | gx [N][4] | ycl [N][8] | vl [N*C][8] | tmp [N*C][2] | wol [2C] | the loss's own block (core_doubles)
template <int K, bool GRAD>
__global__ __launch_bounds__(BLOCK) void dec_output_assign_loss_kernel(int B, int N, int C, const double* __restrict__ v,
                                                                      const double* __restrict__ wo1, const double* __restrict__ target,
                                                                      int method, int kind, int frame, double scale, double* recon,
                                                                      double* loss_part, double* g_v, double* part, int* assignment,
                                                                      int* status) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  DecOutLds s;
  s.x = reinterpret_cast<double*>(smem_raw);
  s.tg = s.x + N * 4;
  s.gx = s.tg + N * 4;
  s.ycl = s.gx + N * 4;
  s.vl = s.ycl + N * 8;
  s.tmp = s.vl + N * C * 8;
  s.wol = s.tmp + N * C * 2;
  dec_out_forward<GRAD>(B, N, C, v, wo1, target, method, recon, s);
  const int st = assign_loss_core<K, GRAD>(N, kind, frame, scale, s.x, s.tg, s.gx, s.wol + 2 * C, blockIdx.x, loss_part, assignment, status);
  if constexpr (GRAD) {
    if (st) {      // a flagged jet hands on exact zeros: through the backward its (possibly NaN) vectors would turn 0 * NaN into NaN
      const size_t pl = (size_t)B * N * C * 4, jc = (size_t)blockIdx.x * N * C * 4;
      for (int e = threadIdx.x; e < N * C * 4; e += BLOCK) g_v[jc + e] = g_v[pl + jc + e] = 0.0;
      for (int e = threadIdx.x; e < 2 * C; e += BLOCK) part[(size_t)blockIdx.x * 2 * C + e] = 0.0;
    } else {
      dec_out_backward(B, N, C, method, g_v, part, s);
    }
  }
}

inline size_t stage_bytes(int N, int C) {
  return sizeof(double) * ((size_t)N * 20 + (size_t)N * C * 10 + 2 * (size_t)C + core_doubles(N));
}
inline size_t alone_bytes(int N) { return sizeof(double) * ((size_t)N * 12 + core_doubles(N)); }

template <int K, bool GRAD>
int launch_stage(int B, int N, int C, const double* v, const double* wo1, const double* target, int method, const AssignLoss& al,
                 double* recon, double* loss_part, double* g_v, double* part, hipStream_t st) {
  return lds_launch(dec_output_assign_loss_kernel<K, GRAD>, "dec_output_assign_loss", dim3(B), dim3(BLOCK), stage_bytes(N, C), st, B, N, C, v, wo1, target,
                    method, al.kind, frame_of(al.kind, al.abs_coord, al.polar_coord), al.scale, recon, loss_part, g_v, part, al.assignment, al.status);
}

template <int K>
int launch_alone(int B, int N, const double* x, const double* y, const AssignLoss& al, double* loss_part, double* gx, hipStream_t st) {
  return lds_launch(hungarian_mse_kernel<K>, "hungarian_mse", dim3(B), dim3(BLOCK), alone_bytes(N), st, N, x, y, al.kind,
                    frame_of(al.kind, al.abs_coord, al.polar_coord), al.scale, loss_part, gx, al.assignment, al.status);
}

}  // namespace

size_t assign_loss_lds_bytes(int N, int C) { return stage_bytes(N, C); }

int check_assign_loss(const AssignLoss& al, int N) {
  LGN_CHECK_ARG(al.kind == LGN_LOSS_MSE || al.kind == LGN_LOSS_HUNGARIAN, "loss: kind=%d is not LGN_LOSS_MSE / LGN_LOSS_HUNGARIAN", al.kind);
  LGN_CHECK_ARG(al.scale > 0.0 && al.scale < INFINITY, "loss: scale=%g must be positive and finite (1 / (batch N D))", al.scale);
  LGN_CHECK_ARG(N >= 1 && N <= LSAP_NMAX, "loss: N = %d outside 1 .. %d", N, LSAP_NMAX);
  return 0;
}

int dec_output_assign_loss(int B, int N, int C, const double* v, const double* wo1, const double* target, int method, const AssignLoss& al,
                           double* recon, double* loss_part, double* g_v, double* part, hipStream_t st) {
  if (int rc = check_assign_loss(al, N)) return rc;
  if (N <= 64) return launch_stage<1, true>(B, N, C, v, wo1, target, method, al, recon, loss_part, g_v, part, st);
  if (N <= 128) return launch_stage<2, true>(B, N, C, v, wo1, target, method, al, recon, loss_part, g_v, part, st);
  return launch_stage<3, true>(B, N, C, v, wo1, target, method, al, recon, loss_part, g_v, part, st);
}

int dec_output_assign_eval(int B, int N, int C, const double* v, const double* wo1, const double* target, int method, const AssignLoss& al,
                           double* recon_real, double* loss_part, hipStream_t st) {
  if (int rc = check_assign_loss(al, N)) return rc;
  if (N <= 64) return launch_stage<1, false>(B, N, C, v, wo1, target, method, al, recon_real, loss_part, nullptr, nullptr, st);
  if (N <= 128) return launch_stage<2, false>(B, N, C, v, wo1, target, method, al, recon_real, loss_part, nullptr, nullptr, st);
  return launch_stage<3, false>(B, N, C, v, wo1, target, method, al, recon_real, loss_part, nullptr, nullptr, st);
}

int hungarian_mse(int B, int N, const double* x, const double* y, const AssignLoss& al, double* loss_part, double* gx, hipStream_t st) {
  if (int rc = check_assign_loss(al, N)) return rc;
  if (N <= 64) return launch_alone<1>(B, N, x, y, al, loss_part, gx, st);
  if (N <= 128) return launch_alone<2>(B, N, x, y, al, loss_part, gx, st);
  return launch_alone<3>(B, N, x, y, al, loss_part, gx, st);
}

}  // namespace lgn
