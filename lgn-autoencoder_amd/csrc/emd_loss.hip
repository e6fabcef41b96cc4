// lgn-autoencoder_amd/csrc/emd_loss.hip -- the energy mover's distance as the last stage of the training / evaluation step: lgn.losses.EMDLoss
// and HybridLoss inside the whole-step calls (LGN_LOSS_EMD, lgn_emd_loss_desc of include/lgn_amd.h).  The sandwich of assign_loss.hip
// around the solver of emd_wave.hpp: output mix -> get_real -> EMD of (x, target) on their relative-polar frames under an lgn_emd_opts
// -> its closed-form gradient d loss / d x -> back into the last level's vectors.  Entry point of its own: lgn_emd_loss_lds_bytes.
//
// One workgroup of BLOCK threads per jet.  After dec_out_forward, x = get_real(reconstruction) and the target sit in LDS; wave 0 does for
// them what one wavefront of emd_grad_opts_kernel<REL> does for a pair in global memory, with the same device functions (emd_dev.hpp):
// stages the two frames, solves, and leaves (g_w, g_y, g_phi) carried back to the Cartesian rows in gx [N][4] (E column 0).  The value
// is therefore lgn_emd_relative_opts_f64's of (x, target) bit for bit -- at default options lgn_emd_relative_f64's, whose kernel makes
// the same roundings.  The other waves wait at the barrier: nothing of the gradient is independent of the flow.  The flow matrix lives
// in LDS only, so the step's workspace does not depend on the loss; a shape whose LDS does not fit is refused at plan time.
//
// The hybrid loss (chamfer_weight > 0, ACC): the step's Chamfer loss has run before this launch, with chamfer_weight as its gradient
// scale.  The stage recomputes x from the last level's vectors (the same bits) and ADDS its g_v, its dWo1 partial row and its term of
// loss_part[b] to what the Chamfer stage wrote -- dec_out_backward<ACC>, the owning thread's read-modify-write, no atomics.
//
// The headers of the output stage are included first: their code (the output mix, get_real) contracts as it does in the Chamfer
// step's kernels, so the reconstruction is that step's bit for bit.  emd_dev.hpp then switches contraction off for the rest of the
// file: costs, frames and sums round one operation at a time, as emd.hip's do.
#include "lds.hpp"
#include "net_dev.hpp"
#include "net.hpp"
#include "emd_plan.hpp"
#include "emd_dev.hpp"

namespace lgn {
namespace {

// LDS of the stage: the output stage's block -- x [N][4] | tg [N][4] | gx [N][4] | ycl [N][8] | vl [N*C][8] | tmp [N*C][2] | wol [2C] --
// then one wavefront's EMD block in emd_kernel's order (emd_plan.hpp: emd_lds_doubles(N, N, true) doubles, two int arrays of N + 1).
// Between the solve and the backward, tmp[0] and tmp[1] carry the value and the status from wave 0 to the workgroup.
struct EmdLossLds {
  size_t x, tg, gx, ycl, vl, tmp, wol, emd, ints, bytes;
  __host__ __device__ EmdLossLds(int N, int C) {
    LdsCarve c;
    x = c.take<double>((size_t)N * 4);
    tg = c.take<double>((size_t)N * 4);
    gx = c.take<double>((size_t)N * 4);
    ycl = c.take<double>((size_t)N * 8);
    vl = c.take<double>((size_t)N * C * 8);
    tmp = c.take<double>((size_t)N * C * 2);
    wol = c.take<double>((size_t)2 * C);
    emd = c.take<double>((size_t)emd_lds_doubles(N, N, true));
    ints = c.take<int>((size_t)2 * (N + 1));
    bytes = c.off;
  }
};
static_assert(emd_lds_total(7, 7, true) == 8 * emd_lds_doubles(7, 7, true) + 4 * 2 * (7 + 1), "emd_plan.hpp counts the two int arrays");

template <int K, bool GRAD, bool ACC>
__global__ __launch_bounds__(BLOCK) void dec_output_emd_loss_kernel(int B, int N, int C, const double* __restrict__ v,
                                                                   const double* __restrict__ wo1, const double* __restrict__ target,
                                                                   int method, lgn_emd_opts opt, double scale, double chamfer_weight,
                                                                   double* recon, double* loss_part, double* g_v, double* part,
                                                                   int* status) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const EmdLossLds L(N, C);
  DecOutLds s;
  s.x = lds_at<double>(smem_raw, L.x);
  s.tg = lds_at<double>(smem_raw, L.tg);
  s.gx = lds_at<double>(smem_raw, L.gx);
  s.ycl = lds_at<double>(smem_raw, L.ycl);
  s.vl = lds_at<double>(smem_raw, L.vl);
  s.tmp = lds_at<double>(smem_raw, L.tmp);
  s.wol = lds_at<double>(smem_raw, L.wol);
  dec_out_forward<GRAD>(B, N, C, v, wo1, target, method, recon, s);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x, rows = N + 1;
    EmdRows rs;
    rs.u = lds_at<double>(smem_raw, L.emd);
    rs.sup = rs.u + rows;
    rs.dist = rs.sup + rows;
    double* ry = rs.dist + rows;
    double* rphi = ry + rows;
    double* jet = rphi + rows;             // [2][4] jet 4-vectors
    FlowLds F;
    F.f = jet + 8;                         // [rows][rows]
    F.ld = rows;
    rs.pred = lds_at<int>(smem_raw, L.ints);
    rs.vis = rs.pred + rows;
    EmdOptCost<K> cf;
    cf.y = ry, cf.phi = rphi, cf.n = N, cf.m = N, cf.lane = lane;
    cf.options(opt);
    double dem[K], vc[K];
    bool bad = false;
    double p0 = 0.0, p1 = 0.0;
    emd_stage_rel<K>(s.x, s.tg, N, N, lane, rs.sup, ry, rphi, jet, dem, cf.qy, cf.qphi, bad, p0, p1);
    const bool norm = opt.norm;
    double T0, T1, score;
    const int st = emd_solve_opts<K>(cf, rs, F, norm, GRAD, bad, p0, p1, dem, vc, T0, T1, score);
    if (GRAD && !st) emd_opt_gradients<K, FlowLds, true>(cf, rs, F, vc, st, norm, T0, T1, s.x, s.tg, jet, s.gx, nullptr);
    if (lane == 0) s.tmp[0] = score, s.tmp[1] = (double)st;
  }
  __syncthreads();
  const double score = s.tmp[0];
  const int st = (int)s.tmp[1];
  __syncthreads();                           // (tmp is the backward's again)
  const size_t b = blockIdx.x;
  if (threadIdx.x == 0) {
    const double term = score * scale;
    loss_part[b] = st ? NAN : (ACC ? chamfer_weight * loss_part[b] + term : term);
    if (status) status[b] = st;
  }
  if constexpr (GRAD) {
    if (st) {      // a flagged jet hands on exact zeros (assign_loss.hip); accumulating, it leaves the Chamfer contribution in place
      if constexpr (!ACC) {
        const size_t pl = (size_t)B * N * C * 4, jc = b * N * C * 4;
        for (int e = threadIdx.x; e < N * C * 4; e += BLOCK) g_v[jc + e] = g_v[pl + jc + e] = 0.0;
        for (int e = threadIdx.x; e < 2 * C; e += BLOCK) part[b * 2 * C + e] = 0.0;
      }
    } else {
      if (scale != 1.0) {                    // (uniform over the grid)
        for (int e = threadIdx.x; e < N * 4; e += BLOCK) s.gx[e] = s.gx[e] * scale;
        __syncthreads();
      }
      dec_out_backward<ACC>(B, N, C, method, g_v, part, s);
    }
  }
}

struct StageArgs {
  int B, N, C;
  const double *v, *wo1, *target;
  int method;
  double *recon, *loss_part, *g_v, *part;
};

template <int K, bool GRAD, bool ACC>
int launch_kga(const StageArgs& a, const EmdLoss& el, hipStream_t st) {
  return lds_launch(dec_output_emd_loss_kernel<K, GRAD, ACC>, "dec_output_emd_loss", dim3(a.B), dim3(BLOCK), EmdLossLds(a.N, a.C).bytes, st,
                    a.B, a.N, a.C, a.v, a.wo1, a.target, a.method, el.opts, el.scale, el.chamfer_weight, a.recon, a.loss_part, a.g_v,
                    a.part, el.status);
}

template <bool GRAD>
int launch_stage(const StageArgs& a, const EmdLoss& el, hipStream_t st) {
  if (int rc = check_emd_loss(el, a.N)) return rc;
  const int K = (a.N + 1 + 63) / 64;       // solver columns per lane, the fictitious node counted
  const bool acc = el.chamfer_weight > 0.0;
#define LGN_EMD_CASE(KK) \
  if (K == KK) return acc ? launch_kga<KK, GRAD, true>(a, el, st) : launch_kga<KK, GRAD, false>(a, el, st);
  LGN_EMD_CASE(1)
  LGN_EMD_CASE(2)
  LGN_EMD_CASE(3)
#undef LGN_EMD_CASE
  set_error("dec_output_emd_loss: N = %d needs more than three columns per lane", a.N);
  return -1;
}

}  // namespace

long long emd_loss_lds_bytes(int N, int C) {
  if (N < 1 || C < 1) return -1;
  return (long long)EmdLossLds(N, C).bytes;
}

int check_emd_loss(const EmdLoss& el, int N) {
  LGN_CHECK_ARG(el.opts.R > 0.0 && el.opts.R < INFINITY, "loss: EMD R = %g (need a finite R > 0)", el.opts.R);
  LGN_CHECK_ARG(el.opts.beta > 0.0 && el.opts.beta < INFINITY, "loss: EMD beta = %g (need a finite beta > 0)", el.opts.beta);
  LGN_CHECK_ARG(el.chamfer_weight >= 0.0 && el.chamfer_weight < INFINITY, "loss: chamfer_weight = %g (need a finite weight >= 0)",
                el.chamfer_weight);
  LGN_CHECK_ARG(el.scale > 0.0 && el.scale < INFINITY, "loss: scale=%g must be positive and finite (the weight of the EMD term)", el.scale);
  LGN_CHECK_ARG(N >= 1 && N <= LGN_EMD_NMAX, "loss: N = %d outside 1 .. %d", N, LGN_EMD_NMAX);
  return 0;
}

int dec_output_emd_loss(int B, int N, int C, const double* v, const double* wo1, const double* target, int method, const EmdLoss& el,
                        double* recon, double* loss_part, double* g_v, double* part, hipStream_t st) {
  return launch_stage<true>(StageArgs{B, N, C, v, wo1, target, method, recon, loss_part, g_v, part}, el, st);
}

int dec_output_emd_eval(int B, int N, int C, const double* v, const double* wo1, const double* target, int method, const EmdLoss& el,
                        double* recon_real, double* loss_part, hipStream_t st) {
  return launch_stage<false>(StageArgs{B, N, C, v, wo1, target, method, recon_real, loss_part, nullptr, nullptr}, el, st);
}

}  // namespace lgn

extern "C" long long lgn_emd_loss_lds_bytes(int N, int C) {
  const long long need = lgn::emd_loss_lds_bytes(N, C);
  if (need < 0) lgn::set_error("emd_loss_lds_bytes: N = %d, C = %d (need N >= 1, C >= 1)", N, C);
  return need;
}
