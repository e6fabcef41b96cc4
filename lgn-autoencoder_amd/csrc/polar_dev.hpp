// lgn-autoencoder_amd/csrc/polar_dev.hpp -- the reference's polar frames of one particle and its phi wrap, for the anomaly scores
// (anomaly.hip) and the EMD score (emd.hip), which stage the same relative-polar frame bit for bit, the reconstruction analysis
// (analysis.hip), the jet images (stats.hip) and the assignment losses (assign_loss.hip).
//
// Floating-point contraction is OFF from here on, as in lsap_wave.hpp: the frames must round as the host computes them.
#pragma once
#pragma clang fp contract(off)

#include <math.h>

#include "common.hpp"

namespace lgn {

constexpr double POLAR_EPS = 1e-16;    // EPS_DEFAULT, get_eps() in fp64 and the eps defaults of the reference

// (x + pi) mod 2 pi - pi with the remainder of torch.remainder, numpy's and Python's %: its sign follows the divisor 2 pi > 0
__device__ __forceinline__ double wrap_phi(double x) {
  const double b = 2.0 * M_PI;
  double m = fmod(x + M_PI, b);
  if (m != 0.0 && m < 0.0) m += b;
  return m - M_PI;
}

// (px, py, pz) -> (pt, eta, phi).  The reference has three functions for it, and they are NOT one function: each puts its
// eps = 1e-16 somewhere else, and every user here is compared with its own to the last bits.
//
//                    restates                                        pt                        phi
//   p4_polar         get_p4_polar (anomaly_detection.py)             sqrt(px^2 + py^2)         atan2(py + eps, px + eps)
//   p_polar_tensor   get_p_polar_tensor (jet_analysis/utils.py)      sqrt(px^2 + py^2)         atan2(py + eps, px)
//   p_polar_loss     get_p_polar (losses/hungarian_mse/utils.py)     sqrt(px^2 + py^2 + eps)   atan2(py + eps, px + eps)
//
// that is, eps on px and py | on py only | on px and py and under the root; eta = asinh(pz / (pt + eps)) in all three.
__device__ __forceinline__ void p4_polar(double px, double py, double pz, double& pt, double& eta, double& phi) {
  pt = sqrt(px * px + py * py);
  eta = asinh(pz / (pt + POLAR_EPS));
  phi = atan2(py + POLAR_EPS, px + POLAR_EPS);
}
__device__ __forceinline__ void p_polar_tensor(double px, double py, double pz, double& pt, double& eta, double& phi) {
  pt = sqrt(px * px + py * py);
  eta = asinh(pz / (pt + POLAR_EPS));
  phi = atan2(py + POLAR_EPS, px);
}
__device__ __forceinline__ void p_polar_loss(double px, double py, double pz, double& pt, double& eta, double& phi) {
  pt = sqrt((px * px + py * py) + POLAR_EPS);
  eta = asinh(pz / (pt + POLAR_EPS));
  phi = atan2(py + POLAR_EPS, px + POLAR_EPS);
}

}  // namespace lgn
