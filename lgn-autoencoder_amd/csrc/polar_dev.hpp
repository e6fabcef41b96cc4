// lgn-autoencoder_amd/csrc/polar_dev.hpp -- the reference's polar frame of one particle (get_p4_polar) and its phi wrap (get_polar_rel),
// shared by the anomaly scores (anomaly.hip) and the EMD score (emd.hip): both stage the same relative-polar frame, bit for bit.
//
// Floating-point contraction is OFF from here on, as in lsap_wave.hpp: the frames must round as the host computes them.
#pragma once
#pragma clang fp contract(off)

#include <math.h>

#include "common.hpp"

namespace lgn {

constexpr double POLAR_EPS = 1e-16;    // EPS_DEFAULT of the reference

// the reference's torch.remainder(x + pi, 2 pi) - pi (float remainder: the sign follows the divisor)
__device__ __forceinline__ double wrap_phi(double x) {
  const double b = 2.0 * M_PI;
  double m = fmod(x + M_PI, b);
  if (m != 0.0 && ((m < 0.0) != (b < 0.0))) m += b;
  return m - M_PI;
}
__device__ __forceinline__ void polar(double px, double py, double pz, double& pT, double& eta, double& phi) {
  pT = sqrt(px * px + py * py);
  eta = asinh(pz / (pT + POLAR_EPS));
  phi = atan2(py + POLAR_EPS, px + POLAR_EPS);
}

}  // namespace lgn
