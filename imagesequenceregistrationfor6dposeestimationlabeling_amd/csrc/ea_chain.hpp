// ea_chain.hpp — the weight chain of a ray (pren.py:338-365 with surface_thickness = 1, _shifted_cumprod's default shift),
// written once for every march: csrc/field_density.hpp's march_ray and march_ray_back, csrc/field_radiance.hpp's RayState
// and csrc/ea_grad.hpp's backward.  Compiled for host and device, and a plain C++ compiler can include it.  Built with
// -ffp-contract=off: host and device give the same bits.
//     c_k = absorbance(rho_k);  w_k = c_k * T_k;  T_0 = 1, T_{k+1} = T_k * (1 - c_k)      (sequential f32, k ascending)
//     depth = max_k(len_k * w_k), the maximum of the PRODUCTS starting from the first one (torch.max: a NaN product makes
//         the depth NaN; with negative lengths the depth can be negative or -0);  hit = any(w_k != 0)
#pragma once
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace ea {

// c_k.  threshold >= 0 (thresholdMode): 1 above the threshold, else 0 (a NaN density: 0), so that w is one-hot at the first
// hit; a sample that was not evaluated counts as below (a caller may stop evaluating a ray after its first hit: the later
// c_k are multiplied by T = 0 whatever they are).  The reference writes (1.0 + 1e-10) - c, which is 1 - c in f32: the f64
// scalar rounds to 1.0f.  threshold < 0: the density itself.
ISR_HD float absorbance(float rho, float threshold, bool evaluated = true) {
  if (threshold >= 0.f) return evaluated && rho > threshold ? 1.0f : 0.0f;
  return rho;
}

struct WeightChain {
  float T, m;
  int32_t any;
  ISR_HD void start() {
    T = 1.0f;
    m = 0.f;
    any = 0;
  }
  // w_k into the maximum and the hit flag
  ISR_HD void take(int k, float len, float w) {
    if (w != 0.f) any = 1;
    const float v = len * w;
    if (k == 0) m = v;
    else if (m == m && (v != v || v > m)) m = v;      // a NaN stays
  }
  // sample k, k ascending -> w_k
  ISR_HD float step(int k, float len, float c) {
    const float w = c * T;
    T = T * (1.0f - c);
    take(k, len, w);
    return w;
  }
};

}  // namespace ea
}  // namespace isr
