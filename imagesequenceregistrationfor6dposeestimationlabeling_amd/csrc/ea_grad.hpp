// ea_grad.hpp — the backward of the emission-absorption march: the rule of include/isr_ea_grad.h, written once and compiled
// for host and device.  csrc/ea_grad.hip holds the kernel and the C entries; a plain C++ compiler can include this header too
// (tools/ea_grad_host_check.cpp).  Every fused multiply-add is written out and everything is built with -ffp-contract=off:
// host and device give the same bits.
//
// What this replaces: the chain autograd runs behind pren.py:362-367 when trainNerfFine.py:353 calls loss.backward() — the
// backward of cumprod, which divides by 1 - c and takes a special path where that is exactly 0, and a few dozen launches
// over (N, P) and (N, P, F) temporaries.  Here the adjoint of the transmittance is a recurrence with no division.
//
// The forward chain is csrc/ea_chain.hpp's, w_k = c_k * T_k, T_{k+1} = T_k * (1 - c_k) with its absorbance; transmittance
// below keeps every T_k, which the backward needs and the forward's running state does not.  tests/test_ea_grad_cpu.py holds
// the two to the same bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ea_chain.hpp"

namespace isr {
namespace ea_grad {

constexpr int kMaxP = 4096;           // isr_ea_march's limits (csrc/field_density.hpp, csrc/field_radiance.hpp)
constexpr int kMaxF = 64;
constexpr int kThreads = 256;         // threads of a workgroup
constexpr int kMaxGroupRays = 64;     // rays one workgroup owns at most: one wave runs their chains, a lane each
constexpr int kRowFloats = 4097;      // floats of LDS per array: (rays of a workgroup) * (P | 1) stays inside

// The LDS row of a ray is P | 1 floats apart from the next: an odd stride, so the lanes that walk their rays in step
// touch different banks.
ISR_HD int row_stride(int P) { return P | 1; }
ISR_HD int rays_per_group(int P) {
  const int r = kRowFloats / row_stride(P);
  return r < 1 ? 1 : (r > kMaxGroupRays ? kMaxGroupRays : r);
}

// Returns null, or what is wrong with the call.
inline const char* check_call(const void* densities, const void* features, int N, int P, int F, float threshold,
                              const void* dimage, const void* ddensities, const void* dfeatures) {
  if (N < 0) return "N < 0";
  if (P < 1 || P > kMaxP) return "P outside 1..4096";
  if (F < 1 || F > kMaxF) return "F outside 1..64";
  if (!(threshold == threshold)) return "threshold is NaN";
  if (N == 0) return nullptr;                       // no rows: the arrays may be null, as for isr_ea_march
  if (!ddensities && !dfeatures) return "both outputs are null";
  if (!(densities && features && dimage)) return "null pointer";
  return nullptr;
}

using ea::absorbance;      // c_k: the density itself, or in threshold mode a step function of it

// g_k, everything that reaches w_k from above: dweights[k], then the image's channels in ascending order
ISR_HD float upstream(const float* dimage, const float* feat, int F, float dweight) {
  float g = dweight;
  for (int ch = 0; ch < F; ++ch) g = __builtin_fmaf(dimage[ch], feat[ch], g);
  return g;
}

// T[k] = T_k for k in [0, P): the forward's chain.  c and T do not overlap, and the loops of both walks are unrolled, so that
// on the device a batch of LDS reads is in flight while the chain, one multiplication a sample, runs in registers.
ISR_HD void transmittance(int P, const float* __restrict__ c, float* __restrict__ T) {
  float t = 1.0f;
#pragma unroll 8
  for (int k = 0; k < P; ++k) {
    T[k] = t;
    t = t * (1.0f - c[k]);
  }
}

// The way down: g[k] holds g_k on entry and ddensities[k] on return.  dopacity = dimage[F]; the opacity is 1 - T_P.
ISR_HD void adjoint(int P, const float* __restrict__ c, const float* __restrict__ T, float dopacity, float* __restrict__ g) {
  float a = -dopacity;
#pragma unroll 8
  for (int k = P - 1; k >= 0; --k) {
    const float gk = g[k], ck = c[k];
    g[k] = T[k] * (gk - a);
    a = __builtin_fmaf(gk, ck, a * (1.0f - ck));
  }
}

// dfeatures[k, ch] from the forward's weight of sample k
ISR_HD float feature_grad(float c, float T, float dimage_ch) { return (c * T) * dimage_ch; }

// ---- host build: the definition the kernel is compared with.  c, T: P floats of scratch each.
inline void backward_ray_host(int P, int F, const float* rho, const float* features, float threshold, const float* dimage,
                              const float* dweights, float* ddensities, float* dfeatures, float* c, float* T) {
  for (int k = 0; k < P; ++k) c[k] = absorbance(rho[k], threshold);
  transmittance(P, c, T);
  if (dfeatures)
    for (int k = 0; k < P; ++k)
      for (int ch = 0; ch < F; ++ch) dfeatures[(size_t)k * F + ch] = feature_grad(c[k], T[k], dimage[ch]);
  if (!ddensities) return;
  if (threshold >= 0.f) {
    for (int k = 0; k < P; ++k) ddensities[k] = 0.f;
    return;
  }
  for (int k = 0; k < P; ++k) ddensities[k] = upstream(dimage, features + (size_t)k * F, F, dweights ? dweights[k] : 0.f);
  adjoint(P, c, T, dimage[F], ddensities);
}

inline void backward_host(const float* rho, const float* features, int N, int P, int F, float threshold, const float* dimage,
                          const float* dweights, float* ddensities, float* dfeatures) {
  std::vector<float> c((size_t)P), T((size_t)P);
  for (long ray = 0; ray < N; ++ray) {
    const size_t q = (size_t)ray * P;
    backward_ray_host(P, F, rho + q, features + q * F, threshold, dimage + (size_t)ray * (F + 1), dweights ? dweights + q : nullptr,
                      ddensities ? ddensities + q : nullptr, dfeatures ? dfeatures + q * F : nullptr, c.data(), T.data());
  }
}

}  // namespace ea_grad
}  // namespace isr
