// ea_grad.hip — the backward of isr_ea_march on the device (ea_grad.hpp states the rule): the entries of
// include/isr_ea_grad.h.  One launch, no workspace, no float atomics, no call synchronises.
//
// A workgroup of kThreads owns rays_per_group(P) whole rays (63 at P = 64, 31 at P = 128, 15 at P = 256, one from P = 2 048
// on) and keeps three rows of P floats per ray in LDS — c_k, T_k and g_k — a ray's rows P | 1 floats from the next ray's.
//   1. all lanes, one (ray, k) pair each, pairs in memory order: c_k from the density, and g_k from dweights and the F
//      features of the pair (consecutive lanes read addresses F floats apart; at F = 3 a wave's three loads cover 768
//      contiguous bytes between them).
//   2. lane r of the first wave walks ray r: T_k on the way up, then ddensities[k] over g_k on the way down.  The lanes
//      walk in step and their rows are an odd stride apart, so they meet no bank conflict.
//   3. all lanes write ddensities in memory order from LDS, then dfeatures, one element each in memory order:
//      (c_k * T_k) * dimage[ch].
// dimage, F + 1 floats a ray, is read through the cache where it is needed.  A workgroup takes further groups of rays in a
// grid-stride loop, so the grid stays small whatever N is.
#include "ea_grad.hpp"
#include "isr_common.hpp"

#include "../../include/isr_ea_grad.h"

#include <algorithm>

namespace {

using namespace isr::ea_grad;

constexpr long kMaxBlocks = 1 << 20;

__global__ __launch_bounds__(kThreads) void ea_grad_kernel(const float* __restrict__ rho, const float* __restrict__ features, int N,
                                                           int P, int F, int R, long groups, float threshold,
                                                           const float* __restrict__ dimage, const float* __restrict__ dweights,
                                                           float* __restrict__ ddensities, float* __restrict__ dfeatures) {
  __shared__ float cs[kRowFloats], Ts[kRowFloats], gs[kRowFloats];
  const int S = row_stride(P);
  const bool chain = ddensities && threshold < 0.f;      // the adjoint runs: otherwise ddensities, if wanted, is +0
  for (long group = blockIdx.x; group < groups; group += gridDim.x) {
    const long ray0 = group * R;
    const int rays = (int)min((long)R, (long)N - ray0);
    const int pairs = rays * P;                          // at most kRowFloats
    const size_t q0 = (size_t)ray0 * P;
    for (int i = threadIdx.x; i < pairs; i += kThreads) {
      const int r = i / P, k = i - r * P;
      const size_t q = q0 + i;
      cs[r * S + k] = absorbance(rho[q], threshold);
      if (chain) gs[r * S + k] = upstream(dimage + (size_t)(ray0 + r) * (F + 1), features + q * F, F, dweights ? dweights[q] : 0.f);
    }
    __syncthreads();
    if ((int)threadIdx.x < rays) {
      const int r = threadIdx.x;
      transmittance(P, cs + r * S, Ts + r * S);
      if (chain) adjoint(P, cs + r * S, Ts + r * S, dimage[(size_t)(ray0 + r) * (F + 1) + F], gs + r * S);
    }
    __syncthreads();
    if (ddensities)
      for (int i = threadIdx.x; i < pairs; i += kThreads) {
        const int r = i / P, k = i - r * P;
        ddensities[q0 + i] = chain ? gs[r * S + k] : 0.f;
      }
    if (dfeatures) {
      const int elems = pairs * F;                       // at most kRowFloats * kMaxF
      for (int e = threadIdx.x; e < elems; e += kThreads) {
        const int i = e / F, ch = e - i * F, r = i / P, k = i - r * P;
        dfeatures[q0 * F + e] = feature_grad(cs[r * S + k], Ts[r * S + k], dimage[(size_t)(ray0 + r) * (F + 1) + ch]);
      }
    }
    __syncthreads();                                     // the rows are free for the next group
  }
}

int check(const char* who, const float* densities, const float* features, int N, int P, int F, float threshold, const float* dimage,
          const float* ddensities, const float* dfeatures) {
  const char* wrong = check_call(densities, features, N, P, F, threshold, dimage, ddensities, dfeatures);
  ISR_REQUIRE(!wrong, "%s: %s (N %d, P %d, F %d)", who, wrong, N, P, F);
  return ISR_OK;
}

}  // namespace

extern "C" int isr_ea_march_backward(const float* densities, const float* features, int N, int P, int F, float threshold,
                                     const float* dimage, const float* dweights, float* ddensities, float* dfeatures,
                                     isr_stream_t stream) {
  if (int rc = check("isr_ea_march_backward", densities, features, N, P, F, threshold, dimage, ddensities, dfeatures)) return rc;
  if (N == 0) return ISR_OK;
  const int R = rays_per_group(P);
  const long groups = ((long)N + R - 1) / R;
  ea_grad_kernel<<<(unsigned)std::min(groups, kMaxBlocks), kThreads, 0, isr::as_stream(stream)>>>(
      densities, features, N, P, F, R, groups, threshold, dimage, dweights, ddensities, dfeatures);
  ISR_CHECK_LAUNCH("ea_grad_kernel");
  return ISR_OK;
}

extern "C" int isr_ea_march_backward_host(const float* densities, const float* features, int N, int P, int F, float threshold,
                                          const float* dimage, const float* dweights, float* ddensities, float* dfeatures) {
  if (int rc = check("isr_ea_march_backward_host", densities, features, N, P, F, threshold, dimage, ddensities, dfeatures)) return rc;
  backward_host(densities, features, N, P, F, threshold, dimage, dweights, ddensities, dfeatures);
  return ISR_OK;
}

extern "C" int isr_ea_grad_geometry(int which) {
  return which == 0 ? kThreads : which == 1 ? kMaxGroupRays : which == 2 ? kRowFloats : -1;
}

extern "C" int isr_ea_grad_rays_per_group(int P) { return P >= 1 && P <= kMaxP ? rays_per_group(P) : -1; }
