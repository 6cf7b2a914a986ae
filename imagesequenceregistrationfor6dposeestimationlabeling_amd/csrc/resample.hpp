// resample.hpp — the fine pass's depths: inverse-CDF samples of a ray's coarse weights (pytorch3d's sample_pdf) and the sorted
// row of pren.py:427-457 (ProbabilisticRaysampler.forward), written once and compiled for host and device.
// csrc/resample.hip holds the kernel and the C entries, include/isr_resample.h states every rule; a plain C++ compiler can
// include this header too (tools/resample_host_check.cpp).  Only + - * / in f32 and f64, no fused multiply-add except
// linspace's explicit fmaf, and everything is built with -ffp-contract=off: host and device give the same bits.
//
// UNPINNED: the rule of sample_pdf is pytorch3d's sample_pdf_python AS FAR AS IT IS KNOWN FROM MEMORY (pytorch3d is not
// available to compare against), and the f64 running sums are torch's CPU sum / cumsum rule as far as it is known.
//
// NON-FINITE INPUT is not refused (nothing synchronises); a row's output depends on that row alone.  A NaN weight makes the
// sum, every pdf value and every knot but cdf_0 = 0 NaN; every search then ends at i = 1, den is NaN (NaN < eps is false),
// and every sample of that row is NaN.  Every NaN that leaves this header is the canonical quiet NaN 0x7FC00000 (host and
// device units disagree on the sign of a generated NaN), and in a sorted row the NaN come last.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rays.hpp"

namespace isr {
namespace resample {

constexpr int kMinPoints = 3, kMaxPoints = 1024;     // P; nb = P - 2 bins carry weight
constexpr int kMaxSamples = 1024;                    // n
constexpr long long kMaxRays = 1ll << 28;            // N
constexpr uint32_t kTagPdf = 2;                      // Philox stream tag (rays.hpp uses 0 and 1)
constexpr uint32_t kNanKey = 0xFFFFFFFFu;

// What a call asks for, made once on the host (make_spec) and read by host and device alike.
struct Spec {
  int nb;                 // weighted bins; the knots are bins[0 .. nb] and cdf[0 .. nb]
  int n;                  // samples per ray
  int det;                // units: linspace(0, 1, n) when set, Philox otherwise
  float eps;
  float ustep;            // linspace_step(0, 1, n)
  uint32_t key0, key1;    // Philox key = seed
};

ISR_HD uint32_t float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// The sort key of a depth: the sign-corrected integer image of its bits (-0 before +0), every NaN the largest key.
ISR_HD uint32_t sort_key(float f) {
  if (f != f) return kNanKey;
  const uint32_t u = float_bits(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

ISR_HD float key_value(uint32_t k) {
  if (k == kNanKey) return bits_float(kNanBits);
  return bits_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// bins_j of a ray's lengths: the mid-point of l_j and l_{j+1}
ISR_HD float mid_point(float lo, float hi) { return 0.5f * (hi + lo); }

// The knots, in place: c[1 .. nb] holds the weights w_0 .. w_{nb-1} on entry and cdf_1 .. cdf_nb on return; c[0] = 0.
//   S = f32(sum_j f64(w_j + eps)),   pdf_j = (w_j + eps) / S,   cdf_{j+1} = f32(sum_{i <= j} f64(pdf_i)).
// The two sums are serial scans in this order — the order is the contract, one thread owns both; the quotients between
// them are independent of each other, so the kernel spreads them over its lanes (the three steps are separate for that).
ISR_HD float weight_sum(const float* c, int nb, float eps) {
  double acc = 0.0;
  for (int j = 0; j < nb; ++j) acc += (double)(c[j + 1] + eps);
  return (float)acc;
}

ISR_HD float pdf_value(float w, float eps, float S) { return (w + eps) / S; }

// c[1 .. nb] holds pdf_0 .. pdf_{nb-1} on entry
ISR_HD void pdf_scan(float* c, int nb) {
  c[0] = 0.f;
  double acc = 0.0;
  for (int j = 0; j < nb; ++j) {
    acc += (double)c[j + 1];
    c[j + 1] = (float)acc;
  }
}

ISR_HD void build_cdf(float* c, int nb, float eps) {
  const float S = weight_sum(c, nb, eps);
  for (int j = 0; j < nb; ++j) c[j + 1] = pdf_value(c[j + 1], eps, S);
  pdf_scan(c, nb);
}

// unit s of ray `ray_id`
ISR_HD float unit_at(const Spec& sp, uint32_t ray_id, int s) {
  if (sp.det) return rays::linspace_at(0.f, 1.f, sp.ustep, sp.n, s);
  uint32_t w[4];
  philox4x32_10(ray_id, 0u, kTagPdf, (uint32_t)(s >> 2), sp.key0, sp.key1, w);
  const uint32_t word = (s & 3) == 0 ? w[0] : (s & 3) == 1 ? w[1] : (s & 3) == 2 ? w[2] : w[3];
  return unit_float(word);
}

// The sample of unit u: i = #{k in 0..nb : cdf_k <= u} by this binary search (searchsorted(right=True) on a monotone row;
// on a row with NaN knots it is this search that is the rule), then the interpolation inside bin [i - 1, min(i, nb)].
ISR_HD float sample_at(const float* bins, const float* cdf, int nb, float eps, float u) {
  int lo = 0, hi = nb + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int below = lo > 0 ? lo - 1 : 0, above = lo < nb ? lo : nb;
  float den = cdf[above] - cdf[below];
  if (den < eps) den = 1.f;
  const float t = (u - cdf[below]) / den;
  const float span = bins[above] - bins[below];
  const float step = t * span;                       // two roundings, not fused
  return canonical(bins[below] + step);
}

// ---- the spec of a call.  Returns null, or what is wrong with the arguments.
inline const char* make_spec(long long N, int nb, int n, int det, float eps, uint64_t seed, Spec& s) {
  if (N < 0 || N > kMaxRays) return "N outside 0..2^28";
  if (nb < kMinPoints - 2 || nb > kMaxPoints - 2) return "P outside 3..1024 (nb = P - 2 outside 1..1022)";
  if (n < 1 || n > kMaxSamples) return "n outside 1..1024";
  if (!(eps > 0.f) || !std::isfinite(eps)) return "eps must be positive and finite";
  s = Spec{};
  s.nb = nb;
  s.n = n;
  s.det = det != 0;
  s.eps = eps;
  s.ustep = rays::linspace_step(0.f, 1.f, n);
  s.key0 = (uint32_t)seed;
  s.key1 = (uint32_t)(seed >> 32);
  return nullptr;
}

// ---- host builds: the definitions the kernel is compared with.  cdf: nb + 1 floats of scratch.
inline void sample_pdf_row(const Spec& sp, const float* bins, const float* weights, uint32_t ray_id, float* cdf, float* samples) {
  for (int j = 0; j < sp.nb; ++j) cdf[j + 1] = weights[j];
  build_cdf(cdf, sp.nb, sp.eps);
  for (int s = 0; s < sp.n; ++s) samples[s] = sample_at(bins, cdf, sp.nb, sp.eps, unit_at(sp, ray_id, s));
}

// bins, cdf: P - 1 floats of scratch each; keys: P_out words; out: P_out = n + (add_input ? P : 0) floats
inline void resample_row(const Spec& sp, const float* lengths, const float* ray_weights, int add_input, uint32_t ray_id,
                         float* bins, float* cdf, uint32_t* keys, float* out) {
  const int P = sp.nb + 2, base = add_input ? P : 0;
  for (int j = 0; j + 1 < P; ++j) bins[j] = mid_point(lengths[j], lengths[j + 1]);
  for (int j = 0; j < sp.nb; ++j) cdf[j + 1] = ray_weights[j + 1];
  build_cdf(cdf, sp.nb, sp.eps);
  for (int k = 0; k < base; ++k) keys[k] = sort_key(lengths[k]);
  for (int s = 0; s < sp.n; ++s) keys[base + s] = sort_key(sample_at(bins, cdf, sp.nb, sp.eps, unit_at(sp, ray_id, s)));
  std::sort(keys, keys + base + sp.n);
  for (int k = 0; k < base + sp.n; ++k) out[k] = key_value(keys[k]);
}

}  // namespace resample
}  // namespace isr
