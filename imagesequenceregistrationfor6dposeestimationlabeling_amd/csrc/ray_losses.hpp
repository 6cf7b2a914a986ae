// ray_losses.hpp — the ray losses of trainNerfFine.py and trainPose.py and their gradients: nutil.mip360loss (nutil.py:140-152),
// the distortion regulariser over a ray's weights and depths, and the Huber terms of trainNerfFine.py:314-336 (nutil.huber of a
// render against the targets sampled at the rays).  Written once and compiled for host and device: csrc/ray_losses.hip holds
// the kernels and the C entries, include/isr_ray_losses.h states every rule, and a plain C++ compiler can include this header
// too (tools/ray_losses_host_check.cpp).  Only + - * / sqrt fabsf and conversions in f32 and f64, one explicit fma whose product
// is exact, and everything is built with -ffp-contract=off: the host and the device build give the same bits.
#pragma once
#include "ordered_sum.hpp"
#include "rays.hpp"

namespace isr {
namespace ray_losses {

constexpr int kMinP = 2, kMaxP = 1024;               // samples of a ray
constexpr long long kMaxRays = 1ll << 28;            // N, and B n
constexpr int kMaxF = 64;                            // colour channels of the render loss
constexpr int kLanes = 64;                           // accumulators of LANE ORDER

// ---- the distortion loss
ISR_HD float depth(float l, float l0) { return (l - l0) + 0.0f; }

// the running maximum: a NaN on either side stays
ISR_HD float max_step(float m, float d) { return (d > m || d != d) ? d : m; }

ISR_HD float midpoint(float t1, float t0) { return (t1 + t0) / 2.0f; }

// one term of inner_i: acc + w_j |ut_i - ut_j|, the product exact in f64
ISR_HD double pair_step(double acc, double wj, float ui, float uj) { return fma(wj, (double)fabsf(ui - uj), acc); }

ISR_HD double ray_term(float w, double inner, float delta) {
  const double q = (((double)w * (double)w) * (double)delta) / 3.0;
  return (double)w * inner + q;
}

ISR_HD float weight_grad(double c, float w, double inner, float delta) {
  const double g = 2.0 * inner + (2.0 * ((double)w * (double)delta)) / 3.0;
  return canonical((float)(c * g));
}

ISR_HD double grad_scale(float upstream, long long N) { return (double)upstream / (double)N; }

ISR_HD float mean_value(double S, double count) { return canonical((float)(S / count)); }

// ---- the render loss
// z2 and q = sqrt(1 + z2) of a difference d
ISR_HD void huber_parts(float d, double s, double& z2, double& q) {
  const double z = (double)d / s;
  z2 = z * z;
  q = sqrt(1.0 + z2);
}

ISR_HD double huber_value(float d, double s) {
  double z2, q;
  huber_parts(d, s, z2, q);
  if (!(z2 < __builtin_inf())) return z2;            // +Inf or NaN
  return (s * z2) / (1.0 + q);
}

ISR_HD float huber_grad(float d, double s, double k) {
  if (d == 0.f) return 0.f;
  double z2, q;
  huber_parts(d, s, z2, q);
  return canonical((float)((k * (double)d) / (s * q)));
}

// the index of ray `row`'s pixel in a (H, W) image, -1 outside: the rule of isr_sample_nearest
ISR_HD long long target_pixel(const float* xys, size_t row, int H, int W) {
  const int ix = rays::nearest_pixel(xys[2 * row], W), iy = rays::nearest_pixel(xys[2 * row + 1], H);
  return ix < 0 || iy < 0 ? -1ll : (long long)iy * W + ix;
}

// the target of element (row, ch) of image b; pix from target_pixel
ISR_HD float target_value(const float* images, const float* sils, int b, int H, int W, int F, long long pix, int ch) {
  if (pix < 0) return 0.f;
  const size_t at = (size_t)b * H * W + (size_t)pix;
  return ch < F ? images[at * F + ch] : sils[at];
}

// ---- shapes: what is wrong, or null
inline const char* check_distortion(long long N, long long P) {
  if (P < kMinP || P > kMaxP) return "P outside 2..1024";
  if (N < 1) return "N < 1 (the mean of no rays has no value)";
  if (N > kMaxRays) return "N above 2^28";
  return nullptr;
}

inline const char* check_render(long long B, long long n, long long F, long long H, long long W, double s) {
  if (B < 1 || n < 1 || H < 1 || W < 1) return "B, n, H or W < 1";
  if (F < 1 || F > kMaxF) return "F outside 1..64";
  if (B > kMaxRays || n > kMaxRays || B * n > kMaxRays) return "B n above 2^28";
  if (H > (1ll << 31) / W || B > (1ll << 31) / (H * W) || B * H * W * F >= (1ll << 31)) return "B H W F reaches 2^31";
  if (!(s > 0.0) || !(s < __builtin_inf())) return "scaling must be finite and above 0";
  return nullptr;
}

// ---- host builds: the definitions the kernels are compared with
// t (P), then ut (K) and delta (K) of one ray
inline void ray_depths(const float* l, int P, float* t, float* ut, float* delta) {
  float mx = depth(l[0], l[0]);
  for (int k = 0; k < P; ++k) {
    t[k] = depth(l[k], l[0]);
    mx = max_step(mx, t[k]);
  }
  for (int k = 0; k < P; ++k) t[k] = t[k] / mx;
  for (int i = 0; i + 1 < P; ++i) {
    ut[i] = midpoint(t[i + 1], t[i]);
    delta[i] = t[i + 1] - t[i];
  }
}

inline double inner_sum(const float* w, const float* ut, int K, int i) {
  double acc = 0.0;
  for (int j = 0; j < K; ++j) acc = pair_step(acc, (double)w[j], ut[i], ut[j]);
  return acc;
}

// one ray's value: LANE ORDER over its terms
inline double distortion_ray(const float* l, const float* w, int P) {
  float t[kMaxP], ut[kMaxP], delta[kMaxP];
  double lane[kLanes];
  ray_depths(l, P, t, ut, delta);
  for (int i = 0; i < kLanes; ++i) lane[i] = 0.0;
  for (int i = 0; i < P - 1; ++i) lane[i % kLanes] += ray_term(w[i], inner_sum(w, ut, P - 1, i), delta[i]);
  for (int s = kLanes / 2; s > 0; s >>= 1)
    for (int i = 0; i < s; ++i) lane[i] += lane[i + s];
  return lane[0];
}

inline void distortion_ray_backward(const float* l, const float* w, int P, double c, float* dw) {
  float t[kMaxP], ut[kMaxP], delta[kMaxP];
  ray_depths(l, P, t, ut, delta);
  for (int i = 0; i < P - 1; ++i) dw[i] = weight_grad(c, w[i], inner_sum(w, ut, P - 1, i), delta[i]);
  dw[P - 1] = 0.f;
}

// one ray's (row_c, row_o) of the render loss
ISR_HD void render_row(const float* rendered, const float* images, const float* sils, const float* xys, size_t row, int n, int F,
                       int H, int W, double s, double* row_c, double* row_o) {
  const int b = (int)(row / (size_t)n);
  const long long pix = target_pixel(xys, row, H, W);
  const float* x = rendered + row * (size_t)(F + 1);
  double c = 0.0;
  for (int ch = 0; ch < F; ++ch) c += huber_value(x[ch] - target_value(images, sils, b, H, W, F, pix, ch), s);
  *row_c = c;
  *row_o = huber_value(x[F] - target_value(images, sils, b, H, W, F, pix, F), s);
}

inline void render_row_backward(const float* rendered, const float* images, const float* sils, const float* xys, size_t row, int n,
                                int F, int H, int W, double s, double kc, double ko, float* drendered) {
  const int b = (int)(row / (size_t)n);
  const long long pix = target_pixel(xys, row, H, W);
  const float* x = rendered + row * (size_t)(F + 1);
  float* g = drendered + row * (size_t)(F + 1);
  for (int ch = 0; ch <= F; ++ch) g[ch] = huber_grad(x[ch] - target_value(images, sils, b, H, W, F, pix, ch), s, ch < F ? kc : ko);
}

}  // namespace ray_losses
}  // namespace isr
