// sample_grad.hpp — the backward of the nearest-pixel sampling: the rule of include/isr_sample_grad.h, written once and
// compiled for host and device.  csrc/sample_grad.hip holds the kernels and the C entries; a plain C++ compiler can include
// this header too (tools/sample_grad_host_check.cpp).  Only f32 additions, and everything is built with -ffp-contract=off:
// host and device give the same bits.
//
// What this replaces: the scatter-add with float atomics that autograd runs behind grid_sample(mode='nearest') in
// nutil.sample_images_at_mc_locs (nutil.py:188-193) when trainPose.py:449 calls loss.backward().
#pragma once
#include <vector>

#include "rays.hpp"

namespace isr {
namespace sample_grad {

constexpr int kLdsRays = 4096;      // rays per image one workgroup sorts in LDS (64-bit keys: 32 KiB)
constexpr int kBlockKeys = 1024;    // keys per block of the radix sort above that
constexpr int kDigitBits = 8;       // bits of a radix digit
constexpr int kDigits = 1 << kDigitBits;

// The pixel ray `row` (of all B * n) belongs to, iy * W + ix, or H * W when it belongs to none: such rays sort last.
ISR_HD uint32_t ray_pixel(const float* xys, size_t row, int H, int W) {
  const int ix = rays::nearest_pixel(xys[2 * row], W), iy = rays::nearest_pixel(xys[2 * row + 1], H);
  return ix < 0 || iy < 0 ? (uint32_t)H * (uint32_t)W : (uint32_t)iy * (uint32_t)W + (uint32_t)ix;
}

// Digit passes that order every pixel value 0 .. H * W: the bits of H * W, in digits of kDigitBits.
inline int radix_passes(int H, int W) {
  int bits = 0;
  for (uint32_t v = (uint32_t)H * (uint32_t)W; v; v >>= 1) ++bits;
  return (bits + kDigitBits - 1) / kDigitBits;
}

// Returns null, or what is wrong with the shape.
inline const char* check_shape(int B, int H, int W, int C, int n) {
  if (B < 1 || H < 1 || W < 1 || n < 1) return "B, H, W or n < 1";
  if (C < 1 || C > rays::kMaxChannels) return "C outside 1..4096";
  if ((long long)B * n > rays::kMaxRays) return "B * n > 2^28";
  if ((long long)B * n * C >= (1ll << 31)) return "B * n * C >= 2^31";
  if ((long long)H * W >= (1ll << 31) - 1) return "H * W >= 2^31 - 1";
  if ((long long)B * H * W >= (1ll << 40) || (long long)B * H * W * C >= (1ll << 40)) return "B * H * W * C >= 2^40";
  return nullptr;
}

// ---- host builds: the definition the kernels are compared with.  Walking the rays in ascending r and adding each into its
// pixel is the chain of the rule: every (pixel, channel) starts at +0 and takes its rays' values in r order.
inline void backward_host(const float* dout, int B, int H, int W, int C, const float* xys, int n, float* dimages) {
  const size_t HW = (size_t)H * W;
  for (size_t i = 0; i < (size_t)B * HW * C; ++i) dimages[i] = 0.f;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < n; ++r) {
      const size_t row = (size_t)b * n + r;
      const uint32_t p = ray_pixel(xys, row, H, W);
      if (p == HW) continue;
      float* px = dimages + ((size_t)b * HW + p) * C;
      for (int c = 0; c < C; ++c) px[c] = px[c] + dout[row * C + c];
    }
}

// The device's route as host code (the host check compares it with backward_host): the rays of image b in the order of the
// key (pixel << 32) | r by a stable radix sort over the pixel's digits from r order, into pix and ray (n each).
inline void sorted_list_host(const float* xys, int b, int H, int W, int n, uint32_t* pix, uint32_t* ray) {
  std::vector<uint32_t> pix2((size_t)n), ray2((size_t)n);
  for (int r = 0; r < n; ++r) {
    pix[r] = ray_pixel(xys, (size_t)b * n + r, H, W);
    ray[r] = (uint32_t)r;
  }
  uint32_t *pi = pix, *ri = ray, *po = pix2.data(), *ro = ray2.data();
  const int passes = radix_passes(H, W);
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = pass * kDigitBits;
    size_t start[kDigits + 1] = {0};
    for (int k = 0; k < n; ++k) ++start[((pi[k] >> shift) & (kDigits - 1)) + 1];
    for (int d = 0; d < kDigits; ++d) start[d + 1] += start[d];
    for (int k = 0; k < n; ++k) {
      const size_t dst = start[(pi[k] >> shift) & (kDigits - 1)]++;
      po[dst] = pi[k];
      ro[dst] = ri[k];
    }
    uint32_t* t = pi; pi = po; po = t;
    t = ri; ri = ro; ro = t;
  }
  if (pi != pix)
    for (int k = 0; k < n; ++k) {
      pix[k] = pi[k];
      ray[k] = ri[k];
    }
}

// The segment sums over a sorted list, as the device's sum kernel makes them; dimages must hold +0 already.
inline void sum_segments_host(const float* dout, int b, int H, int W, int C, int n, const uint32_t* pix, const uint32_t* ray,
                              float* dimages) {
  const uint32_t none = (uint32_t)H * (uint32_t)W;
  for (int k = 0; k < n; ++k) {
    const uint32_t p = pix[k];
    if (p == none || (k > 0 && pix[k - 1] == p)) continue;      // not a segment head
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
      for (int j = k; j < n && pix[j] == p; ++j) acc = acc + dout[((size_t)b * n + ray[j]) * C + c];
      dimages[((size_t)b * none + p) * C + c] = acc;
    }
  }
}

}  // namespace sample_grad
}  // namespace isr
