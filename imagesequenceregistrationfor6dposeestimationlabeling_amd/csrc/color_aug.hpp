// color_aug.hpp — the colour augmentation pass: the arithmetic of include/isr_color_aug.h (which states every rule), written
// once and compiled for host and device.  csrc/color_aug.hip holds the kernel and the C entries; a plain C++ compiler can
// include this header too (tools/color_aug_host_check.cpp).  u8 in, u8 out; f64 in between with + - * /, rint, floor and sqrt
// alone (exp64 is csrc/field_density.hpp's), and everything is built with -ffp-contract=off: host and device give the same
// bits.
//
// What this replaces: the albumentations Compose of augment.py:344-350 as :394-397 and :422-423 apply it.  Every operation is
// an owned definition (cv2's and albumentations' bytes are unpinned); the tail is csrc/augment.hpp's blanking and normalize.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/isr_color_aug.h"
#include "augment.hpp"
#include "field_density.hpp"

namespace isr {
namespace color_aug {

using Program = isr_color_program;
using augment::Frame;

constexpr int kMaxBatch = 16;                  // images per launch: their programs travel as kernel arguments
constexpr int kGrid = ISR_COLOR_AUG_GRID;      // CLAHE's tiles per side
constexpr int kTiles = kGrid * kGrid;
constexpr int kBins = 256;
constexpr long long kMaxPixels = ISR_COLOR_AUG_MAX_PIXELS;
constexpr int kMaxBorder = augment::kMaxBorder;
constexpr uint32_t kTagPoisson = 0, kTagHue = 1;

struct Batch {
  Program p[kMaxBatch];
  int kh[kMaxBatch], kw[kMaxBatch];            // the border kernel, 0 = off
  float mu[3], sd[3];
  int normalize;
};

// ---------------------------------------------------------------- bytes
// (uint8)(x * 255): an f32 product, clamped, truncated; NaN -> 0
ISR_HD uint8_t to_u8(float x) {
  const float p = x * 255.0f;
  if (p >= 255.0f) return 255;
  if (p > 0.0f) return (uint8_t)(int)p;
  return 0;
}

ISR_HD float from_u8(uint8_t q) { return (float)q / 255.0f; }

// clip(rint(v), 0, 255); v finite
ISR_HD uint8_t round8(double v) {
  const double r = rint(v);
  if (r <= 0.0) return 0;
  if (r >= 255.0) return 255;
  return (uint8_t)(int)r;
}

ISR_HD int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

ISR_HD int gray8(const uint8_t* p) {
  return (int)round8((0.299 * (double)p[0] + 0.587 * (double)p[1]) + 0.114 * (double)p[2]);
}

// ---------------------------------------------------------------- colorsys
ISR_HD double frac1(double t) { return t - floor(t); }      // Python's t % 1.0

// colorsys.rgb_to_hls, operation for operation
ISR_HD void rgb_to_hls(double r, double g, double b, double& h, double& l, double& s) {
  const double maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const double minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const double sumc = maxc + minc, rangec = maxc - minc;
  l = sumc / 2.0;
  if (minc == maxc) {
    h = 0.0;
    s = 0.0;
    return;
  }
  s = l <= 0.5 ? rangec / sumc : rangec / ((2.0 - maxc) - minc);
  const double rc = (maxc - r) / rangec, gc = (maxc - g) / rangec, bc = (maxc - b) / rangec;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (2.0 + rc) - bc;
  else h = (4.0 + gc) - rc;
  h = frac1(h / 6.0);
}

ISR_HD double hls_v(double m1, double m2, double hue) {
  hue = frac1(hue);
  if (hue < 1.0 / 6.0) return m1 + ((m2 - m1) * hue) * 6.0;
  if (hue < 0.5) return m2;
  if (hue < 2.0 / 3.0) return m1 + ((m2 - m1) * (2.0 / 3.0 - hue)) * 6.0;
  return m1;
}

// colorsys.hls_to_rgb, operation for operation
ISR_HD void hls_to_rgb(double h, double l, double s, double* rgb) {
  if (s == 0.0) {
    rgb[0] = rgb[1] = rgb[2] = l;
    return;
  }
  const double m2 = l <= 0.5 ? l * (1.0 + s) : (l + s) - (l * s);
  const double m1 = 2.0 * l - m2;
  rgb[0] = hls_v(m1, m2, h + 1.0 / 3.0);
  rgb[1] = hls_v(m1, m2, h);
  rgb[2] = hls_v(m1, m2, h - 1.0 / 3.0);
}

// the pixel in HLS, lightness raised by dl (1 - l), hue turned by dh, back to bytes
ISR_HD void hls_pixel(uint8_t* p, double dl, double dh) {
  double h, l, s, rgb[3];
  rgb_to_hls((double)p[0] / 255.0, (double)p[1] / 255.0, (double)p[2] / 255.0, h, l, s);
  l = l + dl * (1.0 - l);
  h = frac1(h + dh);
  hls_to_rgb(h, l, s, rgb);
  for (int c = 0; c < 3; ++c) p[c] = round8(rgb[c] * 255.0);
}

// ---------------------------------------------------------------- ColorJitter and RandomBrightnessContrast
ISR_HD uint8_t scale8(uint8_t v, double f) { return round8((double)v * f); }
ISR_HD uint8_t blend8(uint8_t v, double f, double other) { return round8((double)v * f + other * (1.0 - f)); }
ISR_HD double mean_gray(uint64_t sum, uint64_t n) { return rint((double)sum / (double)n); }
ISR_HD void saturate_pixel(uint8_t* p, double f) {
  const double g = (double)gray8(p);
  for (int c = 0; c < 3; ++c) p[c] = blend8(p[c], f, g);
}
ISR_HD uint8_t rbc8(uint8_t v, double alpha, double beta) { return round8((double)v * alpha + beta * 255.0); }

// one jitter step on one pixel; m: the image's mean gray at that step (the contrast step alone reads it)
ISR_HD void jitter_pixel(uint8_t* p, const Program& pr, int op, double m) {
  if (op == 0) {
    for (int c = 0; c < 3; ++c) p[c] = scale8(p[c], pr.brightness);
  } else if (op == 1) {
    for (int c = 0; c < 3; ++c) p[c] = blend8(p[c], pr.contrast, m);
  } else if (op == 2) {
    saturate_pixel(p, pr.saturation);
  } else {
    hls_pixel(p, 0.0, pr.hue);
  }
}

// the step at which the contrast runs: the steps before it need no sum over the image
ISR_HD int contrast_step(const Program& pr) {
  for (int st = 0; st < 4; ++st)
    if (pr.order[st] == 1) return st;
  return 4;
}

// ---------------------------------------------------------------- GaussianBlur, ksize 3
ISR_HD int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }      // n >= 2, -1 <= i <= n

ISR_HD uint8_t blur_at(const uint8_t* src, const Frame& f, int x, int y, int c) {
  const int xs[3] = {reflect101(x - 1, f.W), x, reflect101(x + 1, f.W)};
  const int ys[3] = {reflect101(y - 1, f.H), y, reflect101(y + 1, f.H)};
  int sum = 0;
  for (int j = 0; j < 3; ++j) {
    const uint8_t* row = src + (size_t)ys[j] * f.W * 3 + c;
    const int h = (int)row[xs[0] * 3] + 2 * (int)row[xs[1] * 3] + (int)row[xs[2] * 3];
    sum += (j == 1 ? 2 : 1) * h;
  }
  return (uint8_t)((sum + 8) >> 4);
}

// ---------------------------------------------------------------- ISONoise
ISR_HD int luma_sum(const uint8_t* p) {      // max + min
  const int mx = p[0] > p[1] ? (p[0] > p[2] ? p[0] : p[2]) : (p[1] > p[2] ? p[1] : p[2]);
  const int mn = p[0] < p[1] ? (p[0] < p[2] ? p[0] : p[2]) : (p[1] < p[2] ? p[1] : p[2]);
  return mx + mn;
}

// the population standard deviation of li / 510 from the exact sums; N <= 2^20 keeps N s2 and s1^2 below 2^63
ISR_HD double sigma_l(uint64_t s1, uint64_t s2, uint64_t n) {
  const uint64_t d = n * s2 - s1 * s1;           // >= 0 (Cauchy-Schwarz), exact
  return sqrt((double)d) / (510.0 * (double)n);
}

ISR_HD void poisson_cdf(double lambda, double* cdf) {
  double p = density::exp64(-lambda), acc = p;
  cdf[0] = acc;
  for (int k = 1; k < kBins; ++k) {
    p = (p * lambda) / (double)k;
    acc = acc + p;
    cdf[k] = acc;
  }
}

// the smallest k with u <= cdf[k], 255 when there is none; cdf does not decrease
ISR_HD int poisson_k(const double* cdf, uint32_t word) {
  const double u = ((double)word + 0.5) * 2.3283064365386962890625e-10;      // 2^-32
  int lo = 0, hi = kBins - 1;                    // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u <= cdf[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

ISR_HD uint32_t poisson_word(uint32_t pixel, uint32_t k0, uint32_t k1) {
  uint32_t w[4];
  philox4x32_10(pixel, kTagPoisson, 0u, 0u, k0, k1, w);
  return w[0];
}

// Irwin-Hall: twelve 24-bit uniforms summed as integers, minus 6
ISR_HD double irwin_hall(uint32_t pixel, uint32_t k0, uint32_t k1) {
  uint64_t sum = 0;
  for (uint32_t d = 0; d < 3; ++d) {
    uint32_t w[4];
    philox4x32_10(pixel, kTagHue, d, 0u, k0, k1, w);
    for (int i = 0; i < 4; ++i) sum += w[i] >> 8;
  }
  return (double)sum * 5.9604644775390625e-08 - 6.0;      // 2^-24
}

ISR_HD double sigma_hue(const Program& pr) { return (pr.color_shift * 360.0) * pr.intensity; }
ISR_HD double iso_lambda(const Program& pr, double sigma) { return (sigma * pr.intensity) * 255.0; }

ISR_HD void iso_pixel(uint8_t* p, uint32_t pixel, const double* cdf, double sigma_h, uint32_t k0, uint32_t k1) {
  const int k = poisson_k(cdf, poisson_word(pixel, k0, k1));
  const double z = irwin_hall(pixel, k0, k1);
  hls_pixel(p, (double)k / 255.0, (sigma_h * z) / 360.0);
}

// ---------------------------------------------------------------- CLAHE
ISR_HD int clahe_clip(double clip_limit, int area) {
  const double c = (clip_limit * (double)area) / 256.0;
  if (c >= 2147483647.0) return 2147483647;
  const int ci = (int)c;
  return ci < 1 ? 1 : ci;
}

// bin i of a tile's histogram after clipping at `clip` and spreading `excess` (the sum of what the clip cut off): excess / 256
// to every bin, the residual one count at a time over bins 0, step, 2 step, ...
ISR_HD uint32_t clahe_bin(uint32_t h, uint32_t clip, uint32_t excess, uint32_t i) {
  const uint32_t batch = excess / kBins, residual = excess - batch * kBins;
  uint32_t v = (h > clip ? clip : h) + batch;
  if (residual > 0) {
    const uint32_t step = kBins / residual > 1 ? kBins / residual : 1;
    if (i % step == 0 && i / step < residual) v += 1;
  }
  return v;
}

ISR_HD uint8_t clahe_lut_value(uint32_t cdf, int area) { return round8(((double)cdf * 255.0) / (double)area); }

// one tile: hist (256 counts) -> lut (256 bytes)
ISR_HD void clahe_lut(const uint32_t* hist, int clip, int area, uint8_t* lut) {
  uint32_t excess = 0, cdf = 0;
  for (int i = 0; i < kBins; ++i)
    if (hist[i] > (uint32_t)clip) excess += hist[i] - (uint32_t)clip;
  for (int i = 0; i < kBins; ++i) {
    cdf += clahe_bin(hist[i], (uint32_t)clip, excess, (uint32_t)i);
    lut[i] = clahe_lut_value(cdf, area);
  }
}

ISR_HD int tile_of(const Frame& f, int x, int y) { return (y / (f.H / kGrid)) * kGrid + x / (f.W / kGrid); }

// luts: 64 tables of 256 bytes
ISR_HD void clahe_pixel(uint8_t* p, const Frame& f, int x, int y, const uint8_t* luts) {
  const int Y = gray8(p);
  const double txf = (double)x / (double)(f.W / kGrid) - 0.5, tyf = (double)y / (double)(f.H / kGrid) - 0.5;
  const double fx = floor(txf), fy = floor(tyf);
  const double xa = txf - fx, ya = tyf - fy;
  int tx1 = (int)fx, ty1 = (int)fy;
  int tx2 = tx1 + 1, ty2 = ty1 + 1;
  tx1 = tx1 < 0 ? 0 : tx1;
  ty1 = ty1 < 0 ? 0 : ty1;
  tx2 = tx2 > kGrid - 1 ? kGrid - 1 : tx2;
  ty2 = ty2 > kGrid - 1 ? kGrid - 1 : ty2;
  const double l11 = (double)luts[(ty1 * kGrid + tx1) * kBins + Y], l12 = (double)luts[(ty1 * kGrid + tx2) * kBins + Y];
  const double l21 = (double)luts[(ty2 * kGrid + tx1) * kBins + Y], l22 = (double)luts[(ty2 * kGrid + tx2) * kBins + Y];
  const double res = (l11 * (1.0 - xa) + l12 * xa) * (1.0 - ya) + (l21 * (1.0 - xa) + l22 * xa) * ya;
  const int Yn = (int)round8(res);
  for (int c = 0; c < 3; ++c) p[c] = (uint8_t)clamp8(Yn + ((int)p[c] - Y));
}

// ---------------------------------------------------------------- the ends
// out(x, y, 0..2) from the pass's value v3 of the pixel
ISR_HD void finish_pixel(const float* v3, const float* select, const float* under, const float* border_mask, const Frame& f,
                              int kh, int kw, const Batch& bt, int x, int y, float* out3) {
  const size_t pix = (size_t)y * f.W + x;
  const bool keep = !select || select[pix] == 1.f;
  const bool blank = border_mask && kh > 0 && kw > 0 && augment::border_blank(border_mask, f, kh, kw, x, y);
  for (int c = 0; c < 3; ++c) {
    float v = keep ? v3[c] : under ? under[pix * 3 + c] : 0.f;
    if (blank) v = 0.f;
    out3[c] = bt.normalize ? augment::normalize1(v, bt.mu[c], bt.sd[c]) : v;
  }
}

// ---------------------------------------------------------------- checks
inline bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// null, or what is wrong with a program
inline const char* check_program(const Program& p) {
  const double f[9] = {p.brightness, p.contrast, p.saturation, p.hue, p.alpha, p.beta, p.color_shift, p.intensity, p.clip_limit};
  if (!finite_all(f, 9)) return "a factor that is not finite";
  if (p.brightness < 0 || p.contrast < 0 || p.saturation < 0 || p.alpha < 0 || p.color_shift < 0 || p.intensity < 0)
    return "a negative multiplicative factor";
  if (p.clip_limit < 1.0) return "clip_limit below 1";
  if (p.ksize != 0 && p.ksize != 1 && p.ksize != 3) return "ksize outside {0, 1, 3}";
  int seen = 0;
  for (int i = 0; i < 4; ++i) {
    if (p.order[i] < 0 || p.order[i] > 3) return "order is no permutation of 0..3";
    seen |= 1 << p.order[i];
  }
  if (seen != 15) return "order is no permutation of 0..3";
  return nullptr;
}

// The programs of images b0 .. b0 + nb - 1.  Returns null, or what is wrong.
inline const char* make_batch(int b0, int nb, const Program* programs, const int32_t* border, const float* mean3, const float* std3,
                              Batch& bt) {
  bt = Batch{};
  bt.normalize = mean3 ? 1 : 0;
  for (int c = 0; c < 3 && mean3; ++c) {
    bt.mu[c] = mean3[c];
    bt.sd[c] = std3[c];
    if (!(std3[c] != 0.f)) return "std3 holds a zero or a NaN";
  }
  for (int j = 0; j < kMaxBatch; ++j) {
    const size_t b = (size_t)b0 + (j < nb ? j : 0);
    bt.p[j] = programs[b];
    if (const char* bad = check_program(bt.p[j])) return bad;
    if (border) {
      bt.kh[j] = border[2 * b];
      bt.kw[j] = border[2 * b + 1];
      if (bt.kh[j] < 0 || bt.kw[j] < 0 || bt.kh[j] > kMaxBorder || bt.kw[j] > kMaxBorder) return "a border kernel outside 0..255";
    }
  }
  return nullptr;
}

inline bool shape_ok(int B, int H, int W) {
  return B >= 1 && H >= kGrid && W >= kGrid && H % kGrid == 0 && W % kGrid == 0 && (long long)H * W <= kMaxPixels;
}

// One image's workspace: two u8 buffers of H W 3 bytes, each rounded up to 256 (the blur reads one and writes the other), the 64
// look-up tables, the Poisson cdf and the sum of gray.
inline size_t image_buffer_bytes(int H, int W) { return (((size_t)H * W * 3) + 255) / 256 * 256; }
constexpr size_t kLutBytes = (size_t)kTiles * kBins, kCdfBytes = kBins * sizeof(double), kSumBytes = 256;
inline size_t image_ws_bytes(int H, int W) { return 2 * image_buffer_bytes(H, W) + kLutBytes + kCdfBytes + kSumBytes; }

// ---------------------------------------------------------------- host build of one image
inline void pass_host(const float* in, const Frame& f, const Program& pr, float* v) {      // v: (H, W, 3) f32, the pass's result
  const size_t npix = (size_t)f.H * f.W, n3 = npix * 3;
  if (!pr.pass) {
    for (size_t i = 0; i < n3; ++i) v[i] = in[i];
    return;
  }
  std::vector<uint8_t> a(n3), b2(n3);
  for (size_t i = 0; i < n3; ++i) a[i] = to_u8(in[i]);
  if (pr.jitter)
    for (int st = 0; st < 4; ++st) switch (pr.order[st]) {
        case 0:
          for (size_t i = 0; i < n3; ++i) a[i] = scale8(a[i], pr.brightness);
          break;
        case 1: {
          uint64_t sum = 0;
          for (size_t q = 0; q < npix; ++q) sum += (uint64_t)gray8(&a[3 * q]);
          const double m = mean_gray(sum, npix);
          for (size_t i = 0; i < n3; ++i) a[i] = blend8(a[i], pr.contrast, m);
          break;
        }
        case 2:
          for (size_t q = 0; q < npix; ++q) saturate_pixel(&a[3 * q], pr.saturation);
          break;
        default:
          for (size_t q = 0; q < npix; ++q) hls_pixel(&a[3 * q], 0.0, pr.hue);
      }
  if (pr.rbc)
    for (size_t i = 0; i < n3; ++i) a[i] = rbc8(a[i], pr.alpha, pr.beta);
  if (pr.ksize == 3) {
    for (int y = 0; y < f.H; ++y)
      for (int x = 0; x < f.W; ++x)
        for (int c = 0; c < 3; ++c) b2[((size_t)y * f.W + x) * 3 + c] = blur_at(a.data(), f, x, y, c);
    a.swap(b2);
  }
  if (pr.iso) {
    uint64_t s1 = 0, s2 = 0;
    for (size_t q = 0; q < npix; ++q) {
      const uint64_t li = (uint64_t)luma_sum(&a[3 * q]);
      s1 += li;
      s2 += li * li;
    }
    double cdf[kBins];
    poisson_cdf(iso_lambda(pr, sigma_l(s1, s2, npix)), cdf);
    const double sh = sigma_hue(pr);
    for (size_t q = 0; q < npix; ++q) iso_pixel(&a[3 * q], (uint32_t)q, cdf, sh, (uint32_t)pr.noise_key, (uint32_t)(pr.noise_key >> 32));
  }
  if (pr.clahe) {
    const int area = (f.H / kGrid) * (f.W / kGrid);
    std::vector<uint32_t> hist((size_t)kTiles * kBins, 0u);
    std::vector<uint8_t> luts((size_t)kTiles * kBins);
    for (int y = 0; y < f.H; ++y)
      for (int x = 0; x < f.W; ++x) hist[(size_t)tile_of(f, x, y) * kBins + gray8(&a[((size_t)y * f.W + x) * 3])] += 1;
    const int clip = clahe_clip(pr.clip_limit, area);
    for (int t = 0; t < kTiles; ++t) clahe_lut(&hist[(size_t)t * kBins], clip, area, &luts[(size_t)t * kBins]);
    for (int y = 0; y < f.H; ++y)
      for (int x = 0; x < f.W; ++x) clahe_pixel(&a[((size_t)y * f.W + x) * 3], f, x, y, luts.data());
  }
  for (size_t i = 0; i < n3; ++i) v[i] = from_u8(a[i]);
}

inline void image_host(const float* in, const float* select, const float* under, const float* border_mask, const Frame& f,
                       const Batch& bt, int j, float* out) {
  std::vector<float> v((size_t)f.H * f.W * 3);
  pass_host(in, f, bt.p[j], v.data());
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x) {
      const size_t pix = (size_t)y * f.W + x;
      finish_pixel(&v[pix * 3], select, under, border_mask, f, bt.kh[j], bt.kw[j], bt, x, y, out + pix * 3);
    }
}

}  // namespace color_aug
}  // namespace isr
