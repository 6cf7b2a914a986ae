// augment.hpp — training batches: the arithmetic of include/isr_augment.h (which states every rule), written once and
// compiled for host and device.  csrc/augment.hip holds the kernels and the C entries; a plain C++ compiler can include this
// header too (tools/augment_host_check.cpp).  f64 for the warp, f32 with explicit fmaf for the rays, and everything is built
// with -ffp-contract=off: host and device give the same bits.
//
// What this replaces: augment.py:284-432 (generateImages' warps, paste and borderADD blanking), dataGen.py:16-20 (normalize)
// and augment.py:639-685 (getNerfSamples).  The warp is csrc/crop_normalize.hip's: the textbook definition, cv2's own
// bytes unpinned.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rays.hpp"

namespace isr {
namespace augment {

constexpr int kMaxBatch = 16;                  // images per launch: their parameters travel as kernel arguments
constexpr int kMaxSample = 4096;               // S
constexpr int kMaxViewRows = 1 << 20;          // a view's n
constexpr long long kMaxPixels = 1ll << 28;    // H * W
constexpr int kMaxShift = 1 << 24;             // |tra|, |tra1|
constexpr int kMaxBorder = 255;                // kh, kw

// ---------------------------------------------------------------- images
struct ImageParams {
  double inv1[6];        // (M + tra1)^-1: destination (x, y, 1) -> source, row-major 2x3
  double inv2[6];        // (M + tra)^-1
  int dx, dy;            // tra - tra1
  int rx, ry, rw, rh;    // the occluder rectangle
  int kh, kw;            // the border kernel, 0 = off
};

struct ImageBatch {
  ImageParams p[kMaxBatch];
  float mu[3], sd[3];
};

struct Frame {
  int H, W;
};

// A = M with (tx, ty) added to its translation column; inv = A^-1.  False when A is singular or not finite.
inline bool invert_affine(const double* M, double tx, double ty, double* inv) {
  const double a02 = M[2] + tx, a12 = M[5] + ty;
  const double det = M[0] * M[4] - M[1] * M[3];
  if (!(det != 0.0) || !std::isfinite(det) || !std::isfinite(a02) || !std::isfinite(a12)) return false;
  const double i00 = M[4] / det, i01 = -M[1] / det, i10 = -M[3] / det, i11 = M[0] / det;
  inv[0] = i00; inv[1] = i01; inv[2] = -(i00 * a02 + i01 * a12);
  inv[3] = i10; inv[4] = i11; inv[5] = -(i10 * a02 + i11 * a12);
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(inv[i])) return false;
  return true;
}

// the bilinear sum at the source position of destination pixel (x, y); px(x, y): the pixel as f64, 0 outside the frame
template <class Px>
ISR_HD double bilinear(const double* inv, long x, long y, Px px) {
  const double sx = (inv[0] * (double)x + inv[1] * (double)y) + inv[2];
  const double sy = (inv[3] * (double)x + inv[4] * (double)y) + inv[5];
  const double fx0 = floor(sx), fy0 = floor(sy);
  const double fx = sx - fx0, fy = sy - fy0;
  // positions beyond +-2^40 (or NaN) have no neighbour in any frame: every term is 0
  if (!(fx0 > -1.0995e12 && fx0 < 1.0995e12 && fy0 > -1.0995e12 && fy0 < 1.0995e12)) return 0.0;
  const long x0 = (long)fx0, y0 = (long)fy0;
  const double w00 = (1.0 - fx) * (1.0 - fy), w01 = fx * (1.0 - fy), w10 = (1.0 - fx) * fy, w11 = fx * fy;
  return ((px(x0, y0) * w00 + px(x0 + 1, y0) * w01) + px(x0, y0 + 1) * w10) + px(x0 + 1, y0 + 1) * w11;
}

ISR_HD bool in_frame(const Frame& f, long x, long y) { return x >= 0 && x < f.W && y >= 0 && y < f.H; }

// warp(mask, A)(x, y) for a u8 mask: rounded half to even.  rw = 0 or rh = 0: no rectangle.
ISR_HD uint8_t warp_mask(const uint8_t* mask, const Frame& f, const double* inv, int rx, int ry, int rw, int rh, long x,
                              long y) {
  const double v = bilinear(inv, x, y, [&](long xx, long yy) -> double {
    if (!in_frame(f, xx, yy)) return 0.0;
    if (rw > 0 && rh > 0 && xx >= rx && xx < (long)rx + rw && yy >= ry && yy < (long)ry + rh) return 0.0;
    return (double)mask[(size_t)yy * f.W + xx];
  });
  return (uint8_t)rint(v);                     // 0 <= v <= 255
}

// warp(rgb, A)(x, y, c) for an f32 image: one rounding
ISR_HD float warp_rgb(const float* rgb, const Frame& f, const double* inv, int c, long x, long y) {
  return (float)bilinear(inv, x, y, [&](long xx, long yy) -> double {
    return in_frame(f, xx, yy) ? (double)rgb[((size_t)yy * f.W + xx) * 3 + c] : 0.0;
  });
}

// dst_mask(x, y) and dst_mask_orig(x, y) of image parameters p
ISR_HD float mask_out_at(const uint8_t* mask, const Frame& f, const ImageParams& p, int x, int y) {
  const long xs = (long)x - p.dx, ys = (long)y - p.dy;          // the second warp: an integer shift of the clipped first result
  if (!in_frame(f, xs, ys)) return 0.f;
  return (float)warp_mask(mask, f, p.inv1, p.rx, p.ry, p.rw, p.rh, xs, ys);
}

ISR_HD float mask_orig_at(const uint8_t* orig_mask, const Frame& f, const ImageParams& p, int x, int y) {
  return (float)warp_mask(orig_mask, f, p.inv2, 0, 0, 0, 0, x, y);
}

// is the kh x kw dilation of mask_out at (x, y) <= 0.9?  Anchor (kw / 2, kh / 2), positions outside the frame ignored.
ISR_HD bool border_blank(const float* mask_out, const Frame& f, int kh, int kw, int x, int y) {
  const int y_lo = y - kh / 2, x_lo = x - kw / 2;
  const int y0 = y_lo < 0 ? 0 : y_lo, x0 = x_lo < 0 ? 0 : x_lo;
  const int y1 = y_lo + kh > f.H ? f.H : y_lo + kh, x1 = x_lo + kw > f.W ? f.W : x_lo + kw;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx)
      if (mask_out[(size_t)yy * f.W + xx] > 0.9f) return false;
  return true;
}

// (x - mu) / std: an f32 subtraction, then an f32 division
ISR_HD float normalize1(float v, float mu, float sd) {
  const float d = v - mu;
  return d / sd;
}

// rgb_out(x, y, 0..2), given mask_out of the whole image
ISR_HD void rgb_out_at(const float* rgb, const float* canvas, const float* mask_out, const Frame& f, const ImageParams& p,
                            const float* mu, const float* sd, int x, int y, float* out3) {
  const size_t pix = (size_t)y * f.W + x;
  const bool object = mask_out[pix] == 1.f;     // then (x - dx, y - dy) lies in the frame
  const bool blank = p.kh > 0 && p.kw > 0 && border_blank(mask_out, f, p.kh, p.kw, x, y);
  for (int c = 0; c < 3; ++c) {
    float v;
    if (blank) v = 0.f;
    else if (object) v = warp_rgb(rgb, f, p.inv1, c, (long)x - p.dx, (long)y - p.dy);
    else v = canvas ? canvas[pix * 3 + c] : 0.f;
    out3[c] = normalize1(v, mu[c], sd[c]);
  }
}

// The parameters of images b0 .. b0 + nb - 1 (nb <= kMaxBatch).  Returns null, or what is wrong.
inline const char* make_image_batch(int b0, int nb, const int32_t* rect, const double* M, const int32_t* tra, const int32_t* tra1,
                                    const int32_t* border, const float* mean3, const float* std3, ImageBatch& ib) {
  ib = ImageBatch{};
  for (int c = 0; c < 3; ++c) {
    ib.mu[c] = mean3[c];
    ib.sd[c] = std3[c];
    if (!(std3[c] != 0.f)) return "std3 holds a zero or a NaN";
  }
  for (int j = 0; j < kMaxBatch; ++j) {
    const size_t b = (size_t)b0 + (j < nb ? j : 0);
    ImageParams& p = ib.p[j];
    int t[2] = {0, 0}, t1[2] = {0, 0};
    for (int a = 0; a < 2; ++a) {
      if (tra) t[a] = tra[2 * b + a];
      if (tra1) t1[a] = tra1[2 * b + a];
      if (t[a] > kMaxShift || t[a] < -kMaxShift || t1[a] > kMaxShift || t1[a] < -kMaxShift) return "a shift beyond 2^24";
    }
    if (!invert_affine(M + 6 * b, (double)t1[0], (double)t1[1], p.inv1) ||
        !invert_affine(M + 6 * b, (double)t[0], (double)t[1], p.inv2))
      return "a singular or non-finite affine matrix";
    p.dx = t[0] - t1[0];
    p.dy = t[1] - t1[1];
    if (rect) {
      p.rx = rect[4 * b]; p.ry = rect[4 * b + 1]; p.rw = rect[4 * b + 2]; p.rh = rect[4 * b + 3];
      if (p.rw < 0 || p.rh < 0) return "a rectangle of negative width or height";
    }
    if (border) {
      p.kh = border[2 * b]; p.kw = border[2 * b + 1];
      if (p.kh < 0 || p.kw < 0 || p.kh > kMaxBorder || p.kw > kMaxBorder) return "a border kernel outside 0..255";
    }
  }
  return nullptr;
}

// host build of one image
inline void images_host_one(const float* rgb, const uint8_t* mask, const uint8_t* orig_mask, const float* canvas, const Frame& f,
                            const ImageParams& p, const float* mu, const float* sd, float* rgb_out, float* mask_orig_out,
                            float* mask_out) {
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x) {
      const size_t pix = (size_t)y * f.W + x;
      mask_out[pix] = mask_out_at(mask, f, p, x, y);
      mask_orig_out[pix] = mask_orig_at(orig_mask, f, p, x, y);
    }
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x)
      rgb_out_at(rgb, canvas, mask_out, f, p, mu, sd, x, y, rgb_out + ((size_t)y * f.W + x) * 3);
}

// ---------------------------------------------------------------- rays
struct RaySet {
  const float* xys;      // (sum n, 2)
  const float* pos;      // (sum n, 3)
};

struct RayOut {
  float* xys;            // (B, S, 2)
  float* pos;            // (B, S, 3)
  int32_t* index;        // (B, S)
  int32_t* count;        // (B,)
};

struct RayBatch {
  long long start[2][kMaxBatch];   // first row of the image's view in the set's bank
  int n[2][kMaxBatch];             // its rows
  int view[kMaxBatch];
  float m[kMaxBatch][4];           // m00, m01, m10, m11
  float t[kMaxBatch][2];
};

ISR_HD void remap(const float* m, const float* t, float x, float y, float& sx, float& sy) {
  sx = fmaf(y, m[1], x * m[0]) - t[0];
  sy = fmaf(y, m[3], x * m[2]) - t[1];
}

ISR_HD bool touches_outside(float sx, float sy) { return sx >= 1.f || sx <= -1.f || sy >= 1.f || sy <= -1.f; }

ISR_HD bool strictly_inside(float sx, float sy) { return sx > -1.f && sx < 1.f && sy > -1.f && sy < 1.f; }

// the high word of candidate i's key
ISR_HD uint32_t key_word(uint32_t i, uint32_t view, uint32_t set, uint32_t k0, uint32_t k1) {
  uint32_t w[4];
  philox4x32_10(i, view, set, 0u, k0, k1, w);
  return w[0];
}

// The views of images b0 .. b0 + nb - 1.  offsets[1] null: one set.  Returns null, or what is wrong.
inline const char* make_ray_batch(int b0, int nb, const int64_t* const* offsets, int V, const int32_t* view_ids,
                                  const float* rot, const float* t, RayBatch& rb) {
  rb = RayBatch{};
  for (int j = 0; j < nb; ++j) {
    const size_t b = (size_t)b0 + j;
    const int v = view_ids[b];
    if (v < 0 || v >= V) return "a view id outside 0..V-1";
    rb.view[j] = v;
    for (int s = 0; s < 2; ++s) {
      if (!offsets[s]) continue;
      const long long n = offsets[s][v + 1] - offsets[s][v];
      if (n < 0 || offsets[s][v] < 0) return "offsets decrease or start below 0";
      if (n > kMaxViewRows) return "a view of more than 2^20 rows";
      rb.start[s][j] = offsets[s][v];
      rb.n[s][j] = (int)n;
    }
    for (int a = 0; a < 4; ++a) rb.m[j][a] = rot[4 * b + a];
    for (int a = 0; a < 2; ++a) rb.t[j][a] = t[2 * b + a];
  }
  return nullptr;
}

// host build of image j of the batch, set s -> row b of the outputs
inline void rays_host_one(const RaySet& in, const RayBatch& rb, int j, int s, int S, uint32_t k0, uint32_t k1, const RayOut& out,
                          size_t b) {
  const int n = rb.n[s][j];
  const float* xy = in.xys + 2 * rb.start[s][j];
  const float* pos = in.pos + 3 * rb.start[s][j];
  bool filter = false;
  for (int i = 0; i < n && !filter; ++i) {
    float sx, sy;
    remap(rb.m[j], rb.t[j], xy[2 * i], xy[2 * i + 1], sx, sy);
    filter = touches_outside(sx, sy);
  }
  std::vector<uint64_t> keys;
  for (int i = 0; i < n; ++i) {
    float sx, sy;
    remap(rb.m[j], rb.t[j], xy[2 * i], xy[2 * i + 1], sx, sy);
    if (filter && !strictly_inside(sx, sy)) continue;
    keys.push_back(((uint64_t)key_word((uint32_t)i, (uint32_t)rb.view[j], (uint32_t)s, k0, k1) << 32) | (uint32_t)i);
  }
  std::sort(keys.begin(), keys.end());
  const int K = (int)std::min<size_t>((size_t)S, keys.size());
  for (int r = 0; r < S; ++r) {
    const size_t row = b * S + r;
    if (r < K) {
      const uint32_t i = (uint32_t)keys[r];
      remap(rb.m[j], rb.t[j], xy[2 * i], xy[2 * i + 1], out.xys[2 * row], out.xys[2 * row + 1]);
      for (int a = 0; a < 3; ++a) out.pos[3 * row + a] = pos[3 * (size_t)i + a];
      out.index[row] = (int32_t)i;
    } else {
      out.xys[2 * row] = out.xys[2 * row + 1] = 0.f;
      for (int a = 0; a < 3; ++a) out.pos[3 * row + a] = 0.f;
      out.index[row] = -1;
    }
  }
  out.count[b] = K;
}

}  // namespace augment
}  // namespace isr
