// rays.hpp — rays from cameras: the arithmetic of include/isr_rays.h (which states every rule), written once and compiled
// for host and device.  csrc/rays.hip holds the kernels and the C entries; a plain C++ compiler can include this header
// too (tools/rays_host_check.cpp).  Only + - * / and explicit fmaf in f32, and everything is built with -ffp-contract=off:
// host and device give the same bits.
//
// What this replaces: pytorch3d's PerspectiveCameras / NDCMultinomialRaysampler / MonteCarloRaysampler as
// generateCors.py:125-138, :279-293 and genFeat.py:102-106, :162-189 use them, and the silhouette selection of pren.py:229-236
// through nutil.sample_images_at_mc_locs (nutil.py:167-196).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace rays {

constexpr int kGrid = 0, kMonteCarlo = 1;      // ISR_RAYS_GRID, ISR_RAYS_MC
constexpr int kMaxRays = 1 << 28;              // B * n
constexpr int kMaxPoints = 4096;               // P: the march's limit
constexpr int kMaxChannels = 4096;             // C of isr_sample_nearest
constexpr uint32_t kTagXy = 0, kTagStrata = 1; // Philox stream tags

// What a call asks for, made once on the host (make_spec) and read by host and device alike.
struct Spec {
  int mode;
  int B, n;                   // cameras, rays per camera (grid: W * H)
  int W, H;                   // grid only
  float ax, bx, ay, by;       // grid: xs = linspace(ax, bx, W), ys = linspace(ay, by, H)
  float xstep, ystep;         // their steps
  float min_x, wx, min_y, wy; // Monte-Carlo: x = fmaf(u, wx, min_x), wx = max_x - min_x
  int P;
  float lmin, lmax, lstep;    // lengths = linspace(lmin, lmax, P)
  int stratified;
  uint32_t key0, key1;        // Philox key = seed
};

struct Cameras {
  const float* R;             // (B, 3, 3)
  const float* T;             // (B, 3)
  const float* intr;          // (B, 4): fx, fy, px, py in NDC
  const int32_t* ids;         // (B,) or null: 0 .. B-1
};

// ---- linspace(a, b, P)[k] in f32 with step = (b - a) / (P - 1): torch.linspace's values (CPU, f32), bit for bit
ISR_HD float linspace_step(float a, float b, int P) { return P > 1 ? (b - a) / (float)(P - 1) : 0.f; }

ISR_HD float linspace_at(float a, float b, float step, int P, int k) {
  if (P == 1) return a;
  return k < P / 2 ? fmaf(step, (float)k, a) : fmaf(-step, (float)(P - 1 - k), b);
}

// the three-term dot product, in this order
ISR_HD float dot3(float a0, float a1, float a2, const float* r) { return fmaf(a2, r[2], fmaf(a1, r[1], a0 * r[0])); }

// The ray of the NDC point (x, y) of camera (R, T, intr): c = ((x - px) / fx, (y - py) / fy, 1), d = c R^T, o = (-T) R^T.
ISR_HD void ndc_ray(const float* R, const float* T, const float* intr, float x, float y, float* o, float* d) {
  const float cx = (x - intr[2]) / intr[0], cy = (y - intr[3]) / intr[1];
  for (int i = 0; i < 3; ++i) {
    d[i] = dot3(cx, cy, 1.f, R + 3 * i);
    o[i] = dot3(-T[0], -T[1], -T[2], R + 3 * i);
  }
}

ISR_HD int camera_id(const Cameras& c, int b) { return c.ids ? c.ids[b] : b; }

// xy of candidate ray r of camera b
ISR_HD void candidate_xy(const Spec& s, const Cameras& c, int b, int r, float& x, float& y) {
  if (s.mode == kGrid) {      // raster order, y outer
    x = linspace_at(s.ax, s.bx, s.xstep, s.W, r % s.W);
    y = linspace_at(s.ay, s.by, s.ystep, s.H, r / s.W);
  } else {
    uint32_t w[4];
    philox4x32_10((uint32_t)camera_id(c, b), (uint32_t)r, kTagXy, 0u, s.key0, s.key1, w);
    x = fmaf(unit_float(w[0]), s.wx, s.min_x);
    y = fmaf(unit_float(w[1]), s.wy, s.min_y);
  }
}

// length k of candidate ray r of camera b
ISR_HD float length_at(const Spec& s, const Cameras& c, int b, int r, int k) {
  const float l = linspace_at(s.lmin, s.lmax, s.lstep, s.P, k);
  if (s.mode == kGrid || !s.stratified) return l;
  const float lower = k == 0 ? l : 0.5f * (linspace_at(s.lmin, s.lmax, s.lstep, s.P, k - 1) + l);
  const float upper = k == s.P - 1 ? l : 0.5f * (l + linspace_at(s.lmin, s.lmax, s.lstep, s.P, k + 1));
  uint32_t w[4];
  philox4x32_10((uint32_t)camera_id(c, b), (uint32_t)r, kTagStrata, (uint32_t)(k >> 2), s.key0, s.key1, w);
  const uint32_t word = (k & 3) == 0 ? w[0] : (k & 3) == 1 ? w[1] : (k & 3) == 2 ? w[2] : w[3];
  return fmaf(upper - lower, unit_float(word), lower);
}

// grid_sample's nearest pixel (align_corners=True) of NDC coordinate v on an axis of `size` pixels; -1 outside (or NaN)
ISR_HD int nearest_pixel(float v, int size) {
  const float g = -v;
  const float f = rintf(((g + 1.f) / 2.f) * (float)(size - 1));      // half to even
  if (!(f >= 0.f && f <= (float)(size - 1))) return -1;
  return (int)f;
}

// is candidate (x, y) of camera b kept by mask (B, mh, mw)?  Non-zero keeps, NaN included.
ISR_HD bool mask_keeps(const float* mask, int mh, int mw, int b, float x, float y) {
  const int ix = nearest_pixel(x, mw), iy = nearest_pixel(y, mh);
  if (ix < 0 || iy < 0) return false;
  return mask[((size_t)b * mh + iy) * mw + ix] != 0.f;
}

ISR_HD bool candidate_kept(const Spec& s, const Cameras& c, const float* mask, int mh, int mw, int b, int r) {
  float x, y;
  candidate_xy(s, c, b, r, x, y);
  return mask_keeps(mask, mh, mw, b, x, y);
}

// ---- the spec of a call.  Returns null, or what is wrong with the arguments.
inline const char* make_spec(int mode, int B, int W, int H, int n, int P, float min_x, float max_x, float min_y, float max_y,
                             float min_depth, float max_depth, int stratified, uint64_t seed, Spec& s) {
  if (mode != kGrid && mode != kMonteCarlo) return "mode is neither ISR_RAYS_GRID nor ISR_RAYS_MC";
  if (B < 1) return "B < 1";
  if (P < 1 || P > kMaxPoints) return "P outside 1..4096";
  if (!(std::isfinite(min_depth) && std::isfinite(max_depth))) return "min_depth or max_depth is not finite";
  s = Spec{};
  s.mode = mode;
  s.B = B;
  s.P = P;
  s.lmin = min_depth;
  s.lmax = max_depth;
  s.lstep = linspace_step(min_depth, max_depth, P);
  s.stratified = stratified != 0;
  s.key0 = (uint32_t)seed;
  s.key1 = (uint32_t)(seed >> 32);
  if (mode == kGrid) {
    if (W < 1 || H < 1) return "W or H < 1";
    if ((long long)W * H > kMaxRays || (long long)B * W * H > kMaxRays) return "B * W * H > 2^28";
    s.W = W;
    s.H = H;
    s.n = W * H;
    const double range_x = W >= H ? (double)W / (double)H : 1.0, range_y = W >= H ? 1.0 : (double)H / (double)W;
    s.ax = (float)(range_x - range_x / W);       // end points in f64, rounded to f32 once
    s.bx = (float)(-range_x + range_x / W);
    s.ay = (float)(range_y - range_y / H);
    s.by = (float)(-range_y + range_y / H);
    s.xstep = linspace_step(s.ax, s.bx, W);
    s.ystep = linspace_step(s.ay, s.by, H);
  } else {
    if (n < 1) return "n < 1";
    if ((long long)B * n > kMaxRays) return "B * n > 2^28";
    if (!(std::isfinite(min_x) && std::isfinite(max_x) && std::isfinite(min_y) && std::isfinite(max_y)))
      return "min_x, max_x, min_y or max_y is not finite";
    if (!(min_x <= max_x && min_y <= max_y)) return "min_x > max_x or min_y > max_y";
    s.n = n;
    s.min_x = min_x;
    s.wx = max_x - min_x;
    s.min_y = min_y;
    s.wy = max_y - min_y;
  }
  return nullptr;
}

// ---- host builds: the definitions the kernels are compared with
inline void write_row(const Spec& s, const Cameras& c, int b, int r, size_t row, float* origins, float* directions, float* lengths,
                      float* xys) {
  float x, y, o[3], d[3];
  candidate_xy(s, c, b, r, x, y);
  ndc_ray(c.R + 9 * (size_t)b, c.T + 3 * (size_t)b, c.intr + 4 * (size_t)b, x, y, o, d);
  for (int i = 0; i < 3; ++i) {
    origins[3 * row + i] = o[i];
    directions[3 * row + i] = d[i];
  }
  xys[2 * row] = x;
  xys[2 * row + 1] = y;
  for (int k = 0; k < s.P; ++k) lengths[row * s.P + k] = length_at(s, c, b, r, k);
}

inline void bundle_host(const Spec& s, const Cameras& c, float* origins, float* directions, float* lengths, float* xys) {
  for (int b = 0; b < s.B; ++b)
    for (int r = 0; r < s.n; ++r) write_row(s, c, b, r, (size_t)b * s.n + r, origins, directions, lengths, xys);
}

inline int64_t select_count_host(const Spec& s, const Cameras& c, const float* mask, int mh, int mw) {
  int64_t count = 0;
  for (int b = 0; b < s.B; ++b)
    for (int r = 0; r < s.n; ++r) count += candidate_kept(s, c, mask, mh, mw, b, r);
  return count;
}

// kept rays in (camera, ray) order to rows 0 .. count-1 (those below cap), zeros to the rows from count to cap; -> count
inline int64_t select_emit_host(const Spec& s, const Cameras& c, const float* mask, int mh, int mw, int64_t cap, float* origins,
                                float* directions, float* lengths, float* xys, int32_t* src) {
  int64_t count = 0;
  for (int b = 0; b < s.B; ++b)
    for (int r = 0; r < s.n; ++r) {
      if (!candidate_kept(s, c, mask, mh, mw, b, r)) continue;
      if (count < cap) {
        write_row(s, c, b, r, (size_t)count, origins, directions, lengths, xys);
        src[count] = b * s.n + r;
      }
      ++count;
    }
  for (int64_t row = count; row < cap; ++row) {
    for (int i = 0; i < 3; ++i) origins[3 * row + i] = directions[3 * row + i] = 0.f;
    xys[2 * row] = xys[2 * row + 1] = 0.f;
    src[row] = 0;
    for (int k = 0; k < s.P; ++k) lengths[row * s.P + k] = 0.f;
  }
  return count;
}

// images (B, H, W, C), xys (B, n, 2) -> out (B, n, C): the nearest pixel of -xy, zero outside
inline void sample_nearest_host(const float* images, int B, int H, int W, int C, const float* xys, int n, float* out) {
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < n; ++r) {
      const size_t row = (size_t)b * n + r;
      const int ix = nearest_pixel(xys[2 * row], W), iy = nearest_pixel(xys[2 * row + 1], H);
      for (int ch = 0; ch < C; ++ch)
        out[row * C + ch] = ix < 0 || iy < 0 ? 0.f : images[(((size_t)b * H + iy) * W + ix) * C + ch];
    }
}

}  // namespace rays
}  // namespace isr
