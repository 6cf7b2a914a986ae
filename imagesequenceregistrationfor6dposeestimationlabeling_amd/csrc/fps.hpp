// fps.hpp — farthest-point sampling (FPS), its arithmetic stated once and compiled for host and device.  csrc/fps.hip holds
// the kernels and the C entries (include/isr_fps.h); a plain C++ compiler can include this header too (tools/fps_host_check.cpp).
//
// One cloud: `len` points (x, y, z in f32), K wanted.  s_0 = start, mind[i] = +inf, and step k = 1 .. K-1 does, in f32,
//     dx = x[i]-x[s]; dy = y[i]-y[s]; dz = z[i]-z[s]          (s = s_{k-1})
//     d  = fmaf(dz, dz, fmaf(dy, dy, dx*dx))                   (written out: everything is built with -ffp-contract=off)
//     mind[i] = fminf(mind[i], d)
//     s_k = the index of the largest mind[i]; among equal values the LOWEST index wins
// radius2[k] = mind[s_k] when s_k is selected; radius2[0] = +inf.  Duplicate points are legal: once every distinct point is
// taken the largest value is 0 and index 0 is selected again.  Entries k >= len of idx are -1 and of radius2 are 0.
// PRECONDITION: the first `len` points are finite (a NaN distance would make the arg-max depend on the comparison order);
// points past `len` are never read.
// The selection compares (value, index) pairs exactly — no arithmetic — so `better` is a strict total order and the arg-max
// is the same whatever the shape of the reduction: the result is a function of (points, len, start, K) only.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "hd.hpp"

namespace isr {
namespace fps {

constexpr int kMaxPoints = 1 << 30;      // indices and the padded loops stay inside int32

// squared distance of (x, y, z) to (sx, sy, sz): three roundings for the differences, one for the square, two fused adds
ISR_HD float dist2(float x, float y, float z, float sx, float sy, float sz) {
  const float dx = x - sx, dy = y - sy, dz = z - sz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// (v, i) is selected before (bv, bi): larger value, or the same value at a lower index
ISR_HD bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// a candidate that loses to every point (mind >= 0 for finite points)
constexpr int kNoIndex = std::numeric_limits<int>::max();
ISR_HD float no_value() { return -std::numeric_limits<float>::infinity(); }
// the index an arg-max selected.  Finite points always give one; where the precondition is broken and nothing compared
// greater than no_value(), index 0 stands in, so that a selection can never index outside the cloud.
ISR_HD int selected(int bi) { return bi == kNoIndex ? 0 : bi; }

// The definition, as a plain loop: pts (len, 3) row-major, mind a scratch of len floats, idx and radius2 (nullable) K entries.
inline void sample_host(const float* pts, int len, int start, int K, int32_t* idx, float* radius2, float* mind) {
  const float inf = std::numeric_limits<float>::infinity();
  for (int i = 0; i < len; ++i) mind[i] = inf;
  int s = start;
  float r = inf;
  const int n = K < len ? K : len;
  for (int k = 0; k < n; ++k) {
    idx[k] = s;
    if (radius2) radius2[k] = r;
    if (k + 1 == n) break;
    const float sx = pts[3 * (size_t)s], sy = pts[3 * (size_t)s + 1], sz = pts[3 * (size_t)s + 2];
    float bv = no_value();
    int bi = kNoIndex;
    for (int i = 0; i < len; ++i) {
      const float m = fminf(mind[i], dist2(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], sx, sy, sz));
      mind[i] = m;
      if (better(m, i, bv, bi)) {
        bv = m;
        bi = i;
      }
    }
    s = selected(bi);
    r = bv;
  }
  for (int k = n; k < K; ++k) {
    idx[k] = -1;
    if (radius2) radius2[k] = 0.f;
  }
}

}  // namespace fps
}  // namespace isr
