// raster.hpp — the arithmetic of the object-coordinate rasteriser, one definition compiled as device code
// (csrc/render_coords.hip's kernels) and as host code (isr_render_coords_host).  Only + - * /, rint, integer arithmetic and
// comparisons, under the library's -ffp-contract=off: host and device produce the same bits.
//
// The rules (OpenGL's for a depth-tested, uncullled triangle list, with the choices GL leaves open fixed here):
//   vertex    X = (R0*vx + R1*vy) + R2*vz + t in f64 from the f32 vertex; u = (K00*x + K01*y)/z + K02,
//             v = (K10*x + K11*y)/z + K12; the centre of pixel (row r, col c) is (u, v) = (c, r), row 0 on top.
//             u, v are snapped to 1/256 px: rint(u*256) (ties to even), held as int32.
//   coverage  int64 edge functions of the snapped vertices at the pixel centre, the face oriented so that its doubled area
//             is positive (either winding covers: no culling), top-left fill rule, zero area covers nothing.
//   depth     1/z is affine on the screen: w_i = lambda_i / z_i, S = (w0 + w1) + w2, z_pix = area2 / S (f64).  A fragment
//             with z_pix outside [near, far] is discarded.  The z-buffer key is (bits of f32(z_pix)) << 32 | (face + 1):
//             the smallest key wins, so on equal f32 depth the lower face index does (GL_LESS in draw order); a pixel
//             already in the frame buffer (clear = 0) has face field 0 and wins ties against every new fragment.
//   near      a face with a vertex at z < near (or with a non-finite or off-range projection, |u|, |v| >= 2^20 px, or a
//             vertex index outside the mesh) is dropped whole and counted.  GL would clip it: the one deviation.
//   colour    attribute a_i = f32((f32(v) - f32(offset)) / scale); b_i = w_i / S; colour = f32((b0*a0 + b1*a1) + b2*a2)
//             in f64, rounded once; alpha 1.
#pragma once
#include <cmath>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace raster {

constexpr int kSubBits = 8;                    // sub-pixel bits of the snapped grid
constexpr int kSub = 1 << kSubBits;
constexpr double kSnapLimit = 268435456.0;     // 2^28 snapped units = 2^20 px: products of two differences stay < 2^59
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kMaxSide = 16384;                // h, w limit (pixel centres * 256 stay far inside int32)

enum FaceStatus : int { kFaceOk = 0, kFaceDropped = 1, kFaceDegenerate = 2 };

struct Camera {      // one item's K (row-major 3x3) and [R|t] (row-major 3x4)
  double K[9];
  double Rt[12];
};

struct Face {
  int32_t x[3], y[3];     // snapped screen coordinates, oriented: area2 > 0
  double z[3];            // camera depth of the three vertices (same order)
  int32_t vi[3];          // vertex indices (same order)
  int64_t area2;
  int c0, c1, r0, r1;     // pixel box clamped to the image (empty when c0 > c1 or r0 > r1)
  int status;
};

ISR_HD int floor_sub(int32_t a) { return a >> kSubBits; }             // floor(a / 256)
ISR_HD int ceil_sub(int32_t a) { return -((-a) >> kSubBits); }        // ceil(a / 256)

// Project one vertex; false when it is behind the near plane or does not land on the snapped grid.
ISR_HD bool project_vertex(const float* v, const Camera& cam, double near_, int32_t* xs, int32_t* ys, double* zc) {
  const double vx = (double)v[0], vy = (double)v[1], vz = (double)v[2];
  const double* R = cam.Rt;
  const double x = ((R[0] * vx + R[1] * vy) + R[2] * vz) + R[3];
  const double y = ((R[4] * vx + R[5] * vy) + R[6] * vz) + R[7];
  const double z = ((R[8] * vx + R[9] * vy) + R[10] * vz) + R[11];
  *zc = z;
  if (!(z >= near_)) return false;
  const double* K = cam.K;
  const double u = (K[0] * x + K[1] * y) / z + K[2];
  const double w = (K[3] * x + K[4] * y) / z + K[5];
  const double su = rint(u * (double)kSub), sv = rint(w * (double)kSub);
  if (!(su > -kSnapLimit && su < kSnapLimit && sv > -kSnapLimit && sv < kSnapLimit)) return false;
  *xs = (int32_t)su;
  *ys = (int32_t)sv;
  return true;
}

ISR_HD void setup_face(const float* verts, int n_vert, const int32_t* faces, int f, const Camera& cam, double near_,
                              int h, int w, Face* out) {
  Face& F = *out;
  F.status = kFaceDropped;
  F.c0 = F.r0 = 0;
  F.c1 = F.r1 = -1;
  F.area2 = 0;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const int32_t i = faces[3 * (size_t)f + k];
    F.vi[k] = i;
    if (i < 0 || i >= n_vert) {
      ok = false;
      F.x[k] = F.y[k] = 0;
      F.z[k] = 0.0;
      continue;
    }
    if (!project_vertex(verts + 3 * (size_t)i, cam, near_, &F.x[k], &F.y[k], &F.z[k])) {
      ok = false;
      F.x[k] = F.y[k] = 0;
    }
  }
  if (!ok) return;
  int64_t a2 = (int64_t)(F.x[1] - F.x[0]) * (int64_t)(F.y[2] - F.y[0]) - (int64_t)(F.y[1] - F.y[0]) * (int64_t)(F.x[2] - F.x[0]);
  if (a2 == 0) {
    F.status = kFaceDegenerate;
    return;
  }
  if (a2 < 0) {        // orient: swap vertices 1 and 2
    const int32_t tx = F.x[1], ty = F.y[1], ti = F.vi[1];
    const double tz = F.z[1];
    F.x[1] = F.x[2]; F.y[1] = F.y[2]; F.vi[1] = F.vi[2]; F.z[1] = F.z[2];
    F.x[2] = tx; F.y[2] = ty; F.vi[2] = ti; F.z[2] = tz;
    a2 = -a2;
  }
  F.area2 = a2;
  F.status = kFaceOk;
  int32_t xmin = F.x[0], xmax = F.x[0], ymin = F.y[0], ymax = F.y[0];
  for (int k = 1; k < 3; ++k) {
    xmin = F.x[k] < xmin ? F.x[k] : xmin;
    xmax = F.x[k] > xmax ? F.x[k] : xmax;
    ymin = F.y[k] < ymin ? F.y[k] : ymin;
    ymax = F.y[k] > ymax ? F.y[k] : ymax;
  }
  const int c0 = ceil_sub(xmin), c1 = floor_sub(xmax), r0 = ceil_sub(ymin), r1 = floor_sub(ymax);
  F.c0 = c0 < 0 ? 0 : c0;
  F.c1 = c1 > w - 1 ? w - 1 : c1;
  F.r0 = r0 < 0 ? 0 : r0;
  F.r1 = r1 > h - 1 ? h - 1 : r1;
}

// Edge a -> b of an oriented face at the pixel centre (px, py) in snapped units; `in` applies the top-left rule.
ISR_HD int64_t edge(int32_t xa, int32_t ya, int32_t xb, int32_t yb, int64_t px, int64_t py, bool* in) {
  const int64_t dx = (int64_t)xb - xa, dy = (int64_t)yb - ya;
  const int64_t e = dx * (py - ya) - dy * (px - xa);
  const bool top_left = dy < 0 || (dy == 0 && dx > 0);
  *in = e > 0 || (e == 0 && top_left);
  return e;
}

// Coverage of pixel (r, c) by an ok face: the integer barycentrics lam[i] (weight of vertex i, sum = area2).
ISR_HD bool cover(const Face& F, int r, int c, int64_t* lam) {
  const int64_t px = (int64_t)c * kSub, py = (int64_t)r * kSub;
  bool i0, i1, i2;
  lam[0] = edge(F.x[1], F.y[1], F.x[2], F.y[2], px, py, &i0);
  lam[1] = edge(F.x[2], F.y[2], F.x[0], F.y[0], px, py, &i1);
  lam[2] = edge(F.x[0], F.y[0], F.x[1], F.y[1], px, py, &i2);
  return i0 && i1 && i2;
}

// w_i = lambda_i / z_i, S their sum; returns z_pix.
ISR_HD double pixel_depth(const Face& F, const int64_t* lam, double* wgt, double* S) {
  wgt[0] = (double)lam[0] / F.z[0];
  wgt[1] = (double)lam[1] / F.z[1];
  wgt[2] = (double)lam[2] / F.z[2];
  *S = (wgt[0] + wgt[1]) + wgt[2];
  return (double)F.area2 / *S;
}

ISR_HD uint32_t f32_bits(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  return c.u;
}
ISR_HD float bits_f32(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}

// The fragment of face f at pixel (r, c): false when not covered or outside [near, far]; else its z-buffer key.
ISR_HD bool fragment_key(const Face& F, int f, int r, int c, double near_, double far_, unsigned long long* key) {
  int64_t lam[3];
  if (!cover(F, r, c, lam)) return false;
  double wgt[3], S;
  const double zp = pixel_depth(F, lam, wgt, &S);
  if (!(zp >= near_ && zp <= far_)) return false;
  *key = ((unsigned long long)f32_bits((float)zp) << 32) | (unsigned long long)((uint32_t)f + 1u);
  return true;
}

// The key a pixel starts a draw with: empty after a clear, else what the frame buffer holds (face field 0).
ISR_HD unsigned long long initial_key(int clear, float alpha, float depth) {
  if (clear || !(alpha == 1.0f) || !(depth > 0.0f)) return kEmptyKey;
  return (unsigned long long)f32_bits(depth) << 32;
}

ISR_HD float attribute(float v, float o, float scale) {
  const float d = v - o;
  return (float)((double)d / (double)scale);      // f64 quotient of two f32, rounded once: the correctly rounded f32 quotient
}

// Resolve pixel (r, c) whose winning key is `key`: writes rgba (4 floats) and depth in place; returns 1 when the pixel is
// covered afterwards.  A key with face field 0 keeps what the frame buffer holds.
ISR_HD int resolve_pixel(unsigned long long key, int clear, const float* verts, int n_vert, const int32_t* faces,
                                const Camera& cam, double near_, int h, int w, const float* offset3, float scale, int r, int c,
                                float* rgba, float* depth) {
  if (key == kEmptyKey) {
    if (clear) {
      rgba[0] = rgba[1] = rgba[2] = rgba[3] = 0.0f;
      *depth = 0.0f;
      return 0;
    }
    return rgba[3] == 1.0f ? 1 : 0;
  }
  const uint32_t lo = (uint32_t)(key & 0xFFFFFFFFull);
  if (lo == 0u) return 1;
  Face F;
  setup_face(verts, n_vert, faces, (int)(lo - 1u), cam, near_, h, w, &F);
  int64_t lam[3];
  cover(F, r, c, lam);
  double wgt[3], S;
  const double zp = pixel_depth(F, lam, wgt, &S);
  const double b0 = wgt[0] / S, b1 = wgt[1] / S, b2 = wgt[2] / S;
  for (int k = 0; k < 3; ++k) {
    const double a0 = (double)attribute(verts[3 * (size_t)F.vi[0] + k], offset3[k], scale);
    const double a1 = (double)attribute(verts[3 * (size_t)F.vi[1] + k], offset3[k], scale);
    const double a2 = (double)attribute(verts[3 * (size_t)F.vi[2] + k], offset3[k], scale);
    rgba[k] = (float)((b0 * a0 + b1 * a1) + b2 * a2);
  }
  rgba[3] = 1.0f;
  *depth = (float)zp;
  return 1;
}

}  // namespace raster
}  // namespace isr
