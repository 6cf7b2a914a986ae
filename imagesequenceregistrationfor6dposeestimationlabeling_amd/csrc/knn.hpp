// knn.hpp — the exact k nearest neighbours of a point and the local frame (normal) of a neighbourhood, stated once and
// compiled for host and device.  csrc/knn.hip holds the kernels and the C entries (include/isr_knn.h); a plain C++ compiler
// can include this header too (tools/knn_host_check.cpp).
//
// The search.  In f32 (csrc/radius_count.hpp's chain, written out: everything is built with -ffp-contract=off)
//     dx = t.x-q.x; dy = t.y-q.y; dz = t.z-q.z;  d2 = fmaf(dz, dz, fmaf(dy, dy, dx*dx))
// and a target's key is the 64-bit integer (bits of d2) << 32 | index: d2 is never negative, so its bits order as it does,
// and the K smallest keys in ascending order ARE the row: (d2, index) ascending, the lowest index first among equals, at the
// cut as well as inside the list.  A NaN d2 (non-finite input only) takes the bits 0x7fc00000, so that every pass of the
// device's select sees one value for it; the indices stay in [0, Nt).
//
// The frame: include/isr_knn.h states it line by line; local_frame below is that text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace knn {

constexpr int kMaxK = 1024;
constexpr int kMaxTargets = 1 << 24;
constexpr int kJacobiSweeps = 30;
constexpr double kJacobiTol = 1e-30;   // stop once sum_{p<q} c_pq^2 <= kJacobiTol sum_i c_ii^2

ISR_HD uint32_t d2_bits(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = tx - qx, dy = ty - qy, dz = tz - qz;
  union { float f; uint32_t u; } c;
  c.f = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  return c.f != c.f ? 0x7fc00000u : c.u;
}

ISR_HD float bits_d2(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}

ISR_HD uint64_t make_key(uint32_t bits, int j) { return ((uint64_t)bits << 32) | (uint32_t)j; }

// The definition as host code, one query: keys is scratch for Nt entries; idx, d2 (nullable) the row's K entries.
inline void knn_row_host(const float* q, const float* tgt, int Nt, int K, uint64_t* keys, int32_t* idx, float* d2) {
  for (int j = 0; j < Nt; ++j)
    keys[j] = make_key(d2_bits(q[0], q[1], q[2], tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2]), j);
  std::nth_element(keys, keys + (K - 1), keys + Nt);
  std::sort(keys, keys + K);
  for (int r = 0; r < K; ++r) {
    idx[r] = (int32_t)(keys[r] & 0xFFFFFFFFu);
    if (d2) d2[r] = bits_d2((uint32_t)(keys[r] >> 32));
  }
}

ISR_HD int clamp_index(int j, int N) { return j < 0 ? 0 : (j < N ? j : N - 1); }

// One rotation (p, q) of the cyclic Jacobi iteration on the symmetric 3 x 3 a (full storage), v <- v G.  csrc/epnp.hpp's
// rotation: theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (0.5 / theta for
// |theta| > 1e150), c = 1 / sqrt(t^2 + 1), s = t c.
ISR_HD void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double app = a[p][p], aqq = a[q][q];
  const double th = (aqq - app) / (2.0 * apq);
  const double at = th < 0.0 ? -th : th;
  double t = at > 1e150 ? 0.5 / th : 1.0 / (at + sqrt(th * th + 1.0));
  if (at <= 1e150 && th < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const int k = 3 - p - q;                     // the third axis
  const double akp = a[k][p], akq = a[k][q];
  a[k][p] = a[p][k] = c * akp - s * akq;
  a[k][q] = a[q][k] = s * akp + c * akq;
  a[p][p] = app - t * apq;
  a[q][q] = aqq + t * apq;
  a[p][q] = a[q][p] = 0.0;
  for (int r = 0; r < 3; ++r) {
    const double vp = v[r][p], vq = v[r][q];
    v[r][p] = c * vp - s * vq;
    v[r][q] = s * vp + c * vq;
  }
}

// a = v diag(l) v^T: l ascending (a tie keeps the lower axis first), the columns of v the eigenvectors in that order.
ISR_HD void eigen_sym3(double (&a)[3][3], double (&l)[3], double (&v)[3][3]) {
  double w[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double dg = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (!(off > kJacobiTol * dg)) break;
    jacobi_rotate(a, w, 0, 1);
    jacobi_rotate(a, w, 0, 2);
    jacobi_rotate(a, w, 1, 2);
  }
  int order[3] = {0, 1, 2};
  for (int i = 1; i < 3; ++i)                  // insertion sort: stable
    for (int j = i; j > 0 && a[order[j]][order[j]] < a[order[j - 1]][order[j - 1]]; --j) {
      const int t = order[j];
      order[j] = order[j - 1];
      order[j - 1] = t;
    }
  for (int c = 0; c < 3; ++c) {
    l[c] = a[order[c]][order[c]];
    for (int r = 0; r < 3; ++r) v[r][c] = w[r][order[c]];
  }
}

// Point i's curvatures (3) and frame (3 x 3 row-major, columns = eigenvectors) from its row of K neighbours.
ISR_HD void local_frame(const float* pts, int N, const int32_t* row, int K, int i, int disambiguate, double* curv,
                            double* frame) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int r = 0; r < K; ++r) {
    const float* p = pts + 3 * (size_t)clamp_index(row[r], N);
    s[0] += (double)p[0];
    s[1] += (double)p[1];
    s[2] += (double)p[2];
  }
  const double kd = (double)K;
  const double m[3] = {s[0] / kd, s[1] / kd, s[2] / kd};
  double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  for (int r = 0; r < K; ++r) {
    const float* p = pts + 3 * (size_t)clamp_index(row[r], N);
    const double dx = (double)p[0] - m[0], dy = (double)p[1] - m[1], dz = (double)p[2] - m[2];
    cxx = fma(dx, dx, cxx);
    cxy = fma(dx, dy, cxy);
    cxz = fma(dx, dz, cxz);
    cyy = fma(dy, dy, cyy);
    cyz = fma(dy, dz, cyz);
    czz = fma(dz, dz, czz);
  }
  double a[3][3] = {{cxx / kd, cxy / kd, cxz / kd}, {cxy / kd, cyy / kd, cyz / kd}, {cxz / kd, cyz / kd, czz / kd}};
  double l[3], v[3][3];
  eigen_sym3(a, l, v);
  if (disambiguate) {
    const float* pi = pts + 3 * (size_t)i;
    int n0 = 0, n2 = 0;
    for (int r = 0; r < K; ++r) {
      const float* p = pts + 3 * (size_t)clamp_index(row[r], N);
      const double dx = (double)p[0] - (double)pi[0], dy = (double)p[1] - (double)pi[1], dz = (double)p[2] - (double)pi[2];
      if (fma(v[2][0], dz, fma(v[1][0], dy, v[0][0] * dx)) > 0.0) ++n0;
      if (fma(v[2][2], dz, fma(v[1][2], dy, v[0][2] * dx)) > 0.0) ++n2;
    }
    if (2 * n0 < K)
      for (int r = 0; r < 3; ++r) v[r][0] = -v[r][0];
    if (2 * n2 < K)
      for (int r = 0; r < 3; ++r) v[r][2] = -v[r][2];
    v[0][1] = v[1][2] * v[2][0] - v[2][2] * v[1][0];      // column 1 = column 2 x column 0
    v[1][1] = v[2][2] * v[0][0] - v[0][2] * v[2][0];
    v[2][1] = v[0][2] * v[1][0] - v[1][2] * v[0][0];
  }
  for (int c = 0; c < 3; ++c) curv[c] = l[c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) frame[3 * r + c] = v[r][c];
}

}  // namespace knn
}  // namespace isr
