// icp_plane.hpp — point-to-plane ICP with robust weights: the arithmetic of include/isr_icp_plane.h, written once and compiled
// twice — into the kernels of csrc/nn_batched.hip and into the host entry isr_icp_point_to_plane_batch_host, and by a plain
// C++ compiler for tools/icp_plane_host_check.cpp.  Everything is built with -ffp-contract=off; only + - * / sqrt fma appear,
// so host and device give the same bits.
//
// THE RULE (icp.py:101-103 with TransformationEstimationPointToPlane and a robust kernel; what Open3D does there is restated
// from memory and unpinned — see the DEVIATIONS at the end).
//
// PASS it, for the item's 4x4 T (rows 0..2 used) and every source point s (f32 read as f64):
//   p  = T s                                     xform: fma(T[2], z, fma(T[1], y, fma(T[0], x, T[3]))) per row
//   t  = the exact nearest target of p, the lowest index on equality; squared distances in f64 by
//        e = p - t;  s2 = fma(e.z, e.z, fma(e.y, e.y, e.x * e.x))
//   the pair COUNTS iff s2 <= threshold * threshold
//   fitness = n / Ns,  rmse = sqrt(sum s2 / n) (0 for n = 0): Euclidean, whatever the estimator
//
// ROW of a counting pair (row(); nt = the matched target's normal, f32 read as f64, used AS GIVEN: not normalised):
//   r  = fma(e.z, nt.z, fma(e.y, nt.y, e.x * nt.x))
//   c  = p x nt:  c.x = fma(p.y, nt.z, -(p.z * nt.y)),  c.y = fma(p.z, nt.x, -(p.x * nt.z)),  c.z = fma(p.x, nt.y, -(p.y * nt.x))
//   J  = (c.x, c.y, c.z, nt.x, nt.y, nt.z)
//   w  = weight(r):   L2 1;   Huber  |r| <= k ? 1 : k / |r|;   Tukey  |r| <= k ? (1 - (r/k)(r/k))^2 : 0
//   wJ[i] = w * J[i];   A[i][j] = wJ[i] * J[j] (i <= j);   b[i] = wJ[i] * r;   wr2 = (w * r) * r
// Negating nt negates r, c and hence every J[i] and wJ[i] exactly (rounding is symmetric), leaves w alone (it reads |r| and
// r * r), and A, b, wr2 are products of two negated factors: (-a)(-b) = ab bit for bit.  THE RESULT DOES NOT DEPEND ON THE
// SIGN OF A NORMAL.
//
// SUMS, all f64, kSums = 31 per item: [0] sum d (d = sqrt(s2)), [1] sum s2, [2] n, [3..23] the upper triangle of sum w J J^T
// row by row, [24..29] sum w J r, [30] sum w r^2.  A row that does not count (and a row past Ns in the last block) adds +0.0
// to each.  Order (tree64 / reduce_blocks here; on the device block_tree_sums of csrc/nn_batched.hip and reduce_blocks of
// csrc/icp_loop.hpp, which both estimators share):
//   per 64 rows the tree v[l] += v[l + s], s = 32, 16, .. 1 (row l = 0 holds the sum);
//   per 256-row block ((w0 + w1) + w2) + w3;
//   lane l of kLanes = 16 adds blocks l, l + 16, .. in that order onto 0.0; the 16 partials are added in lane order onto 0.0.
// A function of the inputs and Ns only; no float atomics.
//
// END OF A PASS (finish_pass), tested in this order:
//   1 converged   it > 0 and |fitness - previous| < rel_fitness and |rmse - previous| < rel_rmse     status 0
//   2 it >= max_iter                                                                                status 1
//   3 n < 6                                                                                         status 2
//   4 singular    solve6 fails                                                                      status 3
// Any of them stops the item with the T it had.  Otherwise T <- dT T, it <- it + 1.
//
// SOLVE (solve6): A x = -b by Cholesky A = L L^T, column by column; every inner product is  s = fma(-L[i][k], L[j][k], s)
// for k ascending from s = A[i][j]; a pivot that is not > 0, or not finite, is a singular system, and so is a solution with
// a non-finite entry.  y = L^-1 (-b) forwards, x = L^-T y backwards, each by the same fma chain then one division.
//
// UPDATE (compose): x = (alpha, beta, gamma, tx, ty, tz).  The rotation of dT is that of the unit quaternion of
// (1, alpha/2, beta/2, gamma/2): a proper rotation whatever x, about the axis (alpha, beta, gamma) by 2 atan(|.| / 2), made
// with + - * / sqrt only.  T <- dT T row by row:  fma(R[a][2], T[2][b], fma(R[a][1], T[1][b], R[a][0] * T[0][b]))  (+ t[a] for b = 3).
//
// DEVIATIONS, all UNPINNED (Open3D is not available to compare against; stated from memory): Open3D composes
// Rz(gamma) Ry(beta) Rx(alpha) from the same solution x, which agrees with the quaternion form to second order in the step
// and has the same fixed points (x = 0); it solves the 6x6 system with Eigen's LDLT and stops on a failed solve; its robust
// kernels weight the same plane residual r with the same Huber / Tukey formulas; its correspondence test is d < threshold on
// a KD-tree's doubles (here s2 <= threshold^2).
#pragma once
#include "hd.hpp"

namespace isr {
namespace icp_plane {

constexpr int kSums = 31;
constexpr int kA = 3, kB = 24, kWr2 = 30;       // where A's upper triangle, b and sum w r^2 start
constexpr int kLanes = 16;                      // kIcpLanes of csrc/icp_loop.hpp (asserted there)
constexpr int kStateDoubles = 24;               // T 4x4 | fitness, rmse, iterations, correspondences | status, sum w r^2, 0, 0
constexpr int kL2 = 0, kHuber = 1, kTukey = 2;  // ISR_ICP_L2 / _HUBER / _TUKEY
constexpr int kConverged = 0, kMaxIter = 1, kFewPairs = 2, kSingular = 3;
constexpr int kMinPairs = 6;

ISR_HD double fma64(double a, double b, double c) { return __builtin_fma(a, b, c); }
ISR_HD double abs64(double a) { return __builtin_fabs(a); }
ISR_HD double sqrt64(double a) { return __builtin_sqrt(a); }
ISR_HD bool finite64(double a) { return abs64(a) <= 1.7976931348623157e308; }      // false for NaN and the infinities

// p = T s, the chain of xform64 (csrc/nn_batched.hip)
ISR_HD void xform(const double* T, float x, float y, float z, double* p) {
  const double dx = x, dy = y, dz = z;
  p[0] = fma64(T[2], dz, fma64(T[1], dy, fma64(T[0], dx, T[3])));
  p[1] = fma64(T[6], dz, fma64(T[5], dy, fma64(T[4], dx, T[7])));
  p[2] = fma64(T[10], dz, fma64(T[9], dy, fma64(T[8], dx, T[11])));
}

// squared distance of p and a target (f32 read as f64)
ISR_HD double dist2(const double* p, double tx, double ty, double tz) {
  const double ex = p[0] - tx, ey = p[1] - ty, ez = p[2] - tz;
  return fma64(ez, ez, fma64(ey, ey, ex * ex));
}

ISR_HD double weight(int kernel, double k, double r) {
  const double a = abs64(r);
  if (kernel == kHuber) return a <= k ? 1.0 : k / a;
  if (kernel == kTukey) {
    if (!(a <= k)) return 0.0;
    const double q = r / k, u = 1.0 - q * q;
    return u * u;
  }
  return 1.0;
}

// The kSums terms of one source point: p, its nearest target t with normal nt; zeros unless the pair counts.
ISR_HD void row(const double* p, const double* t, const double* nt, double threshold, int kernel, double k, double* v) {
#pragma unroll
  for (int i = 0; i < kSums; ++i) v[i] = 0.0;
  const double ex = p[0] - t[0], ey = p[1] - t[1], ez = p[2] - t[2];
  const double s2 = fma64(ez, ez, fma64(ey, ey, ex * ex));
  if (!(s2 <= threshold * threshold)) return;
  v[0] = sqrt64(s2);
  v[1] = s2;
  v[2] = 1.0;
  const double r = fma64(ez, nt[2], fma64(ey, nt[1], ex * nt[0]));
  double J[6], wJ[6];
  J[0] = fma64(p[1], nt[2], -(p[2] * nt[1]));
  J[1] = fma64(p[2], nt[0], -(p[0] * nt[2]));
  J[2] = fma64(p[0], nt[1], -(p[1] * nt[0]));
  J[3] = nt[0];
  J[4] = nt[1];
  J[5] = nt[2];
  const double w = weight(kernel, k, r);
#pragma unroll
  for (int i = 0; i < 6; ++i) wJ[i] = w * J[i];
  int o = kA;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) v[o++] = wJ[i] * J[j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) v[kB + i] = wJ[i] * r;
  v[kWr2] = (w * r) * r;
}

// The tree of 64 rows, in place: a[0] becomes the sum (what lane 0 of wave_sum_down holds).
ISR_HD void tree64(double* a) {
  for (int s = 32; s > 0; s >>= 1)
    for (int l = 0; l < s; ++l) a[l] += a[l + s];
}

// nblk block sums of one term (stride doubles apart) -> the item's sum
ISR_HD double reduce_blocks(const double* part, int nblk, int stride) {
  double lane[kLanes];
  for (int l = 0; l < kLanes; ++l) {
    double s = 0.0;
    for (int i = l; i < nblk; i += kLanes) s += part[(long)i * stride];
    lane[l] = s;
  }
  double s = 0.0;
  for (int l = 0; l < kLanes; ++l) s += lane[l];
  return s;
}

// A x = -b from the sums; false: singular.  Constant bounds throughout, so that on the device L stays in registers.
ISR_HD bool solve6(const double* v, double* x) {
  double L[6][6];
  {
    int o = kA;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) L[j][i] = v[o++];     // the lower triangle holds A, then L, column by column
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma64(-L[j][k], L[j][k], d);
    if (!(d > 0.0) || !finite64(d)) ok = false;
    const double piv = sqrt64(ok ? d : 1.0);
    L[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = fma64(-L[i][k], L[j][k], s);
      L[i][j] = s / piv;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -v[kB + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = fma64(-L[i][k], y[k], s);
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = 5; k > i; --k) s = fma64(-L[k][i], x[k], s);
    x[i] = s / L[i][i];
    if (!finite64(x[i])) ok = false;
  }
  return ok;
}

// T (rows 0..2 of a row-major 4x4) <- dT(x) T
ISR_HD void compose(const double* x, double* T) {
  const double a = 0.5 * x[0], b = 0.5 * x[1], c = 0.5 * x[2];
  const double nq = 1.0 / sqrt64(fma64(c, c, fma64(b, b, fma64(a, a, 1.0))));
  const double qw = nq, qx = a * nq, qy = b * nq, qz = c * nq;
  const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)},
                          {2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)},
                          {2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)}};
  double Tn[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int col = 0; col < 4; ++col) {
      const double s = fma64(R[r][2], T[8 + col], fma64(R[r][1], T[4 + col], R[r][0] * T[col]));
      Tn[4 * r + col] = col == 3 ? s + x[3 + r] : s;
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
}

// What an item carries from pass to pass
struct Loop {
  double prev_fit, prev_rmse;
  int iter, done;
};

// The end of a pass: v the item's kSums sums.  Writes out[0..7] = fitness, rmse, iterations, correspondences, status,
// sum w r^2, 0, 0 (status is kMaxIter while the loop goes on: every double is written in every pass), applies the stop
// rule, and on continuing composes T (12 doubles).
ISR_HD void finish_pass(const double* v, int Ns, int max_iter, double rel_fitness, double rel_rmse, double* T, Loop* st, double* out) {
  const double n = v[2];
  const double fit = n / (double)Ns;
  const double rmse = n > 0 ? sqrt64(v[1] / n) : 0.0;
  const int it = st->iter;
  out[0] = fit; out[1] = rmse; out[2] = (double)it; out[3] = n;
  out[5] = v[kWr2]; out[6] = 0.0; out[7] = 0.0;
  const bool conv = it > 0 && abs64(st->prev_fit - fit) < rel_fitness && abs64(st->prev_rmse - rmse) < rel_rmse;
  int status = -1;
  double x[6];
  if (conv) status = kConverged;
  else if (it >= max_iter) status = kMaxIter;
  else if (n < (double)kMinPairs) status = kFewPairs;
  else if (!solve6(v, x)) status = kSingular;
  if (status >= 0) {
    out[4] = (double)status;
    st->done = 1;
    return;
  }
  out[4] = (double)kMaxIter;
  st->prev_fit = fit; st->prev_rmse = rmse; st->iter = it + 1;
  compose(x, T);
}

// The argument rules of both entries; null when they hold
inline const char* refuse(const void* src, const void* tgt, const void* nrm, const void* state, unsigned long long src_item_stride,
                          int Ns, int Nt, int B, double threshold, int max_iter, int kernel, double k) {
  if (!src || !tgt || !nrm || !state) return "null pointer";
  if (Ns < 1 || Nt < 1) return "Ns and Nt must be at least 1";
  if (B < 0 || B > 65535) return "B must lie in [0, 65535]";
  if (!(threshold > 0) || max_iter < 0) return "threshold must be positive and max_iter non-negative";
  if (kernel != kL2 && kernel != kHuber && kernel != kTukey) return "unknown kernel";
  if (kernel != kL2 && !(k > 0)) return "k must be positive with the Huber and Tukey kernels";
  if (src_item_stride != 0 && src_item_stride < 3ull * (unsigned long long)Ns) return "src_item_stride must be 0 or at least 3 * Ns";
  return nullptr;
}

// The loop as host code over host pointers: an f64 brute-force search, the sums in the stated order.  block_sums:
// ceil(Ns / 256) * kSums doubles of scratch; nearest: Ns ints of scratch (filled by search(item T, nearest) — the caller may
// run it over threads: it is a function of the inputs only).
template <class Search>
inline void host_item(const float* src, int Ns, const float* tgt, const float* nrm, int Nt, double threshold, int max_iter,
                      double rel_fitness, double rel_rmse, int kernel, double k, double* state, double* block_sums, int* nearest,
                      Search search) {
  double* T = state;
  T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
  Loop st{0.0, 0.0, 0, 0};
  const int nblk = (Ns + 255) / 256;
  for (int pass = 0; pass <= max_iter && !st.done; ++pass) {
    search(T, nearest);
    for (int blk = 0; blk < nblk; ++blk) {
      double wave[4][kSums];
      for (int w = 0; w < 4; ++w) {
        double rows[kSums][64];
        for (int l = 0; l < 64; ++l) {
          const long i = (long)blk * 256 + w * 64 + l;
          double v[kSums];
          for (int q = 0; q < kSums; ++q) v[q] = 0.0;
          if (i < Ns) {
            const int j = nearest[i];
            double p[3];
            xform(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], p);
            const double t[3] = {tgt[3 * (long)j], tgt[3 * (long)j + 1], tgt[3 * (long)j + 2]};
            const double nt[3] = {nrm[3 * (long)j], nrm[3 * (long)j + 1], nrm[3 * (long)j + 2]};
            row(p, t, nt, threshold, kernel, k, v);
          }
          for (int q = 0; q < kSums; ++q) rows[q][l] = v[q];
        }
        for (int q = 0; q < kSums; ++q) {
          tree64(rows[q]);
          wave[w][q] = rows[q][0];
        }
      }
      for (int q = 0; q < kSums; ++q) block_sums[(long)blk * kSums + q] = ((wave[0][q] + wave[1][q]) + wave[2][q]) + wave[3][q];
    }
    double v[kSums];
    for (int q = 0; q < kSums; ++q) v[q] = reduce_blocks(block_sums + q, nblk, kSums);
    finish_pass(v, Ns, max_iter, rel_fitness, rel_rmse, T, &st, state + 16);
  }
}

// nearest[i] = the exact nearest target of T src_i, the lowest index on equality, for rows [i0, i1)
inline void host_search(const double* T, const float* src, const float* tgt, int Nt, long i0, long i1, int* nearest) {
  for (long i = i0; i < i1; ++i) {
    double p[3];
    xform(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], p);
    double best = dist2(p, tgt[0], tgt[1], tgt[2]);
    int bi = 0;
    for (int j = 1; j < Nt; ++j) {
      const double s2 = dist2(p, tgt[3 * (long)j], tgt[3 * (long)j + 1], tgt[3 * (long)j + 2]);
      if (s2 < best) { best = s2; bi = j; }
    }
    nearest[i] = bi;
  }
}

}  // namespace icp_plane
}  // namespace isr
