// seq_refit.hpp — the sequence-level pose: one robust Gauss-Newton over the reprojection residuals of every frame's 2D-3D
// matches.  The arithmetic of include/isr_seq_refit.h, written once and compiled twice — into the kernels of
// csrc/seq_refit.hip and into the host entry isr_seq_refit_host, and by a plain C++ compiler for
// tools/seq_refit_host_check.cpp.  Everything is built with -ffp-contract=off; only + - * / sqrt fma appear, so host and
// device give the same bits.  weight, solve6, compose, tree64 and reduce_blocks are icp_plane.hpp's, called as they are.
//
// THE UNKNOWN is Y (rows 0..2 of a row-major 4x4), which maps the model frame to the sequence frame: frame i, whose pose in
// its own sequence is G_i = [R_i | t_i] (12 doubles), sees the model under P_i = G_i Y.  Every frame constrains the same Y.
//
// ROW of frame i, slot m (row()): p = p3d[i][m] (f32 read as f64), u = p2d[i][m] (f32 read as f64), K = K_i (9 doubles,
// every entry read, as csrc/ransac.hip's Cam::k):
//   q  = Y p                      icp_plane::xform: fma(Y[2], z, fma(Y[1], y, fma(Y[0], x, Y[3]))) per row
//   c  = G_i q                    the same chain over doubles (xform_d)
//   h  = K c                      h[a] = fma(K[3a+2], c.z, fma(K[3a+1], c.y, K[3a] * c.x))
//   pu = h[0] / h[2], pv = h[1] / h[2];   r = (pu - u.x, pv - u.y);   rr = fma(r1, r1, r0 * r0);   a = sqrt(rr)
//   w  = frame_w[i] * icp_plane::weight(kernel, k, a)     (frame_w null: every frame weighs 1; the product is still formed)
//   d(pu)/dc = (K[0..2] - pu K[6..8]) / h[2],  d(pv)/dc = (K[3..5] - pv K[6..8]) / h[2]:   D[e][b] = fma(-p_e, K[6+b], K[3e+b]) / h[2]
//   g_e = D[e] R_i   (a row times a matrix):   g_e[b] = fma(D[e][2], R[2][b], fma(D[e][1], R[1][b], D[e][0] * R[0][b]))
//   J_e = (q x g_e, g_e)          the left perturbation Y <- dT(x) Y, x = (alpha, beta, gamma, t):  dq = alpha x q + t;
//                                 (q x g).x = fma(q.y, g.z, -(q.z * g.y)) and cyclically, as icp_plane::row forms p x n
//   wJ_e[i] = w * J_e[i];   A[i][j] = fma(wJ_1[i], J_1[j], wJ_0[i] * J_0[j]) (i <= j);   b[i] = fma(wJ_1[i], r1, wJ_0[i] * r0);
//   wr2 = w * rr
// The row COUNTS iff m < min(counts[i], cap), c.z > 0, rr and w and the 12 entries of J are finite, and w > 0.  A row that
// does not count adds +0.0 to every sum.  counts[i] > cap cannot be seen from the host: it is clamped to cap; a negative
// count is 0.
//
// SUMS, all f64.  Slots 0..30 are icp_plane's kSums, so that solve6 and compose apply as they are: [0] sum a, [1] sum rr,
// [2] rows counted, [3..23] the upper triangle of sum w J^T J row by row, [24..29] sum w J^T r, [30] sum w rr.  A 32nd
// slot, [31] sum w, exists per block and per frame only (frame_stats reads it; the solve does not).  Order:
//   per 64 slots the tree v[l] += v[l + s], s = 32 .. 1 (icp_plane::tree64; wave_sum_down's lane 0);
//   per 256-slot block ((w0 + w1) + w2) + w3;
//   a frame's blocks are those that hold a real slot, nb_i = ceil(min(counts[i], cap) / 256), 0 for a frame of weight 0
//   (none of its rows can count); they start at the frame's slot 0 and are added by icp_plane::reduce_blocks;
//   the frames' sums are added by reduce_blocks again, in frame order (frame i is "block" i).
// A function of the inputs and n only: no float atomics, and — because nb_i does not read cap beyond the clamp, and an
// empty row adds +0.0 — not a function of cap.
//
// END OF A PASS (finish_pass), pass number it = 0, 1, ..; x is solved (solve6) whenever rows >= 6; tested in this order:
//   1 converged   x was solved and max(|x0|, |x1|, |x2|) < tol_r and max(|x3|, |x4|, |x5|) < tol_t          status 0
//   2 rows < 6                                                                                              status 2
//   3 it >= max_iter                                                                                        status 1
//   4 singular    solve6 failed                                                                             status 3
// Any of them stops the call with the Y it had (the converged step is NOT applied: it is below the tolerances).  Otherwise
// Y <- dT(x) Y by icp_plane::compose.  state[16..23] = mean a, rms = sqrt(sum rr / rows), passes (= it), rows, status,
// sum w rr, 0, 0 of the last pass; frame_stats[i] = (rows, sum w, sum w rr, sum rr) of frame i at the last pass.
//
// OWNED, pinned to no library: the reference has no sequence-level estimator (it takes the transform from one image), so
// everything above — the parameterisation, the weights on the pixel norm a, the tolerances on the step, the stop order — is
// this project's.  The robust scale k is in pixels; with k = 6 a 2 px RANSAC inlier keeps a weight of (1 - 1/9)^2 = 0.79.
#pragma once
#include "icp_plane.hpp"

namespace isr {
namespace seq_refit {

namespace ipl = isr::icp_plane;

constexpr int kSums = ipl::kSums;               // what the solve reads
constexpr int kBlockSums = 32;                  // + [31] sum w, per block and per frame
constexpr int kW = 31;
constexpr int kRows = 256;                      // slots per block
constexpr int kStateDoubles = 24;               // Y 4x4 | mean a, rms, passes, rows | status, sum w rr, 0, 0
constexpr int kFrameStats = 4;                  // rows, sum w, sum w rr, sum rr
constexpr int kConverged = 0, kMaxIter = 1, kFewRows = 2, kSingular = 3;
constexpr int kMinRows = 6;
constexpr int kMaxFrames = 65535;               // a frame is a blockIdx.y

// c = G q over doubles, xform's chain
ISR_HD void xform_d(const double* G, const double* q, double* c) {
  c[0] = ipl::fma64(G[2], q[2], ipl::fma64(G[1], q[1], ipl::fma64(G[0], q[0], G[3])));
  c[1] = ipl::fma64(G[6], q[2], ipl::fma64(G[5], q[1], ipl::fma64(G[4], q[0], G[7])));
  c[2] = ipl::fma64(G[10], q[2], ipl::fma64(G[9], q[1], ipl::fma64(G[8], q[0], G[11])));
}

// min(max(count, 0), cap): the slots of a frame that are real
ISR_HD int real_slots(int count, int cap) { return count < 0 ? 0 : (count > cap ? cap : count); }

// The kBlockSums terms of one slot; zeros unless the row counts.  fw: the frame's weight.
ISR_HD void row(const double* Y, const double* G, const double* K, double fw, float px, float py, float pz, float ux, float uy,
                int kernel, double k, double* v) {
#pragma unroll
  for (int i = 0; i < kBlockSums; ++i) v[i] = 0.0;
  double q[3], c[3];
  ipl::xform(Y, px, py, pz, q);
  xform_d(G, q, c);
  if (!(c[2] > 0.0)) return;
  double h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) h[a] = ipl::fma64(K[3 * a + 2], c[2], ipl::fma64(K[3 * a + 1], c[1], K[3 * a] * c[0]));
  const double pr[2] = {h[0] / h[2], h[1] / h[2]};
  const double r0 = pr[0] - (double)ux, r1 = pr[1] - (double)uy;
  const double rr = ipl::fma64(r1, r1, r0 * r0);
  const double a = ipl::sqrt64(rr);
  const double w = fw * ipl::weight(kernel, k, a);
  double J[2][6];
  bool fin = ipl::finite64(rr) && ipl::finite64(w);
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    double D[3], g[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) D[b] = ipl::fma64(-pr[e], K[6 + b], K[3 * e + b]) / h[2];
#pragma unroll
    for (int b = 0; b < 3; ++b) g[b] = ipl::fma64(D[2], G[8 + b], ipl::fma64(D[1], G[4 + b], D[0] * G[b]));
    J[e][0] = ipl::fma64(q[1], g[2], -(q[2] * g[1]));
    J[e][1] = ipl::fma64(q[2], g[0], -(q[0] * g[2]));
    J[e][2] = ipl::fma64(q[0], g[1], -(q[1] * g[0]));
    J[e][3] = g[0];
    J[e][4] = g[1];
    J[e][5] = g[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) fin = fin && ipl::finite64(J[e][i]);
  }
  if (!fin || !(w > 0.0)) return;
  v[0] = a;
  v[1] = rr;
  v[2] = 1.0;
  double wJ0[6], wJ1[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    wJ0[i] = w * J[0][i];
    wJ1[i] = w * J[1][i];
  }
  int o = ipl::kA;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) v[o++] = ipl::fma64(wJ1[i], J[1][j], wJ0[i] * J[0][j]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) v[ipl::kB + i] = ipl::fma64(wJ1[i], r1, wJ0[i] * r0);
  v[ipl::kWr2] = w * rr;
  v[kW] = w;
}

// The blocks of frame i that the sums read
ISR_HD int frame_blocks(int count, int cap, double fw) {
  if (!(fw != 0.0)) return 0;
  return (real_slots(count, cap) + kRows - 1) / kRows;
}

// frame_stats[0..3] from a frame's kBlockSums sums
ISR_HD void frame_stats(const double* fs, double* out) {
  out[0] = fs[2];
  out[1] = fs[kW];
  out[2] = fs[ipl::kWr2];
  out[3] = fs[1];
}

// The end of pass `it`: v the kSums sums over all frames.  Writes Y's row 3 and out[0..7] (state[16..23]); returns true
// when the call has stopped; otherwise composes Y (12 doubles).
ISR_HD bool finish_pass(const double* v, int it, int max_iter, double tol_r, double tol_t, double* Y, double* out) {
  const double n = v[2];
  out[0] = n > 0 ? v[0] / n : 0.0;
  out[1] = n > 0 ? ipl::sqrt64(v[1] / n) : 0.0;
  out[2] = (double)it;
  out[3] = n;
  out[5] = v[ipl::kWr2];
  out[6] = 0.0;
  out[7] = 0.0;
  double x[6];
  const bool enough = !(n < (double)kMinRows);
  const bool solved = enough && ipl::solve6(v, x);
  bool small = solved;
#pragma unroll
  for (int i = 0; i < 3; ++i) small = small && ipl::abs64(x[i]) < tol_r && ipl::abs64(x[3 + i]) < tol_t;
  int status = -1;
  if (small) status = kConverged;
  else if (!enough) status = kFewRows;
  else if (it >= max_iter) status = kMaxIter;
  else if (!solved) status = kSingular;
  if (status >= 0) {
    out[4] = (double)status;
    return true;
  }
  out[4] = (double)kMaxIter;
  ipl::compose(x, Y);
  return false;
}

// The argument rules of both entries; null when they hold
inline const char* refuse(const void* p3d, const void* p2d, const void* counts, const void* K, const void* G, const void* state,
                          const void* frame_stats, int n, int cap, int kernel, double k, int max_iter) {
  if (cap < 1) return "cap must be at least 1";
  if (n < 0 || n > kMaxFrames) return "n must lie in [0, 65535]";
  if (!state || (n > 0 && (!p3d || !p2d || !counts || !K || !G || !frame_stats))) return "null pointer";   // n = 0: empty arrays
  if (max_iter < 0) return "max_iter must be non-negative";
  if (kernel != ipl::kL2 && kernel != ipl::kHuber && kernel != ipl::kTukey) return "unknown kernel";
  if (kernel != ipl::kL2 && !(k > 0)) return "k must be positive with the Huber and Tukey kernels";
  return nullptr;
}

// One frame's kBlockSums sums as host code: fs[0..31].  block_sums: frame_blocks * kBlockSums doubles of scratch.
inline void host_frame(const float* p3d, const float* p2d, int count, int cap, double fw, const double* K, const double* G,
                       const double* Y, int kernel, double k, double* block_sums, double* fs) {
  const int nb = frame_blocks(count, cap, fw), real = real_slots(count, cap);
  for (int blk = 0; blk < nb; ++blk) {
    double wave[4][kBlockSums];
    for (int w = 0; w < 4; ++w) {
      double rows[kBlockSums][64];
      for (int l = 0; l < 64; ++l) {
        const long m = (long)blk * kRows + w * 64 + l;
        double v[kBlockSums];
        for (int s = 0; s < kBlockSums; ++s) v[s] = 0.0;
        if (m < real) row(Y, G, K, fw, p3d[3 * m], p3d[3 * m + 1], p3d[3 * m + 2], p2d[2 * m], p2d[2 * m + 1], kernel, k, v);
        for (int s = 0; s < kBlockSums; ++s) rows[s][l] = v[s];
      }
      for (int s = 0; s < kBlockSums; ++s) {
        ipl::tree64(rows[s]);
        wave[w][s] = rows[s][0];
      }
    }
    for (int s = 0; s < kBlockSums; ++s) block_sums[(long)blk * kBlockSums + s] = ((wave[0][s] + wave[1][s]) + wave[2][s]) + wave[3][s];
  }
  for (int s = 0; s < kBlockSums; ++s) fs[s] = ipl::reduce_blocks(block_sums + s, nb, kBlockSums);
}

// The sums of one pass at Y as host code over host pointers: v[0..30] and stats (n, 4).  frame_sums: n * kBlockSums doubles
// of scratch; frames(fn): calls fn(i) for every i in [0, n), in any order or in parallel (a frame's sums are a function of
// the inputs only).
template <class Frames>
inline void host_sums(const float* p3d, const float* p2d, const int* counts, const double* frame_w, const double* K,
                      const double* G, int n, int cap, int kernel, double k, const double* Y, double* v, double* stats,
                      double* frame_sums, Frames frames) {
  const int nblk = (cap + kRows - 1) / kRows;
  frames([&](long i) {
    double* scratch = new double[(size_t)(nblk > 0 ? nblk : 1) * kBlockSums];
    host_frame(p3d + (size_t)i * cap * 3, p2d + (size_t)i * cap * 2, counts[i], cap, frame_w ? frame_w[i] : 1.0, K + 9 * i,
               G + 12 * i, Y, kernel, k, scratch, frame_sums + (size_t)i * kBlockSums);
    delete[] scratch;
    frame_stats(frame_sums + (size_t)i * kBlockSums, stats + (size_t)i * kFrameStats);
  });
  for (int s = 0; s < kSums; ++s) v[s] = ipl::reduce_blocks(frame_sums + s, n, kBlockSums);
}

// The loop as host code over host pointers; frame_sums and frames: host_sums'.
template <class Frames>
inline void host_loop(const float* p3d, const float* p2d, const int* counts, const double* frame_w, const double* K,
                      const double* G, int n, int cap, int kernel, double k, int max_iter, double tol_r, double tol_t,
                      double* state, double* stats, double* frame_sums, Frames frames) {
  double* Y = state;
  Y[12] = 0; Y[13] = 0; Y[14] = 0; Y[15] = 1;
  for (int it = 0; it <= max_iter; ++it) {
    double v[kSums];
    host_sums(p3d, p2d, counts, frame_w, K, G, n, cap, kernel, k, Y, v, stats, frame_sums, frames);
    if (finish_pass(v, it, max_iter, tol_r, tol_t, Y, state + 16)) break;
  }
}

}  // namespace seq_refit
}  // namespace isr
