// ransac_seq.hpp — the stopping rule of OpenCV's sequential RANSAC loop, in a form that host and device decide alike.
//
// OpenCV's RANSACPointSetRegistrator::run (calib3d; restated from memory — OpenCV is not available to this build):
//
//   niters = itr; best = 0
//   for h = 0, 1, ...  while h < niters:
//       if hypothesis h has a model and count[h] > max(best, 3):            // modelPoints - 1 = 3
//           best = count[h]; winner = h
//           niters = RANSACUpdateNumIters(confidence, ep = (M - best) / M, 4, niters)
//   RANSACUpdateNumIters(p, ep, m, n): num = max(1 - p, DBL_MIN); den = 1 - (1 - ep)^m
//       den < DBL_MIN -> 0;  log(den) >= 0 or -log(num) >= n * -log(den) -> n;  else cvRound(log(num) / log(den))
//
// The update is min(n, f(best)) with f non-increasing in best, so after any prefix niters = min(itr, f(running max of
// the counts > 3)), and hypothesis h runs iff h < niters(prefix max before h).  Hence the parallel form:
//   h_stop = the first h with seq_stop(max count before h, M, h, num), else itr;   n_eval = h_stop;
//   winner = the lowest h with the maximal count in [0, h_stop).
//
// seq_stop decides  h >= cvRound(log(num) / log(d))  without log / pow (libm and the device library may round those
// differently):  log(num) / log(d) < h + 1/2  <=>  num > d^h sqrt(d)  (d < 1).  It tests  num >= d^h * sqrt(d)  with
// d^h by binary powering in a fixed order — IEEE multiplications and one correctly rounded sqrt, the same bits in the
// host build (isr_ransac_seq_host), the device kernels and tests/seq_ransac_ref.py.  It differs from cv2's log form only
// where log(num) / log(d) lies within rounding of a half-integer.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace isr_seq {

// num = max(1 - confidence, DBL_MIN): cv2's numerator (confidence >= 1 still stops, once d^h underflows it)
__host__ __device__ inline double seq_num(double confidence) {
  const double n = 1.0 - confidence;
  return n > DBL_MIN ? n : DBL_MIN;
}

// Does the sequential loop stop before hypothesis h, given the best count c of the hypotheses before it?
// (h >= itr stops too: the caller's bound.)
__host__ __device__ inline bool seq_stop(int c, int M, int h, double num) {
  if (c <= 3 || M <= 0) return false;               // no model yet: niters is still itr
  const double ep = (double)(M - c) / (double)M;    // cv2's outlier ratio
  const double t = 1.0 - ep;
  const double t2 = t * t;
  const double d = 1.0 - t2 * t2;
  if (d < DBL_MIN) return true;                     // niters = 0
  if (!(d < 1.0)) return false;                     // log(d) >= 0: niters stays
  double base = d, q = 1.0;
  for (int e = h; e > 0; e >>= 1) {
    if (e & 1) q = q * base;
    base = base * base;
  }
  return num >= q * sqrt(d);
}

// The loop over host arrays (isr_ransac_seq_host): winner (-1: no hypothesis with a count > 3) and n_eval = h_stop.
inline void seq_scan(const int32_t* n_inl, const uint8_t* ok, int H, int M, double num, int* winner, int* n_eval) {
  int c = 0, w = -1, h = 0;
  for (; h < H; ++h) {
    if (seq_stop(c, M, h, num)) break;
    const int v = ok[h] ? n_inl[h] : 0;
    if (v > c && v > 3) w = h;
    if (v > c) c = v;
  }
  *winner = w;
  *n_eval = h;
}

}  // namespace isr_seq
