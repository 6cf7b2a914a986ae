// refine_obj.hpp — the device arithmetic of the a16 objective (csrc/refine_pose.hip), shared by the single-item and batched
// entries there and by the device BFGS of csrc/refine_bfgs.hip: one copy of every per-point body, block reduction and
// item reduction, so every caller gets the bits of isr_refine_objective.
#pragma once
#include "isr_common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocks = 64;
constexpr int kAcc = 14;

struct P34 { double p[12]; double k[9]; };

// ---- interpolation != 'bilinear' (pose_refine.py:60-68 forwards `mode=interpolation` to F.grid_sample): separable taps
// per axis, as torch's grid sampler defines them for align_corners=False, padding_mode='border':
//   nearest  the source coordinate is clipped to [0, res-1], then rounded half-to-even (nearbyint); no gradient;
//   bicubic  the source coordinate is NOT clipped; cubic-convolution coefficients with A = -0.75 on the fractional part;
//            each of the four taps is clipped to [0, res-1] (get_value_bounded); gradient = derivative of the coefficients.
struct Taps {
  int n;
  int ix[4];
  double w[4], dw[4];
};

template <int MODE>
__device__ __forceinline__ Taps make_taps(double u, int res) {
  Taps T;
  const double hi = (double)(res - 1);
  if (MODE == 1) {
    const double uc = fmin(fmax(u, 0.0), hi);
    T.n = 1;
    T.ix[0] = (int)rint(uc);
    T.w[0] = 1.0;
    T.dw[0] = 0.0;
  } else {
    const double fl = floor(fmin(fmax(u, -4.0), hi + 4.0));       // far outside every tap clips to the border anyway
    const double t = fmin(fmax(u, -4.0), hi + 4.0) - fl;
    const int x0 = (int)fl;
    const double A = -0.75;
    const double x1 = t + 1.0, s = 1.0 - t, x3 = 2.0 - t;
    T.n = 4;
    T.w[0] = ((A * x1 - 5.0 * A) * x1 + 8.0 * A) * x1 - 4.0 * A;
    T.w[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    T.w[2] = ((A + 2.0) * s - (A + 3.0)) * s * s + 1.0;
    T.w[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
    const bool inside = u > -4.0 && u < hi + 4.0;                  // beyond that the value is constant in u
    T.dw[0] = inside ? (3.0 * A * x1 - 10.0 * A) * x1 + 8.0 * A : 0.0;
    T.dw[1] = inside ? (3.0 * (A + 2.0) * t - 2.0 * (A + 3.0)) * t : 0.0;
    T.dw[2] = inside ? -((3.0 * (A + 2.0) * s - 2.0 * (A + 3.0)) * s) : 0.0;
    T.dw[3] = inside ? -((3.0 * A * x3 - 10.0 * A) * x3 + 8.0 * A) : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 - 1 + i;
      T.ix[i] = x < 0 ? 0 : (x > res - 1 ? res - 1 : x);
    }
  }
  return T;
}

// ---- the per-point bodies, shared by the single-item kernels and the batched one (one copy of the arithmetic).
// acc: sum nominator, sum denominator, d/dt (3) and d/dR (9) of (nom - den), over the points this thread visits.
template <int MODE>
__device__ __forceinline__ void point_taps(const float* __restrict__ X, const float* __restrict__ keys, int i, int e,
                                           const float* __restrict__ qimg, const float* __restrict__ denom, int res,
                                           const P34& P, double* acc) {
  const double x = X[3 * (size_t)i], y = X[3 * (size_t)i + 1], z = X[3 * (size_t)i + 2];
  const double px = P.p[0] * x + P.p[1] * y + P.p[2] * z + P.p[3];
  const double py = P.p[4] * x + P.p[5] * y + P.p[6] * z + P.p[7];
  const double pz = P.p[8] * x + P.p[9] * y + P.p[10] * z + P.p[11];
  const double ipz = 1.0 / pz;
  const double u = px * ipz, v = py * ipz;
  const Taps tx = make_taps<MODE>(u, res), ty = make_taps<MODE>(v, res);
  double nom = 0.0, dnx = 0.0, dny = 0.0, den = 0.0, ddx = 0.0, ddy = 0.0;
  for (int b = 0; b < ty.n; ++b)
    for (int a = 0; a < tx.n; ++a) {
      const size_t o = (size_t)ty.ix[b] * res + tx.ix[a];
      double dot = 0.0;
      for (int c = 0; c < e; ++c) dot += (double)keys[(size_t)i * e + c] * (double)qimg[o * e + c];
      const double d = denom[o];
      const double w = ty.w[b] * tx.w[a], wu = ty.w[b] * tx.dw[a], wv = ty.dw[b] * tx.w[a];
      nom += w * dot; dnx += wu * dot; dny += wv * dot;
      den += w * d;   ddx += wu * d;   ddy += wv * d;
    }
  const double fx = dnx - ddx, fy = dny - ddy;
  acc[0] += nom;
  acc[1] += den;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double g = (fx * (P.k[j] - u * P.k[6 + j]) + fy * (P.k[3 + j] - v * P.k[6 + j])) * ipz;
    acc[2 + j] += g;
    acc[5 + 3 * j] += g * x;
    acc[5 + 3 * j + 1] += g * y;
    acc[5 + 3 * j + 2] += g * z;
  }
}

__device__ __forceinline__ void point_bilinear(const float* __restrict__ X, const float* __restrict__ keys, int i, int e,
                                               const float* __restrict__ qimg, const float* __restrict__ denom, int res,
                                               const P34& P, double* acc) {
  const double x = X[3 * (size_t)i], y = X[3 * (size_t)i + 1], z = X[3 * (size_t)i + 2];
  const double px = P.p[0] * x + P.p[1] * y + P.p[2] * z + P.p[3];
  const double py = P.p[4] * x + P.p[5] * y + P.p[6] * z + P.p[7];
  const double pz = P.p[8] * x + P.p[9] * y + P.p[10] * z + P.p[11];
  const double ipz = 1.0 / pz;
  const double u = px * ipz, v = py * ipz;
  // border padding: clamp, zero gradient outside
  const double hi = (double)(res - 1);
  const double uc = fmin(fmax(u, 0.0), hi), vc = fmin(fmax(v, 0.0), hi);
  const double gu = (u > 0.0 && u < hi) ? 1.0 : 0.0, gv = (v > 0.0 && v < hi) ? 1.0 : 0.0;
  int x0 = (int)floor(uc), y0 = (int)floor(vc);
  x0 = x0 > res - 2 ? res - 2 : x0;
  y0 = y0 > res - 2 ? res - 2 : y0;
  if (res < 2) { x0 = 0; y0 = 0; }
  const int x1 = res < 2 ? 0 : x0 + 1, y1 = res < 2 ? 0 : y0 + 1;
  const double wx = uc - x0, wy = vc - y0;
  const size_t o00 = (size_t)y0 * res + x0, o10 = (size_t)y0 * res + x1, o01 = (size_t)y1 * res + x0,
               o11 = (size_t)y1 * res + x1;
  double nom = 0.0, dnx = 0.0, dny = 0.0;
  for (int c = 0; c < e; ++c) {
    const double k = keys[(size_t)i * e + c];
    const double v00 = qimg[o00 * e + c], v10 = qimg[o10 * e + c], v01 = qimg[o01 * e + c], v11 = qimg[o11 * e + c];
    nom += k * ((1 - wy) * ((1 - wx) * v00 + wx * v10) + wy * ((1 - wx) * v01 + wx * v11));
    dnx += k * ((1 - wy) * (v10 - v00) + wy * (v11 - v01));
    dny += k * ((1 - wx) * (v01 - v00) + wx * (v11 - v10));
  }
  const double d00 = denom[o00], d10 = denom[o10], d01 = denom[o01], d11 = denom[o11];
  const double den = (1 - wy) * ((1 - wx) * d00 + wx * d10) + wy * ((1 - wx) * d01 + wx * d11);
  const double ddx = (1 - wy) * (d10 - d00) + wy * (d11 - d01);
  const double ddy = (1 - wx) * (d01 - d00) + wx * (d11 - d10);
  const double fx = (dnx - ddx) * gu, fy = (dny - ddy) * gv;  // d(nom - den)/d(u, v)
  acc[0] += nom;
  acc[1] += den;
  // d(u,v)/dt = (K_row0 - u K_row2, K_row1 - v K_row2) / pz
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double g = (fx * (P.k[j] - u * P.k[6 + j]) + fy * (P.k[3 + j] - v * P.k[6 + j])) * ipz;   // d/d(camera point)_j
    acc[2 + j] += g;
    acc[5 + 3 * j] += g * x;
    acc[5 + 3 * j + 1] += g * y;
    acc[5 + 3 * j + 2] += g * z;
  }
}

// One block's share of one item: the points blockIdx.x * kThreads + threadIdx.x + k * kBlocks * kThreads, a shuffle tree per
// wave, the four waves summed in a fixed order -> partial[0 .. kAcc).  MODE 0 bilinear, 1 nearest, 2 bicubic.
template <int MODE>
__device__ __forceinline__ void block_objective(const float* __restrict__ X, const float* __restrict__ keys, int N, int e,
                                                const float* __restrict__ qimg, const float* __restrict__ denom, int res,
                                                const P34& P, double* __restrict__ partial) {
  __shared__ double red[kThreads / 64][kAcc];
  double acc[kAcc];
#pragma unroll
  for (int q = 0; q < kAcc; ++q) acc[q] = 0.0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < N; i += kBlocks * kThreads) {
    if constexpr (MODE == 0)
      point_bilinear(X, keys, i, e, qimg, denom, res, P, acc);
    else
      point_taps<MODE>(X, keys, i, e, qimg, denom, res, P, acc);
  }
#pragma unroll
  for (int q = 0; q < kAcc; ++q) {
    double s = acc[q];   // wave_sum_down's tree, written out: through the shared function these kernels take two more registers
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < kAcc)
    partial[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// The kBlocks partials of one item, summed in block order -> out[0 .. nout).
// nout = 4: {score, d/dt}; 13: {score, d/dt (3), d/dR (9)}
__device__ __forceinline__ void reduce_item(const double* __restrict__ partial, int N, double* __restrict__ out, int nout) {
  __shared__ double v[kAcc];
  if (threadIdx.x < kAcc) {
    double s = 0.0;
    for (int b = 0; b < kBlocks; ++b) s += partial[(size_t)b * kAcc + threadIdx.x];
    v[threadIdx.x] = s;
  }
  __syncthreads();
  const double n = (double)N;
  if (threadIdx.x == 0) out[0] = -(v[0] / n - v[1] / n) / 2.0;
  if (threadIdx.x >= 1 && threadIdx.x < nout) out[threadIdx.x] = -(v[1 + threadIdx.x] / n) / 2.0;
}

// One item of a batched evaluation: image img at pose Rt (12 f64 [R|t]) -> this block's partial (kAcc f64).
// An image index out of range gives NaN partials (no read beyond the arrays), hence a NaN row.
template <int MODE>
__device__ __forceinline__ void batch_item(const float* __restrict__ X_all, const float* __restrict__ keys_all,
                                           const int32_t* __restrict__ offs, int n_img, int e,
                                           const float* __restrict__ qimgs, const float* __restrict__ denoms, int res,
                                           const double* __restrict__ Ks, int img, const double* __restrict__ Rt,
                                           double* __restrict__ part) {
  if (img < 0 || img >= n_img) {                       // uniform per block: no barrier is skipped by part of it
    if (threadIdx.x < kAcc) part[threadIdx.x] = __builtin_nan("");
    return;
  }
  const size_t o0 = (size_t)offs[img];
  const int N = offs[img + 1] - offs[img];
  const double* Kc = Ks + 9 * (size_t)img;
  P34 P;                                               // refine_impl's host expression, operand for operand
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      P.p[4 * r + c] = Kc[3 * r] * Rt[c] + Kc[3 * r + 1] * Rt[4 + c] + Kc[3 * r + 2] * Rt[8 + c];
#pragma unroll
  for (int i = 0; i < 9; ++i) P.k[i] = Kc[i];
  const size_t plane = (size_t)res * res;
  block_objective<MODE>(X_all + 3 * o0, keys_all + o0 * e, N, e, qimgs + (size_t)img * plane * e, denoms + (size_t)img * plane,
                        res, P, part);
}

}  // namespace
