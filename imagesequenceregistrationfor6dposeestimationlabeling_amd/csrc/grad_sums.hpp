// grad_sums.hpp — the order in which a trainable field's backward sums over its points, stated once for host and device: the
// key field (field_grad.hpp) and the radiance field (radiance_grad.hpp) both take it from here, and csrc/grad_core.hpp holds
// the kernels that execute it.  A plain C++ compiler can include this header.
//
// Every weight gradient is  dW[j, k] = sum_n g[n, j] * h[n, k]  over the points n in memory order (g: the output-side factor
// of the point, h: the input-side one, a row per point or a row per ray of P points), and every bias gradient the same sum
// with h = 1.  THE ORDER: the points are cut into consecutive blocks of kGradChain; inside a block the sum is the f32 chain
// acc = fmaf(g, h, acc) for n ascending from +0; the block sums are added in block order in f64 and rounded to f32 once.
// A BIAS follows one of two policies, the field's choice:
//     the f32 chain of ones (the key field):  inside a block acc = fmaf(g, 1, acc), as for a weight;
//     the f64 sum (the radiance field):       inside a block acc = acc + (double)g from +0 in point order, f64 throughout.
// (An f32 chain of ones has no products that average out: against the reference's executed code the radiance field's density
// bias came to 14 x the reference's own f32 error with f32 chains of 64 and 11 x with chains of 8, and to 2 x with f64 sums;
// the weights hold 4 x at 64.)  So a gradient is a function of the inputs and the point count alone: no float atomics, nothing
// depends on a grid, a slab, a batch or a stream.  v_mfma_f32_32x32x2_f32 is the k-ordered fmaf chain (field_tile.hpp), so a
// block sum of dW is a matrix-core product whose k index is the point.
#pragma once
#include <cmath>
#include <cstddef>

#include "hd.hpp"

namespace isr {
namespace grad {

// Points per f32 chain of a weight sum: the tile.  Against torch autograd in f64 at 4 096 points the worst dW_l / db_l of the
// key field's tests lies at 2.5 x torch-f32's own deviation with chains of 64, 3.2 x with 128 and 4.9 x with 256 (a db of
// seven entries, which torch sums pairwise): 64 keeps the project's 4 x margin with room.
constexpr int kGradChain = 64;
// Points whose activations the workspace holds at a time, at most: 256 tiles, a workgroup for every CU (measured on the key
// field: two slabs of 16 384 take 0.69 ms where one of 32 768, two workgroups a CU, takes 0.74 ms and four of 8 192 take
// 1.02 ms).  Their block sums are formed and added kGradBatch points at a time, a number each field sets for itself.
constexpr int kGradSlab = 16384;

// One entry: sum_n g[n gs] * h[n hs] over N points in the order above (h == nullptr: the f32 chain of ones).
ISR_HD float blocked_sum(const float* g, long gs, const float* h, long hs, long N) {
  double total = 0.0;
  for (long n0 = 0; n0 < N; n0 += kGradChain) {
    const long n1 = n0 + kGradChain < N ? n0 + kGradChain : N;
    float acc = 0.f;
    for (long n = n0; n < n1; ++n) acc = fmaf(g[n * gs], h ? h[n * hs] : 1.f, acc);
    total += (double)acc;
  }
  return (float)total;
}

// Host: out[k] = the sum over n < N of g[n gs] * Hm[(n / div) K + k] in the order above for every k < K (K <= kMaxK), the
// points walked once.  div = 1: a row of Hm per point; div = P: a row per ray.  Hm == nullptr: K = 1, a bias, by the f64 sum
// where bias64 and by the f32 chain of ones where not.
template <int kMaxK>
inline void blocked_row(const float* g, long gs, const float* Hm, int K, long div, long N, bool bias64, float* out) {
  double total[kMaxK];
  float acc[kMaxK];
  for (int k = 0; k < K; ++k) total[k] = 0.0;
  for (long n0 = 0; n0 < N; n0 += kGradChain) {
    const long n1 = n0 + kGradChain < N ? n0 + kGradChain : N;
    if (!Hm && bias64) {
      double acc64 = 0.0;
      for (long n = n0; n < n1; ++n) acc64 += (double)g[n * gs];
      total[0] += acc64;
      continue;
    }
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (long n = n0; n < n1; ++n) {
      const float gv = g[n * gs];
      if (!Hm) {
        acc[0] = fmaf(gv, 1.f, acc[0]);
        continue;
      }
      const float* h = Hm + (size_t)(n / div) * K;
      for (int k = 0; k < K; ++k) acc[k] = fmaf(gv, h[k], acc[k]);
    }
    for (int k = 0; k < K; ++k) total[k] += (double)acc[k];
  }
  for (int k = 0; k < K; ++k) out[k] = (float)total[k];
}

}  // namespace grad
}  // namespace isr
