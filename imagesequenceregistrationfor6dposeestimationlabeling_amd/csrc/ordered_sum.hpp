// ordered_sum.hpp — the fixed-order f64 sum of the losses (contrastive.hpp, ray_losses.hpp), stated and written once.
//
// REDUCE ORDER.  reduce256 is the sum of up to 256 doubles v[0 .. n-1] (the missing ones are +0) by the tree v[i] += v[i + s]
// for s = 128, 64, .. 1.  The sum of L leaves: reduce256 of every 256 consecutive ones, ascending, then the same of the
// results, until one is left; a level is made even of a single leaf (so -0 alone sums to +0).  Leaves that are f32 are
// converted to f64 as they are read.  The host functions and the kernels below follow this text and nothing else: that is
// what makes a loss of the device equal its host build bit for bit.
//
// A plain C++ compiler sees the host half only (the tools/*_host_check.cpp programs); hipcc sees the kernels too.
#pragma once
#include <cstddef>

#include "hd.hpp"

namespace isr {

constexpr int kReduce = 256;                         // leaves of one reduce256 tree

// ---- host
template <class Leaf>
inline double reduce256(const Leaf* v, int n) {
  double w[kReduce];
  for (int i = 0; i < kReduce; ++i) w[i] = i < n ? (double)v[i] : 0.0;
  for (int s = kReduce / 2; s > 0; s >>= 1)
    for (int i = 0; i < s; ++i) w[i] += w[i + s];
  return w[0];
}

// one level: out[g] = reduce256(in[256 g ..]); out may be in (reads [256 g, 256 g + nn) before it writes [g], and g <= 256 g)
template <class Leaf>
inline long long reduce_level(const Leaf* in, long long L, double* out) {
  const long long L2 = (L + kReduce - 1) / kReduce;
  for (long long g = 0; g < L2; ++g) {
    const int nn = (int)(L - g * kReduce < kReduce ? L - g * kReduce : kReduce);
    out[g] = reduce256(in + g * kReduce, nn);
  }
  return L2;
}

// REDUCE ORDER over leaves[0 .. count); scratch: (count + 255) / 256 doubles at least, and it may be the leaves themselves
template <class Leaf>
inline double ordered_sum(const Leaf* leaves, long long count, double* scratch) {
  long long L = reduce_level(leaves, count, scratch);
  while (L > 1) L = reduce_level(scratch, L, scratch);
  return scratch[0];
}

}  // namespace isr

#if defined(__HIPCC__)
// ---- device
#include "isr_common.hpp"

namespace isr {

// The tree over tree[v][0 .. 256) for v < NV, by a workgroup of kReduce threads whose leaves are stored and fenced by a
// barrier: tree[v][0] is the sum when it returns (a barrier is the last thing it does).
template <int NV>
__device__ __forceinline__ void tree256(double (*tree)[kReduce]) {
  for (int s = kReduce / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int v = 0; v < NV; ++v) tree[v][threadIdx.x] += tree[v][threadIdx.x + s];
    }
    __syncthreads();
  }
}

// One level over NV interleaved sums: out[g * NV + v] = reduce256(in[(256 g ..) * NV + v]).  The level that leaves one value
// also writes result[v] = finish(sum, v): the caller's last step (a mean, a scaled loss).
template <int NV, class In, class Finish>
__global__ __launch_bounds__(kReduce) void reduce_kernel(const In* __restrict__ in, long long L, double* __restrict__ out,
                                                         Finish finish, float* __restrict__ result) {
  __shared__ double tree[NV][kReduce];
  for (long long g = blockIdx.x; g * kReduce < L; g += gridDim.x) {
    const long long i = g * kReduce + threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v) tree[v][threadIdx.x] = i < L ? (double)in[i * NV + v] : 0.0;
    __syncthreads();
    tree256<NV>(tree);
    if ((int)threadIdx.x < NV) {
      out[g * NV + threadIdx.x] = tree[threadIdx.x][0];
      if (L <= kReduce) result[threadIdx.x] = finish(tree[threadIdx.x][0], (int)threadIdx.x);
    }
  }
}

inline long long reduce_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// workgroups of a launch over `items` grid-stride work items
inline unsigned reduce_grid(long long items) { return (unsigned)(items < (1ll << 20) ? items : (1ll << 20)); }

// the two buffers the levels alternate between: `first` values (NV doubles each), then ceil(first / 256); *second: where the
// second one starts
inline size_t reduce_bytes(long long first, int NV, size_t* second) {
  const size_t a = align_up((size_t)first * NV * 8, 256), b = align_up((size_t)reduce_ceil_div(first, kReduce) * NV * 8, 256);
  if (second) *second = a;
  return a + b;
}

// Every level over L leaves (NV values each): the first reads `leaves` and writes bufs[to], the later ones alternate between
// the two buffers; the last one writes result.
template <int NV, class In, class Finish>
int reduce_levels(const char* what, const In* leaves, long long L, double* bufs[2], int to, Finish finish, float* result,
                  hipStream_t st) {
  reduce_kernel<NV, In, Finish><<<reduce_grid(reduce_ceil_div(L, kReduce)), kReduce, 0, st>>>(leaves, L, bufs[to], finish, result);
  ISR_CHECK_LAUNCH(what);
  while (L > kReduce) {
    L = reduce_ceil_div(L, kReduce);
    reduce_kernel<NV, double, Finish><<<reduce_grid(reduce_ceil_div(L, kReduce)), kReduce, 0, st>>>(bufs[to], L, bufs[to ^ 1], finish,
                                                                                                   result);
    ISR_CHECK_LAUNCH(what);
    to ^= 1;
  }
  return ISR_OK;
}

}  // namespace isr
#endif
