// block_prims.hpp — the wave and workgroup primitives the kernels share (device only; wave64).
//
// FLOAT ORDER.  A floating-point sum is part of an entry's stated result, so a site may call a function of this header only
// if the order of operations stays what that site's rule states, for every lane whose value is read.  wave_sum_down is the
// tree v[l] += v[l + s], s = 32 .. 1, whose lane 0 the rules name; wave_reduce's butterfly is for order-free operators
// (integer sums, min, max, or a caller's own rule such as a maximum that keeps NaN).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace isr {

// operators for wave_reduce: the integer min / max, fminf / fmaxf for floats (a NaN loses), and the sum
struct Min {
  __device__ int operator()(int a, int b) const { return min(a, b); }
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct Max {
  __device__ int operator()(int a, int b) const { return max(a, b); }
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct Plus {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};

// op over the wave's 64 values by xor butterfly; the result in every lane
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}

// the tree v[l] += v[l + s] for s = 32, 16, .. 1: lane 0 holds the wave's sum, the other lanes partial ones
template <typename T>
__device__ __forceinline__ T wave_sum_down(T v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  return v;
}

// inclusive scan of x over the wave's lanes
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// Exclusive scan of x over a workgroup of THREADS threads in thread order; the workgroup's sum to total in every thread.
// sw: THREADS / 64 entries of LDS.  One barrier inside and none after: a caller that scans again with the same sw puts a
// barrier between the two calls.
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive_scan(T x, T* sw, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_inclusive_scan(x);
  if (lane == 63) sw[wave] = inc;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const T sv = sw[w];
    if (w < wave) base += sv;
    total += sv;
  }
  return base + inc - x;
}

// The scan of per-workgroup counts between a count and a scatter launch: counts (nblocks per image, the image on blockIdx.z)
// become exclusive offsets in place, and the image's sum goes to total[image].  One workgroup of kOffsetsThreads per image;
// thread t owns the (nblocks + 1023) / 1024 consecutive counts from t * per.  A template, so that only the source files that
// launch it compile it.
constexpr int kOffsetsThreads = 1024;

template <typename T>
__global__ __launch_bounds__(kOffsetsThreads) void block_offsets_kernel(T* __restrict__ counts, int nblocks, T* __restrict__ total) {
  __shared__ T tsum[kOffsetsThreads];
  counts += (size_t)blockIdx.z * nblocks;
  const int t = threadIdx.x;
  const int per = (nblocks + kOffsetsThreads - 1) / kOffsetsThreads;
  T s = 0;
  for (int j = 0; j < per; ++j) {
    const int b = t * per + j;
    if (b < nblocks) s += counts[b];
  }
  tsum[t] = s;
  __syncthreads();
  for (int off = 1; off < kOffsetsThreads; off <<= 1) {   // Hillis-Steele inclusive scan of the threads' sums
    const T v = (t >= off) ? tsum[t - off] : 0;
    __syncthreads();
    tsum[t] += v;
    __syncthreads();
  }
  T run = (t > 0) ? tsum[t - 1] : 0;
  for (int j = 0; j < per; ++j) {
    const int b = t * per + j;
    if (b < nblocks) {
      const T c = counts[b];
      counts[b] = run;
      run += c;
    }
  }
  if (t == kOffsetsThreads - 1) total[blockIdx.z] = tsum[kOffsetsThreads - 1];
}

}  // namespace isr
