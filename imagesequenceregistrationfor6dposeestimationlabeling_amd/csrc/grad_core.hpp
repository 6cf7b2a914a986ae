// grad_core.hpp — what the backwards of the two trainable fields run on the device after their tile kernels: the sums of
// grad_sums.hpp over a slab's points, and the device-side packing they share.  Included by field_grad.hip and
// radiance_grad.hip only.
//
// A field's points are worked through in memory order in slabs of whole chains (kGradChain points).  Per slab the field's own
// first kernels leave, for every point, the two factors of every gradient matrix in the workspace (rows past the end carry
// g = 0); then per batch of the slab's points (for_slabs):
//   * grad_dw_kernel, one wave per (32 x 32 block of a gradient matrix, chain): v_mfma_f32_32x32x2_f32 with the point as its
//     k index, A = the output-side factor and B = the input-side factor straight from the workspace (both are 128-byte rows
//     per half wave), the accumulator from +0: the chain of the rule.  A per-ray input reads the row of the point's ray.
//     Parts narrower than 32 on the input side and every bias are the same chain on the vector unit, a lane per entry (a
//     bias by the field's policy, kBias64).  A block sum goes to the workspace, real entries only, in the standard layout:
//     f32 throughout for the f32 policy, the weights' as f32 and the biases' as f64 for the f64 policy;
//   * grad_combine_kernel, a lane per entry: the batch's block sums onto an f64 accumulator that lives in the workspace from
//     batch to batch and slab to slab, in block order; the last one rounds to f32 and writes dW and db.
#pragma once
#include "field_tile.hpp"
#include "grad_sums.hpp"
#include "isr_common.hpp"

namespace isr {
namespace grad {

using field::Layer;

constexpr int kFlat = 256;      // the per-entry kernels' workgroup

struct ZeroInit {
  __device__ __forceinline__ float operator()(int, int) const { return 0.f; }
};

// Every (point, neuron) pair of the tile below OP over a workgroup of kThreads, a wave step 8 points x 8 neurons (32-byte pieces
// of the workspace's rows, four LDS words per bank of the k-pair-major tile): v = load(point, neuron) for a batch of steps at
// once, so that their memory latencies overlap, then f(point, neuron, v) for each.  OP is a multiple of 32, a batch of every wave.
template <int kThreads, class Ld, class F>
__device__ __forceinline__ void for_tile(int OP, Ld load, F f) {
  constexpr int kWaves = kThreads / 64, kBatch = 32 / kWaves;
  static_assert(kBatch * kWaves == 32, "a batch of every wave covers 32 steps, which divides every OP");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, pl = lane >> 3, jl = lane & 7;
  for (int item0 = w; item0 < OP; item0 += kBatch * kWaves) {
    float v[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int item = item0 + i * kWaves;
      v[i] = load((item & 7) * 8 + pl, (item >> 3) * 8 + jl);
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int item = item0 + i * kWaves;
      f((item & 7) * 8 + pl, (item >> 3) * 8 + jl, v[i]);
    }
  }
}

// One gradient matrix (or part of one) of the dW launch: dW[w_off + j * w_ld + k] = sum_n g[n, j] * h[n or ray of n, k].
struct DwLayer {
  const float* g;
  const float* h;
  int ldg, O, ldh, K;
  int per_ray;               // h has a row per ray of the slab
  int mf;                    // the weights run on the matrix cores; the vector items are then the biases alone
  int w_off, w_ld, b_off;    // b_off < 0: no bias goes with this part
};

// The work items of the dW launch: part l owns items [first[l], first[l + 1]), the matrix-core blocks first (nmf[l]).
template <int kMaxParts>
struct DwArgs {
  DwLayer L[kMaxParts];
  int first[kMaxParts + 1];
  int nmf[kMaxParts];
  int n_parts, w_total, b_total;
};

template <int kMaxParts>
void add_part(DwArgs<kMaxParts>& D, const float* g, int ldg, int O, const float* h, int ldh, int K, int per_ray, bool allow_mf,
              int w_off, int w_ld, int b_off) {
  const int l = D.n_parts++;
  DwLayer& L = D.L[l];
  L = DwLayer{g, h, ldg, O, ldh, K, per_ray, (allow_mf && K >= field::kMfmaMinK) ? 1 : 0, w_off, w_ld, b_off};
  D.nmf[l] = L.mf ? ((O + 31) / 32) * ((K + 31) / 32) : 0;
  const int cols = (L.mf ? 0 : K) + (b_off >= 0 ? 1 : 0);
  D.first[l + 1] = D.first[l] + D.nmf[l] + (O * cols + 63) / 64;
}

// (ray of the slab, sample) of a point, stepped forward through the slab
struct RayWalk {
  int rel, kk, P;
  __device__ __forceinline__ RayWalk(long s0, int row, int P_, long ray_base) : P(P_) {
    const long ng = s0 + row, ray = ng / P_;
    rel = (int)(ray - ray_base);
    kk = (int)(ng - ray * P_);
  }
  __device__ __forceinline__ void step(int by) {
    kk += by;
    while (kk >= P) {
      kk -= P;
      ++rel;
    }
  }
};

// The slab's points are [s0, s0 + n) of the field's, P to a ray, ray_base = s0 / P (a field without rays: 0, 1, 0).  The block
// sums of chain chain0 + blockIdx.y: the weights' to part, the biases' behind them (f32 policy) or to part_b (f64 policy).
template <bool kBias64, int kMaxParts>
__global__ __launch_bounds__(64) void grad_dw_kernel(DwArgs<kMaxParts> D, int n, int chain0, long s0, int P, long ray_base,
                                                     float* __restrict__ part, double* __restrict__ part_b) {
  const int lane = threadIdx.x, c = blockIdx.y;                         // chain chain0 + c of the slab, the batch's c-th
  int item = blockIdx.x, l = 0;
  while (item >= D.first[l + 1]) ++l;
  item -= D.first[l];
  const DwLayer L = D.L[l];
  const int p0 = (chain0 + c) * kGradChain;
  const int left = n - p0;
  const int real = left < kGradChain ? left : kGradChain;               // the chain's points; the tile kernel wrote g = 0 past n
  const float* G = L.g + (size_t)p0 * L.ldg;
  float* out = part + (size_t)c * (kBias64 ? D.w_total : D.w_total + D.b_total);
  if (item < D.nmf[l]) {
    const int KB = (L.K + 31) / 32, jb = item / KB, kb = item - jb * KB;
    const int r = lane & 31, hh = lane >> 5;
    const int k = kb * 32 + r;
    const float* ga = G + (size_t)hh * L.ldg + jb * 32 + r;            // ldg is the layer's width rounded up to 32
    field::f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (!L.per_ray) {
      const float* hb = L.h + (size_t)(p0 + hh) * L.ldh + k;            // ldh likewise: k is inside the row
      for (int s = 0; s < kGradChain / 2; s += 8) {                     // eight loads of each operand in flight
        float av[8], bv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          av[i] = ga[(size_t)2 * (s + i) * L.ldg];
          bv[i] = hb[(size_t)2 * (s + i) * L.ldh];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
      }
    } else {
      RayWalk rw(s0, p0 + hh, P, ray_base);
      for (int s = 0; s < kGradChain / 2; s += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          av[i] = ga[(size_t)2 * (s + i) * L.ldg];
          bv[i] = 2 * (s + i) + hh < real ? L.h[(size_t)rw.rel * L.ldh + k] : 0.f;      // past the end: no such ray
          rw.step(2);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = jb * 32 + 8 * a + 4 * hh + b;
        if (j < L.O && k < L.K) out[L.w_off + j * L.w_ld + k] = acc[4 * a + b];
      }
    return;
  }
  // the vector unit: a lane per entry.  A matrix-core part leaves its bias here; a narrow one its K columns as well.
  const int e = (item - D.nmf[l]) * 64 + lane;
  const int kw = L.mf ? 0 : L.K, cols = kw + (L.b_off >= 0 ? 1 : 0);
  if (e >= L.O * cols) return;
  const int j = e / cols, k = e - j * cols;
  if (kBias64 && k >= kw) {
    double acc64 = 0.0;
    for (int nn = 0; nn < real; ++nn) acc64 += (double)G[(size_t)nn * L.ldg + j];
    part_b[(size_t)c * D.b_total + L.b_off + j] = acc64;
    return;
  }
  // the f32 policy: a bias is the weights' chain over h = 1, in the same loop (a narrow part's waves hold both kinds of lane)
  const bool wt = kBias64 || k < kw;
  float acc = 0.f;
  if (!L.per_ray) {
    const float* hp = L.h + (size_t)p0 * L.ldh + k;
    for (int nn = 0; nn < real; ++nn) acc = fmaf(G[(size_t)nn * L.ldg + j], wt ? hp[(size_t)nn * L.ldh] : 1.f, acc);
  } else {
    RayWalk rw(s0, p0, P, ray_base);
    for (int nn = 0; nn < real; ++nn) {
      acc = fmaf(G[(size_t)nn * L.ldg + j], wt ? L.h[(size_t)rw.rel * L.ldh + k] : 1.f, acc);
      rw.step(1);
    }
  }
  out[wt ? L.w_off + j * L.w_ld + k : D.w_total + L.b_off + j] = acc;
}

template <bool kBias64>
__global__ __launch_bounds__(kFlat) void grad_combine_kernel(const float* __restrict__ part, const double* __restrict__ part_b,
                                                             int nblk, int w_total, int b_total, double* __restrict__ acc64,
                                                             int first, int last, float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * kFlat + threadIdx.x;
  const int E = w_total + b_total;
  if (e >= E) return;
  double acc = first ? 0.0 : acc64[e];
  if (!kBias64)
    for (int c = 0; c < nblk; ++c) acc += (double)part[(size_t)c * E + e];
  else if (e < w_total)
    for (int c = 0; c < nblk; ++c) acc += (double)part[(size_t)c * w_total + e];
  else
    for (int c = 0; c < nblk; ++c) acc += part_b[(size_t)c * b_total + e - w_total];
  acc64[e] = acc;
  if (!last) return;
  if (e < w_total) {
    if (dW) dW[e] = (float)acc;
  } else if (db) {
    db[e - w_total] = (float)acc;
  }
}

// The points of a slab at most: N rounded up to whole chains, one chain at least.
inline int slab_for(long points) {
  const long up = (points + kGradChain - 1) / kGradChain * kGradChain;
  return up < kGradChain ? kGradChain : up > kGradSlab ? kGradSlab : (int)up;
}

// N = 0: every gradient is zero.
inline int zero_grads(float* dW, int w_total, float* db, int b_total, hipStream_t st) {
  if (dW) ISR_CHECK_HIP(hipMemsetAsync(dW, 0, (size_t)w_total * 4, st));
  if (db) ISR_CHECK_HIP(hipMemsetAsync(db, 0, (size_t)b_total * 4, st));
  return ISR_OK;
}

// The NP points in slabs of `slab`: first_kernels(s0, n, ray_base) launches the field's own kernels for the slab [s0, s0 + n)
// (and may re-point D, which every launch takes by value), then the two kernels above per batch of kBatch points.
template <bool kBias64, int kBatch, int kMaxParts, class First>
int for_slabs(DwArgs<kMaxParts>& D, long NP, int slab, int P, float* part, double* part_b, double* acc64, float* dW, float* db,
              hipStream_t st, First first_kernels) {
  static_assert(kBatch % kGradChain == 0 && kGradSlab % kBatch == 0, "chains make batches, batches make slabs");
  const int E = D.w_total + D.b_total;
  for (long s0 = 0; s0 < NP; s0 += slab) {
    const int n = NP - s0 < slab ? (int)(NP - s0) : slab;
    const long ray_base = s0 / P;
    if (int rc = first_kernels(s0, n, ray_base)) return rc;
    for (int b0 = 0; b0 < n; b0 += kBatch) {
      const int nb = n - b0 < kBatch ? n - b0 : kBatch;
      const int nblk = (nb + kGradChain - 1) / kGradChain;
      grad_dw_kernel<kBias64, kMaxParts><<<dim3(D.first[D.n_parts], nblk), 64, 0, st>>>(D, n, b0 / kGradChain, s0, P, ray_base, part,
                                                                                       part_b);
      ISR_CHECK_LAUNCH("grad_dw_kernel");
      grad_combine_kernel<kBias64><<<(E + kFlat - 1) / kFlat, kFlat, 0, st>>>(part, part_b, nblk, D.w_total, D.b_total, acc64,
                                                                              s0 + b0 == 0, s0 + b0 + nb == NP, dW, db);
      ISR_CHECK_LAUNCH("grad_combine_kernel");
    }
  }
  return ISR_OK;
}

// ---- packing a trainable field on the device: a thread per word of the two packs

// the inverse of w_index: word idx of a layer's weight block -> (j, k), padding included
__device__ __forceinline__ void w_unindex(const Layer& L, int idx, int& j, int& k) {
  if (!L.mfma) {
    j = idx / L.kstride;
    k = idx - j * L.kstride;
    return;
  }
  const int q = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8, S8 = L.kstride >> 3;
  k = (blk % S8) * 8 + 2 * q + (lane >> 5);
  j = (blk / S8) * 32 + (lane & 31);
}

// word i of a forward layer whose weights are W[w0 + j * ld + col0 + k] and whose bias is b[b0 + j] (b0 < 0: zeros)
__device__ __forceinline__ bool pack_layer_word(const Layer& L, int i, const uint32_t* W, int w0, int ld, int col0,
                                                const uint32_t* b, int b0, uint32_t& bits) {
  if (i < L.w_off || i >= L.b_off + L.OP) return false;
  if (i < L.b_off) {
    int j, k;
    w_unindex(L, i - L.w_off, j, k);
    if (j < L.O && k < L.K) bits = W[w0 + j * ld + col0 + k];
  } else if (i - L.b_off < L.O && b0 >= 0) {
    bits = b[b0 + i - L.b_off];
  }
  return true;
}

// word t of a transposed layer over W[w0 + j * ld + k]: T's neuron is W's input k, T's input W's neuron j
__device__ __forceinline__ bool pack_t_word(const Layer& T, int t, const uint32_t* W, int w0, int ld, int O, uint32_t& bits) {
  if (t < T.w_off || t >= T.b_off + T.OP) return false;
  if (t < T.b_off) {
    int k, j;
    w_unindex(T, t - T.w_off, k, j);
    if (k < T.O && j < O) bits = W[w0 + j * ld + k];
  }
  return true;
}

// the transposed layout of `lay` (the field's make_layout_t) and the check of the caller's transposed pack against it
template <class Lay, class LayT>
int check_pack_t(const char* who, const Lay& lay, const void* packT, size_t packT_bytes, LayT& layT) {
  make_layout_t(lay, layT);
  ISR_REQUIRE(packT, "%s: null pointer", who);
  ISR_REQUIRE(packT_bytes == (size_t)layT.total_words * 4, "%s: packT_bytes %zu, this field's transposed pack has %zu", who,
              packT_bytes, (size_t)layT.total_words * 4);
  return ISR_OK;
}

}  // namespace grad
}  // namespace isr
