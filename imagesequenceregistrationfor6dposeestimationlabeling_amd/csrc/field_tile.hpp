// field_tile.hpp — the matrix-core layer of a fused field kernel, once, for csrc/field_mlp.hip, csrc/field_density.hip and
// csrc/field_radiance.hip (device only).
//
// A workgroup takes a tile of kTP = 64 points through every layer of its field; the tile's activations live in LDS from the
// first layer to the last.  A layer runs on v_mfma_f32_32x32x2_f32, which is bit for bit the k-ordered fmaf chain: A = the
// weights (M = 32 neurons), B = the activations (N = 32 points), the accumulator loaded with the bias, the k loop in order.
// The weights are not staged in LDS (a 256 x 256 layer is 256 KB): the pack holds them in the order the lanes load them
// (field_mlp.hpp's w_index), so a wave streams its own neurons' rows straight into registers, 8 k's (one 16-byte load per
// lane, 1 KB per wave) ahead of the four MFMAs that use them; the waves read disjoint parts of the layer.
// Widths are padded with zero weights (fmaf(0, x, z) = z for finite x) and padded activations are written as 0, so the
// padding changes no bit.
// Activations in LDS: k-pair major, act[act_index(k, p)] — the B operand of k-step s (lane (r, h) wants k = 2 s + h of
// point r) is 64 consecutive words, and a lane's accumulator registers (neurons 8 a + 4 h + b) leave as two 8-byte stores.
#pragma once
#include <hip/hip_runtime.h>

#include "field_mlp.hpp"

namespace isr {
namespace field {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTP = 64;            // points per tile

__device__ __forceinline__ int act_index(int k, int p) { return ((k >> 1) * kTP + p) * 2 + (k & 1); }

// One wave's share of a layer: neuron blocks mb[0 .. nmb) (32 neurons each) x nnb blocks of 32 points from point block nb0.
template <int kMaxMb>
struct WaveShare {
  int mb[kMaxMb];
  int nmb, nb0, nnb;
};

// Wave w of kWaves and a layer of MB neuron blocks.  More blocks than half the waves: blocks w, w + kWaves, ... below MB,
// over both point blocks.  Otherwise a wave takes one 32 x 32 tile: block w >> 1, point block w & 1.
template <int kWaves>
__device__ __forceinline__ WaveShare<kMaxWidth / 32 / kWaves> wave_share(int MB, int w) {
  constexpr int kMaxMb = kMaxWidth / 32 / kWaves;
  WaveShare<kMaxMb> s;
  if (MB > kWaves / 2) {
    s.nmb = 0;
#pragma unroll
    for (int m = 0; m < kMaxMb; ++m) {
      s.mb[m] = w + m * kWaves;
      s.nmb += s.mb[m] < MB;
    }
    s.nb0 = 0;
    s.nnb = 2;
  } else {
#pragma unroll
    for (int m = 0; m < kMaxMb; ++m) s.mb[m] = 0;
    s.mb[0] = w >> 1;
    s.nmb = (w >> 1) < MB;
    s.nb0 = w & 1;
    s.nnb = 1;
  }
  return s;
}

// What a chain starts from: init(j, p) is the accumulator of neuron j (below the layer's OP) and point p of the tile before
// the first k.  BiasInit is the layer's own bias, the same for every point.
struct BiasInit {
  const float* bl;
  __device__ __forceinline__ float operator()(int j, int) const { return bl[j]; }
};

// NMB blocks of 32 neurons x NNB blocks of 32 points: the accumulators of the whole k loop.
template <int NMB, int NNB, int kMaxMb, class Init>
__device__ __forceinline__ void mfma_layer(const Layer& L, const float* __restrict__ Wl, Init init, const float* act,
                                           const int (&mb)[kMaxMb], int nb0, int lane, f32x16 (&acc)[kMaxMb][2]) {
  const int r = lane & 31, hh = lane >> 5;
  const int S4 = L.kstride >> 3;
#pragma unroll
  for (int m = 0; m < NMB; ++m)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int n = 0; n < NNB; ++n) acc[m][n][4 * a + b] = init(mb[m] * 32 + 8 * a + 4 * hh + b, (nb0 + n) * 32 + r);
      }
  const float4* wp[NMB];
  float4 cur[NMB];
#pragma unroll
  for (int m = 0; m < NMB; ++m) {
    wp[m] = reinterpret_cast<const float4*>(Wl) + (size_t)mb[m] * S4 * 64 + lane;
    cur[m] = wp[m][0];
  }
  const float* bp = act + (nb0 * 32 + r) * 2 + hh;
  for (int s4 = 0; s4 < S4; ++s4) {
    float4 nxt[NMB];
    const int sn = s4 + 1 < S4 ? s4 + 1 : s4;
#pragma unroll
    for (int m = 0; m < NMB; ++m) nxt[m] = wp[m][(size_t)sn * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float bv[NNB];
#pragma unroll
      for (int n = 0; n < NNB; ++n) bv[n] = bp[((4 * s4 + i) * kTP + n * 32) * 2];
#pragma unroll
      for (int m = 0; m < NMB; ++m) {
        const float av = i == 0 ? cur[m].x : i == 1 ? cur[m].y : i == 2 ? cur[m].z : cur[m].w;
#pragma unroll
        for (int n = 0; n < NNB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[n], acc[m][n], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < NMB; ++m) cur[m] = nxt[m];
  }
}

// The accumulators through `activation` into act: k-pair major for the next layer, padded neurons as 0; or, for a field's
// last layer, the tile row-major (64, O) with the padded neurons left out.
template <int kMaxMb, class Act>
__device__ __forceinline__ void store_activations(const Layer& L, const f32x16 (&acc)[kMaxMb][2], const WaveShare<kMaxMb>& s,
                                                  float* act, int lane, bool row_major, Act activation) {
  const int r = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int m = 0; m < kMaxMb; ++m) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (m < s.nmb && n < s.nnb) {
        const int p = (s.nb0 + n) * 32 + r;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int j = s.mb[m] * 32 + 8 * a + 4 * hh;
          float v[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) v[b] = j + b < L.O ? activation(acc[m][n][4 * a + b]) : 0.f;
          if (!row_major) {
            *reinterpret_cast<float2*>(&act[act_index(j, p)]) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2*>(&act[act_index(j + 2, p)]) = make_float2(v[2], v[3]);
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (j + b < L.O) act[p * L.O + j + b] = v[b];
          }
        }
      }
    }
  }
}

// One matrix-core layer of the tile, in place: act holds the layer's input on entry (k-pair major, K padded to kstride with
// zeros) and its output after the call.  Every thread of a workgroup of kWaves waves calls it.  The chains start from
// init(neuron, point) (mfma_tile_layer below: from the layer's bias).
template <int kWaves, class Act, class Init>
__device__ __forceinline__ void mfma_tile_layer_from(const Layer& L, const float* __restrict__ pack, float* act, bool row_major,
                                                     Act activation, Init init) {
  constexpr int kMaxMb = kMaxWidth / 32 / kWaves;
  static_assert(kMaxMb == 1 || kMaxMb == 2, "mfma_tile_layer dispatches one or two neuron blocks per wave");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* Wl = pack + L.w_off;
  const WaveShare<kMaxMb> s = wave_share<kWaves>(L.OP >> 5, w);
  f32x16 acc[kMaxMb][2];
  if constexpr (kMaxMb == 2) {
    if (s.nmb == 2) mfma_layer<2, 2>(L, Wl, init, act, s.mb, s.nb0, lane, acc);
  }
  if (s.nmb == 1 && s.nnb == 2) mfma_layer<1, 2>(L, Wl, init, act, s.mb, s.nb0, lane, acc);
  else if (s.nmb == 1) mfma_layer<1, 1>(L, Wl, init, act, s.mb, s.nb0, lane, acc);
  __syncthreads();                // every wave has read the layer's input: the outputs may take its place
  store_activations(L, acc, s, act, lane, row_major, activation);
  __syncthreads();
}

template <int kWaves, class Act>
__device__ __forceinline__ void mfma_tile_layer(const Layer& L, const float* __restrict__ pack, float* act, bool row_major,
                                                Act activation) {
  mfma_tile_layer_from<kWaves>(L, pack, act, row_major, activation, BiasInit{pack + L.b_off});
}

}  // namespace field
}  // namespace isr
