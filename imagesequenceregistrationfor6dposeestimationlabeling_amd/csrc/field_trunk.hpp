// field_trunk.hpp — what the kernels of csrc/field_density.hip and csrc/field_radiance.hip share (hipcc only): the workgroup's
// geometry, a tile's 64 points made from its rays, the harmonic embedding into LDS and the density trunk on top of
// field_tile.hpp's matrix-core layer; and the argument checks every march entry shares.
//
// 8 waves per workgroup (512 threads, two per SIMD): wave w takes neuron block w of a 256-wide layer over both point blocks.
// The activation buffer holds 384 k's x 64 points = 96 KB, so one workgroup is resident per CU.
// A WORKGROUP OWNS WHOLE RAYS: G = max(1, 64 / P) consecutive rays, their G * P points taken 64 at a time.
#pragma once
#include "field_density.hpp"
#include "field_tile.hpp"
#include "isr_common.hpp"

namespace isr {
namespace density {

using field::act_index;
using field::kTP;

constexpr int kThreads = 512;
constexpr int kActWords = (6 * kMaxH / 2) * kTP * 2;      // 96 KB

inline int rays_per_group(int P) { return P >= kTP ? 1 : kTP / P; }

// The rays [ray0, ray0 + nr) of this workgroup and their `total` samples in `tiles` tiles
struct RayGroup {
  long ray0;
  int nr, total, tiles;
  __device__ __forceinline__ RayGroup(int N, int P, int G) {
    ray0 = (long)blockIdx.x * G;
    nr = (long)N - ray0 < G ? (int)((long)N - ray0) : G;
    total = nr * P;                                  // <= max(64, P) <= kMaxP
    tiles = (total + kTP - 1) / kTP;
  }
};

// ptl (LDS, coordinate-major: ptl[d * 64 + p]) of tile t: o + d * len of the group's samples [64 t, 64 t + 64), rows past
// the end at the origin.  No barrier behind it.
__device__ __forceinline__ void tile_points_from_rays(const RayGroup& rg, int P, int t, const float* __restrict__ origins,
                                                      const float* __restrict__ directions,
                                                      const float* __restrict__ lengths, float* ptl) {
  const int tid = threadIdx.x;
  if (tid < 3 * kTP) {
    const int d = tid >> 6, q = t * kTP + (tid & 63);
    float v = 0.f;
    if (q < rg.total) {
      const int g = q / P, k = q - g * P;
      const long ray = rg.ray0 + g;
      v = origins[3 * ray + d] + directions[3 * ray + d] * lengths[ray * P + k];
    }
    ptl[tid] = v;
  }
}

// e (6H) of the 64 points of ptl into act: k = d * H + i holds the sine, 3H + k the cosine (sincos32, one call per pair);
// k in [6H, kstride) zeros; a barrier behind it
__device__ __forceinline__ void tile_embed(int H, int kstride, const float* __restrict__ pack, float* act, const float* ptl) {
  const int tid = threadIdx.x;
  const float* freqs = pack + kFreqOff;
  for (int i = tid; i < 3 * H * kTP; i += kThreads) {
    const int p = i & (kTP - 1), kk = i >> 6;
    const int d = kk / H, fi = kk - d * H;
    const float a = ptl[d * kTP + p] * freqs[fi];
    float s, c;
    sincos32(a, &s, &c);
    act[act_index(kk, p)] = s;
    act[act_index(3 * H + kk, p)] = c;
  }
  for (int i = tid; i < (kstride - 6 * H) * kTP; i += kThreads) act[act_index(6 * H + (i >> 6), i & (kTP - 1))] = 0.f;
  __syncthreads();
}

// The 64 points of ptl through the trunk: the embedding, every hidden layer on the matrix cores (also a first layer narrower
// than 32: K is padded to 8 with zero weights and zero activations) and the output neuron, a dot product on the vector unit
// (lane p of wave 0 runs the chain of point p) -> dens[p] (LDS).  Every thread of the workgroup calls it; ptl may be
// rewritten after the call, act holds the last hidden activations (k-pair major), dens is complete after the next barrier.
__device__ __forceinline__ void tile_trunk(const Layout& lay, const float* __restrict__ pack, float* act, const float* ptl,
                                           float* dens) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float beta = pack[0];
  tile_embed(lay.H, lay.L[0].kstride, pack, act, ptl);
  for (int l = 0; l < lay.n_hidden; ++l)
    field::mfma_tile_layer<kThreads / 64>(lay.L[l], pack, act, false, [=](float z) { return softplus32(z, beta); });
  if (w == 0) {                   // the chain itself, lane = point
    const float* wo = pack + lay.out_w_off;
    float z = pack[lay.out_b_off];
    for (int k = 0; k < lay.out_K; ++k) z = fmaf(wo[k], act[act_index(k, lane)], z);
    dens[lane] = density32(softplus32(z, beta));
  }
}

// what every march and render entry requires of its rays; pointers: none of the arrays it needs is null
inline int check_march(const char* who, int N, bool pointers, int P, float threshold) {
  if (int rc = check_rows(who, N, pointers)) return rc;
  ISR_REQUIRE(P >= 1 && P <= kMaxP, "%s: P = %d (1..%d)", who, P, kMaxP);
  ISR_REQUIRE(threshold == threshold, "%s: threshold is NaN", who);
  return ISR_OK;
}

}  // namespace density
}  // namespace isr
