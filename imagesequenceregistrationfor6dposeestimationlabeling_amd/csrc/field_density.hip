// field_density.hip — the density field (field_density.hpp) and the ray march on top of it, each ONE launch: the entries of
// include/isr_density.h.
//
// field_mlp.hip's design: a workgroup takes a tile of 64 points through every layer, the tile's activations live in LDS, the
// weights are streamed from the pack in matrix-core order, the bias sits in the accumulator and the k loop runs in order, so
// v_mfma_f32_32x32x2_f32 gives the k-ordered fmaf chain bit for bit.  What differs:
//   * The first layer's input is the harmonic embedding, computed in the kernel into LDS (sincos32, one call per sine /
//     cosine pair).  The activation buffer holds 384 k's x 64 points = 96 KB, so one workgroup is resident per CU; it has
//     8 waves (512 threads), two per SIMD, and wave w takes neuron block w of a 256-wide layer over both point blocks.
//     Neither the (N, 6H) embedding nor a hidden activation is ever in device memory.
//   * Every hidden layer runs on the matrix cores, also a first layer narrower than 32 (K is padded to 8 with zero weights
//     and zero activations).
//   * The output neuron is a dot product on the vector unit: lane p of wave 0 runs the chain of point p.
//   * density_march_kernel makes its points from (origin, direction, length) in the kernel, o + d * len.
// A WORKGROUP OWNS WHOLE RAYS: G = max(1, 64 / P) consecutive rays, their G * P points taken 64 at a time; the densities of
// its rays stay in LDS (P <= 4096), then thread g marches ray g.  In threshold mode with one ray per workgroup and no
// densities asked for, the tiles after the one holding the first hit are not evaluated: march_ray multiplies whatever they
// would give by 0, so no output bit depends on it.
// Rows past the end of a tile's work are evaluated at the origin and never written.
#include "field_density.hpp"
#include "isr_common.hpp"

#include "../../include/isr_density.h"

#include <thread>
#include <vector>

namespace {

using namespace isr::density;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTP = 64;            // points per tile
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kActWords = (6 * kMaxH / 2) * kTP * 2;      // 96 KB

__device__ __forceinline__ int act_index(int k, int p) { return ((k >> 1) * kTP + p) * 2 + (k & 1); }

// One wave's share of a layer: neuron block mb x NNB blocks of 32 points from point block nb0.
template <int NNB>
__device__ __forceinline__ void mfma_block(const Layer& L, const float* __restrict__ Wl, const float* __restrict__ bl,
                                           const float* act, int mb, int nb0, int lane, f32x16 (&acc)[2]) {
  const int r = lane & 31, hh = lane >> 5;
  const int S4 = L.kstride >> 3;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float bias = bl[mb * 32 + 8 * a + 4 * hh + b];
#pragma unroll
      for (int n = 0; n < NNB; ++n) acc[n][4 * a + b] = bias;
    }
  const float4* wp = reinterpret_cast<const float4*>(Wl) + (size_t)mb * S4 * 64 + lane;
  float4 cur = wp[0];
  const float* bp = act + (nb0 * 32 + r) * 2 + hh;
  for (int s4 = 0; s4 < S4; ++s4) {
    const int sn = s4 + 1 < S4 ? s4 + 1 : s4;
    const float4 nxt = wp[(size_t)sn * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float bv[NNB];
#pragma unroll
      for (int n = 0; n < NNB; ++n) bv[n] = bp[((4 * s4 + i) * kTP + n * 32) * 2];
      const float av = i == 0 ? cur.x : i == 1 ? cur.y : i == 2 ? cur.z : cur.w;
#pragma unroll
      for (int n = 0; n < NNB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[n], acc[n], 0, 0, 0);
    }
    cur = nxt;
  }
}

// The 64 points of ptl (LDS, coordinate-major: ptl[d * 64 + p]) through the field; density of point p -> dens[p] (LDS).
// Every thread of the workgroup calls it; ptl may be rewritten after the call, dens is complete after the next barrier.
__device__ __forceinline__ void tile_density(const Layout& lay, const float* __restrict__ pack, float* act, const float* ptl,
                                             float* dens) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int r = lane & 31, hh = lane >> 5;
  const int H = lay.H;
  const float beta = pack[0];
  const float* freqs = pack + kFreqOff;

  // the embedding: k = d * H + i holds the sine, 3H + k the cosine; k in [6H, kstride) zeros
  for (int i = tid; i < 3 * H * kTP; i += kThreads) {
    const int p = i & (kTP - 1), kk = i >> 6;
    const int d = kk / H, fi = kk - d * H;
    const float a = ptl[d * kTP + p] * freqs[fi];
    float s, c;
    sincos32(a, &s, &c);
    act[act_index(kk, p)] = s;
    act[act_index(3 * H + kk, p)] = c;
  }
  for (int i = tid; i < (lay.L[0].kstride - 6 * H) * kTP; i += kThreads) act[act_index(6 * H + (i >> 6), i & (kTP - 1))] = 0.f;
  __syncthreads();

  for (int l = 0; l < lay.n_hidden; ++l) {
    const Layer L = lay.L[l];
    const float* Wl = pack + L.w_off;
    const float* bl = pack + L.b_off;
    const int MB = L.OP >> 5;
    int mb, nb0, nnb;
    if (MB > kWaves / 2) {        // a wave: one neuron block, both point blocks
      mb = w;
      nb0 = 0;
      nnb = 2;
    } else {                      // up to four neuron blocks: a wave takes one 32 x 32 tile
      mb = w >> 1;
      nb0 = w & 1;
      nnb = 1;
    }
    const bool active = mb < MB;
    f32x16 acc[2];
    if (active) {
      if (nnb == 2) mfma_block<2>(L, Wl, bl, act, mb, nb0, lane, acc);
      else mfma_block<1>(L, Wl, bl, act, mb, nb0, lane, acc);
    }
    __syncthreads();              // every wave has read the layer's input: the outputs may take its place
    if (active) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (n < nnb) {
          const int p = (nb0 + n) * 32 + r;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const int j = mb * 32 + 8 * a + 4 * hh;
            float v[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) v[b] = j + b < L.O ? softplus32(acc[n][4 * a + b], beta) : 0.f;
            *reinterpret_cast<float2*>(&act[((j >> 1) * kTP + p) * 2]) = make_float2(v[0], v[1]);
            *reinterpret_cast<float2*>(&act[(((j >> 1) + 1) * kTP + p) * 2]) = make_float2(v[2], v[3]);
          }
        }
      }
    }
    __syncthreads();
  }

  if (w == 0) {                   // the output neuron: the chain itself, lane = point
    const float* wo = pack + lay.out_w_off;
    float z = pack[lay.out_b_off];
    for (int k = 0; k < lay.out_K; ++k) z = fmaf(wo[k], act[act_index(k, lane)], z);
    dens[lane] = density32(softplus32(z, beta));
  }
}

__global__ __launch_bounds__(kThreads) void density_eval_kernel(Layout lay, const float* __restrict__ pack,
                                                                const float* __restrict__ pts, int N, float* __restrict__ out) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  __shared__ float dens[kTP];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * kTP;
  if (tid < 3 * kTP) {
    const int d = tid >> 6, p = tid & 63;
    const long row = row0 + p;
    ptl[tid] = row < N ? pts[3 * row + d] : 0.f;
  }
  __syncthreads();
  tile_density(lay, pack, act, ptl, dens);
  __syncthreads();
  if (tid < kTP && row0 + tid < N) out[row0 + tid] = dens[tid];
}

__global__ __launch_bounds__(kThreads) void density_march_kernel(Layout lay, const float* __restrict__ pack,
                                                                 const float* __restrict__ origins,
                                                                 const float* __restrict__ directions,
                                                                 const float* __restrict__ lengths, int N, int P, int G,
                                                                 float threshold, float* __restrict__ dens_out,
                                                                 float* __restrict__ w_out, float* __restrict__ depth,
                                                                 float* __restrict__ points, int32_t* __restrict__ hit) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  __shared__ float dens[kMaxP];
  const int tid = threadIdx.x;
  const long ray0 = (long)blockIdx.x * G;
  const int nr = (long)N - ray0 < G ? (int)((long)N - ray0) : G;
  const int total = nr * P;                          // <= max(64, P) <= kMaxP
  const int T = (total + kTP - 1) / kTP;
  const bool early = threshold >= 0.f && dens_out == nullptr && G == 1;
  int n_eval = total;
  for (int t = 0; t < T; ++t) {
    const int q = t * kTP + (tid & 63);
    if (tid < 3 * kTP) {
      const int d = tid >> 6;
      float v = 0.f;
      if (q < total) {
        const int g = q / P, k = q - g * P;
        const long ray = ray0 + g;
        v = origins[3 * ray + d] + directions[3 * ray + d] * lengths[ray * P + k];
      }
      ptl[tid] = v;
    }
    __syncthreads();
    tile_density(lay, pack, act, ptl, dens + t * kTP);
    __syncthreads();
    if (early) {
      const int found = tid < kTP && q < total && dens[q] > threshold;
      if (__syncthreads_or(found)) {
        n_eval = (t + 1) * kTP < total ? (t + 1) * kTP : total;
        break;
      }
    }
  }
  if (dens_out)
    for (int q = tid; q < total; q += kThreads) dens_out[ray0 * P + q] = dens[q];
  if (tid < nr) {
    const long ray = ray0 + tid;
    const int left = n_eval - tid * P;               // G > 1: every point was evaluated
    float dep;
    int32_t h;
    march_ray(P, lengths + ray * P, dens + tid * P, left < P ? left : P, threshold, w_out ? w_out + ray * P : nullptr, &dep, &h);
    depth[ray] = dep;
    hit[ray] = h;
    for (int d = 0; d < 3; ++d) points[3 * ray + d] = origins[3 * ray + d] + directions[3 * ray + d] * dep;
  }
}

// the checks every entry shares; on success lay is filled
int check_field(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, Layout& lay) {
  ISR_REQUIRE(pack && widths, "%s: null pointer", who);
  ISR_REQUIRE(make_layout(n_hidden, widths, H, lay), "%s: %d hidden layers (1..%d), a width outside 1..%d or H = %d outside 1..%d",
              who, n_hidden, kMaxHidden, kMaxWidth, H, kMaxH);
  ISR_REQUIRE(pack_bytes == (size_t)lay.total_words * 4, "%s: pack_bytes %zu, this field packs to %zu", who, pack_bytes,
              (size_t)lay.total_words * 4);
  return ISR_OK;
}

int check_march(const char* who, const float* origins, const float* directions, const float* lengths, int N, int P,
                float threshold, const float* depth, const float* points, const int32_t* hit) {
  ISR_REQUIRE(N >= 0, "%s: N = %d", who, N);
  ISR_REQUIRE(P >= 1 && P <= kMaxP, "%s: P = %d (1..%d)", who, P, kMaxP);
  ISR_REQUIRE(threshold == threshold, "%s: threshold is NaN", who);
  ISR_REQUIRE(N == 0 || (origins && directions && lengths && depth && points && hit), "%s: null pointer", who);
  return ISR_OK;
}

struct HostField {
  std::vector<std::vector<float>> wt;
  HostWeights hw;
  bool fma;
  HostField(const Layout& lay, const void* pack) {
    const float* pf = static_cast<const float*>(pack);
    wt.resize(lay.n_hidden);
    for (int l = 0; l < lay.n_hidden; ++l) {
      const Layer& L = lay.L[l];
      wt[l].resize((size_t)L.O * L.K);
      for (int j = 0; j < L.O; ++j)
        for (int k = 0; k < L.K; ++k) wt[l][(size_t)k * L.O + j] = pf[L.w_off + w_index(L, j, k)];
      hw.Wt[l] = wt[l].data();
    }
#ifdef ISR_DENSITY_HAVE_FMA_BUILD
    fma = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#else
    fma = false;
#endif
  }
};

// fn(i) for i in [0, n) over a few threads
template <class F>
void parallel_rows(long n, long per_thread_min, F fn) {
  const int nthreads = n >= 8 * per_thread_min ? 8 : 1;
  if (nthreads == 1) {
    for (long i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t) {
    const long n0 = n * t / nthreads, n1 = n * (t + 1) / nthreads;
    pool.emplace_back([=] {
      for (long i = n0; i < n1; ++i) fn(i);
    });
  }
  for (auto& th : pool) th.join();
}

float point_host(const Layout& lay, const void* pack, const HostField& hf, const float* x) {
#ifdef ISR_DENSITY_HAVE_FMA_BUILD
  if (hf.fma) return point_density_host_fma(lay, pack, hf.hw, x);
#endif
  return point_density_host(lay, pack, hf.hw, x);
}

}  // namespace

extern "C" size_t isr_density_pack_bytes(int n_hidden, const int32_t* widths, int H) {
  Layout lay;
  if (!widths || !make_layout(n_hidden, widths, H, lay)) {
    isr::set_error("isr_density_pack_bytes: null widths, or a hidden layer count (1..%d), a width (1..%d) or H (1..%d) out of range",
                   kMaxHidden, kMaxWidth, kMaxH);
    return 0;
  }
  return (size_t)lay.total_words * 4;
}

extern "C" int isr_density_pack(int n_hidden, const int32_t* widths, int H, const float* freqs, float beta, const float* W,
                                const float* b, void* pack, size_t pack_bytes) {
  Layout lay;
  if (int rc = check_field("isr_density_pack", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  ISR_REQUIRE(freqs && W && b, "isr_density_pack: null pointer");
  ISR_REQUIRE(beta > 0.f && beta <= 3.0e38f, "isr_density_pack: beta = %g must be positive and finite", (double)beta);
  pack_host(lay, freqs, beta, W, b, pack);
  return ISR_OK;
}

extern "C" int isr_density_eval(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* pts,
                                int N, float* out, isr_stream_t stream) {
  Layout lay;
  if (int rc = check_field("isr_density_eval", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  ISR_REQUIRE(N >= 0, "isr_density_eval: N = %d", N);
  ISR_REQUIRE(N == 0 || (pts && out), "isr_density_eval: null pointer");
  if (N == 0) return ISR_OK;
  const unsigned blocks = (unsigned)(((long)N + kTP - 1) / kTP);
  density_eval_kernel<<<blocks, kThreads, 0, isr::as_stream(stream)>>>(lay, static_cast<const float*>(pack), pts, N, out);
  ISR_CHECK_LAUNCH("density_eval_kernel");
  return ISR_OK;
}

extern "C" int isr_density_march(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                 const float* origins, const float* directions, const float* lengths, int N, int P,
                                 float threshold, float* densities, float* weights, float* depth, float* points, int32_t* hit,
                                 isr_stream_t stream) {
  Layout lay;
  if (int rc = check_field("isr_density_march", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  if (int rc = check_march("isr_density_march", origins, directions, lengths, N, P, threshold, depth, points, hit)) return rc;
  if (N == 0) return ISR_OK;
  const int G = P >= kTP ? 1 : kTP / P;
  const unsigned blocks = (unsigned)(((long)N + G - 1) / G);
  density_march_kernel<<<blocks, kThreads, 0, isr::as_stream(stream)>>>(lay, static_cast<const float*>(pack), origins, directions,
                                                                        lengths, N, P, G, threshold, densities, weights, depth,
                                                                        points, hit);
  ISR_CHECK_LAUNCH("density_march_kernel");
  return ISR_OK;
}

extern "C" int isr_density_eval_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                     const float* pts, int N, float* out) {
  Layout lay;
  if (int rc = check_field("isr_density_eval_host", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  ISR_REQUIRE(N >= 0, "isr_density_eval_host: N = %d", N);
  ISR_REQUIRE(N == 0 || (pts && out), "isr_density_eval_host: null pointer");
  if (N == 0) return ISR_OK;
  const HostField hf(lay, pack);
  parallel_rows(N, 64, [&](long i) { out[i] = point_host(lay, pack, hf, pts + 3 * i); });
  return ISR_OK;
}

extern "C" int isr_density_march_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                      const float* origins, const float* directions, const float* lengths, int N, int P,
                                      float threshold, float* densities, float* weights, float* depth, float* points,
                                      int32_t* hit) {
  Layout lay;
  if (int rc = check_field("isr_density_march_host", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  if (int rc = check_march("isr_density_march_host", origins, directions, lengths, N, P, threshold, depth, points, hit)) return rc;
  if (N == 0) return ISR_OK;
  const HostField hf(lay, pack);
  std::vector<float> rho((size_t)N * P);
  parallel_rows((long)N * P, 64, [&](long q) {
    const long ray = q / P;
    float x[3];
    for (int d = 0; d < 3; ++d) x[d] = origins[3 * ray + d] + directions[3 * ray + d] * lengths[q];
    rho[q] = point_host(lay, pack, hf, x);
  });
  for (long ray = 0; ray < N; ++ray) {
    march_ray(P, lengths + ray * P, rho.data() + ray * P, P, threshold, weights ? weights + ray * P : nullptr, &depth[ray],
              &hit[ray]);
    for (int d = 0; d < 3; ++d) points[3 * ray + d] = origins[3 * ray + d] + directions[3 * ray + d] * depth[ray];
  }
  if (densities)
    for (size_t q = 0; q < rho.size(); ++q) densities[q] = rho[q];
  return ISR_OK;
}

extern "C" int isr_density_sincos_host(const float* a, size_t n, float* sin_out, float* cos_out) {
  ISR_REQUIRE(n == 0 || (a && sin_out && cos_out), "isr_density_sincos_host: null pointer");
  for (size_t i = 0; i < n; ++i) sincos32(a[i], &sin_out[i], &cos_out[i]);
  return ISR_OK;
}

extern "C" int isr_density_activations_host(const float* z, size_t n, float beta, float* softplus_out, float* density_out) {
  ISR_REQUIRE(n == 0 || (z && softplus_out && density_out), "isr_density_activations_host: null pointer");
  for (size_t i = 0; i < n; ++i) {
    softplus_out[i] = softplus32(z[i], beta);
    density_out[i] = density32(z[i]);
  }
  return ISR_OK;
}
