// field_radiance.hip — the radiance field (field_radiance.hpp) rendered into per-ray images, and the emission-absorption
// march alone: the entries of include/isr_radiance.h.
//
// field_trunk.hpp's scheme: 8 waves per workgroup, a workgroup owns G = max(1, 64 / P) consecutive rays and takes their
// G * P points 64 at a time through the field in LDS.  Per tile: the density trunk (tile_trunk: the embedding, the hidden
// layers on the matrix cores, the density neuron on h), colour layer 1 in place over h, softplus, colour layer 2
// and the sigmoid into the tile's (64, C) colours at the front of the activation buffer; then thread g advances the render
// of ray g (RayState: T, feat_c, depth, hit in registers) over the tile's samples of its ray in k order.  Nothing per point
// reaches device memory unless densities, colours or weights is asked for.
//   * The direction term is a per-ray bias of colour layer 1 and a tile holds up to 64 different rays (P = 1), so it does not
//     fit beside the 96 KB activation buffer: radiance_dir_kernel takes 64 RAYS as a tile's 64 points, embeds their
//     normalised directions and runs the Wc x 6H block on the matrix cores into the workspace u (N, WcP) — the fmaf chain
//     from b1, so the bits are the host's — and colour layer 1's accumulators start from u[ray of the point][neuron]
//     (field_tile.hpp's mfma_tile_layer_from).
//   * In threshold mode with one ray per workgroup and neither densities nor colours asked for, the tiles behind the one
//     holding the first hit are not evaluated: their samples have weight 0.  The owner still walks their lengths (depth is
//     a maximum over every len_k * w_k) and their points: a point that is not finite has NaN colours and fmaf(0, NaN, .)
//     poisons the features as the full evaluation does.
// Rows past the end of a tile's work are evaluated at the origin with the workgroup's first ray's term and never written.
#include "field_radiance.hpp"
#include "field_trunk.hpp"

#include "../../include/isr_radiance.h"

#include <vector>

namespace {

using namespace isr::radiance;
using isr::density::check_march;
using isr::density::kActWords;
using isr::density::kThreads;
using isr::density::RayGroup;
using isr::density::softplus32;
using isr::density::tile_embed;
using isr::density::tile_points_from_rays;
using isr::density::tile_trunk;
using isr::field::kTP;

// u (N, WcP): 64 rays per workgroup
__global__ __launch_bounds__(kThreads) void radiance_dir_kernel(Layout lay, const float* __restrict__ pack,
                                                                const float* __restrict__ directions, int N,
                                                                float* __restrict__ u) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  const int tid = threadIdx.x;
  const long ray0 = (long)blockIdx.x * kTP;
  if (tid < kTP) {
    const long ray = ray0 + tid;
    float d[3] = {0.f, 0.f, 0.f}, dn[3];
    if (ray < N)
      for (int i = 0; i < 3; ++i) d[i] = directions[3 * ray + i];
    normalize3(d, dn);
    for (int i = 0; i < 3; ++i) ptl[i * kTP + tid] = dn[i];
  }
  __syncthreads();
  tile_embed(lay.d.H, lay.dir.kstride, pack, act, ptl);
  isr::field::mfma_tile_layer<kThreads / 64>(lay.dir, pack, act, true, [](float z) { return z; });      // act[p * Wc + j]
  for (int i = tid; i < kTP * lay.WcP; i += kThreads) {
    const int p = i / lay.WcP, j = i - p * lay.WcP;
    if (ray0 + p < N) u[(ray0 + p) * lay.WcP + j] = j < lay.Wc ? act[p * lay.Wc + j] : 0.f;
  }
}

// where colour layer 1's chains start: u of the point's ray
struct RayTermInit {
  const float* u;
  long ray0;
  int P, total, t0, WcP;      // t0: the tile's first sample among the workgroup's
  __device__ __forceinline__ float operator()(int j, int p) const {
    const int q = t0 + p;
    const long ray = ray0 + (q < total ? q / P : 0);
    return u[ray * WcP + j];
  }
};

__global__ __launch_bounds__(kThreads) void radiance_render_kernel(Layout lay, const float* __restrict__ pack,
                                                                   const float* __restrict__ origins,
                                                                   const float* __restrict__ directions,
                                                                   const float* __restrict__ lengths, int N, int P, int G,
                                                                   float threshold, const float* __restrict__ u,
                                                                   float* __restrict__ image, float* __restrict__ depth,
                                                                   float* __restrict__ points, int32_t* __restrict__ hit,
                                                                   float* __restrict__ w_out, float* __restrict__ dens_out,
                                                                   float* __restrict__ col_out) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  __shared__ float dens[kTP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int C = lay.C;
  const float beta = pack[0];
  const RayGroup rg(N, P, G);
  const long ray0 = rg.ray0;
  const int total = rg.total, T = rg.tiles;
  const bool early = threshold >= 0.f && dens_out == nullptr && col_out == nullptr && G == 1;
  const bool owner = tid < rg.nr;
  const long ray = ray0 + (owner ? tid : 0);
  const float* len = lengths + ray * P;
  RayState<kMaxC> st;
  st.start();
  int k_done = 0;                                    // the owner's samples [0, k_done) are rendered
  for (int t = 0; t < T; ++t) {
    tile_points_from_rays(rg, P, t, origins, directions, lengths, ptl);
    __syncthreads();                                 // also: the owners are done with the previous tile's colours
    tile_trunk(lay.d, pack, act, ptl, dens);         // no barrier behind the density neuron: the next layer reads act first
    isr::field::mfma_tile_layer_from<kThreads / 64>(lay.trunk, pack, act, false, [=](float z) { return softplus32(z, beta); },
                                                    RayTermInit{u, ray0, P, total, t * kTP, lay.WcP});
    isr::field::mfma_tile_layer<kThreads / 64>(lay.out, pack, act, true, [](float z) { return sigmoid32(z); });
    // act[p * C + c]: the colours of the tile's points; dens[p]: their densities
    const int n_tile = total - t * kTP < kTP ? total - t * kTP : kTP;
    if (dens_out)
      for (int i = tid; i < n_tile; i += kThreads) dens_out[ray0 * P + t * kTP + i] = dens[i];
    if (col_out)
      for (int i = tid; i < n_tile * C; i += kThreads) col_out[(ray0 * P + t * kTP) * C + i] = act[i];
    if (owner) {
      const int k1 = (t + 1) * kTP - tid * P < P ? (t + 1) * kTP - tid * P : P;      // G > 1: one tile holds every ray
      for (int k = k_done; k < k1; ++k) {
        const int p = tid * P + k - t * kTP;
        const float w = st.step(k, len[k], dens[p], true, threshold, act + p * C, C, false);
        if (w_out) w_out[ray * P + k] = w;
      }
      k_done = k1 > k_done ? k1 : k_done;
    }
    if (early) {
      const int found = tid < kTP && t * kTP + lane < total && dens[lane] > threshold;
      if (__syncthreads_or(found)) break;
    }
  }
  if (owner) {
    float o[3], d[3];
    for (int i = 0; i < 3; ++i) {
      o[i] = origins[3 * ray + i];
      d[i] = directions[3 * ray + i];
    }
    for (int k = k_done; k < P; ++k) {               // behind the first hit: weight 0
      float x[3];
      for (int i = 0; i < 3; ++i) x[i] = o[i] + d[i] * len[k];
      const float w = st.step(k, len[k], 0.f, false, threshold, nullptr, C, !finite3(x));
      if (w_out) w_out[ray * P + k] = w;
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) image[ray * (C + 1) + c] = st.feat[c];
    image[ray * (C + 1) + C] = st.opacity();
    depth[ray] = st.m;
    hit[ray] = st.any;
    for (int i = 0; i < 3; ++i) points[3 * ray + i] = o[i] + d[i] * st.m;
  }
}

// one ray per lane
__global__ __launch_bounds__(256) void ea_march_kernel(const float* __restrict__ densities, const float* __restrict__ features,
                                                       int N, int P, int F, float threshold, float* __restrict__ image,
                                                       float* __restrict__ weights) {
  const long ray = (long)blockIdx.x * 256 + threadIdx.x;
  if (ray >= N) return;
  ea_march_ray(P, F, densities + ray * P, features + ray * P * F, threshold, image + ray * (F + 1),
               weights ? weights + ray * P : nullptr);
}

int check_field(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                Layout& lay) {
  if (int rc = isr::check_pack_pointers(who, pack, widths)) return rc;
  ISR_REQUIRE(make_layout(n_hidden, widths, H, Wc, C, lay),
              "%s: %d hidden layers (1..%d), a width outside 1..%d, H = %d outside 1..%d, Wc = %d outside 1..%d or C = %d outside "
              "1..%d",
              who, n_hidden, isr::density::kMaxHidden, kMaxWidth, H, kMaxH, Wc, kMaxWidth, C, kMaxC);
  return isr::check_pack_bytes(who, pack_bytes, lay.total_words);
}

int check_ea(const char* who, const float* densities, const float* features, int N, int P, int F, float threshold,
             const float* image) {
  if (int rc = isr::check_rows(who, N, densities && features && image)) return rc;
  ISR_REQUIRE(P >= 1 && P <= kMaxP, "%s: P = %d (1..%d)", who, P, kMaxP);
  ISR_REQUIRE(F >= 1 && F <= kMaxF, "%s: F = %d (1..%d)", who, F, kMaxF);
  ISR_REQUIRE(threshold == threshold, "%s: threshold is NaN", who);
  return ISR_OK;
}

size_t ws_bytes_for(int N, int Wc) { return (size_t)N * (size_t)((Wc + 31) / 32 * 32) * 4; }

}  // namespace

extern "C" size_t isr_radiance_pack_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C) {
  Layout lay;
  if (!widths || !make_layout(n_hidden, widths, H, Wc, C, lay)) {
    isr::set_error("isr_radiance_pack_bytes: null widths, or a hidden layer count (1..%d), a width (1..%d), H (1..%d), Wc (1..%d) "
                   "or C (1..%d) out of range",
                   isr::density::kMaxHidden, kMaxWidth, kMaxH, kMaxWidth, kMaxC);
    return 0;
  }
  return (size_t)lay.total_words * 4;
}

extern "C" int isr_radiance_pack(int n_hidden, const int32_t* widths, int H, int Wc, int C, const float* freqs, float beta,
                                 const float* W, const float* b, void* pack, size_t pack_bytes) {
  Layout lay;
  if (int rc = check_field("isr_radiance_pack", pack, pack_bytes, n_hidden, widths, H, Wc, C, lay)) return rc;
  ISR_REQUIRE(freqs && W && b, "isr_radiance_pack: null pointer");
  ISR_REQUIRE(beta > 0.f && beta <= 3.0e38f, "isr_radiance_pack: beta = %g must be positive and finite", (double)beta);
  pack_host(lay, freqs, beta, W, b, pack);
  return ISR_OK;
}

extern "C" size_t isr_radiance_workspace_bytes(int N, int Wc) {
  if (N < 0 || Wc < 1 || Wc > kMaxWidth) {
    isr::set_error("isr_radiance_workspace_bytes: N = %d, Wc = %d (1..%d)", N, Wc, kMaxWidth);
    return 0;
  }
  return ws_bytes_for(N, Wc);
}

extern "C" int isr_radiance_render(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                                   const float* origins, const float* directions, const float* lengths, int N, int P,
                                   float threshold, float* image, float* depth, float* points, int32_t* hit, float* weights,
                                   float* densities, float* colours, void* ws, size_t ws_bytes, isr_stream_t stream) {
  const char* who = "isr_radiance_render";
  Layout lay;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, Wc, C, lay)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths && image && depth && points && hit, P, threshold)) return rc;
  if (N == 0) return ISR_OK;
  ISR_REQUIRE(ws && ws_bytes >= ws_bytes_for(N, Wc), "%s: workspace of %zu bytes, %zu needed", who, ws ? ws_bytes : (size_t)0,
              ws_bytes_for(N, Wc));
  ISR_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace is not 16-byte aligned", who);
  const float* pk = static_cast<const float*>(pack);
  float* u = static_cast<float*>(ws);
  hipStream_t st = isr::as_stream(stream);
  radiance_dir_kernel<<<(unsigned)(((long)N + kTP - 1) / kTP), kThreads, 0, st>>>(lay, pk, directions, N, u);
  ISR_CHECK_LAUNCH("radiance_dir_kernel");
  const int G = isr::density::rays_per_group(P);
  radiance_render_kernel<<<(unsigned)(((long)N + G - 1) / G), kThreads, 0, st>>>(lay, pk, origins, directions, lengths, N, P, G,
                                                                                 threshold, u, image, depth, points, hit, weights,
                                                                                 densities, colours);
  ISR_CHECK_LAUNCH("radiance_render_kernel");
  return ISR_OK;
}

extern "C" int isr_ea_march(const float* densities, const float* features, int N, int P, int F, float threshold, float* image,
                            float* weights, isr_stream_t stream) {
  if (int rc = check_ea("isr_ea_march", densities, features, N, P, F, threshold, image)) return rc;
  if (N == 0) return ISR_OK;
  ea_march_kernel<<<(unsigned)(((long)N + 255) / 256), 256, 0, isr::as_stream(stream)>>>(densities, features, N, P, F, threshold,
                                                                                         image, weights);
  ISR_CHECK_LAUNCH("ea_march_kernel");
  return ISR_OK;
}

extern "C" int isr_radiance_render_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc,
                                        int C, const float* origins, const float* directions, const float* lengths, int N, int P,
                                        float threshold, float* image, float* depth, float* points, int32_t* hit, float* weights,
                                        float* densities, float* colours) {
  const char* who = "isr_radiance_render_host";
  Layout lay;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, Wc, C, lay)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths && image && depth && points && hit, P, threshold)) return rc;
  if (N == 0) return ISR_OK;
  const HostField hf(lay, pack);
  std::vector<float> u((size_t)N * Wc), rho((size_t)N * P), col((size_t)N * P * C);
  isr::parallel_rows(N, 64, [&](long ray) {
#ifdef ISR_RADIANCE_HAVE_FMA_BUILD
    if (hf.fma) return ray_term_host_fma(lay, pack, hf.hw, directions + 3 * ray, u.data() + ray * Wc);
#endif
    ray_term_host(lay, pack, hf.hw, directions + 3 * ray, u.data() + ray * Wc);
  });
  isr::parallel_rows((long)N * P, 64, [&](long q) {
    const long ray = q / P;
    float x[3];
    for (int d = 0; d < 3; ++d) x[d] = origins[3 * ray + d] + directions[3 * ray + d] * lengths[q];
#ifdef ISR_RADIANCE_HAVE_FMA_BUILD
    if (hf.fma) return point_radiance_host_fma(lay, pack, hf.hw, x, u.data() + ray * Wc, &rho[q], &col[(size_t)q * C]);
#endif
    point_radiance_host(lay, pack, hf.hw, x, u.data() + ray * Wc, &rho[q], &col[(size_t)q * C]);
  });
  if (densities)
    for (size_t q = 0; q < rho.size(); ++q) densities[q] = rho[q];
  if (colours)
    for (size_t q = 0; q < col.size(); ++q) colours[q] = col[q];
  for (long ray = 0; ray < N; ++ray) {
    RayState<kMaxC> st;
    st.start();
    for (int k = 0; k < P; ++k) {
      const size_t q = (size_t)ray * P + k;
      const float w = st.step(k, lengths[q], rho[q], true, threshold, &col[q * C], C, false);
      if (weights) weights[q] = w;
    }
    for (int c = 0; c < C; ++c) image[ray * (C + 1) + c] = st.feat[c];
    image[ray * (C + 1) + C] = st.opacity();
    depth[ray] = st.m;
    hit[ray] = st.any;
    for (int d = 0; d < 3; ++d) points[3 * ray + d] = origins[3 * ray + d] + directions[3 * ray + d] * st.m;
  }
  return ISR_OK;
}

extern "C" int isr_ea_march_host(const float* densities, const float* features, int N, int P, int F, float threshold,
                                 float* image, float* weights) {
  if (int rc = check_ea("isr_ea_march_host", densities, features, N, P, F, threshold, image)) return rc;
  for (long ray = 0; ray < N; ++ray)
    ea_march_ray(P, F, densities + ray * P, features + (size_t)ray * P * F, threshold, image + ray * (F + 1),
                 weights ? weights + ray * P : nullptr);
  return ISR_OK;
}

extern "C" int isr_radiance_sigmoid_host(const float* z, size_t n, float* out) {
  ISR_REQUIRE(n == 0 || (z && out), "isr_radiance_sigmoid_host: null pointer");
  for (size_t i = 0; i < n; ++i) out[i] = sigmoid32(z[i]);
  return ISR_OK;
}

extern "C" int isr_radiance_normalize_host(const float* d, size_t n, float* out) {
  ISR_REQUIRE(n == 0 || (d && out), "isr_radiance_normalize_host: null pointer");
  for (size_t i = 0; i < n; ++i) normalize3(d + 3 * i, out + 3 * i);
  return ISR_OK;
}
