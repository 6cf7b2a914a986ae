// field_density.hip — the density field (field_density.hpp) and the ray march on top of it, each ONE launch: the entries of
// include/isr_density.h.
//
// field_trunk.hpp's scheme: a workgroup of 8 waves takes 64 points at a time through the trunk in LDS, so that neither the
// (N, 6H) embedding nor a hidden activation is ever in device memory, and owns whole rays.
//   * density_march_kernel makes its points from (origin, direction, length) in the kernel, o + d * len.
//   * The densities of a workgroup's rays stay in LDS (P <= 4096), then thread g marches ray g.  In threshold mode with one
//     ray per workgroup and no densities asked for, the tiles after the one holding the first hit are not evaluated:
//     march_ray multiplies whatever they would give by 0, so no output bit depends on it.  The march from the far end
//     (isr_density_march_dir, march_ray_back) does the same from the other side, and both directions together skip the tiles
//     between the first and the last hit.
// Rows past the end of a tile's work are evaluated at the origin and never written.
#include "field_trunk.hpp"

#include "../../include/isr_density.h"
#include "../../include/isr_density_dir.h"

#include <vector>

namespace {

using namespace isr::density;

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
  tile_trunk(lay, pack, act, ptl, dens);
  __syncthreads();
  if (tid < kTP && row0 + tid < N) out[row0 + tid] = dens[tid];
}

// kDir: 0 the march from the near end (march_ray), 1 from the far end (march_ray_back), 2 both.  Outputs of the back march
// of kDir 2 follow the front march's: depth[N + ray], points[3 (N + ray)], hit[N + ray], and a ray's weights are 2P wide,
// [front | back].  In threshold mode with one ray per workgroup and no densities asked for, only the tiles an output bit
// depends on are evaluated: front walks up to the tile of the first hit; back walks down from the far end to the tile of
// the last hit; both walks forward to the tile tf of the first hit and then from the far end down to, but not into, tf
// (the last hit is in tf when nothing lies above it).  rho[0 .. n_eval) and rho[lo_eval .. total) are what was evaluated,
// and all the marches read.
template <int kDir>
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
  const RayGroup rg(N, P, G);
  const long ray0 = rg.ray0;
  const int total = rg.total, T = rg.tiles;
  const bool early = threshold >= 0.f && dens_out == nullptr && G == 1;
  // tile t through the field -> dens[t * 64 ..); with `early`, whether one of its samples is above the threshold
  auto tile = [&](int t) -> bool {
    tile_points_from_rays(rg, P, t, origins, directions, lengths, ptl);
    __syncthreads();
    tile_trunk(lay, pack, act, ptl, dens + t * kTP);
    __syncthreads();
    if (!early) return false;
    const int q = t * kTP + (tid & 63);
    const int found = tid < kTP && q < total && dens[q] > threshold;
    return __syncthreads_or(found) != 0;
  };
  int n_eval = total, lo_eval = 0;
  int tf = kDir == 1 ? 0 : T;                        // the tiles [0, tf) are the forward walk's
  if (kDir != 1)
    for (int t = 0; t < T; ++t)
      if (tile(t)) {
        tf = t + 1;
        n_eval = tf * kTP < total ? tf * kTP : total;
        break;
      }
  if (kDir != 0)
    for (int t = T - 1; t >= tf; --t)
      if (tile(t)) {
        lo_eval = t * kTP;
        break;
      }
  if (dens_out)
    for (int q = tid; q < total; q += kThreads) dens_out[ray0 * P + q] = dens[q];
  if (kDir != 0) __syncthreads();                    // march_ray_back overwrites the densities it reads
  if (tid < rg.nr) {
    const long ray = ray0 + tid;
    float* rho = dens + tid * P;                     // G > 1: every point was evaluated
    float dep;
    int32_t h;
    if (kDir != 1) {
      const int left = n_eval - tid * P;
      float* w = w_out ? w_out + ray * P * (kDir == 2 ? 2 : 1) : nullptr;
      march_ray(P, lengths + ray * P, rho, left < P ? left : P, threshold, w, &dep, &h);
      depth[ray] = dep;
      hit[ray] = h;
      for (int d = 0; d < 3; ++d) points[3 * ray + d] = origins[3 * ray + d] + directions[3 * ray + d] * dep;
    }
    if (kDir != 0) {
      const long out = kDir == 2 ? (long)N + ray : ray;
      const int lo = lo_eval - tid * P;
      float* w = w_out ? (kDir == 2 ? w_out + ray * P * 2 + P : w_out + ray * P) : nullptr;
      march_ray_back(P, lengths + ray * P, rho, lo > 0 ? lo : 0, threshold, w, &dep, &h);
      depth[out] = dep;
      hit[out] = h;
      for (int d = 0; d < 3; ++d) points[3 * out + d] = origins[3 * ray + d] + directions[3 * ray + d] * dep;
    }
  }
}

// the checks every entry shares; on success lay is filled
int check_field(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, Layout& lay) {
  if (int rc = isr::check_pack_pointers(who, pack, widths)) return rc;
  ISR_REQUIRE(make_layout(n_hidden, widths, H, lay), "%s: %d hidden layers (1..%d), a width outside 1..%d or H = %d outside 1..%d",
              who, n_hidden, kMaxHidden, kMaxWidth, H, kMaxH);
  return isr::check_pack_bytes(who, pack_bytes, lay.total_words);
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
  if (int rc = isr::check_rows("isr_density_eval", N, pts && out)) return rc;
  if (N == 0) return ISR_OK;
  const unsigned blocks = (unsigned)(((long)N + kTP - 1) / kTP);
  density_eval_kernel<<<blocks, kThreads, 0, isr::as_stream(stream)>>>(lay, static_cast<const float*>(pack), pts, N, out);
  ISR_CHECK_LAUNCH("density_eval_kernel");
  return ISR_OK;
}

namespace {

int march_device(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                 const float* origins, const float* directions, const float* lengths, int N, int P, float threshold, int direction,
                 float* densities, float* weights, float* depth, float* points, int32_t* hit, isr_stream_t stream) {
  Layout lay;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths && depth && points && hit, P, threshold)) return rc;
  ISR_REQUIRE(direction >= 0 && direction <= 2, "%s: direction = %d (0 front, 1 back, 2 both)", who, direction);
  if (N == 0) return ISR_OK;
  const int G = rays_per_group(P);
  const unsigned blocks = (unsigned)(((long)N + G - 1) / G);
  const float* pk = static_cast<const float*>(pack);
  hipStream_t st = isr::as_stream(stream);
  if (direction == 0)
    density_march_kernel<0><<<blocks, kThreads, 0, st>>>(lay, pk, origins, directions, lengths, N, P, G, threshold, densities,
                                                         weights, depth, points, hit);
  else if (direction == 1)
    density_march_kernel<1><<<blocks, kThreads, 0, st>>>(lay, pk, origins, directions, lengths, N, P, G, threshold, densities,
                                                         weights, depth, points, hit);
  else
    density_march_kernel<2><<<blocks, kThreads, 0, st>>>(lay, pk, origins, directions, lengths, N, P, G, threshold, densities,
                                                         weights, depth, points, hit);
  ISR_CHECK_LAUNCH("density_march_kernel");
  return ISR_OK;
}

// The marches of ray `ray` of N for `direction`, as the entries lay their outputs out: the back march of "both" follows the
// front march's N rows, and a ray's weights are then 2P wide.  rho: the ray's P densities, which the back march overwrites.
void march_ray_host(long ray, int N, int P, const float* lengths, float* rho, float threshold, int direction, float* weights,
                    float* depth, int32_t* hit) {
  const float* len = lengths + ray * P;
  float* w = weights ? weights + ray * (direction == 2 ? 2L * P : P) : nullptr;
  if (direction != 1) march_ray(P, len, rho, P, threshold, w, &depth[ray], &hit[ray]);
  if (direction != 0) {
    const long out = direction == 2 ? (long)N + ray : ray;
    march_ray_back(P, len, rho, 0, threshold, w ? (direction == 2 ? w + P : w) : nullptr, &depth[out], &hit[out]);
  }
}

int march_host(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
               const float* origins, const float* directions, const float* lengths, int N, int P, float threshold, int direction,
               float* densities, float* weights, float* depth, float* points, int32_t* hit) {
  Layout lay;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths && depth && points && hit, P, threshold)) return rc;
  ISR_REQUIRE(direction >= 0 && direction <= 2, "%s: direction = %d (0 front, 1 back, 2 both)", who, direction);
  if (N == 0) return ISR_OK;
  const HostField hf(lay, pack);
  std::vector<float> rho((size_t)N * P);
  isr::parallel_rows((long)N * P, 64, [&](long q) {
    const long ray = q / P;
    float x[3];
    for (int d = 0; d < 3; ++d) x[d] = origins[3 * ray + d] + directions[3 * ray + d] * lengths[q];
    rho[q] = point_host(lay, pack, hf, x);
  });
  if (densities)
    for (size_t q = 0; q < rho.size(); ++q) densities[q] = rho[q];
  for (long ray = 0; ray < N; ++ray) {
    march_ray_host(ray, N, P, lengths, rho.data() + ray * P, threshold, direction, weights, depth, hit);
    for (long out = ray; out < (direction == 2 ? 2L : 1L) * N; out += N)
      for (int d = 0; d < 3; ++d) points[3 * out + d] = origins[3 * ray + d] + directions[3 * ray + d] * depth[out];
  }
  return ISR_OK;
}

}  // namespace

extern "C" int isr_density_march(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                 const float* origins, const float* directions, const float* lengths, int N, int P,
                                 float threshold, float* densities, float* weights, float* depth, float* points, int32_t* hit,
                                 isr_stream_t stream) {
  return march_device("isr_density_march", pack, pack_bytes, n_hidden, widths, H, origins, directions, lengths, N, P, threshold, 0,
                      densities, weights, depth, points, hit, stream);
}

extern "C" int isr_density_march_dir(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                     const float* origins, const float* directions, const float* lengths, int N, int P,
                                     float threshold, int direction, float* densities, float* weights, float* depth,
                                     float* points, int32_t* hit, isr_stream_t stream) {
  return march_device("isr_density_march_dir", pack, pack_bytes, n_hidden, widths, H, origins, directions, lengths, N, P,
                      threshold, direction, densities, weights, depth, points, hit, stream);
}

extern "C" int isr_density_eval_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                     const float* pts, int N, float* out) {
  Layout lay;
  if (int rc = check_field("isr_density_eval_host", pack, pack_bytes, n_hidden, widths, H, lay)) return rc;
  if (int rc = isr::check_rows("isr_density_eval_host", N, pts && out)) return rc;
  if (N == 0) return ISR_OK;
  const HostField hf(lay, pack);
  isr::parallel_rows(N, 64, [&](long i) { out[i] = point_host(lay, pack, hf, pts + 3 * i); });
  return ISR_OK;
}

extern "C" int isr_density_march_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                      const float* origins, const float* directions, const float* lengths, int N, int P,
                                      float threshold, float* densities, float* weights, float* depth, float* points,
                                      int32_t* hit) {
  return march_host("isr_density_march_host", pack, pack_bytes, n_hidden, widths, H, origins, directions, lengths, N, P, threshold,
                    0, densities, weights, depth, points, hit);
}

extern "C" int isr_density_march_dir_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                                          const float* origins, const float* directions, const float* lengths, int N, int P,
                                          float threshold, int direction, float* densities, float* weights, float* depth,
                                          float* points, int32_t* hit) {
  return march_host("isr_density_march_dir_host", pack, pack_bytes, n_hidden, widths, H, origins, directions, lengths, N, P,
                    threshold, direction, densities, weights, depth, points, hit);
}

extern "C" int isr_density_march_given_host(const float* lengths, const float* rho, int N, int P, float threshold, int direction,
                                            float* weights, float* depth, int32_t* hit) {
  const char* who = "isr_density_march_given_host";
  if (int rc = check_march(who, N, lengths && rho && depth && hit, P, threshold)) return rc;
  ISR_REQUIRE(direction >= 0 && direction <= 2, "%s: direction = %d (0 front, 1 back, 2 both)", who, direction);
  std::vector<float> r((size_t)P);
  for (long ray = 0; ray < N; ++ray) {
    for (int k = 0; k < P; ++k) r[k] = rho[ray * P + k];
    march_ray_host(ray, N, P, lengths, r.data(), threshold, direction, weights, depth, hit);
  }
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
