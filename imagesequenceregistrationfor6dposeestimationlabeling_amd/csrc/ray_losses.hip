// ray_losses.hip — the distortion loss and the render loss with their gradients on the device (ray_losses.hpp states the
// arithmetic): the entries of include/isr_ray_losses.h.  No call synchronises, no float atomics, and nothing per pair or per
// sampled target reaches memory.
//
//   distortion_kernel<RB, BACKWARD>   a wave owns a ray: its t, ut and w sit in LDS (12 bytes a sample), lane `lane` owns rows
//                                     i = lane, lane + 64, .. , RB of them at a time in registers, and walks j ascending — every
//                                     lane reads the same LDS address, a broadcast — so each inner_i is one f64 chain whatever RB
//                                     is.  Forward: the lanes' f64 sums meet in a shuffle tree, lane 0 writes the ray's f64 value
//                                     (and ray_loss).  Backward: every lane writes its rows of dweights, column P-1 gets +0.
//   render_rows_kernel                a lane owns a ray of the render: (row_c, row_o), then the tree over the workgroup's 256 rays
//   isr::reduce_kernel                (ordered_sum.hpp) one level of REDUCE ORDER over NV interleaved sums; the level that leaves
//                                     one value also writes the mean(s), MeanFinish
//   render_backward_kernel            a lane owns an element of drendered
// A work item is taken from a grid-stride loop, so no shape within the limits overflows a grid dimension.
#include "ray_losses.hpp"
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_ray_losses.h"

#include <vector>

namespace {

using namespace isr::ray_losses;
using isr::kReduce;

constexpr int kGroupRays = 4;                  // waves (rays) of a distortion workgroup
constexpr int kThreads = kGroupRays * kLanes;
constexpr unsigned kMaxGrid = 1u << 20;

__host__ __device__ constexpr int lds_stride(int P) { return (P + 3) & ~3; }      // floats of one LDS row

template <int RB, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void distortion_kernel(const float* __restrict__ lengths, const float* __restrict__ weights,
                                                              long long N, int P, long long items,
                                                              const float* __restrict__ upstream, double* __restrict__ ray_value,
                                                              float* __restrict__ ray_loss, float* __restrict__ dweights) {
  extern __shared__ __attribute__((aligned(16))) float distortion_lds[];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  const int K = P - 1, stride = lds_stride(P);
  float* ts = distortion_lds + (size_t)wave * 3 * stride;
  float* us = ts + stride;
  float* wsm = us + stride;
  double c = 0.0;
  if (BACKWARD) c = grad_scale(*upstream, N);
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long ray = item * kGroupRays + wave;
    const bool live = ray < N;
    const size_t base = (size_t)(live ? ray : N - 1) * P;
    const float* l = lengths + base;
    const float* w = weights + base;
    __syncthreads();                                     // the previous item's rows are done with
    const float l0 = l[0];
    float mx = depth(l0, l0);
    for (int k = lane; k < P; k += kLanes) {
      const float d = depth(l[k], l0);
      ts[k] = d;
      mx = max_step(mx, d);
      if (k < K) wsm[k] = w[k];
    }
    mx = isr::wave_reduce(mx, [](float m, float d) { return max_step(m, d); });      // max_step keeps a NaN; fmaxf would drop it
    for (int k = lane; k < P; k += kLanes) ts[k] = ts[k] / mx;      // the lane's own entries
    __syncthreads();
    for (int i = lane; i < K; i += kLanes) us[i] = midpoint(ts[i + 1], ts[i]);
    __syncthreads();
    double part = 0.0;
    for (int r0 = 0; r0 < K; r0 += kLanes * RB) {
      float ui[RB];
      double acc[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = r0 + r * kLanes + lane;
        ui[r] = i < K ? us[i] : 0.f;
        acc[r] = 0.0;
      }
#pragma unroll 4
      for (int j = 0; j < K; ++j) {
        const float uj = us[j];
        const double wj = (double)wsm[j];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = pair_step(acc[r], wj, ui[r], uj);
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int i = r0 + r * kLanes + lane;
        if (i < K) {
          const float delta = ts[i + 1] - ts[i];
          if (BACKWARD) {
            if (live) dweights[base + i] = weight_grad(c, wsm[i], acc[r], delta);
          } else {
            part += ray_term(wsm[i], acc[r], delta);
          }
        }
      }
    }
    if (BACKWARD) {
      if (live && lane == 0) dweights[base + K] = 0.f;
    } else {
      part = isr::wave_sum_down(part);                   // lane l < s: v[l] += v[l + s]
      if (live && lane == 0) {
        ray_value[ray] = part;
        if (ray_loss) ray_loss[ray] = isr::canonical((float)part);
      }
    }
  }
}

// the last step of a sum of the ray losses: the mean over its count (sum 0: count0, sum 1: count1)
struct MeanFinish {
  double count0, count1;
  __device__ float operator()(double S, int v) const { return mean_value(S, v == 0 ? count0 : count1); }
};

// (row_c, row_o) of 256 rays, summed by the tree: partial[g] = (sum of row_c, sum of row_o)
__global__ __launch_bounds__(kReduce) void render_rows_kernel(const float* __restrict__ rendered, const float* __restrict__ images,
                                                              const float* __restrict__ sils, const float* __restrict__ xys,
                                                              long long rows, int n, int F, int H, int W, double s,
                                                              double* __restrict__ partial, MeanFinish finish,
                                                              float* __restrict__ result) {
  __shared__ double tree[2][kReduce];
  for (long long g = blockIdx.x; g * kReduce < rows; g += gridDim.x) {
    const long long row = g * kReduce + threadIdx.x;
    double rc = 0.0, ro = 0.0;
    if (row < rows) render_row(rendered, images, sils, xys, (size_t)row, n, F, H, W, s, &rc, &ro);
    __syncthreads();
    tree[0][threadIdx.x] = rc;
    tree[1][threadIdx.x] = ro;
    __syncthreads();
    isr::tree256<2>(tree);
    if (threadIdx.x < 2) {
      partial[g * 2 + threadIdx.x] = tree[threadIdx.x][0];
      if (rows <= kReduce) result[threadIdx.x] = finish(tree[threadIdx.x][0], (int)threadIdx.x);
    }
  }
}

__global__ __launch_bounds__(256) void render_backward_kernel(const float* __restrict__ rendered, const float* __restrict__ images,
                                                              const float* __restrict__ sils, const float* __restrict__ xys,
                                                              long long rows, int n, int F, int H, int W, double s, double count0,
                                                              double count1, const float* __restrict__ upstream,
                                                              float* __restrict__ drendered) {
  const double kc = (double)upstream[0] / count0, ko = (double)upstream[1] / count1;
  const long long total = rows * (F + 1);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long row = e / (F + 1);
    const int ch = (int)(e - row * (F + 1)), b = (int)(row / n);
    const long long pix = target_pixel(xys, (size_t)row, H, W);
    drendered[e] = huber_grad(rendered[e] - target_value(images, sils, b, H, W, F, pix, ch), s, ch < F ? kc : ko);
  }
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

unsigned grid_of(long long items) { return (unsigned)(items < (long long)kMaxGrid ? items : (long long)kMaxGrid); }

int check_distortion_call(const char* who, int64_t N, int P) {
  const char* wrong = check_distortion(N, P);
  ISR_REQUIRE(!wrong, "%s: %s (N %lld, P %d)", who, wrong, (long long)N, P);
  return ISR_OK;
}

int check_render_call(const char* who, int B, int n, int F, int H, int W, double s) {
  const char* wrong = check_render(B, n, F, H, W, s);
  ISR_REQUIRE(!wrong, "%s: %s (B %d, n %d, F %d, H %d, W %d, scaling %g)", who, wrong, B, n, F, H, W, s);
  return ISR_OK;
}

template <bool BACKWARD>
int launch_distortion(const float* lengths, const float* weights, long long N, int P, const float* upstream, double* ray_value,
                      float* ray_loss, float* dweights, hipStream_t st) {
  const long long items = ceil_div(N, kGroupRays);
  const size_t lds = (size_t)kGroupRays * 3 * lds_stride(P) * sizeof(float);      // 48 KB at P = 1024
  const int K = P - 1;
  if (K <= kLanes)
    distortion_kernel<1, BACKWARD><<<grid_of(items), kThreads, lds, st>>>(lengths, weights, N, P, items, upstream, ray_value, ray_loss, dweights);
  else if (K <= 2 * kLanes)
    distortion_kernel<2, BACKWARD><<<grid_of(items), kThreads, lds, st>>>(lengths, weights, N, P, items, upstream, ray_value, ray_loss, dweights);
  else
    distortion_kernel<4, BACKWARD><<<grid_of(items), kThreads, lds, st>>>(lengths, weights, N, P, items, upstream, ray_value, ray_loss, dweights);
  ISR_CHECK_LAUNCH("distortion_kernel");
  return ISR_OK;
}

}  // namespace

extern "C" int isr_ray_losses_geometry(int what) {
  switch (what) {
    case 0: return kGroupRays;
    case 1: return kLanes;
    case 2: return kReduce;
    case 3: return kMaxP;
    default: isr::set_error("isr_ray_losses_geometry: what = %d", what); return 0;
  }
}

extern "C" size_t isr_distortion_workspace_bytes(int64_t N, int P) {
  if (check_distortion_call("isr_distortion_workspace_bytes", N, P)) return 0;
  return isr::reduce_bytes(N, 1, nullptr);
}

extern "C" int isr_distortion_forward(const float* lengths, const float* weights, int64_t N, int P, float* ray_loss_or_null,
                                      float* loss, void* ws, size_t ws_bytes, isr_stream_t stream) {
  if (int rc = check_distortion_call("isr_distortion_forward", N, P)) return rc;
  ISR_REQUIRE(lengths && weights && loss, "isr_distortion_forward: null pointer");
  size_t second;
  const size_t need = isr::reduce_bytes(N, 1, &second);
  ISR_REQUIRE(ws && ws_bytes >= need, "isr_distortion_forward: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = isr::as_stream(stream);
  double* bufs[2] = {static_cast<double*>(ws), reinterpret_cast<double*>(static_cast<char*>(ws) + second)};
  if (int rc = launch_distortion<false>(lengths, weights, N, P, nullptr, bufs[0], ray_loss_or_null, nullptr, st)) return rc;
  return isr::reduce_levels<1>("distortion reduce_kernel", bufs[0], N, bufs, 1, MeanFinish{(double)N, (double)N}, loss, st);
}

extern "C" int isr_distortion_backward(const float* lengths, const float* weights, int64_t N, int P, const float* upstream,
                                       float* dweights, isr_stream_t stream) {
  if (int rc = check_distortion_call("isr_distortion_backward", N, P)) return rc;
  ISR_REQUIRE(lengths && weights && upstream && dweights, "isr_distortion_backward: null pointer");
  return launch_distortion<true>(lengths, weights, N, P, upstream, nullptr, nullptr, dweights, isr::as_stream(stream));
}

extern "C" int isr_distortion_forward_host(const float* lengths, const float* weights, int64_t N, int P, float* ray_loss_or_null,
                                           float* loss) {
  if (int rc = check_distortion_call("isr_distortion_forward_host", N, P)) return rc;
  ISR_REQUIRE(lengths && weights && loss, "isr_distortion_forward_host: null pointer");
  std::vector<double> value((size_t)N);
  double* v = value.data();
  isr::parallel_rows((long)N, 16, [=](long i) {
    v[i] = distortion_ray(lengths + (size_t)i * P, weights + (size_t)i * P, P);
    if (ray_loss_or_null) ray_loss_or_null[i] = isr::canonical((float)v[i]);
  });
  *loss = mean_value(isr::ordered_sum(v, N, v), (double)N);
  return ISR_OK;
}

extern "C" int isr_distortion_backward_host(const float* lengths, const float* weights, int64_t N, int P, const float* upstream,
                                            float* dweights) {
  if (int rc = check_distortion_call("isr_distortion_backward_host", N, P)) return rc;
  ISR_REQUIRE(lengths && weights && upstream && dweights, "isr_distortion_backward_host: null pointer");
  const double c = grad_scale(*upstream, N);
  isr::parallel_rows((long)N, 16, [=](long i) {
    distortion_ray_backward(lengths + (size_t)i * P, weights + (size_t)i * P, P, c, dweights + (size_t)i * P);
  });
  return ISR_OK;
}

extern "C" size_t isr_render_loss_workspace_bytes(int64_t B, int64_t n) {
  if (B < 1 || n < 1 || B > kMaxRays || n > kMaxRays || B * n > kMaxRays) {
    isr::set_error("isr_render_loss_workspace_bytes: B %lld, n %lld", (long long)B, (long long)n);
    return 0;
  }
  return isr::reduce_bytes(ceil_div(B * n, kReduce), 2, nullptr);
}

extern "C" int isr_render_loss_forward(const float* rendered, const float* target_images, const float* target_silhouettes,
                                       const float* xys, int B, int n, int F, int H, int W, double scaling, float* out, void* ws,
                                       size_t ws_bytes, isr_stream_t stream) {
  if (int rc = check_render_call("isr_render_loss_forward", B, n, F, H, W, scaling)) return rc;
  ISR_REQUIRE(rendered && target_images && target_silhouettes && xys && out, "isr_render_loss_forward: null pointer");
  const long long rows = (long long)B * n, L1 = ceil_div(rows, kReduce);
  size_t second;
  const size_t need = isr::reduce_bytes(L1, 2, &second);
  ISR_REQUIRE(ws && ws_bytes >= need, "isr_render_loss_forward: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = isr::as_stream(stream);
  double* bufs[2] = {static_cast<double*>(ws), reinterpret_cast<double*>(static_cast<char*>(ws) + second)};
  const double count0 = (double)rows * (double)F, count1 = (double)rows;
  render_rows_kernel<<<grid_of(L1), kReduce, 0, st>>>(rendered, target_images, target_silhouettes, xys, rows, n, F, H, W, scaling,
                                                      bufs[0], MeanFinish{count0, count1}, out);
  ISR_CHECK_LAUNCH("render_rows_kernel");
  if (rows <= kReduce) return ISR_OK;
  return isr::reduce_levels<2>("render loss reduce_kernel", bufs[0], L1, bufs, 1, MeanFinish{count0, count1}, out, st);
}

extern "C" int isr_render_loss_backward(const float* rendered, const float* target_images, const float* target_silhouettes,
                                        const float* xys, int B, int n, int F, int H, int W, double scaling, const float* upstream,
                                        float* drendered, isr_stream_t stream) {
  if (int rc = check_render_call("isr_render_loss_backward", B, n, F, H, W, scaling)) return rc;
  ISR_REQUIRE(rendered && target_images && target_silhouettes && xys && upstream && drendered,
              "isr_render_loss_backward: null pointer");
  const long long rows = (long long)B * n;
  render_backward_kernel<<<grid_of(ceil_div(rows * (F + 1), 256)), 256, 0, isr::as_stream(stream)>>>(
      rendered, target_images, target_silhouettes, xys, rows, n, F, H, W, scaling, (double)rows * (double)F, (double)rows, upstream,
      drendered);
  ISR_CHECK_LAUNCH("render_backward_kernel");
  return ISR_OK;
}

extern "C" int isr_render_loss_forward_host(const float* rendered, const float* target_images, const float* target_silhouettes,
                                            const float* xys, int B, int n, int F, int H, int W, double scaling, float* out) {
  if (int rc = check_render_call("isr_render_loss_forward_host", B, n, F, H, W, scaling)) return rc;
  ISR_REQUIRE(rendered && target_images && target_silhouettes && xys && out, "isr_render_loss_forward_host: null pointer");
  const long long rows = (long long)B * n;
  std::vector<double> rc((size_t)rows), ro((size_t)rows);
  double *pc = rc.data(), *po = ro.data();
  isr::parallel_rows((long)rows, 256, [=](long i) {
    render_row(rendered, target_images, target_silhouettes, xys, (size_t)i, n, F, H, W, scaling, pc + i, po + i);
  });
  out[0] = mean_value(isr::ordered_sum(pc, rows, pc), (double)rows * (double)F);
  out[1] = mean_value(isr::ordered_sum(po, rows, po), (double)rows);
  return ISR_OK;
}

extern "C" int isr_render_loss_backward_host(const float* rendered, const float* target_images, const float* target_silhouettes,
                                             const float* xys, int B, int n, int F, int H, int W, double scaling,
                                             const float* upstream, float* drendered) {
  if (int rc = check_render_call("isr_render_loss_backward_host", B, n, F, H, W, scaling)) return rc;
  ISR_REQUIRE(rendered && target_images && target_silhouettes && xys && upstream && drendered,
              "isr_render_loss_backward_host: null pointer");
  const long long rows = (long long)B * n;
  const double kc = (double)upstream[0] / ((double)rows * (double)F), ko = (double)upstream[1] / (double)rows;
  isr::parallel_rows((long)rows, 256, [=](long i) {
    render_row_backward(rendered, target_images, target_silhouettes, xys, (size_t)i, n, F, H, W, scaling, kc, ko, drendered);
  });
  return ISR_OK;
}
