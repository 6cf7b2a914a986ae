// refine_pose.hip — a16: the objective of refine_pose() (pose_refine.py:58-91) and its gradient.
//
//   p_img  = (K_crop [R|t]) X,  p = p_img[:2] / p_img[2]
//   score  = -( mean_i <keys_i, bilinear(query_img, p_i)> - mean_i bilinear(denom_img, p_i) ) / 2
// with F.grid_sample(align_corners=False, padding_mode='border', mode='bilinear') on
// p_norm = (p + 0.5) * 2 / res - 1, i.e. the sample position in pixel units is p itself (pixel
// centres at integers) clamped to [0, res-1].  The reference differentiates this with autograd and
// a cv2.Rodrigues round trip; only the translation is live there (pose_refine.py:73-76 builds R from
// a constant), so the analytic gradient the reference-shaped entry returns is d score / d t.
// isr_refine_objective_full adds d score / d R (9, row-major: sum_i g_i X_i^T with g_i the gradient with
// respect to the camera-frame point) for the evidently intended variant that also optimises the rotation
// (the caller chains it with the Rodrigues Jacobian).
// One thread per visible surface point, f64 accumulation, fixed-shape tree reduction.
#include "refine_obj.hpp"

namespace {

template <int MODE>
__global__ __launch_bounds__(kThreads) void refine_obj_taps_kernel(const float* __restrict__ X, const float* __restrict__ keys,
                                                                   int N, int e, const float* __restrict__ qimg,
                                                                   const float* __restrict__ denom, int res, P34 P,
                                                                   double* __restrict__ partial) {
  block_objective<MODE>(X, keys, N, e, qimg, denom, res, P, partial + (size_t)blockIdx.x * kAcc);
}

__global__ __launch_bounds__(kThreads) void refine_obj_kernel(const float* __restrict__ X, const float* __restrict__ keys,
                                                              int N, int e, const float* __restrict__ qimg,
                                                              const float* __restrict__ denom, int res, P34 P,
                                                              double* __restrict__ partial) {
  block_objective<0>(X, keys, N, e, qimg, denom, res, P, partial + (size_t)blockIdx.x * kAcc);
}

__global__ void refine_obj_reduce_kernel(const double* __restrict__ partial, int N, double* __restrict__ out, int nout) {
  reduce_item(partial, N, out, nout);
}

// ---- batched: item = blockIdx.y evaluates image item_img[item] at pose Rt[item]; the same grid stride, the same block
// reduction and the same reduce order per item as a single-item launch, so every row has the single entry's bits.
// An item whose image index is out of range gets NaN partials (no read beyond the arrays), hence a NaN row.
template <int MODE>
__global__ __launch_bounds__(kThreads) void refine_obj_batch_kernel(const float* __restrict__ X_all,
                                                                    const float* __restrict__ keys_all,
                                                                    const int32_t* __restrict__ offs, int n_img, int e,
                                                                    const float* __restrict__ qimgs,
                                                                    const float* __restrict__ denoms, int res,
                                                                    const double* __restrict__ Ks,
                                                                    const int32_t* __restrict__ item_img,
                                                                    const double* __restrict__ Rts,
                                                                    double* __restrict__ partial) {
  const size_t item = blockIdx.y;
  batch_item<MODE>(X_all, keys_all, offs, n_img, e, qimgs, denoms, res, Ks, item_img[item], Rts + 12 * item,
                   partial + (item * kBlocks + blockIdx.x) * kAcc);
}

__global__ void refine_obj_batch_reduce_kernel(const double* __restrict__ partial, const int32_t* __restrict__ offs, int n_img,
                                               const int32_t* __restrict__ item_img, double* __restrict__ out, int nout) {
  const size_t item = blockIdx.x;
  const int img = item_img[item];
  const int N = (img < 0 || img >= n_img) ? 1 : offs[img + 1] - offs[img];
  reduce_item(partial + item * kBlocks * kAcc, N, out + item * nout, nout);
}

}  // namespace

static int refine_impl(const float* X, const float* keys, int N, int e, const float* query_img, const float* denom_img,
                       int res, int mode, const double* Kcrop, const double* Rt, double* out, int nout, void* ws,
                       size_t ws_bytes, isr_stream_t stream_) {
  ISR_REQUIRE(X && keys && query_img && denom_img && Kcrop && Rt && out, "isr_refine_objective: null pointer");
  ISR_REQUIRE(N > 0 && e > 0 && res > 0, "isr_refine_objective: N=%d e=%d res=%d", N, e, res);
  ISR_REQUIRE(mode >= ISR_INTERP_BILINEAR && mode <= ISR_INTERP_BICUBIC, "isr_refine_objective: interpolation mode %d", mode);
  const size_t need = sizeof(double) * kBlocks * kAcc + 256;
  if (!ws || ws_bytes < need) {
    isr::set_error("isr_refine_objective: workspace %zu < %zu", ws_bytes, need);
    return ISR_ERR_WORKSPACE;
  }
  P34 P;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      P.p[4 * r + c] = Kcrop[3 * r] * Rt[c] + Kcrop[3 * r + 1] * Rt[4 + c] + Kcrop[3 * r + 2] * Rt[8 + c];
  for (int i = 0; i < 9; ++i) P.k[i] = Kcrop[i];
  hipStream_t stream = isr::as_stream(stream_);
  isr::Workspace w(ws, ws_bytes);
  double* partial = w.take<double>((size_t)kBlocks * kAcc);
  if (mode == ISR_INTERP_NEAREST)
    refine_obj_taps_kernel<1><<<kBlocks, kThreads, 0, stream>>>(X, keys, N, e, query_img, denom_img, res, P, partial);
  else if (mode == ISR_INTERP_BICUBIC)
    refine_obj_taps_kernel<2><<<kBlocks, kThreads, 0, stream>>>(X, keys, N, e, query_img, denom_img, res, P, partial);
  else
    refine_obj_kernel<<<kBlocks, kThreads, 0, stream>>>(X, keys, N, e, query_img, denom_img, res, P, partial);
  refine_obj_reduce_kernel<<<1, 64, 0, stream>>>(partial, N, out, nout);
  ISR_CHECK_LAUNCH("refine objective kernels");
  return ISR_OK;
}

extern "C" int isr_refine_objective(const float* X, const float* keys, int N, int e, const float* query_img,
                                    const float* denom_img, int res, int interpolation, const double* Kcrop,
                                    const double* Rt, double* out4, void* ws, size_t ws_bytes, isr_stream_t stream) {
  return refine_impl(X, keys, N, e, query_img, denom_img, res, interpolation, Kcrop, Rt, out4, 4, ws, ws_bytes, stream);
}

extern "C" int isr_refine_objective_full(const float* X, const float* keys, int N, int e, const float* query_img,
                                         const float* denom_img, int res, int interpolation, const double* Kcrop,
                                         const double* Rt, double* out13, void* ws, size_t ws_bytes, isr_stream_t stream) {
  return refine_impl(X, keys, N, e, query_img, denom_img, res, interpolation, Kcrop, Rt, out13, 13, ws, ws_bytes, stream);
}

extern "C" size_t isr_refine_objective_batch_workspace_bytes(int n_items) {
  if (n_items <= 0) return 0;
  return sizeof(double) * kBlocks * kAcc * (size_t)n_items + 256;
}

extern "C" int isr_refine_objective_batch(const float* X_all, const float* keys_all, const int32_t* offs_host,
                                          const int32_t* offs, int n_img, int e, const float* query_imgs,
                                          const float* denom_imgs, int res, int interpolation, const double* K,
                                          const int32_t* item_img, const double* Rt, int n_items, double* out, int nout,
                                          void* ws, size_t ws_bytes, isr_stream_t stream_) {
  ISR_REQUIRE(n_items >= 0 && n_items <= 65535, "isr_refine_objective_batch: n_items=%d (0 .. 65535)", n_items);
  ISR_REQUIRE(nout == 4 || nout == 13, "isr_refine_objective_batch: nout=%d (4 or 13)", nout);
  ISR_REQUIRE(interpolation >= ISR_INTERP_BILINEAR && interpolation <= ISR_INTERP_BICUBIC,
              "isr_refine_objective_batch: interpolation mode %d", interpolation);
  ISR_REQUIRE(n_img > 0 && e > 0 && res > 0, "isr_refine_objective_batch: n_img=%d e=%d res=%d", n_img, e, res);
  ISR_REQUIRE(X_all && keys_all && offs_host && offs && query_imgs && denom_imgs && K, "isr_refine_objective_batch: null pointer");
  ISR_REQUIRE(n_items == 0 || (item_img && Rt && out), "isr_refine_objective_batch: null pointer");
  ISR_REQUIRE(offs_host[0] == 0, "isr_refine_objective_batch: offs[0]=%d (0)", offs_host[0]);
  for (int b = 0; b < n_img; ++b)
    ISR_REQUIRE(offs_host[b + 1] > offs_host[b], "isr_refine_objective_batch: image %d has N=%d visible points", b,
                offs_host[b + 1] - offs_host[b]);
  if (n_items == 0) return ISR_OK;
  const size_t need = isr_refine_objective_batch_workspace_bytes(n_items);
  if (!ws || ws_bytes < need) {
    isr::set_error("isr_refine_objective_batch: workspace %zu < %zu", ws_bytes, need);
    return ISR_ERR_WORKSPACE;
  }
  hipStream_t stream = isr::as_stream(stream_);
  isr::Workspace w(ws, ws_bytes);
  double* partial = w.take<double>((size_t)n_items * kBlocks * kAcc);
  const dim3 grid(kBlocks, n_items);
  if (interpolation == ISR_INTERP_NEAREST)
    refine_obj_batch_kernel<1><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs, res, K,
                                                              item_img, Rt, partial);
  else if (interpolation == ISR_INTERP_BICUBIC)
    refine_obj_batch_kernel<2><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs, res, K,
                                                              item_img, Rt, partial);
  else
    refine_obj_batch_kernel<0><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs, res, K,
                                                              item_img, Rt, partial);
  refine_obj_batch_reduce_kernel<<<n_items, 64, 0, stream>>>(partial, offs, n_img, item_img, out, nout);
  ISR_CHECK_LAUNCH("batched refine objective kernels");
  return ISR_OK;
}
