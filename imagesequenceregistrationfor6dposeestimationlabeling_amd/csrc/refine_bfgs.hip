// refine_bfgs.hip — a16 with the optimiser on the device: refine_pose's scipy BFGS (pose_refine.py:93-101) for a block of
// crops, one reverse-communication state machine per item (bfgs_state.hpp), the host only enqueues and reads back.
//
// One round = two launches on the caller's stream:
//   refine_obj_live_kernel  the batched objective body (refine_obj.hpp) for the live items, grid (64, n_items); the
//                           item and its pose come from the device state, rows >= n_live exit at once;
//   bfgs_step_kernel        one block per live item: reduce_item sums the item's 64 partials in block order (the bits of
//                           isr_refine_objective), then one thread advances the item's BFGS, writes the next pose and
//                           appends the item to the next live list.
// The live count of round r is ctl[r % 3]: round r's step kernel counts the next list into ctl[(r+1) % 3] and clears
// ctl[(r+2) % 3], which no launch of rounds r and r+1 reads.  The host enqueues kChunk rounds, then reads the counters
// through one pinned async copy and a stream synchronise.  No cooperative launch, no grid barrier, no graph.
#include "bfgs_state.hpp"
#include "refine_obj.hpp"

namespace {

using isr_bfgs::State;

constexpr int kN = 6;          // the reference's 6-vector [0, 0, 0, t] (pose_refine.py:97-101)
constexpr int kChunk = 8;      // rounds enqueued per host read of the live count
constexpr int kCtl = 4;        // ctl[0..2]: live counts by round % 3; ctl[3]: rounds that had a live item

__device__ __forceinline__ void write_pose(const double* __restrict__ R, const double* t, double* __restrict__ Rt) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rt[4 * r + c] = R[3 * r + c];
    Rt[4 * r + 3] = t[r];
  }
}

__device__ __forceinline__ void write_result(const State* S, int item, int status, double* __restrict__ t_out,
                                             double* __restrict__ fun_out, int32_t* __restrict__ nit_out,
                                             int32_t* __restrict__ nfev_out, int32_t* __restrict__ status_out) {
  for (int j = 0; j < 3; ++j) t_out[3 * (size_t)item + j] = S->x[3 + j];
  fun_out[item] = S->nfev > 0 ? S->old_fval : __builtin_nan("");
  nit_out[item] = S->k;
  nfev_out[item] = S->nfev;
  status_out[item] = status;
}

__global__ void bfgs_init_kernel(int n_items, const double* __restrict__ R, const double* __restrict__ t0, double gtol,
                                 int maxiter, State* __restrict__ states, double* __restrict__ Rt_req,
                                 int32_t* __restrict__ live, int32_t* __restrict__ ctl, double* __restrict__ t_out,
                                 double* __restrict__ fun_out, int32_t* __restrict__ nit_out,
                                 int32_t* __restrict__ nfev_out, int32_t* __restrict__ status_out) {
  const int item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item == 0) {
    ctl[0] = n_items;
    ctl[1] = 0;
    ctl[2] = 0;
    ctl[3] = 0;
  }
  if (item >= n_items) return;
  State* S = states + item;
  const double x0[kN] = {0.0, 0.0, 0.0, t0[3 * (size_t)item], t0[3 * (size_t)item + 1], t0[3 * (size_t)item + 2]};
  isr_bfgs::bfgs_init(S, kN, x0, gtol, maxiter);
  write_pose(R + 9 * (size_t)item, S->xr + 3, Rt_req + 12 * (size_t)item);
  live[item] = item;
  write_result(S, item, isr_bfgs::kStatusRounds, t_out, fun_out, nit_out, nfev_out, status_out);
}

// The batched objective (refine_obj_batch_kernel's body) for the items of the live list.
template <int MODE>
__global__ __launch_bounds__(kThreads) void refine_obj_live_kernel(const float* __restrict__ X_all,
                                                                   const float* __restrict__ keys_all,
                                                                   const int32_t* __restrict__ offs, int n_img, int e,
                                                                   const float* __restrict__ qimgs,
                                                                   const float* __restrict__ denoms, int res,
                                                                   const double* __restrict__ Ks,
                                                                   const int32_t* __restrict__ item_img,
                                                                   const double* __restrict__ Rt_req,
                                                                   double* __restrict__ partial,
                                                                   const int32_t* __restrict__ live,
                                                                   const int32_t* __restrict__ ctl, int cur) {
  if ((int)blockIdx.y >= ctl[cur]) return;             // uniform per block
  const size_t item = live[blockIdx.y];
  batch_item<MODE>(X_all, keys_all, offs, n_img, e, qimgs, denoms, res, Ks, item_img[item], Rt_req + 12 * item,
                   partial + (item * kBlocks + blockIdx.x) * kAcc);
}

__global__ __launch_bounds__(64) void bfgs_step_kernel(const double* __restrict__ partial,
                                                       const int32_t* __restrict__ offs, int n_img,
                                                       const int32_t* __restrict__ item_img,
                                                       const double* __restrict__ R, State* __restrict__ states,
                                                       double* __restrict__ Rt_req, const int32_t* __restrict__ live_cur,
                                                       int32_t* __restrict__ live_next, int32_t* __restrict__ ctl, int cur,
                                                       double* __restrict__ t_out, double* __restrict__ fun_out,
                                                       int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                                       int32_t* __restrict__ status_out) {
  const int n_live = ctl[cur];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl[(cur + 2) % 3] = 0;
    if (n_live > 0) ctl[3] += 1;
  }
  if ((int)blockIdx.x >= n_live) return;               // uniform per block
  const int item = live_cur[blockIdx.x];
  const int img = item_img[item];
  const int N = (img < 0 || img >= n_img) ? 1 : offs[img + 1] - offs[img];
  __shared__ double o[4];
  reduce_item(partial + (size_t)item * kBlocks * kAcc, N, o, 4);
  __syncthreads();
  if (threadIdx.x != 0) return;
  State* S = states + item;
  if (S->phase == isr_bfgs::P_FINISHED) return;
  S->gl[0] = 0.0;                                      // RefineObjective.__call__: the rvec slots of the gradient are 0
  S->gl[1] = 0.0;
  S->gl[2] = 0.0;
  S->gl[3] = o[1];
  S->gl[4] = o[2];
  S->gl[5] = o[3];
  const int r = isr_bfgs::bfgs_step_gl(S, o[0]);
  if (r == isr_bfgs::kNeedEval) {
    write_pose(R + 9 * (size_t)item, S->xr + 3, Rt_req + 12 * (size_t)item);
    live_next[atomicAdd(&ctl[(cur + 1) % 3], 1)] = item;
    write_result(S, item, isr_bfgs::kStatusRounds, t_out, fun_out, nit_out, nfev_out, status_out);
  } else {
    write_result(S, item, S->status, t_out, fun_out, nit_out, nfev_out, status_out);
  }
}

struct BfgsWs {
  double* partial;
  State* states;
  double* Rt_req;
  int32_t* live[2];
  int32_t* ctl;
};

BfgsWs carve(void* ws, size_t ws_bytes, int n) {
  isr::Workspace w(ws, ws_bytes);
  BfgsWs p;
  p.partial = w.take<double>((size_t)n * kBlocks * kAcc);
  p.states = w.take<State>((size_t)n);
  p.Rt_req = w.take<double>((size_t)n * 12);
  p.live[0] = w.take<int32_t>((size_t)n);
  p.live[1] = w.take<int32_t>((size_t)n);
  p.ctl = w.take<int32_t>(kCtl);
  return p;
}

}  // namespace

extern "C" size_t isr_refine_bfgs_batch_workspace_bytes(int n_items) {
  if (n_items <= 0) return 0;
  isr::Workspace w(nullptr, 0);
  const size_t n = (size_t)n_items;
  w.take<double>(n * kBlocks * kAcc);
  w.take<State>(n);
  w.take<double>(n * 12);
  w.take<int32_t>(n);
  w.take<int32_t>(n);
  w.take<int32_t>(kCtl);
  return w.off + 256;
}

extern "C" int isr_refine_bfgs_batch(const float* X_all, const float* keys_all, const int32_t* offs_host,
                                     const int32_t* offs, int n_img, int e, const float* query_imgs,
                                     const float* denom_imgs, int res, int interpolation, const double* K,
                                     const int32_t* item_img, const double* R, const double* t0, int n_items, double gtol,
                                     int maxiter, int max_rounds, double* t_out, double* fun_out, int32_t* nit_out,
                                     int32_t* nfev_out, int32_t* status_out, int32_t* stats_host, void* ws,
                                     size_t ws_bytes, isr_stream_t stream_) {
  ISR_REQUIRE(n_items >= 0 && n_items <= 65535, "isr_refine_bfgs_batch: n_items=%d (0 .. 65535)", n_items);
  ISR_REQUIRE(interpolation >= ISR_INTERP_BILINEAR && interpolation <= ISR_INTERP_BICUBIC,
              "isr_refine_bfgs_batch: interpolation mode %d", interpolation);
  ISR_REQUIRE(n_img > 0 && e > 0 && res > 0, "isr_refine_bfgs_batch: n_img=%d e=%d res=%d", n_img, e, res);
  ISR_REQUIRE(gtol >= 0.0 && maxiter >= 0 && max_rounds >= 0, "isr_refine_bfgs_batch: gtol=%g maxiter=%d max_rounds=%d",
              gtol, maxiter, max_rounds);
  ISR_REQUIRE(X_all && keys_all && offs_host && offs && query_imgs && denom_imgs && K, "isr_refine_bfgs_batch: null pointer");
  ISR_REQUIRE(n_items == 0 || (item_img && R && t0 && t_out && fun_out && nit_out && nfev_out && status_out),
              "isr_refine_bfgs_batch: null pointer");
  ISR_REQUIRE(offs_host[0] == 0, "isr_refine_bfgs_batch: offs[0]=%d (0)", offs_host[0]);
  for (int b = 0; b < n_img; ++b)
    ISR_REQUIRE(offs_host[b + 1] > offs_host[b], "isr_refine_bfgs_batch: image %d has N=%d visible points", b,
                offs_host[b + 1] - offs_host[b]);
  if (stats_host) stats_host[0] = stats_host[1] = 0;
  if (n_items == 0) return ISR_OK;
  const size_t need = isr_refine_bfgs_batch_workspace_bytes(n_items);
  if (!ws || ws_bytes < need) {
    isr::set_error("isr_refine_bfgs_batch: workspace %zu < %zu", ws_bytes, need);
    return ISR_ERR_WORKSPACE;
  }
  static thread_local int32_t* pinned = nullptr;     // the live counts' read-back, one small buffer per host thread
  if (!pinned) ISR_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&pinned), sizeof(int32_t) * kCtl, hipHostMallocDefault));
  hipStream_t stream = isr::as_stream(stream_);
  const BfgsWs p = carve(ws, ws_bytes, n_items);
  bfgs_init_kernel<<<(n_items + 63) / 64, 64, 0, stream>>>(n_items, R, t0, gtol, maxiter, p.states, p.Rt_req, p.live[0],
                                                         p.ctl, t_out, fun_out, nit_out, nfev_out, status_out);
  ISR_CHECK_LAUNCH("device BFGS init");
  int launches = 1, rounds = 0;
  pinned[3] = 0;
  const dim3 grid(kBlocks, n_items);
  while (rounds < max_rounds) {
    const int chunk = max_rounds - rounds < kChunk ? max_rounds - rounds : kChunk;
    for (int c = 0; c < chunk; ++c, ++rounds) {
      const int cur = rounds % 3;
      const int32_t* live_cur = p.live[rounds & 1];
      int32_t* live_next = p.live[(rounds + 1) & 1];
      if (interpolation == ISR_INTERP_NEAREST)
        refine_obj_live_kernel<1><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs,
                                                                 res, K, item_img, p.Rt_req, p.partial, live_cur, p.ctl, cur);
      else if (interpolation == ISR_INTERP_BICUBIC)
        refine_obj_live_kernel<2><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs,
                                                                 res, K, item_img, p.Rt_req, p.partial, live_cur, p.ctl, cur);
      else
        refine_obj_live_kernel<0><<<grid, kThreads, 0, stream>>>(X_all, keys_all, offs, n_img, e, query_imgs, denom_imgs,
                                                                 res, K, item_img, p.Rt_req, p.partial, live_cur, p.ctl, cur);
      bfgs_step_kernel<<<n_items, 64, 0, stream>>>(p.partial, offs, n_img, item_img, R, p.states, p.Rt_req, live_cur,
                                                   live_next, p.ctl, cur, t_out, fun_out, nit_out, nfev_out, status_out);
      ISR_CHECK_LAUNCH("device BFGS round");
      launches += 2;
    }
    ISR_CHECK_HIP(hipMemcpyAsync(pinned, p.ctl, sizeof(int32_t) * kCtl, hipMemcpyDeviceToHost, stream));
    ISR_CHECK_HIP(hipStreamSynchronize(stream));
    if (pinned[rounds % 3] == 0) break;
  }
  if (stats_host) {
    stats_host[0] = pinned[3];
    stats_host[1] = launches;
  }
  return ISR_OK;
}

// ---- the same state machine as host code: the CPU tests and the GPU exactness test drive exactly what the kernel runs.

extern "C" size_t isr_bfgs_state_bytes(void) { return sizeof(State); }

extern "C" int isr_bfgs_host_init(void* state, size_t state_bytes, int n, const double* x0, double gtol, int maxiter,
                                  double* x_next) {
  ISR_REQUIRE(state && x0 && x_next, "isr_bfgs_host_init: null pointer");
  ISR_REQUIRE(state_bytes >= sizeof(State), "isr_bfgs_host_init: state %zu < %zu bytes", state_bytes, sizeof(State));
  ISR_REQUIRE(n >= 1 && n <= isr_bfgs::kMaxN, "isr_bfgs_host_init: n=%d (1 .. %d)", n, isr_bfgs::kMaxN);
  ISR_REQUIRE(gtol >= 0.0 && maxiter >= 0, "isr_bfgs_host_init: gtol=%g maxiter=%d", gtol, maxiter);
  State* S = static_cast<State*>(state);
  isr_bfgs::bfgs_init(S, n, x0, gtol, maxiter);
  for (int i = 0; i < n; ++i) x_next[i] = S->xr[i];
  return ISR_OK;
}

// info (5 i32) = { done, status, nit, nfev, wolfe2 fallbacks }.  x_next: the next point to evaluate, or the result's x
// when done; fun (nullable): the current fval.
extern "C" int isr_bfgs_host_step(void* state, double f, const double* g, double* x_next, double* fun, int32_t* info) {
  ISR_REQUIRE(state && g && x_next && info, "isr_bfgs_host_step: null pointer");
  State* S = static_cast<State*>(state);
  ISR_REQUIRE(S->n >= 1 && S->n <= isr_bfgs::kMaxN, "isr_bfgs_host_step: state not initialised (n=%d)", S->n);
  const int r = isr_bfgs::bfgs_step(S, f, g);
  const bool done = r == isr_bfgs::kDone;
  for (int i = 0; i < S->n; ++i) x_next[i] = done ? S->x[i] : S->xr[i];
  if (fun) *fun = S->old_fval;
  info[0] = done ? 1 : 0;
  info[1] = done ? S->status : isr_bfgs::kStatusRounds;
  info[2] = S->k;
  info[3] = S->nfev;
  info[4] = S->n_wolfe2;
  return ISR_OK;
}
