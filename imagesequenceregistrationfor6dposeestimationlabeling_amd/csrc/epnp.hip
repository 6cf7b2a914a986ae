// epnp.hip — EPnP on gfx950: cv2.solvePnPRansac's final solve (solvePnP(SOLVEPNP_EPNP) over the winner's consensus set),
// for pnp(final="epnp") (isr_pnp_ransac_batch, final_mode ISR_FINAL_EPNP) and on its own (isr_epnp_batch).  The algorithm, every choice in it and
// the reduction shape are stated in csrc/epnp.hpp; isr_epnp_host runs the same header as host code.
//
// Ten launches per chain, the image on blockIdx.z (passes) or blockIdx.x (dense steps), M and the status read on the device:
//   pass 1   sum p, n                       (kEpnpBlocks x 256 threads per image)       solve 1  centroid
//   pass 2   sum (p - c0)(p - c0)^T                                                      solve 2  control points, CC+
//   pass 3   alpha, the 40 M^T M sums                                                    solve 3  12 x 12 Jacobi (one wave, LDS),
//                                                                                                 betas, ccs, sign rule
//   pass 4   sum pc, sum pc (p - c0)^T      (3 candidates)                               solve 4  Procrustes (3 x 3 SVD)
//   pass 5   sum of reprojection errors     (3 candidates)                               solve 5  pick, outputs
// A pass writes one partial per (image, block) — a per-thread loop, the shuffle-down tree, the four waves in order — and the
// next dense step sums them in block order: the shape csrc/epnp.hpp replays on the host.  No device-scope fences, no atomics.
// The dense steps run in one 64-lane workgroup per image with every matrix in LDS: lanes share the Jacobi rotations, one lane
// runs the small serial steps.
#include "block_prims.hpp"
#include "isr_common.hpp"
#include "epnp.hpp"

namespace {

using namespace isr_epnp;

constexpr int kSolveThreads = 64;
constexpr int kKBatch = 16;   // cameras per upload launch (kernel-argument space)

struct BlockSync {
  __device__ void operator()() const { __syncthreads(); }
};

struct KBatch {
  double k[kKBatch][9];
};

__global__ void epnp_set_k_kernel(KBatch kb, int nb, double* __restrict__ dst) {
  const int b = threadIdx.x;
  if (b >= nb) return;
  for (int i = 0; i < 9; ++i) dst[9 * b + i] = kb.k[b][i];
}

__device__ __forceinline__ bool image_live(const int32_t* status_dev, int b) { return !status_dev || status_dev[b] != 0; }

template <int P>
__global__ __launch_bounds__(kEpnpThreads) void epnp_pass_kernel(
    const float* __restrict__ p3d, const float* __restrict__ p2d, const int32_t* __restrict__ M_dev, int M_cap,
    const uint32_t* __restrict__ mask, int mask_words, const double* __restrict__ K_dev, int K_stride,
    const int32_t* __restrict__ status_dev, const double* __restrict__ state, double* __restrict__ partial) {
  constexpr int NA = pass_acc(P);
  __shared__ double red[kEpnpThreads / 64][NA];
  const int b = blockIdx.z;
  if (!image_live(status_dev, b)) return;                 // block-uniform
  const double* st = state + (size_t)b * kStateD;
  if (P != kP1 && !(st[kN] >= 4.0)) return;               // fewer than 4 points: nothing to solve
  p3d += (size_t)b * M_cap * 3; p2d += (size_t)b * M_cap * 2;
  if (mask) mask += (size_t)b * mask_words;
  const Intr K = intr_of(K_dev + (size_t)b * K_stride);
  const int M = min(M_dev[b], M_cap);
  double a[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) a[k] = 0.0;
  for (int m = blockIdx.x * kEpnpThreads + threadIdx.x; m < M; m += kEpnpBlocks * kEpnpThreads) {
    if (!masked(mask, m)) continue;
    const double x = p3d[3 * (size_t)m], y = p3d[3 * (size_t)m + 1], z = p3d[3 * (size_t)m + 2];
    if constexpr (P == kP1) {
      p1_point(a, x, y, z);
    } else if constexpr (P == kP2) {
      p2_point(a, st, x, y, z);
    } else if constexpr (P == kP3) {
      p3_point(a, st, K, x, y, z, p2d[2 * (size_t)m], p2d[2 * (size_t)m + 1]);
    } else if constexpr (P == kP4) {
      p4_point(a, st, x, y, z);
    } else {
      p5_point(a, st, K, x, y, z, p2d[2 * (size_t)m], p2d[2 * (size_t)m + 1]);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    const double s = isr::wave_sum_down(a[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NA)
    partial[((size_t)b * kEpnpBlocks + blockIdx.x) * kMaxAcc + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// The dense step after pass S, one 64-lane workgroup per image (blockIdx.x): the state in LDS, the pass's sums in block
// order, then the step; the state goes back to memory.  S = kP5 also writes the outputs.
template <int S>
__global__ __launch_bounds__(kSolveThreads) void epnp_solve_kernel(
    const float* __restrict__ p3d, const int32_t* __restrict__ M_dev, int M_cap, const uint32_t* __restrict__ mask,
    int mask_words, const double* __restrict__ K_dev, int K_stride, int32_t* __restrict__ status_dev,
    double* __restrict__ state, const double* __restrict__ partial, int nblk, double* __restrict__ pose_dev,
    double* __restrict__ Rt_out, double* __restrict__ err_out, int32_t* __restrict__ chosen_out) {
  constexpr int NA = pass_acc(S);
  __shared__ double st[kStateD];
  __shared__ double sum[kMaxAcc];
  __shared__ double A[144], V[144], vn[48];
  __shared__ double sh[200];
  __shared__ int ish[12];
  __shared__ int first;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!image_live(status_dev, b)) return;
  double* gst = state + (size_t)b * kStateD;
  for (int k = lane; k < kStateD; k += kSolveThreads) st[k] = (S == kP1) ? 0.0 : gst[k];
  if (lane < NA) {
    double s = 0.0;
    for (int blk = 0; blk < nblk; ++blk) s += partial[((size_t)b * kEpnpBlocks + blk) * kMaxAcc + lane];
    sum[lane] = s;
  }
  __syncthreads();
  if constexpr (S == kP1) {
    if (lane == 0) centroid(st, sum);
  } else {
    if (!(st[kN] >= 4.0)) {            // fewer than 4 points: NaN pose, chosen 0 (the chain's status >= 4 excludes this)
      if (S == kP5 && lane < 12) {
        if (Rt_out) Rt_out[(size_t)b * 12 + lane] = NAN;
        if (err_out && lane < 3) err_out[(size_t)b * 3 + lane] = NAN;
        if (chosen_out && lane == 0) chosen_out[b] = 0;
        if (status_dev && lane == 0) status_dev[b] = 0;
      }
      return;
    }
    if constexpr (S == kP2) {
      if (lane == 0) control_points(st, sum, sh, ish);
    } else if constexpr (S == kP3) {
      build_mtm(sum, intr_of(K_dev + (size_t)b * K_stride), A, lane, kSolveThreads);
      __syncthreads();
      jacobi(A, V, 12, lane, kSolveThreads, BlockSync{});
      if (lane == 0) eig_order(A, 12, false, ish);
      __syncthreads();
      if (lane < 48) vn[lane] = V[(lane % 12) * 12 + ish[lane / 12]];
      // the first masked point (sign rule): the lowest set bit below M
      const int M = min(M_dev[b], M_cap);
      if (lane == 0) first = mask ? -1 : 0;
      __syncthreads();
      if (mask) {
        const uint32_t* mk = mask + (size_t)b * mask_words;
        const int W = (M + 31) / 32;
        for (int w0 = 0; w0 < W; w0 += kSolveThreads) {
          const int w = w0 + lane;
          uint32_t bits = (w < W) ? mk[w] : 0u;
          if (w == W - 1 && (M & 31)) bits &= (1u << (M & 31)) - 1u;
          const unsigned long long any = __ballot(bits != 0u);
          if (any) {
            if (lane == __ffsll((long long)any) - 1) first = w * 32 + __ffs(bits) - 1;
            break;
          }
        }
      }
      __syncthreads();
      if (lane == 0) {
        candidates(st, vn, sh);
        const float* p = p3d + (size_t)b * M_cap * 3 + 3 * (size_t)first;
        sign_rule(st, p[0], p[1], p[2]);
      }
    } else if constexpr (S == kP4) {
      if (lane == 0)
        for (int c = 0; c < 3; ++c) procrustes(st, c, sum + 12 * c, sh, ish);
    } else {
      if (lane == 0) {
        double* Rt = sh;           // LDS: no runtime-indexed arrays in registers
        double* err = sh + 12;
        const int ch = pick(st, sum, Rt, err);
        bool fin = true;
        for (int k = 0; k < 12; ++k) fin = fin && (Rt[k] - Rt[k] == 0.0);
        for (int k = 0; k < 12; ++k) {
          if (Rt_out) Rt_out[(size_t)b * 12 + k] = Rt[k];
          if (pose_dev && fin) pose_dev[(size_t)b * 12 + k] = Rt[k];
        }
        if (err_out)
          for (int k = 0; k < 3; ++k) err_out[(size_t)b * 3 + k] = err[k];
        if (chosen_out) chosen_out[b] = ch;
        if (status_dev && !fin) status_dev[b] = 0;   // a non-finite EPnP pose: no pose (cv2 would return it)
      }
    }
  }
  __syncthreads();
  for (int k = lane; k < kStateD; k += kSolveThreads) gst[k] = st[k];
}

struct EpnpWs {
  double* partial;   // B x kEpnpBlocks x kMaxAcc
  double* state;     // B x kStateD
  double* K;         // B x 9 (isr_epnp_batch's cameras)
};

size_t carve_epnp(isr::Workspace& w, int B, EpnpWs* o) {
  o->partial = w.take<double>((size_t)B * kEpnpBlocks * kMaxAcc);
  o->state = w.take<double>((size_t)B * kStateD);
  o->K = w.take<double>((size_t)B * 9);
  return w.off;
}

}  // namespace

namespace isr {

size_t epnp_ws_bytes(int B) {
  Workspace w(nullptr, 0);
  EpnpWs o;
  return carve_epnp(w, B, &o) + 256;
}

int epnp_enqueue(const float* p3d, const float* p2d, const int32_t* M_dev, int M_cap, int B, const uint32_t* mask,
                 int mask_words, const double* K_dev, int K_stride, int32_t* status_dev, double* pose_dev, double* Rt_out,
                 double* err_out, int32_t* chosen_out, void* ws, hipStream_t stream) {
  Workspace w(ws, epnp_ws_bytes(B));
  EpnpWs e;
  carve_epnp(w, B, &e);
  const int nblk = (M_cap + kEpnpThreads - 1) / kEpnpThreads < kEpnpBlocks ? (M_cap + kEpnpThreads - 1) / kEpnpThreads
                                                                            : kEpnpBlocks;
  const dim3 pg(nblk, 1, B);
#define ISR_EPNP_STEP(P)                                                                                                   \
  epnp_pass_kernel<P><<<pg, kEpnpThreads, 0, stream>>>(p3d, p2d, M_dev, M_cap, mask, mask_words, K_dev, K_stride,        \
                                                       status_dev, e.state, e.partial);                                   \
  epnp_solve_kernel<P><<<B, kSolveThreads, 0, stream>>>(p3d, M_dev, M_cap, mask, mask_words, K_dev, K_stride, status_dev, \
                                                        e.state, e.partial, nblk, pose_dev, Rt_out, err_out, chosen_out)
  ISR_EPNP_STEP(kP1);
  ISR_EPNP_STEP(kP2);
  ISR_EPNP_STEP(kP3);
  ISR_EPNP_STEP(kP4);
  ISR_EPNP_STEP(kP5);
#undef ISR_EPNP_STEP
  ISR_CHECK_LAUNCH("epnp kernels");
  return ISR_OK;
}

}  // namespace isr

extern "C" size_t isr_epnp_batch_workspace_bytes(int M_cap, int B) {
  if (M_cap <= 0 || B <= 0) return 0;
  return isr::epnp_ws_bytes(B);
}

extern "C" int isr_epnp_batch(const float* p3d, const float* p2d, const int32_t* M_dev, int M_cap, int B, const uint32_t* mask,
                              const double* Kcams, double* Rt_out, double* rep_err_out, int32_t* chosen_out, void* ws,
                              size_t ws_bytes, isr_stream_t stream_) {
  ISR_REQUIRE(p3d && p2d && M_dev && Kcams && Rt_out && rep_err_out && chosen_out, "isr_epnp_batch: null pointer");
  ISR_REQUIRE(M_cap > 0 && B > 0, "isr_epnp_batch: M_cap=%d B=%d", M_cap, B);
  if (!ws || ws_bytes < isr_epnp_batch_workspace_bytes(M_cap, B)) {
    isr::set_error("isr_epnp_batch: workspace %zu < %zu", ws_bytes, isr_epnp_batch_workspace_bytes(M_cap, B));
    return ISR_ERR_WORKSPACE;
  }
  hipStream_t stream = isr::as_stream(stream_);
  isr::Workspace w(ws, ws_bytes);
  EpnpWs e;
  carve_epnp(w, B, &e);
  for (int b0 = 0; b0 < B; b0 += kKBatch) {
    const int nb = (B - b0 < kKBatch) ? B - b0 : kKBatch;
    KBatch kb;
    for (int b = 0; b < kKBatch; ++b)
      for (int i = 0; i < 9; ++i) kb.k[b][i] = Kcams[9 * (size_t)(b0 + (b < nb ? b : 0)) + i];
    epnp_set_k_kernel<<<1, kKBatch, 0, stream>>>(kb, nb, e.K + 9 * (size_t)b0);
  }
  ISR_CHECK_LAUNCH("epnp_set_k_kernel");
  return isr::epnp_enqueue(p3d, p2d, M_dev, M_cap, B, mask, (M_cap + 31) / 32, e.K, 9, nullptr, nullptr, Rt_out, rep_err_out,
                           chosen_out, ws, stream);
}

// The same header as host code, the device's reduction shape replayed (csrc/epnp.hpp): the exactness reference.
extern "C" int isr_epnp_host(const float* p3d, const float* p2d, const uint32_t* mask, int M, const double* Kcam, double* Rt,
                             double* rep_err, int32_t* chosen) {
  ISR_REQUIRE(p3d && p2d && Kcam && Rt && rep_err && chosen, "isr_epnp_host: null pointer");
  ISR_REQUIRE(M >= 0, "isr_epnp_host: M=%d", M);
  double st[kStateD] = {};
  double sum[kMaxAcc];
  double A[144], V[144], vn[48], sh[200];
  int ish[12];
  const Intr K = intr_of(Kcam);
  auto P = [&](int m, int k) { return (double)p3d[3 * (size_t)m + k]; };
  auto Q = [&](int m, int k) { return (double)p2d[2 * (size_t)m + k]; };
  host_pass<4>(M, mask, [&](double (&a)[4], int m) { p1_point(a, P(m, 0), P(m, 1), P(m, 2)); }, sum);
  centroid(st, sum);
  ISR_REQUIRE(st[kN] >= 4.0, "isr_epnp_host: %d masked points (EPnP needs 4)", (int)st[kN]);
  host_pass<6>(M, mask, [&](double (&a)[6], int m) { p2_point(a, st, P(m, 0), P(m, 1), P(m, 2)); }, sum);
  control_points(st, sum, sh, ish);
  host_pass<40>(M, mask, [&](double (&a)[40], int m) { p3_point(a, st, K, P(m, 0), P(m, 1), P(m, 2), Q(m, 0), Q(m, 1)); }, sum);
  build_mtm(sum, K, A, 0, 1);
  jacobi(A, V, 12, 0, 1, NoSync{});
  eig_order(A, 12, false, ish);
  for (int e = 0; e < 48; ++e) vn[e] = V[(e % 12) * 12 + ish[e / 12]];
  int first = 0;
  while (!masked(mask, first)) ++first;
  candidates(st, vn, sh);
  sign_rule(st, P(first, 0), P(first, 1), P(first, 2));
  host_pass<36>(M, mask, [&](double (&a)[36], int m) { p4_point(a, st, P(m, 0), P(m, 1), P(m, 2)); }, sum);
  for (int c = 0; c < 3; ++c) procrustes(st, c, sum + 12 * c, sh, ish);
  host_pass<3>(M, mask, [&](double (&a)[3], int m) { p5_point(a, st, K, P(m, 0), P(m, 1), P(m, 2), Q(m, 0), Q(m, 1)); }, sum);
  *chosen = pick(st, sum, Rt, rep_err);
  return ISR_OK;
}

// The Jacobi stage on its own (host): a symmetric n x n (n <= 12) -> eigenvalues ascending, eigenvectors as columns.
extern "C" int isr_epnp_jacobi_host(const double* A_in, int n, double* evals, double* evecs) {
  ISR_REQUIRE(A_in && evals && evecs, "isr_epnp_jacobi_host: null pointer");
  ISR_REQUIRE(n >= 1 && n <= 12, "isr_epnp_jacobi_host: n=%d (1..12)", n);
  double A[144], V[144];
  int idx[12];
  for (int k = 0; k < n * n; ++k) A[k] = A_in[k];
  jacobi(A, V, n, 0, 1, NoSync{});
  eig_order(A, n, false, idx);
  for (int i = 0; i < n; ++i) {
    evals[i] = A[idx[i] * n + idx[i]];
    for (int r = 0; r < n; ++r) evecs[r * n + i] = V[r * n + idx[i]];
  }
  return ISR_OK;
}
