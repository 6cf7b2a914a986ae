// icp_loop.hpp — K4: the ICP loop of csrc/nn_batched.hip, written once for its three entries (isr_icp_point_to_point, its
// batch, isr_icp_point_to_plane_batch).  Included by nn_batched.hip below launch_search, the way nn_grid.hpp is: one
// translation unit, so the searches are instantiated once.
//
// registration_icp(source, target, threshold, init, estimation) of icp.py:101-103, enqueued as max_iter + 1 evaluation passes
// with NO host round trip.  A pass is two launches: the search (nn_search_kernel<.., EXACT>: one packed (f32 d2 bits, index)
// minimum per source point, near ties flagged) and the estimator's pass kernel (icp_pass<Est>), in which every workgroup
//   resolve_flagged   decides its flagged points over ALL targets in f64,
//   take_winner       reads and re-arms its 256 packed slots,
//   Est::row          forms each point's terms (the estimator's: PointToPoint or PointToPlane below),
//   block_sums        reduces them in a fixed shape, delivers the block's sums and takes a ticket,
// and the LAST workgroup of the item to arrive (agent-scope fences order the block sums before the ticket)
//   reduce_blocks     adds the blocks in a fixed order, and
//   Est::finish       (thread 0) applies Open3D's stopping rule (|d fitness| < rel_fitness and |d rmse| < rel_rmse, or the
//                     iteration budget) and, if the loop continues, composes T <- dT T.
// A device flag per item turns its remaining launches into no-ops once the rule fires.  blockIdx.y is the problem (the single
// call is a grid of one): every per-problem pointer moves to the item's slice — source (src_item_stride floats apart, 0 =
// shared), packed / prev_idx / amb (Ns apart), block sums (gridDim.x rows apart), IcpState (own ticket), and what the
// estimator owns (to_item) — and the code is the single problem's, sum for sum: item b of a batch gives the single call's bits.
#pragma once
#include "../../include/isr_icp_plane.h"
#include "icp_plane.hpp"

namespace {

namespace ipl = isr::icp_plane;

struct IcpState {
  double prev_fit, prev_rmse;
  int32_t iter, done;
  int32_t ticket, pad;   // workgroups that have delivered their sums in the current pass
};
static_assert(sizeof(IcpState) == kIcpStateInts * sizeof(int32_t) && offsetof(IcpState, done) == 5 * sizeof(int32_t),
              "nn_search_kernel<.., ITEMS> steps from one item's done flag to the next by kIcpStateInts");

constexpr int kIcpLanes = 16;
static_assert(ipl::kLanes == kIcpLanes && ipl::kStateDoubles == ISR_ICP_PLANE_STATE_DOUBLES && ipl::kL2 == ISR_ICP_L2 &&
                  ipl::kHuber == ISR_ICP_HUBER && ipl::kTukey == ISR_ICP_TUKEY,
              "csrc/icp_plane.hpp, include/isr_icp_plane.h and the point-to-point loop disagree");

// ------------------------------------------------------------------------------- the pieces of a pass
// Near ties the search flagged (nn_search_kernel<.., EXACT>): the exact nearest neighbour over ALL targets in f64 — squared
// distance by the fma chain the rows use, lowest index on exact ties — decided by the whole workgroup and written back
// into the point's packed slot (one or two points per pass on 20 000-point clouds, in one or two workgroups).  T: the item's.
__device__ __forceinline__ void resolve_flagged(const double* __restrict__ T, const float* __restrict__ src,
                                                const float* __restrict__ tgt, int Nt, int Ns, int32_t* __restrict__ amb,
                                                unsigned long long* __restrict__ packed) {
  __shared__ int nflag, flist[kThreads];
  __shared__ double wd[4][kThreads / 64];
  __shared__ int wi[4][kThreads / 64];
  const int tid = threadIdx.x;
  const int qi = blockIdx.x * kThreads + tid;
  if (tid == 0) nflag = 0;
  __syncthreads();
  if (qi < Ns && amb[qi]) {
    amb[qi] = 0;
    flist[atomicAdd(&nflag, 1)] = qi;
  }
  __syncthreads();
  const int nf = nflag;                             // block-uniform
  // up to kRes flagged points per sweep over the targets: a target is loaded once and tried against each of them
  // (the sweep is bound by load latency — round 3's first version resolved one point per sweep, ~35 us each)
  constexpr int kRes = 4;
  for (int f0 = 0; f0 < nf; f0 += kRes) {
    double qx[kRes], qy[kRes], qz[kRes], bd[kRes];
    int bi[kRes];
#pragma unroll
    for (int k = 0; k < kRes; ++k) {
      const int pq = flist[min(f0 + k, nf - 1)];
      xform64(T, src[3 * (size_t)pq], src[3 * (size_t)pq + 1], src[3 * (size_t)pq + 2], qx[k], qy[k], qz[k]);
      bd[k] = __builtin_inf();
      bi[k] = 0x7fffffff;
    }
#pragma unroll 4
    for (int j = tid; j < Nt; j += kThreads) {
      const double tx = tgt[3 * (size_t)j], ty = tgt[3 * (size_t)j + 1], tz = tgt[3 * (size_t)j + 2];
#pragma unroll
      for (int k = 0; k < kRes; ++k) {
        const double ex = qx[k] - tx, ey = qy[k] - ty, ez = qz[k] - tz;
        const double s2 = fma(ez, ez, fma(ey, ey, ex * ex));
        if (s2 < bd[k]) { bd[k] = s2; bi[k] = j; }  // ascending j per thread: ties keep the lower index
      }
    }
#pragma unroll
    for (int k = 0; k < kRes; ++k) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd[k], off, 64);
        const int oi = __shfl_xor(bi[k], off, 64);
        if (od < bd[k] || (od == bd[k] && oi < bi[k])) { bd[k] = od; bi[k] = oi; }
      }
      if ((tid & 63) == 0) { wd[k][tid >> 6] = bd[k]; wi[k][tid >> 6] = bi[k]; }
    }
    __syncthreads();
    if (tid < kRes && f0 + tid < nf) {
      double d = wd[tid][0];
      int i = wi[tid][0];
      for (int w = 1; w < kThreads / 64; ++w)
        if (wd[tid][w] < d || (wd[tid][w] == d && wi[tid][w] < i)) { d = wd[tid][w]; i = wi[tid][w]; }
      packed[flist[f0 + tid]] = ((unsigned long long)__float_as_uint((float)d) << 32) | (unsigned int)i;
    }
    __syncthreads();
  }
}

// The search's winner for point qi (-1: none; else < Nt: the search posts indices of the target only); re-arms the slot
// for the next pass, which starts from this neighbour (prev_idx).
__device__ __forceinline__ int take_winner(unsigned long long* __restrict__ packed, int32_t* __restrict__ prev_idx, int qi) {
  const unsigned long long pk = packed[qi];
  packed[qi] = ~0ull;
  const int bi = pk != ~0ull ? (int)(unsigned int)pk : -1;
  prev_idx[qi] = bi;
  return bi;
}

// The workgroup's N sums (block_tree_sums, csrc/nn_batched.hip) into row blockIdx.x of part_sums, then a ticket: true in
// every thread of the item's last workgroup to arrive, which then sees every block's sums.
template <int N>
__device__ __forceinline__ bool block_sums(const double (&v)[N], double* __restrict__ part_sums, int32_t* ticket) {
  __shared__ int last;
  const int tid = threadIdx.x;
  block_tree_sums<N>(v, part_sums + (size_t)blockIdx.x * N);
  __threadfence();                                  // the block's sums are visible device-wide ...
  __syncthreads();
  if (tid == 0) last = (atomicAdd(ticket, 1) == (int)gridDim.x - 1);   // ... before its ticket is
  __syncthreads();
  if (!last) return false;                          // block-uniform
  __threadfence();
  if (tid == 0) *ticket = 0;
  return true;
}

// nblk rows of N block sums -> the item's N sums (in LDS), by ONE workgroup, in a fixed shape: lane l of sum k adds blocks
// l, l + kIcpLanes, ...; the kIcpLanes partials are added in lane order.  Run-to-run reproducible, a function of Ns alone;
// ipl::reduce_blocks (csrc/icp_plane.hpp) states the same order for the host.
template <int N>
__device__ __forceinline__ const double* reduce_blocks(const double* __restrict__ part_sums, int nblk) {
  __shared__ double part[N][kIcpLanes];
  __shared__ double tot[N];
  for (int idx = threadIdx.x; idx < N * kIcpLanes; idx += blockDim.x) {
    const int k = idx / kIcpLanes, l = idx % kIcpLanes;
    double s = 0.0;
    for (int i = l; i < nblk; i += kIcpLanes) s += part_sums[(size_t)i * N + k];
    part[k][l] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
    for (int l = 0; l < kIcpLanes; ++l) s += part[threadIdx.x][l];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  return tot;
}

// ------------------------------------------------------------------------------- the estimators
// Cyclic Jacobi on a symmetric 4x4; every loop has constant bounds and is unrolled so A and V
// stay in registers (indexed dynamically they live in scratch memory: 60 us per call instead of 10).
__device__ void jacobi4_largest(double A[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, dia = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      dia += A[p][p] * A[p][p];
#pragma unroll
      for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
    }
    // off-diagonal mass below 1e-34 of the diagonal's: the eigenvector is converged to ~1e-17 — Jacobi
    // converges quadratically, so the sweeps this saves (it used to run until off underflowed) are pure
    // serial latency in a one-thread tail
    if (off <= 1e-34 * dia) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        if (A[p][r] != 0.0) {
          const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- A J
            const double akp = A[k][p], akr = A[k][r];
            A[k][p] = c * akp - sn * akr;
            A[k][r] = sn * akp + c * akr;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- J^T A
            const double apk = A[p][k], ark = A[r][k];
            A[p][k] = c * apk - sn * ark;
            A[r][k] = sn * apk + c * ark;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkr = V[k][r];
            V[k][p] = c * vkp - sn * vkr;
            V[k][r] = sn * vkp + c * vkr;
          }
        }
      }
  }
  double lam = A[0][0];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = V[k][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    if (A[j][j] > lam) {
      lam = A[j][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = V[k][j];
    }
  }
}

// Point-to-point: the kNV sums of nn_finalize_kernel<true> (f64 distance of the winner, radius test, covariance terms);
// dT is the rigid fit of the matched pairs (Horn's closed form: largest eigenvector of the 4x4 quaternion matrix by cyclic
// Jacobi — always a proper rotation, equal to the SVD/Kabsch solution).  T (read by the searches, composed in place) and
// result (fitness, inlier_rmse, iterations, inliers) are the caller's, out_item_stride doubles apart.
struct PointToPoint {
  static constexpr int kSums = kNV;
  double* T;
  double* result;
  size_t out_item_stride;
  __device__ __forceinline__ void to_item(size_t b) { T += b * out_item_stride; result += b * out_item_stride; }
  __host__ __device__ const double* search_T() const { return T; }
  __device__ __forceinline__ void init() const { T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1; }
  __device__ __forceinline__ void row(const float* __restrict__ src, int qi, const float* __restrict__ tgt, int bi, double radius,
                                      double (&v)[kSums]) const {
    double q0, q1, q2;
    xform64(T, src[3 * (size_t)qi], src[3 * (size_t)qi + 1], src[3 * (size_t)qi + 2], q0, q1, q2);
    const double t0 = tgt[3 * (size_t)bi], t1 = tgt[3 * (size_t)bi + 1], t2 = tgt[3 * (size_t)bi + 2];
    const double ex = q0 - t0, ey = q1 - t1, ez = q2 - t2;
    const double s2 = fma(ez, ez, fma(ey, ey, ex * ex));
    if (s2 <= radius * radius) {
      v[0] = sqrt(s2); v[1] = s2; v[2] = 1.0;
      const double q[3] = {q0, q1, q2}, tt[3] = {t0, t1, t2};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        v[3 + r] = q[r];
        v[6 + r] = tt[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[9 + 3 * r + c] = q[r] * tt[c];
      }
    }
  }
  __device__ void finish(const double* v, int Ns, int max_iter, double rel_fitness, double rel_rmse, IcpState* __restrict__ st) const {
    const double n = v[2];
    const double fit = n / (double)Ns;
    const double rmse = n > 0 ? sqrt(v[1] / n) : 0.0;
    const int it = st->iter;
    result[0] = fit; result[1] = rmse; result[2] = (double)it; result[3] = n;
    const bool conv = it > 0 && fabs(st->prev_fit - fit) < rel_fitness && fabs(st->prev_rmse - rmse) < rel_rmse;
    if (conv || it >= max_iter || n < 3) { st->done = 1; return; }
    st->prev_fit = fit; st->prev_rmse = rmse; st->iter = it + 1;
    // rigid fit of the matched pairs: S = sum (q - mq)(t - mt)^T
    double mq[3], mt[3], S[3][3];
    for (int a = 0; a < 3; ++a) { mq[a] = v[3 + a] / n; mt[a] = v[6 + a] / n; }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[a][b] = v[9 + 3 * a + b] - n * mq[a] * mt[b];
    double N4[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double q[4];
    jacobi4_largest(N4, q);
    const double nq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * nq, x = q[1] * nq, y = q[2] * nq, z = q[3] * nq;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    double U[3][4];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) U[a][b] = R[a][b];
      U[a][3] = mt[a] - (R[a][0] * mq[0] + R[a][1] * mq[1] + R[a][2] * mq[2]);
    }
    double Tn[12];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 4; ++b)
        Tn[4 * a + b] = U[a][0] * T[b] + U[a][1] * T[4 + b] + U[a][2] * T[8 + b] + (b == 3 ? U[a][3] : 0.0);
    for (int k = 0; k < 12; ++k) T[k] = Tn[k];
  }
};

// Point-to-plane (include/isr_icp_plane.h): the row, the 31 sums, the 6x6 solve and the update are csrc/icp_plane.hpp's and
// nothing else, so that the host entry isr_icp_point_to_plane_batch_host gives the same bits.  The searches read an item's T
// from rows kIcpItemDoubles apart (their instantiation is point-to-point's): the loop keeps its working T in the workspace
// in that layout (Tw) and mirrors it into the caller's (B, 24) state after every pass.
struct PointToPlane {
  static constexpr int kSums = ipl::kSums;
  const float* nrm;
  int kernel;
  double kw;
  double* Tw;
  double* state;
  __device__ __forceinline__ void to_item(size_t b) { state += b * ipl::kStateDoubles; Tw += b * kIcpItemDoubles; }
  __host__ __device__ const double* search_T() const { return Tw; }
  __device__ __forceinline__ void init() const {
    for (int k = 0; k < 12; ++k) Tw[k] = state[k];
    state[12] = 0; state[13] = 0; state[14] = 0; state[15] = 1;
  }
  __device__ __forceinline__ void row(const float* __restrict__ src, int qi, const float* __restrict__ tgt, int bi_, double threshold,
                                      double (&v)[kSums]) const {
    const size_t bi = (unsigned int)bi_;
    double p[3];
    ipl::xform(Tw, src[3 * (size_t)qi], src[3 * (size_t)qi + 1], src[3 * (size_t)qi + 2], p);
    const double t[3] = {tgt[3 * bi], tgt[3 * bi + 1], tgt[3 * bi + 2]};
    const double nt[3] = {nrm[3 * bi], nrm[3 * bi + 1], nrm[3 * bi + 2]};
    ipl::row(p, t, nt, threshold, kernel, kw, v);
  }
  __device__ void finish(const double* tot, int Ns, int max_iter, double rel_fitness, double rel_rmse, IcpState* __restrict__ st) const {
    double sums[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) sums[k] = tot[k];
    ipl::Loop lp{st->prev_fit, st->prev_rmse, st->iter, st->done};
    double T[12], out[8];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tw[k];
    ipl::finish_pass(sums, Ns, max_iter, rel_fitness, rel_rmse, T, &lp, out);
#pragma unroll
    for (int k = 0; k < 12; ++k) { Tw[k] = T[k]; state[k] = T[k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) state[16 + k] = out[k];
    st->prev_fit = lp.prev_fit; st->prev_rmse = lp.prev_rmse; st->iter = lp.iter;
    __threadfence();
    st->done = lp.done;
  }
};

// ------------------------------------------------------------------------------- the kernels
// One pass and one init, written once; each estimator has a thin kernel of its own over them with the flat argument list
// (the one-template form, the estimator travelling as a struct argument, met the register conditions but put the bench step
// above the parent's range in one of two timing sessions — profiles/icp_pass_ab.txt — so the fallback it is).
template <class Est>
__device__ __forceinline__ void icp_pass(
    const float* __restrict__ src, int Ns, const float* __restrict__ tgt, int Nt, double radius,
    unsigned long long* __restrict__ packed, int32_t* __restrict__ prev_idx, int32_t* __restrict__ amb,
    double* __restrict__ part_sums, int max_iter, double rel_fitness, double rel_rmse, IcpState* __restrict__ st,
    size_t src_item_stride, Est est) {
  {
    const size_t b = blockIdx.y;
    src += b * src_item_stride;
    packed += b * Ns; prev_idx += b * Ns; amb += b * Ns;
    part_sums += b * gridDim.x * Est::kSums;
    st += b;
    est.to_item(b);
  }
  if (st->done) return;
  const int qi = blockIdx.x * kThreads + threadIdx.x;
  resolve_flagged(est.search_T(), src, tgt, Nt, Ns, amb, packed);
  // the row of this thread's source point (zeros for no neighbour, a pair beyond the radius, a row past Ns)
  double v[Est::kSums];
#pragma unroll
  for (int k = 0; k < Est::kSums; ++k) v[k] = 0.0;
  if (qi < Ns) {
    const int bi = take_winner(packed, prev_idx, qi);
    if (bi >= 0) est.row(src, qi, tgt, bi, radius, v);
  }
  if (!block_sums<Est::kSums>(v, part_sums, &st->ticket)) return;
  const double* sums = reduce_blocks<Est::kSums>(part_sums, gridDim.x);
  if (threadIdx.x == 0) est.finish(sums, Ns, max_iter, rel_fitness, rel_rmse, st);
}

__global__ __launch_bounds__(kThreads) void icp_finalize_update_kernel(
    const float* __restrict__ src, int Ns, const float* __restrict__ tgt, int Nt, double radius,
    unsigned long long* __restrict__ packed, int32_t* __restrict__ prev_idx, int32_t* __restrict__ amb,
    double* __restrict__ part_sums, int max_iter,
    double rel_fitness, double rel_rmse, double* __restrict__ T, IcpState* __restrict__ st, double* __restrict__ result,
    size_t src_item_stride, size_t out_item_stride) {
  icp_pass(src, Ns, tgt, Nt, radius, packed, prev_idx, amb, part_sums, max_iter, rel_fitness, rel_rmse, st, src_item_stride,
           PointToPoint{T, result, out_item_stride});
}

__global__ __launch_bounds__(kThreads) void icp_plane_finalize_update_kernel(
    const float* __restrict__ src, int Ns, const float* __restrict__ tgt, const float* __restrict__ nrm, int Nt,
    double threshold, unsigned long long* __restrict__ packed, int32_t* __restrict__ prev_idx, int32_t* __restrict__ amb,
    double* __restrict__ part_sums, int max_iter, double rel_fitness, double rel_rmse, int kernel, double kw,
    double* __restrict__ Tw, IcpState* __restrict__ st, double* __restrict__ state, size_t src_item_stride) {
  icp_pass(src, Ns, tgt, Nt, threshold, packed, prev_idx, amb, part_sums, max_iter, rel_fitness, rel_rmse, st, src_item_stride,
           PointToPlane{nrm, kernel, kw, Tw, state});
}

template <class Est>
__device__ __forceinline__ void icp_init(IcpState* st, unsigned long long* packed, int32_t* amb, int Ns, Est est) {
  const size_t b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Ns) { packed[b * Ns + i] = ~0ull; amb[b * Ns + i] = 0; }
  if (i != 0) return;
  st += b;
  est.to_item(b);
  st->prev_fit = 0; st->prev_rmse = 0; st->iter = 0; st->done = 0; st->ticket = 0;
  est.init();
}

__global__ void icp_init_kernel(IcpState* st, double* T, unsigned long long* packed, int32_t* amb, int Ns,
                                size_t out_item_stride) {
  icp_init(st, packed, amb, Ns, PointToPoint{T, nullptr, out_item_stride});
}

__global__ void icp_plane_init_kernel(IcpState* st, double* __restrict__ state, double* __restrict__ Tw,
                                      unsigned long long* packed, int32_t* amb, int Ns) {
  icp_init(st, packed, amb, Ns, PointToPlane{nullptr, 0, 0.0, Tw, state});
}

// max |t|^2 over the target cloud (f32, rounded up a little): the rounding-displacement bound of the EXACT search
__global__ __launch_bounds__(kThreads) void cloud_r2max_kernel(const float* __restrict__ tgt, int Nt, float* __restrict__ out) {
  __shared__ float red[kThreads / 64];
  float m = 0.f;
  for (int j = threadIdx.x; j < Nt; j += kThreads) {
    const float x = tgt[3 * (size_t)j], y = tgt[3 * (size_t)j + 1], z = tgt[3 * (size_t)j + 2];
    m = fmaxf(m, __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *out = 1.0001f * fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ------------------------------------------------------------------------------- the host side
// The loop's buffers, carved in one place: over a null workspace for the *_workspace_bytes entries (w.off is the answer),
// over the caller's for the loop.  item: extra_item_doubles per problem (point-to-plane's Tw).
struct IcpBufs {
  double* part_sums;
  IcpState* st;
  double* item;
  unsigned long long* packed;
  int32_t *prev_idx, *amb;
  float *t2_bound, *tile_box;
};

IcpBufs carve(isr::Workspace& w, const NNPlan& p, int Ns, int Nt, int B, int nsums, int extra_item_doubles) {
  IcpBufs b;
  b.part_sums = w.take<double>((size_t)B * p.fblocks * nsums);
  b.st = w.take<IcpState>(B);
  b.item = w.take<double>((size_t)B * extra_item_doubles);
  b.packed = w.take<unsigned long long>((size_t)B * Ns);
  b.prev_idx = w.take<int32_t>((size_t)B * Ns);
  b.amb = w.take<int32_t>((size_t)B * Ns);
  b.t2_bound = w.take<float>(1);
  b.tile_box = w.take<float>((size_t)((Nt + kTile - 1) / kTile) * 6);
  return b;
}

size_t icp_workspace_bytes(int Ns, int Nt, int B, int nsums, int extra_item_doubles) {
  if (Ns <= 0 || Nt <= 0 || B <= 0) return 0;
  isr::Workspace w(nullptr, 0);
  carve(w, make_plan(Ns, Nt, B, true), Ns, Nt, B, nsums, extra_item_doubles);
  return w.off;
}

// init, the target's bound and tile boxes (once per call: the target is shared), then max_iter + 1 passes of two launches:
// 3 + 2 (max_iter + 1) launches whatever B is.  Always the brute-force search (the grid searches lose here: most source
// points have their neighbour 5-20 mm away and a 20 mm ball covers a large part of the object — 18 ms / 103 ms against
// 2.5 ms per loop, round 2), with near ties decided in f64: every pass returns the EXACT nearest neighbours, as a KD-tree
// on doubles does.  items: the searches with the problem on blockIdx.z (nn_search_kernel<.., ITEMS>; the batch entries) or
// the single call's own instantiations (B = 1).  An item that has stopped raises its own done flag: its workgroups of the
// remaining launches leave at once.
template <class Est>
int run_icp_loop(const char* what, const NNPlan& p, const IcpBufs& b, hipStream_t stream, const float* src, size_t src_item_stride,
                 int Ns, const float* tgt, int Nt, int B, bool items, double threshold, int max_iter, double rel_fitness,
                 double rel_rmse, const Est& est) {
  const bool warm = isr::tuning(ISR_TUNE_ICP_WARM) != 0;          // tuning knob: 0 keeps every pass on the cold kernel
  const dim3 rows(p.fblocks, B);
  if constexpr (std::is_same_v<Est, PointToPoint>)
    icp_init_kernel<<<rows, kThreads, 0, stream>>>(b.st, est.T, b.packed, b.amb, Ns, est.out_item_stride);
  else
    icp_plane_init_kernel<<<rows, kThreads, 0, stream>>>(b.st, est.state, est.Tw, b.packed, b.amb, Ns);
  cloud_r2max_kernel<<<1, kThreads, 0, stream>>>(tgt, Nt, b.t2_bound);
  // per-wave tile cull of the searches (nn_search_kernel): boxes of the target's 256-point tiles; the radius caps every
  // lane's bound (f32, rounded up: the pass's f64 test s2 <= threshold^2 decides what counts).  Pays when the clouds' rows are
  // spatially ordered (registration.icp_point_to_point sorts them); otherwise every box is the whole cloud and nothing is skipped.
  const float cull_r2 = (float)(threshold * threshold * 1.0001 + 1e-6);
  if (ISR_ICP_CULL) tile_box_kernel<<<(Nt + kTile - 1) / kTile, 256, 0, stream>>>(tgt, Nt, b.tile_box);
  const dim3 grid(p.qblocks, p.nsplit, B);
  for (int it = 0; it <= max_iter; ++it) {
    // from the second pass on: the warm-started filter search, bounded by the previous pass's neighbour
    const int32_t* w_idx = (it > 0 && warm) ? b.prev_idx : nullptr;
    launch_search(p, grid, stream, src, Ns, tgt, Nt, est.search_T(), nullptr, nullptr, nullptr, &b.st->done, nullptr, b.packed, w_idx,
                  b.amb, b.t2_bound, ISR_ICP_CULL ? b.tile_box : nullptr, cull_r2, items, src_item_stride);
    if constexpr (std::is_same_v<Est, PointToPoint>)
      icp_finalize_update_kernel<<<rows, kThreads, 0, stream>>>(src, Ns, tgt, Nt, threshold, b.packed, b.prev_idx, b.amb, b.part_sums,
                                                                max_iter, rel_fitness, rel_rmse, est.T, b.st, est.result,
                                                                src_item_stride, est.out_item_stride);
    else
      icp_plane_finalize_update_kernel<<<rows, kThreads, 0, stream>>>(src, Ns, tgt, est.nrm, Nt, threshold, b.packed, b.prev_idx,
                                                                      b.amb, b.part_sums, max_iter, rel_fitness, rel_rmse,
                                                                      est.kernel, est.kw, est.Tw, b.st, est.state, src_item_stride);
  }
  ISR_CHECK_LAUNCH(what);
  return ISR_OK;
}

}  // namespace
