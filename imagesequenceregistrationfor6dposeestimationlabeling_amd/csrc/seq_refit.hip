// seq_refit.hip — the sequence-level pose (include/isr_seq_refit.h states the entries, csrc/seq_refit.hpp the rule and its
// arithmetic).  A pass is three launches on the caller's stream:
//   seq_accumulate_kernel   grid (ceil(cap / 256), n): a thread forms the row of one slot in registers, each of the 32 sums
//                           crosses the wave by wave_sum_down, the workgroup writes its 32 doubles.  A workgroup past the
//                           frame's real slots (or of a frame of weight 0) returns: nobody reads its sums.
//   seq_frame_kernel        grid n: the frame's blocks -> its 32 sums (reduce_blocks' order) and its frame_stats.
//   seq_finish_kernel       one workgroup: the frames' sums -> 31 sums (reduce_blocks' order), then thread 0 applies the
//                           rule's end of a pass and writes Y, the state and the flag.
// No workgroup waits for another: no tickets, no device-scope fences, no float atomics; the stream orders the launches.
// Every launch of a pass after the stop reads the flag and returns.  Pass 0 does not read the flag (its finish writes it),
// so every workspace word that is read has been written in the same call.
#include "isr_common.hpp"

#include <vector>

#include "../../include/isr_seq_refit.h"
#include "block_prims.hpp"
#include "seq_refit.hpp"

namespace {

namespace sr = isr::seq_refit;
namespace ipl = isr::icp_plane;
static_assert(sr::kStateDoubles == ISR_SEQ_REFIT_STATE_DOUBLES && sr::kFrameStats == ISR_SEQ_REFIT_FRAME_STATS &&
                  ipl::kL2 == ISR_ICP_L2 && ipl::kHuber == ISR_ICP_HUBER && ipl::kTukey == ISR_ICP_TUKEY,
              "csrc/seq_refit.hpp and include/isr_seq_refit.h disagree");

constexpr int kThreads = sr::kRows;                       // a thread per slot
constexpr int kReduceThreads = sr::kBlockSums * ipl::kLanes;      // a thread per (sum, lane)
static_assert(kThreads == 256 && kReduceThreads == 512, "the sums' order is stated for 256-slot blocks of four waves");

__global__ __launch_bounds__(kThreads) void seq_accumulate_kernel(
    const float* __restrict__ p3d, const float* __restrict__ p2d, const int32_t* __restrict__ counts,
    const double* __restrict__ frame_w, const double* __restrict__ K, const double* __restrict__ G, int cap, int nblk, int kernel,
    double kw, const double* __restrict__ state, const int32_t* __restrict__ done, int pass, double* __restrict__ block_sums) {
  __shared__ double red[kThreads / 64][sr::kBlockSums];
  if (pass > 0 && *done) return;
  const int i = blockIdx.y, tid = threadIdx.x;
  const double fw = frame_w ? frame_w[i] : 1.0;
  const int count = counts[i];
  if ((int)blockIdx.x >= sr::frame_blocks(count, cap, fw)) return;      // block-uniform
  // the frame's 9 + 12 doubles and Y's 12, uniform over the workgroup
  double Yl[12], Gl[12], Kl[9];
#pragma unroll
  for (int q = 0; q < 12; ++q) { Yl[q] = state[q]; Gl[q] = G[(size_t)i * 12 + q]; }
#pragma unroll
  for (int q = 0; q < 9; ++q) Kl[q] = K[(size_t)i * 9 + q];
  const int m = blockIdx.x * kThreads + tid;              // < nblk * 256 <= cap + 255
  double v[sr::kBlockSums];
#pragma unroll
  for (int q = 0; q < sr::kBlockSums; ++q) v[q] = 0.0;
  if (m < sr::real_slots(count, cap)) {                   // m < cap: inside both arrays
    const size_t s = (size_t)i * cap + m;
    sr::row(Yl, Gl, Kl, fw, p3d[3 * s], p3d[3 * s + 1], p3d[3 * s + 2], p2d[2 * s], p2d[2 * s + 1], kernel, kw, v);
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < sr::kBlockSums; ++q) {
    const double s = isr::wave_sum_down(v[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (tid < sr::kBlockSums)
    block_sums[((size_t)i * nblk + blockIdx.x) * sr::kBlockSums + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// part (count values of one sum, stride doubles apart) -> icp_plane::reduce_blocks' result, by kBlockSums x kLanes threads:
// thread (q, l) adds values l, l + 16, .. of sum q onto 0.0, then thread q < kBlockSums adds the lanes in order onto 0.0.
__device__ __forceinline__ double reduce_lanes(const double* __restrict__ part, int count, int stride,
                                               double (*lanes)[ipl::kLanes]) {
  const int tid = threadIdx.x, q = tid / ipl::kLanes, l = tid % ipl::kLanes;
  double s = 0.0;
#pragma unroll 8
  for (int b = l; b < count; b += ipl::kLanes) s += part[(size_t)b * stride + q];
  lanes[q][l] = s;
  __syncthreads();
  double t = 0.0;
  if (tid < sr::kBlockSums) {
    for (int k = 0; k < ipl::kLanes; ++k) t += lanes[tid][k];
  }
  return t;                                               // threads 0 .. kBlockSums - 1 hold sum tid
}

__global__ __launch_bounds__(kReduceThreads) void seq_frame_kernel(const int32_t* __restrict__ counts,
                                                                   const double* __restrict__ frame_w, int cap, int nblk,
                                                                   const double* __restrict__ block_sums,
                                                                   const int32_t* __restrict__ done, int pass,
                                                                   double* __restrict__ frame_sums, double* __restrict__ frame_stats) {
  __shared__ double lanes[sr::kBlockSums][ipl::kLanes];
  __shared__ double fs[sr::kBlockSums];
  if (pass > 0 && *done) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int nb = sr::frame_blocks(counts[i], cap, frame_w ? frame_w[i] : 1.0);      // <= nblk
  const double t = reduce_lanes(block_sums + (size_t)i * nblk * sr::kBlockSums, nb, sr::kBlockSums, lanes);
  if (tid < sr::kBlockSums) {
    frame_sums[(size_t)i * sr::kBlockSums + tid] = t;
    fs[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double out[sr::kFrameStats];
    sr::frame_stats(fs, out);
#pragma unroll
    for (int q = 0; q < sr::kFrameStats; ++q) frame_stats[(size_t)i * sr::kFrameStats + q] = out[q];
  }
}

__global__ __launch_bounds__(kReduceThreads) void seq_finish_kernel(const double* __restrict__ frame_sums, int n, int max_iter,
                                                                    double tol_r, double tol_t, int pass,
                                                                    double* __restrict__ state, int32_t* __restrict__ done) {
  __shared__ double lanes[sr::kBlockSums][ipl::kLanes];
  __shared__ double tot[sr::kBlockSums];
  if (pass > 0 && *done) return;
  const int tid = threadIdx.x;
  const double t = reduce_lanes(frame_sums, n, sr::kBlockSums, lanes);
  if (tid < sr::kBlockSums) tot[tid] = t;
  __syncthreads();
  if (tid != 0) return;
  double sums[sr::kSums], Y[12], out[8];
#pragma unroll
  for (int q = 0; q < sr::kSums; ++q) sums[q] = tot[q];
#pragma unroll
  for (int q = 0; q < 12; ++q) Y[q] = state[q];
  const bool stop = sr::finish_pass(sums, pass, max_iter, tol_r, tol_t, Y, out);
#pragma unroll
  for (int q = 0; q < 12; ++q) state[q] = Y[q];
  state[12] = 0; state[13] = 0; state[14] = 0; state[15] = 1;
#pragma unroll
  for (int q = 0; q < 8; ++q) state[16 + q] = out[q];
  if (done) *done = stop ? 1 : 0;                         // null for n = 0: one launch, no later pass
}

int blocks_of(int cap) { return (cap + sr::kRows - 1) / sr::kRows; }

}  // namespace

extern "C" size_t isr_seq_refit_workspace_bytes(int n, int cap) {
  if (n < 1 || cap < 1) return 0;
  return isr::align_up((size_t)n * blocks_of(cap) * sr::kBlockSums * sizeof(double), 256) +
         isr::align_up((size_t)n * sr::kBlockSums * sizeof(double), 256) + 256;
}

extern "C" int isr_seq_refit(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w, const double* K,
                             const double* G, int n, int cap, int kernel, double k, int max_iter, double tol_r, double tol_t,
                             double* state, double* frame_stats, void* ws, size_t ws_bytes, isr_stream_t stream_) {
  if (const char* why = sr::refuse(p3d, p2d, counts, K, G, state, frame_stats, n, cap, kernel, k, max_iter)) {
    isr::set_error("isr_seq_refit: %s (n=%d cap=%d kernel=%d k=%g max_iter=%d)", why, n, cap, kernel, k, max_iter);
    return ISR_ERR_ARG;
  }
  if (n > 0 && (!ws || ws_bytes < isr_seq_refit_workspace_bytes(n, cap))) {
    isr::set_error("isr_seq_refit: workspace %zu < %zu", ws_bytes, isr_seq_refit_workspace_bytes(n, cap));
    return ISR_ERR_ARG;
  }
  hipStream_t stream = isr::as_stream(stream_);
  if (n == 0) {                                           // no frame_sums to read: the sums are zeros, status 2
    seq_finish_kernel<<<1, kReduceThreads, 0, stream>>>(nullptr, 0, max_iter, tol_r, tol_t, 0, state, nullptr);
    ISR_CHECK_LAUNCH("seq refit kernels");
    return ISR_OK;
  }
  const int nblk = blocks_of(cap);
  isr::Workspace w(ws, ws_bytes);
  double* block_sums = w.take<double>((size_t)n * nblk * sr::kBlockSums);
  double* frame_sums = w.take<double>((size_t)n * sr::kBlockSums);
  int32_t* done = w.take<int32_t>(1);
  for (int pass = 0; pass <= max_iter; ++pass) {
    seq_accumulate_kernel<<<dim3(nblk, n), kThreads, 0, stream>>>(p3d, p2d, counts, frame_w, K, G, cap, nblk, kernel, k, state, done,
                                                                  pass, block_sums);
    seq_frame_kernel<<<n, kReduceThreads, 0, stream>>>(counts, frame_w, cap, nblk, block_sums, done, pass, frame_sums, frame_stats);
    seq_finish_kernel<<<1, kReduceThreads, 0, stream>>>(frame_sums, n, max_iter, tol_r, tol_t, pass, state, done);
  }
  ISR_CHECK_LAUNCH("seq refit kernels");
  return ISR_OK;
}

// The same loop as host code over HOST pointers (csrc/seq_refit.hpp): the tests' reference, and the entry of CPU users.
extern "C" int isr_seq_refit_host(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w, const double* K,
                                  const double* G, int n, int cap, int kernel, double k, int max_iter, double tol_r, double tol_t,
                                  double* state, double* frame_stats) {
  if (const char* why = sr::refuse(p3d, p2d, counts, K, G, state, frame_stats, n, cap, kernel, k, max_iter)) {
    isr::set_error("isr_seq_refit_host: %s (n=%d cap=%d kernel=%d k=%g max_iter=%d)", why, n, cap, kernel, k, max_iter);
    return ISR_ERR_ARG;
  }
  std::vector<double> frame_sums((size_t)(n > 0 ? n : 1) * sr::kBlockSums);
  sr::host_loop(p3d, p2d, counts, frame_w, K, G, n, cap, kernel, k, max_iter, tol_r, tol_t, state, frame_stats, frame_sums.data(),
                [&](auto fn) { isr::parallel_rows(n, 2, fn); });
  return ISR_OK;
}

// The 31 sums of ONE pass at Y (12 doubles are read), as the loop forms them: what the tests compare with their restatement.
extern "C" int isr_seq_refit_sums_host(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w,
                                       const double* K, const double* G, int n, int cap, int kernel, double k, const double* Y,
                                       double* sums, double* frame_stats) {
  const char* why = sr::refuse(p3d, p2d, counts, K, G, Y, frame_stats, n, cap, kernel, k, 0);
  if (!why && !sums) why = "null pointer";
  if (why) {
    isr::set_error("isr_seq_refit_sums_host: %s (n=%d cap=%d kernel=%d k=%g)", why, n, cap, kernel, k);
    return ISR_ERR_ARG;
  }
  std::vector<double> frame_sums((size_t)(n > 0 ? n : 1) * sr::kBlockSums);
  sr::host_sums(p3d, p2d, counts, frame_w, K, G, n, cap, kernel, k, Y, sums, frame_stats, frame_sums.data(),
                [&](auto fn) { isr::parallel_rows(n, 2, fn); });
  return ISR_OK;
}
