// fps.hip — farthest-point sampling of B clouds (fps.hpp states the arithmetic): the entries of include/isr_fps.h.
//
// K selections are K-1 strictly dependent steps, each one pass over the cloud plus a global arg-max.  The seam between two
// steps is a KERNEL BOUNDARY: one launch per step, all of them enqueued on the caller's stream with no host synchronise.
// No workgroup ever waits for another inside a launch — no grid barrier, no flag, no atomic, no fence — so nothing here
// depends on how many workgroups are resident at once.
//   init:    the caller's (B, M, 3) rows -> x, y, z planes in the workspace (16-byte loads in the step), mind = +inf, the
//            lengths, the first "partial" (+inf, start) of every cloud, and the -1 / 0 padding of idx / radius2 past len.
//   step k:  workgroup (g, b) reduces the G partial (value, index) pairs step k-1 left in one half of a ping-pong buffer —
//            every workgroup does so redundantly, so all of them know s_{k-1}; workgroup (0, b) records idx[b, k-1] and
//            radius2[b, k-1]; each workgroup then updates its slice of mind against s_{k-1} and writes its own partial to
//            the other half.  The launch that records the last selection updates nothing (a (1, B) grid).
// Reductions: lanes by __shfl_xor, waves through LDS, workgroups through the partials; every level compares (value, index)
// exactly with fps::better, a strict total order, so the winner does not depend on G, the slice or the order of the levels.
#include "fps.hpp"
#include "isr_common.hpp"

#include "../../include/isr_fps.h"

#include <vector>

namespace {

using namespace isr::fps;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / isr::kWave;
constexpr int kPass = kThreads * 4;     // points a workgroup takes per pass: one float4 per thread and plane
constexpr int kMaxG = 1024;             // workgroups per cloud at most: 4 per CU, the chip filled once
constexpr int kInitClouds = 64;         // clouds per init launch: their lengths and starts travel as kernel arguments
constexpr int kMaxClouds = 65535;       // blockIdx.y

struct Pair {
  float v;
  int i;
};

struct Plan {
  float* planes;     // per cloud x, y, z, mind: 4 planes of Mpad floats
  Pair* part;        // per cloud 2 halves of kMaxG partials
  int* lens;         // B
  int M, Mpad;
  int slice;         // points per workgroup, a multiple of kPass
};

struct InitArgs {
  int len[kInitClouds];
  int start[kInitClouds];
};

__device__ __forceinline__ float* plane(const Plan& p, int b, int c) { return p.planes + ((size_t)b * 4 + c) * p.Mpad; }

// The workgroup's best pair, in every thread.  sv / si: kWaves entries, not in use by a reduction still in flight.
__device__ __forceinline__ void block_best(float& bv, int& bi, float* sv, int* si) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = bv;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = sv[0];
  bi = si[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (better(sv[w], si[w], bv, bi)) {
      bv = sv[w];
      bi = si[w];
    }
}

__global__ __launch_bounds__(kThreads) void fps_init_kernel(Plan p, InitArgs a, int b0, const float* __restrict__ pts, int K,
                                                            int32_t* __restrict__ idx, float* __restrict__ radius2) {
  const int b = b0 + blockIdx.y;
  const int len = a.len[blockIdx.y];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) p.lens[b] = len;
  if (i < kMaxG) {
    Pair q;
    q.v = INFINITY;
    q.i = a.start[blockIdx.y];
    p.part[(size_t)b * 2 * kMaxG + i] = q;
  }
  if (i < len) {
    const float* src = pts + ((size_t)b * p.M + i) * 3;
    plane(p, b, 0)[i] = src[0];
    plane(p, b, 1)[i] = src[1];
    plane(p, b, 2)[i] = src[2];
    plane(p, b, 3)[i] = INFINITY;
  }
  if (i >= len && i < K) {
    idx[(size_t)b * K + i] = -1;
    if (radius2) radius2[(size_t)b * K + i] = 0.f;
  }
}

template <bool kUpdate>
__global__ __launch_bounds__(kThreads) void fps_step_kernel(Plan p, int k, int K, int32_t* __restrict__ idx,
                                                            float* __restrict__ radius2) {
  __shared__ float sv[2][kWaves];
  __shared__ int si[2][kWaves];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = p.lens[b];
  if (k - 1 >= len) return;                          // this cloud is exhausted: init wrote its padding
  const int G = (len + p.slice - 1) / p.slice;
  if ((int)blockIdx.x >= G) return;                  // a shorter cloud of the batch

  // s_{k-1}: the best of the partials of step k-1
  const Pair* in = p.part + ((size_t)b * 2 + ((k - 1) & 1)) * kMaxG;
  float bv = no_value();
  int bi = kNoIndex;
  for (int g = tid; g < G; g += kThreads) {
    const Pair q = in[g];
    if (better(q.v, q.i, bv, bi)) {
      bv = q.v;
      bi = q.i;
    }
  }
  block_best(bv, bi, sv[0], si[0]);
  bi = selected(bi);
  if (blockIdx.x == 0 && tid == 0) {
    idx[(size_t)b * K + k - 1] = bi;
    if (radius2) radius2[(size_t)b * K + k - 1] = bv;
  }
  if (!kUpdate) return;

  const float* x = plane(p, b, 0);
  const float* y = plane(p, b, 1);
  const float* z = plane(p, b, 2);
  float* mind = plane(p, b, 3);
  const float sx = x[bi], sy = y[bi], sz = z[bi];
  const int base = blockIdx.x * p.slice;
  const int end = min(base + p.slice, len);
  bv = no_value();
  bi = kNoIndex;
  // i is a multiple of 4 below len, and the planes hold Mpad = M rounded up to 4 floats: the 16-byte accesses stay inside
  // them.  Lanes past `end` (they are past len: base and slice are multiples of 4) compute on whatever is there and are no
  // candidates.
  for (int i = base + tid * 4; i < end; i += kPass) {
    const float4 X = *reinterpret_cast<const float4*>(x + i);
    const float4 Y = *reinterpret_cast<const float4*>(y + i);
    const float4 Z = *reinterpret_cast<const float4*>(z + i);
    float4 m = *reinterpret_cast<const float4*>(mind + i);
    m.x = fminf(m.x, dist2(X.x, Y.x, Z.x, sx, sy, sz));
    m.y = fminf(m.y, dist2(X.y, Y.y, Z.y, sx, sy, sz));
    m.z = fminf(m.z, dist2(X.z, Y.z, Z.z, sx, sy, sz));
    m.w = fminf(m.w, dist2(X.w, Y.w, Z.w, sx, sy, sz));
    *reinterpret_cast<float4*>(mind + i) = m;
    if (better(m.x, i, bv, bi)) { bv = m.x; bi = i; }
    if (i + 1 < end && better(m.y, i + 1, bv, bi)) { bv = m.y; bi = i + 1; }
    if (i + 2 < end && better(m.z, i + 2, bv, bi)) { bv = m.z; bi = i + 2; }
    if (i + 3 < end && better(m.w, i + 3, bv, bi)) { bv = m.w; bi = i + 3; }
  }
  block_best(bv, bi, sv[1], si[1]);
  if (tid == 0) {
    Pair q;
    q.v = bv;
    q.i = bi;
    p.part[((size_t)b * 2 + (k & 1)) * kMaxG + blockIdx.x] = q;
  }
}

__global__ void fps_empty_kernel() {}

int slice_for(int maxlen) {
  const long per = ((long)maxlen + kMaxG - 1) / kMaxG;
  return (int)((per + kPass - 1) / kPass * kPass);
}

size_t carve(isr::Workspace& ws, int B, int M, Plan& p) {
  p.M = M;
  p.Mpad = (M + 3) / 4 * 4;
  p.lens = ws.take<int>(B);
  p.part = ws.take<Pair>((size_t)B * 2 * kMaxG);
  p.planes = ws.take<float>((size_t)B * 4 * p.Mpad);
  return ws.off;
}

// the checks both samplers share; maxlen: the longest cloud
int check_sample(const char* who, const float* pts, int B, int M, const int32_t* lengths, const int32_t* start, int K,
                 const int32_t* idx, int& maxlen) {
  ISR_REQUIRE(pts && idx, "%s: null pointer", who);
  ISR_REQUIRE(B >= 1 && B <= kMaxClouds, "%s: B = %d (1..%d)", who, B, kMaxClouds);
  ISR_REQUIRE(M >= 1 && M <= kMaxPoints, "%s: M = %d (1..%d)", who, M, kMaxPoints);
  ISR_REQUIRE(K >= 1, "%s: K = %d", who, K);
  maxlen = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lengths ? lengths[b] : M;
    ISR_REQUIRE(len >= 1 && len <= M, "%s: lengths[%d] = %d outside 1..%d", who, b, len, M);
    const int s = start ? start[b] : 0;
    ISR_REQUIRE(s >= 0 && s < len, "%s: start[%d] = %d outside 0..%d", who, b, s, len - 1);
    maxlen = len > maxlen ? len : maxlen;
  }
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_fps_workspace_bytes(int B, int M) {
  if (B < 1 || B > kMaxClouds || M < 1 || M > kMaxPoints) {
    isr::set_error("isr_fps_workspace_bytes: B = %d (1..%d), M = %d (1..%d)", B, kMaxClouds, M, kMaxPoints);
    return 0;
  }
  isr::Workspace ws(nullptr, 0);
  Plan p;
  return carve(ws, B, M, p);
}

extern "C" int isr_fps_sample(const float* pts, int B, int M, const int32_t* lengths, const int32_t* start, int K, int32_t* idx,
                              float* radius2, void* ws_ptr, size_t ws_bytes, isr_stream_t stream) {
  int maxlen = 0;
  if (int rc = check_sample("isr_fps_sample", pts, B, M, lengths, start, K, idx, maxlen)) return rc;
  ISR_REQUIRE(ws_ptr, "isr_fps_sample: null workspace");
  isr::Workspace ws(ws_ptr, ws_bytes);
  Plan p;
  carve(ws, B, M, p);
  ISR_REQUIRE(ws.ok(), "isr_fps_sample: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  p.slice = slice_for(maxlen);
  hipStream_t st = isr::as_stream(stream);

  const int cover = max(max(maxlen, K), kMaxG);
  const unsigned init_blocks = (unsigned)(((long)cover + kThreads - 1) / kThreads);
  for (int b0 = 0; b0 < B; b0 += kInitClouds) {
    const int nb = min(kInitClouds, B - b0);
    InitArgs a;
    for (int j = 0; j < kInitClouds; ++j) {
      a.len[j] = j < nb ? (lengths ? lengths[b0 + j] : M) : 0;
      a.start[j] = j < nb && start ? start[b0 + j] : 0;
    }
    fps_init_kernel<<<dim3(init_blocks, nb), kThreads, 0, st>>>(p, a, b0, pts, K, idx, radius2);
    ISR_CHECK_LAUNCH("fps_init_kernel");
  }
  const int steps = min(K, maxlen);                  // selections any cloud still makes
  const unsigned G = (unsigned)((maxlen + p.slice - 1) / p.slice);
  for (int k = 1; k <= steps; ++k) {
    if (k < steps)
      fps_step_kernel<true><<<dim3(G, B), kThreads, 0, st>>>(p, k, K, idx, radius2);
    else
      fps_step_kernel<false><<<dim3(1, B), kThreads, 0, st>>>(p, k, K, idx, radius2);
    ISR_CHECK_LAUNCH("fps_step_kernel");
  }
  return ISR_OK;
}

extern "C" int isr_fps_sample_host(const float* pts, int B, int M, const int32_t* lengths, const int32_t* start, int K,
                                   int32_t* idx, float* radius2) {
  int maxlen = 0;
  if (int rc = check_sample("isr_fps_sample_host", pts, B, M, lengths, start, K, idx, maxlen)) return rc;
  std::vector<float> mind((size_t)maxlen);
  for (int b = 0; b < B; ++b)
    sample_host(pts + (size_t)b * M * 3, lengths ? lengths[b] : M, start ? start[b] : 0, K, idx + (size_t)b * K,
                radius2 ? radius2 + (size_t)b * K : nullptr, mind.data());
  return ISR_OK;
}

extern "C" int isr_fps_launch_floor(int launches, isr_stream_t stream) {
  ISR_REQUIRE(launches >= 0, "isr_fps_launch_floor: launches = %d", launches);
  for (int n = 0; n < launches; ++n) fps_empty_kernel<<<1, 64, 0, isr::as_stream(stream)>>>();
  ISR_CHECK_LAUNCH("fps_empty_kernel");
  return ISR_OK;
}
