// knn.hip — the exact k-nearest-neighbour search and the local frames (knn.hpp states both rules): the entries of
// include/isr_knn.h.
//
// knn_kernel: brute force, never an (Nq x Nt) matrix.  A workgroup of W waves takes W queries, one per wave, and streams the
// targets through one LDS tile of kTile points that all its waves share.  A wave finds its K-th smallest d2 by a radix
// select over the 32 bits of d2 (a non-negative f32 orders as its unsigned bits), one 8-bit digit per pass over the targets:
// the distances are recomputed on every pass, not stored, and the digit's 256-bin histogram of the targets that match the
// digits found so far lives in LDS (integer atomics; a wave whose lanes all hold the same digit adds once).  A fifth pass
// gathers the keys below the K-th value and the first ties at it in index order — a ballot prefix keeps that order — as
// 64-bit keys (d2 bits << 32 | index) in LDS, a bitonic sort puts them in ascending order, and the row is written.
// No float atomics; a wave's row depends on its query and the targets only, so neither W nor the grid shows in the result.
// W follows K alone, so that keys + histograms + tile stay below 64 KiB of LDS: 16 waves up to K = 256, 8 up to 512, then 4.
//
// local_frames_kernel: one lane per point runs knn::local_frame, the host's code.
#include "knn.hpp"
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_knn.h"

#include <vector>

namespace {

using namespace isr::knn;

constexpr int kTile = 1024;          // targets per staged tile (12 KiB)
constexpr int kBins = 256;           // one 8-bit digit per pass
constexpr size_t kWorkspaceBytes = 256;
constexpr int kFrameThreads = 64;

int waves_for(int Kpad) { return Kpad <= 256 ? 16 : (Kpad <= 512 ? 8 : 4); }

size_t lds_bytes(int W, int Kpad) { return (size_t)W * Kpad * 8 + (size_t)W * kBins * 4 + (size_t)kTile * 3 * 4; }

// the tile [base, base + n) of tgt into LDS: a flat, coalesced copy of 3 n floats; barriers on both sides
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ tgt, int base, int n) {
  __syncthreads();
  const float* src = tgt + 3 * (size_t)base;
  for (int k = threadIdx.x; k < 3 * n; k += blockDim.x) tile[k] = src[k];
  __syncthreads();
}

__global__ __launch_bounds__(1024) void knn_kernel(const float* __restrict__ qry, int Nq, const float* __restrict__ tgt, int Nt,
                                                   int K, int Kpad, int32_t* __restrict__ idx, float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t* keys = reinterpret_cast<uint64_t*>(lds) + (size_t)wave * Kpad;
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds + (size_t)W * Kpad * 8) + wave * kBins;
  float* tile = reinterpret_cast<float*>(lds + (size_t)W * Kpad * 8 + (size_t)W * kBins * 4);

  const long q_raw = (long)blockIdx.x * W + wave;
  const bool live = q_raw < Nq;                        // a wave past the last query works on the last one and writes nothing
  const long q = live ? q_raw : (long)Nq - 1;
  const float qx = qry[3 * q], qy = qry[3 * q + 1], qz = qry[3 * q + 2];

  // ---- the K-th smallest d2 by radix select: prefix = its digits so far, k_rem = its rank among the targets that share them
  uint32_t prefix = 0;
  int k_rem = K;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = lane; b < kBins; b += 64) hist[b] = 0;
    for (int base = 0; base < Nt; base += kTile) {
      const int n = min(kTile, Nt - base);
      stage_tile(tile, tgt, base, n);
      for (int t0 = 0; t0 < n; t0 += 64) {             // the whole wave makes every trip: the ballots see all 64 lanes
        const int t = t0 + lane;
        const bool valid = t < n;
        const uint32_t u = valid ? d2_bits(qx, qy, qz, tile[3 * t], tile[3 * t + 1], tile[3 * t + 2]) : 0u;
        const bool in = valid && (shift == 24 || (u >> ((shift + 8) & 31)) == prefix);
        const uint32_t digit = (u >> shift) & (kBins - 1);
        const unsigned long long m_in = __ballot(in);
        if (m_in != 0) {
          const int first_lane = __ffsll((long long)m_in) - 1;
          const uint32_t first = __shfl(digit, first_lane, 64);
          if (__ballot(in && digit == first) == m_in) {
            if (lane == first_lane) atomicAdd(&hist[first], (uint32_t)__popcll(m_in));
          } else if (in) {
            atomicAdd(&hist[digit], 1u);
          }
        }
      }
    }
    __syncthreads();
    // lane l owns bins 4 l .. 4 l + 3; an inclusive scan over the lanes finds the bin where the count reaches k_rem
    uint32_t c[4], own = 0;
    for (int b = 0; b < 4; ++b) {
      c[b] = hist[4 * lane + b];
      own += c[b];
    }
    const uint32_t incl = isr::wave_inclusive_scan(own);     // every wave has its own query: a scan of the wave alone
    const unsigned long long reach = __ballot(incl >= (uint32_t)k_rem);
    const int owner = reach ? __ffsll((long long)reach) - 1 : 63;
    uint32_t below = __shfl(incl - own, owner, 64);
    int bin = 3;
    bool found = false;
    for (int b = 0; b < 4; ++b) {
      const uint32_t cb = __shfl(c[b], owner, 64);
      if (!found) {
        if (below + cb >= (uint32_t)k_rem || b == 3) {
          bin = b;
          found = true;
        } else {
          below += cb;
        }
      }
    }
    prefix = (prefix << 8) | (uint32_t)(4 * owner + bin);
    k_rem -= (int)below;
    __syncthreads();
  }
  // prefix is the K-th smallest d2's bits; K - k_rem targets lie below it, and the first k_rem of those equal to it are taken

  // ---- gather: keys below the cut in index order, then the ties; every slot starts as a valid key, the padding sorts last
  for (int r = lane; r < Kpad; r += 64) keys[r] = r < K ? make_key(0xFFFFFFFFu, 0) : ~0ull;
  const int n_below = K - k_rem;
  int seen_below = 0, seen_tie = 0;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  for (int base = 0; base < Nt; base += kTile) {
    const int n = min(kTile, Nt - base);
    stage_tile(tile, tgt, base, n);
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int t = t0 + lane;
      const bool valid = t < n;
      const uint32_t u = valid ? d2_bits(qx, qy, qz, tile[3 * t], tile[3 * t + 1], tile[3 * t + 2]) : 0xFFFFFFFFu;
      const bool less = valid && u < prefix, tie = valid && u == prefix;
      const unsigned long long m_less = __ballot(less), m_tie = __ballot(tie);
      if (less) {
        const int slot = seen_below + __popcll(m_less & lt_mask);
        if (slot < n_below) keys[slot] = make_key(u, base + t);
      }
      if (tie) {
        const int rank = seen_tie + __popcll(m_tie & lt_mask);
        if (rank < k_rem) keys[n_below + rank] = make_key(u, base + t);
      }
      seen_below += __popcll(m_less);
      seen_tie += __popcll(m_tie);
    }
  }
  __syncthreads();

  // ---- bitonic sort of the wave's Kpad keys, ascending
  for (int k = 2; k <= Kpad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < Kpad; i += 64) {
        const int p = i ^ j;
        if (p > i) {
          const uint64_t a = keys[i], b = keys[p];
          if ((a > b) == ((i & k) == 0)) {
            keys[i] = b;
            keys[p] = a;
          }
        }
      }
      __syncthreads();
    }

  if (!live) return;
  for (int r = lane; r < K; r += 64) {
    const uint64_t key = keys[r];
    idx[(size_t)q * K + r] = (int32_t)(key & 0xFFFFFFFFu);
    if (d2_out) d2_out[(size_t)q * K + r] = bits_d2((uint32_t)(key >> 32));
  }
}

__global__ __launch_bounds__(kFrameThreads) void local_frames_kernel(const float* __restrict__ pts, int N,
                                                                     const int32_t* __restrict__ idx, int K, int disambiguate,
                                                                     double* __restrict__ curvatures, double* __restrict__ frames) {
  const long i = (long)blockIdx.x * kFrameThreads + threadIdx.x;
  if (i >= N) return;
  double curv[3], frame[9];
  local_frame(pts, N, idx + (size_t)i * K, K, (int)i, disambiguate, curv, frame);
  for (int c = 0; c < 3; ++c) curvatures[3 * i + c] = curv[c];
  for (int c = 0; c < 9; ++c) frames[9 * i + c] = frame[c];
}

int check_shape(const char* who, int Nq, int Nt, int K) {
  ISR_REQUIRE(Nq >= 1, "%s: Nq = %d (at least 1)", who, Nq);
  ISR_REQUIRE(Nt >= 1 && Nt <= kMaxTargets, "%s: Nt = %d (1..%d)", who, Nt, kMaxTargets);
  ISR_REQUIRE(K >= 1 && K <= kMaxK && K <= Nt, "%s: K = %d (1..min(Nt = %d, %d))", who, K, Nt, kMaxK);
  return ISR_OK;
}

int check_knn(const char* who, const float* qry, int Nq, const float* tgt, int Nt, int K, const int32_t* idx) {
  if (int rc = check_shape(who, Nq, Nt, K)) return rc;
  ISR_REQUIRE(qry && tgt && idx, "%s: null pointer", who);
  return ISR_OK;
}

int check_frames(const char* who, const float* pts, int N, const int32_t* idx, int K, const double* curvatures,
                 const double* frames) {
  ISR_REQUIRE(N >= 1, "%s: N = %d (at least 1)", who, N);
  ISR_REQUIRE(K >= 1 && K <= kMaxK, "%s: K = %d (1..%d)", who, K, kMaxK);
  ISR_REQUIRE(pts && idx && curvatures && frames, "%s: null pointer", who);
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_knn_workspace_bytes(int Nq, int Nt, int K) {
  if (check_shape("isr_knn_workspace_bytes", Nq, Nt, K)) return 0;
  return kWorkspaceBytes;
}

extern "C" int isr_knn(const float* qry, int Nq, const float* tgt, int Nt, int K, int32_t* idx, float* d2, void* ws,
                       size_t ws_bytes, isr_stream_t stream) {
  if (int rc = check_knn("isr_knn", qry, Nq, tgt, Nt, K, idx)) return rc;
  ISR_REQUIRE(ws, "isr_knn: null workspace");
  ISR_REQUIRE(ws_bytes >= kWorkspaceBytes, "isr_knn: workspace %zu bytes, needs %zu", ws_bytes, kWorkspaceBytes);
  const int Kpad = isr::pad_pow2(K), W = waves_for(Kpad);
  const unsigned blocks = (unsigned)(((long)Nq + W - 1) / W);
  knn_kernel<<<blocks, W * 64, lds_bytes(W, Kpad), isr::as_stream(stream)>>>(qry, Nq, tgt, Nt, K, Kpad, idx, d2);
  ISR_CHECK_LAUNCH("knn_kernel");
  return ISR_OK;
}

extern "C" int isr_knn_host(const float* qry, int Nq, const float* tgt, int Nt, int K, int32_t* idx, float* d2) {
  if (int rc = check_knn("isr_knn_host", qry, Nq, tgt, Nt, K, idx)) return rc;
  isr::parallel_rows(Nq, 64, [=](long i) {
    std::vector<uint64_t> keys((size_t)Nt);
    knn_row_host(qry + 3 * i, tgt, Nt, K, keys.data(), idx + (size_t)i * K, d2 ? d2 + (size_t)i * K : nullptr);
  });
  return ISR_OK;
}

extern "C" int isr_local_frames(const float* pts, int N, const int32_t* idx, int K, int disambiguate, double* curvatures,
                                double* frames, isr_stream_t stream) {
  if (int rc = check_frames("isr_local_frames", pts, N, idx, K, curvatures, frames)) return rc;
  const unsigned blocks = (unsigned)(((long)N + kFrameThreads - 1) / kFrameThreads);
  local_frames_kernel<<<blocks, kFrameThreads, 0, isr::as_stream(stream)>>>(pts, N, idx, K, disambiguate, curvatures, frames);
  ISR_CHECK_LAUNCH("local_frames_kernel");
  return ISR_OK;
}

extern "C" int isr_local_frames_host(const float* pts, int N, const int32_t* idx, int K, int disambiguate, double* curvatures,
                                     double* frames) {
  if (int rc = check_frames("isr_local_frames_host", pts, N, idx, K, curvatures, frames)) return rc;
  isr::parallel_rows(N, 64, [=](long i) {
    local_frame(pts, N, idx + (size_t)i * K, K, (int)i, disambiguate, curvatures + 3 * i, frames + 9 * i);
  });
  return ISR_OK;
}
