// contrastive.hip — the contrastive key loss and its gradient on the device (contrastive.hpp states the arithmetic): the
// entries of include/isr_contrastive.h.  No call synchronises, no float atomics; the logits are recomputed tile by tile and
// never stored, so the extra memory is O(B S) (and the partial sums of the split column pass).
//
// A lane owns a row (forward_kernel, backward_rows_kernel) or a negative (backward_columns_kernel) and keeps its D floats in
// registers; the other side streams through LDS in tiles of kBlock = 64 vectors, one inner chain of the header's sum orders
// per tile, read back by every lane at once (a broadcast).  Workgroups are one wave wide: at trainPose.py's B S = 16 384 rows
// that is one wave per CU, and a wave-wide barrier costs next to nothing.  The kernels are compiled for D padded to
// DP in {4, 12, 16, 32, 64}; EXACT (D == DP) drops the per-component test.  A work item (a row block of a batch item, a
// column block of a negative set and, in the split pass, a 1024-row range) is taken from a grid-stride loop, so no shape
// within the limits overflows a grid dimension.
//
//   forward_kernel            m, t, pos, rows of 64 rows: pass 1 the maximum, pass 2 the sums
//   isr::reduce_kernel        (ordered_sum.hpp) REDUCE ORDER level by level, the last level writes loss, LossFinish
//   backward_rows_kernel      dq, dk of 64 rows
//   backward_columns_kernel   dn of 64 columns; with Bn == 1 and few columns every 1024-row range is a work item of its own
//                             that writes its middle accumulator to the workspace, and
//   combine_columns_kernel    adds those in ascending order: the same order as the unsplit pass, so the same bits.
#include "contrastive.hpp"
#include "isr_common.hpp"

#include "../../include/isr_contrastive.h"

#include <vector>

namespace {

using namespace isr::contrastive;
using isr::kReduce;

constexpr int kThreads = 64;                   // rows (columns) of a workgroup: one wave
constexpr unsigned kMaxGrid = 1u << 20;
constexpr size_t kSplitBytes = 64u << 20;      // the split column pass is used while its partial sums fit this
constexpr int kSplitBelowBlocks = 512;         // and while the unsplit pass would start fewer workgroups than this

__host__ __device__ constexpr int pad_of(int D) { return D <= 4 ? 4 : D <= 12 ? 12 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }

// a tile of `cnt` vectors of D floats, contiguous in global memory, to LDS rows of DP floats
template <int DP>
__device__ __forceinline__ void load_tile(float* tile, const float* __restrict__ src, int cnt, int D) {
  for (int e = threadIdx.x; e < cnt * D; e += kThreads) {
    const int v = e / D, d = e - v * D;
    tile[v * DP + d] = src[e];
  }
}

template <int DP, bool EXACT>
__device__ __forceinline__ float tile_dot(const float (&own)[DP], const float (&other)[DP], int D) {
  float l = own[0] * other[0];
#pragma unroll
  for (int d = 1; d < DP; ++d)
    if (EXACT || d < D) l = fmaf(own[d], other[d], l);
  return l;
}

template <int DP>
__device__ __forceinline__ void read_vec(float (&v)[DP], const float* row) {
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = row[d];
}

template <int DP, bool EXACT>
__device__ __forceinline__ void load_own(float (&v)[DP], const float* __restrict__ src, int D) {
#pragma unroll
  for (int d = 0; d < DP; ++d) v[d] = (EXACT || d < D) ? src[d] : 0.f;
}

template <int DP, bool EXACT>
__global__ __launch_bounds__(kThreads) void forward_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ n, long long S, int M, int Din, int Bn,
                                                           long long blocks_per_b, long long items, float* __restrict__ m_out,
                                                           float* __restrict__ t_out, float* __restrict__ pos_out,
                                                           float* __restrict__ rows_out) {
  __shared__ __attribute__((aligned(16))) float tile[kBlock * DP];
  const int D = EXACT ? DP : Din;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long b = item / blocks_per_b, s = (item - b * blocks_per_b) * kThreads + threadIdx.x;
    const bool live = s < S;
    const size_t row = (size_t)b * S + (live ? s : S - 1);
    float qr[DP], kr[DP], nr[DP];
    load_own<DP, EXACT>(qr, q + row * D, D);
    load_own<DP, EXACT>(kr, k + row * D, D);
    const float pos = tile_dot<DP, EXACT>(qr, kr, D);
    const float* nb = n + (Bn == 1 ? (size_t)0 : (size_t)b * M * D);
    float m = pos;
    for (int j0 = 0; j0 < M; j0 += kBlock) {
      const int cnt = M - j0 < kBlock ? M - j0 : kBlock;
      __syncthreads();
      load_tile<DP>(tile, nb + (size_t)j0 * D, cnt, D);
      __syncthreads();
      for (int jj = 0; jj < cnt; ++jj) {
        read_vec<DP>(nr, tile + jj * DP);
        m = max_step(m, tile_dot<DP, EXACT>(qr, nr, D));
      }
    }
    double T = (double)exp32(pos - m);
    for (int j0 = 0; j0 < M; j0 += kBlock) {
      const int cnt = M - j0 < kBlock ? M - j0 : kBlock;
      __syncthreads();
      load_tile<DP>(tile, nb + (size_t)j0 * D, cnt, D);
      __syncthreads();
      float c = 0.f;
      for (int jj = 0; jj < cnt; ++jj) {
        read_vec<DP>(nr, tile + jj * DP);
        c += exp32(tile_dot<DP, EXACT>(qr, nr, D) - m);
      }
      T += (double)c;
    }
    if (live) {
      const float t = log_sum(T);
      m_out[row] = isr::canonical(m);
      t_out[row] = t;
      pos_out[row] = isr::canonical(pos);
      rows_out[row] = isr::canonical(t - (pos - m));
    }
  }
}

// the last step of the sum of the rows: the loss
struct LossFinish {
  double scale;
  long long rows;
  __device__ float operator()(double R, int) const { return loss_value(R, scale, rows); }
};

template <int DP, bool EXACT>
__global__ __launch_bounds__(kThreads) void backward_rows_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                 const float* __restrict__ n, long long S, int M, int Din, int Bn,
                                                                 long long blocks_per_b, long long items, double scale,
                                                                 long long rows, const float* __restrict__ m_in,
                                                                 const float* __restrict__ t_in, const float* __restrict__ g,
                                                                 float* __restrict__ dq, float* __restrict__ dk) {
  __shared__ __attribute__((aligned(16))) float tile[kBlock * DP];
  const int D = EXACT ? DP : Din;
  const float c = grad_scale(g ? *g : 1.f, scale, rows);
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long b = item / blocks_per_b, s = (item - b * blocks_per_b) * kThreads + threadIdx.x;
    const bool live = s < S;
    const size_t row = (size_t)b * S + (live ? s : S - 1);
    float qr[DP], kr[DP], nr[DP];
    load_own<DP, EXACT>(qr, q + row * D, D);
    load_own<DP, EXACT>(kr, k + row * D, D);
    const float m = m_in[row], t = t_in[row];
    const float a = exp32((tile_dot<DP, EXACT>(qr, kr, D) - m) - t) - 1.0f;
    if (dk && live) {
      const float ca = c * a;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (EXACT || d < D) dk[row * D + d] = isr::canonical(ca * qr[d]);
    }
    if (!dq) continue;                                   // uniform: the whole grid skips the tiles
    const float* nb = n + (Bn == 1 ? (size_t)0 : (size_t)b * M * D);
    float outer[DP], inner[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) outer[d] = 0.f;
    for (int j0 = 0; j0 < M; j0 += kBlock) {
      const int cnt = M - j0 < kBlock ? M - j0 : kBlock;
      __syncthreads();
      load_tile<DP>(tile, nb + (size_t)j0 * D, cnt, D);
      __syncthreads();
#pragma unroll
      for (int d = 0; d < DP; ++d) inner[d] = 0.f;
      for (int jj = 0; jj < cnt; ++jj) {
        read_vec<DP>(nr, tile + jj * DP);
        const float p = exp32((tile_dot<DP, EXACT>(qr, nr, D) - m) - t);
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (EXACT || d < D) inner[d] = fmaf(p, nr[d], inner[d]);
      }
#pragma unroll
      for (int d = 0; d < DP; ++d) outer[d] += inner[d];
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (EXACT || d < D) dq[row * D + d] = isr::canonical(c * fmaf(a, kr[d], outer[d]));
    }
  }
}

// splits == 1: a work item is (negative set, column block) and writes dn.  splits > 1 (Bn == 1): a work item is
// (column block, 1024-row range) and writes that range's middle accumulator to partial (splits, M, D).
template <int DP, bool EXACT>
__global__ __launch_bounds__(kThreads) void backward_columns_kernel(const float* __restrict__ q, const float* __restrict__ n,
                                                                    long long S, long long B, int M, int Din, int Bn,
                                                                    long long col_blocks, long long splits, long long items,
                                                                    double scale, const float* __restrict__ m_in,
                                                                    const float* __restrict__ t_in, const float* __restrict__ g,
                                                                    float* __restrict__ dn, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tile[kBlock * DP];
  __shared__ float mt[kBlock], tt[kBlock];
  const int D = EXACT ? DP : Din;
  const float c = grad_scale(g ? *g : 1.f, scale, B * S);
  const long long set_rows = Bn == 1 ? B * S : S;        // the rows a negative set meets
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long per_set = col_blocks * splits;
    const long long bn = item / per_set, rest = item - bn * per_set;
    const long long cb = rest / splits, sp = rest - cb * splits;
    const long long j = cb * kThreads + threadIdx.x;
    const bool live = j < M;
    const size_t col = (size_t)bn * M + (live ? j : M - 1);
    float nc[DP], qr[DP], outer[DP], mid[DP], inner[DP];
    load_own<DP, EXACT>(nc, n + col * D, D);
    const size_t row0 = Bn == 1 ? (size_t)0 : (size_t)bn * S;
    const long long first = splits > 1 ? sp * kSuperRows : 0;
    const long long last = splits > 1 ? (first + kSuperRows < set_rows ? first + kSuperRows : set_rows) : set_rows;
#pragma unroll
    for (int d = 0; d < DP; ++d) outer[d] = 0.f;
    for (long long s0 = first; s0 < last; s0 += kSuperRows) {
#pragma unroll
      for (int d = 0; d < DP; ++d) mid[d] = 0.f;
      const long long s1 = s0 + kSuperRows < last ? s0 + kSuperRows : last;
      for (long long i0 = s0; i0 < s1; i0 += kBlock) {
        const int cnt = (int)(s1 - i0 < kBlock ? s1 - i0 : kBlock);
        __syncthreads();
        load_tile<DP>(tile, q + (row0 + i0) * D, cnt, D);
        if ((int)threadIdx.x < cnt) {
          mt[threadIdx.x] = m_in[row0 + i0 + threadIdx.x];
          tt[threadIdx.x] = t_in[row0 + i0 + threadIdx.x];
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DP; ++d) inner[d] = 0.f;
        for (int ii = 0; ii < cnt; ++ii) {
          read_vec<DP>(qr, tile + ii * DP);
          const float p = exp32((tile_dot<DP, EXACT>(qr, nc, D) - mt[ii]) - tt[ii]);
#pragma unroll
          for (int d = 0; d < DP; ++d)
            if (EXACT || d < D) inner[d] = fmaf(p, qr[d], inner[d]);
        }
#pragma unroll
        for (int d = 0; d < DP; ++d) mid[d] += inner[d];
      }
#pragma unroll
      for (int d = 0; d < DP; ++d) outer[d] += mid[d];
    }
    if (live) {
      if (splits > 1) {
        float* out = partial + ((size_t)sp * M + j) * D;
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (EXACT || d < D) out[d] = mid[d];
      } else {
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (EXACT || d < D) dn[col * D + d] = isr::canonical(c * outer[d]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void combine_columns_kernel(const float* __restrict__ partial, long long splits, long long count,
                                                              double scale, long long rows, const float* __restrict__ g,
                                                              float* __restrict__ dn) {
  const float c = grad_scale(g ? *g : 1.f, scale, rows);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long long)gridDim.x * 256) {
    float outer = 0.f;
    for (long long sp = 0; sp < splits; ++sp) outer += partial[sp * count + e];
    dn[e] = isr::canonical(c * outer);
  }
}

struct Shape {
  long long B, S, rows;
  int M, D, Bn;
};

int check_call(const char* who, int64_t B, int64_t S, int64_t M, int D, int64_t Bn, Shape& sh) {
  const char* wrong = check_shape(B, S, M, D, Bn);
  ISR_REQUIRE(!wrong, "%s: %s (B %lld, S %lld, M %lld, D %d, Bn %lld)", who, wrong, (long long)B, (long long)S, (long long)M, D,
              (long long)Bn);
  sh = Shape{B, S, B * S, (int)M, D, Bn == 1 ? 1 : 0};     // Bn 1: shared negatives; 0: one set per batch item
  return ISR_OK;
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// the 1024-row ranges the column pass is split into (1: not split)
long long column_splits(const Shape& sh) {
  if (sh.Bn != 1) return 1;
  const long long ranges = ceil_div(sh.rows, kSuperRows);
  if (ranges < 2 || ceil_div(sh.M, kThreads) >= kSplitBelowBlocks) return 1;
  if ((size_t)ranges * sh.M * sh.D * 4 > kSplitBytes) return 1;
  return ranges;
}

// the first level reads the rows themselves: the buffers hold the sums from the second level on
size_t reduce_bytes(const Shape& sh, size_t* second) { return isr::reduce_bytes(ceil_div(sh.rows, kReduce), 1, second); }

size_t workspace_bytes(const Shape& sh) {
  const long long splits = column_splits(sh);
  const size_t split = splits > 1 ? isr::align_up((size_t)splits * sh.M * sh.D * 4, 256) : 0;
  const size_t red = reduce_bytes(sh, nullptr);
  return red > split ? red : split;
}

unsigned grid_of(long long items) { return (unsigned)(items < (long long)kMaxGrid ? items : (long long)kMaxGrid); }

#define ISR_CON_DISPATCH(D, CALL)                      \
  switch (pad_of(D)) {                                 \
    case 4: { constexpr int DP = 4; if ((D) == DP) { constexpr bool EX = true; CALL; } else { constexpr bool EX = false; CALL; } } break;   \
    case 12: { constexpr int DP = 12; if ((D) == DP) { constexpr bool EX = true; CALL; } else { constexpr bool EX = false; CALL; } } break; \
    case 16: { constexpr int DP = 16; if ((D) == DP) { constexpr bool EX = true; CALL; } else { constexpr bool EX = false; CALL; } } break; \
    case 32: { constexpr int DP = 32; if ((D) == DP) { constexpr bool EX = true; CALL; } else { constexpr bool EX = false; CALL; } } break; \
    default: { constexpr int DP = 64; if ((D) == DP) { constexpr bool EX = true; CALL; } else { constexpr bool EX = false; CALL; } } break; \
  }

}  // namespace

extern "C" size_t isr_contrastive_workspace_bytes(int64_t B, int64_t S, int64_t M, int D, int64_t Bn) {
  Shape sh;
  if (check_call("isr_contrastive_workspace_bytes", B, S, M, D, Bn, sh)) return 0;
  return workspace_bytes(sh);
}

extern "C" int isr_contrastive_geometry(int what) {
  switch (what) {
    case 0: return kThreads;       // rows of a row workgroup, columns of a column workgroup
    case 1: return kBlock;         // vectors of an LDS tile = terms of an inner chain
    case 2: return kSuperRows;     // rows of a middle accumulator = rows of a split range
    case 3: return kReduce;   // leaves of a reduce256 tree
    default: isr::set_error("isr_contrastive_geometry: what = %d", what); return 0;
  }
}

extern "C" int64_t isr_contrastive_column_splits(int64_t B, int64_t S, int64_t M, int D, int64_t Bn) {
  Shape sh;
  if (check_call("isr_contrastive_column_splits", B, S, M, D, Bn, sh)) return 0;
  return column_splits(sh);
}

extern "C" int isr_contrastive_forward(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D,
                                       int64_t Bn, double scale, float* m, float* t, float* pos, float* rows, float* loss,
                                       void* ws, size_t ws_bytes, isr_stream_t stream) {
  Shape sh;
  if (int rc = check_call("isr_contrastive_forward", B, S, M, D, Bn, sh)) return rc;
  ISR_REQUIRE(q && k && n && m && t && pos && rows && loss, "isr_contrastive_forward: null pointer");
  ISR_REQUIRE(ws && ws_bytes >= workspace_bytes(sh), "isr_contrastive_forward: workspace of %zu bytes, %zu needed", ws_bytes,
              workspace_bytes(sh));
  hipStream_t st = isr::as_stream(stream);
  const long long blocks_per_b = ceil_div(sh.S, kThreads), items = sh.B * blocks_per_b;
  ISR_CON_DISPATCH(D, (forward_kernel<DP, EX><<<grid_of(items), kThreads, 0, st>>>(q, k, n, sh.S, sh.M, D, sh.Bn, blocks_per_b,
                                                                                    items, m, t, pos, rows)));
  ISR_CHECK_LAUNCH("contrastive forward_kernel");
  size_t second;
  reduce_bytes(sh, &second);
  double* bufs[2] = {static_cast<double*>(ws), reinterpret_cast<double*>(static_cast<char*>(ws) + second)};
  return isr::reduce_levels<1>("contrastive reduce_kernel", rows, sh.rows, bufs, 0, LossFinish{scale, sh.rows}, loss, st);
}

extern "C" int isr_contrastive_backward(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D,
                                        int64_t Bn, double scale, const float* m, const float* t, const float* g_dev_or_null,
                                        float* dq, float* dk, float* dn, void* ws, size_t ws_bytes, isr_stream_t stream) {
  Shape sh;
  if (int rc = check_call("isr_contrastive_backward", B, S, M, D, Bn, sh)) return rc;
  ISR_REQUIRE(q && k && n && m && t, "isr_contrastive_backward: null pointer");
  ISR_REQUIRE(ws && ws_bytes >= workspace_bytes(sh), "isr_contrastive_backward: workspace of %zu bytes, %zu needed", ws_bytes,
              workspace_bytes(sh));
  hipStream_t st = isr::as_stream(stream);
  if (dq || dk) {
    const long long blocks_per_b = ceil_div(sh.S, kThreads), items = sh.B * blocks_per_b;
    ISR_CON_DISPATCH(D, (backward_rows_kernel<DP, EX><<<grid_of(items), kThreads, 0, st>>>(
                            q, k, n, sh.S, sh.M, D, sh.Bn, blocks_per_b, items, scale, sh.rows, m, t, g_dev_or_null, dq, dk)));
    ISR_CHECK_LAUNCH("contrastive backward_rows_kernel");
  }
  if (dn) {
    const long long col_blocks = ceil_div(sh.M, kThreads), splits = column_splits(sh);
    const long long items = (sh.Bn == 1 ? 1 : sh.B) * col_blocks * splits;
    float* partial = static_cast<float*>(ws);
    ISR_CON_DISPATCH(D, (backward_columns_kernel<DP, EX><<<grid_of(items), kThreads, 0, st>>>(
                            q, n, sh.S, sh.B, sh.M, D, sh.Bn, col_blocks, splits, items, scale, m, t, g_dev_or_null, dn, partial)));
    ISR_CHECK_LAUNCH("contrastive backward_columns_kernel");
    if (splits > 1) {
      const long long count = (long long)sh.M * sh.D;
      combine_columns_kernel<<<grid_of(ceil_div(count, 256)), 256, 0, st>>>(partial, splits, count, scale, sh.rows, g_dev_or_null, dn);
      ISR_CHECK_LAUNCH("contrastive combine_columns_kernel");
    }
  }
  return ISR_OK;
}

extern "C" int isr_contrastive_forward_host(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M,
                                            int D, int64_t Bn, double scale, float* m, float* t, float* pos, float* rows,
                                            float* loss) {
  Shape sh;
  if (int rc = check_call("isr_contrastive_forward_host", B, S, M, D, Bn, sh)) return rc;
  ISR_REQUIRE(q && k && n && m && t && pos && rows && loss, "isr_contrastive_forward_host: null pointer");
  isr::parallel_rows((long)sh.rows, 16, [=](long i) {
    const float* nb = n + (sh.Bn == 1 ? (size_t)0 : (size_t)(i / sh.S) * sh.M * D);
    forward_row(q + (size_t)i * D, k + (size_t)i * D, nb, sh.M, D, m + i, t + i, pos + i, rows + i);
  });
  std::vector<double> scratch((size_t)ceil_div(sh.rows, kReduce));
  *loss = loss_value(isr::ordered_sum(rows, sh.rows, scratch.data()), scale, sh.rows);
  return ISR_OK;
}

extern "C" int isr_contrastive_backward_host(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M,
                                             int D, int64_t Bn, double scale, const float* m, const float* t, const float* g_or_null,
                                             float* dq, float* dk, float* dn) {
  Shape sh;
  if (int rc = check_call("isr_contrastive_backward_host", B, S, M, D, Bn, sh)) return rc;
  ISR_REQUIRE(q && k && n && m && t, "isr_contrastive_backward_host: null pointer");
  const float c = grad_scale(g_or_null ? *g_or_null : 1.f, scale, sh.rows);
  if (dq || dk)
    isr::parallel_rows((long)sh.rows, 16, [=](long i) {
      const float* nb = n + (sh.Bn == 1 ? (size_t)0 : (size_t)(i / sh.S) * sh.M * D);
      backward_row(q + (size_t)i * D, k + (size_t)i * D, nb, sh.M, D, m[i], t[i], c, dq ? dq + (size_t)i * D : nullptr,
                   dk ? dk + (size_t)i * D : nullptr);
    });
  if (dn) {
    const long long sets = sh.Bn == 1 ? 1 : sh.B, set_rows = sh.Bn == 1 ? sh.rows : sh.S;
    isr::parallel_rows((long)(sets * sh.M), 16, [=](long e) {
      const size_t row0 = (size_t)(e / sh.M) * (sh.Bn == 1 ? 0 : sh.S);
      backward_column(q + row0 * D, m + row0, t + row0, set_rows, n + (size_t)e * D, D, c, dn + (size_t)e * D);
    });
  }
  return ISR_OK;
}
