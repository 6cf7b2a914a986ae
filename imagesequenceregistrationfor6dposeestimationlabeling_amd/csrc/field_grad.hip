// field_grad.hip — the key field's backward (field_grad.hpp) and the device-side packing of a trainable field: the entries of
// include/isr_field_grad.h.  No call synchronises, no float atomics.
//
// N is worked through in slabs of whole chains (kGradChain points): one launch of the first kernel per slab, then the other two
// per batch of kGradBatch of the slab's points:
//   * field_grad_tile_kernel, field_mlp.hip's design (a workgroup, here of 8 waves, takes a tile of 64 points through every layer,
//     the activations in LDS): the forward again, leaving every layer's input h_{l-1} (S, in rounded up to 32) and slope
//     omega cos32(a) in the workspace, then the way down: g_l = u_l * slope over the slope's place, and u_{l-1} as a tile layer
//     over the transposed pack from a zero accumulator (mfma_tile_layer_from), in the same LDS.  Rows past N carry g = 0.
//   * field_grad_dw_kernel, one wave per (32 x 32 block of a dW_l, chain): v_mfma_f32_32x32x2_f32 with the point as its k
//     index, A = g_l and B = h_{l-1} straight from the workspace (both are 128-byte rows per half wave), the accumulator from
//     +0: the chain of the rule.  Layers narrower than 32 on the input side and every db are the same chain on the vector
//     unit, a lane per entry.  A block sum goes to the workspace, real entries only, in the standard layout.
//   * field_grad_combine_kernel, a lane per entry: the batch's block sums onto an f64 accumulator that lives in the
//     workspace from batch to batch and slab to slab, in block order; the last one rounds to f32 and writes dW and db.
#include "field_grad.hpp"
#include "field_tile.hpp"
#include "isr_common.hpp"

#include "../../include/isr_field_grad.h"

#include <vector>

namespace {

using namespace isr::field;

constexpr int kThreads = 512;                            // the tile kernel's workgroup: 8 waves, a neuron block each
constexpr int kFlat = 256;                               // the per-entry kernels' workgroup
constexpr int kActWords = (kMaxWidth / 2) * kTP * 2;      // 64 KB
constexpr int kInWords = kMfmaMinK * kTP;                 // 8 KB: the input of a vector-unit layer, k-major

static_assert(kGradChain % kTP == 0 && kGradBatch % kGradChain == 0 && kGradSlab % kGradBatch == 0, "tiles make chains, chains make batches and slabs");

// What the kernels share: both layouts and, per layer, where the slab's h_{l-1} (S, ldh) and g_l (S, OP) are.
struct GradArgs {
  Layout lay, layT;
  float* h[kMaxLayers];
  float* g[kMaxLayers];
  int ldh[kMaxLayers];
};

// The work items of the dW launch: layer l owns items [first[l], first[l + 1]), the matrix-core blocks first (nmf[l]).
struct DwArgs {
  int first[kMaxLayers + 1];
  int nmf[kMaxLayers];
  int w_std[kMaxLayers], b_std[kMaxLayers];
  int E, w_total;
};

struct ZeroInit {
  __device__ __forceinline__ float operator()(int, int) const { return 0.f; }
};

// Every (point, neuron) pair of the tile below OP over the workgroup, a wave step 8 points x 8 neurons (32-byte pieces of the
// workspace's rows, four LDS words per bank of the k-pair-major tile): v = load(point, neuron) for a batch of steps at once,
// so that their memory latencies overlap, then f(point, neuron, v) for each.  OP is a multiple of 32, a batch of every wave.
template <class Ld, class F>
__device__ __forceinline__ void for_tile(int OP, Ld load, F f) {
  constexpr int kWaves = kThreads / 64, kBatch = 32 / kWaves;
  static_assert(kBatch * kWaves == 32, "a batch of every wave covers 32 steps, which divides every OP");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, pl = lane >> 3, jl = lane & 7;
  for (int item0 = w; item0 < OP; item0 += kBatch * kWaves) {
    float v[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int item = item0 + i * kWaves;
      v[i] = load((item & 7) * 8 + pl, (item >> 3) * 8 + jl);
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int item = item0 + i * kWaves;
      f((item & 7) * 8 + pl, (item >> 3) * 8 + jl, v[i]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void field_grad_tile_kernel(GradArgs A, const float* __restrict__ pack,
                                                                   const float* __restrict__ packT,
                                                                   const float* __restrict__ pts, int n,
                                                                   const float* __restrict__ dout, int ld_dout) {
  __shared__ float act[kActWords];
  __shared__ float inb[kInWords];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kTP;
  const uint32_t* pack_u = reinterpret_cast<const uint32_t*>(pack);
  const int nl = A.lay.n_layers;

  if (w < 3) {
    const int row = row0 + lane;
    inb[w * kTP + lane] = row < n ? pts[3 * (size_t)row + w] : 0.f;
  }
  __syncthreads();

  // the forward: act holds a layer's angles a (z of a linear layer), then its outputs
  for (int l = 0; l < nl; ++l) {
    const Layer L = A.lay.L[l];
    const float omega = pack[l];
    const bool sine = pack_u[8 + l] != 0;
    const auto angle = [=](float z) { return sine ? omega * z : z; };
    if (!L.mfma) {
      const float* Wl = pack + L.w_off;
      const float* bl = pack + L.b_off;
      if (l > 0) {
        for (int i = tid; i < L.K * kTP; i += kThreads) {
          const int k = i >> 6, p = i & 63;
          inb[i] = act[act_index(k, p)];
        }
        __syncthreads();
      }
      const int p = lane;
      for (int jp = w; jp < L.OP / 2; jp += kThreads / 64) {
        const int j0 = 2 * jp;
        const float* w0 = Wl + j0 * L.kstride;
        const float* w1 = w0 + L.kstride;
        float z0 = bl[j0], z1 = bl[j0 + 1];
        for (int k = 0; k < L.K; ++k) {
          const float hk = inb[k * kTP + p];
          z0 = fmaf(w0[k], hk, z0);
          z1 = fmaf(w1[k], hk, z1);
        }
        *reinterpret_cast<float2*>(&act[act_index(j0, p)]) = make_float2(j0 < L.O ? angle(z0) : 0.f, j0 + 1 < L.O ? angle(z1) : 0.f);
      }
      __syncthreads();
    } else {
      mfma_tile_layer<kThreads / 64>(L, pack, act, false, angle);
    }
    float* S = A.g[l] + (size_t)row0 * L.OP;
    float* Hn = l + 1 < nl ? A.h[l + 1] + (size_t)row0 * L.OP : nullptr;      // ldh[l + 1] is this layer's OP
    for_tile(L.OP, [&](int p, int j) { return act[act_index(j, p)]; }, [&](int p, int j, float a) {
      float hv = 0.f, sv = 0.f;
      if (j < L.O) {
        if (sine) {
          float sn, cs;
          sin_cos32(a, &sn, &cs);
          hv = sn;
          sv = omega * cs;
        } else {
          hv = a;
          sv = 1.f;
        }
      }
      act[act_index(j, p)] = hv;
      S[p * L.OP + j] = sv;
      if (Hn) Hn[p * L.OP + j] = hv;
    });
    __syncthreads();
  }

  // the way down: act holds u_l, then g_l, then u_{l-1}
  {
    const Layer L = A.lay.L[nl - 1];
    for_tile(L.OP, [&](int p, int j) { return (j < L.O && row0 + p < n) ? dout[(size_t)(row0 + p) * ld_dout + j] : 0.f; },
             [&](int p, int j, float u) { act[act_index(j, p)] = u; });
    __syncthreads();
  }
  for (int l = nl - 1; l >= 0; --l) {
    const Layer L = A.lay.L[l];
    const bool sine = pack_u[8 + l] != 0;
    float* G = A.g[l] + (size_t)row0 * L.OP;
    for_tile(L.OP, [&](int p, int j) { return sine ? G[p * L.OP + j] : 1.f; }, [&](int p, int j, float sv) {
      const int idx = act_index(j, p);
      float gv = 0.f;
      if (j < L.O && row0 + p < n) {
        const float u = act[idx];
        gv = sine ? u * sv : u;
      }
      act[idx] = gv;
      G[p * L.OP + j] = gv;
    });
    __syncthreads();
    if (l == 0) break;
    const Layer T = A.layT.L[l];
    if (T.mfma) {
      mfma_tile_layer_from<kThreads / 64>(T, packT, act, false, [](float z) { return z; }, ZeroInit{});
    } else {                        // K_l < 32: the chain on the vector unit, the transposed rows wave-uniform
      const float* WT = packT + T.w_off;
      const int p = lane;
      for (int k = w; k < L.K; k += kThreads / 64) {
        const float* wr = WT + k * T.kstride;
        float acc = 0.f;
        for (int j = 0; j < L.O; ++j) acc = fmaf(wr[j], act[act_index(j, p)], acc);
        inb[k * kTP + p] = acc;
      }
      __syncthreads();
      for (int i = tid; i < T.OP * kTP; i += kThreads) {
        const int k = i >> 6, pp = i & 63;
        act[act_index(k, pp)] = k < L.K ? inb[i] : 0.f;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64) void field_grad_dw_kernel(GradArgs A, DwArgs D, const float* __restrict__ pts, int n, int chain0,
                                                           float* __restrict__ part) {
  const int lane = threadIdx.x, c = blockIdx.y;                         // chain chain0 + c of the slab, the batch's c-th
  int item = blockIdx.x, l = 0;
  while (item >= D.first[l + 1]) ++l;
  item -= D.first[l];
  const Layer L = A.lay.L[l];
  const int p0 = (chain0 + c) * kGradChain;
  const int left = n - p0;
  const int real = left < kGradChain ? left : kGradChain;               // the chain's points
  const int padded = (real + kTP - 1) / kTP * kTP;                      // and the rows the tile kernel wrote (g = 0 past n)
  const float* G = A.g[l] + (size_t)p0 * L.OP;
  float* out = part + (size_t)c * D.E;
  if (item < D.nmf[l]) {
    const int KB = (L.K + 31) / 32, jb = item / KB, kb = item - jb * KB;
    const int r = lane & 31, hh = lane >> 5, ldh = A.ldh[l];
    const float* ga = G + (size_t)hh * L.OP + jb * 32 + r;
    const float* hb = A.h[l] + (size_t)(p0 + hh) * ldh + kb * 32 + r;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int s0 = 0; s0 < padded / 2; s0 += 8) {        // a tile's rows are 32 steps: eight loads of each operand in flight
      float av[8], bv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        av[i] = ga[(size_t)2 * (s0 + i) * L.OP];
        bv[i] = hb[(size_t)2 * (s0 + i) * ldh];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
    }
    const int k = kb * 32 + r;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = jb * 32 + 8 * a + 4 * hh + b;
        if (j < L.O && k < L.K) out[D.w_std[l] + j * L.K + k] = acc[4 * a + b];
      }
    return;
  }
  // the vector unit: a lane per entry.  A matrix-core layer leaves its bias here; a narrow one its K + 1 columns.
  const int e = (item - D.nmf[l]) * 64 + lane;
  const int cols = L.mfma ? 1 : L.K + 1;
  if (e >= L.O * cols) return;
  const int j = e / cols, k = L.mfma ? L.K : e - j * cols;
  const float* hp = nullptr;
  int hs = 0;
  if (k < L.K) {
    hp = l == 0 ? pts + (size_t)p0 * 3 + k : A.h[l] + (size_t)p0 * A.ldh[l] + k;
    hs = l == 0 ? 3 : A.ldh[l];
  }
  float acc = 0.f;
  for (int nn = 0; nn < real; ++nn) acc = fmaf(G[(size_t)nn * L.OP + j], hp ? hp[(size_t)nn * hs] : 1.f, acc);
  if (k < L.K) out[D.w_std[l] + j * L.K + k] = acc;
  else out[D.w_total + D.b_std[l] + j] = acc;
}

__global__ __launch_bounds__(kFlat) void field_grad_combine_kernel(const float* __restrict__ part, int nblk, int E, int w_total,
                                                                      double* __restrict__ acc64, int first, int last,
                                                                      float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * kFlat + threadIdx.x;
  if (e >= E) return;
  double acc = first ? 0.0 : acc64[e];
  for (int c = 0; c < nblk; ++c) acc += (double)part[(size_t)c * E + e];
  acc64[e] = acc;
  if (!last) return;
  if (e < w_total) {
    if (dW) dW[e] = (float)acc;
  } else if (db) {
    db[e - w_total] = (float)acc;
  }
}

struct PackArgs {
  Layout lay, layT;
  float omega[kMaxLayers];
  int sine[kMaxLayers];
  int w_std[kMaxLayers], b_std[kMaxLayers];
};

// the inverse of w_index: word idx of a layer's weight block -> (j, k), padding included
__device__ __forceinline__ void w_unindex(const Layer& L, int idx, int& j, int& k) {
  if (!L.mfma) {
    j = idx / L.kstride;
    k = idx - j * L.kstride;
    return;
  }
  const int q = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8, S8 = L.kstride >> 3;
  k = (blk % S8) * 8 + 2 * q + (lane >> 5);
  j = (blk / S8) * 32 + (lane & 31);
}

// a thread per word of the two packs: its source entry, or zero
__global__ __launch_bounds__(kFlat) void field_pack_kernel(PackArgs P, const uint32_t* __restrict__ W,
                                                              const uint32_t* __restrict__ b, uint32_t* __restrict__ pack,
                                                              uint32_t* __restrict__ packT) {
  const int i = blockIdx.x * kFlat + threadIdx.x;
  const int total = P.lay.total_words, nl = P.lay.n_layers;
  if (i < total) {
    uint32_t bits = 0u;
    if (i < kHeaderWords) {
      if (i < nl && P.sine[i]) bits = __float_as_uint(P.omega[i]);
      if (i >= 8 && i - 8 < nl && P.sine[i - 8]) bits = 1u;
    } else {
      for (int l = 0; l < nl; ++l) {
        const Layer L = P.lay.L[l];
        if (i >= L.w_off && i < L.b_off) {
          int j, k;
          w_unindex(L, i - L.w_off, j, k);
          if (j < L.O && k < L.K) bits = W[P.w_std[l] + j * L.K + k];
        } else if (i >= L.b_off && i < L.b_off + L.O) {
          bits = b[P.b_std[l] + i - L.b_off];
        }
      }
    }
    pack[i] = bits;
  } else if (i < total + P.layT.total_words) {
    const int t = i - total;
    uint32_t bits = 0u;
    for (int l = 1; l < nl; ++l) {
      const Layer T = P.layT.L[l];
      const Layer L = P.lay.L[l];
      if (t >= T.w_off && t < T.b_off) {
        int k, j;
        w_unindex(T, t - T.w_off, k, j);        // T's neuron is W's input k, T's input W's neuron j
        if (k < L.K && j < L.O) bits = W[P.w_std[l] + j * L.K + k];
      }
    }
    packT[t] = bits;
  }
}

// the checks every entry shares; on success lay is filled
int check_field(const char* who, const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, Layout& lay) {
  if (int rc = isr::check_pack_pointers(who, pack, widths)) return rc;
  ISR_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: %d layers (1..%d)", who, n_layers, kMaxLayers);
  ISR_REQUIRE(make_layout(n_layers, widths, lay),
              "%s: widths out of range (widths[0] = 3, every width in 1..%d, the last at most %d)", who, kMaxWidth, kMaxOut);
  return isr::check_pack_bytes(who, pack_bytes, lay.total_words);
}

int check_pack_t(const char* who, const Layout& lay, const void* packT, size_t packT_bytes, Layout& layT) {
  make_layout_t(lay, layT);
  ISR_REQUIRE(packT, "%s: null pointer", who);
  ISR_REQUIRE(packT_bytes == (size_t)layT.total_words * 4, "%s: packT_bytes %zu, this field's transposed pack has %zu", who,
              packT_bytes, (size_t)layT.total_words * 4);
  return ISR_OK;
}

int check_io(const char* who, const Layout& lay, const float* pts, int N, const float* dout, int ld_dout) {
  if (int rc = isr::check_rows(who, N, pts && dout)) return rc;
  ISR_REQUIRE(ld_dout >= lay.L[lay.n_layers - 1].O, "%s: ld_dout %d < out width %d", who, ld_dout, lay.L[lay.n_layers - 1].O);
  return ISR_OK;
}

// The workspace of a slab of `slab` points: where everything is from `base` on, and how many bytes that takes.
struct Carve {
  double* acc64;
  float* part;
  float* h[kMaxLayers];
  float* g[kMaxLayers];
  int ldh[kMaxLayers];
  size_t bytes;
};

Carve carve(const Layout& lay, int slab, int E, void* base) {
  Carve c;
  isr::Workspace ws(base, 0);
  c.acc64 = ws.take<double>((size_t)E);
  c.part = ws.take<float>((size_t)((slab < kGradBatch ? slab : kGradBatch) / kGradChain) * E);
  for (int l = 0; l < lay.n_layers; ++l) {
    c.ldh[l] = l ? lay.L[l - 1].OP : 0;
    c.h[l] = l ? ws.take<float>((size_t)slab * c.ldh[l]) : nullptr;
    c.g[l] = ws.take<float>((size_t)slab * lay.L[l].OP);
  }
  c.bytes = isr::align_up(ws.off, 256);
  return c;
}

int slab_for(int N) {
  const long up = ((long)N + kGradChain - 1) / kGradChain * kGradChain;
  return up < kGradChain ? kGradChain : up > kGradSlab ? kGradSlab : (int)up;
}

bool layout_of(int n_layers, const int32_t* widths, Layout& lay) {
  return widths && n_layers >= 1 && n_layers <= kMaxLayers && make_layout(n_layers, widths, lay);
}

}  // namespace

extern "C" size_t isr_field_grad_pack_bytes(int n_layers, const int32_t* widths) {
  Layout lay, layT;
  if (!layout_of(n_layers, widths, lay)) {
    isr::set_error("isr_field_grad_pack_bytes: null widths, or a layer count (1..%d) or width (3, then 1..%d, the last <= %d) out of range",
                   kMaxLayers, kMaxWidth, kMaxOut);
    return 0;
  }
  make_layout_t(lay, layT);
  return (size_t)layT.total_words * 4;
}

extern "C" int isr_field_pack_device(int n_layers, const int32_t* widths, const float* W, const float* b, const float* omega,
                                     const int32_t* sine, void* pack, size_t pack_bytes, void* packT, size_t packT_bytes,
                                     isr_stream_t stream) {
  PackArgs P;
  if (int rc = check_field("isr_field_pack_device", pack, pack_bytes, n_layers, widths, P.lay)) return rc;
  if (int rc = check_pack_t("isr_field_pack_device", P.lay, packT, packT_bytes, P.layT)) return rc;
  ISR_REQUIRE(W && b && omega && sine, "isr_field_pack_device: null pointer");
  int w_total, b_total;
  std_offsets(P.lay, P.w_std, P.b_std, &w_total, &b_total);
  for (int l = 0; l < kMaxLayers; ++l) {
    P.omega[l] = l < n_layers ? omega[l] : 0.f;
    P.sine[l] = l < n_layers && sine[l] ? 1 : 0;
  }
  const int words = P.lay.total_words + P.layT.total_words;
  field_pack_kernel<<<(words + kFlat - 1) / kFlat, kFlat, 0, isr::as_stream(stream)>>>(
      P, reinterpret_cast<const uint32_t*>(W), reinterpret_cast<const uint32_t*>(b), static_cast<uint32_t*>(pack),
      static_cast<uint32_t*>(packT));
  ISR_CHECK_LAUNCH("field_pack_kernel");
  return ISR_OK;
}

extern "C" size_t isr_field_grad_workspace_bytes(int n_layers, const int32_t* widths, int N) {
  Layout lay;
  if (!layout_of(n_layers, widths, lay) || N < 0) {
    isr::set_error("isr_field_grad_workspace_bytes: null widths, N < 0, or a layer count (1..%d) or width (3, then 1..%d, the last <= %d) "
                   "out of range", kMaxLayers, kMaxWidth, kMaxOut);
    return 0;
  }
  int w_std[kMaxLayers], b_std[kMaxLayers], w_total, b_total;
  std_offsets(lay, w_std, b_std, &w_total, &b_total);
  return carve(lay, slab_for(N), w_total + b_total, nullptr).bytes;
}

extern "C" int isr_field_backward(const void* pack, size_t pack_bytes, const void* packT, size_t packT_bytes, int n_layers,
                                  const int32_t* widths, const float* pts, int N, const float* dout, int ld_dout, float* dW,
                                  float* db, void* ws, size_t ws_bytes, isr_stream_t stream) {
  GradArgs A;
  if (int rc = check_field("isr_field_backward", pack, pack_bytes, n_layers, widths, A.lay)) return rc;
  if (int rc = check_pack_t("isr_field_backward", A.lay, packT, packT_bytes, A.layT)) return rc;
  if (int rc = check_io("isr_field_backward", A.lay, pts, N, dout, ld_dout)) return rc;
  DwArgs D;
  int b_total;
  std_offsets(A.lay, D.w_std, D.b_std, &D.w_total, &b_total);
  D.E = D.w_total + b_total;
  hipStream_t st = isr::as_stream(stream);
  if (N == 0) {
    if (dW) ISR_CHECK_HIP(hipMemsetAsync(dW, 0, (size_t)D.w_total * 4, st));
    if (db) ISR_CHECK_HIP(hipMemsetAsync(db, 0, (size_t)b_total * 4, st));
    return ISR_OK;
  }
  ISR_REQUIRE(ws, "isr_field_backward: null workspace");
  int slab = slab_for(N);
  while (slab > kGradChain && carve(A.lay, slab, D.E, nullptr).bytes > ws_bytes) slab -= kGradChain;
  const Carve cv = carve(A.lay, slab, D.E, ws);
  ISR_REQUIRE(cv.bytes <= ws_bytes, "isr_field_backward: ws_bytes %zu, one chain of %d points needs %zu", ws_bytes, kGradChain, cv.bytes);
  D.first[0] = 0;
  for (int l = 0; l < kMaxLayers; ++l) {
    A.h[l] = l < n_layers ? cv.h[l] : nullptr;
    A.g[l] = l < n_layers ? cv.g[l] : nullptr;
    A.ldh[l] = l < n_layers ? cv.ldh[l] : 0;
    if (l < n_layers) {
      const Layer& L = A.lay.L[l];
      D.nmf[l] = L.mfma ? (L.OP / 32) * ((L.K + 31) / 32) : 0;
      D.first[l + 1] = D.first[l] + D.nmf[l] + (L.O * (L.mfma ? 1 : L.K + 1) + 63) / 64;
    } else {
      D.nmf[l] = D.w_std[l] = D.b_std[l] = 0;
      D.first[l + 1] = D.first[l];
    }
  }
  const float* pack_f = static_cast<const float*>(pack);
  const float* packT_f = static_cast<const float*>(packT);
  for (long s0 = 0; s0 < N; s0 += slab) {
    const int n = N - s0 < slab ? (int)(N - s0) : slab;
    const float* p = pts + 3 * (size_t)s0;
    field_grad_tile_kernel<<<(n + kTP - 1) / kTP, kThreads, 0, st>>>(A, pack_f, packT_f, p, n, dout + (size_t)s0 * ld_dout, ld_dout);
    ISR_CHECK_LAUNCH("field_grad_tile_kernel");
    for (int b0 = 0; b0 < n; b0 += kGradBatch) {
      const int nb = n - b0 < kGradBatch ? n - b0 : kGradBatch;
      const int nblk = (nb + kGradChain - 1) / kGradChain;
      field_grad_dw_kernel<<<dim3(D.first[n_layers], nblk), 64, 0, st>>>(A, D, p, n, b0 / kGradChain, cv.part);
      ISR_CHECK_LAUNCH("field_grad_dw_kernel");
      field_grad_combine_kernel<<<(D.E + kFlat - 1) / kFlat, kFlat, 0, st>>>(cv.part, nblk, D.E, D.w_total, cv.acc64, s0 + b0 == 0,
                                                                           s0 + b0 + nb == N, dW, db);
      ISR_CHECK_LAUNCH("field_grad_combine_kernel");
    }
  }
  return ISR_OK;
}

extern "C" int isr_field_backward_host(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts,
                                       int N, const float* dout, int ld_dout, float* dW, float* db) {
  Layout lay;
  if (int rc = check_field("isr_field_backward_host", pack, pack_bytes, n_layers, widths, lay)) return rc;
  if (int rc = check_io("isr_field_backward_host", lay, pts, N, dout, ld_dout)) return rc;
  int w_std[kMaxLayers], b_std[kMaxLayers], w_total, b_total;
  std_offsets(lay, w_std, b_std, &w_total, &b_total);
  std::vector<std::vector<float>> dense(n_layers), H(n_layers), G(n_layers);
  const float* rows[kMaxLayers];
  std::vector<int> row_layer;
  for (int l = 0; l < n_layers; ++l) {
    dense[l].resize((size_t)lay.L[l].O * lay.L[l].K);
    unpack_layer(lay.L[l], static_cast<const float*>(pack), dense[l].data(), false);
    rows[l] = dense[l].data();
    H[l].resize((size_t)N * lay.L[l].K);
    G[l].resize((size_t)N * lay.L[l].O);
    for (int j = 0; j < lay.L[l].O; ++j) row_layer.push_back(l);
  }
  // points are independent up to the sums: g and h of every point first, then a row of a dW_l (and its db) at a time
  isr::parallel_rows(N, 64, [&](long n) {
    float *hp[kMaxLayers], *gp[kMaxLayers];
    for (int l = 0; l < n_layers; ++l) {
      hp[l] = H[l].data() + (size_t)n * lay.L[l].K;
      gp[l] = G[l].data() + (size_t)n * lay.L[l].O;
    }
    point_grads(lay, pack, rows, pts + 3 * (size_t)n, dout + (size_t)n * ld_dout, hp, gp);
  });
  isr::parallel_rows((long)row_layer.size(), 8, [&](long r) {
    const int l = row_layer[r], j = (int)r - b_std[l];
    const Layer& L = lay.L[l];
    if (dW) blocked_row(G[l].data() + j, L.O, H[l].data(), L.K, N, dW + w_std[l] + (size_t)j * L.K);
    if (db) db[b_std[l] + j] = blocked_sum(G[l].data() + j, L.O, nullptr, 0, N);
  });
  return ISR_OK;
}

extern "C" int isr_field_cos_host(const float* a, size_t n, float* out) {
  ISR_REQUIRE(n == 0 || (a && out), "isr_field_cos_host: null pointer");
  for (size_t i = 0; i < n; ++i) out[i] = cos32(a[i]);
  return ISR_OK;
}

extern "C" int isr_field_grad_geometry(int which) {
  return which == 0 ? kGradChain : which == 1 ? kTP : which == 2 ? kGradSlab : which == 3 ? kGradBatch : -1;
}
