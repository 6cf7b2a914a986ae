// field_grad.hip — the key field's backward (field_grad.hpp) and the device-side packing of a trainable field: the entries of
// include/isr_field_grad.h.  No call synchronises, no float atomics.
//
// grad_core.hpp has the scheme (slabs, batches, the dW and combine kernels, the words of a pack) and what it shares with the
// radiance field's backward.  The key field's own:
//   * field_grad_tile_kernel, field_mlp.hip's design (a workgroup, here of 8 waves, takes a tile of 64 points through every layer,
//     the activations in LDS): the forward again, leaving every layer's input h_{l-1} (S, in rounded up to 32) and slope
//     omega cos32(a) in the workspace, then the way down: g_l = u_l * slope over the slope's place, and u_{l-1} as a tile layer
//     over the transposed pack from a zero accumulator (mfma_tile_layer_from), in the same LDS.  Rows past N carry g = 0.
//   * the dW launch has one part per layer, none per ray; layer 0 reads its input from the caller's points (stride 3), and a
//     bias is the f32 chain of ones (grad_dw_kernel<false, kMaxLayers>, grad_combine_kernel<false>).
//   * field_pack_kernel writes the header words (omega, the sine flags) itself.
#include "field_grad.hpp"
#include "grad_core.hpp"

#include "../../include/isr_field_grad.h"

#include <vector>

namespace {

using namespace isr::field;
using isr::grad::for_tile;
using isr::grad::kFlat;
using isr::grad::ZeroInit;
using DwArgs = isr::grad::DwArgs<kMaxLayers>;

constexpr int kThreads = 512;                            // the tile kernel's workgroup: 8 waves, a neuron block each
constexpr int kActWords = (kMaxWidth / 2) * kTP * 2;      // 64 KB
constexpr int kInWords = kMfmaMinK * kTP;                 // 8 KB: the input of a vector-unit layer, k-major

static_assert(kGradChain == kTP, "a tile is a chain: grad_dw_kernel reads the 64 rows the tile kernel wrote");

// What the tile kernel takes: both layouts and, per layer, where the slab's h_{l-1} (S, ldh) and g_l (S, OP) are.
struct GradArgs {
  Layout lay, layT;
  float* h[kMaxLayers];
  float* g[kMaxLayers];
  int ldh[kMaxLayers];
};

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
    for_tile<kThreads>(L.OP, [&](int p, int j) { return act[act_index(j, p)]; }, [&](int p, int j, float a) {
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
    for_tile<kThreads>(L.OP, [&](int p, int j) { return (j < L.O && row0 + p < n) ? dout[(size_t)(row0 + p) * ld_dout + j] : 0.f; },
             [&](int p, int j, float u) { act[act_index(j, p)] = u; });
    __syncthreads();
  }
  for (int l = nl - 1; l >= 0; --l) {
    const Layer L = A.lay.L[l];
    const bool sine = pack_u[8 + l] != 0;
    float* G = A.g[l] + (size_t)row0 * L.OP;
    for_tile<kThreads>(L.OP, [&](int p, int j) { return sine ? G[p * L.OP + j] : 1.f; }, [&](int p, int j, float sv) {
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

struct PackArgs {
  Layout lay, layT;
  float omega[kMaxLayers];
  int sine[kMaxLayers];
  int w_std[kMaxLayers], b_std[kMaxLayers];
};

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
      bool done = false;
      for (int l = 0; l < nl && !done; ++l)
        done = isr::grad::pack_layer_word(P.lay.L[l], i, W, P.w_std[l], P.lay.L[l].K, 0, b, P.b_std[l], bits);
    }
    pack[i] = bits;
  } else if (i < total + P.layT.total_words) {
    const int t = i - total;
    uint32_t bits = 0u;
    bool done = false;
    for (int l = 1; l < nl && !done; ++l) done = isr::grad::pack_t_word(P.layT.L[l], t, W, P.w_std[l], P.lay.L[l].K, P.lay.L[l].O, bits);
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
  if (int rc = isr::grad::check_pack_t("isr_field_pack_device", P.lay, packT, packT_bytes, P.layT)) return rc;
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
  return carve(lay, isr::grad::slab_for(N), w_total + b_total, nullptr).bytes;
}

extern "C" int isr_field_backward(const void* pack, size_t pack_bytes, const void* packT, size_t packT_bytes, int n_layers,
                                  const int32_t* widths, const float* pts, int N, const float* dout, int ld_dout, float* dW,
                                  float* db, void* ws, size_t ws_bytes, isr_stream_t stream) {
  GradArgs A;
  if (int rc = check_field("isr_field_backward", pack, pack_bytes, n_layers, widths, A.lay)) return rc;
  if (int rc = isr::grad::check_pack_t("isr_field_backward", A.lay, packT, packT_bytes, A.layT)) return rc;
  if (int rc = check_io("isr_field_backward", A.lay, pts, N, dout, ld_dout)) return rc;
  int w_std[kMaxLayers], b_std[kMaxLayers];
  DwArgs D{};
  std_offsets(A.lay, w_std, b_std, &D.w_total, &D.b_total);
  const int E = D.w_total + D.b_total;
  hipStream_t st = isr::as_stream(stream);
  if (N == 0) return isr::grad::zero_grads(dW, D.w_total, db, D.b_total, st);
  ISR_REQUIRE(ws, "isr_field_backward: null workspace");
  int slab = isr::grad::slab_for(N);
  while (slab > kGradChain && carve(A.lay, slab, E, nullptr).bytes > ws_bytes) slab -= kGradChain;
  const Carve cv = carve(A.lay, slab, E, ws);
  ISR_REQUIRE(cv.bytes <= ws_bytes, "isr_field_backward: ws_bytes %zu, one chain of %d points needs %zu", ws_bytes, kGradChain, cv.bytes);
  for (int l = 0; l < kMaxLayers; ++l) {
    A.h[l] = l < n_layers ? cv.h[l] : nullptr;
    A.g[l] = l < n_layers ? cv.g[l] : nullptr;
    A.ldh[l] = l < n_layers ? cv.ldh[l] : 0;
    if (l >= n_layers) continue;
    const Layer& L = A.lay.L[l];                        // layer 0's input: the slab's points, set before each slab's launch
    isr::grad::add_part(D, cv.g[l], L.OP, L.O, l ? cv.h[l] : nullptr, l ? cv.ldh[l] : 3, L.K, 0, true, w_std[l], L.K, b_std[l]);
  }
  const float* pack_f = static_cast<const float*>(pack);
  const float* packT_f = static_cast<const float*>(packT);
  return isr::grad::for_slabs<false, kGradBatch>(D, N, slab, 1, cv.part, nullptr, cv.acc64, dW, db, st, [&](long s0, int n, long) -> int {
    D.L[0].h = pts + 3 * (size_t)s0;
    field_grad_tile_kernel<<<(n + kTP - 1) / kTP, kThreads, 0, st>>>(A, pack_f, packT_f, D.L[0].h, n, dout + (size_t)s0 * ld_dout, ld_dout);
    ISR_CHECK_LAUNCH("field_grad_tile_kernel");
    return ISR_OK;
  });
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
    if (dW) isr::grad::blocked_row<kMaxWidth>(G[l].data() + j, L.O, H[l].data(), L.K, 1, N, false, dW + w_std[l] + (size_t)j * L.K);
    if (db) isr::grad::blocked_row<kMaxWidth>(G[l].data() + j, L.O, nullptr, 1, 1, N, false, db + b_std[l] + j);
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
