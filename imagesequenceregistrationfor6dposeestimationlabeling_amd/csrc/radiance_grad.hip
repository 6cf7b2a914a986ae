// radiance_grad.hip — the radiance field's backward (radiance_grad.hpp) and the device-side packing of a trainable field:
// the entries of include/isr_radiance_grad.h.  No call synchronises, no float atomics.
//
// grad_core.hpp has the scheme (slabs, batches, the dW and combine kernels, the words of a pack) and what it shares with the
// key field's backward.  The radiance field's own, per slab of the N * P points in memory order:
//   * radiance_grad_dir_kernel, 64 of the slab's RAYS per workgroup (field_radiance.hip's radiance_dir_kernel): the
//     embedding e_dir of the normalised direction into the workspace (rays, 6H rounded up to 32) and the direction term u, the
//     chain from b1 over W1's direction columns on the matrix cores (rays, Wc rounded up to 32).
//   * radiance_grad_tile_kernel, field_trunk.hpp's scheme (8 waves take 64 points through every layer, the activations in
//     LDS): the forward again — the points of the tile from their rays, the embedding, the hidden layers, the density neuron,
//     colour layer 1 from u[ray of the point] and colour layer 2 — leaving every layer's input and slope32 in the workspace,
//     then the way down: g = u * slope over the slope's place and u of the layer below as a tile layer over the transposed
//     pack (mfma_tile_layer_from; u_top starts from w_out[k] * g_o).  A TILE IS 64 CONSECUTIVE POINTS IN MEMORY ORDER, not whole
//     rays as in the render: the sums are chains over points in memory order and a slab boundary cuts a ray, so the tile is
//     the chain; a point's ray is its index / P.  Rows past the end carry g = 0.
//     LDS: the 96 KB activation buffer of the trunk scheme, 768 bytes of points and 256 bytes of g_o: one workgroup per CU.
//   * the dW launch has a part per hidden layer, the density row, W1's trunk columns, W1's direction columns (a per-ray input:
//     e_dir[ray of the point]) and W2, and a bias is the f64 sum (grad_dw_kernel<true, kMaxDw>, grad_combine_kernel<true>).
//   * radiance_pack_kernel writes the header words (beta, H, the layer count, the frequencies) and the density row itself.
#include "radiance_grad.hpp"
#include "field_trunk.hpp"
#include "grad_core.hpp"

#include "../../include/isr_radiance_grad.h"

#include <vector>

namespace {

using namespace isr::radiance;
using isr::density::check_march;
using isr::density::kActWords;
using isr::density::kMaxHidden;
using isr::density::kThreads;
using isr::density::softplus32;
using isr::density::tile_embed;
using isr::field::act_index;
using isr::field::kTP;
using isr::grad::add_part;
using isr::grad::for_tile;
using isr::grad::kFlat;
using isr::grad::pack_layer_word;
using isr::grad::pack_t_word;
using isr::grad::ZeroInit;

constexpr int kMaxDw = kMaxHidden + 4;      // hidden layers, density row, W1's trunk part, W1's direction part, W2
using DwArgs = isr::grad::DwArgs<kMaxDw>;

static_assert(kGradChain == kTP, "a tile is a chain");

// What the tile kernel leaves in the slab workspace (S rows each; widths rounded up to 32).
struct TileArgs {
  Layout lay;
  GradLayout T;
  float* e;                  // (S, ldE): the embedding of the point
  float* h[kMaxHidden];      // (S, OP_l): the output of hidden layer l
  float* g[kMaxHidden];      // (S, OP_l): its slope, then g_l
  float* a1;                 // (S, WcP): colour layer 1's activations
  float* g1;                 // (S, WcP): its slope, then g1
  float* q;                  // (S, 32)
  float* go;                 // (S)
  float* u;                  // (R, WcP): the direction terms of the slab's rays
  float* edir;               // (R, ldE): their embeddings
  int ldE;
};

// where colour layer 1's chains start: u of the point's ray.  k0: the slab's first point's sample index within its ray
struct RayTermInit {
  const float* u;
  int row0, last, k0, P, WcP;      // last: the slab's last point (rows past it take its ray)
  __device__ __forceinline__ float operator()(int j, int p) const {
    const int row = row0 + p < last ? row0 + p : last;
    return u[(size_t)((k0 + row) / P) * WcP + j];
  }
};

// where u_top's chains start: w_out[k] * g_o of the point, one f32 product
struct DensityInit {
  const float* wo;
  const float* go;      // LDS, the tile's
  int Wt;
  __device__ __forceinline__ float operator()(int k, int p) const { return k < Wt ? wo[k] * go[p] : 0.f; }
};

// e_dir (R, ldE) and u (R, WcP) of the rays [ray_base, ray_base + R): 64 rays per workgroup
__global__ __launch_bounds__(kThreads) void radiance_grad_dir_kernel(Layout lay, const float* __restrict__ pack,
                                                                     const float* __restrict__ directions, long ray_base, int R,
                                                                     float* __restrict__ u, float* __restrict__ edir, int ldE) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kTP;
  if (tid < kTP) {
    float d[3] = {0.f, 0.f, 0.f}, dn[3];
    if (r0 + tid < R)
      for (int i = 0; i < 3; ++i) d[i] = directions[3 * (ray_base + r0 + tid) + i];
    normalize3(d, dn);
    for (int i = 0; i < 3; ++i) ptl[i * kTP + tid] = dn[i];
  }
  __syncthreads();
  tile_embed(lay.d.H, lay.dir.kstride, pack, act, ptl);
  const int E = 6 * lay.d.H;
  for (int i = tid; i < kTP * ldE; i += kThreads) {
    const int p = i / ldE, k = i - p * ldE;
    if (r0 + p < R) edir[(size_t)(r0 + p) * ldE + k] = k < E ? act[act_index(k, p)] : 0.f;
  }
  isr::field::mfma_tile_layer<kThreads / 64>(lay.dir, pack, act, true, [](float z) { return z; });      // act[p * Wc + j]
  for (int i = tid; i < kTP * lay.WcP; i += kThreads) {
    const int p = i / lay.WcP, j = i - p * lay.WcP;
    if (r0 + p < R) u[(size_t)(r0 + p) * lay.WcP + j] = j < lay.Wc ? act[p * lay.Wc + j] : 0.f;
  }
}

// the slab's points [s0, s0 + n) of the bundle, 64 per workgroup; ray_base = s0 / P
__global__ __launch_bounds__(kThreads) void radiance_grad_tile_kernel(TileArgs A, const float* __restrict__ pack,
                                                                      const float* __restrict__ packT,
                                                                      const float* __restrict__ origins,
                                                                      const float* __restrict__ directions,
                                                                      const float* __restrict__ lengths, long s0, int n, int P,
                                                                      long ray_base, const float* __restrict__ d_dens,
                                                                      const float* __restrict__ d_col) {
  __shared__ float act[kActWords];
  __shared__ float ptl[3 * kTP];
  __shared__ float gol[kTP];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * kTP;
  const float beta = pack[0];
  const int nh = A.lay.d.n_hidden, C = A.lay.C, Wc = A.lay.Wc, WcP = A.lay.WcP;
  const auto ident = [](float z) { return z; };

  if (tid < 3 * kTP) {
    const int d = tid >> 6, row = row0 + (tid & 63);
    float v = 0.f;                                   // rows past the end: the origin
    if (row < n) {
      const long ng = s0 + row, ray = ng / P;
      v = origins[3 * ray + d] + directions[3 * ray + d] * lengths[ng];
    }
    ptl[tid] = v;
  }
  __syncthreads();
  tile_embed(A.lay.d.H, A.lay.d.L[0].kstride, pack, act, ptl);
  {
    const int E = 6 * A.lay.d.H, ldE = A.ldE;
    float* Er = A.e + (size_t)row0 * ldE;
    for_tile<kThreads>(ldE, [&](int p, int k) { return k < E ? act[act_index(k, p)] : 0.f; }, [&](int p, int k, float v) { Er[p * ldE + k] = v; });
  }

  // the forward: act holds a layer's z, then its activations
  for (int l = 0; l < nh; ++l) {
    const Layer L = A.lay.d.L[l];
    isr::field::mfma_tile_layer<kThreads / 64>(L, pack, act, false, ident);
    float* Hn = A.h[l] + (size_t)row0 * L.OP;
    float* S = A.g[l] + (size_t)row0 * L.OP;
    for_tile<kThreads>(L.OP, [&](int p, int j) { return act[act_index(j, p)]; }, [&](int p, int j, float z) {
      float hv = 0.f, sv = 0.f;
      if (j < L.O) {
        hv = softplus32(z, beta);
        sv = slope32(z, beta);
      }
      act[act_index(j, p)] = hv;
      Hn[p * L.OP + j] = hv;
      S[p * L.OP + j] = sv;
    });
    __syncthreads();
  }
  if (w == 0) {                   // the density neuron's chain, lane = point (tile_trunk's); the next layer reads act first
    const float* wo = pack + A.lay.d.out_w_off;
    float z = pack[A.lay.d.out_b_off];
    for (int k = 0; k < A.lay.d.out_K; ++k) z = fmaf(wo[k], act[act_index(k, lane)], z);
    const int row = row0 + lane;
    float gv = 0.f;
    if (row < n) {
      const float dr = d_dens ? d_dens[s0 + row] : 0.f;
      gv = (dr * dexp32(softplus32(z, beta))) * slope32(z, beta);
    }
    gol[lane] = gv;
    A.go[row0 + lane] = gv;
  }
  isr::field::mfma_tile_layer_from<kThreads / 64>(A.lay.trunk, pack, act, false, ident,
                                                  RayTermInit{A.u, row0, n - 1, (int)(s0 - ray_base * P), P, WcP});
  {
    float* A1 = A.a1 + (size_t)row0 * WcP;
    float* S = A.g1 + (size_t)row0 * WcP;
    for_tile<kThreads>(WcP, [&](int p, int j) { return act[act_index(j, p)]; }, [&](int p, int j, float z) {
      float hv = 0.f, sv = 0.f;
      if (j < Wc) {
        hv = softplus32(z, beta);
        sv = slope32(z, beta);
      }
      act[act_index(j, p)] = hv;
      A1[p * WcP + j] = hv;
      S[p * WcP + j] = sv;
    });
    __syncthreads();
  }
  isr::field::mfma_tile_layer<kThreads / 64>(A.lay.out, pack, act, false, [](float z) { return sigmoid32(z); });

  // the way down: act holds q, then u of a layer, then its g
  {
    float* Q = A.q + (size_t)row0 * 32;
    for_tile<kThreads>(32, [&](int p, int c) { return (c < C && row0 + p < n && d_col) ? d_col[(size_t)(s0 + row0 + p) * C + c] : 0.f; },
             [&](int p, int c, float dc) {
               const int idx = act_index(c, p);
               float qv = 0.f;
               if (c < C && row0 + p < n) {
                 const float col = act[idx];
                 qv = dc * (col * (1.0f - col));
               }
               act[idx] = qv;
               Q[p * 32 + c] = qv;
             });
    __syncthreads();
  }
  isr::field::mfma_tile_layer_from<kThreads / 64>(A.T.outT, packT, act, false, ident, ZeroInit{});
  {
    float* G = A.g1 + (size_t)row0 * WcP;
    for_tile<kThreads>(WcP, [&](int p, int j) { return G[p * WcP + j]; }, [&](int p, int j, float sv) {
      const int idx = act_index(j, p);
      float gv = 0.f;
      if (j < Wc && row0 + p < n) gv = act[idx] * sv;
      act[idx] = gv;
      G[p * WcP + j] = gv;
    });
    __syncthreads();
  }
  isr::field::mfma_tile_layer_from<kThreads / 64>(A.T.trunkT, packT, act, false, ident,
                                                  DensityInit{pack + A.lay.d.out_w_off, gol, A.lay.d.out_K});
  for (int l = nh - 1; l >= 0; --l) {
    const Layer L = A.lay.d.L[l];
    float* G = A.g[l] + (size_t)row0 * L.OP;
    for_tile<kThreads>(L.OP, [&](int p, int j) { return G[p * L.OP + j]; }, [&](int p, int j, float sv) {
      const int idx = act_index(j, p);
      float gv = 0.f;
      if (j < L.O && row0 + p < n) gv = act[idx] * sv;
      act[idx] = gv;
      G[p * L.OP + j] = gv;
    });
    __syncthreads();
    if (l == 0) break;
    isr::field::mfma_tile_layer_from<kThreads / 64>(A.T.T[l], packT, act, false, ident, ZeroInit{});
  }
}

struct PackArgs {
  Layout lay;
  GradLayout T;
  StdOffsets so;
  float freqs[kMaxH];
  float beta;
};

// a thread per word of the two packs: its source entry, or zero
__global__ __launch_bounds__(kFlat) void radiance_pack_kernel(PackArgs A, const uint32_t* __restrict__ W,
                                                              const uint32_t* __restrict__ b, uint32_t* __restrict__ pack,
                                                              uint32_t* __restrict__ packT) {
  const int i = blockIdx.x * kFlat + threadIdx.x;
  const int total = A.lay.total_words, nh = A.lay.d.n_hidden;
  const int Wt = A.lay.d.out_K, ld1 = Wt + 6 * A.lay.d.H;
  if (i < total) {
    uint32_t bits = 0u;
    if (i < isr::density::kHeaderWords) {
      if (i == 0) bits = __float_as_uint(A.beta);
      else if (i == 1) bits = (uint32_t)A.lay.d.H;
      else if (i == 2) bits = (uint32_t)nh;
      else if (i >= isr::density::kFreqOff && i - isr::density::kFreqOff < A.lay.d.H) bits = __float_as_uint(A.freqs[i - isr::density::kFreqOff]);
    } else {
      bool done = false;
      for (int l = 0; l < nh && !done; ++l)
        done = pack_layer_word(A.lay.d.L[l], i, W, A.so.w[l], A.lay.d.L[l].K, 0, b, A.so.b[l], bits);
      if (!done) {
        if (i >= A.lay.d.out_w_off && i < A.lay.d.out_w_off + Wt) bits = W[A.so.w[nh] + i - A.lay.d.out_w_off];
        else if (i == A.lay.d.out_b_off) bits = b[A.so.b[nh]];
        else if (pack_layer_word(A.lay.dir, i, W, A.so.w[nh + 1], ld1, Wt, b, A.so.b[nh + 1], bits)) {
        } else if (pack_layer_word(A.lay.trunk, i, W, A.so.w[nh + 1], ld1, 0, b, -1, bits)) {
        } else pack_layer_word(A.lay.out, i, W, A.so.w[nh + 2], A.lay.Wc, 0, b, A.so.b[nh + 2], bits);
      }
    }
    pack[i] = bits;
  } else if (i < total + A.T.total_words) {
    const int t = i - total;
    uint32_t bits = 0u;
    bool done = false;
    for (int l = 1; l < nh && !done; ++l) done = pack_t_word(A.T.T[l], t, W, A.so.w[l], A.lay.d.L[l].K, A.lay.d.L[l].O, bits);
    if (!done && !pack_t_word(A.T.trunkT, t, W, A.so.w[nh + 1], ld1, A.lay.Wc, bits))
      pack_t_word(A.T.outT, t, W, A.so.w[nh + 2], A.lay.Wc, A.lay.C, bits);
    packT[t] = bits;
  }
}

bool layout_of(int n_hidden, const int32_t* widths, int H, int Wc, int C, Layout& lay) {
  return widths && make_layout(n_hidden, widths, H, Wc, C, lay);
}

void shape_error(const char* who) {
  isr::set_error("%s: null widths, or a hidden layer count (1..%d), a width (1..%d), H (1..%d), Wc (1..%d) or C (1..%d) out of range",
                 who, kMaxHidden, kMaxWidth, kMaxH, kMaxWidth, kMaxC);
}

// the checks every entry shares; on success lay is filled
int check_field(const char* who, const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                Layout& lay) {
  if (int rc = isr::check_pack_pointers(who, pack, widths)) return rc;
  ISR_REQUIRE(make_layout(n_hidden, widths, H, Wc, C, lay),
              "%s: %d hidden layers (1..%d), a width outside 1..%d, H = %d outside 1..%d, Wc = %d outside 1..%d or C = %d outside "
              "1..%d",
              who, n_hidden, kMaxHidden, kMaxWidth, H, kMaxH, Wc, kMaxWidth, C, kMaxC);
  return isr::check_pack_bytes(who, pack_bytes, lay.total_words);
}

int rays_of_slab(int slab, int N, int P) {                       // the rays `slab` consecutive points can touch, at most
  const long r = (long)slab / P + 2;
  return r < N ? (int)r : N;
}

// The workspace of a slab of `slab` points: where everything is from `base` on, and how many bytes that takes.
struct Carve {
  double* acc64;
  double* part_b;
  float* part;
  TileArgs t;
  size_t bytes;
};

Carve carve(const Layout& lay, int slab, int R, const StdOffsets& so, void* base) {
  Carve c;
  isr::Workspace ws(base, 0);
  const size_t chains = (size_t)((slab < kGradBatch ? slab : kGradBatch) / kGradChain);
  c.acc64 = ws.take<double>((size_t)so.w_total + so.b_total);
  c.part_b = ws.take<double>(chains * so.b_total);
  c.part = ws.take<float>(chains * so.w_total);
  c.t.ldE = (6 * lay.d.H + 31) / 32 * 32;
  c.t.e = ws.take<float>((size_t)slab * c.t.ldE);
  for (int l = 0; l < kMaxHidden; ++l) {
    c.t.h[l] = l < lay.d.n_hidden ? ws.take<float>((size_t)slab * lay.d.L[l].OP) : nullptr;
    c.t.g[l] = l < lay.d.n_hidden ? ws.take<float>((size_t)slab * lay.d.L[l].OP) : nullptr;
  }
  c.t.a1 = ws.take<float>((size_t)slab * lay.WcP);
  c.t.g1 = ws.take<float>((size_t)slab * lay.WcP);
  c.t.q = ws.take<float>((size_t)slab * 32);
  c.t.go = ws.take<float>((size_t)slab);
  c.t.u = ws.take<float>((size_t)R * lay.WcP);
  c.t.edir = ws.take<float>((size_t)R * c.t.ldE);
  c.bytes = isr::align_up(ws.off, 256);
  return c;
}

}  // namespace

extern "C" size_t isr_radiance_grad_pack_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C) {
  Layout lay;
  GradLayout T;
  if (!layout_of(n_hidden, widths, H, Wc, C, lay)) {
    shape_error("isr_radiance_grad_pack_bytes");
    return 0;
  }
  make_layout_t(lay, T);
  return (size_t)T.total_words * 4;
}

extern "C" int isr_radiance_pack_device(int n_hidden, const int32_t* widths, int H, int Wc, int C, const float* freqs, float beta,
                                        const float* W, const float* b, void* pack, size_t pack_bytes, void* packT,
                                        size_t packT_bytes, isr_stream_t stream) {
  const char* who = "isr_radiance_pack_device";
  PackArgs A;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, Wc, C, A.lay)) return rc;
  if (int rc = isr::grad::check_pack_t(who, A.lay, packT, packT_bytes, A.T)) return rc;
  ISR_REQUIRE(freqs && W && b, "%s: null pointer", who);
  ISR_REQUIRE(beta > 0.f && beta <= 3.0e38f, "%s: beta = %g must be positive and finite", who, (double)beta);
  std_offsets(A.lay, A.so);
  for (int i = 0; i < kMaxH; ++i) A.freqs[i] = i < H ? freqs[i] : 0.f;
  A.beta = beta;
  const int words = A.lay.total_words + A.T.total_words;
  radiance_pack_kernel<<<(words + kFlat - 1) / kFlat, kFlat, 0, isr::as_stream(stream)>>>(
      A, reinterpret_cast<const uint32_t*>(W), reinterpret_cast<const uint32_t*>(b), static_cast<uint32_t*>(pack),
      static_cast<uint32_t*>(packT));
  ISR_CHECK_LAUNCH("radiance_pack_kernel");
  return ISR_OK;
}

extern "C" size_t isr_radiance_grad_workspace_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C, int N, int P) {
  Layout lay;
  if (!layout_of(n_hidden, widths, H, Wc, C, lay)) {
    shape_error("isr_radiance_grad_workspace_bytes");
    return 0;
  }
  if (N < 0 || P < 1 || P > kMaxP) {
    isr::set_error("isr_radiance_grad_workspace_bytes: N = %d, P = %d (1..%d)", N, P, kMaxP);
    return 0;
  }
  StdOffsets so;
  std_offsets(lay, so);
  const int slab = isr::grad::slab_for((long)N * P);
  return carve(lay, slab, rays_of_slab(slab, N > 1 ? N : 1, P), so, nullptr).bytes;
}

extern "C" int isr_radiance_backward(const void* pack, size_t pack_bytes, const void* packT, size_t packT_bytes, int n_hidden,
                                     const int32_t* widths, int H, int Wc, int C, const float* origins, const float* directions,
                                     const float* lengths, int N, int P, const float* d_densities, const float* d_colours,
                                     float* dW, float* db, void* ws, size_t ws_bytes, isr_stream_t stream) {
  const char* who = "isr_radiance_backward";
  Layout lay;
  GradLayout T;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, Wc, C, lay)) return rc;
  if (int rc = isr::grad::check_pack_t(who, lay, packT, packT_bytes, T)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths, P, 0.f)) return rc;
  StdOffsets so;
  std_offsets(lay, so);
  hipStream_t st = isr::as_stream(stream);
  if (N == 0) return isr::grad::zero_grads(dW, so.w_total, db, so.b_total, st);
  ISR_REQUIRE(ws, "%s: null workspace", who);
  ISR_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace is not 16-byte aligned", who);
  const long NP = (long)N * P;
  int slab = isr::grad::slab_for(NP);
  while (slab > kGradChain && carve(lay, slab, rays_of_slab(slab, N, P), so, nullptr).bytes > ws_bytes) slab -= kGradChain;
  const int Rcap = rays_of_slab(slab, N, P);
  const Carve cv = carve(lay, slab, Rcap, so, ws);
  ISR_REQUIRE(cv.bytes <= ws_bytes, "%s: ws_bytes %zu, one chain of %d points needs %zu", who, ws_bytes, kGradChain, cv.bytes);
  TileArgs A = cv.t;
  A.lay = lay;
  A.T = T;
  DwArgs D{};
  D.w_total = so.w_total;
  D.b_total = so.b_total;
  const int nh = lay.d.n_hidden, Wt = lay.d.out_K, E6 = 6 * H;
  for (int l = 0; l < nh; ++l) {
    const Layer& L = lay.d.L[l];
    add_part(D, A.g[l], L.OP, L.O, l ? A.h[l - 1] : A.e, l ? lay.d.L[l - 1].OP : A.ldE, L.K, 0, true, so.w[l], L.K, so.b[l]);
  }
  const float* h_top = A.h[nh - 1];
  const int ld_top = lay.d.L[nh - 1].OP;
  add_part(D, A.go, 1, 1, h_top, ld_top, Wt, 0, false, so.w[nh], Wt, so.b[nh]);
  add_part(D, A.g1, lay.WcP, Wc, h_top, ld_top, Wt, 0, true, so.w[nh + 1], Wt + E6, so.b[nh + 1]);
  add_part(D, A.g1, lay.WcP, Wc, A.edir, A.ldE, E6, 1, true, so.w[nh + 1] + Wt, Wt + E6, -1);
  add_part(D, A.q, 32, C, A.a1, lay.WcP, Wc, 0, true, so.w[nh + 2], Wc, so.b[nh + 2]);
  const float* pk = static_cast<const float*>(pack);
  const float* pkT = static_cast<const float*>(packT);
  return isr::grad::for_slabs<true, kGradBatch>(D, NP, slab, P, cv.part, cv.part_b, cv.acc64, dW, db, st, [&](long s0, int n, long ray_base) -> int {
    const int R = (int)((s0 + n - 1) / P - ray_base) + 1;             // <= Rcap
    radiance_grad_dir_kernel<<<(R + kTP - 1) / kTP, kThreads, 0, st>>>(lay, pk, directions, ray_base, R, A.u, A.edir, A.ldE);
    ISR_CHECK_LAUNCH("radiance_grad_dir_kernel");
    radiance_grad_tile_kernel<<<(n + kTP - 1) / kTP, kThreads, 0, st>>>(A, pk, pkT, origins, directions, lengths, s0, n, P, ray_base,
                                                                         d_densities, d_colours);
    ISR_CHECK_LAUNCH("radiance_grad_tile_kernel");
    return ISR_OK;
  });
}

extern "C" int isr_radiance_backward_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc,
                                          int C, const float* origins, const float* directions, const float* lengths, int N,
                                          int P, const float* d_densities, const float* d_colours, float* dW, float* db) {
  const char* who = "isr_radiance_backward_host";
  Layout lay;
  if (int rc = check_field(who, pack, pack_bytes, n_hidden, widths, H, Wc, C, lay)) return rc;
  if (int rc = check_march(who, N, origins && directions && lengths, P, 0.f)) return rc;
  backward_host([](long n, long per_thread_min, auto fn) { isr::parallel_rows(n, per_thread_min, fn); }, lay, pack, origins,
                directions, lengths, N, P, d_densities, d_colours, dW, db);
  return ISR_OK;
}

extern "C" int isr_radiance_grad_slopes_host(const float* z, size_t n, float beta, float* slope_out, float* dexp_out) {
  ISR_REQUIRE(n == 0 || z, "isr_radiance_grad_slopes_host: null pointer");
  for (size_t i = 0; i < n; ++i) {
    if (slope_out) slope_out[i] = slope32(z[i], beta);
    if (dexp_out) dexp_out[i] = dexp32(z[i]);
  }
  return ISR_OK;
}

extern "C" int isr_radiance_grad_geometry(int which) {
  return which == 0 ? kGradChain : which == 1 ? kTP : which == 2 ? kGradSlab : which == 3 ? kGradBatch : -1;
}
