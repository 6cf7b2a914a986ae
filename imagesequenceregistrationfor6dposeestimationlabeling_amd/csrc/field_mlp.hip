// field_mlp.hip — the key field (a SIREN coordinate MLP, field_mlp.hpp) evaluated in ONE launch: the entries of
// include/isr_field.h.
//
// A workgroup (4 waves) takes a tile of 64 points through every layer; the tile's activations live in LDS from the first
// layer to the last, and only the last layer's columns go to device memory.
//   * Layers with in >= 32 run on v_mfma_f32_32x32x2_f32, which is bit for bit the k-ordered fmaf chain: A = the weights
//     (M = 32 neurons), B = the activations (N = 32 points), the accumulator loaded with the bias, the k loop in order.  The
//     weights are not staged in LDS (a 256 x 256 layer is 256 KB): the pack holds them in the order the lanes load them, so a
//     wave streams its own neurons' rows straight into registers, 8 k's (one 16-byte load per lane, 1 KB per wave) ahead of
//     the four MFMAs that use them; the four waves read disjoint quarters of the layer.
//   * Narrower layers (layer 0 has in = 3) are the chain itself on the vector unit, the weights wave-uniform.
//   * Widths are padded with zero weights (fmaf(0, x, z) = z for finite x) and padded activations are written as 0, so the
//     padding changes no bit; rows past N are evaluated at the origin and never written.
// Activations in LDS: k-pair major, act[((k >> 1) * 64 + p) * 2 + (k & 1)] — the B operand of k-step s (lane (r, h) wants
// k = 2 s + h of point r) is 64 consecutive words, and a lane's accumulator registers (neurons 8 a + 4 h + b) leave as
// two 8-byte stores.
#include "field_mlp.hpp"
#include "isr_common.hpp"

#include "../../include/isr_field.h"

#include <thread>
#include <vector>

namespace {

using namespace isr::field;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTP = 64;            // points per workgroup
constexpr int kThreads = 256;
constexpr int kActWords = (kMaxWidth / 2) * kTP * 2;      // 64 KB
constexpr int kInWords = kMfmaMinK * kTP;                 // 8 KB: the input of a vector-unit layer, k-major

// One wave's share of a matrix-core layer: NMB blocks of 32 neurons x NNB blocks of 32 points.
template <int NMB, int NNB>
__device__ __forceinline__ void mfma_layer(const Layer& L, const float* __restrict__ Wl, const float* __restrict__ bl,
                                           const float* act, const int (&mb)[2], int nb0, int lane, f32x16 (&acc)[2][2]) {
  const int r = lane & 31, hh = lane >> 5;
  const int S4 = L.kstride >> 3;
#pragma unroll
  for (int m = 0; m < NMB; ++m)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float bias = bl[mb[m] * 32 + 8 * a + 4 * hh + b];
#pragma unroll
        for (int n = 0; n < NNB; ++n) acc[m][n][4 * a + b] = bias;
      }
  const float4* wp[NMB];
  float4 cur[NMB];
#pragma unroll
  for (int m = 0; m < NMB; ++m) {
    wp[m] = reinterpret_cast<const float4*>(Wl) + (size_t)mb[m] * S4 * 64 + lane;
    cur[m] = wp[m][0];
  }
  const float* bp = act + (nb0 * 32 + r) * 2 + hh;
  for (int s4 = 0; s4 < S4; ++s4) {
    float4 nxt[NMB];
    const int sn = s4 + 1 < S4 ? s4 + 1 : s4;
#pragma unroll
    for (int m = 0; m < NMB; ++m) nxt[m] = wp[m][(size_t)sn * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float bv[NNB];
#pragma unroll
      for (int n = 0; n < NNB; ++n) bv[n] = bp[((4 * s4 + i) * kTP + n * 32) * 2];
#pragma unroll
      for (int m = 0; m < NMB; ++m) {
        const float av = i == 0 ? cur[m].x : i == 1 ? cur[m].y : i == 2 ? cur[m].z : cur[m].w;
#pragma unroll
        for (int n = 0; n < NNB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[n], acc[m][n], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < NMB; ++m) cur[m] = nxt[m];
  }
}

__global__ __launch_bounds__(kThreads) void field_eval_kernel(Layout lay, const float* __restrict__ pack,
                                                              const float* __restrict__ pts, int N, float* __restrict__ out,
                                                              int ld_out) {
  __shared__ float act[kActWords];
  __shared__ float inb[kInWords];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int r = lane & 31, hh = lane >> 5;
  const long row0 = (long)blockIdx.x * kTP;
  const uint32_t* pack_u = reinterpret_cast<const uint32_t*>(pack);

  if (w < 3) {
    const long row = row0 + lane;
    inb[w * kTP + lane] = row < N ? pts[3 * row + w] : 0.f;
  }
  __syncthreads();

  for (int l = 0; l < lay.n_layers; ++l) {
    const Layer L = lay.L[l];
    const bool last = l == lay.n_layers - 1;
    const float omega = pack[l];
    const bool sine = pack_u[8 + l] != 0;
    const float* Wl = pack + L.w_off;
    const float* bl = pack + L.b_off;
    if (!L.mfma) {
      if (l > 0) {
        for (int i = tid; i < L.K * kTP; i += kThreads) {
          const int k = i >> 6, p = i & 63;
          inb[i] = act[((k >> 1) * kTP + p) * 2 + (k & 1)];
        }
        __syncthreads();
      }
      const int p = lane;
      for (int jp = w; jp < L.OP / 2; jp += 4) {
        const int j0 = 2 * jp;
        const float* w0 = Wl + j0 * L.kstride;
        const float* w1 = w0 + L.kstride;
        float z0 = bl[j0], z1 = bl[j0 + 1];
        for (int k = 0; k < L.K; ++k) {
          const float hk = inb[k * kTP + p];
          z0 = fmaf(w0[k], hk, z0);
          z1 = fmaf(w1[k], hk, z1);
        }
        const float v0 = j0 < L.O ? activate(z0, sine, omega) : 0.f;
        const float v1 = j0 + 1 < L.O ? activate(z1, sine, omega) : 0.f;
        if (!last) {
          *reinterpret_cast<float2*>(&act[(jp * kTP + p) * 2]) = make_float2(v0, v1);
        } else {
          if (j0 < L.O) act[p * L.O + j0] = v0;
          if (j0 + 1 < L.O) act[p * L.O + j0 + 1] = v1;
        }
      }
      __syncthreads();
    } else {
      const int MB = L.OP >> 5;
      int mb[2] = {0, 0}, nmb, nb0, nnb;
      if (MB > 2) {               // a wave: neuron blocks w and w + 4, both point blocks
        mb[0] = w;
        mb[1] = w + 4;
        nmb = (w < MB) + (w + 4 < MB);
        nb0 = 0;
        nnb = 2;
      } else {                    // one or two neuron blocks (the last layer): a wave takes one 32 x 32 tile
        mb[0] = w >> 1;
        nmb = (w >> 1) < MB;
        nb0 = w & 1;
        nnb = 1;
      }
      f32x16 acc[2][2];
      if (nmb == 2) mfma_layer<2, 2>(L, Wl, bl, act, mb, nb0, lane, acc);
      else if (nmb == 1 && nnb == 2) mfma_layer<1, 2>(L, Wl, bl, act, mb, nb0, lane, acc);
      else if (nmb == 1) mfma_layer<1, 1>(L, Wl, bl, act, mb, nb0, lane, acc);
      __syncthreads();            // every wave has read the layer's input: the outputs may take its place
#pragma unroll
      for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (m < nmb && n < nnb) {
            const int p = (nb0 + n) * 32 + r;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const int j = mb[m] * 32 + 8 * a + 4 * hh;
              float v[4];
#pragma unroll
              for (int b = 0; b < 4; ++b) v[b] = j + b < L.O ? activate(acc[m][n][4 * a + b], sine, omega) : 0.f;
              if (!last) {
                *reinterpret_cast<float2*>(&act[((j >> 1) * kTP + p) * 2]) = make_float2(v[0], v[1]);
                *reinterpret_cast<float2*>(&act[(((j >> 1) + 1) * kTP + p) * 2]) = make_float2(v[2], v[3]);
              } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                  if (j + b < L.O) act[p * L.O + j + b] = v[b];
              }
            }
          }
        }
      }
      __syncthreads();
    }
    if (last) {                   // act holds the tile row-major (64, O): coalesced rows out
      for (int i = tid; i < kTP * L.O; i += kThreads) {
        const int p = i / L.O, c = i - p * L.O;
        const long row = row0 + p;
        if (row < N) out[(size_t)row * ld_out + c] = act[i];
      }
    }
  }
}

// the checks every entry shares; on success lay is filled
int check_field(const char* who, const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, Layout& lay) {
  ISR_REQUIRE(pack && widths, "%s: null pointer", who);
  ISR_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: %d layers (1..%d)", who, n_layers, kMaxLayers);
  ISR_REQUIRE(make_layout(n_layers, widths, lay),
              "%s: widths out of range (widths[0] = 3, every width in 1..%d, the last at most %d)", who, kMaxWidth, kMaxOut);
  ISR_REQUIRE(pack_bytes == (size_t)lay.total_words * 4, "%s: pack_bytes %zu, this field packs to %zu", who, pack_bytes,
              (size_t)lay.total_words * 4);
  return ISR_OK;
}

int check_io(const char* who, const Layout& lay, const float* pts, int N, const float* out, int ld_out) {
  ISR_REQUIRE(N >= 0, "%s: N = %d", who, N);
  ISR_REQUIRE(ld_out >= lay.L[lay.n_layers - 1].O, "%s: ld_out %d < out width %d", who, ld_out, lay.L[lay.n_layers - 1].O);
  ISR_REQUIRE(N == 0 || (pts && out), "%s: null pointer", who);
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_field_pack_bytes(int n_layers, const int32_t* widths) {
  Layout lay;
  if (!widths || n_layers < 1 || n_layers > kMaxLayers || !make_layout(n_layers, widths, lay)) {
    isr::set_error("isr_field_pack_bytes: null widths, or a layer count (1..%d) or width (3, then 1..%d, the last <= %d) out of range",
                   kMaxLayers, kMaxWidth, kMaxOut);
    return 0;
  }
  return (size_t)lay.total_words * 4;
}

extern "C" int isr_field_pack(int n_layers, const int32_t* widths, const float* W, const float* b, const float* omega,
                              const int32_t* sine, void* pack, size_t pack_bytes) {
  Layout lay;
  if (int rc = check_field("isr_field_pack", pack, pack_bytes, n_layers, widths, lay)) return rc;
  ISR_REQUIRE(W && b && omega && sine, "isr_field_pack: null pointer");
  pack_host(lay, W, b, omega, sine, pack);
  return ISR_OK;
}

extern "C" int isr_field_eval(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts, int N,
                              float* out, int ld_out, isr_stream_t stream) {
  Layout lay;
  if (int rc = check_field("isr_field_eval", pack, pack_bytes, n_layers, widths, lay)) return rc;
  if (int rc = check_io("isr_field_eval", lay, pts, N, out, ld_out)) return rc;
  if (N == 0) return ISR_OK;
  const unsigned blocks = (unsigned)(((long)N + kTP - 1) / kTP);
  field_eval_kernel<<<blocks, kThreads, 0, isr::as_stream(stream)>>>(lay, static_cast<const float*>(pack), pts, N, out, ld_out);
  ISR_CHECK_LAUNCH("field_eval_kernel");
  return ISR_OK;
}

extern "C" int isr_field_eval_host(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts,
                                   int N, float* out, int ld_out) {
  Layout lay;
  if (int rc = check_field("isr_field_eval_host", pack, pack_bytes, n_layers, widths, lay)) return rc;
  if (int rc = check_io("isr_field_eval_host", lay, pts, N, out, ld_out)) return rc;
  if (N == 0) return ISR_OK;
  const float* pf = static_cast<const float*>(pack);
  std::vector<std::vector<float>> dense(n_layers);
  const float* rows[kMaxLayers];
  for (int l = 0; l < n_layers; ++l) {
    const Layer& L = lay.L[l];
    dense[l].resize((size_t)L.O * L.K);
    for (int j = 0; j < L.O; ++j)
      for (int k = 0; k < L.K; ++k) dense[l][(size_t)j * L.K + k] = pf[L.w_off + w_index(L, j, k)];
    rows[l] = dense[l].data();
  }
  // rows are independent: a few threads over row ranges (the fmaf chain is long: 2 * 256^2 per point and hidden layer)
  const int nthreads = N >= 512 ? 8 : 1;
  if (nthreads == 1) {
    eval_rows_host(lay, pack, rows, pts, 0, N, out, ld_out);
    return ISR_OK;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t) {
    const long n0 = (long)N * t / nthreads, n1 = (long)N * (t + 1) / nthreads;
    pool.emplace_back([&, n0, n1] { eval_rows_host(lay, pack, rows, pts, n0, n1, out, ld_out); });
  }
  for (auto& th : pool) th.join();
  return ISR_OK;
}

extern "C" int isr_field_sin_host(const float* a, size_t n, float* out) {
  ISR_REQUIRE(n == 0 || (a && out), "isr_field_sin_host: null pointer");
  for (size_t i = 0; i < n; ++i) out[i] = sin32(a[i]);
  return ISR_OK;
}
