// field_mlp.hip — the key field (a SIREN coordinate MLP, field_mlp.hpp) evaluated in ONE launch: the entries of
// include/isr_field.h.
//
// field_tile.hpp's design with 4 waves per workgroup: a wave takes neuron blocks w and w + 4 of a wide layer.  What is the
// key field's own:
//   * Layers narrower than 32 on the input side (layer 0 has in = 3) are the chain itself on the vector unit, the weights
//     wave-uniform, their input copied k-major into inb.
//   * The last layer leaves the tile row-major (64, O) in LDS, so that only its columns go to device memory, in coalesced
//     rows; rows past N are evaluated at the origin and never written.
#include "field_tile.hpp"
#include "isr_common.hpp"

#include "../../include/isr_field.h"

#include <vector>

namespace {

using namespace isr::field;

constexpr int kThreads = 256;
constexpr int kActWords = (kMaxWidth / 2) * kTP * 2;      // 64 KB
constexpr int kInWords = kMfmaMinK * kTP;                 // 8 KB: the input of a vector-unit layer, k-major

__global__ __launch_bounds__(kThreads) void field_eval_kernel(Layout lay, const float* __restrict__ pack,
                                                              const float* __restrict__ pts, int N, float* __restrict__ out,
                                                              int ld_out) {
  __shared__ float act[kActWords];
  __shared__ float inb[kInWords];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
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
    const auto activation = [=](float z) { return activate(z, sine, omega); };
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
        const float v0 = j0 < L.O ? activation(z0) : 0.f;
        const float v1 = j0 + 1 < L.O ? activation(z1) : 0.f;
        if (!last) {
          *reinterpret_cast<float2*>(&act[act_index(j0, p)]) = make_float2(v0, v1);
        } else {
          if (j0 < L.O) act[p * L.O + j0] = v0;
          if (j0 + 1 < L.O) act[p * L.O + j0 + 1] = v1;
        }
      }
      __syncthreads();
    } else {
      mfma_tile_layer<kThreads / 64>(L, pack, act, last, activation);
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
  if (int rc = isr::check_pack_pointers(who, pack, widths)) return rc;
  ISR_REQUIRE(n_layers >= 1 && n_layers <= kMaxLayers, "%s: %d layers (1..%d)", who, n_layers, kMaxLayers);
  ISR_REQUIRE(make_layout(n_layers, widths, lay),
              "%s: widths out of range (widths[0] = 3, every width in 1..%d, the last at most %d)", who, kMaxWidth, kMaxOut);
  return isr::check_pack_bytes(who, pack_bytes, lay.total_words);
}

int check_io(const char* who, const Layout& lay, const float* pts, int N, const float* out, int ld_out) {
  if (int rc = isr::check_rows(who, N, pts && out)) return rc;
  ISR_REQUIRE(ld_out >= lay.L[lay.n_layers - 1].O, "%s: ld_out %d < out width %d", who, ld_out, lay.L[lay.n_layers - 1].O);
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
  std::vector<std::vector<float>> dense(n_layers);
  const float* rows[kMaxLayers];
  for (int l = 0; l < n_layers; ++l) {
    dense[l].resize((size_t)lay.L[l].O * lay.L[l].K);
    unpack_layer(lay.L[l], static_cast<const float*>(pack), dense[l].data(), false);
    rows[l] = dense[l].data();
  }
  // rows are independent: a few threads over row ranges (the fmaf chain is long: 2 * 256^2 per point and hidden layer)
  isr::parallel_rows(N, 64, [&](long n) { eval_rows_host(lay, pack, rows, pts, n, n + 1, out, ld_out); });
  return ISR_OK;
}

extern "C" int isr_field_sin_host(const float* a, size_t n, float* out) {
  ISR_REQUIRE(n == 0 || (a && out), "isr_field_sin_host: null pointer");
  for (size_t i = 0; i < n; ++i) out[i] = sin32(a[i]);
  return ISR_OK;
}
