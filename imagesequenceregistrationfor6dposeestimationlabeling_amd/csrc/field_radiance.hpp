// field_radiance.hpp — the arithmetic of the radiance field: field_density.hpp's density field plus the colour head of
// NeuralRadianceFieldFeat in mode="color" (nerf.py:182-189, :230-268) and the emission-absorption render of a ray
// (pren.py:338-369), defined once and compiled for host and device.  csrc/field_radiance.hip holds the kernels and the C
// entries; include/isr_radiance.h states every rule written here.
//
// The PACK: field_density.hpp's pack of the density field (the same words isr_density_pack writes), then three layers in
// field_mlp.hpp's matrix-core order, each with its bias padded to 32 rows:
//     dir    K = 6H, O = Wc: W1's direction columns and b1           (the per-ray term u)
//     trunk  K = Wt, O = Wc: W1's trunk columns; its bias words stay zero and are not read (the chains start from u)
//     out    K = Wc, O = C:  W2 and b2
#pragma once
#include "field_density.hpp"

namespace isr {
namespace radiance {

using density::kMaxH;
using density::kMaxP;
using density::kMaxWidth;
using field::Layer;

constexpr int kMaxC = 32;          // colour channels of the fused head
constexpr int kMaxF = 64;          // feature channels of the march alone

struct Layout {
  density::Layout d;
  int Wc, C, WcP;                  // WcP: Wc rounded up to 32, the row stride of the direction terms
  int total_words;
  Layer dir, trunk, out;
};

ISR_HD bool make_layout(int n_hidden, const int32_t* widths, int H, int Wc, int C, Layout& lay) {
  if (!density::make_layout(n_hidden, widths, H, lay.d)) return false;
  if (Wc < 1 || Wc > kMaxWidth || C < 1 || C > kMaxC) return false;
  int off = lay.d.total_words;
  field::add_layer(6 * H, Wc, 1, off, lay.dir);
  field::add_layer(lay.d.out_K, Wc, 1, off, lay.trunk);
  field::add_layer(Wc, C, 1, off, lay.out);
  lay.Wc = Wc;
  lay.C = C;
  lay.WcP = lay.dir.OP;
  lay.total_words = off;
  return true;
}

// 1 / (1 + exp(-z)): an f64 value with an error near 2e-16 rounded once to f32.  exp64 saturates to 0 and +Inf, which gives
// the limits 1 and 0; NaN gives NaN.
ISR_HD float sigmoid32(float z) {
  const double e = density::exp64(-(double)z);
  return (float)(1.0 / (1.0 + e));
}

// d / max(||d||, 1e-12): torch.nn.functional.normalize on CPU f32 tensors.  The square root and the quotients are taken in
// f64 and rounded to f32, which is the correctly rounded f32 result (53 >= 2 * 24 + 2 bits), on every build.
ISR_HD void normalize3(const float* d, float* out) {
  const float s = __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0]));
  const float n = (float)__builtin_sqrt((double)s);
  const float m = n < 1e-12f ? 1e-12f : n;             // a NaN norm stays NaN
  for (int i = 0; i < 3; ++i) out[i] = (float)((double)d[i] / (double)m);
}

// The running state of one ray's render: ea_chain.hpp's weight chain (T, m, any) and the features; step() takes the samples
// in k order.
template <int kChannels>
struct RayState : ea::WeightChain {
  float feat[kChannels];
  ISR_HD void start() {
    ea::WeightChain::start();
#pragma unroll
    for (int c = 0; c < kChannels; ++c) feat[c] = 0.f;
  }
  // sample k: its length, its density (evaluated == false: a sample behind the first hit of thresholdMode, c_k * 0) and its
  // colours col[0 .. C) (nan_colour: the sample's point is not finite, every colour is NaN).  -> w_k
  ISR_HD float step(int k, float len, float rho, bool evaluated, float threshold, const float* col, int C, bool nan_colour) {
    const float w = ea::WeightChain::step(k, len, ea::absorbance(rho, threshold, evaluated));
    if (col) {
#pragma unroll
      for (int ch = 0; ch < kChannels; ++ch)
        if (ch < C) feat[ch] = __builtin_fmaf(w, col[ch], feat[ch]);
    } else if (nan_colour) {
#pragma unroll
      for (int ch = 0; ch < kChannels; ++ch)
        if (ch < C) feat[ch] = __builtin_fmaf(w, __builtin_nanf(""), feat[ch]);
    }
    return w;
  }
  ISR_HD float opacity() const { return 1.0f - T; }
};

ISR_HD bool finite3(const float* x) {
  return (x[0] - x[0] == 0.f) && (x[1] - x[1] == 0.f) && (x[2] - x[2] == 0.f);
}

// The march alone of one ray: rho (P), features (P, F) -> image (F + 1) and, where not null, weights (P).  The channels are
// taken 16 at a time, each pass running the same weight chain again.
ISR_HD void ea_march_ray(int P, int F, const float* rho, const float* features, float threshold, float* image,
                               float* weights) {
  RayState<16> st;
  for (int c0 = 0; c0 < F; c0 += 16) {
    st.start();
    const int nc = F - c0 < 16 ? F - c0 : 16;
    for (int k = 0; k < P; ++k) {
      const float w = st.step(k, 0.f, rho[k], true, threshold, features + (size_t)k * F + c0, nc, false);
      if (c0 == 0 && weights) weights[k] = w;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < nc) image[c0 + c] = st.feat[c];
  }
  image[F] = st.opacity();
}

// Host: the field's weights, W (hidden matrices, density row, W1 (Wc, Wt + 6H), W2 (C, Wc)) and b -> pack
inline void pack_host(const Layout& lay, const float* freqs, float beta, const float* W, const float* b, void* pack) {
  float* pf = static_cast<float*>(pack);
  uint32_t* pu = static_cast<uint32_t*>(pack);
  for (int i = 0; i < lay.total_words; ++i) pu[i] = 0u;
  density::pack_host(lay.d, freqs, beta, W, b, pack);
  for (int l = 0; l < lay.d.n_hidden; ++l) {
    W += (size_t)lay.d.L[l].O * lay.d.L[l].K;
    b += lay.d.L[l].O;
  }
  W += lay.d.out_K;
  b += 1;
  const int Wt = lay.d.out_K, E = 6 * lay.d.H;
  for (int j = 0; j < lay.Wc; ++j) {
    const float* row = W + (size_t)j * (Wt + E);
    for (int k = 0; k < Wt; ++k) pf[lay.trunk.w_off + field::w_index(lay.trunk, j, k)] = row[k];
    for (int k = 0; k < E; ++k) pf[lay.dir.w_off + field::w_index(lay.dir, j, k)] = row[Wt + k];
    pf[lay.dir.b_off + j] = b[j];
  }
  W += (size_t)lay.Wc * (Wt + E);
  b += lay.Wc;
  field::pack_layer(lay.out, W, b, pf);
}

// Host: every layer's weights transposed (Wt[k * O + j]), so that the chains of a layer advance together
struct HostWeights {
  density::HostWeights d;
  const float *dir, *trunk, *out;
};

// Host: the direction term u (Wc) of one ray
__attribute__((always_inline)) inline void ray_term_body(const Layout& lay, const void* pack, const HostWeights& hw,
                                                         const float* dirv, float* u) {
  float dn[3], e[6 * kMaxH];
  const float* pf = static_cast<const float*>(pack);
  normalize3(dirv, dn);
  density::embed_point(dn, pf + density::kFreqOff, lay.d.H, e);
  for (int j = 0; j < lay.Wc; ++j) u[j] = pf[lay.dir.b_off + j];
  for (int k = 0; k < 6 * lay.d.H; ++k) {
    const float ek = e[k];
    const float* wk = hw.dir + (size_t)k * lay.Wc;
    for (int j = 0; j < lay.Wc; ++j) u[j] = __builtin_fmaf(wk[j], ek, u[j]);
  }
}

// Host: one point through the field -> its density and its C colours; u is its ray's direction term.  The k loops are
// outermost and ascending; the trunk is field_density.hpp's trunk_body, whose last activations the colour head reads.
__attribute__((always_inline)) inline void point_radiance_body(const Layout& lay, const void* pack, const HostWeights& hw,
                                                               const float* x, const float* u, float* dens, float* colours) {
  float z[kMaxWidth], g[kMaxWidth];
  const float* pf = static_cast<const float*>(pack);
  const float beta = pf[0];
  const float* h = density::trunk_body(lay.d, pack, hw.d, x, z, g, dens);
  for (int j = 0; j < lay.Wc; ++j) z[j] = u[j];
  for (int k = 0; k < lay.trunk.K; ++k) {
    const float hk = h[k];
    const float* wk = hw.trunk + (size_t)k * lay.Wc;
    for (int j = 0; j < lay.Wc; ++j) z[j] = __builtin_fmaf(wk[j], hk, z[j]);
  }
  for (int j = 0; j < lay.Wc; ++j) g[j] = density::softplus32(z[j], beta);
  for (int c = 0; c < lay.C; ++c) z[c] = pf[lay.out.b_off + c];
  for (int k = 0; k < lay.Wc; ++k) {
    const float gk = g[k];
    const float* wk = hw.out + (size_t)k * lay.C;
    for (int c = 0; c < lay.C; ++c) z[c] = __builtin_fmaf(wk[c], gk, z[c]);
  }
  for (int c = 0; c < lay.C; ++c) colours[c] = sigmoid32(z[c]);
}

inline void ray_term_host(const Layout& lay, const void* pack, const HostWeights& hw, const float* dirv, float* u) {
  ray_term_body(lay, pack, hw, dirv, u);
}
inline void point_radiance_host(const Layout& lay, const void* pack, const HostWeights& hw, const float* x, const float* u,
                                float* dens, float* colours) {
  point_radiance_body(lay, pack, hw, x, u, dens, colours);
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
// the same functions compiled for CPUs with a fused multiply-add instruction (field_density.hpp's point_density_host_fma)
__attribute__((target("avx2,fma"))) inline void ray_term_host_fma(const Layout& lay, const void* pack, const HostWeights& hw,
                                                                  const float* dirv, float* u) {
  ray_term_body(lay, pack, hw, dirv, u);
}
__attribute__((target("avx2,fma"))) inline void point_radiance_host_fma(const Layout& lay, const void* pack,
                                                                        const HostWeights& hw, const float* x, const float* u,
                                                                        float* dens, float* colours) {
  point_radiance_body(lay, pack, hw, x, u, dens, colours);
}
#define ISR_RADIANCE_HAVE_FMA_BUILD 1
#endif

// Host: field_density.hpp's HostField of the trunk and the three colour layers unpacked and transposed
struct HostField {
  density::HostField d;
  std::vector<float> dir, trunk, out;
  HostWeights hw;
  bool fma;
  HostField(const Layout& lay, const void* pack) : d(lay.d, pack), fma(d.fma) {
    auto take = [&](const Layer& L, std::vector<float>& dst) {
      dst.resize((size_t)L.O * L.K);
      field::unpack_layer(L, static_cast<const float*>(pack), dst.data(), true);
      return dst.data();
    };
    hw.d = d.hw;
    hw.dir = take(lay.dir, dir);
    hw.trunk = take(lay.trunk, trunk);
    hw.out = take(lay.out, out);
  }
};

}  // namespace radiance
}  // namespace isr
