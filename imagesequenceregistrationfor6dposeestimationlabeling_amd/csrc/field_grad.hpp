// field_grad.hpp — the backward of field_mlp.hpp's coordinate MLP with respect to its weights and biases, defined once and
// compiled for host and device.  csrc/field_grad.hip holds the kernels and the C entries (include/isr_field_grad.h).
//
// One point, with the forward's z_j (the fmaf chain), a_j = omega * z_j and h'_j = sin32(a_j), and u_l the gradient arriving at
// layer l's output (u of the last layer: the columns below O of the upstream row), from the last layer down:
//     sine layer:    s_j = omega * cos32(a_j) (one f32 multiply),  g_j = u_j * s_j (one f32 multiply)
//     linear layer:  g_j = u_j
//     u_{l-1}[k] = acc after  acc = fmaf(W_l[j,k], g_j, acc)  for j ascending from acc = +0      (not below layer 0)
// and over the N points   dW_l[j,k] = sum_n g_l[n,j] h_{l-1}[n,k],   db_l[j] = sum_n g_l[n,j]   in the order of grad_sums.hpp, a bias
// by the f32 chain of ones.  u_{l-1} is a tile layer over the TRANSPOSED weights from a zero accumulator (field_tile.hpp).
//
// The transposed pack: 64 zero header words, then for every layer l >= 1 the weights W_l^T as a layer with in = O_l rounded up
// to 32 (matrix-core order; a layer with K_l < 32 is row-major with in = O_l) and out = K_l, zero padded, and a zero bias.
#pragma once
#include "field_mlp.hpp"
#include "grad_sums.hpp"

namespace isr {
namespace field {

using grad::kGradChain;
using grad::kGradSlab;
// Points whose block sums are formed and added at a time (grad_sums.hpp).
constexpr int kGradBatch = 8192;

// cos(a) for an f32 a: sin32's reduction and kernels, the quadrant taken in f64, one rounding to f32.  cos32(+-0) = 1; NaN
// and +-Inf give NaN.
ISR_HD float cos32(float a) {
  double n, s, c;
  const double r = reduce_pio2((double)a, &n);
  sincos_kernel(r, &s, &c);
  const double q = n - 4.0 * rint(n * 0.25);      // n mod 4 in {-2, ..., 2}
  const double v = (q == 0.0) ? c : (q == 1.0) ? -s : (q == -1.0) ? s : -c;
  return (float)v;
}

// sin32(a) and cos32(a) from one reduction: the same bits as the two calls.
ISR_HD void sin_cos32(float a, float* sn, float* cs) {
  double n, s, c;
  const double r = reduce_pio2((double)a, &n);
  sincos_kernel(r, &s, &c);
  const double q = n - 4.0 * rint(n * 0.25);
  *sn = (float)((q == 0.0) ? s : (q == 1.0) ? c : (q == -1.0) ? -c : -s);
  *cs = (float)((q == 0.0) ? c : (q == 1.0) ? -s : (q == -1.0) ? s : -c);
}

// The layers of the transposed pack (L[0] is empty: nothing flows below layer 0).
ISR_HD void make_layout_t(const Layout& lay, Layout& t) {
  int off = kHeaderWords;
  t.n_layers = lay.n_layers;
  t.L[0] = Layer{0, 0, 0, 0, 0, off, off};
  for (int l = 1; l < lay.n_layers; ++l) {
    const Layer& L = lay.L[l];
    add_layer(L.mfma ? L.OP : L.O, L.K, L.mfma, off, t.L[l]);
  }
  t.total_words = off;
}

// Where the real entries of layer l sit in the standard layout (every W (out, in) row-major, layer after layer; every b).
ISR_HD void std_offsets(const Layout& lay, int* w_off, int* b_off, int* w_total, int* b_total) {
  int w = 0, b = 0;
  for (int l = 0; l < lay.n_layers; ++l) {
    w_off[l] = w;
    b_off[l] = b;
    w += lay.L[l].O * lay.L[l].K;
    b += lay.L[l].O;
  }
  *w_total = w;
  *b_total = b;
}

// Host: the transposed pack of W (standard layout).
inline void pack_t_host(const Layout& lay, const Layout& t, const float* W, float* packT) {
  for (int i = 0; i < t.total_words; ++i) packT[i] = 0.f;
  for (int l = 0; l < lay.n_layers; ++l) {
    const Layer& L = lay.L[l];
    if (l > 0)
      for (int j = 0; j < L.O; ++j)
        for (int k = 0; k < L.K; ++k) packT[t.L[l].w_off + w_index(t.L[l], k, j)] = W[(size_t)j * L.K + k];
    W += (size_t)L.O * L.K;
  }
}

// One point: the forward from pt, keeping every layer's input (H[l], K_l floats) and slope, then the rule above from the
// upstream row `up` (O_last floats; nullptr: zeros) down: G[l] (O_l floats).  dense[l]: W_l row-major.
inline void point_grads(const Layout& lay, const void* pack, const float* const* dense, const float* pt, const float* up,
                        float* const* H, float* const* G) {
  const float* pf = static_cast<const float*>(pack);
  float h[kMaxWidth], u[kMaxWidth], v[kMaxWidth];
  for (int k = 0; k < 3; ++k) h[k] = pt[k];
  for (int l = 0; l < lay.n_layers; ++l) {
    const Layer& L = lay.L[l];
    const bool sine = header_sine(pack, l);
    const float omega = header_omega(pack, l);
    for (int k = 0; k < L.K; ++k) H[l][k] = h[k];
    for (int j = 0; j < L.O; ++j) {
      const float* w = dense[l] + (size_t)j * L.K;
      float z = pf[L.b_off + j];
      for (int k = 0; k < L.K; ++k) z = fmaf(w[k], H[l][k], z);
      if (sine) {
        const float a = omega * z;
        float sn, cs;
        sin_cos32(a, &sn, &cs);
        h[j] = sn;
        G[l][j] = omega * cs;          // the slope, until the way down replaces it by g
      } else {
        h[j] = z;
      }
    }
  }
  const Layer& last = lay.L[lay.n_layers - 1];
  for (int j = 0; j < last.O; ++j) u[j] = up ? up[j] : 0.f;
  for (int l = lay.n_layers - 1; l >= 0; --l) {
    const Layer& L = lay.L[l];
    const bool sine = header_sine(pack, l);
    for (int j = 0; j < L.O; ++j) G[l][j] = sine ? u[j] * G[l][j] : u[j];
    if (l == 0) break;
    for (int k = 0; k < L.K; ++k) {
      float acc = 0.f;
      for (int j = 0; j < L.O; ++j) acc = fmaf(dense[l][(size_t)j * L.K + k], G[l][j], acc);
      v[k] = acc;
    }
    for (int k = 0; k < L.K; ++k) u[k] = v[k];
  }
}

}  // namespace field
}  // namespace isr
