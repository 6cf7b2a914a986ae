// field_mlp.hpp — the arithmetic of a coordinate MLP (the key field of refine_pose: nerf.py:201-202's SIREN feature head),
// defined once and compiled for host and device.  csrc/field_mlp.hip holds the kernel and the C entries (include/isr_field.h).
//
// A field is n_layers <= 8 layers; layer l has W_l (out_l, in_l), b_l (out_l,) and either an omega_l (a sine layer,
// h <- sin32(omega * (W h + b)), Sitzmann et al. 2020) or none (a linear layer, h <- W h + b).  in_0 = 3, in_l = out_{l-1},
// every width <= 256, the last <= 32.  One point's value:
//     z_j = b_j;  z_j = fmaf(W[j,k], h[k], z_j) for k ascending;  a = omega * z_j (one f32 multiply);  h'_j = sin32(a)
// — a function of the point and the weights only.  Everything is built with -ffp-contract=off, and sin32 below uses
// + - * rint and conversions alone, so the host and the device build of this header give the same bits.
//
// The PACK is the padded form both builds read: 64 header words (omega_l bits at [l], sine flag at [8 + l]), then per layer
// the weights and the bias, zero padded.  A layer with in_l >= 32 is stored in the order the matrix-core kernel loads it
// (w_index); a narrower one (layer 0 has in = 3) row-major with the row stride rounded up to 4.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace field {

constexpr int kMaxLayers = 8;
constexpr int kMaxWidth = 256;
constexpr int kMaxOut = 32;
constexpr int kHeaderWords = 64;
constexpr int kMfmaMinK = 32;      // layers at least this wide on the input side run on v_mfma_f32_32x32x2_f32

struct Layer {
  int K, O;        // in, out
  int OP;          // out rounded up to 32 (rows of zero weights and zero bias)
  int mfma;        // 1: matrix-core order, kstride = K rounded up to 8; 0: row-major, kstride = K rounded up to 4
  int kstride;
  int w_off, b_off;   // in 4-byte words from the start of the pack
};

struct Layout {
  int n_layers;
  int total_words;
  Layer L[kMaxLayers];
};

// Layer `L` of a pack: K inputs, O outputs, in matrix-core order or not, its words from `off` on (which moves past them).
ISR_HD void add_layer(int K, int O, int mfma, int& off, Layer& L) {
  L.K = K;
  L.O = O;
  L.OP = (O + 31) / 32 * 32;
  L.mfma = mfma;
  L.kstride = mfma ? (K + 7) / 8 * 8 : (K + 3) / 4 * 4;
  L.w_off = off;
  off += L.OP * L.kstride;
  L.b_off = off;
  off += L.OP;
}

// false: a layer count or a width outside the limits (lay is then unspecified)
ISR_HD bool make_layout(int n_layers, const int32_t* widths, Layout& lay) {
  if (n_layers < 1 || n_layers > kMaxLayers || widths[0] != 3) return false;
  int off = kHeaderWords;
  for (int l = 0; l < n_layers; ++l) {
    const int K = widths[l], O = widths[l + 1];
    if (O < 1 || O > kMaxWidth) return false;
    add_layer(K, O, K >= kMfmaMinK ? 1 : 0, off, lay.L[l]);
  }
  if (widths[n_layers] > kMaxOut) return false;
  lay.n_layers = n_layers;
  lay.total_words = off;
  return true;
}

// Where W[j, k] of a layer sits inside its weight block.  Matrix-core order: 32-row blocks; per block and per group of 8 k's,
// lane (k & 1) * 32 + (j & 31) owns four consecutive words, the k's 8g + 2i + (k & 1) for i = 0..3 — one 16-byte load per
// lane feeds four v_mfma_f32_32x32x2_f32 (A operand: lane (r, h) holds A[r][h]).
ISR_HD int w_index(const Layer& L, int j, int k) {
  if (!L.mfma) return j * L.kstride + k;
  const int lane = (k & 1) * 32 + (j & 31);
  return (((j >> 5) * (L.kstride >> 3) + (k >> 3)) * 64 + lane) * 4 + ((k & 7) >> 1);
}

// The reduction and the kernels of sin32 below and of sincos32 (field_density.hpp), in f64.
// Cody-Waite: n = rint(x * 2/pi), r = (x - n C1) - n C2 with C1 the leading 33 bits of pi/2 -- n C1 and the subtraction are
// exact for |n| < 2^20 -- clamped to [-1, 1] (it is within pi/4 wherever the reduction is accurate).  -> r, n in *n.
ISR_HD double reduce_pio2(double x, double* n_out) {
  const double n = rint(x * 6.36619772367581382433e-01);
  const double r0 = (x - n * 1.57079632673412561417e+00) - n * 6.07710050650619224932e-11;
  const double r = (n == 0.0) ? x : r0;
  *n_out = n;
  return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// sin(r) and cos(r) on |r| <= pi/4: the degree-13 / degree-14 kernels of Sun's fdlibm
ISR_HD void sincos_kernel(double r, double* s, double* c) {
  const double r2 = r * r;
  const double ps = -1.66666666666666324348e-01 +
                    r2 * (8.33333333332248946124e-03 +
                          r2 * (-1.98412698298579493134e-04 +
                                r2 * (2.75573137070700676789e-06 +
                                      r2 * (-2.50507602534068634195e-08 + r2 * 1.58969099521155010221e-10))));
  const double pc = -0.5 + r2 * (4.16666666666666019037e-02 +
                                 r2 * (-1.38888888888741095749e-03 +
                                       r2 * (2.48015872894767294178e-05 +
                                             r2 * (-2.75573143513906633035e-07 +
                                                   r2 * (2.08757232129817482790e-09 + r2 * -1.13596475577881948265e-11)))));
  *s = r * (1.0 + r2 * ps);
  *c = 1.0 + r2 * pc;
}

// sin(a) for an f32 a, correctly rounded up to the rounding of an f64 result whose error is ~1e-16 (within 1 ulp of the true
// sine for |a| <= 2^17; measured 0.5 ulp).  Beyond 2^17 the reduction loses accuracy but r is clamped, so the value stays in
// [-1, 1] and is the same on every build; n can reach 2e38 there, so the quadrant is taken in f64.  NaN and +-Inf give NaN
// (every comparison is false for them); sin32(-0) = -0.
ISR_HD float sin32(float a) {
  double n, s, c;
  const double r = reduce_pio2((double)a, &n);
  sincos_kernel(r, &s, &c);
  const double q = n - 4.0 * rint(n * 0.25);      // n mod 4 in {-2, ..., 2}
  const double v = (q == 0.0) ? s : (q == 1.0) ? c : (q == -1.0) ? -c : -s;
  return (float)v;
}

// A pre-activation to the layer's output.
ISR_HD float activate(float z, bool sine, float omega) {
  if (!sine) return z;
  const float a = omega * z;
  return sin32(a);
}

inline float header_omega(const void* pack, int l) { return static_cast<const float*>(pack)[l]; }
inline bool header_sine(const void* pack, int l) { return static_cast<const uint32_t*>(pack)[8 + l] != 0; }

// Host: one layer's W (O, K) row-major and b (O,) to their places in the pack (the padding is not touched)
inline void pack_layer(const Layer& L, const float* W, const float* b, float* pack) {
  for (int j = 0; j < L.O; ++j) {
    for (int k = 0; k < L.K; ++k) pack[L.w_off + w_index(L, j, k)] = W[(size_t)j * L.K + k];
    pack[L.b_off + j] = b[j];
  }
}

// Host: the layer's weights out of the pack: dst[j * K + k], or transposed dst[k * O + j]
inline void unpack_layer(const Layer& L, const float* pack, float* dst, bool transposed) {
  for (int j = 0; j < L.O; ++j)
    for (int k = 0; k < L.K; ++k) dst[transposed ? (size_t)k * L.O + j : (size_t)j * L.K + k] = pack[L.w_off + w_index(L, j, k)];
}

// Host: W (row-major, layer after layer), b, omega, sine -> pack (lay.total_words words).
inline void pack_host(const Layout& lay, const float* W, const float* b, const float* omega, const int32_t* sine, void* pack) {
  float* pf = static_cast<float*>(pack);
  uint32_t* pu = static_cast<uint32_t*>(pack);
  for (int i = 0; i < lay.total_words; ++i) pu[i] = 0u;
  for (int l = 0; l < lay.n_layers; ++l) {
    const Layer& L = lay.L[l];
    pf[l] = sine[l] ? omega[l] : 0.f;
    pu[8 + l] = sine[l] ? 1u : 0u;
    pack_layer(L, W, b, pf);
    W += (size_t)L.O * L.K;
    b += L.O;
  }
}

// Host: rows [n0, n1) of pts (N, 3) through the packed field into out (N, ld_out), columns < out_last.  dense: the layers'
// weights unpacked row-major (unpack_layer), so that the inner loop is the plain chain.
inline void eval_rows_host(const Layout& lay, const void* pack, const float* const* dense, const float* pts, long n0, long n1,
                           float* out, long ld_out) {
  const float* pf = static_cast<const float*>(pack);
  float h[kMaxWidth], g[kMaxWidth];
  for (long n = n0; n < n1; ++n) {
    for (int k = 0; k < 3; ++k) h[k] = pts[3 * n + k];
    for (int l = 0; l < lay.n_layers; ++l) {
      const Layer& L = lay.L[l];
      const bool sine = header_sine(pack, l);
      const float omega = header_omega(pack, l);
      for (int j = 0; j < L.O; ++j) {
        const float* w = dense[l] + (size_t)j * L.K;
        float z = pf[L.b_off + j];
        for (int k = 0; k < L.K; ++k) z = fmaf(w[k], h[k], z);
        g[j] = activate(z, sine, omega);
      }
      for (int j = 0; j < L.O; ++j) h[j] = g[j];
    }
    const Layer& last = lay.L[lay.n_layers - 1];
    for (int j = 0; j < last.O; ++j) out[n * ld_out + j] = h[j];
  }
}

}  // namespace field
}  // namespace isr
