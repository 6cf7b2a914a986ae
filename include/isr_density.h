/*
 * isr_density.h — C ABI of the density field of libisr_hip.so: the harmonic-embedding MLP of the reference's
 * NeuralRadianceFieldFeat (nerf.py:106-144, :163-177, :206-228; customForwardForDensity, :417-432) and the ray march that
 * turns its densities into surface points (pren.py:338-365; genFeat.py:185-198, generateCors.py:299-334).
 * The conventions are those of isr_hip.h and isr_field.h (return value ISR_OK or a negative ISR_ERR_*, text in
 * isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * A field: H frequencies f (1..64), n_hidden (1..4) hidden layers of widths[0..n_hidden) (each 1..256), one output neuron,
 * one beta > 0.  Layer 0 has in = 6 H, layer l in = widths[l-1]; W holds the hidden matrices (out, in) row-major one after
 * another and then the output row (widths[n_hidden-1] values), b the hidden biases and then the output bias.  A point x:
 *     a[d*H + i] = x[d] * f[i];  e = [sin a ..., cos a ...]  (6 H values)
 *     z_j = b_j;  z_j = fmaf(W[j,k], h[k], z_j), k ascending;  h'_j = softplus_beta(z_j)     (every hidden layer)
 *     density = 1 - exp(-softplus_beta(b + sum_k w[k] h[k]))                                   (the same chain)
 * with the library's own sine, cosine, softplus and exponential (csrc/field_density.hpp: each within 1 ulp of the f64
 * value, every finite argument): a function of the point and the weights only, and the same bits from the device entries
 * and the _host entries.
 *
 * The march of one ray with P lengths and densities rho_k (surface_thickness 1, the only one supported):
 *     threshold >= 0:  c_k = rho_k > threshold ? 1 : 0,  w_k = c_k * prod_{j<k} (1 - c_j)       (thresholdMode)
 *     threshold <  0:  w_k = rho_k * prod_{j<k} (1 - rho_j), sequentially in f32
 *     depth = max_k(lengths_k * w_k) starting from the first product;  point = origin + direction * depth;
 *     hit = any(w_k != 0).
 */
#ifndef ISR_DENSITY_H
#define ISR_DENSITY_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Size of the packed field in bytes; 0 (and isr_last_error()) for a null `widths` or a count, width or H out of range. */
size_t isr_density_pack_bytes(int n_hidden, const int32_t* widths, int H);

/* Lay the field out in the padded form both evaluations read.  Every pointer is a HOST pointer; pack a buffer of
 * pack_bytes = isr_density_pack_bytes(n_hidden, widths, H) bytes.  The caller copies the pack to the device once. */
int isr_density_pack(int n_hidden, const int32_t* widths, int H, const float* freqs, float beta, const float* W, const float* b,
                     void* pack, size_t pack_bytes);

/* pts (N, 3) f32 -> out (N,) f32.  pack: the DEVICE copy of what isr_density_pack wrote for the same n_hidden, widths (a
 * HOST array) and H.  N = 0 is a valid call that launches nothing (pts and out may then be null). */
int isr_density_eval(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* pts, int N,
                     float* out, isr_stream_t stream);

/* origins (N, 3), directions (N, 3), lengths (N, P) f32, 1 <= P <= 4096 -> depth (N,), points (N, 3) f32, hit (N,) int32,
 * and where the pointers are not null densities (N, P) and weights (N, P) f32.  The points o + d * len are made in the
 * kernel.  Every output is written for every ray, also for rays that hit nothing (depth as defined, point, hit = 0). */
int isr_density_march(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* origins,
                      const float* directions, const float* lengths, int N, int P, float threshold, float* densities,
                      float* weights, float* depth, float* points, int32_t* hit, isr_stream_t stream);

/* The same evaluations as host code over HOST pointers (pack as isr_density_pack wrote it): the tests' reference. */
int isr_density_eval_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* pts,
                          int N, float* out);
int isr_density_march_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* origins,
                           const float* directions, const float* lengths, int N, int P, float threshold, float* densities,
                           float* weights, float* depth, float* points, int32_t* hit);

/* sin_out[i], cos_out[i] = sincos32(a[i]); host code over HOST pointers. */
int isr_density_sincos_host(const float* a, size_t n, float* sin_out, float* cos_out);

/* softplus_out[i] = softplus_beta(z[i]) and density_out[i] = 1 - exp(-z[i]) as the field computes them; host code. */
int isr_density_activations_host(const float* z, size_t n, float beta, float* softplus_out, float* density_out);

#ifdef __cplusplus
}
#endif

#endif /* ISR_DENSITY_H */
