/*
 * isr_radiance_grad.h — C ABI of the radiance field's backward in libisr_hip.so: the gradients of isr_radiance.h's field
 * (the harmonic-embedding trunk, the density neuron and the colour head of NeuralRadianceFieldFeat in mode="color") with
 * respect to its weights and biases, and the device-side packing a trainable field needs.
 *
 * trainNerfFine.py:174-186 trains mlp, density_layer and color_layer.  These entries give isr_radiance_render's field its
 * backward: from the upstream gradients of the per-point densities and colours to dW and db of every layer.  The
 * conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued
 * on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * The rule (csrc/radiance_grad.hpp is the one place the arithmetic is written).  One point n = ray * P + k; the forward's
 * quantities are the bits of isr_radiance.h / isr_density.h, recomputed from the rays: z_l the fmaf chains of the hidden
 * layers, h_l = softplus32(z_l, beta), z_o the density neuron's chain, s = softplus32(z_o, beta), z1 the chains of colour
 * layer 1 (started from the ray's direction term), a1 = softplus32(z1, beta), col = sigmoid32(z2).  Upstream:
 * drho = d_densities[n], dcol_c = d_colours[n, c].
 *     colour layer 2:   q_c = dcol_c * (col_c * (1 - col_c))                 (f32 operations in that order)
 *                       u1[k] = acc after  acc = fmaf(W2[c,k], q_c, acc)  for c ascending from +0
 *     colour layer 1:   g1_j = u1_j * slope32(z1_j, beta)                    (one f32 multiply)
 *     density neuron:   g_o = (drho * dexp32(s)) * slope32(z_o, beta)        (two f32 multiplies in that order)
 *     into h_top:       u_top[k] = acc after  acc = w_out[k] * g_o (one f32 product), then acc = fmaf(W1[j,k], g1_j, acc)
 *                       for j ascending over Wc; k < Wt only: W1's direction columns produce no downstream gradient
 *     hidden layers, from the top down:   g_l = u_l * slope32(z_l, beta);
 *                       u_{l-1}[k] = acc after  acc = fmaf(W_l[j,k], g_l[j], acc)  for j ascending from +0
 *                       (nothing is computed below layer 0)
 * slope32(z, beta) is the derivative of softplus32: sigmoid(beta z) with beta z the exact f64 product, evaluated once in
 * f64 as 1 / (1 + exp(-beta z)) and rounded once; exactly 1 where beta z > 20, where softplus32 is the identity (torch's
 * threshold).  dexp32(s) = exp(-s) evaluated in f64 and rounded once (within 1 ulp): NOT 1 - rho, which loses every bit
 * once rho rounds to 1.
 *
 * Every weight gradient is a sum over the N * P points of (output-side factor) x (input-side factor):
 *     dW_l         g_l    x  h_{l-1}; layer 0's input is the 6H embedding e of the point
 *     density row  g_o    x  h_top
 *     dW1          g1     x  [h_top, e_dir(ray of the point)], width Wt + 6H; the direction block is NOT reduced per ray
 *     dW2          q      x  a1
 *     biases       the same output-side factor x 1
 * in this order: the points in memory order in consecutive blocks of 64 (isr_radiance_grad_geometry(0)); inside a block the
 * f32 chain acc = fmaf(g, h, acc), n ascending from +0; the block sums added in block order in f64, rounded to f32 once.
 * A BIAS is summed in f64 throughout: inside a block acc = acc + (double)g, n ascending from +0; the block sums added in block
 * order; one rounding to f32.  (A chain of ones has no products that average out: with f32 chains the density bias of the
 * reference's executed code came to 14 x the reference's own f32 error, with f64 sums to 2 x.)
 * The result is a function of the inputs, N and P only: no float atomics, the same bytes on every call and from
 * isr_radiance_backward and isr_radiance_backward_host.  Origins, directions, lengths and the frequencies get no gradient.
 *
 * W, b, dW and db are in isr_radiance_pack's layout: the hidden matrices (out, in) row-major, the density row (Wt), W1
 * (Wc, Wt + 6H) with the trunk's columns first, W2 (C, Wc); the biases likewise.
 */
#ifndef ISR_RADIANCE_GRAD_H
#define ISR_RADIANCE_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Size in bytes of the transposed pack the backward reads beside isr_radiance_pack_bytes' forward pack; 0 (and
 * isr_last_error()) for a null `widths` or a shape isr_radiance_pack_bytes refuses. */
size_t isr_radiance_grad_pack_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C);

/* Pack on the device: W and b DEVICE arrays in isr_radiance_pack's layout, widths and freqs (H entries) HOST arrays read
 * during the call.  Writes every word of pack (byte for byte what isr_radiance_pack makes from the same numbers, header
 * and zero padding included) and of packT (64 zero words, then W_l^T of every hidden layer l >= 1, W1's trunk columns
 * transposed and W2^T, each in matrix-core order with the input side rounded up to 32 and a zero bias) in one launch, with
 * no host round trip. */
int isr_radiance_pack_device(int n_hidden, const int32_t* widths, int H, int Wc, int C, const float* freqs, float beta,
                             const float* W, const float* b, void* pack, size_t pack_bytes, void* packT, size_t packT_bytes,
                             isr_stream_t stream);

/* Bytes of workspace isr_radiance_backward wants for N rays of P samples: an f64 accumulator per gradient entry, one
 * block sum (f32 for a weight, f64 for a bias) per entry and chain of a batch of min(S, isr_radiance_grad_geometry(3))
 * points, per layer the slab's inputs and gradients (S rows, widths rounded up to 32), and the direction embeddings and
 * direction terms of the slab's rays, S = min(N * P rounded up to 64, isr_radiance_grad_geometry(2)): it grows with N * P
 * up to the slab and not beyond.  0 on an error. */
size_t isr_radiance_grad_workspace_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C, int N, int P);

/* origins (N, 3), directions (N, 3), lengths (N, P), d_densities (N, P), d_colours (N, P, C) -> dW and db in
 * isr_radiance_pack's W / b layout, real entries only; every entry is written on every call, N = 0 writes zeros and
 * launches nothing else.  d_densities or d_colours may be null, which means zeros; dW or db may be null (it is then not
 * written).  The forward is recomputed from the rays; nothing per point is kept beyond the workspace's slab.  pack and
 * packT: what isr_radiance_pack_device wrote.  ws: ws_bytes bytes of device scratch, at least
 * isr_radiance_grad_workspace_bytes(.., 64 points); the points are worked through in slabs of the largest multiple of 64
 * the workspace holds (at most the geometry's slab), and the result does not depend on the slab.  Refuses what
 * isr_radiance_render refuses (a shape out of range, P outside 1..4096, a null array with N > 0), and a null or short
 * workspace. */
int isr_radiance_backward(const void* pack, size_t pack_bytes, const void* packT, size_t packT_bytes, int n_hidden,
                          const int32_t* widths, int H, int Wc, int C, const float* origins, const float* directions,
                          const float* lengths, int N, int P, const float* d_densities, const float* d_colours, float* dW,
                          float* db, void* ws, size_t ws_bytes, isr_stream_t stream);

/* The same gradients as host code over HOST pointers (pack as isr_radiance_pack wrote it): the tests' reference. */
int isr_radiance_backward_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                               const float* origins, const float* directions, const float* lengths, int N, int P,
                               const float* d_densities, const float* d_colours, float* dW, float* db);

/* slope_out[i] = slope32(z[i], beta) and dexp_out[i] = dexp32(z[i]), host code over HOST pointers; either output may be
 * null. */
int isr_radiance_grad_slopes_host(const float* z, size_t n, float beta, float* slope_out, float* dexp_out);

/* The widths of the backward (tests and tools): which = 0 the chain length, 1 the tile, 2 the largest slab, 3 the batch of
 * points whose block sums are held at a time; -1 otherwise. */
int isr_radiance_grad_geometry(int which);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RADIANCE_GRAD_H */
