/*
 * isr_ray_losses.h — C ABI of the ray losses of libisr_hip.so and of their gradients: the distortion regulariser
 * nutil.mip360loss (nutil.py:140-152) over a ray's weights and depths, and the Huber terms of trainNerfFine.py:314-336
 * (nutil.huber of a render against nutil.sample_images_at_mc_locs of its targets, .abs().mean()).  Both are fused: the
 * distortion loss recomputes its (P-1, P-1) pairs from two LDS rows per ray and never stores one, so a call needs O(N P)
 * memory in total and O(N) workspace; the render loss reads the targets at the rays and never stores the samples.  The
 * conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued
 * on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.  Every device entry has a
 * _host twin over HOST pointers in the same library, the tests' reference: both are compiled from csrc/ray_losses.hpp, which
 * states the arithmetic once, with only + - * / sqrt fabsf and conversions in f32 and f64 (the library is built with
 * -ffp-contract=off), and give the same bits.  There are no float atomics.  Every output is a function of the inputs only:
 * not of the launch geometry, and not of which other rays share the call.  The upstream gradient is read on the device.
 * tests/ray_losses_ref.py restates both rules in NumPy.
 *
 * ---- 1. THE DISTORTION LOSS.  lengths (N, P) and weights (N, P), contiguous f32.  Per ray, with K = P - 1:
 *   d_k  = (l_k - l_0) + 0.0f                 f32, k = 0 .. P-1 (the + 0.0f makes every zero +0, so the maximum has one sign)
 *   mx   = the maximum of the d_k, NaN if any is NaN
 *   t_k  = d_k / mx                           f32
 *   ut_i = (t_{i+1} + t_i) / 2,  delta_i = t_{i+1} - t_i                          f32, i = 0 .. K-1
 *   inner_i = the f64 chain from +0, over j = 0 .. K-1 ascending, of  acc + (double)w_j * (double)fabsf(ut_i - ut_j)
 *             (the product of two f32 values is exact in f64: one rounding per term, whether or not it is fused)
 *   term_i  = (double)w_i * inner_i + (((double)w_i * (double)w_i) * (double)delta_i) / 3.0                      f64
 *   ray     = LANE ORDER sum of the term_i;   ray_loss = (float)ray
 *   loss    = (float)(S / (double)N),  S the f64 sum of the N values `ray` (not of their f32 roundings) in REDUCE ORDER
 * The pairs are formed directly with an absolute value: an unsorted row is an ordinary input.  weights[:, P-1] is never read
 * (the reference's [..., :-1] cut).  P = 2 gives inner = 0 and ray = w_0^2 / 3.
 *   GRADIENT, of weights only (lengths get none: in the step they come from linspace or from detached coarse weights):
 *   c = (double)upstream / (double)N
 *   dweights_i = (float)(c * (2.0 * inner_i + (2.0 * ((double)w_i * (double)delta_i)) / 3.0)),  i < K;   dweights_{P-1} = +0
 * inner_i is recomputed by the same chain, so forward and backward agree on its bits.  Nothing per pair reaches memory.
 *   SUM ORDER of inner_i: chosen f64 throughout.  On the fixture's weights (a march of random densities) against the
 * reference's executed code in f64, in multiples of the reference-f32's own deviation, the gradient measured: an f32 chain
 * over j 1.92 (64 coarse depths) and 2.05 (128 fine depths); f32 chains of 64 added in f64 the same 1.92 and 2.05 (the worst
 * entry sits inside one chain); the f64 chain 0.37 and 0.50 (profiles/ray_losses_parity.json), because only the f32 roundings
 * of t, ut and |ut_i - ut_j|, which the reference shares, remain.  The bound is 4.
 *   LANE ORDER.  64 f64 accumulators from +0; term_i is added to accumulator i mod 64, i ascending; the accumulators are
 * summed by the tree v[l] += v[l + s], s = 32, 16 .. 1.
 *   REDUCE ORDER.  256 consecutive values (missing ones are +0) are summed by the tree v[i] += v[i + s], s = 128, 64 .. 1, in
 * f64; the results are summed the same way, until one is left (the order of isr_contrastive.h).
 *   NON-FINITE INPUT is not refused: nothing synchronises.  A row whose depths are all equal has mx = 0 and t = 0 / 0: its
 * ray_loss and its dweights (column P-1 excepted) are NaN and so is loss, as in the reference; a NaN depth or weight does the
 * same to its row.  No other ray's ray_loss or dweights row changes.  Every NaN written is 0x7FC00000.
 *   LIMITS.  2 <= P <= 1024, 1 <= N <= 2^28 (N = 0 is REFUSED: the mean of no rays has no value); non-null lengths, weights,
 * loss, upstream, dweights and workspace; ray_loss may be null.  Anything else is ISR_ERR_ARG with a message, and nothing on the
 * device is touched.
 *
 * ---- 2. THE RENDER LOSS.  rendered (B, n, F+1) [colours | opacity], target_images (B, H, W, F), target_silhouettes (B, H, W),
 * xys (B, n, 2), contiguous f32; s = scaling, an f64.  Per element (b, r, ch), ch = 0 .. F:
 *   y = the target (ch < F: target_images, channel ch; ch = F: target_silhouettes) at pixel (nearest_pixel(xys_x, W),
 *       nearest_pixel(xys_y, H)) of image b, csrc/rays.hpp's nearest_pixel: round-half-even of ((-xy + 1) / 2) (size - 1), the rule
 *       of isr_sample_nearest (grid_sample, align_corners=True, mode='nearest', at -xy); 0 outside the image
 *   d = x - y                                  f32
 *   z = (double)d / s,  z2 = z * z,  q = sqrt(1.0 + z2)                            f64
 *   h = (s * z2) / (1.0 + q)                   f64: s (sqrt(1 + z^2) - 1) without the cancellation;  h = z2 where z2 is +Inf or NaN
 *   row_c = the f64 chain from +0 of the h of ch = 0 .. F-1 ascending;  row_o = the h of ch = F
 *   out[0] = (float)(Sc / (double)(B n F)),  out[1] = (float)(So / (double)(B n)),  Sc and So the sums of the B n values row_c
 *            and row_o in REDUCE ORDER: each an f64 sum in a fixed order, rounded once
 * h >= 0, so the reference's .abs() changes nothing; its clamp(1e-4) of 1 + z^2 >= 1 never binds for finite input, and NaN
 * propagates through both (torch's clamp keeps NaN).  An infinite d gives +Inf, as the reference's sqrt does.
 *   GRADIENT, of rendered only:  k_v = (double)upstream_v / count_v  (v = 0: colours, count B n F; v = 1: opacity, count B n)
 *   drendered = (float)((k_v * (double)d) / (s * q)),  and exactly +0 where d == 0 (whatever upstream holds)
 *   LIMITS.  B, n, H, W >= 1, 1 <= F <= 64, B n <= 2^28, B H W F < 2^31; s finite and > 0; non-null pointers.  Anything else is
 * ISR_ERR_ARG with a message.  Every NaN written is 0x7FC00000.
 *
 * LAUNCHES.  distortion forward: one over the rays (a wave owns a ray), then one per level of REDUCE ORDER (one up to 256 rays,
 * two up to 65 536); backward: one.  render loss forward: one over the rays, which also sums its 256 rows, then one per
 * further level; backward: one.
 */
#ifndef ISR_RAY_LOSSES_H
#define ISR_RAY_LOSSES_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_DISTORTION_MAX_P 1024
#define ISR_RENDER_LOSS_MAX_F 64

/* bytes of workspace the forward needs; 0 (and isr_last_error()) for a refused shape */
size_t isr_distortion_workspace_bytes(int64_t N, int P);

/* ray_loss_or_null: (N) f32; loss: 1 f32; both on the device, every byte written. */
int isr_distortion_forward(const float* lengths, const float* weights, int64_t N, int P, float* ray_loss_or_null, float* loss,
                           void* ws, size_t ws_bytes, isr_stream_t stream);

/* upstream: a DEVICE pointer to 1 f32.  dweights (N, P), written whole. */
int isr_distortion_backward(const float* lengths, const float* weights, int64_t N, int P, const float* upstream, float* dweights,
                            isr_stream_t stream);

int isr_distortion_forward_host(const float* lengths, const float* weights, int64_t N, int P, float* ray_loss_or_null, float* loss);

/* upstream: a HOST pointer */
int isr_distortion_backward_host(const float* lengths, const float* weights, int64_t N, int P, const float* upstream,
                                 float* dweights);

size_t isr_render_loss_workspace_bytes(int64_t B, int64_t n);

/* out: 2 f32 on the device (colour, silhouette). */
int isr_render_loss_forward(const float* rendered, const float* target_images, const float* target_silhouettes, const float* xys,
                            int B, int n, int F, int H, int W, double scaling, float* out, void* ws, size_t ws_bytes,
                            isr_stream_t stream);

/* upstream: a DEVICE pointer to 2 f32 (colour, silhouette).  drendered (B, n, F+1), written whole. */
int isr_render_loss_backward(const float* rendered, const float* target_images, const float* target_silhouettes, const float* xys,
                             int B, int n, int F, int H, int W, double scaling, const float* upstream, float* drendered,
                             isr_stream_t stream);

int isr_render_loss_forward_host(const float* rendered, const float* target_images, const float* target_silhouettes,
                                 const float* xys, int B, int n, int F, int H, int W, double scaling, float* out);

/* upstream: a HOST pointer */
int isr_render_loss_backward_host(const float* rendered, const float* target_images, const float* target_silhouettes,
                                  const float* xys, int B, int n, int F, int H, int W, double scaling, const float* upstream,
                                  float* drendered);

/* The kernels' widths (tests cover their boundaries; no result depends on them).  what 0: rays of a distortion workgroup,
 * 1: lanes that share a ray, 2: leaves of a reduction tree = rays of a render-loss workgroup, 3: the largest P; 0 otherwise. */
int isr_ray_losses_geometry(int what);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RAY_LOSSES_H */
