/*
 * isr_radiance.h — C ABI of the radiance field of libisr_hip.so: the density field of isr_density.h plus the colour head of
 * the reference's NeuralRadianceFieldFeat in mode="color" (nerf.py:182-189, :230-268, :340-402), rendered into per-ray
 * images by the emission-absorption march (pren.py:298-369), and that march alone over tensors the caller already has.
 * The conventions are those of isr_hip.h and isr_density.h (return value ISR_OK or a negative ISR_ERR_*, text in
 * isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h, isr_density.h and their ABI versions do not
 * change.
 *
 * A radiance field is a density field exactly as isr_density.h defines it (H <= 64 frequencies f, n_hidden <= 4 hidden
 * layers of widths <= 256, one beta, one density neuron) and a colour head
 *     Linear(Wt + 6H -> Wc), Softplus(beta), Linear(Wc -> C), Sigmoid
 * with Wt = widths[n_hidden - 1] the last hidden width, 1 <= Wc <= 256, 1 <= C <= 32 (3 in the reference).  W1 (Wc, Wt + 6H)
 * has the trunk's columns first and the direction's after them (nerf.py:263-266's concatenation), W2 is (C, Wc).
 *
 * DIRECTION of a ray d = (dx, dy, dz), once per ray:
 *     n  = sqrt(fmaf(dz, dz, fmaf(dy, dy, dx * dx)))          (f32; correspondences.norm3_f32's rule)
 *     dn = d / max(n, 1e-12f)                                 (true f32 quotients; a NaN n stays NaN)
 *     e_dir = the harmonic embedding of dn with the field's own frequencies and sincos32 (isr_density.h's order, 6H wide)
 * — torch.nn.functional.normalize on CPU f32 tensors bit for bit (tests/test_radiance_cpu.py), which matters: at H = 60 the
 * last bit of dn is many periods of the top frequencies.
 *
 * COLOUR LAYER 1 of a point with last hidden activations h (the bits the density neuron reads):
 *     per ray:    u_j = b1_j;  u_j = fmaf(W1[j, Wt + k], e_dir[k], u_j)  for k ascending over 6H
 *     per point:  z_j = u_j;   z_j = fmaf(W1[j, k], h[k], z_j)           for k ascending over Wt
 *                 g_j = softplus32(z_j, beta)
 * The order is the library's own choice (torch's GEMM order is not known): the direction is a per-ray bias.
 * COLOUR LAYER 2:  colour_c = sigmoid32(z), z = b2_c;  z = fmaf(W2[c, k], g[k], z) for k ascending over Wc.
 * sigmoid32 is 1 / (1 + exp(-z)) evaluated in f64 and rounded once: within 1 ulp of the f64 value for every finite z
 * (measured 0.5001), the same bits from the host and the device build, NaN for NaN, 0 and 1 at -inf and +inf.
 *
 * RENDER of one ray with P lengths: rho_k, c_k and w_k are exactly isr_density.h's march (threshold >= 0: thresholdMode,
 * c_k = rho_k > threshold ? 1 : 0; threshold < 0: c_k = rho_k; w_k = c_k * prod_{j<k} (1 - c_j); surface_thickness 1), and
 *     feat_c = 0;  feat_c = fmaf(w_k, colour_{k,c}, feat_c)  for k ascending
 *     T = 1;       T = T * (1 - c_k)                         for k ascending;   opacity = 1 - T
 *     image = [feat_0 .. feat_{C-1} | opacity]
 * The reference writes (1.0 + 1e-10) - c_k; the f64 scalar rounds to 1.0f, so the eps vanishes in f32 and is not restated.
 * depth, hit and the surface point are isr_density_march's.  A point that is not finite has NaN colours, and
 * fmaf(0, NaN, feat) is NaN: such a sample poisons its own ray's features whatever its weight, here as in torch.
 *
 * W and b of isr_radiance_pack: the hidden matrices (out, in) row-major one after another, the density row, W1, W2; the
 * hidden biases, the density bias, b1, b2.
 */
#ifndef ISR_RADIANCE_H
#define ISR_RADIANCE_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Size of the packed field in bytes; 0 (and isr_last_error()) for a null `widths` or a count, width, H, Wc or C out of
 * range. */
size_t isr_radiance_pack_bytes(int n_hidden, const int32_t* widths, int H, int Wc, int C);

/* Lay the field out in the padded form every entry reads.  Every pointer is a HOST pointer; the caller copies the pack to
 * the device once. */
int isr_radiance_pack(int n_hidden, const int32_t* widths, int H, int Wc, int C, const float* freqs, float beta, const float* W,
                      const float* b, void* pack, size_t pack_bytes);

/* Bytes of device workspace isr_radiance_render needs for N rays: the rays' direction terms u, (N, Wc rounded up to 32) f32.
 * 0 for N = 0; 0 and isr_last_error() for N < 0 or Wc out of range. */
size_t isr_radiance_workspace_bytes(int N, int Wc);

/* origins (N, 3), directions (N, 3), lengths (N, P) f32, 1 <= P <= 4096 -> image (N, C + 1) f32 [features | opacity],
 * depth (N,), points (N, 3) f32, hit (N,) int32, and where the pointers are not null weights (N, P), densities (N, P) and
 * colours (N, P, C) f32.  Every non-null output is written for every ray.  pack: the DEVICE copy of what isr_radiance_pack
 * wrote for the same n_hidden, widths (a HOST array), H, Wc and C; ws: ws_bytes >= isr_radiance_workspace_bytes(N, Wc) bytes
 * of device memory, 16-byte aligned, whatever it holds.  Two launches: the direction terms of the rays on the matrix cores
 * into ws, then the render; neither the colour head's (N P, Wt + 6H) input nor an activation nor a colour reaches device
 * memory unless densities or colours is asked for.  In threshold mode with P >= 64 and neither densities nor colours asked
 * for, the samples behind the 64-sample tile that holds the first hit are not evaluated: their weight is 0, and the bits of
 * every output are those of the full evaluation as long as finite points have finite colours (no overflow inside the
 * field).  N = 0 is a valid call that launches nothing.  Refused: isr_density_march's cases, Wc or C out of range, a null or
 * short workspace. */
int isr_radiance_render(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                        const float* origins, const float* directions, const float* lengths, int N, int P, float threshold,
                        float* image, float* depth, float* points, int32_t* hit, float* weights, float* densities,
                        float* colours, void* ws, size_t ws_bytes, isr_stream_t stream);

/* The raymarcher alone: densities (N, P), features (N, P, F) f32, 1 <= P <= 4096, 1 <= F <= 64 -> image (N, F + 1)
 * [features | opacity] and, where not null, weights (N, P).  The chain is the render's: marching isr_radiance_render's own
 * densities and colours gives its image bit for bit. */
int isr_ea_march(const float* densities, const float* features, int N, int P, int F, float threshold, float* image,
                 float* weights, isr_stream_t stream);

/* The same evaluations as host code over HOST pointers (pack as isr_radiance_pack wrote it): the tests' reference. */
int isr_radiance_render_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, int Wc, int C,
                             const float* origins, const float* directions, const float* lengths, int N, int P,
                             float threshold, float* image, float* depth, float* points, int32_t* hit, float* weights,
                             float* densities, float* colours);
int isr_ea_march_host(const float* densities, const float* features, int N, int P, int F, float threshold, float* image,
                      float* weights);

/* out[i] = sigmoid32(z[i]); host code over HOST pointers. */
int isr_radiance_sigmoid_host(const float* z, size_t n, float* out);

/* d (n, 3) -> out (n, 3), the DIRECTION rule above; host code over HOST pointers. */
int isr_radiance_normalize_host(const float* d, size_t n, float* out);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RADIANCE_H */
