/*
 * isr_field.h — C ABI of the key field of libisr_hip.so: a coordinate MLP (SIREN) evaluated in one launch.
 *
 * refine_pose asks a neural field for the key descriptors of the visible surface points (pose_refine.py:52-53:
 * neural_radiance_field.batched_customForward; the field's feature head is nerf.py:201-202).  These entries evaluate such a
 * field on the device: N points through every layer in one kernel, no intermediate activation in device memory.
 * The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work
 * enqueued on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * A field: n_layers (1..8) layers, widths[0..n_layers] with widths[0] = 3, every width in 1..256, the last at most 32.
 * Layer l: W_l (widths[l+1], widths[l]) row-major f32, b_l (widths[l+1],) f32, and either omega_l (sine[l] != 0:
 * h <- sin(omega_l * (W_l h + b_l))) or none (sine[l] == 0: h <- W_l h + b_l).  The value of a point is
 *     z_j = b_j;  z_j = fmaf(W[j,k], h[k], z_j), k ascending;  a = omega * z_j in f32;  h'_j = sin32(a)
 * with sin32 the library's own sine (csrc/field_mlp.hpp: within 1 ulp for |a| <= 2^17, NaN for NaN or +-Inf): a function
 * of the point and the weights only, and the same bits from isr_field_eval and isr_field_eval_host.
 */
#ifndef ISR_FIELD_H
#define ISR_FIELD_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Size of the packed field in bytes; 0 (and isr_last_error()) for a null `widths` or a layer count or width out of range. */
size_t isr_field_pack_bytes(int n_layers, const int32_t* widths);

/* Lay the field out in the padded form both evaluations read.  Every pointer is a HOST pointer: W the layers' matrices one
 * after another, b their biases one after another, omega and sine n_layers entries each (omega[l] is ignored where
 * sine[l] == 0), pack a buffer of pack_bytes = isr_field_pack_bytes(n_layers, widths) bytes.  The caller copies the pack
 * to the device once, for isr_field_eval. */
int isr_field_pack(int n_layers, const int32_t* widths, const float* W, const float* b, const float* omega, const int32_t* sine,
                   void* pack, size_t pack_bytes);

/* pts (N, 3) f32 -> out (N, ld_out) f32, ld_out >= widths[n_layers]; columns >= widths[n_layers] and rows >= N are not
 * written.  pack: the DEVICE copy of what isr_field_pack wrote for the same n_layers and widths (a HOST array).  N = 0 is a
 * valid call that launches nothing (pts and out may then be null). */
int isr_field_eval(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts, int N, float* out,
                   int ld_out, isr_stream_t stream);

/* The same evaluation as host code over HOST pointers (pack as isr_field_pack wrote it): the tests' reference. */
int isr_field_eval_host(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts, int N,
                        float* out, int ld_out);

/* out[i] = sin32(a[i]), host code over HOST pointers. */
int isr_field_sin_host(const float* a, size_t n, float* out);

#ifdef __cplusplus
}
#endif

#endif /* ISR_FIELD_H */
