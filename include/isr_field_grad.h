/*
 * isr_field_grad.h — C ABI of the key field's backward in libisr_hip.so: the gradients of a SIREN coordinate MLP
 * (isr_field.h) with respect to its weights and biases, and the device-side packing a trainable field needs.
 *
 * trainPose.py trains the feature head alone (feature_layer.requires_grad_(True)) and makes its keys by
 * batched_customForward (trainPose.py:362, 379-380).  These entries give isr_field_eval's field its backward: from the
 * upstream gradient of the keys to dW_l and db_l of every layer.  The conventions are those of isr_hip.h (return value ISR_OK
 * or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h's entry list
 * and ISR_ABI_VERSION do not change.
 *
 * The rule (csrc/field_grad.hpp is the one place the arithmetic is written).  For one point, with isr_field.h's z_j,
 * a_j = omega * z_j and h'_j = sin32(a_j), and u_l the gradient arriving at layer l's output, from the last layer down:
 *     sine layer:    s_j = omega * cos32(a_j) (one f32 multiply),  g_j = u_j * s_j (one f32 multiply)
 *     linear layer:  g_j = u_j
 *     u_{l-1}[k] = acc after  acc = fmaf(W_l[j,k], g_j, acc)  for j ascending from +0            (not below layer 0)
 * and over the points  dW_l[j,k] = sum_n g_l[n,j] h_{l-1}[n,k],  db_l[j] = sum_n g_l[n,j]  in this order: consecutive blocks
 * of 64 points (isr_field_grad_geometry(0)); inside a block the f32 chain acc = fmaf(g, h, acc), n ascending from +0 (db:
 * h = 1); the block sums added in block order in f64, rounded to f32 once.  The result is a function of the inputs and N
 * only, and the same bits from isr_field_backward and isr_field_backward_host.  Points get no gradient.
 * cos32 is the library's own cosine: sin32's reduction and kernels, NaN for NaN or +-Inf, cos32(+-0) = 1.
 *
 * The standard layout of W, b, dW and db: every layer's (out, in) matrix row-major, layer after layer; every bias likewise.
 */
#ifndef ISR_FIELD_GRAD_H
#define ISR_FIELD_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Size in bytes of the transposed pack the backward reads beside isr_field_pack_bytes' forward pack; 0 (and
 * isr_last_error()) for a null `widths` or a layer count or width out of range. */
size_t isr_field_grad_pack_bytes(int n_layers, const int32_t* widths);

/* Pack on the device: W and b DEVICE arrays in the standard layout, omega and sine HOST arrays of n_layers entries (read
 * during the call).  Writes every word of pack (byte for byte what isr_field_pack makes from the same numbers, header and
 * zero padding included) and of packT (the transposed weights in matrix-core order) in one launch, with no host round trip. */
int isr_field_pack_device(int n_layers, const int32_t* widths, const float* W, const float* b, const float* omega,
                          const int32_t* sine, void* pack, size_t pack_bytes, void* packT, size_t packT_bytes, isr_stream_t stream);

/* Bytes of workspace isr_field_backward wants for N points: an f64 accumulator per gradient entry, one f32 block sum per
 * entry and chain of a batch of min(S, isr_field_grad_geometry(3)) points, and per layer the slab's inputs (S, in rounded up
 * to 32) and gradients (S, out rounded up to 32), S = min(N rounded up to 64, isr_field_grad_geometry(2)): it grows with N up
 * to the slab and not beyond.  0 on an error. */
size_t isr_field_grad_workspace_bytes(int n_layers, const int32_t* widths, int N);

/* pts (N, 3), dout (N, ld_dout) with ld_dout >= widths[n_layers] (only columns below widths[n_layers] are read) -> dW and
 * db in the standard layout, real entries only; every entry is written on every call, N = 0 writes zeros.  Either of dW and
 * db may be null (it is then not written).  The forward is recomputed from pts.  pack and packT: what
 * isr_field_pack_device wrote.  ws: ws_bytes bytes of device scratch, at least isr_field_grad_workspace_bytes(.., min(N, 64));
 * N is worked through in slabs of the largest multiple of 64 points the workspace holds (at most the geometry's slab),
 * and the result does not depend on the slab. */
int isr_field_backward(const void* pack, size_t pack_bytes, const void* packT, size_t packT_bytes, int n_layers,
                       const int32_t* widths, const float* pts, int N, const float* dout, int ld_dout, float* dW, float* db,
                       void* ws, size_t ws_bytes, isr_stream_t stream);

/* The same gradients as host code over HOST pointers (pack as isr_field_pack wrote it): the tests' reference. */
int isr_field_backward_host(const void* pack, size_t pack_bytes, int n_layers, const int32_t* widths, const float* pts, int N,
                            const float* dout, int ld_dout, float* dW, float* db);

/* out[i] = cos32(a[i]), host code over HOST pointers. */
int isr_field_cos_host(const float* a, size_t n, float* out);

/* The widths of the backward (tests and tools): which = 0 the chain length, 1 the tile, 2 the largest slab, 3 the batch of
 * points whose block sums are held at a time; -1 otherwise. */
int isr_field_grad_geometry(int which);

#ifdef __cplusplus
}
#endif

#endif /* ISR_FIELD_GRAD_H */
