/*
 * isr_sample_grad.h — C ABI of the backward of isr_sample_nearest (isr_rays.h) in libisr_hip.so: the gradient of
 * nutil.sample_images_at_mc_locs with respect to the images, which is what lets trainPose.py's contrastive loss train the
 * encoder (trainPose.py:397-400, :423, :449).  The conventions are those of isr_hip.h (return value ISR_OK or a negative
 * ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h's entry list and
 * ISR_ABI_VERSION do not change.
 *
 * The rule (csrc/sample_grad.hpp is the one place it is written).  dout (B, n, C) f32, xys (B, n, 2) f32, an image of H x W
 * pixels -> dimages (B, H, W, C) f32.  With ix = nearest_pixel(xys[b,r,0], W) and iy = nearest_pixel(xys[b,r,1], H) — the
 * forward's own function (csrc/rays.hpp), so that the two never disagree on a tie or a NaN — ray r of image b belongs to
 * pixel (iy, ix) when both are >= 0 and to no pixel otherwise (outside on any side, or a NaN coordinate).  Then
 *     dimages[b,iy,ix,c] = acc after  acc = acc + dout[b,r,c]  over the pixel's rays, r ascending, from acc = +0
 * in f32: one serial chain per (pixel, channel).  A pixel with no ray is +0 in every channel; a pixel whose only ray
 * carries -0 is +0; a NaN or an infinity in dout reaches exactly the (pixel, channel) entries it is added into.
 * The result is a function of (dout, xys, H, W) only — not of the launch, the workspace size or a previous call — with no
 * float atomics anywhere, and the same bits from isr_sample_nearest_backward and isr_sample_nearest_backward_host.
 *
 * Limits: B, H, W, C, n at least 1, C <= 4096, B n <= 2^28, B n C < 2^31 (the forward's), H W < 2^31 - 1, B H W C < 2^40.
 */
#ifndef ISR_SAMPLE_GRAD_H
#define ISR_SAMPLE_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace isr_sample_nearest_backward wants: the sorted (pixel, ray) list of every image, and above
 * isr_sample_grad_geometry(0) rays per image a second list and the radix sort's (digit, block) table.  0 (and
 * isr_last_error()) for a shape out of range. */
size_t isr_sample_grad_workspace_bytes(int B, int H, int W, int n);

/* DEVICE pointers.  Every element of dimages is written by every successful call, whatever the buffer held.  ws: ws_bytes
 * bytes of device scratch, at least isr_sample_grad_workspace_bytes(B, H, W, n); a smaller one is refused. */
int isr_sample_nearest_backward(const float* dout, int B, int H, int W, int C, const float* xys, int n, float* dimages, void* ws,
                                size_t ws_bytes, isr_stream_t stream);

/* The same gradient as host code over HOST pointers: the tests' reference. */
int isr_sample_nearest_backward_host(const float* dout, int B, int H, int W, int C, const float* xys, int n, float* dimages);

/* The constants the tests need: which = 0 the largest n sorted in LDS by one workgroup per image, 1 the keys per block of
 * the radix sort above it, 2 the bits of a radix digit; -1 otherwise. */
int isr_sample_grad_geometry(int which);

#ifdef __cplusplus
}
#endif

#endif /* ISR_SAMPLE_GRAD_H */
