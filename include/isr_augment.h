/*
 * isr_augment.h — C ABI of the training-batch front end of libisr_hip.so: from device-resident training views and their
 * correspondences to the arguments of training.pose_train_step, with no host round trip per batch.  These entries are the
 * geometric core of augment.py:284-432 (generateImages: two warps of the image and of the occluded mask, one of the original
 * mask, the paste over the canvas, the borderADD blanking) with dataGen.py:16-20 (normalize), and augment.py:639-685
 * (getNerfSamples: the affine remap of the ray locations, the inside filter and the random sample).  The conventions are those
 * of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call
 * synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.  Every device entry has a _host twin over HOST
 * pointers in the same library, the tests' reference: both are compiled from csrc/augment.hpp, which states the arithmetic
 * once, and the library is built with -ffp-contract=off, so host and device give the same bits.
 *
 * The per-image parameters (affine matrices, shifts, rectangles, kernel sizes, view ids, ray matrices) are small and are drawn
 * on the host: they are HOST pointers in both builds and travel as kernel arguments.  The kernels call no sine or cosine.
 *
 * WHAT IS PINNED TO WHAT.  The warp: to oracle/preprocess_oracle.warp_affine's definition (the textbook one, shared with
 * csrc/crop_normalize.hip) and, independently, to torch.nn.functional.grid_sample in f64.  normalize: to torch's f32
 * expression of dataGen.py:16-20, bit for bit.  The ray remap and the candidate set: to the executed lines of
 * augment.py:639-685 (tests/golden/ref_augment.npz).  Philox4x32-10: Random123's known answers (csrc/hd.hpp).  UNPINNED,
 * from memory: cv2.warpAffine's own bytes (OpenCV quantises the sample position to 1/32 px and the weights to 2^-15; this
 * definition does not, so parity with cv2 is unpinned and the definition is owned), cv2.dilate's anchor and border rule, and
 * cv2.getRotationMatrix2D's formula (made by the Python layer).  torch.randperm's stream is not reproduced.
 *
 * ---- IMAGES (isr_augment_images).  Per image b, all (H, W[, 3]) row-major:
 *   rgb f32, mask u8 holding 0/1 (the mask that may carry an occluder), orig_mask u8 (may be the same pointer as mask),
 *   canvas f32 or null (null: zeros), on the device; and on the host
 *   rect (B, 4) i32 = (x, y, w, h): mask reads inside [x, x+w) x [y, y+h) give 0 (w = 0 or h = 0: none; null: none);
 *   M (B, 2, 3) f64, source -> destination as cv2.warpAffine takes it; tra, tra1 (B, 2) i32 (null: zeros);
 *   border (B, 2) i32 = (kh, kw), 0 = off (null: off); mean3, std3 f32.
 * warp(img, A)(x, y), A source -> destination: (sx, sy) = A^-1 (x, y, 1) in f64 — i00 = A11 / det, i01 = -A01 / det,
 * i10 = -A10 / det, i11 = A00 / det, i02 = -(i00 A02 + i01 A12), i12 = -(i10 A02 + i11 A12); sx = (i00 x + i01 y) + i02;
 * x0 = floor(sx), fx = sx - x0, likewise y; v = ((p00 w00 + p01 w01) + p10 w10) + p11 w11 in f64 with w00 = (1-fx)(1-fy),
 * w01 = fx (1-fy), w10 = (1-fx) fy, w11 = fx fy and neighbours outside the frame counting as 0.  u8 images: rint(v) (half to
 * even); f32 images: (float)v, one rounding.
 *   first      = warp(rgb, M + tra1),  first_mask = warp(occluded mask, M + tra1)         (the translation column + tra1)
 *   dst(x, y)  = first(x - dx, y - dy) where that pixel lies in the W x H frame, else 0;  (dx, dy) = tra - tra1
 *                — what cv2.warpAffine(first, I + (tra - tra1)) does: the first result is clipped to the frame before it is
 *                shifted, pixels shifted in from outside are 0.  dst_mask likewise from first_mask.
 *   mask_out      = dst_mask as f32;   mask_orig_out = warp(orig_mask, M + tra) as f32
 *   out(x, y, c)  = dst where dst_mask == 1, else canvas (0 when null)
 *   border (kh, kw) both > 0: out = 0 where the maximum of dst_mask over rows y - kh/2 .. y - kh/2 + kh - 1 and columns
 *                x - kw/2 .. x - kw/2 + kw - 1 (integer division; positions outside the frame ignored) is <= 0.9
 *   rgb_out       = (out - mean3[c]) / std3[c]: an f32 subtraction, then an f32 division.
 * Two launches, the second reads mask_out; no workspace.  rgb_out, mask_out and mask_orig_out must not overlap any input.
 *
 * ---- RAYS (isr_augment_rays).  A bank holds the correspondences of V views, concatenated: xys (sum n, 2) and pos (sum n, 3)
 * f32 on the device, offsets (V + 1) i64 on the HOST (view v owns rows offsets[v] .. offsets[v+1]).  Two banks in one call:
 * the front set and, unless its pointers are null, the back set (set 1).  On the host: view_ids (B,) i32, rot (B, 4) f32 =
 * (m00, m01, m10, m11), the 2x2 of getRotationMatrix2D((0, 0), trR, trS) cast to f32, and t (B, 2) f32 = trT / (imD / 2).
 *   row (x, y):  s_x = fmaf(y, m01, x * m00) - t_x,   s_y = fmaf(y, m11, x * m10) - t_y          (f32)
 *   if any s_x or s_y of the view is >= 1 or <= -1: the candidates are the rows with -1 < s_x < 1 and -1 < s_y < 1;
 *   otherwise every row is a candidate.  m: their number.
 *   candidate i gets the key (philox4x32_10(counter = (i, view id, set, 0), key = seed).x << 32) | i; the output is the
 *   min(S, m) candidates with the smallest keys, in key order: a function of (seed, view id, set, the view's rows, rot, t).
 * Outputs per set, on the device: xys_out (B, S, 2) the remapped locations, pos_out (B, S, 3), index_out (B, S) i32 (the row in
 * the view, -1 past the count), count (B,) i32 = min(S, m); rows past the count are zeros.  One workgroup per (image, set):
 * a radix select of the cut on the key's high word, an ordered gather (ranks from ballots and a scan, ties at the cut in row
 * order) and a bitonic sort in LDS.  Integer LDS atomics build the select's histograms (counts only); no float atomics, none
 * that decide order.  No workspace.
 *
 * LIMITS.  Images: 1 <= B, 1 <= H, W, H W <= 2^28, det(M) != 0 and finite, |tra|, |tra1| <= 2^24, rect w, h >= 0,
 * 0 <= kh, kw <= 255, std3 != 0.  Rays: 1 <= B, 1 <= S <= 4096, 1 <= V, offsets non-decreasing from 0, a view's n <= 2^20,
 * 0 <= view id < V.  Anything else is ISR_ERR_ARG with a message.
 */
#ifndef ISR_AUGMENT_H
#define ISR_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_AUGMENT_MAX_SAMPLE 4096
#define ISR_AUGMENT_MAX_VIEW_ROWS (1 << 20)

int isr_augment_images(const float* rgb, const uint8_t* mask, const uint8_t* orig_mask, const float* canvas, int B, int H, int W,
                       const int32_t* rect_host, const double* M_host, const int32_t* tra_host, const int32_t* tra1_host,
                       const int32_t* border_host, const float* mean3, const float* std3, float* rgb_out, float* mask_orig_out,
                       float* mask_out, isr_stream_t stream);

int isr_augment_images_host(const float* rgb, const uint8_t* mask, const uint8_t* orig_mask, const float* canvas, int B, int H,
                            int W, const int32_t* rect_host, const double* M_host, const int32_t* tra_host,
                            const int32_t* tra1_host, const int32_t* border_host, const float* mean3, const float* std3,
                            float* rgb_out, float* mask_orig_out, float* mask_out);

int isr_augment_rays(const float* xys_front, const float* pos_front, const int64_t* offsets_front_host, const float* xys_back,
                     const float* pos_back, const int64_t* offsets_back_host, int V, const int32_t* view_ids_host,
                     const float* rot_host, const float* t_host, int B, int S, uint64_t seed, float* xys_out_front,
                     float* pos_out_front, int32_t* index_out_front, int32_t* count_front, float* xys_out_back,
                     float* pos_out_back, int32_t* index_out_back, int32_t* count_back, isr_stream_t stream);

int isr_augment_rays_host(const float* xys_front, const float* pos_front, const int64_t* offsets_front_host,
                          const float* xys_back, const float* pos_back, const int64_t* offsets_back_host, int V,
                          const int32_t* view_ids_host, const float* rot_host, const float* t_host, int B, int S, uint64_t seed,
                          float* xys_out_front, float* pos_out_front, int32_t* index_out_front, int32_t* count_front,
                          float* xys_out_back, float* pos_out_back, int32_t* index_out_back, int32_t* count_back);

#ifdef __cplusplus
}
#endif

#endif /* ISR_AUGMENT_H */
