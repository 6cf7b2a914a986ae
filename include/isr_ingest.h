/*
 * isr_ingest.h — C ABI of the sequence ingest of libisr_hip.so: the per-frame body of
 *     cowrendersynth.generate_bop_realsamples (cowrendersynth.py:667-736),
 * which turns a BOP frame and its mask into a square training view of maxB x maxB pixels and the camera matrix that follows
 * the crop.  The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(),
 * work enqueued on `stream`, no call synchronises, a refused call launches nothing and writes nothing); isr_hip.h's entry list
 * and ISR_ABI_VERSION do not change.  The device entry has a _host twin over HOST pointers in the same library, the tests'
 * reference: both are compiled from csrc/ingest.hpp, which states the arithmetic once, and the library is built with
 * -ffp-contract=off, so host and device give the same bits.  No atomics of any kind; nothing depends on scheduling order: two
 * calls give identical bytes.  Every output element is written on every accepted call.
 *
 * ---- INPUTS, per frame i of n.  rgb (n, H, W, 3) u8, mask (n, H, W, Cm) u8 with Cm in {1, 3}, K_in (n, 9) f64 (row-major
 * 3 x 3).  Scalars: maxB, offset, make_ndc, sil_mode (ISR_INGEST_SIL_*).
 *
 * ---- THE RULE (line numbers are cowrendersynth.py's).
 *   Gate (:667).  The source value of channel c at (y, x) is rgb[y, x, c] where mask[y, x, min(c, Cm - 1)] != 0, else 0:
 *     c1[np.where(m1 == 0)] = 0 is elementwise over the three mask channels; a one-channel mask gates all three.
 *   Box (:668).  x2, y2, w, h = cv2.boundingRect of mask channel 0: the box of its non-zero pixels, (0, 0, 0, 0) when there
 *     are none (isr_mask_bbox's definition).
 *   Geometry (:669-690), all integers.  w2 = w - (w & 1), h2 = h - (h & 1); hw = w2 / 2, hh = h2 / 2; maxd = max(w2, h2);
 *     side = maxd + 2 offset; hs1 = side / 2.  The canvas pixel (cy, cx) holds the gated source at
 *     (y2 + cy - (hs1 - hh), x2 + cx - (hs1 - hw)) when hs1 - hh <= cy < hs1 + hh and hs1 - hw <= cx < hs1 + hw, else 0.
 *     The canvas is never materialised.
 *   Resize (:701-704): the textbook bilinear rule for u8 images, an OWNED definition.  Output pixel (dy, dx) reads the canvas at
 *     sx = ((dx + 0.5) * side) / maxB - 0.5, sy likewise, in f64; x0 = floor(sx), fx = sx - x0; the neighbours x0, x0 + 1 (and
 *     y0, y0 + 1) are clamped into [0, side - 1] (edge replication); with w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy),
 *     w10 = (1 - fx) fy, w11 = fx fy the sum is ((p00 w00 + p01 w01) + p10 w10) + p11 w11 in f64 (csrc/crop_normalize.hip's
 *     sample_u8 order), rounded with rint (half to even) to u8; the image value is (float)u8 / 255.0f, one f32 division.
 *     cv2's own 8-bit resize is fixed-point [from memory] and can differ from this by a grey level: cv2's bytes are unpinned.
 *   Silhouette.  Mask channel 0 (ungated, its own byte values) through the same canvas.  ISR_INGEST_SIL_LINEAR: the bilinear
 *     rule above, / 255.  ISR_INGEST_SIL_NEAREST: the canvas at (floor(dy side / maxB), floor(dx side / maxB)), / 255.
 *     WHY BOTH EXIST.  The reference passes cv2.INTER_CUBIC (:702) and cv2.INTER_NEAREST (:704) as the THIRD POSITIONAL argument
 *     of cv2.resize(src, dsize, ...).  By OpenCV's signature resize(src, dsize[, dst[, fx[, fy[, interpolation]]]]) that slot is
 *     dst, so both calls run the default INTER_LINEAR — stated FROM MEMORY: cv2 is not available to this project and the
 *     claim is UNPINNED.  LINEAR is therefore the default (what the call does); NEAREST is what the call says, and gives
 *     the 0/1 silhouette that augment.PoseBatches requires when the mask holds 0/255.
 *   Camera (:717-736), f64, one operation per written operation.  cx = K[0][2] + (double)(-x2 + hs1 - hw),
 *     cy = K[1][2] + (double)(-y2 + hs1 - hh), the integers summed first (x2, y2 are the box before the even cut, hw, hh after).
 *     K = (K * maxB) / side on all nine elements; K[2][2] = 1.  If make_ndc: K = (K * 2) / maxB; K[2][2] = 0;
 *     K[0][2] = -(K[0][2] - 1); K[1][2] = -(K[1][2] - 1).  K_out (n, 16) is the row-major 4 x 4 with the 3 x 3 in its corner,
 *     [3][2] = [2][3] = 1 and +0 elsewhere.
 *
 * ---- OUTPUTS.  images (n, maxB, maxB, 3) f32; silhouettes (n, maxB, maxB) f32; K_out (n, 16) f64;
 * geom (n, 8) i32 = (x2, y2, w2, h2, hw, hh, side, hs1); status (n) i32.
 * side == 0 needs offset == 0 and a box of at most one pixel a side; the reference would fail inside cv2.  Such a frame gets
 * status 1, +0 in images and silhouettes and a quiet NaN (0x7ff8000000000000) in all 16 elements of its K_out row; its geom
 * row is still the rule's.  Every other frame has status 0; an empty mask with offset > 0 is an ordinary frame (a black
 * image, the camera shifted by the rule).
 *
 * ---- THE KERNELS: three launches per call, whatever n is.  (1) The box pass: frames on blockIdx.z (groups of
 * ISR_INGEST_FRAME_GROUP on blockIdx.y), strips of rows on blockIdx.x; a workgroup of 256 reads its strip's mask bytes with
 * 16-byte loads (one-by-one head and tail where the strip's first and last byte are not 16-aligned), reduces min / max over 64
 * lanes with cross-lane moves and over its four waves in LDS, and stores its partial box to the workspace (n, strips, 4) i32.
 * (2) The geometry pass: one thread per frame folds the strips in strip order and writes geom, status and K_out.  (3) The
 * resize pass: one lane per output pixel does the three colours and the silhouette from the same four neighbour addresses.
 * The box never visits the host.
 *
 * LIMITS.  1 <= n <= ISR_INGEST_FRAME_GROUP * 65535; 1 <= H, W with H W <= 2^28; 1 <= maxB <= 4096; 0 <= offset <= 4096;
 * Cm in {1, 3}; sil_mode one of ISR_INGEST_SIL_*; the workspace 16-byte aligned and workspace_bytes >=
 * isr_ingest_workspace_bytes; outputs and workspace overlap no input and not each other.  Anything else is ISR_ERR_ARG with a
 * message.
 */
#ifndef ISR_INGEST_H
#define ISR_INGEST_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_INGEST_SIL_LINEAR 0
#define ISR_INGEST_SIL_NEAREST 1
#define ISR_INGEST_FRAME_GROUP 64
#define ISR_INGEST_MAX_B 4096
#define ISR_INGEST_MAX_OFFSET 4096

/* Bytes of device workspace for n frames of H x W with Cm mask channels; 0 when the shape is refused. */
size_t isr_ingest_workspace_bytes(int n, int H, int W, int Cm);

int isr_ingest_views(const uint8_t* rgb, const uint8_t* mask, const double* K_in, int n, int H, int W, int Cm, int maxB,
                     int offset, int make_ndc, int sil_mode, float* images, float* silhouettes, double* K_out, int32_t* geom,
                     int32_t* status, void* ws, size_t workspace_bytes, isr_stream_t stream);

int isr_ingest_views_host(const uint8_t* rgb, const uint8_t* mask, const double* K_in, int n, int H, int W, int Cm, int maxB,
                          int offset, int make_ndc, int sil_mode, float* images, float* silhouettes, double* K_out,
                          int32_t* geom, int32_t* status);

/* 0: threads per workgroup, 1: frames per blockIdx.z group, 2: launches per call; else -1. */
int isr_ingest_geometry(int which);

/* Rows per strip and strips per frame of the box pass for a frame of H x W x Cm; 0 when the shape is refused. */
int isr_ingest_strip_rows(int H, int W, int Cm);
int isr_ingest_strips(int H, int W, int Cm);

/* The launch floor: the call's three launches with empty kernels over n frames (for tools/bench_ingest.py). */
int isr_ingest_launch_floor(int n, int H, int W, int Cm, int maxB, isr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISR_INGEST_H */
