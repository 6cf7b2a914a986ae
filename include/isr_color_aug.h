/*
 * isr_color_aug.h — C ABI of the colour augmentation of libisr_hip.so: the albumentations pass of augment.py:344-350,
 *     Compose([ColorJitter(), RandomBrightnessContrast(p=0.2), GaussianBlur(blur_limit=(1, 3)), ISONoise(), CLAHE()]),
 * which generateImages applies to the object's pixels (:394-397) and to the whole composite (:422-423).  The conventions are
 * those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call
 * synchronises, a refused call launches nothing and writes nothing); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 * The device entry has a _host twin over HOST pointers in the same library, the tests' reference: both are compiled from
 * csrc/color_aug.hpp, which states the arithmetic once, and the library is built with -ffp-contract=off, so host and device
 * give the same bits.  No float atomics; nothing depends on scheduling order: two calls give identical bytes.
 *
 * WHAT IS PINNED TO WHAT.  The u8 round trip: NumPy's (x * 255).astype(uint8) and .astype(float32) / 255.  The brightness,
 * contrast and saturation blends: PIL's ImageEnhance within one level; the blur's interior: PIL's ImageFilter.Kernel, byte for
 * byte.  The hue model: the standard library's colorsys, formula for formula.  Philox4x32-10: Random123's known answers
 * (csrc/hd.hpp).  UNPINNED, owned definitions written from the libraries' documented behaviour: every byte of
 * albumentations' and cv2's own output.  Stated differences: (a) cv2 rotates hue in 8-bit HSV with a 2-degree hue; here the
 * rotation is colorsys' HLS in f64 (a rotation keeps a pixel's channel maximum and minimum in both models, so they agree up to
 * cv2's quantisation), and one colour model serves ColorJitter and ISONoise; (b) ISONoise's hue noise is an Irwin-Hall sum of
 * twelve uniforms, not NumPy's normal: its tails end at 6 sigma, and host and device need no logarithm or cosine to agree on;
 * (c) CLAHE equalises the luma Y = gray and keeps the chroma R - Y, G - Y, B - Y, where the libraries use L* of CIE LAB (a cube
 * root and a 2.4 power that host and device libraries round differently); (d) the draws are the caller's (programs), not
 * albumentations' stream.
 *
 * ---- THE PASS.  in (B, H, W, 3) f32 in [0, 1] -> out (B, H, W, 3) f32, under one isr_color_program per image (HOST memory,
 * travels as kernel arguments).  program.pass == 0: the image's f32 bytes are the pass's result, untouched (no quantisation).
 * Otherwise, with v a u8 channel value and "round" = clip(rint(value), 0, 255) in f64, rint half to even:
 *   1. q = (uint8)(x * 255.0f): an f32 product, clamped to [0, 255] (NaN -> 0), truncated.
 *   2. jitter != 0 — ColorJitter: the four steps order[0..3] (a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue).
 *      gray(R, G, B) = round((0.299 R + 0.587 G) + 0.114 B).
 *        brightness  v <- round(v * brightness)
 *        contrast    v <- round(v * contrast + m * (1 - contrast)), m = rint(sum of gray / (H W)) over the image at that step
 *        saturation  v <- round(v * saturation + g * (1 - saturation)), g the pixel's gray at that step
 *        hue         (h, l, s) = colorsys.rgb_to_hls(R / 255, G / 255, B / 255); h <- frac(h + hue), frac(t) = t - floor(t)
 *                    (Python's t % 1.0); (R, G, B) <- round(colorsys.hls_to_rgb(h, l, s) * 255)
 *   3. rbc != 0 — RandomBrightnessContrast: v <- round(v * alpha + beta * 255).
 *   4. ksize == 3 — GaussianBlur: the separable [1, 2, 1] / 4 kernel (cv2's fixed kernel for size 3, sigma 0), border
 *      reflect-101, in integers: (sum of the nine weighted neighbours + 8) >> 4.  ksize 0 (gate off) and 1: identity.
 *   5. iso != 0 — ISONoise.  Per pixel li = max + min of the channels (0..510).  sigma_L = sqrt(N sum(li^2) - sum(li)^2) /
 *      (510 N), the sums exact integers, N = H W; lambda = (sigma_L * intensity) * 255.
 *      cdf: p_0 = exp64(-lambda) (csrc/field_density.hpp's), p_k = (p_{k-1} * lambda) / k, cdf_k = cdf_{k-1} + p_k, k < 256.
 *      Philox counter (pixel index y W + x, tag, draw, 0), key = noise_key (low word, high word).
 *      k: tag 0, draw 0, word 0: u = (w + 0.5) 2^-32; the smallest k with u <= cdf_k, 255 when there is none.
 *      z: tag 1, draws 0..2: the twelve words >> 8 summed as integers, times 2^-24, minus 6.
 *      (h, l, s) as in the hue step; l <- l + (k / 255) (1 - l); h <- frac(h + (sigma_h * z) / 360), sigma_h = (color_shift *
 *      360) * intensity; (R, G, B) <- round(hls_to_rgb(h, l, s) * 255).
 *   6. clahe != 0 — CLAHE on an 8 x 8 grid of tiles of tw = W / 8 by th = H / 8 pixels, area = tw th, on Y = gray:
 *      clip = max((int)((clip_limit * area) / 256), 1).  Per tile: the histogram h of Y; excess = sum max(h - clip, 0);
 *      h <- min(h, clip) + excess / 256; residual = excess % 256 spread one count at a time over bins 0, step, 2 step, ...
 *      (step = max(256 / residual, 1)) while bins and residual last; lut_i = round((cdf_i * 255) / area).
 *      Per pixel: txf = x / tw - 0.5, tx1 = floor(txf), xa = txf - tx1, tx2 = tx1 + 1, both clamped to [0, 7]; rows likewise;
 *      Y' = round((lut[ty1][tx1][Y] (1 - xa) + lut[ty1][tx2][Y] xa) (1 - ya) + (lut[ty2][tx1][Y] (1 - xa) + lut[ty2][tx2][Y] xa)
 *      ya); v <- clip(Y' + (v - Y), 0, 255).
 *   7. x' = (float)q / 255.0f.
 * Compose's order with each transform's own probability (0.5, 0.2, 0.5, 0.5, 0.5) is the Python layer's draw.
 *
 * ---- TWO OPTIONAL ENDS.  select (B, H, W) f32 holding 0/1 and under (B, H, W, 3) f32 or null: y = x' where select == 1,
 * else under (0 when under is null); select null: y = x'.  The tail: border_host (B, 2) i32 = (kh, kw) with border_mask
 * (B, H, W) f32 — y = 0 where isr_augment.h's dilation of border_mask is <= 0.9 — and mean3 / std3 (HOST, 3 f32 each, both or
 * neither): out = (y - mean3[c]) / std3[c], the functions of csrc/augment.hpp.  Null means off: out = y.
 *
 * ---- THE KERNELS.  Per 16 images a chain of at most eight launches, each skipped when no image's program asks for its stage:
 * the bytes with the jitter steps before the contrast; the sum of gray (one workgroup per image); the contrast, the steps
 * after it and RandomBrightnessContrast; the blur; ISONoise's sums and cdf (one workgroup per image, one lane for the chain);
 * ISONoise's pixels; CLAHE's tables (one workgroup per tile and image); the finish (CLAHE's look-ups, f32, both ends).  The
 * per-pixel launches give every 256 pixels a workgroup.  Between launches the image's bytes sit in a per-image workspace: two
 * u8 buffers of H W 3 bytes, each rounded up to 256 (the blur reads one and writes the other), the 64 tables (16 384 bytes),
 * the cdf (2 048) and the sum (256).  What one launch writes the next one reads: no hand-off between workgroups, no fence.
 * Histogram counts use integer LDS atomics (counts do not depend on order); nothing else is atomic.
 *
 * LIMITS.  1 <= B; H, W multiples of 8, >= 8, H W <= 2^20; every factor finite; brightness, contrast, saturation, alpha,
 * color_shift, intensity >= 0; clip_limit >= 1; ksize in {0, 1, 3}; order a permutation of 0..3; 0 <= kh, kw <= 255;
 * std3 != 0; out and the workspace overlap no input and not each other; the workspace 8-byte aligned, workspace_bytes >=
 * isr_color_aug_workspace_bytes.
 * Programs are checked whether their gates are on or off.  Anything else is ISR_ERR_ARG with a message.
 */
#ifndef ISR_COLOR_AUG_H
#define ISR_COLOR_AUG_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_COLOR_AUG_MAX_PIXELS (1 << 20)
#define ISR_COLOR_AUG_GRID 8

/* One image's program: 120 bytes, no padding (ten i32, nine f64, one u64). */
typedef struct isr_color_program {
  int32_t pass;      /* 0: the image is returned untouched */
  int32_t jitter;    /* ColorJitter on */
  int32_t order[4];  /* 0 brightness, 1 contrast, 2 saturation, 3 hue */
  int32_t rbc;       /* RandomBrightnessContrast on */
  int32_t ksize;     /* GaussianBlur: 0 off, else 1 or 3 */
  int32_t iso;       /* ISONoise on */
  int32_t clahe;     /* CLAHE on */
  double brightness, contrast, saturation, hue;
  double alpha, beta;
  double color_shift, intensity;
  double clip_limit;
  uint64_t noise_key;
} isr_color_program;

/* Bytes of device workspace for B images of H x W; 0 when the shape is refused. */
size_t isr_color_aug_workspace_bytes(int B, int H, int W);

int isr_augment_color(const float* in, int B, int H, int W, const isr_color_program* programs_host, const float* select,
                      const float* under, const int32_t* border_host, const float* border_mask, const float* mean3,
                      const float* std3, float* out, void* ws, size_t workspace_bytes, isr_stream_t stream);

int isr_augment_color_host(const float* in, int B, int H, int W, const isr_color_program* programs_host, const float* select,
                           const float* under, const int32_t* border_host, const float* border_mask, const float* mean3,
                           const float* std3, float* out);

/* The noise draws of pixels 0 .. n-1 under noise_key at a given lambda, as host code: k_out (n) i32, z_out (n) f64.  For tests. */
int isr_color_aug_draws_host(uint64_t noise_key, int n, double lambda, int32_t* k_out, double* z_out);

/* 0: threads per workgroup of the per-pixel launches, 1: images per launch, 2: the most launches per 16 images,
   3: sizeof(isr_color_program); else -1. */
int isr_color_aug_geometry(int which);

#ifdef __cplusplus
}
#endif

#endif /* ISR_COLOR_AUG_H */
