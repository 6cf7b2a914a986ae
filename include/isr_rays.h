/*
 * isr_rays.h — C ABI of the ray bundles of libisr_hip.so: cameras in, rays out, on the device.  These entries are what
 * generateCors.py:125-138, :279-304 and genFeat.py:102-106, :162-189 get from pytorch3d's PerspectiveCameras,
 * NDCMultinomialRaysampler and MonteCarloRaysampler, and what pren.py:229-236 selects with a silhouette through
 * nutil.sample_images_at_mc_locs (nutil.py:167-196).  The conventions are those of isr_hip.h (return value ISR_OK or a
 * negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h's entry list and
 * ISR_ABI_VERSION do not change.  Every device entry has a _host twin over HOST pointers in the same library, the tests'
 * reference: host and device use only + - * / and explicit fmaf in f32 (the library is built with -ffp-contract=off) and give
 * the same bits.  csrc/rays.hpp states the arithmetic once.
 *
 * WHAT IS PINNED TO WHAT.  linspace: to torch.linspace (CPU, f32), bit for bit.  The image sampling: to
 * torch.nn.functional.grid_sample(mode='nearest', align_corners=True), value for value.  Philox4x32-10: to Random123's
 * known-answer vectors.  The camera convention, the NDC conversion of screen-space intrinsics (done by the Python layer), the
 * grid's extent for W != H and the strata rule are pytorch3d's AS FAR AS THEY ARE KNOWN FROM MEMORY — pytorch3d is not
 * available to compare against: those rules are UNPINNED.  The signs are held to something physical instead: a BOP pose
 * converted by generateCors.py:98-102's two statements, a world point X in front of the camera and its OpenCV pixel give a ray
 * with origin + direction * Z_cam = X (tests/test_rays_cpu.py).
 *
 * CAMERA.  Row vectors, as pytorch3d documents them: X_cam = X_world R + T, x_ndc = fx X/Z + px, y_ndc = fy Y/Z + py; NDC is
 * +x left, +y up.  R (B, 3, 3) row-major, T (B, 3), intr (B, 4) = (fx, fy, px, py) IN NDC, all f32.  PRECONDITION: fx, fy != 0.
 *
 * THE RAY OF AN NDC POINT (x, y).  With dot3(a, r) = fmaf(a2, r2, fmaf(a1, r1, a0 * r0)) and R_i the i-th ROW of R:
 *     c = ((x - px) / fx, (y - py) / fy, 1);   directions_i = dot3(c, R_i)   (c R^T; not normalised)
 *                                              origins_i    = dot3(-T, R_i)  ((-T) R^T: the camera centre)
 * the closed form of pytorch3d's "unproject the planes z = 1 and z = 2, direction = plane2 - plane1, origin = plane1 -
 * direction", without the rounding noise of its 4x4 inverse.  origin + direction * z is the world point at camera depth z.
 *
 * linspace(a, b, P) in f32: step = (b - a) / (P - 1); element k is fmaf(step, k, a) for k < P / 2 (integer division), otherwise
 * fmaf(-step, P - 1 - k, b); for P = 1 it is a.
 *
 * GRID (mode ISR_RAYS_GRID; n = W H rays per camera; min_x .. max_y, stratified, seed and camera_ids are not read).
 * range_x = W / H and range_y = 1 when W >= H, otherwise range_x = 1 and range_y = H / W;
 *     xs = linspace(range_x - range_x / W, -range_x + range_x / W, W),   ys likewise with range_y and H,
 * the end points computed in f64 and rounded to f32 once.  Ray r = i W + j (raster order, y outer) has xy = (xs[j], ys[i]):
 * pixel (row i, column j), whose OpenCV centre is (u, v) = (j + 0.5, i + 0.5).  lengths = linspace(min_depth, max_depth, P) for
 * every ray.
 *
 * MONTE-CARLO (mode ISR_RAYS_MC; n rays per camera; W and H are not read).  torch's random stream is not reproduced.
 * Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (camera_id, ray, tag, block);
 * u = (word >> 8) * 2^-24, in [0, 1).  camera_ids (B,) int32 or null for 0 .. B-1: a ray is a function of (seed, camera_id, ray
 * index) only, not of the batch it rides in.
 *     tag 0, block 0:  x = fmaf(u(word 0), max_x - min_x, min_x),  y = fmaf(u(word 1), max_y - min_y, min_y)
 * in [min, max] and, whenever (max - min) 2^-24 is at least half the spacing of f32 below max (it is for -1 .. 1), below max.
 * lengths = linspace(min_depth, max_depth, P) =: l, and with stratified != 0 (pytorch3d's _jiggle_within_stratas, from memory):
 *     lower_k = k == 0 ? l_0 : 0.5 (l_{k-1} + l_k),   upper_k = k == P-1 ? l_{P-1} : 0.5 (l_k + l_{k+1}),
 *     l'_k = fmaf(upper_k - lower_k, u, lower_k),   u = u(word k % 4) of tag 1, block k / 4:
 * inside [lower_k, upper_k], so l' does not decrease along a ray.
 *
 * IMAGE SAMPLING AT RAYS (isr_sample_nearest; nutil.py:188-193).  images (B, H, W, C) f32, xys (B, n, 2) -> out (B, n, C):
 *     g = -xy;   ix = rint(((g_x + 1) / 2) * (W - 1)),  iy = rint(((g_y + 1) / 2) * (H - 1))   in f32, halves to even;
 * out = images[b, iy, ix, :], zeros where ix or iy falls outside the image (NaN included).
 *
 * MASK SELECTION (pren.py:230-236).  mask (B, mh, mw) f32; candidate ray (b, r) is kept when the mask sampled at its xy by
 * the rule above is non-zero (NaN is non-zero, as for torch.where).  The kept rays are compacted in (camera, ray) order —
 * torch.where's — by count, scan and emit, without atomics: the order is fixed.  isr_rays_select_count writes the number of
 * kept rays to count_dev and prepares the workspace; isr_rays_select_emit, given the same arguments and that workspace,
 * writes kept ray i < cap to row i of origins, directions (cap, 3), lengths (cap, P), xys (cap, 2) and src (cap) — src: the
 * candidate's index b n + r — and ZEROS to the rows from count to cap: every byte of the outputs is written.  A cap short of
 * the count loses rows; nothing is written outside.
 *
 * LIMITS.  B >= 1, B n <= 2^28 (grid: n = W H; W, H >= 1), 1 <= P <= 4096, finite depths and ranges with min <= max,
 * mask and image sides >= 1 with at most 2^28 pixels per image, 1 <= C <= 4096 and B n C < 2^31, 0 <= cap <= 2^28.  Anything
 * else is ISR_ERR_ARG with a message.
 */
#ifndef ISR_RAYS_H
#define ISR_RAYS_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_RAYS_GRID 0
#define ISR_RAYS_MC 1

/* Bytes of scratch the selection needs for B cameras of n candidate rays; 0 (and isr_last_error()) for a refused shape. */
size_t isr_rays_workspace_bytes(int B, int n);

/* Every candidate ray: origins, directions (B, n, 3), lengths (B, n, P), xys (B, n, 2) f32 on the device. */
int isr_rays_bundle(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B, int W, int H,
                    int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth, float max_depth,
                    int stratified, uint64_t seed, float* origins, float* directions, float* lengths, float* xys,
                    isr_stream_t stream);

int isr_rays_bundle_host(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B, int W,
                         int H, int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth,
                         float max_depth, int stratified, uint64_t seed, float* origins, float* directions, float* lengths,
                         float* xys);

/* The number of candidate rays the mask keeps -> count_dev (one int32 on the device).  The workspace needs no preparation,
 * may be reused, and is what isr_rays_select_emit reads. */
int isr_rays_select_count(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B, int W,
                          int H, int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth,
                          float max_depth, int stratified, uint64_t seed, const float* mask, int mh, int mw, int32_t* count_dev,
                          void* ws, size_t ws_bytes, isr_stream_t stream);

/* The kept rays, after isr_rays_select_count with the same arguments on the same stream.  cap: rows of the outputs. */
int isr_rays_select_emit(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B, int W,
                         int H, int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth,
                         float max_depth, int stratified, uint64_t seed, const float* mask, int mh, int mw, const void* ws,
                         size_t ws_bytes, int64_t cap, float* origins, float* directions, float* lengths, float* xys, int32_t* src,
                         isr_stream_t stream);

int isr_rays_select_count_host(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B,
                               int W, int H, int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth,
                               float max_depth, int stratified, uint64_t seed, const float* mask, int mh, int mw, int32_t* count);

int isr_rays_select_emit_host(int mode, const float* R, const float* T, const float* intr, const int32_t* camera_ids, int B,
                              int W, int H, int n, int P, float min_x, float max_x, float min_y, float max_y, float min_depth,
                              float max_depth, int stratified, uint64_t seed, const float* mask, int mh, int mw, int64_t cap,
                              float* origins, float* directions, float* lengths, float* xys, int32_t* src);

/* images (B, H, W, C), xys (B, n, 2) on the device -> out (B, n, C). */
int isr_sample_nearest(const float* images, int B, int H, int W, int C, const float* xys, int n, float* out, isr_stream_t stream);

int isr_sample_nearest_host(const float* images, int B, int H, int W, int C, const float* xys, int n, float* out);

/* Philox4x32-10 of counter[4] under key[2] -> words[4] and, unless null, units[4] = (word >> 8) * 2^-24.  Host only. */
int isr_rays_philox_host(const uint32_t* counter, const uint32_t* key, uint32_t* words, float* units);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RAYS_H */
