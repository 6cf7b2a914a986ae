/*
 * isr_seq_refit.h — C ABI of the sequence-level pose of libisr_hip.so: one robust Gauss-Newton over the reprojection
 * residuals of every frame's 2D-3D matches, for the rigid transform Y between two sequences.  Frame i of the second sequence
 * has a known pose G_i in its own sequence's frame and sees the first sequence's model under P_i = G_i Y; every frame's
 * matches constrain the same six numbers.  The conventions are those of isr_hip.h (return value ISR_OK or a negative
 * ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call synchronises); isr_hip.h's entry list and
 * ISR_ABI_VERSION do not change.
 *
 * THE RULE is stated once, in csrc/seq_refit.hpp, which is also its arithmetic for the kernels and for the _host entry; in
 * short, per pass:
 *   row of frame i, slot m < min(counts[i], cap):  q = Y p,  c = G_i q,  r = pi(K_i, c) - u  (2 values, pixels),
 *   a = |r|,  w = frame_w[i] * weight(kernel, k, a)  (ISR_ICP_L2 / _HUBER / _TUKEY of isr_icp_plane.h, k in pixels),
 *   J = J_pi(K_i, c) R_i [ -[q]x | I ]  (2 x 6: a left perturbation of Y); the row counts iff c.z > 0, every value is
 *   finite and w > 0;
 *   31 f64 sums in the layout of isr_icp_plane.h (sum a, sum r.r, rows; the upper triangle of sum w J^T J; sum w J^T r;
 *   sum w r.r) in a fixed order — a tree per 64 slots, ((w0 + w1) + w2) + w3 per 256-slot block, 16 lanes over a frame's
 *   blocks, 16 lanes over the frames — no float atomics: a function of the inputs and n only, and not of cap;
 *   stop, tested in this order: the solved step has max |rotation| < tol_r and max |translation| < tol_t -> status 0
 *   (the step is not applied);  rows < 6 -> 2;  pass >= max_iter -> 1;  singular system -> 3;  otherwise Y <- dT(x) Y with
 *   the unrolled 6x6 Cholesky and the quaternion update of isr_icp_plane.h.  A stopped call keeps the Y it had.
 * OWNED: the reference has no such estimator; nothing here is pinned to a library.
 * Non-finite inputs never make an access leave the arrays: their rows do not count.
 */
#ifndef ISR_SEQ_REFIT_H
#define ISR_SEQ_REFIT_H

#include <stddef.h>
#include <stdint.h>

#include "isr_icp_plane.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of `state`: Y 4x4 row-major (start in rows 0..2, result out; row 3 is written as 0 0 0 1) |
 * mean a, rms = sqrt(sum r.r / rows), passes, rows counted |
 * status (0 converged, 1 max_iter, 2 rows < 6, 3 singular), sum w r.r, two reserved zeros: all of the last pass.
 * Every double beyond the start is written by every call, whatever the buffer held. */
#define ISR_SEQ_REFIT_STATE_DOUBLES 24
/* Doubles per frame of `frame_stats`: rows counted, sum w, sum w r.r, sum r.r at the last pass (the labelling QA signal). */
#define ISR_SEQ_REFIT_FRAME_STATS 4

/* Bytes of scratch isr_seq_refit needs; 0 for n < 1 or cap < 1. */
size_t isr_seq_refit_workspace_bytes(int n, int cap);

/* p3d (n, cap, 3) f32 model-frame points, p2d (n, cap, 2) f32 pixels, counts (n) i32 (the first counts[i] slots of frame i
 * are real; a count above cap cannot be seen from the host and is clamped to cap by the kernels, a negative one is 0),
 * frame_w (n) f64 or null (null: every frame weighs 1; 0 drops a frame), K (n, 9) f64 row-major cameras, G (n, 12) f64
 * [R_i | t_i] row-major, state (24) f64, frame_stats (n, 4) f64: all on the device.
 * 3 (max_iter + 1) launches on `stream`, no host read: a pass is accumulate (grid (ceil(cap / 256), n)), the per-frame
 * reduction, and the cross-frame reduction with the solve; passes after the stop see a flag and return at once.  n = 0 is
 * one launch, which writes the state with status 2.
 * Refused with ISR_ERR_ARG before any launch: a null state, with n > 0 any other null array (frame_w excepted: null is
 * its default) and a null or short workspace, cap < 1, n outside [0, 65535], max_iter < 0, an unknown kernel, k <= 0 with
 * ISR_ICP_HUBER or ISR_ICP_TUKEY. */
int isr_seq_refit(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w, const double* K,
                  const double* G, int n, int cap, int kernel, double k, int max_iter, double tol_r, double tol_t, double* state,
                  double* frame_stats, void* ws, size_t ws_bytes, isr_stream_t stream);

/* The same loop as host code over HOST pointers: the same bits.  For tests and CPU users. */
int isr_seq_refit_host(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w, const double* K,
                       const double* G, int n, int cap, int kernel, double k, int max_iter, double tol_r, double tol_t,
                       double* state, double* frame_stats);

/* The 31 sums of ONE pass at Y (its first 12 doubles are read), formed as the loop forms them, over HOST pointers:
 * sums[0] sum a, [1] sum r.r, [2] rows, [3..23] the upper triangle of sum w J^T J row by row, [24..29] sum w J^T r,
 * [30] sum w r.r; frame_stats (n, 4) as above.  For tests. */
int isr_seq_refit_sums_host(const float* p3d, const float* p2d, const int32_t* counts, const double* frame_w, const double* K,
                            const double* G, int n, int cap, int kernel, double k, const double* Y, double* sums,
                            double* frame_stats);

#ifdef __cplusplus
}
#endif

#endif /* ISR_SEQ_REFIT_H */
