/*
 * isr_icp_plane.h — C ABI of the point-to-plane ICP of libisr_hip.so: registration_icp(source, target, threshold, init,
 * TransformationEstimationPointToPlane(kernel)) of icp.py:101-103, for B starts against one target in one call, beside
 * isr_icp_point_to_point_batch (which stays the default and keeps its bits).  The conventions are those of isr_hip.h (return
 * value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call synchronises);
 * isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * THE RULE is stated once, in csrc/icp_plane.hpp, which is also its arithmetic for the kernels and for the _host entry; in
 * short, per pass and item:
 *   p = T s in f64 (fma chain); the source point's EXACT nearest target (f64 decision of near ties, lowest index on
 *   equality); a pair counts iff s2 <= threshold^2; fitness = n / Ns, rmse = sqrt(sum s2 / n) — Euclidean, as Open3D
 *   evaluates every estimator;
 *   r = (p - t).n_t with n_t the matched target's normal AS GIVEN (not normalised);  J = [p x n_t, n_t];  w(r) by `kernel`:
 *       ISR_ICP_L2     1
 *       ISR_ICP_HUBER  1 if |r| <= k, else k / |r|
 *       ISR_ICP_TUKEY  (1 - (r/k)^2)^2 if |r| <= k, else 0
 *   31 f64 sums (sum d, sum s2, n; the upper triangle of sum w J J^T; sum w J r; sum w r^2) in a fixed order — a tree per 64
 *   rows, ((w0 + w1) + w2) + w3 per 256-row block, 16 lanes over the blocks, the lanes in order — no float atomics: a
 *   function of the inputs and Ns only;
 *   stop, tested in this order: converged (it > 0, |d fitness| < rel_fitness and |d rmse| < rel_rmse) -> status 0;
 *   it >= max_iter -> 1;  n < 6 -> 2;  singular system (a Cholesky pivot <= 0 or non-finite, or a non-finite solution) -> 3;
 *   otherwise A x = -b by an unrolled 6x6 Cholesky, x = (alpha, beta, gamma, t), and T <- dT T where dT's rotation is that
 *   of the unit quaternion of (1, alpha/2, beta/2, gamma/2).
 * The result does not depend on the sign of a normal, bit for bit.  A stopped item keeps the T it had.
 * UNPINNED, from memory (Open3D is not available to compare against): Open3D composes Rz(gamma) Ry(beta) Rx(alpha) — the two
 * agree to second order in the step and have the same fixed points — solves with LDLT, and tests d < threshold.
 * PRECONDITION: finite inputs.  Non-finite ones never make an access leave the arrays; the numbers are then unspecified.
 * OUT OF SCOPE: colored and generalized ICP, source normals, a scale estimate.
 */
#ifndef ISR_ICP_PLANE_H
#define ISR_ICP_PLANE_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_ICP_L2 0
#define ISR_ICP_HUBER 1
#define ISR_ICP_TUKEY 2

/* Doubles per item of `state`: T 4x4 row-major (start in, result out; row 3 is written as 0 0 0 1) |
 * fitness, inlier_rmse, iterations, correspondences |
 * status (0 converged, 1 max_iter, 2 n < 6, 3 singular), sum w r^2 of the last pass, two reserved zeros.
 * Every double beyond the start is written by every call, whatever the buffer held. */
#define ISR_ICP_PLANE_STATE_DOUBLES 24

/* Bytes of scratch isr_icp_point_to_plane_batch needs; 0 for Ns, Nt or B < 1. */
size_t isr_icp_point_to_plane_batch_workspace_bytes(int Ns, int Nt, int B);

/* src: B clouds of Ns points, src_item_stride floats apart (0: one cloud for all items, else >= 3 Ns); tgt (Nt, 3) and
 * tgt_normals (Nt, 3) f32; state (B, 24) f64; all on the device.  3 + 2 (max_iter + 1) launches whatever B is; every item
 * stops on its own and equals its own B = 1 call bit for bit.
 * Refused without touching a device: null pointers, Ns or Nt < 1, B outside [0, 65535], threshold <= 0, max_iter < 0, an
 * unknown kernel, k <= 0 with ISR_ICP_HUBER or ISR_ICP_TUKEY, a stride in (0, 3 Ns), a short workspace (ISR_ERR_WORKSPACE).
 * B = 0 is a no-op. */
int isr_icp_point_to_plane_batch(const float* src, size_t src_item_stride, int Ns, const float* tgt, const float* tgt_normals,
                                 int Nt, int B, double threshold, int max_iter, double rel_fitness, double rel_rmse, int kernel,
                                 double k, double* state, void* ws, size_t ws_bytes, isr_stream_t stream);

/* The same loop as host code over HOST pointers, with an f64 brute-force search: the same bits.  For tests and CPU users. */
int isr_icp_point_to_plane_batch_host(const float* src, size_t src_item_stride, int Ns, const float* tgt,
                                      const float* tgt_normals, int Nt, int B, double threshold, int max_iter,
                                      double rel_fitness, double rel_rmse, int kernel, double k, double* state);

#ifdef __cplusplus
}
#endif

#endif /* ISR_ICP_PLANE_H */
