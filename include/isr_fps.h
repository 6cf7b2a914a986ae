/*
 * isr_fps.h — C ABI of farthest-point sampling (FPS) in libisr_hip.so.
 *
 * The reference thins its key candidates with pytorch3d.ops.sample_farthest_points on the CPU (genFeat.py:198-201).  These
 * entries do it on the device, for B clouds at once.  The arithmetic and the tie rule are stated in csrc/fps.hpp:
 *     s_0 = start;  mind[i] = +inf;  for k = 1 .. K-1:
 *         d = fmaf(dz, dz, fmaf(dy, dy, dx*dx)) to s_{k-1} in f32;  mind[i] = fminf(mind[i], d);
 *         s_k = the index of the largest mind[i], the LOWEST index among equal values;
 *     radius2[k] = mind[s_k] at its selection, radius2[0] = +inf;  entries k >= len: idx = -1, radius2 = 0.
 * The result is a function of (points, len, start, K) only, and isr_fps_sample and isr_fps_sample_host give the same bits.
 * Finite coordinates in the first len points of every cloud are a precondition; points past len are never read.
 * The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), the caller
 * owns every buffer, work enqueued on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 */
#ifndef ISR_FPS_H
#define ISR_FPS_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace isr_fps_sample needs for B clouds of up to M points; 0 (and isr_last_error()) for B < 1, M < 1 or
 * M > 2^30. */
size_t isr_fps_workspace_bytes(int B, int M);

/* pts (B, M, 3) f32 on the DEVICE; lengths and start are HOST arrays of B entries (null: every length M, every start 0),
 * read before the call returns; idx (B, K) i32 and radius2 (B, K) f32 (nullable) on the device, every element written
 * whatever the buffers held.  K launches of one step each are enqueued on `stream`: no workgroup waits for another.
 * Refused before any device access: a null pts, idx or ws, B < 1, M < 1 or > 2^30, K < 1, a length outside 1..M, a start
 * outside 0..length-1, ws_bytes < isr_fps_workspace_bytes(B, M). */
int isr_fps_sample(const float* pts, int B, int M, const int32_t* lengths, const int32_t* start, int K, int32_t* idx,
                   float* radius2, void* ws, size_t ws_bytes, isr_stream_t stream);

/* The same sampling as host code over HOST pointers (one thread): the tests' reference. */
int isr_fps_sample_host(const float* pts, int B, int M, const int32_t* lengths, const int32_t* start, int K, int32_t* idx,
                        float* radius2);

/* Measurement only (tools/bench_fps.py): `launches` back-to-back launches of an empty kernel on `stream`, the floor under
 * the cost of a step. */
int isr_fps_launch_floor(int launches, isr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISR_FPS_H */
