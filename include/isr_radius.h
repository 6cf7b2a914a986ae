/*
 * isr_radius.h — C ABI of the fixed-radius neighbour count of libisr_hip.so: for every point of a cloud, how many of the
 * cloud's points lie within `radius` of it.  It is what a radius-outlier filter needs (generateCors.py:254-259 cleans the
 * marching-cubes vertices with Open3D's remove_radius_outlier before the view loop).
 * The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work
 * enqueued on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * counts[i] = #{ j : d2(i, j) <= r2 }, the point itself included, with, in f32,
 *     dx = x[j]-x[i]; dy = y[j]-y[i]; dz = z[j]-z[i];  d2 = fmaf(dz, dz, fmaf(dy, dy, dx*dx));  r = (float)radius;  r2 = r * r
 * and clamped to cap when cap > 0 (cap <= 0: the full count).  Integers, a function of the points, radius and cap only, and
 * the same from the device entry and the _host entry (csrc/radius_count.hpp states the rule and the cell grid once).
 * PRECONDITION: finite coordinates.  Non-finite ones never make an access leave the arrays; the counts are then unspecified.
 */
#ifndef ISR_RADIUS_H
#define ISR_RADIUS_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch isr_radius_count needs for N points; 0 (and isr_last_error()) for N outside 1..2^30. */
size_t isr_radius_workspace_bytes(int N);

/* pts (N, 3) f32 on the device -> counts (N,) int32.  Refused: N < 1, a radius that is not finite, not positive or whose
 * f32 square is below the smallest normal f32 (radius < 1.1e-19), null pointers, ws_bytes < isr_radius_workspace_bytes(N).
 * The workspace needs no preparation and may be reused by the next call on the same stream. */
int isr_radius_count(const float* pts, int N, double radius, int cap, int32_t* counts, void* ws, size_t ws_bytes,
                     isr_stream_t stream);

/* The same count as host code over HOST pointers: the tests' reference. */
int isr_radius_count_host(const float* pts, int N, double radius, int cap, int32_t* counts);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RADIUS_H */
