/*
 * isr_density_dir.h — the ray march of isr_density.h with a direction: from the near end of the ray (the first hit, what
 * isr_density_march computes), from its far end (the last hit: the exit point of the surface, prenBack.py:378-381 as
 * generateCors.py:331-334 uses it), or both in one launch.  Conventions, the field and its pack are isr_density.h's;
 * isr_density.h's own entry list, isr_hip.h's and ISR_ABI_VERSION do not change.
 *
 * The march from the far end of one ray with P lengths and densities rho_k:
 *     c_k = rho_k > threshold ? 1 : 0 (a NaN gives 0) when threshold >= 0;  c_k = rho_k when threshold < 0
 *     A_{P-1} = 1,  A_k = A_{k+1} * (1 - c_{k+1}) for k descending, sequentially in f32;  w2_k = c_k * A_k
 *     depth = max_k(lengths_k * w2_k), for k ascending from the first product (a NaN product makes the depth NaN);
 *     point = origin + direction * depth;  hit = any(w2_k != 0).
 * In threshold mode w2 is one at the LAST density above the threshold and zero elsewhere.  The reference's
 * (1 + 1e-10) - c is 1 - c in f32.
 */
#ifndef ISR_DENSITY_DIR_H
#define ISR_DENSITY_DIR_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_MARCH_FRONT 0
#define ISR_MARCH_BACK 1
#define ISR_MARCH_BOTH 2

/* isr_density_march's arguments and `direction`.
 *   ISR_MARCH_FRONT: isr_density_march itself, the same bits.
 *   ISR_MARCH_BACK:  depth (N,), points (N, 3), hit (N,) and, where not null, weights (N, P) of the march from the far end.
 *   ISR_MARCH_BOTH:  depth (2, N), points (2, N, 3), hit (2, N): the front march's, then the back march's; weights (N, 2 P),
 *                    a ray's front weights and then its back weights (prenBack.py:385's cat).
 * densities (N, P) where not null, in every direction.  Every output is written for every ray. */
int isr_density_march_dir(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H, const float* origins,
                          const float* directions, const float* lengths, int N, int P, float threshold, int direction,
                          float* densities, float* weights, float* depth, float* points, int32_t* hit, isr_stream_t stream);

/* The same as host code over HOST pointers: the tests' reference. */
int isr_density_march_dir_host(const void* pack, size_t pack_bytes, int n_hidden, const int32_t* widths, int H,
                               const float* origins, const float* directions, const float* lengths, int N, int P, float threshold,
                               int direction, float* densities, float* weights, float* depth, float* points, int32_t* hit);

/* The march alone, of GIVEN densities rho (N, P), host code over HOST pointers: weights (nullable), depth and hit shaped as
 * above for `direction`.  For tests against recorded densities. */
int isr_density_march_given_host(const float* lengths, const float* rho, int N, int P, float threshold, int direction,
                                 float* weights, float* depth, int32_t* hit);

#ifdef __cplusplus
}
#endif

#endif /* ISR_DENSITY_DIR_H */
