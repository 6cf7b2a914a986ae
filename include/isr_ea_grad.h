/*
 * isr_ea_grad.h — C ABI of the backward of isr_ea_march (isr_radiance.h) in libisr_hip.so: the gradient of the
 * emission-absorption march of pren.py:338-369 with respect to its densities and features, which is what lets
 * trainNerfFine.py's losses (trainNerfFine.py:324-336, :353) train the fields behind the renderer.  The conventions are those
 * of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no call
 * synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.
 *
 * The rule (csrc/ea_grad.hpp is the one place it is written).  All f32: rho (N, P), features (N, P, F), threshold,
 * dimage (N, F + 1) laid out as [features | opacity], dweights (N, P) or null for zeros -> ddensities (N, P) and
 * dfeatures (N, P, F); either output may be null (not wanted), not both.  Per ray:
 *   c_k = rho_k (threshold < 0), or 1 where rho_k > threshold and 0 elsewhere (threshold >= 0)
 *   T_0 = 1,  w_k = c_k * T_k,  T_{k+1} = T_k * (1 - c_k)         the forward's chain: w_k are isr_ea_march's weights, bit for bit
 *   dfeatures[k, ch] = w_k * dimage[ch]
 *   threshold >= 0:  ddensities[k] = +0 (c_k is a step function of rho_k)
 *   threshold <  0:  g_k = dweights[k] (or +0), then g_k = fmaf(dimage[ch], features[k, ch], g_k) for ch ascending;
 *                    a_P = -dimage[F] (the opacity is 1 - T_P); for k = P-1 .. 0:
 *                        ddensities[k] = T_k * (g_k - a_{k+1})
 *                        a_k = fmaf(g_k, c_k, a_{k+1} * (1 - c_k))
 * No division: a density of exactly 1 is an ordinary input.  NaN and infinities follow IEEE through these expressions, and
 * a ray's outputs depend on that ray's inputs only.  The result is a function of the arguments only — not of the launch or
 * of a previous call — with no float atomics, and the same bits from isr_ea_march_backward and isr_ea_march_backward_host.
 *
 * Limits: isr_ea_march's, 1 <= P <= 4096 and 1 <= F <= 64.
 */
#ifndef ISR_EA_GRAD_H
#define ISR_EA_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEVICE pointers.  Every element of each non-null output is written by every successful call, whatever the buffer held.
 * N = 0 is a valid call that launches nothing, whatever the pointers are.  Refused: N < 0, P or F out of range, a NaN
 * threshold, and with N > 0 null densities, features or dimage, or both outputs null. */
int isr_ea_march_backward(const float* densities, const float* features, int N, int P, int F, float threshold,
                          const float* dimage, const float* dweights, float* ddensities, float* dfeatures, isr_stream_t stream);

/* The same gradient as host code over HOST pointers: the tests' reference. */
int isr_ea_march_backward_host(const float* densities, const float* features, int N, int P, int F, float threshold,
                               const float* dimage, const float* dweights, float* ddensities, float* dfeatures);

/* The constants the tests need: which = 0 the threads of a workgroup, 1 the most rays one workgroup owns, 2 the floats of
 * LDS per array that bound (rays of a workgroup) * (P | 1); -1 otherwise. */
int isr_ea_grad_geometry(int which);

/* The rays one workgroup of isr_ea_march_backward owns at P samples per ray; -1 for P out of range. */
int isr_ea_grad_rays_per_group(int P);

#ifdef __cplusplus
}
#endif

#endif /* ISR_EA_GRAD_H */
