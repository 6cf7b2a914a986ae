/*
 * isr_resample.h — C ABI of the fine pass's ray sampling of libisr_hip.so: a ray's coarse weights and depths in, its
 * importance-sampled depths out, on the device.  These entries are what pren.py:203-226 and pren2.py:204-217 get from
 * ProbabilisticRaysampler (pren.py:372-457) over pytorch3d's sample_pdf, the hierarchical pass of trainNerfFine.py:288-300.
 * The conventions are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued
 * on `stream`, no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.  Every device entry has a _host
 * twin over HOST pointers in the same library, the tests' reference: host and device use only + - * / in f32 and f64 (the
 * library is built with -ffp-contract=off) and give the same bits.  csrc/resample.hpp states the arithmetic once.
 *
 * WHAT IS PINNED TO WHAT.  ProbabilisticRaysampler.forward — the mid-points, the [1:-1] slice of the weights, the det rule,
 * the concatenation and the sort — is pinned to the reference's own executed code (tests/golden/ref_resample.npz).  The
 * deterministic units are isr_rays.h's linspace, pinned there to torch.linspace.  The rule of sample_pdf below is pytorch3d's
 * sample_pdf_python AS FAR AS IT IS KNOWN FROM MEMORY — pytorch3d is not available to compare against — and the f64 running
 * sums are torch's CPU sum / cumsum rule as far as it is known: those rules are UNPINNED.  They are held to a torch
 * restatement of the same rule in f32 and f64 (tests/resample_ref.py; profiles/resample_parity.json).  torch's random
 * stream is not reproduced.
 *
 * sample_pdf(bins (nb + 1), weights (nb), n, det, eps) of one ray, f32 unless said otherwise:
 *     w'_j = weights[j] + eps
 *     S = the sum of the w'_j, j ascending, in an f64 accumulator, rounded to f32 once
 *     pdf_j = w'_j / S
 *     cdf_0 = 0,  cdf_{j+1} = the f64 running sum of the pdf_j, j ascending, rounded to f32 per knot (the running sum itself
 *             stays f64); a correctly rounded running sum is monotone, so the knots never decrease
 *     u_s: det != 0: linspace(0, 1, n)[s] by isr_rays.h's linspace rule;  otherwise Philox4x32-10 with
 *             key = (seed & 0xffffffff, seed >> 32), counter = (ray_id, 0, 2, s / 4), word s % 4, u = (word >> 8) * 2^-24.
 *             ray_ids (N,) int32 or null for 0 .. N-1: a ray's samples are a function of (seed, ray_id, its row) only, not of
 *             the batch it rides in.
 *     i = the number of knots k in 0 .. nb with cdf_k <= u (searchsorted(right=True)), by the binary search
 *             lo = 0, hi = nb + 1;  while lo < hi: mid = (lo + hi) / 2;  cdf_mid <= u ? lo = mid + 1 : hi = mid;  i = lo
 *     below = max(i - 1, 0),  above = min(i, nb)
 *     den = cdf_above - cdf_below;  den < eps ? den = 1
 *     t = (u - cdf_below) / den
 *     z = bins_below + t * (bins_above - bins_below)      (two roundings, not fused)
 *
 * resample_lengths(lengths (P), ray_weights (P), n, add_input, ...) of one ray (pren.py:427-457):
 *     bins_j = 0.5f * (l_{j+1} + l_j), j = 0 .. P-2;  weights = ray_weights[1 .. P-2], so nb = P - 2
 *     the row is lengths followed by the n samples when add_input != 0, the samples alone otherwise:
 *     P_out = n + (add_input ? P : 0), sorted ascending by the sign-corrected integer image of the f32 bits: -0 before +0, NaN
 *     last.  The sorted row is unique as bits.
 *
 * NON-FINITE OR NEGATIVE INPUT is not refused: nothing synchronises.  A row's output depends on that row alone.  A NaN weight
 * gives a row whose n samples are all NaN (sorted last, after the lengths).  Every NaN written is 0x7FC00000.
 *
 * LIMITS.  3 <= P <= 1024 (isr_sample_pdf: 1 <= nb <= 1022), 1 <= n <= 1024, 0 <= N <= 2^28 (N = 0 enqueues nothing), eps > 0
 * and finite.  Anything else is ISR_ERR_ARG with a message.  One launch per call; no workspace.
 */
#ifndef ISR_RESAMPLE_H
#define ISR_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bins (N, nb + 1), weights (N, nb) -> samples (N, n), unsorted, in sample order. */
int isr_sample_pdf(const float* bins, const float* weights, int64_t N, int nb, int n, int det, float eps, uint64_t seed,
                   const int32_t* ray_ids, float* samples, isr_stream_t stream);

int isr_sample_pdf_host(const float* bins, const float* weights, int64_t N, int nb, int n, int det, float eps, uint64_t seed,
                        const int32_t* ray_ids, float* samples);

/* lengths (N, P), ray_weights (N, P) -> out (N, P_out), every row sorted.  Every byte of out is written. */
int isr_resample_lengths(const float* lengths, const float* ray_weights, int64_t N, int P, int n, int add_input, int det,
                         float eps, uint64_t seed, const int32_t* ray_ids, float* out, isr_stream_t stream);

int isr_resample_lengths_host(const float* lengths, const float* ray_weights, int64_t N, int P, int n, int add_input, int det,
                              float eps, uint64_t seed, const int32_t* ray_ids, float* out);

/* The rays one workgroup owns for this shape (sorted != 0: isr_resample_lengths with P lengths; 0: isr_sample_pdf with
 * P = nb + 1 knots); 0 (and isr_last_error()) for a refused shape.  The result of a call does not depend on it. */
int isr_resample_rays_per_group(int P, int n, int add_input, int sorted);

#ifdef __cplusplus
}
#endif

#endif /* ISR_RESAMPLE_H */
