/*
 * isr_adam.h — C ABI of the optimiser of libisr_hip.so: a fused multi-tensor Adam, one launch per step for every tensor of
 * every parameter group (trainPose.py:208-236, :450 and trainNerfFine.py:214, :354 call torch.optim.Adam).  The conventions
 * are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`, no
 * call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.  The device entry has a _host twin over HOST
 * pointers in the same library, the tests' reference: both are compiled from csrc/adam.hpp, which states the arithmetic once,
 * and the library is built with -ffp-contract=off, so host and device give the same bits.
 *
 * WHAT IS PINNED TO WHAT.  The arithmetic is OWNED: it is the definition below, restated in NumPy by tests/adam_ref.py, and
 * it is Adam as torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay added to the gradient) computes it, in an
 * order of this library's choosing.  torch's own bits are unpinned: its foreach, fused and single-tensor paths differ from
 * each other; the tests hold this definition within twice torch-f32's own distance from torch-f64.
 *
 * ---- THE ARITHMETIC.  A tensor whose step counter holds t - 1 takes its t-th step (t >= 1).  Its group gives lr, beta1,
 * beta2, eps, weight_decay and ramp.  Scalars, in f64:
 *   lr_t  = ramp > 0 ? lr * min(1, (t + 1) / ramp) : lr        (trainPose.py:229-236: frac = (iteration + 1) / 2000 with
 *                                                               iteration = t; the division is one f64 division)
 *   beta^t by binary powering over the bits of t, low bit first, on pairs (high, low) of f64 whose sum is the value:
 *           r = (1, 0), b = (beta, 0);  while t: { if t & 1: r = mul(r, b);  t >>= 1;  if t: b = mul(b, b) };  answer: r.high
 *           mul((ah, al), (ch, cl)):  p = ah * ch;  e = fma(ah, ch, -p);  e = fma(ah, cl, e);  e = fma(al, ch, e);
 *                                     h = p + e;  l = e - (h - p);  -> (h, l)
 *         a function of (beta, t) alone on which the host and the device agree (libm's pow is not).  Plain f64 products
 *         would do for that, but each squaring doubles the relative error: at t = 2000 they end 86 (beta = 0.999) to 417
 *         (beta = 0.9) ulp from pow; the pairs end within 1 ulp.
 *   bc1 = 1 - beta1^t,  bc2 = 1 - beta2^t,  step = lr_t / bc1,  r = sqrt(bc2)
 * Rounded once to f32 each: step, r, c1 = 1 - beta1, c2 = 1 - beta2 (the f64 differences), beta2, eps, weight_decay.
 * Per element, in f32 (fmaf: one rounding; every other operation rounds by itself):
 *   g' = weight_decay != 0 ? fmaf(weight_decay, p, g) : g
 *   m' = fmaf(c1, g' - m, m)
 *   v' = fmaf(c2, g' * g', beta2 * v)
 *   p' = fmaf(-step, m' / (sqrtf(v') / r + eps), p)
 * Non-finite gradients propagate as IEEE has them: no check, no skip, no host read.  With zero_grads, +0 is stored to g after
 * it has been read.
 *
 * ---- THE TABLE.  T descriptors (isr_adam_tensor): the four arrays of n f32 each, the group, and `slot`, the tensor's place
 * in the i64 array of step counters.  The arrays of one tensor must not overlap each other or another tensor's, and a slot
 * appears at most once.  The update is one launch of isr_adam_chunks(table) workgroups: a workgroup owns ISR_ADAM_CHUNK
 * consecutive elements of one tensor, which it finds by binary search of chunk_start (T + 1 running chunk counts,
 * chunk_start[i + 1] - chunk_start[i] = ceil(n_i / ISR_ADAM_CHUNK); isr_adam_table_host makes them).  Where p, g, m and v share
 * one misalignment from 16 bytes (all multiples of 4 bytes), lanes move 16 bytes, the up to 3 elements before the first
 * aligned one and after the last whole quad go one by one; otherwise every element goes one by one.  No workgroup waits for
 * another, there are no atomics and no workspace: every workgroup of a tensor reads the same counter, and a second launch, in
 * stream order, adds 1 to the counters of the tensors in the table.  The host never reads a counter.
 *
 * isr_adam_table_host checks a HOST copy of the table and writes chunk_start; the device entries take the table and
 * chunk_start on the DEVICE and trust them to be copies of what that call accepted (they cannot read them without a
 * synchronisation).  `groups_host` is a HOST array (G, 6) f64 of (lr, beta1, beta2, eps, weight_decay, ramp): it travels as
 * kernel arguments, so a learning rate changes without an upload.
 *
 * LIMITS.  1 <= G <= 8; 0 <= T (T = 0: nothing is done, ISR_OK); n >= 0 (a tensor of no elements is skipped, and its counter
 * still counts the step); 0 <= group < G; 0 <= slot < n_slots; the chunks of a table number at most 2^31 - 1; 0 <= beta < 1,
 * eps > 0, lr >= 0, weight_decay >= 0, ramp >= 0, all finite; non-null p, g, m, v (multiples of 4 bytes) where n > 0; f32
 * only.  Anything else is ISR_ERR_ARG with a message, and nothing is written.
 */
#ifndef ISR_ADAM_H
#define ISR_ADAM_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISR_ADAM_MAX_GROUPS 8
#define ISR_ADAM_CHUNK 4096      /* elements per workgroup */
#define ISR_ADAM_GROUP_DOUBLES 6 /* lr, beta1, beta2, eps, weight_decay, ramp */

typedef struct isr_adam_tensor {
  float* p;      /* parameter, updated in place */
  float* g;      /* gradient (written only with zero_grads) */
  float* m;      /* exp_avg */
  float* v;      /* exp_avg_sq */
  int64_t n;     /* elements */
  int32_t group; /* row of groups_host */
  int32_t slot;  /* index of its counter in steps */
} isr_adam_tensor; /* 48 bytes */

/* sizeof(isr_adam_tensor) and ISR_ADAM_CHUNK as the library was built, for bindings */
int isr_adam_geometry(int what); /* 0: descriptor bytes, 1: chunk elements, 2: threads per workgroup, 3: max groups */

/* Checks the table (HOST), and writes chunk_start_host (T + 1) i32 when it is not null.  Returns the number of chunks in
 * *chunks (nullable). */
int isr_adam_table_host(const isr_adam_tensor* table_host, int T, int G, int64_t n_slots, int32_t* chunk_start_host,
                        int64_t* chunks);

/* One step of every tensor in the table; then steps[slot] += 1 for each of them.  chunks: what isr_adam_table_host gave. */
int isr_adam_step(const isr_adam_tensor* table, const int32_t* chunk_start, int T, int64_t chunks, const double* groups_host,
                  int G, int64_t* steps, int zero_grads, isr_stream_t stream);

/* +0 to every gradient of the table, in one launch. */
int isr_adam_zero_grads(const isr_adam_tensor* table, const int32_t* chunk_start, int T, int64_t chunks, isr_stream_t stream);

/* The same step as host code over HOST pointers (table, arrays and steps); checks the table itself. */
int isr_adam_step_host(const isr_adam_tensor* table_host, int T, const double* groups_host, int G, int64_t* steps_host,
                       int64_t n_slots, int zero_grads);

/* The scalars of step t for one group (6 f64): out4 f64 = (lr_t, beta1^t, beta2^t, 0) and out2 f32 = (step, r). */
int isr_adam_scalars_host(const double* group_host, int64_t t, double* out4, float* out2);

#ifdef __cplusplus
}
#endif

#endif /* ISR_ADAM_H */
