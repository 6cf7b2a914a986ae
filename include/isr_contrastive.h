/*
 * isr_contrastive.h — C ABI of the contrastive key loss of libisr_hip.so and of its gradient: what trainPose.py:417-423 gets
 * from nutil.returnCrossEntropyWithNeg (and its siblings returnCrossEntropy, returnCrossEntropy2; nutil.py:349-403), the
 * cross-entropy of every query against its positive key and a set of negative keys, fused: the (B, 1 + M, S) logits are
 * recomputed tile by tile and never stored, so a call needs O(B S) memory beside its inputs and gradients.  The conventions
 * are those of isr_hip.h (return value ISR_OK or a negative ISR_ERR_*, text in isr_last_error(), work enqueued on `stream`,
 * no call synchronises); isr_hip.h's entry list and ISR_ABI_VERSION do not change.  These are the library's first entries
 * with a gradient.  Every device entry has a _host twin over HOST pointers in the same library, the tests' reference: host
 * and device use only + - * / fmaf rintf and conversions in f32 and f64 (the library is built with -ffp-contract=off) and give
 * the same bits.  csrc/contrastive.hpp states the arithmetic once.  There are no float atomics.
 *
 * INPUTS, contiguous f32: q (B, S, D) the queries, k (B, S, D) the positive key of each query, n (Bn, M, D) the negative
 * keys, Bn == B (item b's rows meet n[b]) or Bn == 1 (every row meets n[0]; an extension: the reference needs Bn == B).
 * Row i = b S + s.  scale: an f64, the reference's 1 / 1000 (an f32 0.001 is 4.7e-8 off: most of an f32 ulp of the loss).
 *
 * THE RULE, f32 unless said otherwise:
 *     dot(a, c) = a_0 c_0, then fmaf(a_d, c_d, .) for d = 1 .. D-1;    pos_i = dot(q_i, k_i),  neg_ij = dot(q_i, n_j)
 *     m_i = pos_i, then for j ascending: if neg_ij > m_i or neg_ij is NaN, m_i = neg_ij
 *     T_i (f64) = (double)exp32(pos_i - m_i) + the sum over j of exp32(neg_ij - m_i) in SUM ORDER J
 *     t_i = (float)log(T_i), the logarithm in f64 (field_density.hpp's log1p64 of T_i - 1; T_i >= 1)
 *     row_i = t_i - (pos_i - m_i)
 *     ppos_i = exp32((pos_i - m_i) - t_i),  p_ij = exp32((neg_ij - m_i) - t_i)
 * — torch's shifted log-softmax, not a merged log-sum-exp: subtracting m + t from a logit of magnitude 90 would lose the low
 * bits of t.  The backward recomputes pos and neg by the same chain and so gets the same bits.
 *     loss = (float)(scale * (R / (double)(B S))),  R the f64 sum of the row_i in REDUCE ORDER
 *     c = (float)(((double)g * scale) / (double)(B S)),  a_i = ppos_i - 1
 *     dq_id = c * fmaf(a_i, k_id, sum over j of p_ij n_jd in SUM ORDER J)
 *     dk_id = (c * a_i) * q_id
 *     dn_jd = c * (sum over i of p_ij q_id in SUM ORDER I), i over the rows of item b (Bn == B) or over all B S rows (Bn == 1)
 *
 * SUM ORDER J.  The terms of the 64 consecutive columns 64 c .. 64 c + 63 are one f32 chain from +0 (for a vector, fmaf(p, n_d,
 * chain_d)); the chains are added in ascending c — for T_i to the f64 accumulator, for dq to an f32 accumulator from +0.
 * SUM ORDER I.  The terms of 64 consecutive rows are one f32 chain from +0; 16 consecutive chains (1024 rows) are added in
 * ascending order to an f32 accumulator from +0; those are added in ascending order to an f32 accumulator from +0.  Rows are
 * counted from the first row the column meets.
 * REDUCE ORDER.  256 consecutive values (missing ones are +0) are summed by the tree v[i] += v[i + s], s = 128, 64 .. 1, in
 * f64; the results are summed the same way, until one is left.
 * One chain over all M columns would reach 6 x torch-f32's own deviation from f64 at M = 4097; the blocked orders stay near 1 x.
 *
 * exp32(x), x <= 0 (every argument above is): 0 for x < -87 (no subnormal results), NaN for NaN, exp32(0) = 1, otherwise
 * kf = rintf(x log2 e), r = x - kf ln2 in two fmaf (ln2 = 0.693359375 - 2.12194440e-4), a degree-5 polynomial in fmaf, and
 * an exact scaling by 2^kf.  Its measured error is in profiles/contrastive_host_sanitizers.txt.
 *
 * INDEPENDENCE.  A row's m, t, pos, row, dq, dk depend on that row and its negatives only; a column's dn on that column and
 * the rows it meets only.  Nothing depends on the launch geometry, the batch size, or a neighbour.
 * NON-FINITE INPUT is not refused: nothing synchronises.  A row with a NaN or +Inf logit, or whose logits are all -Inf, has a
 * NaN t, row, dq and dk (and m, if a logit is NaN); loss is then NaN, and so is dn of every column the row meets.  A -Inf logit
 * beside a finite maximum has p = 0 (and then 0 x Inf = NaN in that row's dq, as in torch).  Every NaN written is 0x7FC00000.
 *
 * LIMITS.  1 <= D <= 64, S >= 1, M >= 1, B >= 1, B S <= 2^28, M <= 2^24, Bn in {1, B}.  Anything else is ISR_ERR_ARG with a
 * message, and nothing on the device is touched.
 */
#ifndef ISR_CONTRASTIVE_H
#define ISR_CONTRASTIVE_H

#include <stddef.h>
#include <stdint.h>

#include "isr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace either call needs for this shape; 0 (and isr_last_error()) for a refused shape */
size_t isr_contrastive_workspace_bytes(int64_t B, int64_t S, int64_t M, int D, int64_t Bn);

/* m, t, pos, rows: (B S) f32; loss: 1 f32; all on the device, every byte of each written.  Two or more launches. */
int isr_contrastive_forward(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D, int64_t Bn,
                            double scale, float* m, float* t, float* pos, float* rows, float* loss, void* ws, size_t ws_bytes,
                            isr_stream_t stream);

/* m, t: what the forward wrote.  g_dev_or_null: a DEVICE pointer to the upstream gradient (1 f32), null for 1.  dq (B, S, D),
 * dk (B, S, D), dn (Bn, M, D): any may be null; those given are written whole.  dq and dk: one launch; dn: one, or two. */
int isr_contrastive_backward(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D, int64_t Bn,
                             double scale, const float* m, const float* t, const float* g_dev_or_null, float* dq, float* dk,
                             float* dn, void* ws, size_t ws_bytes, isr_stream_t stream);

int isr_contrastive_forward_host(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D,
                                 int64_t Bn, double scale, float* m, float* t, float* pos, float* rows, float* loss);

/* g_or_null: a HOST pointer */
int isr_contrastive_backward_host(const float* q, const float* k, const float* n, int64_t B, int64_t S, int64_t M, int D,
                                  int64_t Bn, double scale, const float* m, const float* t, const float* g_or_null, float* dq,
                                  float* dk, float* dn);

/* The kernels' widths (tests cover their boundaries; no result depends on them).  what 0: rows (columns) of a workgroup,
 * 1: vectors of an LDS tile, 2: rows of a range of the split column pass, 3: leaves of a reduction tree; 0 otherwise. */
int isr_contrastive_geometry(int what);

/* The 1024-row ranges the column pass (dn) is split into for this shape: 1 = not split; 0 for a refused shape. */
int64_t isr_contrastive_column_splits(int64_t B, int64_t S, int64_t M, int D, int64_t Bn);

#ifdef __cplusplus
}
#endif

#endif /* ISR_CONTRASTIVE_H */
