// contrastive.hpp — the contrastive key loss of trainPose.py (nutil.returnCrossEntropy*, nutil.py:349-403) and its gradient:
// the cross-entropy of every query against its positive key and a set of negative keys, written once and compiled for host
// and device.  csrc/contrastive.hip holds the kernels and the C entries, include/isr_contrastive.h states every rule; a plain
// C++ compiler can include this header too (tools/contrastive_host_check.cpp, which defines __host__ and __device__ away).
// Only + - * / in f32 and f64, explicit fmaf, rintf and conversions, and everything is built with -ffp-contract=off: the
// host and the device build give the same bits.
//
// q (B, S, D), k (B, S, D), n (Bn, M, D), Bn == B or 1.  Row i = (b, s); its negatives are n[Bn == 1 ? 0 : b].
//
//   logit:   dot(a, c) = a_0 * c_0, then fmaf(a_d, c_d, .) for d = 1 .. D-1.  pos_i = dot(q_i, k_i), neg_ij = dot(q_i, n_j).
//   max:     m_i = pos_i, then for j ascending: neg_ij > m_i or neg_ij is NaN -> m_i = neg_ij (a NaN stays).
//   sums over j (SUM ORDER J): the terms of 64 consecutive columns j = 64 c .. 64 c + 63 are one f32 chain from 0 (the first
//            term is added to +0), and the chains are added in ascending c — to an f64 accumulator for t_i, which starts at
//            (double)exp32(pos_i - m_i), and to an f32 accumulator from 0 for each component of sum_j p_ij n_j.
//   t_i = (float)log1p64(T_i - 1.0), T_i the f64 accumulator (T_i >= 1: the maximum contributes exp32(0) = 1).
//   row_i = t_i - (pos_i - m_i);   ppos_i = exp32((pos_i - m_i) - t_i);   p_ij = exp32((neg_ij - m_i) - t_i).
//   loss = (float)(scale * (R / (double)(B S))), scale an f64, R the f64 sum of the row_i in REDUCE ORDER (ordered_sum.hpp).
//   c = (float)(((double)g * scale) / (double)(B S)),  a_i = ppos_i - 1
//   dq_id = c * fmaf(a_i, k_id, sum_j p_ij n_jd);   dk_id = (c * a_i) * q_id;   dn_jd = c * sum_i p_ij q_id
//   sums over i (SUM ORDER I), over the rows of batch item b (Bn == B, i = s) or over all rows (Bn == 1, i = b S + s): the terms
//            of 64 consecutive rows are one f32 chain from 0; 16 consecutive such chains (1024 rows) are added in ascending
//            order to an f32 accumulator from 0; those accumulators are added in ascending order to an f32 accumulator from 0.
//
// NON-FINITE INPUT is not refused (nothing synchronises).  A row with a NaN or +Inf logit, or whose logits are all -Inf, has
// m or T NaN: its m (if NaN), t, row, dq and dk are NaN, loss is NaN, and dn of every column that row meets is NaN.  A -Inf
// logit beside a finite maximum has p = 0.  Every NaN written is the canonical quiet NaN 0x7FC00000.
#pragma once
#include "field_density.hpp"
#include "ordered_sum.hpp"

#include "hd.hpp"

namespace isr {
namespace contrastive {

constexpr int kMaxD = 64;
constexpr long long kMaxRows = 1ll << 28;            // B S
constexpr int kMaxM = 1 << 24;
constexpr int kBlock = 64;                           // terms of one inner chain
constexpr int kSuper = 16;                           // inner chains of one middle accumulator (SUM ORDER I)
constexpr int kSuperRows = kBlock * kSuper;

// exp(x) in f32 for x <= 0 (every argument of the rule is): 0 below -87 (no subnormal results), NaN for NaN, exp32(0) = 1.
//   kf = rintf(x * log2(e));  r = fmaf(kf, -ln2_hi, x);  r = fmaf(kf, -ln2_lo, r)       (|r| <= 0.3466)
//   P = the degree-5 polynomial below by Horner in fmaf;  e = fmaf(r * r, P, r) + 1;  exp32 = e * 2^kf, exact (kf >= -126).
// Error against the correctly rounded exponential: tools/contrastive_host_check.cpp measures it over [-104, 0].
ISR_HD float exp32(float x) {
  if (!(x == x)) return bits_float(kNanBits);
  if (x < -87.0f) return 0.0f;
  const float kf = rintf(x * 1.44269504088896341f);
  float r = fmaf(kf, -0.693359375f, x);
  r = fmaf(kf, 2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  const float e = fmaf(r * r, p, r) + 1.0f;
  return e * bits_float((uint32_t)((int)kf + 127) << 23);
}

ISR_HD float dot(const float* a, const float* c, int D) {
  float l = a[0] * c[0];
  for (int d = 1; d < D; ++d) l = fmaf(a[d], c[d], l);
  return l;
}

ISR_HD float max_step(float m, float l) { return (l > m || l != l) ? l : m; }

ISR_HD float log_sum(double T) { return canonical((float)density::log1p64(T - 1.0)); }

ISR_HD float grad_scale(float g, double scale, long long rows) {
  return (float)(((double)g * scale) / (double)rows);
}

ISR_HD float loss_value(double R, double scale, long long rows) {
  return canonical((float)(scale * (R / (double)rows)));
}

// What is wrong with a shape, or null.
inline const char* check_shape(long long B, long long S, long long M, long long D, long long Bn) {
  if (D < 1 || D > kMaxD) return "D outside 1..64";
  if (B < 1 || S < 1) return "B and S must be at least 1";
  if (B > kMaxRows || S > kMaxRows || B * S > kMaxRows) return "B S above 2^28";
  if (M < 1 || M > kMaxM) return "M outside 1..2^24";
  if (Bn != 1 && Bn != B) return "Bn must be 1 or B";
  return nullptr;
}

// ---- host builds: the definitions the kernels are compared with
// One row's m, t, pos, row.  q, k: the row's D floats; n: its M negatives.
inline void forward_row(const float* q, const float* k, const float* n, int M, int D, float* m_out, float* t_out, float* pos_out,
                        float* row_out) {
  const float pos = dot(q, k, D);
  float m = pos;
  for (int j = 0; j < M; ++j) m = max_step(m, dot(q, n + (size_t)j * D, D));
  double T = (double)exp32(pos - m);
  for (int j0 = 0; j0 < M; j0 += kBlock) {
    float c = 0.f;
    for (int j = j0; j < M && j < j0 + kBlock; ++j) c += exp32(dot(q, n + (size_t)j * D, D) - m);
    T += (double)c;
  }
  const float t = log_sum(T);
  *m_out = canonical(m);
  *t_out = t;
  *pos_out = canonical(pos);
  *row_out = canonical(t - (pos - m));
}

// One row's dq and dk (either may be null) from its saved m and t.
inline void backward_row(const float* q, const float* k, const float* n, int M, int D, float m, float t, float c, float* dq,
                         float* dk) {
  const float pos = dot(q, k, D);
  const float a = exp32((pos - m) - t) - 1.0f;
  if (dk) {
    const float ca = c * a;
    for (int d = 0; d < D; ++d) dk[d] = canonical(ca * q[d]);
  }
  if (!dq) return;
  float outer[kMaxD], inner[kMaxD];
  for (int d = 0; d < D; ++d) outer[d] = 0.f;
  for (int j0 = 0; j0 < M; j0 += kBlock) {
    for (int d = 0; d < D; ++d) inner[d] = 0.f;
    for (int j = j0; j < M && j < j0 + kBlock; ++j) {
      const float* nj = n + (size_t)j * D;
      const float p = exp32((dot(q, nj, D) - m) - t);
      for (int d = 0; d < D; ++d) inner[d] = fmaf(p, nj[d], inner[d]);
    }
    for (int d = 0; d < D; ++d) outer[d] += inner[d];
  }
  for (int d = 0; d < D; ++d) dq[d] = canonical(c * fmaf(a, k[d], outer[d]));
}

// One column's dn over `rows` rows q (rows, D) with their m and t.
inline void backward_column(const float* q, const float* m, const float* t, long long rows, const float* nj, int D, float c,
                            float* dn) {
  float outer[kMaxD], mid[kMaxD], inner[kMaxD];
  for (int d = 0; d < D; ++d) outer[d] = 0.f;
  for (long long s0 = 0; s0 < rows; s0 += kSuperRows) {
    for (int d = 0; d < D; ++d) mid[d] = 0.f;
    for (long long i0 = s0; i0 < rows && i0 < s0 + kSuperRows; i0 += kBlock) {
      for (int d = 0; d < D; ++d) inner[d] = 0.f;
      for (long long i = i0; i < rows && i < i0 + kBlock; ++i) {
        const float* qi = q + (size_t)i * D;
        const float p = exp32((dot(qi, nj, D) - m[i]) - t[i]);
        for (int d = 0; d < D; ++d) inner[d] = fmaf(p, qi[d], inner[d]);
      }
      for (int d = 0; d < D; ++d) mid[d] += inner[d];
    }
    for (int d = 0; d < D; ++d) outer[d] += mid[d];
  }
  for (int d = 0; d < D; ++d) dn[d] = canonical(c * outer[d]);
}

}  // namespace contrastive
}  // namespace isr
