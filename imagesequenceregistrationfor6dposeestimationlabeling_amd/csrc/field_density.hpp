// field_density.hpp — the arithmetic of the density field (nerf.py:106-144, :163-177, :206-228, :417-432: HarmonicEmbedding,
// Linear + Softplus(beta) layers, one output neuron, 1 - exp(-x)) and of the ray march on top of it (pren.py:338-365), defined
// once and compiled for host and device.  csrc/field_density.hip holds the kernels and the C entries (include/isr_density.h).
//
// One point x (3 f32), frequencies f[0..H), H in 1..64:
//     a[d*H + i] = x[d] * f[i]                      (one f32 multiply)
//     e = [sin(a[0]) .. sin(a[3H-1]), cos(a[0]) .. cos(a[3H-1])]         (sincos32 below; 6H wide, nerf.py:143-144's order)
//     hidden layer:  z_j = b_j;  z_j = fmaf(W[j,k], h[k], z_j) for k ascending;  h'_j = softplus32(z_j, beta)
//     output:        z = b;  z = fmaf(w[k], h[k], z) for k ascending;  density = density32(softplus32(z, beta))
// 1..4 hidden layers, widths 1..256.  A point's value is a function of the point and the weights only.  Everything is built
// with -ffp-contract=off and uses + - * /, rint, conversions and integer operations alone, so the host build and the device
// build of this header give the same bits.  (Widths are padded with zero weights: fmaf(0, h, z) = z except that a z of -0
// becomes +0, which softplus32 does not tell apart; the output neuron is not padded.  A NaN result is a NaN on both builds; its sign and
// payload are the hardware's.)
//
// Measured against f64 (numpy / mpmath, tests/test_density_cpu.py):
//     sincos32    0.5001 ulp of the f64 sine / cosine of the same f32 argument, over every finite f32 range tested
//     softplus32  0.5001 ulp of log1p(exp(beta z)) / beta evaluated in f64 (z where beta z > 20)
//     density32   0.5001 ulp of -expm1(-s)
// — each is an f64 result with an error near 1e-16, rounded once to f32.  The tests hold all three to 1 ulp.
//
// The PACK: 128 header words ([0] beta, [1] H, [2] n_hidden, [64 + i] f[i]), then per hidden layer the weights in
// field_mlp.hpp's matrix-core order (w_index, every layer, kstride = in rounded up to 8) and the bias, zero padded to 32 rows;
// then the output neuron's weights (row-major, padded to 4) and its bias (4 words).
#pragma once
#include <vector>

#include "ea_chain.hpp"
#include "field_mlp.hpp"

namespace isr {
namespace density {

using field::Layer;
using field::w_index;

constexpr int kMaxHidden = 4;
constexpr int kMaxWidth = 256;
constexpr int kMaxH = 64;
constexpr int kHeaderWords = 128;
constexpr int kFreqOff = 64;
constexpr int kMaxP = 4096;        // points per ray of the march

struct Layout {
  int n_hidden, H;
  int total_words;
  int out_K, out_w_off, out_b_off;
  Layer L[kMaxHidden];
};

ISR_HD bool make_layout(int n_hidden, const int32_t* widths, int H, Layout& lay) {
  if (n_hidden < 1 || n_hidden > kMaxHidden || H < 1 || H > kMaxH) return false;
  int off = kHeaderWords;
  int K = 6 * H;
  for (int l = 0; l < n_hidden; ++l) {
    const int O = widths[l];
    if (O < 1 || O > kMaxWidth) return false;
    field::add_layer(K, O, 1, off, lay.L[l]);
    K = O;
  }
  lay.n_hidden = n_hidden;
  lay.H = H;
  lay.out_K = K;
  lay.out_w_off = off;
  off += (K + 3) / 4 * 4;
  lay.out_b_off = off;
  off += 4;
  lay.total_words = off;
  return true;
}

ISR_HD double from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}
ISR_HD uint64_t to_bits(double d) {
  uint64_t u;
  __builtin_memcpy(&u, &d, 8);
  return u;
}
ISR_HD uint32_t to_bits32(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// The first 320 bits of the binary fraction of 2/pi, most significant word first, behind one word of zeros (bit positions
// <= 0).  Produced with mpmath at 600 bits of working precision:
//     v = int(mpmath.floor(mpmath.mpf(2) / mpmath.pi * mpmath.mpf(2) ** 320));  word i = (v >> (32 * (9 - i))) & 0xffffffff
ISR_HD uint32_t two_over_pi_word(int i) {
  constexpr uint32_t kBits[11] = {0x00000000u, 0xa2f9836eu, 0x4e441529u, 0xfc2757d1u, 0xf534ddc0u, 0xdb629599u,
                                  0x3c439041u, 0xfe5163abu, 0xdebbc561u, 0xb7246e3au, 0x424dd2e0u};
  return kBits[i];
}

// sin(a) and cos(a) of an f32 a, each an f64 result (error ~1e-16) rounded once: within 1 ulp of the true values for EVERY
// finite a (measured 0.5001).  |a| < 2^17: sin32's reduction (field::reduce_pio2), the same bits as sin32 for the sine.
// Otherwise Payne-Hanek: |a| = m 2^e with m the 24-bit mantissa as an integer; the bits of 2/pi whose weight times 2^e is 4
// or more contribute whole turns and are skipped, m times the next 128 bits (integer arithmetic, 32-bit limbs) gives
// a 2/pi mod 4 as 2 integer and 126 fraction bits, of which 96 fraction bits are kept: the quadrant n and a fraction in
// [-1/2, 1/2) with at least 60 significant bits even where a is nearest a multiple of pi/2; r = fraction * pi/2, then
// field::sincos_kernel on |r| <= pi/4.  The table reaches past the largest finite f32 (e = 104 needs bit 262), so the rule
// beyond 2^64 is the same rule and the same accuracy.  NaN and +-Inf give NaN for both; sin(-0) = -0, cos(-0) = 1.
ISR_HD void sincos32(float a, float* sn, float* cs) {
  const uint32_t ab = to_bits32(a);
  const uint32_t ax = ab & 0x7fffffffu;
  if (ax >= 0x7f800000u) {
    *sn = a - a;
    *cs = a - a;
    return;
  }
  double r, s, c;
  int q;
  bool neg = false;
  if (ax < 0x48000000u) {            // |a| < 2^17
    double n;
    r = field::reduce_pio2((double)a, &n);
    q = (int)n & 3;
  } else {
    neg = (ab >> 31) != 0;
    const uint32_t m = (ax & 0x007fffffu) | 0x00800000u;
    const int e = (int)(ax >> 23) - 150;            // |a| = m * 2^e, -6 <= e <= 104
    const int p0 = e + 30;                          // first bit of the window in the padded table: its weight times 2^e is 2
    const int j = p0 >> 5, sh = p0 & 31;
    uint32_t w[4];
    for (int i = 0; i < 4; ++i) {
      const uint32_t hi = two_over_pi_word(j + i), lo = two_over_pi_word(j + i + 1);
      w[i] = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
    }
    const uint64_t p3 = (uint64_t)m * w[3];
    const uint64_t p2 = (uint64_t)m * w[2] + (p3 >> 32);
    const uint64_t p1 = (uint64_t)m * w[1] + (p2 >> 32);
    const uint64_t pp = (uint64_t)m * w[0] + (p1 >> 32);
    const uint32_t q0 = (uint32_t)pp, q1 = (uint32_t)p1, q2 = (uint32_t)p2, q3 = (uint32_t)p3;
    // the product mod 2^128 is q0:q1:q2:q3 = (a 2/pi mod 4) * 2^126
    const uint64_t f64hi = ((((uint64_t)q0 << 32) | q1) << 2) | (q2 >> 30);       // fraction bits 1..64
    const uint32_t f32lo = (q2 << 2) | (q3 >> 30);                                 // fraction bits 65..96
    q = (int)(q0 >> 30) + (int)(f64hi >> 63);       // a fraction of 1/2 or more belongs to the next quadrant
    const double frac = (double)(int64_t)f64hi * 5.42101086242752217004e-20 +      // 2^-64
                        (double)f32lo * 1.26217744835361888865e-29;                // 2^-96
    r = frac * 1.57079632679489655800e+00;
    q &= 3;
  }
  field::sincos_kernel(r, &s, &c);
  double vs = (q == 0) ? s : (q == 1) ? c : (q == 3) ? -c : -s;
  const double vc = (q == 0) ? c : (q == 1) ? -s : (q == 3) ? s : -c;
  if (neg) vs = -vs;
  *sn = (float)vs;
  *cs = (float)vc;
}

// expm1(r) for |r| <= 0.35: fdlibm's e_exp.c kernel, exp(r) = 1 + r + r c / (2 - c), c = r - r^2 P(r^2)
ISR_HD double expm1_kernel(double r) {
  const double t = r * r;
  const double c = r - t * (1.66666666666666019037e-01 +
                            t * (-2.77777777770155933842e-03 +
                                 t * (6.61375632143793436117e-05 +
                                      t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
  return r - (r * c) / (c - 2.0);
}

// x = k ln2 + r, |r| <= ln2 / 2 (fdlibm's two-part ln2); x finite, |x| < 746
ISR_HD double reduce_ln2(double x, int* k) {
  const double kf = rint(x * 1.44269504088896338700e+00);
  *k = (int)kf;
  return (x - kf * 6.93147180369123816490e-01) - kf * 1.90821492927058770002e-10;
}

// exp(x) in f64, error below 1 ulp; 0 below -708 (no subnormal results), +Inf above 709, NaN for NaN
ISR_HD double exp64(double x) {
  if (!(x == x)) return x;
  if (x < -708.0) return 0.0;
  if (x > 709.0) return from_bits(0x7ff0000000000000ull);
  int k;
  const double r = reduce_ln2(x, &k);
  return from_bits((uint64_t)(k + 1023) << 52) * (1.0 + expm1_kernel(r));
}

// log(1 + y) in f64 for y >= 0 (NaN for NaN): fdlibm's s_log1p.c — u = 1 + y, the rounding of u put back as c / u, and
// e_log.c's kernel on u = 2^k m with m in [sqrt(1/2), sqrt(2))
ISR_HD double log1p64(double y) {
  if (!(y == y)) return y;
  const double u = 1.0 + y;
  double c = (u >= 2.0) ? 1.0 - (u - y) : y - (u - 1.0);
  c = c / u;
  const uint64_t ub = to_bits(u);
  int k = (int)(ub >> 52) - 1023;
  const uint64_t mant = ub & 0x000fffffffffffffull;
  double m;
  if (mant >= 0x0006a09e667f3bcdull) {
    k += 1;
    m = from_bits(mant | 0x3fe0000000000000ull);
  } else {
    m = from_bits(mant | 0x3ff0000000000000ull);
  }
  const double f = m - 1.0;
  const double hfsq = 0.5 * f * f;
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 +
                         w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1;
  const double dk = (double)k;
  return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + (dk * 1.90821492927058770002e-10 + c))) - f);
}

// torch.nn.Softplus(beta): z where beta z > 20, else log1p(exp(beta z)) / beta.  beta z is the exact f64 product of the two
// f32 values, the result one rounding of an f64 value.
ISR_HD float softplus32(float z, float beta) {
  const double t = (double)beta * (double)z;
  if (t > 20.0) return z;
  return (float)(log1p64(exp64(t)) / (double)beta);
}

// 1 - exp(-s) as -expm1(-s): no cancellation for small s.  s >= 0 in the field; NaN gives NaN.
ISR_HD float density32(float s) {
  const double x = -(double)s;
  if (!(x == x)) return s;
  if (x < -40.0) return 1.0f;
  if (x > 700.0) return -from_bits(0x7ff0000000000000ull);
  int k;
  const double r = reduce_ln2(x, &k);
  const double p = expm1_kernel(r);
  if (k == 0) return (float)(-p);
  const double tk = from_bits((uint64_t)(k + 1023) << 52);
  return (float)(-(tk * p + (tk - 1.0)));
}

// The march of one ray: ea_chain.hpp's chain, threshold >= 0 (thresholdMode) or the emission-absorption weights.
// Only rho[0 .. n_eval) counts: in threshold mode a caller may stop evaluating a ray after its first hit, the later c_k
// are multiplied by 0 whatever they are.  weights may be null.
ISR_HD void march_ray(int P, const float* len, const float* rho, int n_eval, float threshold, float* weights, float* depth,
                            int32_t* hit) {
  ea::WeightChain ch;
  ch.start();
  for (int k = 0; k < P; ++k) {
    const float w = ch.step(k, len[k], ea::absorbance(rho[k], threshold, k < n_eval));
    if (weights) weights[k] = w;
  }
  *depth = ch.m;
  *hit = ch.any;
}

// The march of the same ray taken from its far end (prenBack.py:378-381: weights2 = rho * flip(shifted_cumprod(1 - flip(rho)))).
//   A_{P-1} = 1, A_k = A_{k+1} * (1 - c_{k+1}) for k descending; c_k as in march_ray (ea::absorbance); w2_k = c_k * A_k: in
//   threshold mode one-hot at the LAST hit, the exit point.
//   depth = max_k(len_k * w2_k), taken for k ascending from the first product with march_ray's NaN rule; hit = any(w2_k != 0).
// Only rho[lo_eval .. P) is read: in threshold mode a caller may leave the samples in front of the tile holding the last hit
// unevaluated, their c_k is multiplied by A_k = 0 whatever it is.  rho[lo_eval .. P) is OVERWRITTEN with the weights (the
// descending pass leaves them there for the ascending maximum); weights may be null.
ISR_HD void march_ray_back(int P, const float* len, float* rho, int lo_eval, float threshold, float* weights, float* depth,
                                 int32_t* hit) {
  float absorb = 1.0f;
  for (int k = P - 1; k >= lo_eval; --k) {
    const float c = ea::absorbance(rho[k], threshold);
    rho[k] = c * absorb;
    absorb = absorb * (1.0f - c);
  }
  ea::WeightChain ch;
  ch.start();
  for (int k = 0; k < P; ++k) {
    const float w = k >= lo_eval ? rho[k] : 0.0f;      // in front of lo_eval: c_k * A_k with A_k = 0 and c_k 0 or 1
    if (weights) weights[k] = w;
    ch.take(k, len[k], w);
  }
  *depth = ch.m;
  *hit = ch.any;
}

// Host: W (row-major, hidden layers then the output row), b -> pack (lay.total_words words)
inline void pack_host(const Layout& lay, const float* freqs, float beta, const float* W, const float* b, void* pack) {
  float* pf = static_cast<float*>(pack);
  uint32_t* pu = static_cast<uint32_t*>(pack);
  for (int i = 0; i < lay.total_words; ++i) pu[i] = 0u;
  pf[0] = beta;
  pu[1] = (uint32_t)lay.H;
  pu[2] = (uint32_t)lay.n_hidden;
  for (int i = 0; i < lay.H; ++i) pf[kFreqOff + i] = freqs[i];
  for (int l = 0; l < lay.n_hidden; ++l) {
    const Layer& L = lay.L[l];
    field::pack_layer(L, W, b, pf);
    W += (size_t)L.O * L.K;
    b += L.O;
  }
  for (int k = 0; k < lay.out_K; ++k) pf[lay.out_w_off + k] = W[k];
  pf[lay.out_b_off] = b[0];
}

// e (6H) of one point
ISR_HD void embed_point(const float* x, const float* freqs, int H, float* e) {
  for (int d = 0; d < 3; ++d)
    for (int i = 0; i < H; ++i) {
      const float a = x[d] * freqs[i];
      sincos32(a, &e[d * H + i], &e[3 * H + d * H + i]);
    }
}

// Host: the hidden layers' weights transposed (Wt[l][k * O + j]), so that the chain of every neuron advances together
struct HostWeights {
  const float* Wt[kMaxHidden];
};

// one point through the trunk: the embedding, the hidden layers, the output neuron -> the last hidden activations (in z or
// g, lay.out_K of them) and *dens.  The k loop is outermost and ascending, each z_j sees its own k-ordered fmaf chain.
// Inlined into its callers, so that each compiles the loops for its own instruction set.
__attribute__((always_inline)) inline const float* trunk_body(const Layout& lay, const void* pack, const HostWeights& hw,
                                                              const float* x, float* z, float* g, float* dens) {
  float e[6 * kMaxH];
  const float* pf = static_cast<const float*>(pack);
  const float beta = pf[0];
  embed_point(x, pf + kFreqOff, lay.H, e);
  const float* h = e;
  for (int l = 0; l < lay.n_hidden; ++l) {              // n_hidden >= 1: e does not outlive the call
    const Layer& L = lay.L[l];
    const float* wt = hw.Wt[l];
    for (int j = 0; j < L.O; ++j) z[j] = pf[L.b_off + j];
    for (int k = 0; k < L.K; ++k) {
      const float hk = h[k];
      const float* wk = wt + (size_t)k * L.O;
      for (int j = 0; j < L.O; ++j) z[j] = __builtin_fmaf(wk[j], hk, z[j]);
    }
    for (int j = 0; j < L.O; ++j) g[j] = softplus32(z[j], beta);      // every z is complete: h may be g
    h = g;
  }
  float zo = pf[lay.out_b_off];
  for (int k = 0; k < lay.out_K; ++k) zo = __builtin_fmaf(pf[lay.out_w_off + k], h[k], zo);
  *dens = density32(softplus32(zo, beta));
  return h;
}

__attribute__((always_inline)) inline float point_density_body(const Layout& lay, const void* pack, const HostWeights& hw,
                                                               const float* x) {
  float z[kMaxWidth], g[kMaxWidth], dens;
  trunk_body(lay, pack, hw, x, z, g, &dens);
  return dens;
}

inline float point_density_host(const Layout& lay, const void* pack, const HostWeights& hw, const float* x) {
  return point_density_body(lay, pack, hw, x);
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
// the same function compiled for CPUs with a fused multiply-add instruction (fmaf is correctly rounded either way: the
// bits do not depend on which of the two runs); callers ask __builtin_cpu_supports("fma") first
__attribute__((target("avx2,fma"))) inline float point_density_host_fma(const Layout& lay, const void* pack,
                                                                        const HostWeights& hw, const float* x) {
  return point_density_body(lay, pack, hw, x);
}
#define ISR_DENSITY_HAVE_FMA_BUILD 1
#endif

// Host: a pack's hidden layers unpacked and transposed, and whether this CPU runs the _fma builds
struct HostField {
  std::vector<std::vector<float>> wt;
  HostWeights hw;
  bool fma;
  HostField(const Layout& lay, const void* pack) {
    wt.resize(lay.n_hidden);
    for (int l = 0; l < lay.n_hidden; ++l) {
      wt[l].resize((size_t)lay.L[l].O * lay.L[l].K);
      field::unpack_layer(lay.L[l], static_cast<const float*>(pack), wt[l].data(), true);
      hw.Wt[l] = wt[l].data();
    }
#ifdef ISR_DENSITY_HAVE_FMA_BUILD
    fma = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
#else
    fma = false;
#endif
  }
};

}  // namespace density
}  // namespace isr
