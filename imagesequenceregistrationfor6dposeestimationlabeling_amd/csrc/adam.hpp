// adam.hpp — the fused multi-tensor Adam: the arithmetic of include/isr_adam.h (which states every rule), written once and
// compiled for host and device.  csrc/adam.hip holds the kernels and the C entries; a plain C++ compiler can include this
// header too (tools/adam_host_check.cpp).  f64 scalars per (group, t), f32 elements with explicit fmaf, and everything is
// built with -ffp-contract=off: host and device give the same bits.
//
// What this replaces: torch.optim.Adam's step and zero_grad in trainPose.py:208-236, :246, :450 and trainNerfFine.py:214,
// :238, :354, with trainPose.py:229-236's learning-rate ramp moved into the step.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/isr_adam.h"

#include "hd.hpp"

namespace isr {
namespace adam {

constexpr int kMaxGroups = ISR_ADAM_MAX_GROUPS;
constexpr int kChunk = ISR_ADAM_CHUNK;
constexpr int kThreads = 256;                          // a workgroup: kChunk / kThreads = 16 elements a lane, 4 quads
constexpr long long kMaxChunks = 2147483647ll;

static_assert(sizeof(isr_adam_tensor) == 48, "isr_adam_tensor is 48 bytes in every binding");
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of quads per lane");

// what does not depend on t, made on the host: the kernel's arguments
struct Group {
  double lr, beta1, beta2, ramp;
  float c1, c2, beta2f, eps, wd;      // 1 - beta1, 1 - beta2, beta2, eps, weight_decay: one rounding each
  int pad;
};

struct Groups {
  Group g[kMaxGroups];
};

// what depends on t: one rounding to f32 each
struct Scalars {
  float step, r;
};

// null, or what is wrong with the group's six numbers
inline const char* make_group(const double* six, Group& out) {
  const double lr = six[0], b1 = six[1], b2 = six[2], eps = six[3], wd = six[4], ramp = six[5];
  if (!(lr >= 0.0) || !std::isfinite(lr)) return "lr must be finite and >= 0";
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return "betas must lie in [0, 1)";
  if (!(eps > 0.0) || !std::isfinite(eps)) return "eps must be finite and > 0";
  if (!(wd >= 0.0) || !std::isfinite(wd)) return "weight_decay must be finite and >= 0";
  if (!(ramp >= 0.0) || !std::isfinite(ramp)) return "ramp must be finite and >= 0";
  out.lr = lr;
  out.beta1 = b1;
  out.beta2 = b2;
  out.ramp = ramp;
  out.c1 = (float)(1.0 - b1);
  out.c2 = (float)(1.0 - b2);
  out.beta2f = (float)b2;
  out.eps = (float)eps;
  out.wd = (float)wd;
  out.pad = 0;
  if (!(out.eps > 0.f)) return "eps rounds to 0 in f32";
  return nullptr;
}

// (h, l) = (ah + al) (ch + cl) in double-double: the product's rounding error by fma, both cross terms, one fast two-sum
ISR_HD void dd_mul(double ah, double al, double ch, double cl, double& h, double& l) {
  const double p = ah * ch;
  double e = fma(ah, ch, -p);
  e = fma(ah, cl, e);
  e = fma(al, ch, e);
  h = p + e;
  l = e - (h - p);
}

// beta^t, t >= 0: binary powering over the bits of t, low bit first, in double-double; the high word is the answer
ISR_HD double pow_int(double beta, long long t) {
  double rh = 1.0, rl = 0.0, bh = beta, bl = 0.0;
  while (t > 0) {
    if (t & 1) dd_mul(rh, rl, bh, bl, rh, rl);
    t >>= 1;
    if (t > 0) dd_mul(bh, bl, bh, bl, bh, bl);
  }
  return rh;
}

ISR_HD double lr_at(double lr, double ramp, long long t) {
  if (!(ramp > 0.0)) return lr;
  const double frac = (double)(t + 1) / ramp;
  return lr * (frac < 1.0 ? frac : 1.0);
}

// t: the 1-based step
ISR_HD Scalars scalars_at(const Group& g, long long t) {
  const double bc1 = 1.0 - pow_int(g.beta1, t), bc2 = 1.0 - pow_int(g.beta2, t);
  Scalars s;
  s.step = (float)(lr_at(g.lr, g.ramp, t) / bc1);
  s.r = (float)sqrt(bc2);
  return s;
}

ISR_HD void update1(const Group& G, const Scalars& s, float& p, float g, float& m, float& v) {
  const float g1 = G.wd != 0.f ? fmaf(G.wd, p, g) : g;
  const float m1 = fmaf(G.c1, g1 - m, m);
  const float v1 = fmaf(G.c2, g1 * g1, G.beta2f * v);
  p = fmaf(-s.step, m1 / (sqrtf(v1) / s.r + G.eps), p);
  m = m1;
  v = v1;
}

// null, or what is wrong with the table; chunk_start (T + 1, nullable) and *chunks (nullable) are written when it is right.
// seen: n_slots bytes of scratch the caller provides (zeroed here).
inline const char* check_table(const isr_adam_tensor* table, int T, int G, long long n_slots, unsigned char* seen,
                               int32_t* chunk_start, long long* chunks, int* at) {
  for (long long s = 0; s < n_slots; ++s) seen[s] = 0;
  long long total = 0;
  for (int i = 0; i < T; ++i) {
    const isr_adam_tensor& d = table[i];
    *at = i;
    if (d.n < 0) return "negative element count";
    if (d.group < 0 || d.group >= G) return "group index outside 0 .. G - 1";
    if (d.slot < 0 || d.slot >= n_slots) return "step slot outside 0 .. n_slots - 1";
    if (seen[d.slot]) return "two tensors share a step slot";
    seen[d.slot] = 1;
    if (d.n > 0) {
      if (!d.p || !d.g || !d.m || !d.v) return "null array";
      if (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.m | (uintptr_t)d.v) & 3u) return "an array is not 4-byte aligned";
    }
    total += (d.n + kChunk - 1) / kChunk;
    if (total > kMaxChunks) return "more than 2^31 - 1 chunks";
  }
  if (chunk_start) {
    long long c = 0;
    chunk_start[0] = 0;
    for (int i = 0; i < T; ++i) {
      c += (table[i].n + kChunk - 1) / kChunk;
      chunk_start[i + 1] = (int32_t)c;
    }
  }
  if (chunks) *chunks = total;
  return nullptr;
}

// the tensor that owns chunk c: the i in [0, T) with chunk_start[i] <= c < chunk_start[i + 1]  (0 <= c < chunk_start[T])
ISR_HD int find_tensor(const int32_t* chunk_start, int T, int c) {
  int lo = 0, hi = T;      // chunk_start[lo] <= c < chunk_start[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (chunk_start[mid] <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the elements before the first one at which p is 16-byte aligned, or -1 when p, g, m and v do not share one misalignment
ISR_HD int shared_head(const isr_adam_tensor& d) {
  const unsigned a = (unsigned)((uintptr_t)d.p & 15u);
  if (((uintptr_t)d.g & 15u) != a || ((uintptr_t)d.m & 15u) != a || ((uintptr_t)d.v & 15u) != a || (a & 3u)) return -1;
  return (int)(((16u - a) & 15u) >> 2);
}

// the host build of one step over a checked table
inline void step_host(const isr_adam_tensor* table, int T, const Groups& groups, int64_t* steps, bool zero_grads) {
  for (int i = 0; i < T; ++i) {
    const isr_adam_tensor& d = table[i];
    const Group& G = groups.g[d.group];
    const Scalars s = scalars_at(G, (long long)steps[d.slot] + 1);
    for (int64_t e = 0; e < d.n; ++e) {
      update1(G, s, d.p[e], d.g[e], d.m[e], d.v[e]);
      if (zero_grads) d.g[e] = 0.f;
    }
  }
  for (int i = 0; i < T; ++i) steps[table[i].slot] += 1;
}

}  // namespace adam
}  // namespace isr
