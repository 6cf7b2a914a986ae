// hd.hpp — what host and device code share, written once: the host/device function macro, the float-bits helpers, Philox4x32-10
// and pad_pow2.  A plain C++ compiler can include this header (the tools/*_host_check.cpp programs do, through the feature
// headers); it does not include hip_runtime.h.  Everything is built with -ffp-contract=off: host and device give the same bits.
#pragma once
#include <cstdint>

// A function of a feature header that both the kernels and the host definitions call.
#if defined(__HIPCC__)
#define ISR_HD __host__ __device__ inline
#else
#define ISR_HD inline
#endif

namespace isr {

// ---- float bits
constexpr uint32_t kNanBits = 0x7FC00000u;           // the canonical quiet NaN: every NaN an entry writes

ISR_HD float bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

ISR_HD float canonical(float z) { return z != z ? bits_float(kNanBits) : z; }

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants)
ISR_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// u = (word >> 8) * 2^-24, in [0, 1): exact in f32
ISR_HD float unit_float(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-08f; }

// ---- the power of two at or above K (1 for K < 1)
ISR_HD constexpr int pad_pow2(int K) {
  int p = 1;
  while (p < K) p <<= 1;
  return p;
}

}  // namespace isr
