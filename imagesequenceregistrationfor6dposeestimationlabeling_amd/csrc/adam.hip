// adam.hip — the fused multi-tensor Adam (include/isr_adam.h states every rule, csrc/adam.hpp the arithmetic):
//   isr_adam_step: one launch over every tensor of every group, one 256-thread workgroup per chunk of 4 096 elements, found
//     by binary search of chunk_start; then one small launch that bumps the step counters.  HBM-bound byte work: 16 bytes
//     read and 12 written per element (16 with zero_grads), moved as dwordx4 where p, g, m and v share their misalignment.
//   isr_adam_zero_grads: the same split, storing +0 to every gradient.
// The groups travel as kernel arguments, the table and the counters stay on the device: no copy, no synchronisation, no
// workspace, no atomics, no hand-off between workgroups.
#include "isr_common.hpp"

#include <vector>

#include "../../include/isr_adam.h"
#include "adam.hpp"

namespace {

using namespace isr::adam;

enum Mode { kStep = 0, kStepZero = 1, kZero = 2 };

// The table's pointers are loaded from memory, so the compiler takes them for generic ones and would emit flat_load /
// flat_store: every array is device global memory, and saying so gives global_load_dwordx4 / global_store_dwordx4.
typedef __attribute__((address_space(1))) float gfloat;
typedef float quad __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) quad gquad;

struct Arrays {
  gfloat *p, *g, *m, *v;
};

template <int MODE>
__device__ __forceinline__ void one_element(const Group& G, const Scalars& s, const Arrays& a, int64_t e) {
  if (MODE != kZero) {
    float p = a.p[e], m = a.m[e], v = a.v[e];
    update1(G, s, p, a.g[e], m, v);
    a.p[e] = p;
    a.m[e] = m;
    a.v[e] = v;
  }
  if (MODE != kStep) a.g[e] = 0.f;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void adam_kernel(const isr_adam_tensor* __restrict__ table,
                                                        const int32_t* __restrict__ chunk_start, int T, Groups groups,
                                                        const int64_t* __restrict__ steps) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int i = find_tensor(chunk_start, T, c);
  const isr_adam_tensor d = table[i];
  const int64_t lo = (int64_t)(c - chunk_start[i]) * kChunk;
  const int64_t hi = d.n - lo < kChunk ? d.n : lo + kChunk;      // [lo, hi) inside [0, n)
  if (lo >= hi) return;
  Scalars s{0.f, 1.f};
  // d.group was checked on the host (isr_adam_table_host); the mask keeps a stray one inside the argument block
  const Group& G = groups.g[d.group & (kMaxGroups - 1)];
  if (MODE != kZero) s = scalars_at(G, (long long)steps[d.slot] + 1);
  const Arrays a{(gfloat*)d.p, (gfloat*)d.g, (gfloat*)d.m, (gfloat*)d.v};

  const int head = shared_head(d);
  if (head < 0) {      // no common alignment: every element by itself
    for (int64_t e = lo + tid; e < hi; e += kThreads) one_element<MODE>(G, s, a, e);
    return;
  }
  // lo is a multiple of 4, so the first aligned element of the chunk is lo + head
  const int64_t a0 = lo + head < hi ? lo + head : hi;
  const int64_t quads = (hi - a0) >> 2, a1 = a0 + 4 * quads;
  for (int64_t q = tid; q < quads; q += kThreads) {
    const int64_t e = a0 + 4 * q;
    if (MODE != kZero) {
      quad p = *(const gquad*)(a.p + e);
      const quad g = *(const gquad*)(a.g + e);
      quad m = *(const gquad*)(a.m + e);
      quad v = *(const gquad*)(a.v + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        update1(G, s, pk, g[k], mk, vk);
        p[k] = pk;
        m[k] = mk;
        v[k] = vk;
      }
      *(gquad*)(a.p + e) = p;
      *(gquad*)(a.m + e) = m;
      *(gquad*)(a.v + e) = v;
    }
    if (MODE != kStep) *(gquad*)(a.g + e) = quad{0.f, 0.f, 0.f, 0.f};
  }
  // the up to 3 elements before a0 and the up to 3 from a1 on: lanes 0 .. 2 and 3 .. 5
  if (tid < 3) {
    const int64_t e = lo + tid;
    if (e < a0) one_element<MODE>(G, s, a, e);
  } else if (tid < 6) {
    const int64_t e = a1 + (tid - 3);
    if (e < hi) one_element<MODE>(G, s, a, e);
  }
}

__global__ __launch_bounds__(kThreads) void adam_bump_kernel(const isr_adam_tensor* __restrict__ table, int T,
                                                             int64_t* __restrict__ steps) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < T) steps[table[i].slot] += 1;      // a slot belongs to one tensor of the table
}

int make_groups(const char* who, const double* groups_host, int G, Groups& out) {
  ISR_REQUIRE(G >= 1 && G <= kMaxGroups, "%s: G=%d outside 1..%d", who, G, kMaxGroups);
  ISR_REQUIRE(groups_host, "%s: null groups", who);
  out = Groups{};
  for (int k = 0; k < G; ++k) {
    const char* bad = make_group(groups_host + ISR_ADAM_GROUP_DOUBLES * k, out.g[k]);
    ISR_REQUIRE(!bad, "%s: group %d: %s", who, k, bad);
  }
  return ISR_OK;
}

int check_launch_args(const char* who, const void* table, const void* chunk_start, int T, int64_t chunks) {
  ISR_REQUIRE(T >= 0, "%s: T=%d", who, T);
  ISR_REQUIRE(T == 0 || (table && chunk_start), "%s: null table", who);
  ISR_REQUIRE(chunks >= 0 && chunks <= kMaxChunks && (T > 0 || chunks == 0), "%s: chunks=%lld with T=%d", who,
              (long long)chunks, T);
  return ISR_OK;
}

}  // namespace

extern "C" int isr_adam_geometry(int what) {
  switch (what) {
    case 0: return (int)sizeof(isr_adam_tensor);
    case 1: return kChunk;
    case 2: return kThreads;
    case 3: return kMaxGroups;
    default: isr::set_error("isr_adam_geometry: what=%d", what); return ISR_ERR_ARG;
  }
}

extern "C" int isr_adam_table_host(const isr_adam_tensor* table_host, int T, int G, int64_t n_slots, int32_t* chunk_start_host,
                                   int64_t* chunks) {
  const char* who = "isr_adam_table_host";
  ISR_REQUIRE(T >= 0 && (T == 0 || table_host), "%s: T=%d or a null table", who, T);
  ISR_REQUIRE(G >= 1 && G <= kMaxGroups, "%s: G=%d outside 1..%d", who, G, kMaxGroups);
  ISR_REQUIRE(n_slots >= 0, "%s: n_slots=%lld", who, (long long)n_slots);
  std::vector<unsigned char> seen((size_t)n_slots);
  long long total = 0;
  int at = 0;
  const char* bad = check_table(table_host, T, G, n_slots, seen.data(), chunk_start_host, &total, &at);
  ISR_REQUIRE(!bad, "%s: tensor %d: %s", who, at, bad);
  if (chunks) *chunks = total;
  return ISR_OK;
}

extern "C" int isr_adam_step(const isr_adam_tensor* table, const int32_t* chunk_start, int T, int64_t chunks,
                             const double* groups_host, int G, int64_t* steps, int zero_grads, isr_stream_t stream) {
  const char* who = "isr_adam_step";
  Groups groups;
  if (int rc = make_groups(who, groups_host, G, groups)) return rc;
  if (int rc = check_launch_args(who, table, chunk_start, T, chunks)) return rc;
  if (T == 0) return ISR_OK;
  ISR_REQUIRE(steps, "%s: null steps", who);
  if (chunks > 0) {
    if (zero_grads)
      adam_kernel<kStepZero><<<(unsigned)chunks, kThreads, 0, isr::as_stream(stream)>>>(table, chunk_start, T, groups, steps);
    else
      adam_kernel<kStep><<<(unsigned)chunks, kThreads, 0, isr::as_stream(stream)>>>(table, chunk_start, T, groups, steps);
    ISR_CHECK_LAUNCH("adam_kernel");
  }
  adam_bump_kernel<<<(unsigned)((T + kThreads - 1) / kThreads), kThreads, 0, isr::as_stream(stream)>>>(table, T, steps);
  ISR_CHECK_LAUNCH("adam_bump_kernel");
  return ISR_OK;
}

extern "C" int isr_adam_zero_grads(const isr_adam_tensor* table, const int32_t* chunk_start, int T, int64_t chunks,
                                   isr_stream_t stream) {
  const char* who = "isr_adam_zero_grads";
  if (int rc = check_launch_args(who, table, chunk_start, T, chunks)) return rc;
  if (T == 0 || chunks == 0) return ISR_OK;
  adam_kernel<kZero><<<(unsigned)chunks, kThreads, 0, isr::as_stream(stream)>>>(table, chunk_start, T, Groups{}, nullptr);
  ISR_CHECK_LAUNCH("adam_kernel");
  return ISR_OK;
}

extern "C" int isr_adam_step_host(const isr_adam_tensor* table_host, int T, const double* groups_host, int G,
                                  int64_t* steps_host, int64_t n_slots, int zero_grads) {
  const char* who = "isr_adam_step_host";
  Groups groups;
  if (int rc = make_groups(who, groups_host, G, groups)) return rc;
  ISR_REQUIRE(T >= 0 && (T == 0 || table_host), "%s: T=%d or a null table", who, T);
  if (T == 0) return ISR_OK;
  ISR_REQUIRE(steps_host && n_slots >= 0, "%s: null steps or n_slots=%lld", who, (long long)n_slots);
  std::vector<unsigned char> seen((size_t)n_slots);
  int at = 0;
  const char* bad = check_table(table_host, T, G, n_slots, seen.data(), nullptr, nullptr, &at);
  ISR_REQUIRE(!bad, "%s: tensor %d: %s", who, at, bad);
  for (int i = 0; i < T; ++i)
    ISR_REQUIRE(steps_host[table_host[i].slot] >= 0, "%s: tensor %d: negative step counter", who, i);
  step_host(table_host, T, groups, steps_host, zero_grads != 0);
  return ISR_OK;
}

extern "C" int isr_adam_scalars_host(const double* group_host, int64_t t, double* out4, float* out2) {
  const char* who = "isr_adam_scalars_host";
  ISR_REQUIRE(group_host && out4 && out2, "%s: null pointer", who);
  ISR_REQUIRE(t >= 1, "%s: t=%lld (the step is 1-based)", who, (long long)t);
  Group g;
  const char* bad = make_group(group_host, g);
  ISR_REQUIRE(!bad, "%s: %s", who, bad);
  const Scalars s = scalars_at(g, (long long)t);
  out4[0] = lr_at(g.lr, g.ramp, (long long)t);
  out4[1] = pow_int(g.beta1, (long long)t);
  out4[2] = pow_int(g.beta2, (long long)t);
  out4[3] = 0.0;
  out2[0] = s.step;
  out2[1] = s.r;
  return ISR_OK;
}
