// ea_grad_host_check.cpp — csrc/ea_grad.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/ea_grad_host_check.cpp -o ea_grad_host_check && ./ea_grad_host_check
// Drives backward_host with arrays of exactly the sizes the header asks for, and the device's route restated on the host —
// the rows of a workgroup's rays at the LDS stride P | 1 inside arrays of exactly kRowFloats floats, walked by the same
// upstream / transmittance / adjoint / feature_grad — and checks that the two give the same bits, that a null dweights
// equals zeros, that each output may be left out, that threshold mode gives +0 densities, and that check_call refuses what
// include/isr_ea_grad.h says it refuses.  The cases are the tests' edge cases: P = 1, 2, 3, 64, 65, 257, 2 048, 4 096, F = 1,
// 3, 16, 17, 33, 64, ray counts around a workgroup's share, densities of 0, of 1, above 1 and negative, a NaN density, and a
// dimage with a NaN and an infinity.  Prints one line per case; exit status 0 = all hold.  The log of one such run is
// profiles/ea_grad_host_sanitizers.txt.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/ea_grad.hpp"

using namespace isr::ea_grad;

namespace {

unsigned seed = 24680u;
float uni() {                                        // U(0, 1)
  seed = seed * 1664525u + 1013904223u;
  return (float)((seed >> 8) & 0xffff) / 65536.f;
}

int fails = 0;

bool same(const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    uint32_t u, v;
    std::memcpy(&u, &a[i], 4);
    std::memcpy(&v, &b[i], 4);
    if (u != v && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  }
  return true;
}

// The kernel's three phases over one workgroup's rays, with its index arithmetic and arrays of the kernel's sizes.
void group_route(const float* rho, const float* features, int N, int P, int F, float threshold, const float* dimage,
                 const float* dweights, float* ddensities, float* dfeatures) {
  const int R = rays_per_group(P), S = row_stride(P);
  const bool chain = ddensities && threshold < 0.f;
  std::vector<float> cs(kRowFloats), Ts(kRowFloats), gs(kRowFloats);
  for (long ray0 = 0; ray0 < N; ray0 += R) {
    const int rays = (int)std::min<long>(R, N - ray0), pairs = rays * P;
    const size_t q0 = (size_t)ray0 * P;
    for (int i = 0; i < pairs; ++i) {
      const int r = i / P, k = i - r * P;
      cs.at(r * S + k) = absorbance(rho[q0 + i], threshold);
      if (chain) gs.at(r * S + k) = upstream(dimage + (size_t)(ray0 + r) * (F + 1), features + (q0 + i) * F, F, dweights ? dweights[q0 + i] : 0.f);
    }
    for (int r = 0; r < rays; ++r) {
      if ((size_t)r * S + P > (size_t)kRowFloats) { ++fails; return; }      // a row would leave the array
      transmittance(P, cs.data() + r * S, Ts.data() + r * S);
      if (chain) adjoint(P, cs.data() + r * S, Ts.data() + r * S, dimage[(size_t)(ray0 + r) * (F + 1) + F], gs.data() + r * S);
    }
    for (int i = 0; i < pairs && ddensities; ++i) ddensities[q0 + i] = chain ? gs.at((i / P) * S + i % P) : 0.f;
    for (int e = 0; e < pairs * F && dfeatures; ++e) {
      const int i = e / F, ch = e - i * F, r = i / P, k = i - r * P;
      dfeatures[q0 * F + e] = feature_grad(cs.at(r * S + k), Ts.at(r * S + k), dimage[(size_t)(ray0 + r) * (F + 1) + ch]);
    }
  }
}

// rho kinds: 0 U(0, 1), 1 small, 2 all 0, 3 all 1, 4 U(-0.5, 1.5), 5 a NaN in the middle ray; dimage kinds: 0 random, 1 a NaN
// and an infinity
void run(const char* what, int N, int P, int F, int rho_kind, int dimage_kind, float threshold) {
  const size_t NP = (size_t)N * P;
  std::vector<float> rho(NP), feat(NP * F), dimage((size_t)N * (F + 1)), dw(NP), zeros(NP, 0.f);
  for (auto& v : rho) v = rho_kind == 1 ? 0.05f * uni() : rho_kind == 2 ? 0.f : rho_kind == 3 ? 1.f : rho_kind == 4 ? 2.f * uni() - 0.5f : uni();
  if (rho_kind == 5) rho[(size_t)(N / 2) * P + P / 2] = std::numeric_limits<float>::quiet_NaN();
  for (auto& v : feat) v = 2.f * uni() - 1.f;
  for (auto& v : dimage) v = 2.f * uni() - 1.f;
  for (auto& v : dw) v = 2.f * uni() - 1.f;
  if (dimage_kind == 1) {
    dimage[dimage.size() / 3] = std::numeric_limits<float>::quiet_NaN();
    dimage[dimage.size() / 2] = std::numeric_limits<float>::infinity();
  }
  bool ok = check_call(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), rho.data(), nullptr) == nullptr;
  std::vector<float> dd(NP, 7.f), df(NP * F, 7.f), dd2(NP, 9.f), df2(NP * F, 9.f), dd3(NP, 5.f), df3(NP * F, 5.f);
  backward_host(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), dw.data(), dd.data(), df.data());
  group_route(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), dw.data(), dd2.data(), df2.data());
  ok = ok && same(dd, dd2) && same(df, df2);
  backward_host(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), dw.data(), dd3.data(), nullptr);      // each output alone
  backward_host(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), dw.data(), nullptr, df3.data());
  ok = ok && same(dd, dd3) && same(df, df3);
  backward_host(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), nullptr, dd2.data(), df2.data());      // null dweights = zeros
  group_route(rho.data(), feat.data(), N, P, F, threshold, dimage.data(), zeros.data(), dd3.data(), df3.data());
  ok = ok && same(dd2, dd3) && same(df2, df3);
  if (threshold >= 0.f)
    for (float v : dd) {
      uint32_t u;
      std::memcpy(&u, &v, 4);
      ok = ok && u == 0;                              // +0, not -0
    }
  std::printf("%-58s N %-5d P %-5d F %-3d rays a group %-3d %s\n", what, N, P, F, rays_per_group(P), ok ? "ok" : "FAILED");
  fails += !ok;
}

}  // namespace

int main() {
  for (int P : {1, 2, 3, 64, 65, 257})
    for (int F : {1, 3, 16, 17, 33}) run("sizes", 5, P, F, (P + F) % 2, 0, -1.f);
  for (int P : {1, 64, 128, 256, 2048}) {
    const int R = rays_per_group(P);
    for (int N : {std::max(R - 1, 1), R, R + 1, 2 * R + 1}) run("ray counts around a workgroup's share", N, P, 3, 1, 0, -1.f);
  }
  run("P = 4 096, F = 64", 2, 4096, 64, 1, 0, -1.f);
  run("densities all 0", 6, 40, 3, 2, 0, -1.f);
  run("densities all 1", 6, 40, 3, 3, 0, -1.f);
  run("densities above 1 and negative", 6, 40, 3, 4, 0, -1.f);
  run("a NaN density in the middle ray", 7, 40, 3, 5, 0, -1.f);
  run("dimage with a NaN and an infinity", 6, 40, 3, 1, 1, -1.f);
  run("threshold mode", 70, 40, 3, 1, 0, 0.02f);
  run("threshold mode, a NaN density", 7, 40, 3, 5, 1, 0.5f);
  run("threshold mode, nothing above", 6, 40, 3, 0, 0, 2.f);
  const float x = 0.f;
  bool refused = check_call(&x, &x, -1, 5, 3, -1.f, &x, &x, &x) && check_call(&x, &x, 2, 0, 3, -1.f, &x, &x, &x) &&
                 check_call(&x, &x, 2, 4097, 3, -1.f, &x, &x, &x) && check_call(&x, &x, 2, 5, 0, -1.f, &x, &x, &x) &&
                 check_call(&x, &x, 2, 5, 65, -1.f, &x, &x, &x) && check_call(&x, &x, 2, 5, 3, NAN, &x, &x, &x) &&
                 check_call(&x, &x, 2, 5, 3, -1.f, &x, nullptr, nullptr) && check_call(nullptr, &x, 2, 5, 3, -1.f, &x, &x, &x) &&
                 check_call(&x, nullptr, 2, 5, 3, -1.f, &x, &x, &x) && check_call(&x, &x, 2, 5, 3, -1.f, nullptr, &x, &x) &&
                 !check_call(nullptr, nullptr, 0, 5, 3, -1.f, nullptr, nullptr, nullptr) &&
                 check_call(nullptr, nullptr, 0, 5, 65, -1.f, nullptr, &x, &x) && !check_call(&x, &x, 2, 4096, 64, 0.f, &x, nullptr, &x);
  for (int P = 1; P <= kMaxP; ++P) {
    const int R = rays_per_group(P);
    refused = refused && R >= 1 && R <= kMaxGroupRays && (size_t)(R - 1) * row_stride(P) + P <= (size_t)kRowFloats;
  }
  std::printf("%-58s %s\n", "refusals; every P's rows stay inside the arrays", refused ? "ok" : "FAILED");
  fails += !refused;
  std::printf(fails ? "%d cases FAILED\n" : "all cases hold\n", fails);
  return fails != 0;
}
