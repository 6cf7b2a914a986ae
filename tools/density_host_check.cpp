// density_host_check.cpp — csrc/field_density.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/density_host_check.cpp -o density_host_check && ./density_host_check
// Runs sin32 and sincos32 over every exponent of f32 (both signs, the extremes of the mantissa) and the non-finite values, softplus32 and
// density32 over a sweep that crosses every branch, packs fields at the limits of the layout (H = 1 and 64, widths 1 and 256,
// 1 and 4 hidden layers) and evaluates points through them, and marches rays in both modes including P = 1 and a partly
// evaluated ray, marches the same rays from the far end (march_ray_back: both modes, P = 1, a partly evaluated ray, NaN
// densities, a null weights pointer) against the flipped forward march, and takes a key field (csrc/field_mlp.hpp) of odd widths through make_layout / pack_host / eval_rows_host, so that
// the helpers the two headers share run from both sides.  Checks ranges and a few identities; prints one line per case; exit status 0 = all hold.
// The log of one such run is profiles/density_host_sanitizers.txt.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __host__
#define __device__
#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/field_density.hpp"

using namespace isr::density;

namespace {

int report(const char* name, int bad) {
  std::printf("%-44s %s\n", name, bad ? "MISMATCH" : "ok");
  return bad;
}

int check_sincos() {
  int bad = 0;
  for (uint32_t e = 0; e < 255; ++e)
    for (uint32_t m : {0u, 1u, 0x400000u, 0x7fffffu, 0x2aaaaau})
      for (uint32_t sg : {0u, 0x80000000u}) {
        const uint32_t u = sg | (e << 23) | m;
        float a, s, c;
        std::memcpy(&a, &u, 4);
        sincos32(a, &s, &c);
        if (!(std::fabs(s) <= 1.f) || !(std::fabs(c) <= 1.f)) ++bad;
        const float s1 = isr::field::sin32(a);
        if (!(std::fabs(s1) <= 1.f) || (e < 144 && std::memcmp(&s1, &s, 4) != 0)) ++bad;       // |a| < 2^17: the same bits
        if (std::fabs((double)s - std::sin((double)a)) > 1.2e-7 || std::fabs((double)c - std::cos((double)a)) > 1.2e-7) ++bad;
      }
  float s, c;
  for (float a : {INFINITY, -INFINITY, NAN}) {
    sincos32(a, &s, &c);
    const float s1 = isr::field::sin32(a);
    if (s == s || c == c || s1 == s1) ++bad;
  }
  sincos32(-0.f, &s, &c);
  if (!std::signbit(s) || c != 1.f || !std::signbit(isr::field::sin32(-0.f))) ++bad;
  return report("sin32 / sincos32: every exponent, non-finite, -0", bad);
}

int check_activations() {
  int bad = 0;
  for (float beta : {10.f, 1.f, 0.01f, 1000.f})
    for (int i = -4000; i <= 4000; ++i) {
      const float z = (float)i * 0.05f;
      const float s = softplus32(z, beta);
      const double t = (double)beta * z;
      const double ref = t > 20 ? z : std::log1p(std::exp(t)) / beta;
      if (!(s >= 0.f) || std::fabs(s - ref) > 1e-6 * (std::fabs(ref) + 1e-30)) ++bad;
      const float d = density32(std::fabs(z));
      if (!(d >= 0.f && d <= 1.f) || std::fabs(d - -std::expm1(-std::fabs((double)z))) > 1e-7) ++bad;
    }
  if (softplus32(-INFINITY, 10.f) != 0.f || softplus32(3e38f, 10.f) != 3e38f || density32(3e38f) != 1.f) ++bad;
  const float n1 = softplus32(NAN, 10.f), n2 = density32(NAN);
  if (n1 == n1 || n2 == n2) ++bad;
  return report("softplus32 / density32: sweep, limits, NaN", bad);
}

int check_field(int H, int n_hidden, int width, int N) {
  std::vector<int32_t> widths(n_hidden, width);
  Layout lay;
  if (!make_layout(n_hidden, widths.data(), H, lay)) return report("make_layout", 1);
  size_t nw = 0, nb = 0;
  int K = 6 * H;
  for (int l = 0; l < n_hidden; ++l) {
    nw += (size_t)width * K;
    nb += width;
    K = width;
  }
  nw += K;
  nb += 1;
  std::vector<float> W(nw), b(nb), freqs(H), pack(lay.total_words);
  unsigned s = 12345u + H + width;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 32768.f - 1.f;
  };
  for (auto& v : W) v = rnd() / std::sqrt((float)width);
  for (auto& v : b) v = 0.1f * rnd();
  for (int i = 0; i < H; ++i) freqs[i] = 0.1f * std::ldexp(1.f, i);
  pack_host(lay, freqs.data(), 10.f, W.data(), b.data(), pack.data());
  const HostField hf(lay, pack.data());      // the library's own unpacking of the pack
  const HostWeights& hw = hf.hw;
  const std::vector<std::vector<float>>& wt = hf.wt;
  int bad = 0;
  // the pack round trip: every weight where w_index says
  {
    const float* w = W.data();
    for (int l = 0; l < n_hidden; ++l) {
      const Layer& L = lay.L[l];
      for (int j = 0; j < L.O; ++j)
        for (int k = 0; k < L.K; ++k)
          if (wt[l][(size_t)k * L.O + j] != w[(size_t)j * L.K + k]) ++bad;
      w += (size_t)L.O * L.K;
    }
  }
  std::vector<float> rho(N);
  for (int n = 0; n < N; ++n) {
    const float x[3] = {1.2f * rnd(), 1.2f * rnd(), 1.2f * rnd()};
    rho[n] = point_density_host(lay, pack.data(), hw, x);
    if (!(rho[n] >= 0.f && rho[n] <= 1.f)) ++bad;
  }
  // march: both modes, whole and partly evaluated, weights and no weights
  std::vector<float> len(N), wts(N);
  for (int n = 0; n < N; ++n) len[n] = 0.1f * (float)(n + 1);
  for (float thr : {0.2f, -1.f, 2.f}) {
    float d0, d1;
    int32_t h0, h1;
    march_ray(N, len.data(), rho.data(), N, thr, wts.data(), &d0, &h0);
    march_ray(N, len.data(), rho.data(), N, thr, nullptr, &d1, &h1);
    if (d0 != d1 || h0 != h1) ++bad;
    if (thr >= 0.f) {
      int first = N;
      for (int n = N - 1; n >= 0; --n)
        if (rho[n] > thr) first = n;
      if (h0 != (first < N) || d0 != (first < N ? len[first] : 0.f)) ++bad;
      if (first < N) {
        march_ray(N, len.data(), rho.data(), first + 1, thr, nullptr, &d1, &h1);       // stopped after the first hit
        if (d0 != d1 || h0 != h1) ++bad;
      }
    }
  }
  float d;
  int32_t h;
  march_ray(1, len.data(), rho.data(), 1, 0.2f, wts.data(), &d, &h);
  char name[96];
  std::snprintf(name, sizeof name, "field H %2d, %d x %3d, %3d points, marches", H, n_hidden, width, N);
  return report(name, bad);
}

// a key field of widths no multiple of 4, 8 or 32 on either side of kMfmaMinK: layout, pack, unpack, host evaluation
int check_key_field() {
  namespace kf = isr::field;
  const int32_t widths[5] = {3, 5, 40, 33, 7};
  const float omega[4] = {30.f, 1.5f, 0.f, 2.f};
  const int32_t sine[4] = {1, 1, 0, 1};
  kf::Layout lay;
  if (!kf::make_layout(4, widths, lay)) return report("field::make_layout", 1);
  size_t nw = 0, nb = 0;
  for (int l = 0; l < 4; ++l) {
    nw += (size_t)widths[l] * widths[l + 1];
    nb += widths[l + 1];
  }
  std::vector<float> W(nw), b(nb), pack(lay.total_words);
  unsigned s = 777u;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 32768.f - 1.f;
  };
  for (auto& v : W) v = 0.2f * rnd();
  for (auto& v : b) v = 0.1f * rnd();
  kf::pack_host(lay, W.data(), b.data(), omega, sine, pack.data());
  int bad = 0;
  std::vector<std::vector<float>> dense(4);
  const float* rows[kf::kMaxLayers];
  const float* w = W.data();
  for (int l = 0; l < 4; ++l) {
    const kf::Layer& L = lay.L[l];
    dense[l].resize((size_t)L.O * L.K);
    kf::unpack_layer(L, pack.data(), dense[l].data(), false);
    if (std::memcmp(dense[l].data(), w, dense[l].size() * 4) != 0) ++bad;            // the round trip
    if (L.mfma != (L.K >= kf::kMfmaMinK) || L.OP % 32 || L.OP < L.O) ++bad;
    rows[l] = dense[l].data();
    w += dense[l].size();
  }
  const int N = 70;
  std::vector<float> pts(3 * N), out((size_t)N * 8, -7.f);
  for (auto& v : pts) v = rnd();
  kf::eval_rows_host(lay, pack.data(), rows, pts.data(), 0, N, out.data(), 8);
  for (int n = 0; n < N; ++n) {
    for (int j = 0; j < 7; ++j)
      if (!(std::fabs(out[n * 8 + j]) <= 1.f)) ++bad;                                // the last layer is a sine
    if (out[n * 8 + 7] != -7.f) ++bad;                                               // the column past the width is not written
  }
  return report("key field 3-5-40-33-7: layout, pack, host rows", bad);
}

// march_ray_back against march_ray on the flipped ray: the weights are the forward weights of the reversed densities,
// reversed; a partly evaluated ray in threshold mode gives the bits of the fully evaluated one.
int check_back_march() {
  int bad = 0;
  unsigned s = 99u;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 65536.f;
  };
  for (int P : {1, 2, 63, 64, 65, 200, kMaxP})
    for (float thr : {0.5f, -1.f}) {
      std::vector<float> len(P), rho(P), rev(P), ones(P, 1.f), w(P), wrev(P), work(P);
      for (int k = 0; k < P; ++k) {
        len[k] = 0.01f * (float)k - 0.3f;
        rho[k] = rnd() * (thr < 0.f ? 0.2f : 1.f);
        if (P > 2 && k == P / 2) rho[k] = NAN;
        rev[P - 1 - k] = rho[k];
      }
      float dep, drev;
      int32_t hit, hrev;
      work = rho;
      march_ray_back(P, len.data(), work.data(), 0, thr, w.data(), &dep, &hit);
      march_ray(P, ones.data(), rev.data(), P, thr, wrev.data(), &drev, &hrev);
      for (int k = 0; k < P; ++k)
        if (std::memcmp(&w[k], &wrev[P - 1 - k], 4) != 0 && !(w[k] != w[k] && wrev[P - 1 - k] != wrev[P - 1 - k])) ++bad;
      if (hit != hrev) ++bad;
      work = rho;
      float dep0;
      int32_t hit0;
      march_ray_back(P, len.data(), work.data(), 0, thr, nullptr, &dep0, &hit0);             // null weights: the same depth
      if (std::memcmp(&dep, &dep0, 4) != 0 || hit != hit0) ++bad;
      if (thr >= 0.f && hit) {
        int last = P - 1;
        while (!(rho[last] > thr)) --last;
        const int lo = last / 64 * 64;                                                       // the tile of the last hit
        std::vector<float> part(rho), w2(P);
        for (int k = 0; k < lo; ++k) part[k] = 7.f;                                          // in front of lo: above the threshold, never read
        float dep2;
        int32_t hit2;
        march_ray_back(P, len.data(), part.data(), lo, thr, w2.data(), &dep2, &hit2);
        for (int k = 0; k < lo; ++k)
          if (part[k] != 7.f) ++bad;                                                         // nor written
        if (std::memcmp(&dep, &dep2, 4) != 0 || hit2 != 1 || std::memcmp(w.data(), w2.data(), (size_t)P * 4) != 0) ++bad;
        if (w[last] != 1.f) ++bad;
      }
    }
  return report("march_ray_back: flipped march, partial ray, null", bad);
}

}  // namespace

int main() {
  int bad = 0;
  bad += check_sincos();
  bad += check_activations();
  bad += check_field(1, 1, 1, 3);
  bad += check_field(1, 4, 256, 5);
  bad += check_field(64, 1, 256, 5);
  bad += check_field(60, 2, 256, 33);
  bad += check_field(4, 2, 33, 70);
  bad += check_field(64, 4, 1, 4);
  bad += check_key_field();
  bad += check_back_march();
  Layout lay;
  const int32_t w5[5] = {8, 8, 8, 8, 8}, w257[1] = {257};
  int refused = 0;
  refused += !make_layout(5, w5, 4, lay);
  refused += !make_layout(1, w257, 4, lay);
  refused += !make_layout(1, w5, 0, lay);
  refused += !make_layout(1, w5, 65, lay);
  bad += report("layouts out of range are refused", refused != 4);
  std::printf("%s\n", bad ? "FAILED" : "all cases hold");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
