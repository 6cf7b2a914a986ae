// resample_host_check.cpp — csrc/resample.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/resample_host_check.cpp -o resample_host_check && ./resample_host_check
// Drives sample_pdf_row and resample_row over the shapes of the tests — P = 3, 4, 5, 64, 257 and 1024, n = 1, 7, P and 1024,
// with and without the input samples, both kinds of units — and over the degenerate rows: all-zero weights, one spike, heavy
// weights, repeated and unsorted lengths, a NaN weight, infinite and negative weights, NaN and infinite lengths; with arrays of
// exactly the sizes the header asks for.  Checks what can be checked without a second implementation: the row is sorted by
// its keys, holds every input length bit for bit, the samples of a clean row lie in [bins_0, bins_nb], a NaN weight gives
// canonical NaN samples sorted last, a row does not depend on its ray id when the units are deterministic and does when
// they are not.  Prints one line per case; exit status 0 = all hold.  The log of one such run is
// profiles/resample_host_sanitizers.txt.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/resample.hpp"

using namespace isr::resample;

namespace {

unsigned seed = 2468u;
float rnd() {                                        // in [0, 1)
  seed = seed * 1664525u + 1013904223u;
  return (float)((seed >> 8) & 0xffff) / 65536.f;
}

enum Kind { kRandom, kZero, kSpike, kHeavy, kRepeated, kUnsorted, kNanWeight, kInfWeight, kNegWeight, kNanLength, kInfLength, kKinds };
const char* kNames[kKinds] = {"random", "all-zero weights", "one spike", "heavy weights", "repeated lengths", "unsorted lengths",
                              "a NaN weight", "an infinite weight", "negative weights", "a NaN length", "an infinite length"};

int fails = 0;

void run(int P, int n, int add, int det, Kind kind) {
  Spec sp;
  const char* wrong = make_spec(1, P - 2, n, det, 1e-5f, 0x500000003ull, sp);
  if (wrong) {
    std::printf("P %-5d n %-5d refused: %s\n", P, n, wrong);
    ++fails;
    return;
  }
  std::vector<float> ln((size_t)P), w((size_t)P), bins((size_t)P - 1), cdf((size_t)P - 1), out((size_t)n + (add ? P : 0)), again(out.size());
  std::vector<uint32_t> keys(out.size());
  float z = 0.1f;
  for (int k = 0; k < P; ++k) {
    z += kind == kRepeated && rnd() < 0.5f ? 0.f : 0.01f + rnd() * 0.05f;
    ln[k] = z;
    const float r = rnd();
    w[k] = kind == kZero || kind == kSpike ? 0.f : r * r * r * r * (kind == kHeavy ? 1e4f : 1.f);
  }
  const int mid = P / 2 < P - 1 ? (P / 2 > 0 ? P / 2 : 1) : P - 2;
  if (kind == kSpike) w[mid] = 1.f;
  if (kind == kUnsorted)
    for (int k = P - 1; k > 0; --k) std::swap(ln[k], ln[(int)(rnd() * (k + 1))]);
  if (kind == kNanWeight) w[mid] = std::numeric_limits<float>::quiet_NaN();
  if (kind == kInfWeight) w[mid] = std::numeric_limits<float>::infinity();
  if (kind == kNegWeight)
    for (int k = 0; k < P; k += 2) w[k] = -w[k];
  if (kind == kNanLength) ln[mid] = std::numeric_limits<float>::quiet_NaN();
  if (kind == kInfLength) ln[P - 1] = std::numeric_limits<float>::infinity();

  resample_row(sp, ln.data(), w.data(), add, 17u, bins.data(), cdf.data(), keys.data(), out.data());
  bool ok = true;
  for (size_t k = 1; k < out.size(); ++k) ok = ok && sort_key(out[k - 1]) <= sort_key(out[k]);
  if (add)
    for (int k = 0; k < P; ++k) {
      bool found = false;
      for (size_t j = 0; j < out.size() && !found; ++j) found = sort_key(out[j]) == sort_key(ln[k]);
      ok = ok && found;
    }
  int nans = 0;
  for (float v : out) nans += float_bits(v) == isr::kNanBits;
  const bool clean = kind <= kRepeated;
  if (clean) {
    ok = ok && nans == 0;
    std::vector<float> s((size_t)n), c2((size_t)P - 1);
    sample_pdf_row(sp, bins.data(), w.data() + 1, 17u, c2.data(), s.data());
    for (float v : s) ok = ok && v >= bins[0] && v <= bins[P - 2];
    for (int j = 0; j + 1 < P - 1; ++j) ok = ok && c2[j] <= c2[j + 1];                  // the knots never decrease
  }
  if (kind == kNanWeight) {
    ok = ok && nans == n;
    for (int s = 0; s < n; ++s) ok = ok && float_bits(out[out.size() - 1 - s]) == isr::kNanBits;
  }
  resample_row(sp, ln.data(), w.data(), add, 18u, bins.data(), cdf.data(), keys.data(), again.data());
  bool equal = true;
  for (size_t k = 0; k < out.size(); ++k) equal = equal && float_bits(out[k]) == float_bits(again[k]);
  if (det) ok = ok && equal;
  if (!det && clean && kind != kZero && n >= 7) ok = ok && !equal;
  std::printf("P %-5d n %-5d add %d det %d  %-20s row %-5zu NaN %-5d %s\n", P, n, add, det, kNames[kind], out.size(), nans,
              ok ? "ok" : "FAILED");
  fails += !ok;
}

}  // namespace

int main() {
  Spec sp;
  const bool refusals = make_spec(1, 0, 4, 0, 1e-5f, 0, sp) && make_spec(1, 1023, 4, 0, 1e-5f, 0, sp) && make_spec(1, 6, 0, 0, 1e-5f, 0, sp) &&
                        make_spec(1, 6, 1025, 0, 1e-5f, 0, sp) && make_spec(1, 6, 4, 0, 0.f, 0, sp) &&
                        make_spec(1, 6, 4, 0, std::numeric_limits<float>::infinity(), 0, sp) && make_spec(-1, 6, 4, 0, 1e-5f, 0, sp) &&
                        make_spec((1ll << 28) + 1, 6, 4, 0, 1e-5f, 0, sp) && !make_spec(0, 1, 1, 0, 1e-5f, 0, sp);
  std::printf("make_spec refuses what the header says               %s\n", refusals ? "ok" : "FAILED");
  fails += !refusals;
  const int Ps[] = {3, 4, 5, 64, 257, 1024};
  for (int P : Ps) {
    const int ns[] = {1, 7, P, 1024};
    for (int n : ns)
      for (int add = 0; add < 2; ++add)
        for (int det = 0; det < 2; ++det) run(P, n, add, det, kRandom);
  }
  for (int kind = kZero; kind < kKinds; ++kind)
    for (int P : {3, 5, 64})
      for (int det = 0; det < 2; ++det) run(P, P == 3 ? 1 : 2 * P, 1, det, (Kind)kind);
  std::printf("%s\n", fails ? "FAILED" : "all hold");
  return fails ? 1 : 0;
}
