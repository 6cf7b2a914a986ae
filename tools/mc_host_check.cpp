// mc_host_check.cpp — csrc/mc_extract.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/mc_host_check.cpp -o mc_host_check && ./mc_host_check
// Runs mc::count_host and mc::emit_host into buffers of exactly the counted sizes (ASan guards both ends) over: the smallest
// volume, unequal dimensions with uniform noise (nearly every edge crosses), the volume of all 256 corner patterns, a ball,
// all-below and all-above volumes, values equal to iso, and a volume holding NaN and infinities.  Checks per case that every
// vertex lies on a grid edge inside the volume, every triangle names three distinct vertices below V, every vertex is used,
// and — where the surface does not leave the volume — that every directed triangle edge occurs once and its reverse once.
// Prints one line per case; exit status 0 = all hold.  The log of one such run is profiles/mc_host_sanitizers.txt.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <utility>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/mc_extract.hpp"

namespace {

struct Lcg {
  unsigned s;
  float next() {                       // U[0, 1)
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) / 16777216.f;
  }
};

// closed: the surface must be a closed manifold; finite: every coordinate must be finite and inside the volume
int check(const char* name, const std::vector<float>& vol, int nx, int ny, int nz, float iso, bool closed, bool finite) {
  using namespace isr::mc;
  std::vector<int32_t> first((size_t)nx * ny * nz);
  int64_t V, F;
  count_host(vol.data(), nx, ny, nz, iso, first.data(), V, F);
  std::vector<double> verts(3 * (size_t)V);
  std::vector<int32_t> tris(3 * (size_t)F);
  emit_host(vol.data(), nx, ny, nz, iso, first.data(), verts.data(), tris.data());
  int bad = 0;
  const int dims[3] = {nx, ny, nz};
  for (int64_t v = 0; v < V && finite; ++v) {
    int whole = 0;
    for (int c = 0; c < 3; ++c) {
      const double x = verts[3 * v + c];
      if (!(x >= 0 && x <= dims[c] - 1)) ++bad;
      whole += x == std::floor(x);
    }
    if (whole < 2) ++bad;              // on a grid edge: at most one coordinate is fractional
  }
  std::vector<char> used((size_t)V, 0);
  std::set<std::pair<int32_t, int32_t>> edges;
  for (int64_t f = 0; f < F; ++f) {
    const int32_t* t = &tris[3 * f];
    for (int n = 0; n < 3; ++n) {
      if (t[n] < 0 || t[n] >= V) {
        ++bad;
        continue;
      }
      used[t[n]] = 1;
      if (!edges.insert({t[n], t[(n + 1) % 3]}).second) ++bad;      // a directed edge twice
    }
    if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) ++bad;
  }
  for (int64_t v = 0; v < V; ++v)
    if (!used[v]) ++bad;
  if (closed)
    for (const auto& e : edges)
      if (!edges.count({e.second, e.first})) ++bad;
  std::printf("%-34s %3d x %3d x %3d  V %6lld  F %6lld: %s\n", name, nx, ny, nz, (long long)V, (long long)F, bad ? "MISMATCH" : "ok");
  return bad;
}

std::vector<float> noise(int n, unsigned seed) {
  Lcg g{seed};
  std::vector<float> v((size_t)n);
  for (float& x : v) x = g.next();
  return v;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check("smallest", noise(8, 1u), 2, 2, 2, 0.5f, false, true);
  bad += check("noise, unequal dimensions", noise(17 * 13 * 9, 2u), 17, 13, 9, 0.5f, false, true);
  bad += check("noise, a flat volume", noise(2 * 40 * 3, 3u), 2, 40, 3, 0.5f, false, true);
  {
    // the 256 corner patterns as 2 x 2 x 2 blocks, every other point below
    const int nx = 34, ny = 34, nz = 4;
    Lcg g{4u};
    std::vector<float> v((size_t)nx * ny * nz);
    for (float& x : v) x = 0.3f - (0.1f + 0.9f * g.next());
    for (int c = 0; c < 256; ++c)
      for (int b = 0; b < 8; ++b)
        if (!(c >> b & 1)) {
          float& x = v[((size_t)(1 + 2 * (c % 16) + (b & 1)) * ny + 1 + 2 * (c / 16) + (b >> 1 & 1)) * nz + 1 + (b >> 2 & 1)];
          x = 0.6f - x;                // mirrored to the above side
        }
    bad += check("all 256 corner patterns", v, nx, ny, nz, 0.3f, true, true);
  }
  {
    const int n = 24;
    std::vector<float> v((size_t)n * n * n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k)
          v[((size_t)i * n + j) * n + k] = 64.f - ((i - 11.3f) * (i - 11.3f) + (j - 12.1f) * (j - 12.1f) + (k - 11.7f) * (k - 11.7f));
    bad += check("ball", v, n, n, n, 0.f, true, true);
  }
  bad += check("all below", noise(5 * 4 * 3, 5u), 5, 4, 3, 2.f, true, true);
  bad += check("all above", noise(5 * 4 * 3, 5u), 5, 4, 3, -1.f, true, true);
  {
    std::vector<float> v(27, -1.f);
    v[13] = 0.25f;                     // the centre equal to iso: six vertices at one position
    bad += check("a value equal to iso", v, 3, 3, 3, 0.25f, true, true);
  }
  {
    std::vector<float> v = noise(6 * 5 * 7, 6u);
    v[17] = std::numeric_limits<float>::quiet_NaN();
    v[60] = std::numeric_limits<float>::infinity();
    v[61] = -std::numeric_limits<float>::infinity();
    v[100] = std::numeric_limits<float>::quiet_NaN();
    v[101] = std::numeric_limits<float>::quiet_NaN();
    bad += check("NaN and infinities", v, 6, 5, 7, 0.5f, false, false);
  }
  std::printf("%s\n", bad ? "FAILED" : "all cases hold");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
