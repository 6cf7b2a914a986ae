// radius_host_check.cpp — csrc/radius_count.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/radius_host_check.cpp -o radius_host_check && ./radius_host_check
// Counts clouds through count_host — one point, two points at exactly the radius, coincident points, clusters, two clusters
// so far apart that the cell edge has to grow, a box of no extent, huge and tiny coordinates, every cap — with scratch
// arrays of exactly the sizes the header asks for, and compares with the count over every pair.  Prints one line per case;
// exit status 0 = all hold.  The log of one such run is profiles/radius_host_sanitizers.txt.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/radius_count.hpp"

using namespace isr::radius;

namespace {

unsigned seed = 12345u;
float rnd() {
  seed = seed * 1664525u + 1013904223u;
  return (float)((seed >> 8) & 0xffff) / 32768.f - 1.f;
}

int check(const char* name, const std::vector<float>& pts, float r) {
  const int N = (int)(pts.size() / 3);
  int bad = 0;
  for (int cap : {0, 1, 21}) {
    std::vector<int32_t> counts(N), start(kMaxCells), end(kMaxCells);
    std::vector<float> sorted(3 * (size_t)N);
    count_host(pts.data(), N, r, cap, counts.data(), sorted.data(), start.data(), end.data());
    const float r2 = r * r;
    for (int i = 0; i < N; ++i) {
      int c = 0;
      for (int j = 0; j < N; ++j)
        if (dist2(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) <= r2) ++c;
      if (cap > 0 && c > cap) c = cap;
      if (counts[i] != c) ++bad;
    }
  }
  std::printf("%-52s N %-6d %s\n", name, N, bad ? "MISMATCH" : "ok");
  return bad;
}

std::vector<float> cluster(int n, float cx, float cy, float cz, float spread) {
  std::vector<float> p;
  for (int i = 0; i < n; ++i) {
    p.push_back(cx + spread * rnd());
    p.push_back(cy + spread * rnd());
    p.push_back(cz + spread * rnd());
  }
  return p;
}

void append(std::vector<float>& a, const std::vector<float>& b) { a.insert(a.end(), b.begin(), b.end()); }

}  // namespace

int main() {
  int bad = 0;
  bad += check("one point", {0.25f, -1.f, 3.f}, 0.05f);
  bad += check("two points at exactly r (d2 == r2)", {2, 3, 4, 3, 3, 4}, 1.f);
  bad += check("33 coincident points", cluster(33, 0.1f, 0.2f, 0.3f, 0.f), 0.05f);
  std::vector<float> three = cluster(400, 0, 0, 0, 0.1f);
  append(three, cluster(350, 0.3f, 0.1f, -0.2f, 0.1f));
  append(three, cluster(250, -0.4f, 0.5f, 0.2f, 0.1f));
  bad += check("three clusters", three, 0.05f);
  append(three, std::vector<float>(three.begin(), three.begin() + 60));
  bad += check("three clusters with duplicates", three, 0.05f);
  std::vector<float> far = cluster(60, 0, 0, 0, 0.04f);
  append(far, cluster(60, 1000.f, 1000.f, 1000.f, 0.04f));
  bad += check("two clusters 1000 apart, r = 0.01 (h grows)", far, 0.01f);
  std::vector<float> huge = cluster(50, 0, 0, 0, 1.f);
  for (auto& v : huge) v *= 3.0e38f;
  bad += check("coordinates near the largest f32", huge, 1.0e19f);
  std::vector<float> tiny = cluster(50, 0, 0, 0, 1.f);
  for (auto& v : tiny) v *= 1.0e-18f;
  bad += check("r near the smallest accepted", tiny, 1.1e-19f);
  std::vector<float> line = cluster(300, 0, 0, 0, 1.f);
  for (size_t i = 0; i < line.size(); i += 3) line[i + 1] = line[i + 2] = 0.5f;
  bad += check("points on a line (two axes without extent)", line, 0.01f);
  Grid g;
  const float mn[3] = {0, 0, 0}, inf[3] = {INFINITY, 1, 1}, nan[3] = {NAN, 1, 1};
  make_grid(mn, inf, 0.1f, g);
  int one = g.cells == 1;
  make_grid(mn, nan, 0.1f, g);
  one += g.cells == 1;
  one += cell_coord(NAN, 0.0, 1.0, 5) == 0 && cell_coord(INFINITY, 0.0, 1.0, 5) == 4 && cell_coord(-INFINITY, 0.0, 1.0, 5) == 0;
  std::printf("%-52s %s\n", "a box that is no box is one cell; NaN has cell 0", one == 3 ? "ok" : "MISMATCH");
  bad += one != 3;
  std::printf("%s\n", bad ? "FAILED" : "all cases hold");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
