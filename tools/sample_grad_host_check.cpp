// sample_grad_host_check.cpp — csrc/sample_grad.hpp (over csrc/rays.hpp) as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/sample_grad_host_check.cpp -o sample_grad_host_check && ./sample_grad_host_check
// Drives backward_host, and the device's route restated on the host (sorted_list_host: the stable radix sort over the
// pixel's digits; sum_segments_host: the chains over the segments), with arrays of exactly the sizes the header asks for, and
// checks that the two give the same bits, that the sorted list is the order of the key (pixel << 32) | r, that pixels
// without a ray hold +0, and that check_shape refuses what include/isr_sample_grad.h says it refuses.  The cases are the
// tests' edge cases: n = 1, every ray on one pixel (n = 2, 64, 65, 4 097), every ray on its own pixel, rays outside on each
// side, NaN and infinite coordinates, half-integer positions, W = 1, H = 1, C = 1, 12, 13, 65, a middle image that keeps
// nothing, dout of zeros, of -0 and with a NaN and an infinity, and images past one and two radix digits.  Prints one line
// per case; exit status 0 = all hold.  The log of one such run is profiles/sample_grad_host_sanitizers.txt.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/sample_grad.hpp"

using namespace isr::sample_grad;

namespace {

unsigned seed = 13579u;
float uni() {                                        // U(-1, 1)
  seed = seed * 1664525u + 1013904223u;
  return (float)((seed >> 8) & 0xffff) / 32768.f - 1.f;
}

int fails = 0;

// xy kinds: 0 random in +-1.1, 1 every ray at the centre, 2 ray r on pixel r (n = H W), 3 image 1 outside
void run(const char* what, int B, int H, int W, int C, int n, int xy_kind, int dout_kind) {
  const size_t N = (size_t)B * n, HW = (size_t)H * W;
  std::vector<float> dout(N * C), xys(N * 2), a(B * HW * C, 7.f), b(B * HW * C, 0.f);
  for (auto& v : dout) v = dout_kind == 1 ? 0.f : dout_kind == 2 ? -0.f : uni();
  if (dout_kind == 3) {
    dout[dout.size() / 3] = std::numeric_limits<float>::quiet_NaN();
    dout[dout.size() / 2] = std::numeric_limits<float>::infinity();
  }
  for (size_t i = 0; i < N; ++i) {
    const int r = (int)(i % n), img = (int)(i / n);
    float x = 1.1f * uni(), y = 1.1f * uni();
    if (xy_kind == 1) x = y = 0.f;
    if (xy_kind == 2) {
      x = W > 1 ? -(2.f * (float)(r % W) / (float)(W - 1) - 1.f) : 0.f;
      y = H > 1 ? -(2.f * (float)(r / W) / (float)(H - 1) - 1.f) : 0.f;
    }
    if (xy_kind == 3 && img == 1) x = 1.5f;
    if (xy_kind == 4) {                              // each side, NaN, infinities, exact halves on 5 pixels
      const float xs[] = {1.5f, -1.5f, 0.f, 0.f, NAN, 0.f, INFINITY, 0.f, 0.75f, 0.25f, -0.25f, -0.75f};
      const float ys[] = {0.f, 0.f, 1.5f, -1.5f, 0.f, NAN, 0.f, -INFINITY, 0.25f, -0.25f, 0.75f, -0.75f};
      x = xs[r % 12];
      y = ys[r % 12];
    }
    xys[2 * i] = x;
    xys[2 * i + 1] = y;
  }
  bool ok = check_shape(B, H, W, C, n) == nullptr;
  backward_host(dout.data(), B, H, W, C, xys.data(), n, a.data());
  size_t kept = 0;
  std::vector<uint32_t> pix((size_t)n), ray((size_t)n);
  std::vector<char> hit(HW);
  for (int img = 0; img < B; ++img) {
    sorted_list_host(xys.data(), img, H, W, n, pix.data(), ray.data());
    for (int k = 0; k < n; ++k) {
      ok = ok && ray[k] < (uint32_t)n && pix[k] == ray_pixel(xys.data(), (size_t)img * n + ray[k], H, W);
      if (k > 0) ok = ok && (((uint64_t)pix[k - 1] << 32) | ray[k - 1]) < (((uint64_t)pix[k] << 32) | ray[k]);
      kept += pix[k] != HW;
    }
    sum_segments_host(dout.data(), img, H, W, C, n, pix.data(), ray.data(), b.data());
    std::fill(hit.begin(), hit.end(), 0);
    for (int k = 0; k < n; ++k)
      if (pix[k] != HW) hit[pix[k]] = 1;
    for (size_t p = 0; p < HW; ++p)
      for (int c = 0; c < C && !hit[p]; ++c) {
        uint32_t bits;
        std::memcpy(&bits, &a[((size_t)img * HW + p) * C + c], 4);
        ok = ok && bits == 0;                        // +0, not -0
      }
  }
  for (size_t i = 0; i < a.size(); ++i) {
    uint32_t u, v;
    std::memcpy(&u, &a[i], 4);
    std::memcpy(&v, &b[i], 4);
    ok = ok && (u == v || (std::isnan(a[i]) && std::isnan(b[i])));
  }
  std::printf("%-58s rays %-6zu kept %-6zu passes %d  %s\n", what, N, kept, radix_passes(H, W), ok ? "ok" : "FAILED");
  fails += !ok;
}

}  // namespace

int main() {
  run("n = 1", 2, 4, 5, 3, 1, 0, 0);
  for (int n : {2, 64, 65, 4097}) run("every ray on one pixel", 2, 5, 7, 3, n, 1, 0);
  run("every ray on its own pixel, 3 x 5", 1, 3, 5, 2, 15, 2, 0);
  run("outside on each side, NaN, infinities, exact halves", 1, 5, 5, 2, 36, 4, 0);
  run("W = 1", 2, 6, 1, 2, 40, 0, 0);
  run("H = 1", 2, 1, 6, 2, 40, 0, 0);
  run("H = W = 1", 1, 1, 1, 2, 9, 0, 0);
  for (int C : {1, 12, 13, 65}) run("channels", 2, 6, 7, C, 100, 0, 0);
  run("B = 3, the middle image keeps nothing", 3, 5, 6, 4, 50, 3, 0);
  run("dout of zeros", 2, 4, 4, 3, 60, 0, 1);
  run("dout of -0", 2, 4, 4, 3, 60, 0, 2);
  run("dout with a NaN and an infinity", 2, 4, 4, 3, 60, 0, 3);
  run("3 x 100 pixels (two digits)", 2, 3, 100, 1, 5000, 0, 0);
  run("300 x 300 pixels (three digits)", 2, 300, 300, 1, 5000, 0, 0);
  run("224 x 224, every ray on its own pixel", 1, 224, 224, 1, 224 * 224, 2, 0);
  bool refused = check_shape(0, 4, 4, 3, 5) && check_shape(2, 0, 4, 3, 5) && check_shape(2, 4, 0, 3, 5) && check_shape(2, 4, 4, 0, 5) &&
                 check_shape(2, 4, 4, 4097, 5) && check_shape(2, 4, 4, 3, 0) && check_shape(2, 4, 4, 3, (1 << 27) + 1) &&
                 check_shape(2, 4, 4, 4096, 1 << 18) && check_shape(1, 1 << 16, 1 << 15, 3, 5) &&
                 check_shape(1 << 12, 1 << 14, 1 << 14, 1, 5) && check_shape(1, 1 << 14, 1 << 14, 4096, 5) &&
                 !check_shape(16, 224, 224, 12, 1024) && radix_passes(224, 224) == 2 && radix_passes(1, 255) == 1 &&
                 radix_passes(1, 256) == 2 && radix_passes(300, 300) == 3 && radix_passes(1, 1) == 1;
  std::printf("%-58s %s\n", "shapes out of range are refused; digit passes", refused ? "ok" : "FAILED");
  fails += !refused;
  std::printf(fails ? "%d cases FAILED\n" : "all cases hold\n", fails);
  return fails != 0;
}
