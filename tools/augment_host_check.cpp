// augment_host_check.cpp — csrc/augment.hpp as plain host code, for a sanitizer build:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/augment_host_check.cpp -o augment_host_check && ./augment_host_check
// Drives images_host_one and rays_host_one over the shapes of the tests — frames 1x1, 2x3, 5x8, 16x16 and 224x224, shifts that
// empty the frame or exceed it, rectangles at a corner, across the edge, empty and covering everything, border kernels up to
// 19x19 on a 5x8 frame, NaN and infinity in the colours, affine matrices that throw the source position to +-1e300; views of
// 0, 1, S-1, S, S+1 and 4 097 rows with inside counts 0, 1 and S+-1 — with arrays of exactly the sizes the header asks for, and
// checks what can be checked without a second implementation: masks stay 0/1, the clip between the two warps, the paste,
// distinct candidate rows in key order, the zeros past the count.  Prints one line per case; exit status 0 = all hold.  The
// log of one such run is profiles/augment_host_sanitizers.txt.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imagesequenceregistrationfor6dposeestimationlabeling_amd/csrc/augment.hpp"

using namespace isr::augment;

namespace {

unsigned seed = 4321u;
float rnd() {      // in [-1, 1)
  seed = seed * 1664525u + 1013904223u;
  return (float)((seed >> 8) & 0xffff) / 32768.f - 1.f;
}

int check_images(const char* name, int H, int W, const double* M, int tx, int ty, int t1x, int t1y, int rx, int ry, int rw, int rh,
                 int kh, int kw, bool canvas_on, int special) {
  const Frame f{H, W};
  const size_t n = (size_t)H * W;
  std::vector<float> rgb(3 * n), canvas(3 * n), out(3 * n), mo(n), mk(n);
  std::vector<uint8_t> mask(n), orig(n);
  for (size_t i = 0; i < 3 * n; ++i) {
    rgb[i] = 0.5f + 0.5f * rnd();
    canvas[i] = 2.f + rnd();
  }
  for (size_t i = 0; i < n; ++i) {
    mask[i] = special == 2 ? 1 : rnd() > -0.5f;
    orig[i] = rnd() > -0.5f;
  }
  if (special == 1) {
    rgb[0] = NAN;
    rgb[3 * n - 1] = INFINITY;
    rgb[3 * (n / 2)] = -INFINITY;
  }
  const int32_t rect[4] = {rx, ry, rw, rh}, tra[2] = {tx, ty}, tra1[2] = {t1x, t1y}, border[2] = {kh, kw};
  const float mu[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  ImageBatch ib;
  const char* wrong = make_image_batch(0, 1, rect, M, tra, tra1, border, mu, sd, ib);
  if (wrong) {
    std::printf("%-64s refused: %s\n", name, wrong);
    return 1;
  }
  images_host_one(rgb.data(), mask.data(), orig.data(), canvas_on ? canvas.data() : nullptr, f, ib.p[0], ib.mu, ib.sd, out.data(),
                  mo.data(), mk.data());
  int bad = 0;
  size_t pasted = 0;
  for (size_t i = 0; i < n; ++i) {
    bad += !(mk[i] == 0.f || mk[i] == 1.f) || !(mo[i] == 0.f || mo[i] == 1.f);
    pasted += mk[i] == 1.f;
    const int x = (int)(i % W), y = (int)(i / W);
    const bool blank = kh > 0 && kw > 0 && border_blank(mk.data(), f, kh, kw, x, y);
    if (mk[i] != 1.f)      // the canvas (or zero), normalised, wherever the mask did not paste
      for (int c = 0; c < 3; ++c) bad += out[3 * i + c] != normalize1(blank || !canvas_on ? 0.f : canvas[3 * i + c], mu[c], sd[c]);
    else if (special != 1)
      for (int c = 0; c < 3; ++c) bad += !(out[3 * i + c] == out[3 * i + c]);
  }
  if (special == 2) bad += pasted != 0;      // the case built to be emptied by the clip
  std::printf("%-64s %dx%d pasted %-6zu %s\n", name, H, W, pasted, bad ? "MISMATCH" : "ok");
  return bad;
}

int check_rays(const char* name, int n, int m_inside, int S, const float* rot, const float* t, uint32_t view, int set) {
  std::vector<float> xy(2 * (size_t)n + 2), pos(3 * (size_t)n + 3);
  for (int i = 0; i < n; ++i) {
    xy[2 * i] = 0.9f * rnd();
    xy[2 * i + 1] = 0.9f * rnd();
    if (i >= m_inside) xy[2 * i + (i & 1)] = (i & 2) ? 1.0f : -1.5f;
    for (int a = 0; a < 3; ++a) pos[3 * i + a] = (float)(3 * i + a);
  }
  RayBatch rb{};
  rb.start[set][0] = 0;
  rb.n[set][0] = n;
  rb.view[0] = (int)view;
  for (int a = 0; a < 4; ++a) rb.m[0][a] = rot[a];
  rb.t[0][0] = t[0];
  rb.t[0][1] = t[1];
  std::vector<float> xo(2 * (size_t)S), po(3 * (size_t)S);
  std::vector<int32_t> idx(S), count(1);
  const RaySet in{xy.data(), pos.data()};
  const RayOut out{xo.data(), po.data(), idx.data(), count.data()};
  rays_host_one(in, rb, 0, set, S, 77u, 5u, out, 0);
  int bad = 0;
  const int K = count[0];
  bad += K < 0 || K > S || K > n;
  uint64_t last = 0;
  std::vector<char> seen(n + 1, 0);
  for (int r = 0; r < S; ++r) {
    if (r < K) {
      const int i = idx[r];
      if (i < 0 || i >= n) {
        ++bad;
        continue;
      }
      bad += seen[i]++;
      const uint64_t key = ((uint64_t)key_word((uint32_t)i, view, (uint32_t)set, 77u, 5u) << 32) | (uint32_t)i;
      bad += r > 0 && key <= last;
      last = key;
      bad += po[3 * r] != (float)(3 * i);
      float sx, sy;
      remap(rot, t, xy[2 * i], xy[2 * i + 1], sx, sy);
      bad += std::memcmp(&sx, &xo[2 * r], 4) != 0 || std::memcmp(&sy, &xo[2 * r + 1], 4) != 0;
    } else {
      bad += idx[r] != -1 || xo[2 * r] != 0.f || xo[2 * r + 1] != 0.f || po[3 * r] != 0.f || po[3 * r + 1] != 0.f || po[3 * r + 2] != 0.f;
    }
  }
  std::printf("%-64s n %-5d S %-5d count %-5d %s\n", name, n, S, K, bad ? "MISMATCH" : "ok");
  return bad;
}

void rotation(double cx, double cy, double deg, double scale, double* M) {
  const double ang = deg * 3.14159265358979323846 / 180.0, a = scale * std::cos(ang), b = scale * std::sin(ang);
  M[0] = a; M[1] = b; M[2] = (1 - a) * cx - b * cy;
  M[3] = -b; M[4] = a; M[5] = b * cx + (1 - a) * cy;
}

}  // namespace

int main() {
  int bad = 0;
  double M[6];
  const int sizes[5][2] = {{1, 1}, {2, 3}, {5, 8}, {16, 16}, {224, 224}};
  const double rots[4] = {0, 90, 37, 271}, scales[3] = {0.5, 1.0, 1.137};
  int k = 0;
  for (const auto& hw : sizes)
    for (double rot : rots) {
      const int H = hw[0], W = hw[1];
      rotation((W - 1) / 2.0, (H - 1) / 2.0, rot, scales[k % 3], M);
      char name[96];
      std::snprintf(name, sizeof name, "rot %g scale %g, rectangle and border kind %d", rot, scales[k % 3], k % 4);
      const int rect[4][4] = {{0, 0, 2, 2}, {W - 1, H - 1, 3, 3}, {1, 1, 0, 5}, {-2, -2, W + 4, H + 4}};
      const int kern[4][2] = {{0, 0}, {1, 1}, {2, 3}, {19, 19}};
      bad += check_images(name, H, W, M, k % 3 - 1, 1 - k % 3, (k + 1) % 3 - 1, 0, rect[k % 4][0], rect[k % 4][1], rect[k % 4][2],
                          rect[k % 4][3], kern[k % 4][0], kern[k % 4][1], k % 2 == 0, 0);
      ++k;
    }
  rotation(3.5, 2.0, 0, 1.0, M);
  bad += check_images("a shift that empties the frame", 5, 8, M, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, true, 0);
  bad += check_images("tra - tra1 larger than the frame", 5, 8, M, 20, -13, -1, 1, 0, 0, 0, 0, 3, 3, false, 0);
  bad += check_images("the clip between the two warps empties an all-ones mask", 5, 8, M, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, true, 2);
  bad += check_images("shifts at the limit 2^24", 5, 8, M, kMaxShift, -kMaxShift, -kMaxShift, kMaxShift, 0, 0, 0, 0, 2, 2, true, 0);
  bad += check_images("a 19 x 19 kernel on a 5 x 8 frame", 5, 8, M, 0, 0, 0, 0, 2, 1, 3, 2, 19, 19, true, 0);
  bad += check_images("a 255 x 255 kernel on a 16 x 16 frame", 16, 16, M, 0, 0, 0, 0, 0, 0, 0, 0, 255, 255, false, 0);
  rotation(3.5, 2.0, 37, 1.137, M);
  bad += check_images("NaN and infinity in the colours", 5, 8, M, 1, 0, 0, 1, 0, 0, 0, 0, 2, 3, true, 1);
  const double tiny[6] = {1e-150, 0, 0, 0, 1e-150, 0}, far[6] = {1, 0, 1e300, 0, 1, -1e300};
  bad += check_images("a source position beyond every integer (scale 1e-150)", 5, 8, tiny, 1, 1, 0, 0, 0, 0, 0, 0, 2, 2, true, 0);
  bad += check_images("a translation of 1e300", 5, 8, far, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, true, 0);

  ImageBatch ib;
  const double singular[6] = {1, 2, 0, 2, 4, 0}, nan_m[6] = {NAN, 0, 0, 0, 1, 0};
  const float mu[3] = {0, 0, 0}, sd[3] = {1, 1, 1}, sd0[3] = {1, 0, 1};
  const int32_t big[2] = {kMaxShift + 1, 0}, neg_rect[4] = {0, 0, -1, 1}, kern[2] = {256, 1};
  rotation(0, 0, 0, 1, M);
  int refused = 0;
  refused += make_image_batch(0, 1, nullptr, singular, nullptr, nullptr, nullptr, mu, sd, ib) != nullptr;
  refused += make_image_batch(0, 1, nullptr, nan_m, nullptr, nullptr, nullptr, mu, sd, ib) != nullptr;
  refused += make_image_batch(0, 1, nullptr, M, nullptr, nullptr, nullptr, mu, sd0, ib) != nullptr;
  refused += make_image_batch(0, 1, nullptr, M, big, nullptr, nullptr, mu, sd, ib) != nullptr;
  refused += make_image_batch(0, 1, neg_rect, M, nullptr, nullptr, nullptr, mu, sd, ib) != nullptr;
  refused += make_image_batch(0, 1, nullptr, M, nullptr, nullptr, kern, mu, sd, ib) != nullptr;
  refused += make_image_batch(0, 1, nullptr, M, nullptr, nullptr, nullptr, mu, sd, ib) == nullptr;
  std::printf("%-64s %s\n", "image arguments out of range are refused", refused == 7 ? "ok" : "MISMATCH");
  bad += refused != 7;

  const float ident[4] = {1, 0, 0, 1}, zero[2] = {0, 0}, warp[4] = {0.9f, 0.4f, -0.4f, 0.9f}, shift[2] = {0.25f, -0.125f};
  const int S = 8;
  for (int n : {0, 1, S - 1, S, S + 1, 4097}) {
    char name[96];
    std::snprintf(name, sizeof name, "every row inside, n = %d", n);
    bad += check_rays(name, n, n, S, ident, zero, 3, 0);
  }
  for (int m : {0, 1, S - 1, S + 1}) {
    char name[96];
    std::snprintf(name, sizeof name, "20 rows, %d inside", m);
    bad += check_rays(name, 20, m, S, ident, zero, 4, 1);
  }
  bad += check_rays("4 097 rows, 2 000 inside before the remap, S = 4 096", 4097, 2000, 4096, warp, shift, 0xffffffffu, 1);
  bad += check_rays("4 097 rows, all inside, S = 4 096", 4097, 4097, 4096, ident, zero, 0, 0);
  bad += check_rays("S = 1", 300, 100, 1, warp, shift, 9, 0);

  RayBatch rb;
  const int64_t off_ok[3] = {0, 5, 9}, off_big[3] = {0, 5, 5 + (int64_t)kMaxViewRows + 1}, off_down[3] = {0, 5, 4};
  const int32_t ids01[2] = {0, 1}, ids2[1] = {2};
  const float rot2[8] = {1, 0, 0, 1, 1, 0, 0, 1}, t2[4] = {0, 0, 0, 0};
  const int64_t* one[2] = {off_ok, nullptr};
  const int64_t* two_big[2] = {off_ok, off_big};
  const int64_t* down[2] = {off_down, nullptr};
  refused = 0;
  refused += make_ray_batch(0, 2, one, 2, ids01, rot2, t2, rb) == nullptr;
  refused += make_ray_batch(0, 1, one, 2, ids2, rot2, t2, rb) != nullptr;
  refused += make_ray_batch(0, 2, two_big, 2, ids01, rot2, t2, rb) != nullptr;
  refused += make_ray_batch(0, 2, down, 2, ids01, rot2, t2, rb) != nullptr;
  std::printf("%-64s %s\n", "ray arguments out of range are refused", refused == 4 ? "ok" : "MISMATCH");
  bad += refused != 4;
  std::printf("%s\n", bad ? "FAILED" : "all cases hold");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
