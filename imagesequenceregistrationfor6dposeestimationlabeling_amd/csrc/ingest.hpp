// ingest.hpp — sequence ingest: the arithmetic of include/isr_ingest.h (which states every rule), written once and compiled
// for host and device.  csrc/ingest.hip holds the kernels and the C entries; a plain C++ compiler can include this header too
// (tools/ingest_host_check.cpp).  Integers for the box and the canvas, f64 for the resize and the camera, one f32 division at
// the end, and everything is built with -ffp-contract=off: host and device give the same bits.
//
// What this replaces: cowrendersynth.py:667-736, the body of generate_bop_realsamples' loop over frames.
//
// THE SILHOUETTE HAS TWO MODES because the reference's call and its wording disagree.  It writes
//     cv2.resize(squareRGB1, (maxB, maxB), cv2.INTER_CUBIC)  and  cv2.resize(squareMask1, (maxB, maxB), cv2.INTER_NEAREST),
// the flag as the third positional argument.  OpenCV's signature is resize(src, dsize[, dst[, fx[, fy[, interpolation]]]]), so
// that slot is dst and both calls run the default INTER_LINEAR.  This is stated FROM MEMORY — cv2 is not available to this
// project — and is UNPINNED.  kSilLinear (the default) is what the call does; kSilNearest is what it says.  The bilinear rule
// here is the textbook one (csrc/crop_normalize.hip's sample_u8 order, edge replication): an owned definition.  cv2's 8-bit
// resize is fixed-point and can differ by a grey level.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace ingest {

constexpr int kSilLinear = 0, kSilNearest = 1;
constexpr int kThreads = 256;                  // every launch
constexpr int kFrameGroup = 64;                // frames on blockIdx.z; groups of them on blockIdx.y
constexpr int kMaxGroups = 65535;
constexpr long long kMaxPixels = 1ll << 28;    // H * W
constexpr int kMaxB = 4096;
constexpr int kMaxOffset = 4096;
constexpr int kStripBytes = 1 << 16;           // a strip's mask bytes: 16 chunks of 16 bytes per lane
constexpr int kMaxStripRows = 64;
constexpr int kChunk = 16;

struct Frame {
  const uint8_t* rgb;     // (H, W, 3)
  const uint8_t* mask;    // (H, W, Cm)
  int H, W, Cm;
};

struct Geom {
  int x2, y2, w2, h2, hw, hh, side, hs1;
};

// A partial box: the extremes of the non-zero pixels seen so far; x1 < 0 while there are none.
struct Box {
  int x0, y0, x1, y1;
};

ISR_HD Box empty_box(int H, int W) { return Box{W, H, -1, -1}; }

ISR_HD void box_add(Box& b, int x, int y) {
  b.x0 = x < b.x0 ? x : b.x0;
  b.x1 = x > b.x1 ? x : b.x1;
  b.y0 = y < b.y0 ? y : b.y0;
  b.y1 = y > b.y1 ? y : b.y1;
}

ISR_HD void box_merge(Box& b, const Box& o) {
  b.x0 = o.x0 < b.x0 ? o.x0 : b.x0;
  b.x1 = o.x1 > b.x1 ? o.x1 : b.x1;
  b.y0 = o.y0 < b.y0 ? o.y0 : b.y0;
  b.y1 = o.y1 > b.y1 ? o.y1 : b.y1;
}

// rows per strip and strips per frame of the box pass
ISR_HD int strip_rows(int H, int W, int Cm) {
  const long long row_bytes = (long long)W * Cm;
  long long r = kStripBytes / row_bytes;
  r = r < 1 ? 1 : r;
  r = r > kMaxStripRows ? kMaxStripRows : r;
  return (int)(r > H ? H : r);
}
ISR_HD int strips_of(int H, int W, int Cm) {
  const int r = strip_rows(H, W, Cm);
  return (H + r - 1) / r;
}

// One mask byte at byte offset `off` of its frame (off < 3 * 2^28): channel 0 of pixel (off % row_bytes) / Cm when Cm divides.
ISR_HD void box_byte(Box& b, uint32_t off, uint8_t v, uint32_t row_bytes, int Cm) {
  if (!v) return;
  const uint32_t y = off / row_bytes, o = off - y * row_bytes;
  if (Cm == 3 && o % 3u) return;
  box_add(b, (int)(o / (uint32_t)Cm), (int)y);
}

// Sixteen mask bytes, as four little-endian words, at byte offset `off` of their frame.
ISR_HD void box_chunk(Box& b, uint32_t off, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t row_bytes,
                             int Cm) {
  if (!(w0 | w1 | w2 | w3)) return;
  const uint32_t w[4] = {w0, w1, w2, w3};
  uint32_t m = 0;      // bit i: byte i is non-zero
#pragma unroll
  for (int i = 0; i < 16; ++i) m |= (((w[i >> 2] >> (8 * (i & 3))) & 255u) ? 1u : 0u) << i;
  if (Cm == 3) {       // keep channel 0: the bytes whose offset in the row is a multiple of 3 (row_bytes is one too)
    const uint32_t first = (3u - off % 3u) % 3u;
    m &= first == 0 ? 0x9249u : first == 1 ? 0x2492u : 0x4924u;
  }
  if (!m) return;
  const uint32_t lo = off + (uint32_t)__builtin_ctz(m), hi = off + (31u - (uint32_t)__builtin_clz(m));
  const uint32_t ylo = lo / row_bytes, yhi = hi / row_bytes;
  if (ylo == yhi) {    // one row: its first and last non-zero pixel bound the others
    box_add(b, (int)((lo - ylo * row_bytes) / (uint32_t)Cm), (int)ylo);
    box_add(b, (int)((hi - ylo * row_bytes) / (uint32_t)Cm), (int)ylo);
    return;
  }
  for (int i = 0; i < 16; ++i)
    if ((m >> i) & 1u) {
      const uint32_t o = off + (uint32_t)i, y = o / row_bytes;
      box_add(b, (int)((o - y * row_bytes) / (uint32_t)Cm), (int)y);
    }
}

// cowrendersynth.py:668-690: the box (x, y, w, h) = cv2.boundingRect -> the even cut, the square side and its half
ISR_HD Geom make_geom(const Box& b, int offset) {
  const bool any = b.x1 >= 0;
  Geom g;
  g.x2 = any ? b.x0 : 0;
  g.y2 = any ? b.y0 : 0;
  int w2 = any ? b.x1 - b.x0 + 1 : 0, h2 = any ? b.y1 - b.y0 + 1 : 0;
  if (w2 % 2 != 0) w2 = w2 - 1;
  if (h2 % 2 != 0) h2 = h2 - 1;
  g.w2 = w2;
  g.h2 = h2;
  g.hw = w2 / 2;
  g.hh = h2 / 2;
  const int maxd = w2 > h2 ? w2 : h2;
  g.side = maxd + 2 * offset;
  g.hs1 = g.side / 2;
  return g;
}

ISR_HD double quiet_nan() {
  union { uint64_t u; double d; } c;
  c.u = 0x7ff8000000000000ull;
  return c.d;
}

// cowrendersynth.py:717-736 -> the row-major 4 x 4 of KObj; NaN everywhere when side == 0
ISR_HD void camera(const double* K_in, const Geom& g, int maxB, int make_ndc, double* K_out) {
  if (g.side == 0) {
    for (int i = 0; i < 16; ++i) K_out[i] = quiet_nan();
    return;
  }
  double K[9];
  for (int i = 0; i < 9; ++i) K[i] = K_in[i];
  K[2] = K[2] + (double)(-g.x2 + g.hs1 - g.hw);
  K[5] = K[5] + (double)(-g.y2 + g.hs1 - g.hh);
  for (int i = 0; i < 9; ++i) K[i] = (K[i] * (double)maxB) / (double)g.side;
  K[8] = 1.0;
  if (make_ndc) {
    for (int i = 0; i < 9; ++i) K[i] = (K[i] * 2.0) / (double)maxB;
    K[8] = 0.0;
    K[2] = -(K[2] - 1.0);
    K[5] = -(K[5] - 1.0);
  }
  for (int i = 0; i < 16; ++i) K_out[i] = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K_out[4 * r + c] = K[3 * r + c];
  K_out[4 * 3 + 2] = 1.0;
  K_out[4 * 2 + 3] = 1.0;
}

// One axis of the resize: output index d -> the two clamped canvas indices and the weight of the second
ISR_HD void resize_axis(int d, int side, int maxB, int& i0, int& i1, double& fr) {
  const double s = (((double)d + 0.5) * (double)side) / (double)maxB - 0.5;
  const double f0 = floor(s);
  fr = s - f0;
  const long a = (long)f0, b = a + 1;                 // -1 <= a <= side - 1
  const long top = (long)side - 1;
  i0 = (int)(a < 0 ? 0 : a > top ? top : a);
  i1 = (int)(b < 0 ? 0 : b > top ? top : b);
}

// The canvas at (cy, cx), 0 <= cy, cx < side: the gated colours and the ungated mask channel 0, as f64
ISR_HD void canvas_at(const Frame& f, const Geom& g, int cy, int cx, double* col3, double& m0) {
  const int top = g.hs1 - g.hh, left = g.hs1 - g.hw;
  if (cy < top || cy >= g.hs1 + g.hh || cx < left || cx >= g.hs1 + g.hw) {
    col3[0] = col3[1] = col3[2] = m0 = 0.0;
    return;
  }
  const size_t p = (size_t)(g.y2 + cy - top) * (size_t)f.W + (size_t)(g.x2 + cx - left);
  const uint8_t* mk = f.mask + p * (size_t)f.Cm;
  const uint8_t* px = f.rgb + p * 3;
  m0 = (double)mk[0];
  for (int c = 0; c < 3; ++c) col3[c] = mk[c < f.Cm ? c : f.Cm - 1] ? (double)px[c] : 0.0;
}

ISR_HD float to_unit(double v) { return (float)(uint8_t)rint(v) / 255.0f; }      // 0 <= v <= 255

// Output pixel (dy, dx) of a frame with side > 0: rgb3 and sil
ISR_HD void view_pixel(const Frame& f, const Geom& g, int maxB, int sil_mode, int dy, int dx, float* rgb3, float& sil) {
  int x0, x1, y0, y1;
  double fx, fy;
  resize_axis(dx, g.side, maxB, x0, x1, fx);
  resize_axis(dy, g.side, maxB, y0, y1, fy);
  double p00[3], p01[3], p10[3], p11[3], m00, m01, m10, m11;
  canvas_at(f, g, y0, x0, p00, m00);
  canvas_at(f, g, y0, x1, p01, m01);
  canvas_at(f, g, y1, x0, p10, m10);
  canvas_at(f, g, y1, x1, p11, m11);
  const double w00 = (1.0 - fx) * (1.0 - fy), w01 = fx * (1.0 - fy), w10 = (1.0 - fx) * fy, w11 = fx * fy;
  for (int c = 0; c < 3; ++c) rgb3[c] = to_unit(((p00[c] * w00 + p01[c] * w01) + p10[c] * w10) + p11[c] * w11);
  if (sil_mode == kSilNearest) {
    const int cx = (int)(((long long)dx * g.side) / maxB), cy = (int)(((long long)dy * g.side) / maxB);
    double unused[3], m;
    canvas_at(f, g, cy, cx, unused, m);
    sil = (float)(uint8_t)m / 255.0f;
  } else {
    sil = to_unit(((m00 * w00 + m01 * w01) + m10 * w10) + m11 * w11);
  }
}

// The shape limits of include/isr_ingest.h; null when they hold
inline const char* check_shape(int n, int H, int W, int Cm, int maxB, int offset, int sil_mode) {
  if (n < 1 || (long long)n > (long long)kFrameGroup * kMaxGroups) return "n outside 1 .. 64 * 65535";
  if (H < 1 || W < 1 || (long long)H * W > kMaxPixels) return "H, W must be >= 1 with H W <= 2^28";
  if (Cm != 1 && Cm != 3) return "Cm must be 1 or 3";
  if (maxB < 1 || maxB > kMaxB) return "maxB outside 1 .. 4096";
  if (offset < 0 || offset > kMaxOffset) return "offset outside 0 .. 4096";
  if (sil_mode != kSilLinear && sil_mode != kSilNearest) return "sil_mode must be ISR_INGEST_SIL_LINEAR or ISR_INGEST_SIL_NEAREST";
  return nullptr;
}

// ---------------------------------------------------------------- host build
inline uint32_t load_word(const uint8_t* p) {      // little-endian, as the device's 16-byte load sees it
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The partial box of rows [r0, r1) of a frame's mask, by the device's walk: head bytes to the first 16-aligned address,
// 16-byte chunks, tail bytes.
inline Box strip_box_host(const uint8_t* mask, int H, int W, int Cm, int r0, int r1) {
  Box b = empty_box(H, W);
  const uint32_t row_bytes = (uint32_t)W * (uint32_t)Cm;
  const uint32_t beg = (uint32_t)r0 * row_bytes, end = (uint32_t)r1 * row_bytes;
  uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)(mask + beg) & 15u)) & 15u);
  if (head > end - beg) head = end - beg;
  const uint32_t chunks = (end - beg - head) / kChunk;
  for (uint32_t o = beg; o < beg + head; ++o) box_byte(b, o, mask[o], row_bytes, Cm);
  for (uint32_t k = 0; k < chunks; ++k) {
    const uint32_t o = beg + head + k * kChunk;
    box_chunk(b, o, load_word(mask + o), load_word(mask + o + 4), load_word(mask + o + 8), load_word(mask + o + 12), row_bytes, Cm);
  }
  for (uint32_t o = beg + head + chunks * kChunk; o < end; ++o) box_byte(b, o, mask[o], row_bytes, Cm);
  return b;
}

// One frame, all five outputs
inline void frame_host(const Frame& f, const double* K_in, int maxB, int offset, int make_ndc, int sil_mode, float* image,
                       float* sil, double* K_out, int32_t* geom, int32_t* status) {
  const int rows = strip_rows(f.H, f.W, f.Cm), strips = strips_of(f.H, f.W, f.Cm);
  Box b = empty_box(f.H, f.W);
  for (int s = 0; s < strips; ++s) {
    const int r0 = s * rows, r1 = r0 + rows < f.H ? r0 + rows : f.H;
    box_merge(b, strip_box_host(f.mask, f.H, f.W, f.Cm, r0, r1));
  }
  const Geom g = make_geom(b, offset);
  const int32_t gv[8] = {g.x2, g.y2, g.w2, g.h2, g.hw, g.hh, g.side, g.hs1};
  for (int i = 0; i < 8; ++i) geom[i] = gv[i];
  *status = g.side == 0 ? 1 : 0;
  camera(K_in, g, maxB, make_ndc, K_out);
  for (int dy = 0; dy < maxB; ++dy)
    for (int dx = 0; dx < maxB; ++dx) {
      float* o = image + ((size_t)dy * maxB + dx) * 3;
      float& s = sil[(size_t)dy * maxB + dx];
      if (g.side == 0) {
        o[0] = o[1] = o[2] = s = 0.0f;
      } else {
        view_pixel(f, g, maxB, sil_mode, dy, dx, o, s);
      }
    }
}

}  // namespace ingest
}  // namespace isr
