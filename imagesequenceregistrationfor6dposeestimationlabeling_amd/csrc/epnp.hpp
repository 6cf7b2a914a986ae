// epnp.hpp — EPnP (Lepetit, Moreno-Noguer, Fua, IJCV 2009, as in OpenCV's calib3d/src/epnp.cpp; restated from memory —
// OpenCV is not available to this build) in f64, one header built for the device (csrc/epnp.hip) and as host code
// (isr_epnp_host).  Only + - * /, sqrt and comparisons, under the library's -ffp-contract=off: host and device produce the
// same bits.  cv2.solvePnPRansac(flags=SOLVEPNP_P3P) ends with solvePnP(SOLVEPNP_EPNP) over the winner's consensus set;
// pnp(final="epnp") runs this solver there.
//
// Input: the masked correspondences (p_m world, f32; (u_m, v_m) pixels, f32; n of them), K (f_u = K[0], f_v = K[4],
// u_c = K[2], v_c = K[5]: EPnP ignores skew).  Pixels are used as they are (cv2 undistorts them with zero distortion and
// maps them back through K: the same values up to rounding).
//
//   1. control points   c0 = mean p;  A = sum (p - c0)(p - c0)^T;  Jacobi eigen-decomposition of A, eigenvalues d
//                       descending (negative rounding clamped to 0), unit eigenvectors u, each signed so that its component
//                       of largest magnitude (the first of equal ones) is positive;  c_i = c0 + sqrt(d_{i-1}/n) u_{i-1}.
//                       (The pose of noisy data depends on these signs; cv2 takes whatever its SVD returns.)
//   2. barycentric      CC = [c1 - c0 | c2 - c0 | c3 - c0];  CC+ its SVD pseudo-inverse: CC^T CC = W diag(s^2) W^T (Jacobi),
//                       CC+ = sum_{s_i > tol} w_i (CC w_i)^T / s_i^2, tol = 2 DBL_EPSILON (s_1 + s_2 + s_3) (cv::SVBkSb's
//                       cut-off, cvInvert(CV_SVD)).  alpha_{1..3} = CC+ (p - c0), alpha_0 = 1 - alpha_1 - alpha_2 - alpha_3.
//                       A planar set (d_3 = 0) gets c3 = c0 and alpha_3 = 0.
//   3. M^T M            rows [alpha_j f_u, 0, alpha_j (u_c - u)] and [0, alpha_j f_v, alpha_j (v_c - v)], j = 0..3.  Its
//                       78 distinct entries are f_u^2 S, f_v^2 S, f_u Su, f_v Sv, Sw and zeros of the 40 point sums
//                       S_jk = sum a_j a_k, Su_jk = sum a_j a_k du, Sv_jk = sum a_j a_k dv, Sw_jk = sum a_j a_k (du^2 + dv^2)
//                       (j <= k; du = u_c - u, dv = v_c - v): 40 accumulators instead of 78, the same matrix to rounding.
//   4. null space       cyclic Jacobi on M^T M (12 x 12); v_1..v_4 = the eigenvectors of the four smallest eigenvalues,
//                       ascending (cv2: the last four rows of U^T of its SVD).
//   5. candidates       L (6 x 10) and rho (6 squared control-point distances, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)),
//                       columns [b11 b12 b22 b13 b23 b33 b14 b24 b34 b44];  approx_1 (columns {0,1,3,6}), approx_2 ({0,1,2}),
//                       approx_3 ({0..4}): least squares by Householder QR (cv2: cvSolve(CV_SVD); the same solution for a
//                       full-rank L), OpenCV's sign rules; each refined by 5 Gauss-Newton steps on beta (6 x 4, Householder QR).
//   6. pose             ccs = sum_i beta_i v_i;  if the first masked point's depth sum_j alpha_j ccs_j.z < 0, ccs = -ccs.
//                       Procrustes: pc = sum_j alpha_j ccs_j;  B = sum pc (p - c0)^T (= sum (pc - mean pc)(p - mean p)^T:
//                       sum (p - c0) is 0);  B^T B = V diag(s^2) V^T (Jacobi, descending), v_3 = v_1 x v_2,
//                       u_i = B v_i / s_i (i = 1, 2), u_3 = sign(det B) (u_1 x u_2) — the SVD B = U S V^T without a division
//                       by s_3 (planar sets: s_3 = 0, det B = 0 -> +);  R = U V^T, its third row negated if det R < 0 (cv2);
//                       t = mean pc - R c0.
//   7. pick             mean reprojection error  mean sqrt((u - u^)^2 + (v - v^)^2),  u^ = u_c + f_u X/Z  per candidate;
//                       candidate 1, then 2 if strictly smaller, then 3 if strictly smaller (cv2's order).  chosen = 1..3.
//
// Reduction shape: every sum over points (steps 1, 3, 6, 7) strides an image's points over kEpnpBlocks x kEpnpThreads slots —
// slot (blk, t) takes m = blk * 256 + t + i * kEpnpBlocks * 256 in ascending i — sums each wave's 64 slots by the shuffle-down
// tree (offsets 32 .. 1), the block's four waves as ((w0 + w1) + w2) + w3, and the blocks in order.  The layout depends on
// neither the capacity nor the batch, and the host build replays it, so an image's result depends only on its own points
// and mask.  Every dense step reads the sums and runs the same code on host and device.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace isr_epnp {

constexpr int kEpnpBlocks = 64;    // workgroups per image of a pass over the points
constexpr int kEpnpThreads = 256;
constexpr int kMaxAcc = 40;        // the widest pass (M^T M)
constexpr int kJacobiSweeps = 60;
constexpr double kJacobiTol = 1e-30;   // stop once sum_{p<q} a_pq^2 <= kJacobiTol sum_i a_ii^2

// The passes over the points and their accumulator counts.
enum Pass { kP1 = 0, kP2 = 1, kP3 = 2, kP4 = 3, kP5 = 4 };
__host__ __device__ constexpr int pass_acc(int p) { return p == kP1 ? 4 : p == kP2 ? 6 : p == kP3 ? 40 : p == kP4 ? 36 : 3; }

// Per-image state (doubles): what the dense steps hand to the next pass.
enum : int {
  kN = 0,        // masked points
  kC0 = 1,       // centroid (3)
  kCw = 4,       // control points c_0..c_3 (12)
  kCi = 16,      // CC+ (3 x 3 row-major)
  kCcs = 25,     // 3 candidates x control points in the camera frame (36), sign fixed
  kRt = 61,      // 3 candidates x [R|t] (36)
  kErr = 97,     // 3 candidates' mean reprojection error
  kStateD = 128,
};

struct Intr { double fu, fv, uc, vc; };

__host__ __device__ inline Intr intr_of(const double* K) { return Intr{K[0], K[4], K[2], K[5]}; }

__host__ __device__ inline bool masked(const uint32_t* mask, int m) { return !mask || ((mask[m >> 5] >> (m & 31)) & 1u); }

// ------------------------------------------------------------------------------------------- per-point terms
__host__ __device__ inline void p1_point(double (&a)[4], double x, double y, double z) {
  a[0] += x; a[1] += y; a[2] += z; a[3] += 1.0;
}

__host__ __device__ inline void p2_point(double (&a)[6], const double* st, double x, double y, double z) {
  const double dx = x - st[kC0], dy = y - st[kC0 + 1], dz = z - st[kC0 + 2];
  a[0] += dx * dx; a[1] += dx * dy; a[2] += dx * dz; a[3] += dy * dy; a[4] += dy * dz; a[5] += dz * dz;
}

__host__ __device__ inline void alpha_of(const double* st, double x, double y, double z, double (&al)[4]) {
  const double dx = x - st[kC0], dy = y - st[kC0 + 1], dz = z - st[kC0 + 2];
  const double* ci = st + kCi;
  al[1] = ci[0] * dx + ci[1] * dy + ci[2] * dz;
  al[2] = ci[3] * dx + ci[4] * dy + ci[5] * dz;
  al[3] = ci[6] * dx + ci[7] * dy + ci[8] * dz;
  al[0] = 1.0 - al[1] - al[2] - al[3];
}

__host__ __device__ inline void p3_point(double (&a)[40], const double* st, const Intr& K, double x, double y, double z,
                                         double u, double v) {
  double al[4];
  alpha_of(st, x, y, z, al);
  const double du = K.uc - u, dv = K.vc - v, w = du * du + dv * dv;
  int i = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = j; k < 4; ++k) {
      const double q = al[j] * al[k];
      a[i] += q; a[10 + i] += q * du; a[20 + i] += q * dv; a[30 + i] += q * w;
      ++i;
    }
}

// camera-frame point of candidate c: ((a0 c0 + a1 c1) + a2 c2) + a3 c3
__host__ __device__ inline double pc_coord(const double* ccs, const double (&al)[4], int k) {
  return ((al[0] * ccs[k] + al[1] * ccs[3 + k]) + al[2] * ccs[6 + k]) + al[3] * ccs[9 + k];
}

__host__ __device__ inline void p4_point(double (&a)[36], const double* st, double x, double y, double z) {
  double al[4];
  alpha_of(st, x, y, z, al);
  const double d[3] = {x - st[kC0], y - st[kC0 + 1], z - st[kC0 + 2]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double* ccs = st + kCcs + 12 * c;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pc = pc_coord(ccs, al, j);
      a[12 * c + j] += pc;
#pragma unroll
      for (int k = 0; k < 3; ++k) a[12 * c + 3 + 3 * j + k] += pc * d[k];
    }
  }
}

__host__ __device__ inline void p5_point(double (&a)[3], const double* st, const Intr& K, double x, double y, double z,
                                         double u, double v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double* T = st + kRt + 12 * c;
    const double Xc = T[0] * x + T[1] * y + T[2] * z + T[3];
    const double Yc = T[4] * x + T[5] * y + T[6] * z + T[7];
    const double iz = 1.0 / (T[8] * x + T[9] * y + T[10] * z + T[11]);
    const double ue = K.uc + K.fu * Xc * iz, ve = K.vc + K.fv * Yc * iz;
    const double eu = u - ue, ev = v - ve;
    a[c] += sqrt(eu * eu + ev * ev);
  }
}

// ------------------------------------------------------------------------------------------- dense steps
struct NoSync {
  __host__ __device__ void operator()() const {}
};

// Cyclic Jacobi eigen-decomposition of the symmetric n x n A (row-major, overwritten: eigenvalues on the diagonal), V <- the
// eigenvectors as columns.  Lanes lane, lane + nl, ... update rows k of a rotation (n <= nl on the device: one wave); each
// element is computed by the same expression whichever lane owns it, so one lane (host) gives the same bits.  Rotation
// (p, q) for a_pq != 0, rows in order: theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1))
// (0.5 / theta for |theta| > 1e150), c = 1 / sqrt(t^2 + 1), s = t c.
template <class Sync>
__host__ __device__ inline void jacobi(double* A, double* V, int n, int lane, int nl, Sync sync) {
  for (int k = lane; k < n * n; k += nl) V[k] = (k / n == k % n) ? 1.0 : 0.0;
  sync();
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int p = 0; p < n; ++p) {
      dg += A[p * n + p] * A[p * n + p];
      for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
    }
    if (!(off > kJacobiTol * dg)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double app = A[p * n + p], aqq = A[q * n + q];
        const double th = (aqq - app) / (2.0 * apq);
        const double at = th < 0.0 ? -th : th;
        double t = at > 1e150 ? 0.5 / th : 1.0 / (at + sqrt(th * th + 1.0));
        if (at <= 1e150 && th < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        sync();
        for (int k = lane; k < n; k += nl) {
          if (k != p && k != q) {
            const double akp = A[k * n + p], akq = A[k * n + q];
            const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
            A[k * n + p] = nkp; A[p * n + k] = nkp;
            A[k * n + q] = nkq; A[q * n + k] = nkq;
          }
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
        if (lane == 0) {
          A[p * n + p] = app - t * apq;
          A[q * n + q] = aqq + t * apq;
          A[p * n + q] = 0.0;
          A[q * n + p] = 0.0;
        }
        sync();
      }
  }
}

// idx <- the order of the eigenvalues diag(A): ascending (desc = false) or descending, ties by index.
__host__ __device__ inline void eig_order(const double* A, int n, bool desc, int* idx) {
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int i = 1; i < n; ++i) {   // insertion sort: stable
    const int x = idx[i];
    const double vx = A[x * n + x];
    int j = i - 1;
    while (j >= 0 && (desc ? A[idx[j] * n + idx[j]] < vx : A[idx[j] * n + idx[j]] > vx)) {
      idx[j + 1] = idx[j];
      --j;
    }
    idx[j + 1] = x;
  }
}

// Step 1's mean from the sums of pass 1.
__host__ __device__ inline void centroid(double* st, const double* a4) {
  st[kN] = a4[3];
  for (int k = 0; k < 3; ++k) st[kC0 + k] = a4[k] / a4[3];
}

// Step 1 + 2 (one lane): sums a6 of pass 2 -> control points, CC+.  sh: 40 doubles of scratch, ish: 3 ints.
__host__ __device__ inline void control_points(double* st, const double* a6, double* sh, int* ish) {
  double* A = sh;        // 9
  double* V = sh + 9;    // 9
  double* CC = sh + 18;  // 9
  const double n = st[kN];
  A[0] = a6[0]; A[1] = a6[1]; A[2] = a6[2];
  A[3] = a6[1]; A[4] = a6[3]; A[5] = a6[4];
  A[6] = a6[2]; A[7] = a6[4]; A[8] = a6[5];
  jacobi(A, V, 3, 0, 1, NoSync{});
  eig_order(A, 3, true, ish);
  for (int k = 0; k < 3; ++k) st[kCw + k] = st[kC0 + k];
  for (int i = 1; i <= 3; ++i) {
    const int e = ish[i - 1];
    const double d = A[e * 3 + e] > 0.0 ? A[e * 3 + e] : 0.0;
    // the axis' sign: its component of largest magnitude positive (the first of equal ones) — the noisy result depends
    // on it, so it is fixed rather than left to the factorisation (cv2: whatever its SVD returns)
    int rm = 0;
    for (int r = 1; r < 3; ++r)
      if ((V[r * 3 + e] < 0.0 ? -V[r * 3 + e] : V[r * 3 + e]) > (V[rm * 3 + e] < 0.0 ? -V[rm * 3 + e] : V[rm * 3 + e])) rm = r;
    const double k = V[rm * 3 + e] < 0.0 ? -sqrt(d / n) : sqrt(d / n);
    for (int r = 0; r < 3; ++r) st[kCw + 3 * i + r] = st[kC0 + r] + k * V[r * 3 + e];
  }
  for (int r = 0; r < 3; ++r)
    for (int i = 1; i <= 3; ++i) CC[r * 3 + (i - 1)] = st[kCw + 3 * i + r] - st[kCw + r];
  // CC^T CC = W diag(s^2) W^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = CC[i] * CC[j] + CC[3 + i] * CC[3 + j] + CC[6 + i] * CC[6 + j];
  jacobi(A, V, 3, 0, 1, NoSync{});
  double s[3], ssum = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s[i] = sqrt(A[i * 3 + i] > 0.0 ? A[i * 3 + i] : 0.0);
    ssum += s[i];
  }
  const double tol = 2.0 * DBL_EPSILON * ssum;
  double* ci = st + kCi;
  for (int k = 0; k < 9; ++k) ci[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (!(s[i] > tol)) continue;
    const double is2 = 1.0 / (s[i] * s[i]);
    double cw[3];   // CC w_i
#pragma unroll
    for (int r = 0; r < 3; ++r) cw[r] = CC[r * 3] * V[i] + CC[r * 3 + 1] * V[3 + i] + CC[r * 3 + 2] * V[6 + i];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) ci[r * 3 + c] += V[r * 3 + i] * cw[c] * is2;
  }
}

// Step 3: M^T M (12 x 12 row-major) from the 40 sums; element e = 12 r + c for e = lane, lane + nl, ...
__host__ __device__ inline void build_mtm(const double* s40, const Intr& K, double* A, int lane, int nl) {
  for (int e = lane; e < 144; e += nl) {
    const int r = e / 12, c = e % 12;
    const int j = r / 3, a = r % 3, k = c / 3, b = c % 3;
    const int lo = j < k ? j : k, hi = j < k ? k : j;
    const int i = lo * 4 - lo * (lo - 1) / 2 + (hi - lo);   // index of pair (lo, hi) in the j <= k order
    double v;
    if (a == 0 && b == 0) v = K.fu * K.fu * s40[i];
    else if (a == 1 && b == 1) v = K.fv * K.fv * s40[i];
    else if (a == 2 && b == 2) v = s40[30 + i];
    else if ((a == 0 && b == 2) || (a == 2 && b == 0)) v = K.fu * s40[10 + i];
    else if ((a == 1 && b == 2) || (a == 2 && b == 1)) v = K.fv * s40[20 + i];
    else v = 0.0;
    A[e] = v;
  }
}

// Least squares min |A x - b| for A (m x k row-major, m = 6, k <= 5) by Householder QR; A and b are overwritten.  h: 6
// doubles of scratch.  An exactly zero pivot sets its unknown to 0 (a basic solution; cv2's cvSolve(CV_SVD) would return the
// minimum-norm one).
__host__ __device__ inline void lsq_qr(double* A, double* b, int k, double* x, double* h) {
  const int m = 6;
  for (int j = 0; j < k; ++j) {
    double nn = 0.0;
    for (int i = j; i < m; ++i) nn += A[i * k + j] * A[i * k + j];
    const double nrm = sqrt(nn);
    if (nrm == 0.0) continue;
    const double alpha = A[j * k + j] > 0.0 ? -nrm : nrm;
    double hh = 0.0;
    for (int i = j; i < m; ++i) {
      h[i] = (i == j) ? A[i * k + j] - alpha : A[i * k + j];
      hh += h[i] * h[i];
    }
    if (hh == 0.0) continue;
    for (int c = j; c < k; ++c) {
      double s = 0.0;
      for (int i = j; i < m; ++i) s += h[i] * A[i * k + c];
      const double f = 2.0 * s / hh;
      for (int i = j; i < m; ++i) A[i * k + c] -= f * h[i];
    }
    double s = 0.0;
    for (int i = j; i < m; ++i) s += h[i] * b[i];
    const double f = 2.0 * s / hh;
    for (int i = j; i < m; ++i) b[i] -= f * h[i];
  }
  for (int i = k - 1; i >= 0; --i) {
    double v = b[i];
    for (int c = i + 1; c < k; ++c) v -= A[i * k + c] * x[c];
    x[i] = A[i * k + i] == 0.0 ? 0.0 : v / A[i * k + i];   // an exactly zero pivot (planar sets): that unknown 0
  }
}

// 5 Gauss-Newton steps on beta (cv2's gauss_newton / compute_A_and_b_gauss_newton).  sh: 40 doubles of scratch.
__host__ __device__ inline void gauss_newton(const double* L, const double* rho, double* be, double* sh) {
  double* A = sh;        // 24
  double* b = sh + 24;   // 6
  double* x = sh + 30;   // 4
  double* h = sh + 34;   // 6
  for (int it = 0; it < 5; ++it) {
    for (int i = 0; i < 6; ++i) {
      const double* l = L + 10 * i;
      A[4 * i + 0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
      A[4 * i + 1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
      A[4 * i + 2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
      A[4 * i + 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
      b[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] +
                       l[4] * be[1] * be[2] + l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] +
                       l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
    }
    lsq_qr(A, b, 4, x, h);
    for (int i = 0; i < 4; ++i) be[i] += x[i];
  }
}

// Step 5 (one lane): the 4 null-space vectors (v + 12 i, i = 0..3: v_1..v_4) -> L, rho, the three refined beta vectors ->
// ccs of the three candidates (before the sign rule).  sh: 200 doubles of scratch.
__host__ __device__ inline void candidates(double* st, const double* v, double* sh) {
  double* L = sh;           // 60
  double* rho = sh + 60;    // 6
  double* be = sh + 66;     // 3 x 4
  double* A = sh + 78;      // 30
  double* b = sh + 108;     // 6
  double* x = sh + 114;     // 5
  double* h = sh + 119;     // 6
  double* gn = sh + 125;    // 40
  const double* cw = st + kCw;
  int a = 0, c = 1;
  for (int p = 0; p < 6; ++p) {
    double dv[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dv[i][k] = v[12 * i + 3 * a + k] - v[12 * i + 3 * c + k];
    auto dot = [&](int i, int j) { return dv[i][0] * dv[j][0] + dv[i][1] * dv[j][1] + dv[i][2] * dv[j][2]; };
    double* l = L + 10 * p;
    l[0] = dot(0, 0);
    l[1] = 2 * dot(0, 1);
    l[2] = dot(1, 1);
    l[3] = 2 * dot(0, 2);
    l[4] = 2 * dot(1, 2);
    l[5] = dot(2, 2);
    l[6] = 2 * dot(0, 3);
    l[7] = 2 * dot(1, 3);
    l[8] = 2 * dot(2, 3);
    l[9] = dot(3, 3);
    const double e0 = cw[3 * a] - cw[3 * c], e1 = cw[3 * a + 1] - cw[3 * c + 1], e2 = cw[3 * a + 2] - cw[3 * c + 2];
    rho[p] = e0 * e0 + e1 * e1 + e2 * e2;
    if (++c > 3) { ++a; c = a + 1; }
  }
  // approx_1: [b11 b12 b13 b14] from columns {0, 1, 3, 6}
  {
    for (int i = 0; i < 6; ++i) {
      A[4 * i] = L[10 * i]; A[4 * i + 1] = L[10 * i + 1]; A[4 * i + 2] = L[10 * i + 3]; A[4 * i + 3] = L[10 * i + 6];
      b[i] = rho[i];
    }
    lsq_qr(A, b, 4, x, h);
    double* B = be;
    if (x[0] < 0) {
      B[0] = sqrt(-x[0]);
      B[1] = -x[1] / B[0]; B[2] = -x[2] / B[0]; B[3] = -x[3] / B[0];
    } else {
      B[0] = sqrt(x[0]);
      B[1] = x[1] / B[0]; B[2] = x[2] / B[0]; B[3] = x[3] / B[0];
    }
  }
  // approx_2: [b11 b12 b22] from columns {0, 1, 2}
  {
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 3; ++j) A[3 * i + j] = L[10 * i + j];
      b[i] = rho[i];
    }
    lsq_qr(A, b, 3, x, h);
    double* B = be + 4;
    if (x[0] < 0) {
      B[0] = sqrt(-x[0]);
      B[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
    } else {
      B[0] = sqrt(x[0]);
      B[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
    }
    if (x[1] < 0) B[0] = -B[0];
    B[2] = 0.0; B[3] = 0.0;
  }
  // approx_3: [b11 b12 b22 b13 b23] from columns {0..4}
  {
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 5; ++j) A[5 * i + j] = L[10 * i + j];
      b[i] = rho[i];
    }
    lsq_qr(A, b, 5, x, h);
    double* B = be + 8;
    if (x[0] < 0) {
      B[0] = sqrt(-x[0]);
      B[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
    } else {
      B[0] = sqrt(x[0]);
      B[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
    }
    if (x[1] < 0) B[0] = -B[0];
    B[2] = x[3] / B[0];
    B[3] = 0.0;
  }
  for (int cnd = 0; cnd < 3; ++cnd) {
    double* B = be + 4 * cnd;
    gauss_newton(L, rho, B, gn);
    double* ccs = st + kCcs + 12 * cnd;
    for (int k = 0; k < 12; ++k) ccs[k] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 12; ++k) ccs[k] += B[i] * v[12 * i + k];
  }
}

// Step 6's sign rule: the first masked point (x, y, z) in front of the camera, per candidate.
__host__ __device__ inline void sign_rule(double* st, double x, double y, double z) {
  double al[4];
  alpha_of(st, x, y, z, al);
  for (int cnd = 0; cnd < 3; ++cnd) {
    double* ccs = st + kCcs + 12 * cnd;
    if (pc_coord(ccs, al, 2) < 0.0)
      for (int k = 0; k < 12; ++k) ccs[k] = -ccs[k];
  }
}

// Step 6's Procrustes for candidate cnd from its 12 sums (sum pc, then B row-major).  sh: 40 doubles, ish: 3 ints.
__host__ __device__ inline void procrustes(double* st, int cnd, const double* a12, double* sh, int* ish) {
  double* A = sh;        // 9: B^T B
  double* V = sh + 9;    // 9
  double* U = sh + 18;   // 9 (columns)
  double* W = sh + 27;   // 9 (columns: v_1, v_2, v_3)
  const double* B = a12 + 3;
  const double n = st[kN];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = B[i] * B[j] + B[3 + i] * B[3 + j] + B[6 + i] * B[6 + j];
  jacobi(A, V, 3, 0, 1, NoSync{});
  eig_order(A, 3, true, ish);
  double s[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = ish[i];
    s[i] = sqrt(A[e * 3 + e] > 0.0 ? A[e * 3 + e] : 0.0);
    for (int r = 0; r < 3; ++r) W[r * 3 + i] = V[r * 3 + e];
  }
  W[2] = W[3] * W[7] - W[6] * W[4];
  W[5] = W[6] * W[1] - W[0] * W[7];
  W[8] = W[0] * W[4] - W[3] * W[1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    for (int r = 0; r < 3; ++r) U[r * 3 + i] = (B[r * 3] * W[i] + B[r * 3 + 1] * W[3 + i] + B[r * 3 + 2] * W[6 + i]) / s[i];
  const double detB = B[0] * (B[4] * B[8] - B[5] * B[7]) - B[1] * (B[3] * B[8] - B[5] * B[6]) + B[2] * (B[3] * B[7] - B[4] * B[6]);
  const double sg = detB < 0.0 ? -1.0 : 1.0;
  U[2] = sg * (U[3] * U[7] - U[6] * U[4]);
  U[5] = sg * (U[6] * U[1] - U[0] * U[7]);
  U[8] = sg * (U[0] * U[4] - U[3] * U[1]);
  double* T = st + kRt + 12 * cnd;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[4 * i + j] = U[i * 3] * W[j * 3] + U[i * 3 + 1] * W[j * 3 + 1] + U[i * 3 + 2] * W[j * 3 + 2];
  const double detR = T[0] * T[5] * T[10] + T[1] * T[6] * T[8] + T[2] * T[4] * T[9] - T[2] * T[5] * T[8] -
                      T[1] * T[4] * T[10] - T[0] * T[6] * T[9];
  if (detR < 0.0) { T[8] = -T[8]; T[9] = -T[9]; T[10] = -T[10]; }
  const double* c0 = st + kC0;
  for (int i = 0; i < 3; ++i) {
    const double pc0 = a12[i] / n;
    T[4 * i + 3] = pc0 - (T[4 * i] * c0[0] + T[4 * i + 1] * c0[1] + T[4 * i + 2] * c0[2]);
  }
}

// Step 7: the pick (cv2's order) -> Rt (12), err (3); returns chosen = 1..3.
__host__ __device__ inline int pick(double* st, const double* a3, double* Rt, double* err) {
  const double n = st[kN];
  for (int c = 0; c < 3; ++c) st[kErr + c] = a3[c] / n;
  int N = 0;
  if (st[kErr + 1] < st[kErr + N]) N = 1;
  if (st[kErr + 2] < st[kErr + N]) N = 2;
  for (int k = 0; k < 12; ++k) Rt[k] = st[kRt + 12 * N + k];
  for (int c = 0; c < 3; ++c) err[c] = st[kErr + c];
  return N + 1;
}

// ------------------------------------------------------------------------------------------- host replay
// One pass over an image's points in the device's reduction shape: slots, wave trees, wave order, blocks in order.
template <int NA, class F>
inline void host_pass(int M, const uint32_t* mask, F&& point, double* out) {
  for (int k = 0; k < NA; ++k) out[k] = 0.0;
  for (int blk = 0; blk < kEpnpBlocks; ++blk) {
    double acc[kEpnpThreads][NA];
    for (int t = 0; t < kEpnpThreads; ++t) {
      double a[NA];
      for (int k = 0; k < NA; ++k) a[k] = 0.0;
      for (int m = blk * kEpnpThreads + t; m < M; m += kEpnpBlocks * kEpnpThreads)
        if (masked(mask, m)) point(a, m);
      for (int k = 0; k < NA; ++k) acc[t][k] = a[k];
    }
    double wv[4][NA];
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < NA; ++k) {
        double s[64];
        for (int l = 0; l < 64; ++l) s[l] = acc[64 * w + l][k];
        for (int off = 32; off > 0; off >>= 1)
          for (int l = 0; l < off; ++l) s[l] = s[l] + s[l + off];
        wv[w][k] = s[0];
      }
    for (int k = 0; k < NA; ++k) out[k] += ((wv[0][k] + wv[1][k]) + wv[2][k]) + wv[3][k];
  }
}

}  // namespace isr_epnp
