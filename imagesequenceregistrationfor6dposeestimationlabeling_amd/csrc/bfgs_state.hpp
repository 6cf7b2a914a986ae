// bfgs_state.hpp — scipy.optimize.minimize(method='BFGS') as a reverse-communication state machine, f64, n <= 8.
//
// A port of SciPy 1.15's _minimize_bfgs (scipy/optimize/_optimize.py), _line_search_wolfe12, line_search_wolfe1 /
// scalar_search_wolfe1 with DCSRCH and dcstep (_linesearch.py, _dcsrch.py), and the fallback line_search_wolfe2 /
// scalar_search_wolfe2 with _zoom, _cubicmin and _quadmin.  SciPy is BSD-3-Clause licensed, Copyright (c) 2001-2002
// Enthought, Inc. 2003, SciPy Developers; DCSRCH / dcstep derive from MINPACK-2 (Argonne National Laboratory,
// J. J. More' and D. J. Thuente).  Every constant and rule is SciPy's; the comments name the statement each block ports.
//
// The same code runs as host code (isr_bfgs_host_*) and on the device (isr_refine_bfgs_batch, one thread per item): it
// only uses + - * / and sqrt, each correctly rounded on both sides, and the library is built with -ffp-contract=off, so
// host and device runs of one problem have the same bits.  Against numpy the sums of np.dot run in index order here; BLAS
// may order (or fuse) them differently, so a scipy run agrees to rounding, not bit for bit.
//
// Protocol.  bfgs_init() sets the first point to evaluate (x0) in S->xr.  Each bfgs_step(S, f, g) consumes the value and
// gradient at S->xr and returns kBfgsNeedEval with the next point in S->xr, or kBfgsDone with S->status set.  A point
// equal to the last one evaluated is not asked for again (scipy's ScalarFunction caches its last x), so nfev counts
// distinct evaluations as scipy's does.  All state lives in the struct (no local arrays): on the device the struct is in
// global memory and the kernel uses no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace isr_bfgs {

#define BFGS_HD __host__ __device__ __forceinline__

constexpr int kMaxN = 8;
constexpr int kNeedEval = 0;
constexpr int kDone = 1;

// scipy's warnflag; kStatusRounds is this project's "max_rounds ran out while the item was live".
constexpr int kStatusOk = 0, kStatusMaxIter = 1, kStatusLineSearch = 2, kStatusNaN = 3, kStatusRounds = 4;

// _minimize_bfgs(..., c1=1e-4, c2=0.9) and the line searches' limits as _minimize_bfgs passes them
constexpr double kC1 = 1e-4, kC2 = 0.9, kAmin = 1e-100, kAmax = 1e100, kXtol = 1e-14, kXrtol = 0.0;
constexpr int kDcsrchIter = 100, kWolfe2Iter = 10, kZoomIter = 10;

enum Phase : int32_t {
  P_START, P_OUTER, P_DC_ITER, P_DC_EVAL, P_W2_FIRST, P_W2_LOOP, P_W2_NEXT, P_Z_LOOP, P_Z_EVAL, P_FINISHED
};
enum Task : int32_t { T_START, T_FG, T_CONV, T_WARN, T_ERROR };

struct State {
  int32_t n, maxiter, phase, status;
  int32_t k, nfev, n_wolfe2, have_last;
  double gtol;
  double old_fval, old_old_fval, gnorm;
  double x[kMaxN], gfk[kMaxN], pk[kMaxN], sk[kMaxN], yk[kMaxN];
  double H[kMaxN * kMaxN], T[kMaxN * kMaxN];
  double xr[kMaxN];                  // the point asked for
  double xl[kMaxN], gl[kMaxN], fl;   // the last point evaluated and its (f, g)
  double gval[kMaxN];                // the line search's gradient at its accepted step
  // the line search of one iteration
  double derphi0, phi0, old_phi0, ls_alpha, ls_fval;
  // DCSRCH
  int32_t dc_i, dc_task, dc_stage, dc_brackt;
  double dc_stp, dc_f, dc_g, dc_finit, dc_ginit, dc_gtest, dc_width, dc_width1;
  double dc_stx, dc_fx, dc_gx, dc_sty, dc_fy, dc_gy, dc_stmin, dc_stmax;
  // scalar_search_wolfe2
  int32_t w_i, z_i;
  double w_a0, w_a1, w_phi_a0, w_phi_a1, w_dphi_a0, w_dphi_a1;
  // _zoom
  double z_lo, z_hi, z_phi_lo, z_phi_hi, z_dphi_lo, z_phi_rec, z_rec, z_aj;
};

// Python's min / max of two (the first argument wins ties and NaN comparisons), np.clip (NaN propagates), np.sign.
BFGS_HD double pymin(double a, double b) { return b < a ? b : a; }
BFGS_HD double pymax(double a, double b) { return b > a ? b : a; }
BFGS_HD bool isnan_(double v) { return __builtin_isnan(v); }
BFGS_HD bool isfinite_(double v) { return __builtin_isfinite(v); }
BFGS_HD double npclip(double v, double lo, double hi) { return isnan_(v) ? v : (v < lo ? lo : (v > hi ? hi : v)); }
BFGS_HD double npsign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }
BFGS_HD double fabs_(double v) { return __builtin_fabs(v); }

BFGS_HD double dot(const double* a, const double* b, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += a[i] * b[i];
  return s;
}

// np.amax(np.abs(v)): NaN propagates
BFGS_HD double norm_inf(const double* v, int n) {
  double m = fabs_(v[0]);
  for (int i = 1; i < n; ++i) {
    const double a = fabs_(v[i]);
    if (isnan_(m) || isnan_(a)) m = isnan_(m) ? m : a;
    else if (a > m) m = a;
  }
  return m;
}

// np.errstate(divide='raise', over='raise', invalid='raise'): an operation raises when it makes a NaN out of non-NaN
// operands (invalid) or an infinity out of finite ones (overflow, divide by zero).
struct Fpe {
  bool bad = false;
  BFGS_HD double operator()(double r, double a, double b) {
    if ((isnan_(r) && !isnan_(a) && !isnan_(b)) || (__builtin_isinf(r) && !__builtin_isinf(a) && !__builtin_isinf(b)))
      bad = true;
    return r;
  }
};

// _cubicmin(a, fa, fpa, b, fb, c, fc): false where scipy returns None
BFGS_HD bool cubicmin(double a, double fa, double fpa, double b, double fb, double c, double fc, double* xmin) {
  Fpe e;
  const double C = fpa;
  const double db = e(b - a, b, a);
  const double dc = e(c - a, c, a);
  const double dbdc = e(db * dc, db, dc);
  const double denom = e(e(dbdc * dbdc, dbdc, dbdc) * e(db - dc, db, dc), dbdc * dbdc, db - dc);
  const double db2 = e(db * db, db, db), dc2 = e(dc * dc, dc, dc);
  const double d00 = dc2, d01 = -db2, d10 = -e(dc2 * dc, dc2, dc), d11 = e(db2 * db, db2, db);
  const double fbfa = e(fb - fa, fb, fa), Cdb = e(C * db, C, db);
  const double fcfa = e(fc - fa, fc, fa), Cdc = e(C * dc, C, dc);
  const double v0 = e(fbfa - Cdb, fbfa, Cdb), v1 = e(fcfa - Cdc, fcfa, Cdc);
  double A = d00 * v0 + d01 * v1;   // np.dot: not a ufunc, no floating-point check
  double B = d10 * v0 + d11 * v1;
  A = e(A / denom, A, denom);
  B = e(B / denom, B, denom);
  const double BB = e(B * B, B, B), A3 = e(3.0 * A, 3.0, A), A3C = e(A3 * C, A3, C);
  const double radical = e(BB - A3C, BB, A3C);
  const double sr = e(sqrt(radical), radical, 0.0);
  const double num = e(-B + sr, -B, sr);
  const double q = e(num / A3, num, A3);
  const double r = e(a + q, a, q);
  if (e.bad || !isfinite_(r)) return false;
  *xmin = r;
  return true;
}

// _quadmin(a, fa, fpa, b, fb)
BFGS_HD bool quadmin(double a, double fa, double fpa, double b, double fb, double* xmin) {
  Fpe e;
  const double D = fa, C = fpa;
  const double a1 = e(a * 1.0, a, 1.0);
  const double db = e(b - a1, b, a1);
  const double fbD = e(fb - D, fb, D), Cdb = e(C * db, C, db);
  const double num = e(fbD - Cdb, fbD, Cdb), dd = e(db * db, db, db);
  const double B = e(num / dd, num, dd);
  const double B2 = e(2.0 * B, 2.0, B);
  const double q = e(C / B2, C, B2);
  const double r = e(a - q, a, q);
  if (e.bad || !isfinite_(r)) return false;
  *xmin = r;
  return true;
}

struct Dc {
  double stx, fx, dx, sty, fy, dy, stp;
  int32_t brackt;
};

// dcstep (MINPACK-2 via _dcsrch.py): the updated interval (stx, sty) and the new trial step.  Values in, a struct out
// (no references: the compiler keeps it all in registers).
BFGS_HD Dc dcstep(double stx, double fx, double dx, double sty, double fy, double dy, double stp, double fp, double dp,
                  int32_t brackt, double stpmin, double stpmax) {
  const double sgnd = npsign(dp) * npsign(dx);
  double stpf;
  if (fp > fx) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = pymax(pymax(fabs_(theta), fabs_(dx)), fabs_(dp));
    const double ts = theta / s;
    double gamma = s * sqrt(ts * ts - (dx / s) * (dp / s));
    if (stp < stx) gamma = gamma * -1.0;
    const double p = (gamma - dx) + theta;
    const double q = ((gamma - dx) + gamma) + dp;
    const double r = p / q;
    const double stpc = stx + r * (stp - stx);
    const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
    if (fabs_(stpc - stx) <= fabs_(stpq - stx))
      stpf = stpc;
    else
      stpf = stpc + (stpq - stpc) / 2.0;
    brackt = 1;
  } else if (sgnd < 0.0) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = pymax(pymax(fabs_(theta), fabs_(dx)), fabs_(dp));
    const double ts = theta / s;
    double gamma = s * sqrt(ts * ts - (dx / s) * (dp / s));
    if (stp > stx) gamma = gamma * -1.0;
    const double p = (gamma - dp) + theta;
    const double q = ((gamma - dp) + gamma) + dx;
    const double r = p / q;
    const double stpc = stp + r * (stx - stp);
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (fabs_(stpc - stp) > fabs_(stpq - stp))
      stpf = stpc;
    else
      stpf = stpq;
    brackt = 1;
  } else if (fabs_(dp) < fabs_(dx)) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = pymax(pymax(fabs_(theta), fabs_(dx)), fabs_(dp));
    const double ts = theta / s;
    const double rad = ts * ts - (dx / s) * (dp / s);
    double gamma = s * sqrt(rad > 0.0 ? rad : 0.0);          // max(0, rad): a NaN gives 0
    if (stp > stx) gamma = -gamma;
    const double p = (gamma - dp) + theta;
    const double q = (gamma + (dx - dp)) + gamma;
    const double r = p / q;
    double stpc;
    if (r < 0.0 && gamma != 0.0)
      stpc = stp + r * (stx - stp);
    else if (stp > stx)
      stpc = stpmax;
    else
      stpc = stpmin;
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      if (fabs_(stpc - stp) < fabs_(stpq - stp))
        stpf = stpc;
      else
        stpf = stpq;
      if (stp > stx)
        stpf = pymin(stp + 0.66 * (sty - stp), stpf);
      else
        stpf = pymax(stp + 0.66 * (sty - stp), stpf);
    } else {
      if (fabs_(stpc - stp) > fabs_(stpq - stp))
        stpf = stpc;
      else
        stpf = stpq;
      stpf = npclip(stpf, stpmin, stpmax);
    }
  } else {
    if (brackt) {
      const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
      const double s = pymax(pymax(fabs_(theta), fabs_(dy)), fabs_(dp));
      const double ts = theta / s;
      double gamma = s * sqrt(ts * ts - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      const double p = (gamma - dp) + theta;
      const double q = ((gamma - dp) + gamma) + dy;
      const double r = p / q;
      stpf = stp + r * (sty - stp);
    } else if (stp > stx) {
      stpf = stpmax;
    } else {
      stpf = stpmin;
    }
  }
  Dc o;
  o.brackt = brackt;
  o.stp = stpf;
  if (fp > fx) {
    o.stx = stx; o.fx = fx; o.dx = dx;
    o.sty = stp; o.fy = fp; o.dy = dp;
  } else {
    const bool swap = sgnd < 0.0;
    o.sty = swap ? stx : sty; o.fy = swap ? fx : fy; o.dy = swap ? dx : dy;
    o.stx = stp; o.fx = fp; o.dx = dp;
  }
  return o;
}

// DCSRCH._iterate(stp, f, g, task) with ftol = c1, gtol = c2, stpmin = amin, stpmax = amax
BFGS_HD void dcsrch_iterate(State* S) {
  const double p5 = 0.5, p66 = 0.66, xtrapl = 1.1, xtrapu = 4.0;
  double stp = S->dc_stp;
  const double f = S->dc_f, g = S->dc_g;
  if (S->dc_task == T_START) {
    int32_t task = T_START;
    if (stp < kAmin) task = T_ERROR;
    if (stp > kAmax) task = T_ERROR;
    if (g >= 0) task = T_ERROR;
    if (task == T_ERROR) { S->dc_task = task; return; }
    S->dc_brackt = 0;
    S->dc_stage = 1;
    S->dc_finit = f;
    S->dc_ginit = g;
    S->dc_gtest = kC1 * S->dc_ginit;
    S->dc_width = kAmax - kAmin;
    S->dc_width1 = S->dc_width / p5;
    S->dc_stx = 0.0; S->dc_fx = S->dc_finit; S->dc_gx = S->dc_ginit;
    S->dc_sty = 0.0; S->dc_fy = S->dc_finit; S->dc_gy = S->dc_ginit;
    S->dc_stmin = 0.0;
    S->dc_stmax = stp + xtrapu * stp;
    S->dc_task = T_FG;
    return;
  }
  const double ftest = S->dc_finit + stp * S->dc_gtest;
  if (S->dc_stage == 1 && f <= ftest && g >= 0) S->dc_stage = 2;
  int32_t task = S->dc_task;
  if (S->dc_brackt && (stp <= S->dc_stmin || stp >= S->dc_stmax)) task = T_WARN;
  if (S->dc_brackt && S->dc_stmax - S->dc_stmin <= kXtol * S->dc_stmax) task = T_WARN;
  if (stp == kAmax && f <= ftest && g <= S->dc_gtest) task = T_WARN;
  if (stp == kAmin && (f > ftest || g >= S->dc_gtest)) task = T_WARN;
  if (f <= ftest && fabs_(g) <= kC2 * -S->dc_ginit) task = T_CONV;
  if (task == T_WARN || task == T_CONV) { S->dc_task = task; return; }

  // stage 1 with a lower value that fails the sufficient decrease: dcstep on the modified function psi (f - stp gtest)
  const bool psi = S->dc_stage == 1 && f <= S->dc_fx && f > ftest;
  const double gtest = S->dc_gtest;
  const double stx = S->dc_stx, sty = S->dc_sty;
  const double fx = psi ? S->dc_fx - S->dc_stx * gtest : S->dc_fx;
  const double fy = psi ? S->dc_fy - S->dc_sty * gtest : S->dc_fy;
  const double gx = psi ? S->dc_gx - gtest : S->dc_gx;
  const double gy = psi ? S->dc_gy - gtest : S->dc_gy;
  const double fp = psi ? f - stp * gtest : f;
  const double gp = psi ? g - gtest : g;
  const Dc d = dcstep(stx, fx, gx, sty, fy, gy, stp, fp, gp, S->dc_brackt, S->dc_stmin, S->dc_stmax);
  stp = d.stp;
  S->dc_brackt = d.brackt;
  S->dc_stx = d.stx;
  S->dc_sty = d.sty;
  S->dc_fx = psi ? d.fx + d.stx * gtest : d.fx;
  S->dc_fy = psi ? d.fy + d.sty * gtest : d.fy;
  S->dc_gx = psi ? d.dx + gtest : d.dx;
  S->dc_gy = psi ? d.dy + gtest : d.dy;
  if (S->dc_brackt) {
    if (fabs_(S->dc_sty - S->dc_stx) >= p66 * S->dc_width1) stp = S->dc_stx + p5 * (S->dc_sty - S->dc_stx);
    S->dc_width1 = S->dc_width;
    S->dc_width = fabs_(S->dc_sty - S->dc_stx);
  }
  if (S->dc_brackt) {
    S->dc_stmin = pymin(S->dc_stx, S->dc_sty);
    S->dc_stmax = pymax(S->dc_stx, S->dc_sty);
  } else {
    S->dc_stmin = stp + xtrapl * (stp - S->dc_stx);
    S->dc_stmax = stp + xtrapu * (stp - S->dc_stx);
  }
  stp = npclip(stp, kAmin, kAmax);
  if ((S->dc_brackt && (stp <= S->dc_stmin || stp >= S->dc_stmax)) ||
      (S->dc_brackt && S->dc_stmax - S->dc_stmin <= kXtol * S->dc_stmax))
    stp = S->dc_stx;
  S->dc_stp = stp;
  S->dc_task = T_FG;
}

// Ask for xk + a pk (numpy's xk + s*pk).  True when it equals the last point evaluated: its (f, g) are reused.
BFGS_HD bool want(State* S, double a, int32_t resume) {
  bool same = S->have_last != 0;
  for (int i = 0; i < S->n; ++i) {
    S->xr[i] = S->x[i] + a * S->pk[i];
    same = same && S->xr[i] == S->xl[i];
  }
  S->phase = resume;
  return same;
}

// the first step guess of scalar_search_wolfe1 / scalar_search_wolfe2
BFGS_HD double first_step(double phi0, double old_phi0, double derphi0) {
  double a1 = 1.0;
  if (derphi0 != 0.0) {
    a1 = pymin(1.0, 1.01 * 2.0 * (phi0 - old_phi0) / derphi0);
    if (a1 < 0.0) a1 = 1.0;
  }
  return a1;
}

BFGS_HD void finish(State* S, int32_t warnflag) {
  // fval = old_fval; the status by scipy's precedence
  int32_t st = kStatusOk;
  bool nan_x = false;
  for (int i = 0; i < S->n; ++i) nan_x = nan_x || isnan_(S->x[i]);
  if (warnflag == kStatusLineSearch)
    st = kStatusLineSearch;
  else if (S->k >= S->maxiter)
    st = kStatusMaxIter;
  else if (isnan_(S->gnorm) || isnan_(S->old_fval) || nan_x)
    st = kStatusNaN;
  S->status = st;
  S->phase = P_FINISHED;
}

// Line search done: alpha_k = S->ls_alpha, the new fval S->ls_fval, gfkp1 = S->gval.  The rest of the BFGS iteration.
// Returns true when the run has finished.
BFGS_HD bool bfgs_update(State* S) {
  const int n = S->n;
  const double alpha = S->ls_alpha;
  S->old_old_fval = S->phi0;
  S->old_fval = S->ls_fval;
  for (int i = 0; i < n; ++i) {
    S->sk[i] = alpha * S->pk[i];
    S->x[i] = S->x[i] + S->sk[i];
    S->yk[i] = S->gval[i] - S->gfk[i];
    S->gfk[i] = S->gval[i];
  }
  S->k += 1;
  S->gnorm = norm_inf(S->gfk, n);
  if (S->gnorm <= S->gtol) { finish(S, kStatusOk); return true; }
  // alpha_k * vecnorm(pk) <= xrtol * (xrtol + vecnorm(xk))
  const double npk = sqrt(dot(S->pk, S->pk, n)), nxk = sqrt(dot(S->x, S->x, n));
  if (alpha * npk <= kXrtol * (kXrtol + nxk)) { finish(S, kStatusOk); return true; }
  if (!isfinite_(S->old_fval)) { finish(S, kStatusLineSearch); return true; }
  const double rhok_inv = dot(S->yk, S->sk, n);
  const double rhok = rhok_inv == 0.0 ? 1000.0 : 1.0 / rhok_inv;
  // Hk = A1 (Hk A2) + rhok sk sk^T, A1 = I - sk yk^T rhok, A2 = I - yk sk^T rhok
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int l = 0; l < n; ++l) {
        const double a2 = (l == j ? 1.0 : 0.0) - S->yk[l] * S->sk[j] * rhok;
        s += S->H[i * kMaxN + l] * a2;
      }
      S->T[i * kMaxN + j] = s;
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int l = 0; l < n; ++l) {
        const double a1 = (i == l ? 1.0 : 0.0) - S->sk[i] * S->yk[l] * rhok;
        s += a1 * S->T[l * kMaxN + j];
      }
      S->H[i * kMaxN + j] = s + rhok * S->sk[i] * S->sk[j];
    }
  S->phase = P_OUTER;
  return false;
}

BFGS_HD void copy_n(double* dst, const double* src, int n) {
  for (int i = 0; i < n; ++i) dst[i] = src[i];
}

// line_search_wolfe1 failed: line_search_wolfe2(f, fprime, xk, pk, gfk, old_fval, old_old_fval, c1=c1, c2=c2, amax=amax)
// starts with phi(alpha1).  Same return convention as want().
BFGS_HD bool start_wolfe2(State* S) {
  S->n_wolfe2 += 1;
  S->w_a0 = 0.0;
  S->w_a1 = pymin(first_step(S->phi0, S->old_phi0, S->derphi0), kAmax);
  return want(S, S->w_a1, P_W2_FIRST);
}

// Runs until a new evaluation is needed (kNeedEval, point in S->xr) or the run ends (kDone).
BFGS_HD int run(State* S) {
  const int n = S->n;
  for (;;) {
    switch (S->phase) {
      case P_START: {                                   // old_fval = f(x0); gfk = myfprime(x0)
        S->old_fval = S->fl;
        copy_n(S->gfk, S->gl, n);
        for (int i = 0; i < n * kMaxN; ++i) S->H[i] = 0.0;
        for (int i = 0; i < n; ++i) S->H[i * kMaxN + i] = 1.0;
        S->old_old_fval = S->old_fval + sqrt(dot(S->gfk, S->gfk, n)) / 2.0;
        S->gnorm = norm_inf(S->gfk, n);
        S->phase = P_OUTER;
        break;
      }
      case P_OUTER: {                                   // while (gnorm > gtol) and (k < maxiter)
        if (!(S->gnorm > S->gtol && S->k < S->maxiter)) { finish(S, kStatusOk); return kDone; }
        for (int i = 0; i < n; ++i) {                   // pk = -np.dot(Hk, gfk)
          double s = 0.0;
          for (int j = 0; j < n; ++j) s += S->H[i * kMaxN + j] * S->gfk[j];
          S->pk[i] = -s;
        }
        // line_search_wolfe1 -> scalar_search_wolfe1 -> DCSRCH(alpha1, phi0, derphi0, maxiter=100)
        S->derphi0 = dot(S->gfk, S->pk, n);
        S->phi0 = S->old_fval;
        S->old_phi0 = S->old_old_fval;
        copy_n(S->gval, S->gfk, n);
        S->dc_stp = first_step(S->phi0, S->old_phi0, S->derphi0);
        S->dc_f = S->phi0;
        S->dc_g = S->derphi0;
        S->dc_task = T_START;
        S->dc_i = 0;
        S->phase = P_DC_ITER;
        break;
      }
      case P_DC_ITER: {
        dcsrch_iterate(S);
        bool fail = !isfinite_(S->dc_stp);
        if (!fail && S->dc_task == T_FG) {
          if (!want(S, S->dc_stp, P_DC_EVAL)) return kNeedEval;
          break;
        }
        fail = fail || S->dc_task == T_WARN || S->dc_task == T_ERROR;
        if (!fail) {                                    // CONVERGENCE
          S->ls_alpha = S->dc_stp;
          S->ls_fval = S->dc_f;
          if (bfgs_update(S)) return kDone;
          break;
        }
        if (!start_wolfe2(S)) return kNeedEval;
        break;
      }
      case P_DC_EVAL: {                                 // phi1 = phi(stp); derphi1 = derphi(stp)
        S->dc_f = S->fl;
        S->dc_g = dot(S->gl, S->pk, n);
        copy_n(S->gval, S->gl, n);
        S->dc_i += 1;
        S->phase = P_DC_ITER;
        if (S->dc_i >= kDcsrchIter && !start_wolfe2(S)) return kNeedEval;   // DCSRCH did not converge in 100 iterations
        break;
      }
      case P_W2_FIRST: {                                // phi_a1 = phi(alpha1)
        S->w_phi_a1 = S->fl;
        S->w_phi_a0 = S->phi0;
        S->w_dphi_a0 = S->derphi0;
        S->w_i = 0;
        S->phase = P_W2_LOOP;
        break;
      }
      case P_W2_LOOP: {
        if (S->w_i >= kWolfe2Iter) {                    // maxiter reached: alpha1, derphi_star None -> myfprime(xkp1)
          S->ls_alpha = S->w_a1;
          S->ls_fval = S->w_phi_a1;
          copy_n(S->gval, S->gl, n);
          if (bfgs_update(S)) return kDone;
          break;
        }
        if (S->w_a1 == 0.0 || S->w_a0 > kAmax) { finish(S, kStatusLineSearch); return kDone; }
        if ((S->w_phi_a1 > S->phi0 + kC1 * S->w_a1 * S->derphi0) || ((S->w_phi_a1 >= S->w_phi_a0) && S->w_i > 0)) {
          S->z_lo = S->w_a0; S->z_hi = S->w_a1; S->z_phi_lo = S->w_phi_a0; S->z_phi_hi = S->w_phi_a1;
          S->z_dphi_lo = S->w_dphi_a0;
          S->z_phi_rec = S->phi0; S->z_rec = 0.0; S->z_i = 0;
          S->phase = P_Z_LOOP;
          break;
        }
        S->w_dphi_a1 = dot(S->gl, S->pk, n);            // derphi(alpha1), at the point phi just evaluated
        copy_n(S->gval, S->gl, n);
        if (fabs_(S->w_dphi_a1) <= -kC2 * S->derphi0) {
          S->ls_alpha = S->w_a1;
          S->ls_fval = S->w_phi_a1;
          if (bfgs_update(S)) return kDone;
          break;
        }
        if (S->w_dphi_a1 >= 0.0) {
          S->z_lo = S->w_a1; S->z_hi = S->w_a0; S->z_phi_lo = S->w_phi_a1; S->z_phi_hi = S->w_phi_a0;
          S->z_dphi_lo = S->w_dphi_a1;
          S->z_phi_rec = S->phi0; S->z_rec = 0.0; S->z_i = 0;
          S->phase = P_Z_LOOP;
          break;
        }
        const double a2 = pymin(2.0 * S->w_a1, kAmax);
        S->w_a0 = S->w_a1;
        S->w_a1 = a2;
        S->w_phi_a0 = S->w_phi_a1;
        S->w_dphi_a0 = S->w_dphi_a1;
        if (!want(S, S->w_a1, P_W2_NEXT)) return kNeedEval;
        break;
      }
      case P_W2_NEXT: {
        S->w_phi_a1 = S->fl;
        S->w_i += 1;
        S->phase = P_W2_LOOP;
        break;
      }
      case P_Z_LOOP: {                                  // _zoom: the next trial step
        const double dalpha = S->z_hi - S->z_lo;
        double a, b;
        if (dalpha < 0) { a = S->z_hi; b = S->z_lo; } else { a = S->z_lo; b = S->z_hi; }
        double aj = 0.0, cchk = 0.0;
        bool ok = false;
        if (S->z_i > 0) {
          cchk = 0.2 * dalpha;
          ok = cubicmin(S->z_lo, S->z_phi_lo, S->z_dphi_lo, S->z_hi, S->z_phi_hi, S->z_rec, S->z_phi_rec, &aj);
        }
        if (S->z_i == 0 || !ok || aj > b - cchk || aj < a + cchk) {
          const double qchk = 0.1 * dalpha;
          ok = quadmin(S->z_lo, S->z_phi_lo, S->z_dphi_lo, S->z_hi, S->z_phi_hi, &aj);
          if (!ok || aj > b - qchk || aj < a + qchk) aj = S->z_lo + 0.5 * dalpha;
        }
        S->z_aj = aj;
        if (!want(S, aj, P_Z_EVAL)) return kNeedEval;
        break;
      }
      case P_Z_EVAL: {
        const double aj = S->z_aj, phi_aj = S->fl;
        if ((phi_aj > S->phi0 + kC1 * aj * S->derphi0) || (phi_aj >= S->z_phi_lo)) {
          S->z_phi_rec = S->z_phi_hi; S->z_rec = S->z_hi;
          S->z_hi = aj; S->z_phi_hi = phi_aj;
        } else {
          const double dphi_aj = dot(S->gl, S->pk, n);
          copy_n(S->gval, S->gl, n);
          if (fabs_(dphi_aj) <= -kC2 * S->derphi0) {
            S->ls_alpha = aj;
            S->ls_fval = phi_aj;
            if (bfgs_update(S)) return kDone;
            break;
          }
          if (dphi_aj * (S->z_hi - S->z_lo) >= 0) {
            S->z_phi_rec = S->z_phi_hi; S->z_rec = S->z_hi;
            S->z_hi = S->z_lo; S->z_phi_hi = S->z_phi_lo;
          } else {
            S->z_phi_rec = S->z_phi_lo; S->z_rec = S->z_lo;
          }
          S->z_lo = aj; S->z_phi_lo = phi_aj; S->z_dphi_lo = dphi_aj;
        }
        S->z_i += 1;
        if (S->z_i > kZoomIter) { finish(S, kStatusLineSearch); return kDone; }
        S->phase = P_Z_LOOP;
        break;
      }
      default:
        return kDone;
    }
  }
}

// minimize(..., x0, method='BFGS', options={gtol, maxiter}): the first point to evaluate is x0 (in S->xr).
BFGS_HD void bfgs_init(State* S, int n, const double* x0, double gtol, int maxiter) {
  S->n = n;
  S->gtol = gtol;
  S->maxiter = maxiter;
  S->phase = P_START;
  S->status = kStatusRounds;
  S->k = 0;
  S->nfev = 0;
  S->n_wolfe2 = 0;
  S->have_last = 0;
  S->gnorm = 0.0;
  S->old_fval = 0.0;
  for (int i = 0; i < n; ++i) {
    S->x[i] = x0[i];
    S->xr[i] = x0[i];
  }
}

// f at S->xr, its gradient already written to S->gl -> as bfgs_step.  The kernel fills S->gl in place: no local array.
BFGS_HD int bfgs_step_gl(State* S, double f) {
  if (S->phase == P_FINISHED) return kDone;
  for (int i = 0; i < S->n; ++i) S->xl[i] = S->xr[i];
  S->fl = f;
  S->have_last = 1;
  S->nfev += 1;
  return run(S);
}

// (f, g) at S->xr -> kNeedEval (next point in S->xr) or kDone (S->status, S->x, S->old_fval, S->k, S->nfev final).
BFGS_HD int bfgs_step(State* S, double f, const double* g) {
  if (S->phase == P_FINISHED) return kDone;
  for (int i = 0; i < S->n; ++i) S->gl[i] = g[i];
  return bfgs_step_gl(S, f);
}

#undef BFGS_HD

}  // namespace isr_bfgs
