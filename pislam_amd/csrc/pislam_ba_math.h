// pislam_ba_math.h — the arithmetic of pislam_local_ba_batch (include/pislam_hip.h: that comment is the contract), stated
// ONCE for the device kernel (pislam_ba_kernels.h) and for a plain C++ compiler (tools/probes/ba_host_check.cpp): one
// observation's terms in binary32 (the pose call's rows, pq::obs_rows, and from them the point rows), the 3 x 3 point
// blocks, the chains that build the reduced camera system, the points' back substitution and, for the host only, the
// whole call for one window run serially (pba::host_window).  The Levenberg rule is the pose call's (prf::LAMBDA_0,
// prf::lambda_down, prf::lambda_up); the retraction is pq::retract.
// Every operation is written out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_pose_math.h"

namespace pba {

using psm::finite_d;
using psm::finite_f;

constexpr int MAX_KF = 32, MAX_FREE = 16, MAX_PTS = 4096, MAX_STRIDE = prf::MAX_STRIDE, MAX_ROUNDS = 4;
constexpr int MAX_N = 6 * MAX_FREE;            // unknowns of the reduced camera system
constexpr int LDA = MAX_N + 1;                 // its row: N columns, the right-hand side at column MAX_N
constexpr int CAM = 27, CROSS = 18, PT = 9;    // stored terms of an observation (H_k 21 + g_k 6; W 6 x 3) and a point
constexpr uint16_t NO_OBS = 0xffff;

struct Params {
  int rounds, iters[MAX_ROUNDS], huber_rounds, min_obs;
  double eps;
};

// One window as the call reads it; the counts are already clamped (psm::clamp_count), nfree is kf_free as given.
struct Window {
  const float *poses, *cams, *xw;              // [nkf][12], [nkf][5], [npt][3]
  const int32_t *obs;                          // [n][3]
  const uint8_t *kf;                           // [n]
  const uint16_t *pt;                          // [n]
  const uint8_t *level;                        // [n] or null
  const float *inv_sigma2;                     // [nlevels]
  int nlevels;
  uint32_t nkf, nfree, npt, n;
};

// Observation i is in order: its key frame and point exist and it comes after observation i - 1.
PISLAM_HD bool obs_in_order(const Window &W, uint32_t i) {
  if (W.kf[i] >= W.nkf || W.pt[i] >= W.npt) return false;
  if (i == 0) return true;
  return W.pt[i] > W.pt[i - 1] || (W.pt[i] == W.pt[i - 1] && W.kf[i] > W.kf[i - 1]);
}

// The terms of one observation that is not dead: the pose call's 28 (cam[27] is rho), the 18 cross terms W (row a of
// the camera, column j of the point, at 3 a + j) and the point's 9 (V's upper triangle row by row, then g_p).
struct ObsTerms {
  float cam[pq::TERMS], cross[CROSS], pt[PT], chi2;
};

// One observation of the point Xf at the pose T under cam.  False: dead (nothing of t is meaningful).
PISLAM_HD bool obs_eval(const float *T, const float *cam, const float *Xf, float u, float v, float ur, bool stereo, float w,
                        bool robust, ObsTerms &t) {
  pq::ObsRows r;
  if (!pq::obs_rows(T, cam, Xf[0], Xf[1], Xf[2], u, v, ur, stereo, w, robust, r, &t.chi2)) return false;
  pq::row_terms(r, stereo, t.cam);
  // the rows with respect to the point: the translation part of the camera rows times R (the 0.0f entries drop out)
  float Pu[3], Pv[3], Pr[3];
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
    Pu[j] = r.Ju[3] * T[j] + r.Ju[5] * T[6 + j];
    Pv[j] = r.Jv[4] * T[3 + j] + r.Jv[5] * T[6 + j];
    Pr[j] = r.Jr[3] * T[j] + r.Jr[5] * T[6 + j];
  }
PISLAM_UNROLL
  for (int a = 0; a < 6; a++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) {
      float s = r.Ju[a] * Pu[j] + r.Jv[a] * Pv[j];
      if (stereo) s = s + r.Jr[a] * Pr[j];
      t.cross[3 * a + j] = s * r.wr;
    }
  }
  int o = 0;
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
PISLAM_UNROLL
    for (int k = j; k < 3; k++) {
      float s = Pu[j] * Pu[k] + Pv[j] * Pv[k];
      if (stereo) s = s + Pr[j] * Pr[k];
      t.pt[o++] = s * r.wr;
    }
  }
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
    float s = Pu[j] * r.eu + Pv[j] * r.ev;
    if (stereo) s = s + Pr[j] * r.er;
    t.pt[6 + j] = s * r.wr;
  }
  return true;
}

// Observation i of a pass: T and cam are its key frame's, Xf its point's.  Its active flag is set anew on
// classification.  True: it contributes (active and not dead) and t holds its terms.
PISLAM_HD bool pass_one(const Window &W, uint32_t i, const float *T, const float *cam, const float *Xf, bool classify,
                        bool robust, uint8_t *active, ObsTerms &t) {
  float w = 1.0f;
  bool dead = false;
  if (W.level) {
    const int l = W.level[i];
    if (l < W.nlevels) w = W.inv_sigma2[l];
    else dead = true;
  }
  const int32_t *o = W.obs + 3 * (size_t)i;
  const bool stereo = o[2] != pq::MONO;
  bool live = false;
  t.chi2 = 0.0f;
  if (!dead && (classify || *active))
    live = obs_eval(T, cam, Xf, pq::obs_px(o[0]), pq::obs_px(o[1]), stereo ? pq::obs_px(o[2]) : 0.0f, stereo, w, robust, t);
  if (classify) *active = live && t.chi2 <= (stereo ? pq::TH_STEREO : pq::TH_MONO);
  return live && *active;
}

// A point's damped block V' (V's diagonal times s = 1.0 + lambda) eliminated without pivoting, as pq::solve_n<3> does
// it: F = (a00, a01, a02, b11, b12, c22, f1, f2, f3).  False: a pivot that is not > 0 (a NaN fails): the point is HELD.
PISLAM_HD bool factor3(const double *V, double s, double *F) {
  const double a00 = V[0] * s, a01 = V[1], a02 = V[2], a11 = V[3] * s, a12 = V[4], a22 = V[5] * s;
  const double f1 = a01 / a00, f2 = a02 / a00;
  const double b11 = a11 - f1 * a01, b12 = a12 - f1 * a02;
  const double b21 = a12 - f2 * a01, b22 = a22 - f2 * a02;
  const double f3 = b21 / b11;
  const double c22 = b22 - f3 * b12;
  F[0] = a00, F[1] = a01, F[2] = a02, F[3] = b11, F[4] = b12, F[5] = c22, F[6] = f1, F[7] = f2, F[8] = f3;
  return a00 > 0.0 && b11 > 0.0 && c22 > 0.0;
}
// V' x = b from the factors.
PISLAM_HD void solve3(const double *F, double b0, double b1, double b2, double *x) {
  b1 = b1 - F[6] * b0;
  b2 = b2 - F[7] * b0;
  b2 = b2 - F[8] * b1;
  x[2] = b2 / F[5];
  x[1] = (b1 - F[4] * x[2]) / F[3];
  x[0] = ((b0 - F[1] * x[1]) - F[2] * x[2]) / F[0];
}

// What a pass left (one of two sets) and what an iteration made of it, as the chains below read it.
struct Store {
  const float *cam, *cross;                    // [n][CAM], [n][CROSS]: observations of free key frames that contribute
  const uint8_t *on;                           // [n]: the observation contributes
  const double *V;                             // [npt][PT]: the point sums
  const double *fac;                           // [npt][9]
  const uint8_t *held;                         // [npt]
  const double *Y;                             // [n][CROSS]: rows of W V'^-1, observations of free key frames that
                                               // contribute and whose point is not held
  const uint16_t *slot;                        // [npt][MAX_FREE]: the observation of (point, free key frame) or NO_OBS
  const uint16_t *klist;                       // the observations of free key frame k, ascending, at kstart[k] ..
  const uint32_t *kstart;                      // [nfree + 1]
  const uint16_t *pt;                          // [n]
};

// The chains below walk a key frame's list CHUNK observations at a time: the loads of a chunk do not depend on one
// another and are issued together, the sums still take the observations one by one in ascending order.
constexpr int CHUNK = 8;

// The sum t of the stored camera term `term` over key frame k's contributing observations, ascending, from +0.0.
PISLAM_HD double cam_sum(const Store &S, int k, int term) {
  double h = 0.0;
  const uint32_t e1 = S.kstart[k + 1];
  for (uint32_t e0 = S.kstart[k]; e0 < e1; e0 += CHUNK) {
    float t[CHUNK];
    bool use[CHUNK];
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++) {
      const uint32_t o = S.klist[e0 + u < e1 ? e0 + u : e0];
      use[u] = e0 + u < e1 && S.on[o];
      t[u] = S.cam[CAM * (size_t)o + term];
    }
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++)
      if (use[u]) h = h + (double)t[u];
  }
  return h;
}

// A chunk of key frame ki's list as the chains read it: the observations oi, whether each takes part (it is in the
// list, contributes and its point is not held) and its point.
struct Chunk {
  uint32_t oi[CHUNK], p[CHUNK];
  bool use[CHUNK];
};
PISLAM_HD void chunk_of(const Store &S, uint32_t e0, uint32_t e1, Chunk &c) {
PISLAM_UNROLL
  for (int u = 0; u < CHUNK; u++) c.oi[u] = S.klist[e0 + u < e1 ? e0 + u : e0];
PISLAM_UNROLL
  for (int u = 0; u < CHUNK; u++) c.use[u] = e0 + u < e1 && S.on[c.oi[u]], c.p[u] = S.pt[c.oi[u]];
PISLAM_UNROLL
  for (int u = 0; u < CHUNK; u++) c.use[u] = c.use[u] && !S.held[c.p[u]];
}

// Entry (6 ki + ai, 6 kj + aj), ki <= kj and row <= column, of the reduced camera system at s = 1.0 + lambda.
PISLAM_HD double reduced_entry(const Store &S, int ki, int ai, int kj, int aj, double s) {
  double acc = 0.0;
  if (ki == kj) {
    acc = cam_sum(S, ki, ai * 6 - ai * (ai - 1) / 2 + (aj - ai));
    if (ai == aj) acc = acc * s;
  }
  const uint32_t e1 = S.kstart[ki + 1];
  for (uint32_t e0 = S.kstart[ki]; e0 < e1; e0 += CHUNK) {
    Chunk c;
    chunk_of(S, e0, e1, c);
    uint32_t oj[CHUNK];
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++) {
      oj[u] = ki == kj ? c.oi[u] : S.slot[MAX_FREE * (size_t)c.p[u] + kj];
      if (oj[u] == NO_OBS) c.use[u] = false, oj[u] = c.oi[u];
    }
    double y[CHUNK][3];
    float w[CHUNK][3];
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++) {
      c.use[u] = c.use[u] && S.on[oj[u]];
PISLAM_UNROLL
      for (int j = 0; j < 3; j++)
        y[u][j] = S.Y[CROSS * (size_t)c.oi[u] + 3 * ai + j], w[u][j] = S.cross[CROSS * (size_t)oj[u] + 3 * aj + j];
    }
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++)
      if (c.use[u]) acc = acc - ((y[u][0] * (double)w[u][0] + y[u][1] * (double)w[u][1]) + y[u][2] * (double)w[u][2]);
  }
  return acc;
}

// Its right-hand side at row 6 ki + ai.
PISLAM_HD double reduced_rhs(const Store &S, int ki, int ai) {
  double acc = -cam_sum(S, ki, 21 + ai);
  const uint32_t e1 = S.kstart[ki + 1];
  for (uint32_t e0 = S.kstart[ki]; e0 < e1; e0 += CHUNK) {
    Chunk c;
    chunk_of(S, e0, e1, c);
    double y[CHUNK][3], g[CHUNK][3];
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++) {
PISLAM_UNROLL
      for (int j = 0; j < 3; j++)
        y[u][j] = S.Y[CROSS * (size_t)c.oi[u] + 3 * ai + j], g[u][j] = S.V[PT * (size_t)c.p[u] + 6 + j];
    }
PISLAM_UNROLL
    for (int u = 0; u < CHUNK; u++)
      if (c.use[u]) acc = acc + ((y[u][0] * g[u][0] + y[u][1] * g[u][1]) + y[u][2] * g[u][2]);
  }
  return acc;
}

// The rows of W V'^-1 of point p's observations [o0, o1) (nothing for a held point).
PISLAM_HD void point_rows(const Store &S, const uint8_t *kf, uint32_t nfree, uint32_t p, uint32_t o0, uint32_t o1, double *Y) {
  if (S.held[p]) return;
  const double *F = S.fac + 9 * (size_t)p;
  for (uint32_t o = o0; o < o1; o++) {
    if (!S.on[o] || kf[o] >= nfree) continue;
    const float *w = S.cross + CROSS * (size_t)o;
PISLAM_UNROLL
    for (int a = 0; a < 6; a++) solve3(F, (double)w[3 * a], (double)w[3 * a + 1], (double)w[3 * a + 2], Y + CROSS * (size_t)o + 3 * a);
  }
}

// Point p's step from the camera step d: dp = V'^-1 (-g_p - W_p^T d) over its observations [o0, o1), ascending.  A held
// point takes no step.  False: a word of dp is not finite.
PISLAM_HD bool point_step(const Store &S, const uint8_t *kf, uint32_t nfree, uint32_t p, uint32_t o0, uint32_t o1,
                          const double *d, double *dp) {
  dp[0] = 0.0, dp[1] = 0.0, dp[2] = 0.0;
  if (S.held[p]) return true;
  const double *g = S.V + PT * (size_t)p + 6;
  double b[3] = {-g[0], -g[1], -g[2]};
  for (uint32_t o = o0; o < o1; o++) {
    if (!S.on[o] || kf[o] >= nfree) continue;
    const float *w = S.cross + CROSS * (size_t)o;
    const double *dk = d + 6 * (size_t)kf[o];
PISLAM_UNROLL
    for (int j = 0; j < 3; j++)
      b[j] = b[j] - ((((((double)w[j] * dk[0] + (double)w[3 + j] * dk[1]) + (double)w[6 + j] * dk[2]) + (double)w[9 + j] * dk[3]) +
                      (double)w[12 + j] * dk[4]) + (double)w[15 + j] * dk[5]);
  }
  solve3(S.fac + 9 * (size_t)p, b[0], b[1], b[2], dp);
  return finite_d(dp[0]) && finite_d(dp[1]) && finite_d(dp[2]);
}

// First observation of point p: the lower bound of p in the sorted pt[0 .. n).
PISLAM_HD uint32_t first_obs(const uint16_t *pt, uint32_t n, uint32_t p) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (pt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

#if !defined(__HIPCC__)
}  // namespace pba
#include <vector>
namespace pba {
// ---- the host's serial form of the whole call for one window (the probe; never the library's hot path) --------------

struct Result {
  uint32_t ninliers, status;
  double cost;
};

// poses_out [nkf][12], xw_out [npt][3], inlier [n].
inline void host_window(const Window &W, const Params &prm, float *poses_out, float *xw_out, uint8_t *inlier, Result *R) {
  const uint32_t n = W.n, nkf = W.nkf, npt = W.npt;
  for (size_t i = 0; i < 12 * (size_t)nkf; i++) poses_out[i] = W.poses[i];
  for (size_t i = 0; i < 3 * (size_t)npt; i++) xw_out[i] = W.xw[i];
  for (uint32_t i = 0; i < n; i++) inlier[i] = 0;
  R->ninliers = 0, R->cost = 0.0;
  bool shaped = W.nfree <= (uint32_t)MAX_FREE && W.nfree <= nkf;
  for (uint32_t i = 0; i < n; i++) shaped = shaped && obs_in_order(W, i);
  if (!shaped) {
    R->status = 3;
    return;
  }
  bool fin = true;
  for (size_t i = 0; i < 12 * (size_t)nkf; i++) fin = fin && finite_f(W.poses[i]);
  for (size_t i = 0; i < 5 * (size_t)nkf; i++) fin = fin && finite_f(W.cams[i]);
  for (size_t i = 0; i < 3 * (size_t)npt; i++) fin = fin && finite_f(W.xw[i]);
  if (!fin) {
    R->status = 2;
    return;
  }
  if (n < (uint32_t)prm.min_obs) {
    R->status = 1;
    return;
  }
  const uint32_t nfree = W.nfree, N = 6 * nfree;
  // the index: a point's observations, a free key frame's observations, the observation of (point, free key frame)
  std::vector<uint32_t> pstart(npt + 1), kstart(nfree + 1, 0);
  for (uint32_t p = 0; p <= npt; p++) pstart[p] = p < npt ? first_obs(W.pt, n, p) : n;
  std::vector<uint16_t> slot((size_t)MAX_FREE * npt + 1, NO_OBS), klist(n + 1);
  for (uint32_t k = 0, e = 0; k < nfree; k++) {
    for (uint32_t i = 0; i < n; i++)
      if (W.kf[i] == k) klist[e++] = (uint16_t)i, slot[(size_t)MAX_FREE * W.pt[i] + k] = (uint16_t)i;
    kstart[k + 1] = e;
  }
  // the state, the two sets a pass fills, what an iteration makes
  std::vector<double> T(12 * (size_t)nfree + 1), Tt(T.size()), X(3 * (size_t)npt + 1), Xt(X.size());
  for (size_t i = 0; i < 12 * (size_t)nfree; i++) T[i] = (double)W.poses[i];
  for (size_t i = 0; i < 3 * (size_t)npt; i++) X[i] = (double)W.xw[i];
  std::vector<float> cam[2], cross[2];
  std::vector<uint8_t> on[2], held(npt + 1);
  std::vector<double> V[2], fac(9 * (size_t)npt + 1), Y((size_t)CROSS * n + 1), A((size_t)LDA * MAX_N), d(MAX_N);
  for (int s = 0; s < 2; s++)
    cam[s].resize((size_t)CAM * n + 1), cross[s].resize((size_t)CROSS * n + 1), on[s].resize(n + 1), V[s].resize((size_t)PT * npt + 1);
  uint8_t *active = inlier;                    // the mask is the active set
  for (uint32_t i = 0; i < n; i++) active[i] = 1;

  // One pass at (Ts, Xs) into `set`: sums = (F, the number of contributing observations, their chi2).
  auto pass = [&](const std::vector<double> &Ts, const std::vector<double> &Xs, int set, bool classify, bool robust,
                  double *sums) {
    std::vector<float> Tf(12 * (size_t)nkf + 1);
    for (size_t i = 0; i < 12 * (size_t)nkf; i++) Tf[i] = i < 12 * (size_t)nfree ? (float)Ts[i] : W.poses[i];
    double part[prf::PARTIALS][3] = {};
    for (uint32_t p = 0; p < npt; p++) {
      const float Xf[3] = {(float)Xs[3 * (size_t)p], (float)Xs[3 * (size_t)p + 1], (float)Xs[3 * (size_t)p + 2]};
      double v[PT] = {}, s[3] = {};
      for (uint32_t i = pstart[p]; i < pstart[p + 1]; i++) {
        const uint32_t k = W.kf[i];
        ObsTerms t;
        const bool c = pass_one(W, i, &Tf[12 * (size_t)k], W.cams + 5 * (size_t)k, Xf, classify, robust, &active[i], t);
        on[set][i] = c;
        if (!c) continue;
        for (int j = 0; j < PT; j++) v[j] = v[j] + (double)t.pt[j];
        s[0] = s[0] + (double)t.cam[27], s[1] = s[1] + 1.0, s[2] = s[2] + (double)t.chi2;
        if (k < nfree) {
          for (int j = 0; j < CAM; j++) cam[set][(size_t)CAM * i + j] = t.cam[j];
          for (int j = 0; j < CROSS; j++) cross[set][(size_t)CROSS * i + j] = t.cross[j];
        }
      }
      for (int j = 0; j < PT; j++) V[set][(size_t)PT * p + j] = v[j];
      for (int j = 0; j < 3; j++) part[p % prf::PARTIALS][j] += s[j];
    }
    for (int h = prf::PARTIALS / 2; h >= 1; h /= 2)
      for (int q = 0; q < h; q++)
        for (int j = 0; j < 3; j++) part[q][j] += part[q + h][j];
    for (int j = 0; j < 3; j++) sums[j] = part[0][j];
  };

  // One solve at lambda from `set`: the trial state and dmax.  False: no step at this lambda.
  auto step = [&](int set, double lambda, double *dmax) {
    const double s = 1.0 + lambda;
    for (uint32_t p = 0; p < npt; p++) held[p] = !factor3(&V[set][(size_t)PT * p], s, &fac[9 * (size_t)p]);
    const Store S{cam[set].data(), cross[set].data(), on[set].data(), V[set].data(), fac.data(), held.data(), Y.data(),
                  slot.data(), klist.data(), kstart.data(), W.pt};
    for (uint32_t p = 0; p < npt; p++) point_rows(S, W.kf, nfree, p, pstart[p], pstart[p + 1], Y.data());
    for (uint32_t i = 0; i < N; i++) {
      for (uint32_t j = i; j < N; j++)
        A[(size_t)LDA * i + j] = A[(size_t)LDA * j + i] = reduced_entry(S, i / 6, i % 6, j / 6, j % 6, s);
      A[(size_t)LDA * i + MAX_N] = reduced_rhs(S, i / 6, i % 6);
    }
    bool ok = true;
    for (uint32_t c = 0; c < N; c++) {
      ok = ok && A[(size_t)LDA * c + c] > 0.0;
      for (uint32_t r = c + 1; r < N; r++) {
        const double f = A[(size_t)LDA * r + c] / A[(size_t)LDA * c + c];
        for (uint32_t j = c + 1; j < N; j++) A[(size_t)LDA * r + j] = A[(size_t)LDA * r + j] - f * A[(size_t)LDA * c + j];
        A[(size_t)LDA * r + MAX_N] = A[(size_t)LDA * r + MAX_N] - f * A[(size_t)LDA * c + MAX_N];
      }
    }
    if (!ok) return false;
    for (uint32_t r = N; r-- > 0;) {
      d[r] = A[(size_t)LDA * r + MAX_N] / A[(size_t)LDA * r + r];
      ok = ok && finite_d(d[r]);
      for (uint32_t q = 0; q < r; q++) A[(size_t)LDA * q + MAX_N] = A[(size_t)LDA * q + MAX_N] - A[(size_t)LDA * q + r] * d[r];
    }
    double m = 0.0;
    for (uint32_t r = 0; r < N; r++) m = fmax(m, fabs(d[r]));
    for (uint32_t p = 0; p < npt; p++) {
      double dp[3];
      ok = point_step(S, W.kf, nfree, p, pstart[p], pstart[p + 1], d.data(), dp) && ok;
      for (int j = 0; j < 3; j++) Xt[3 * (size_t)p + j] = X[3 * (size_t)p + j] + dp[j], m = fmax(m, fabs(dp[j]));
    }
    if (!ok) return false;
    for (uint32_t k = 0; k < nfree; k++) pq::retract(&T[12 * (size_t)k], &d[6 * (size_t)k], &Tt[12 * (size_t)k]);
    *dmax = m;
    return true;
  };

  double sums[3], trial[3];
  uint32_t evals = 0, code = 0;
  int set = 0;
  pass(T, X, set, false, 0 < prm.huber_rounds, sums);
  evals++;
  for (int r = 0; r < prm.rounds; r++) {
    double lambda = prf::LAMBDA_0;
    for (int it = 0; it < prm.iters[r]; it++) {
      double dmax;
      if (!step(set, lambda, &dmax)) {
        lambda = prf::lambda_up(lambda);
        continue;
      }
      pass(Tt, Xt, set ^ 1, false, r < prm.huber_rounds, trial);
      evals++;
      if (trial[0] < sums[0]) {
        T = Tt, X = Xt, set ^= 1;
        for (int j = 0; j < 3; j++) sums[j] = trial[j];
        lambda = prf::lambda_down(lambda);
      } else {
        lambda = prf::lambda_up(lambda);
      }
      if (dmax <= prm.eps) break;
    }
    pass(T, X, set, true, r + 1 < prm.huber_rounds, sums);
    evals++;
    R->ninliers = (uint32_t)sums[1], R->cost = sums[2];
    if (r + 1 < prm.rounds && R->ninliers < (uint32_t)prm.min_obs) {
      code = 1;
      break;
    }
  }
  for (size_t i = 0; i < 12 * (size_t)nfree; i++) poses_out[i] = (float)T[i];
  for (size_t i = 0; i < 3 * (size_t)npt; i++) xw_out[i] = (float)X[i];
  R->status = code | evals << 8;
}
#endif

}  // namespace pba
