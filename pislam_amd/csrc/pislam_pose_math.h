// pislam_pose_math.h — the arithmetic of pislam_pose_refine_batch (include/pislam_hip.h: that comment is the contract),
// stated ONCE for the device kernel (pislam_pose_kernels.h) and for a plain C++ compiler (tools/probes/
// pose_host_check.cpp): the per-observation terms in binary32, the 6 x 6 solve and the Cayley retraction in binary64,
// what the Levenberg rule of pislam_refine_math.h needs of the call (Rule) and, for the host's serial form of the whole
// procedure there (prf::host_refine), the frame as a Problem.
// Every operation is written out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_refine_math.h"

namespace pq {

using psm::fdiv;
using psm::finite_d;
using psm::finite_f;
using psm::fsqrt;

constexpr int TERMS = 28;                      // 21 upper-triangle terms, 6 gradient terms, rho
constexpr int SUMS = 30;                       // + the number of active observations that are not dead, + their chi2
constexpr int MAX_STRIDE = prf::MAX_STRIDE;
constexpr int MAX_LEVELS = 16;
constexpr float Z_MIN = 0x1p-10f;
constexpr float TH_MONO = 5.991f, TH_STEREO = 7.815f;
constexpr int32_t OBS_MAX = 1 << 22;
constexpr int32_t MONO = INT32_MIN;

PISLAM_HD int32_t clamp_obs(int32_t v) { return v < -OBS_MAX ? -OBS_MAX : (v > OBS_MAX ? OBS_MAX : v); }
PISLAM_HD float obs_px(int32_t q8) { return (float)clamp_obs(q8) * (1.0f / 256.0f); }   // exact

// What one observation leaves before its terms are formed: the Jacobian rows of the error for the left increment, the
// errors, the robust weight and rho.  (The local bundle adjustment, pislam_ba_math.h, forms more terms from them.)
struct ObsRows {
  float Ju[6], Jv[6], Jr[6], eu, ev, er, wr, rho;
};

// One observation at the pose T (r0..r8, t0..t2, already rounded to float) with the weight w.  False: dead (nothing
// is written).  Otherwise *chi2_out is the plain chi2 and o holds the rows.
PISLAM_HD bool obs_rows(const float *T, const float *cam, float X, float Y, float Z, float u, float v, float ur, bool stereo,
                        float w, bool robust, ObsRows &o, float *chi2_out) {
  const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], bf = cam[4];
  const float x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9];
  const float y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10];
  const float z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11];
  if (!(z >= Z_MIN)) return false;
  const float iz = fdiv(1.0f, z);
  const float px = x * iz, py = y * iz;
  const float pu = fx * px + cx, pv = fy * py + cy;
  const float eu = u - pu, ev = v - pv;
  float er = 0.0f;
  float e2 = eu * eu + ev * ev;
  if (stereo) {
    er = ur - (pu - bf * iz);
    e2 = e2 + er * er;
  }
  const float chi2 = e2 * w;
  if (!finite_f(chi2)) return false;
  *chi2_out = chi2;
  const float th = stereo ? TH_STEREO : TH_MONO;
  float wr = w, rho = chi2;
  if (robust && chi2 > th) {
    const float k = fsqrt(fdiv(th, chi2));
    wr = w * k;
    rho = (chi2 * k) * 2.0f - th;
  }
  const float a = fx * iz, b = fy * iz, c = bf * iz;
  const float pxy = px * py;
  float *Ju = o.Ju, *Jv = o.Jv, *Jr = o.Jr;
  Ju[0] = pxy * fx, Ju[1] = -((1.0f + px * px) * fx), Ju[2] = py * fx, Ju[3] = -a, Ju[4] = 0.0f, Ju[5] = px * a;
  Jv[0] = (1.0f + py * py) * fy, Jv[1] = -(pxy * fy), Jv[2] = -(px * fy), Jv[3] = 0.0f, Jv[4] = -b, Jv[5] = py * b;
  Jr[0] = Ju[0] - c * py, Jr[1] = Ju[1] + c * px, Jr[2] = Ju[2], Jr[3] = Ju[3], Jr[4] = 0.0f, Jr[5] = Ju[5] - c * iz;
  o.eu = eu, o.ev = ev, o.er = er, o.wr = wr, o.rho = rho;
  return true;
}

// The 28 terms t[0..27] of an observation's rows.
PISLAM_HD void row_terms(const ObsRows &r, bool stereo, float *t) {
  const float *Ju = r.Ju, *Jv = r.Jv, *Jr = r.Jr;
  const float eu = r.eu, ev = r.ev, er = r.er, wr = r.wr, rho = r.rho;
  int o = 0;
PISLAM_UNROLL
  for (int j = 0; j < 6; j++) {
PISLAM_UNROLL
    for (int k = j; k < 6; k++) {
      float s = Ju[j] * Ju[k] + Jv[j] * Jv[k];
      if (stereo) s = s + Jr[j] * Jr[k];
      t[o++] = s * wr;
    }
  }
PISLAM_UNROLL
  for (int j = 0; j < 6; j++) {
    float s = Ju[j] * eu + Jv[j] * ev;
    if (stereo) s = s + Jr[j] * er;
    t[21 + j] = s * wr;
  }
  t[27] = rho;
}

// One observation as the pose call sums it: false: dead (nothing is written).  Otherwise *chi2_out is the plain chi2
// and t[0..27] are the 28 terms.
PISLAM_HD bool obs_terms(const float *T, const float *cam, float X, float Y, float Z, float u, float v, float ur, bool stereo,
                     float w, bool robust, float *t, float *chi2_out) {
  ObsRows r;
  if (!obs_rows(T, cam, X, Y, Z, u, v, ur, stereo, w, robust, r, chi2_out)) return false;
  row_terms(r, stereo, t);
  return true;
}

// A d = -g with A = H, A_jj = H_jj * (1 + lambda); S = the N (N + 1) / 2 sums of H's upper triangle, row by row, then
// the N sums of g.  Gaussian elimination without pivoting, back substitution.  False: a pivot that is not > 0 (a NaN
// fails) or a d that is not finite.  pin_last: the last unknown is taken out first (row and column N - 1 become those
// of the identity, its right-hand side 0), so it comes out as 0.
template <int N>
PISLAM_HD bool solve_n(const double *S, double lambda, double *d, bool pin_last = false) {
  double A[N][N], b[N];
  {
    int o = 0;
PISLAM_UNROLL
    for (int j = 0; j < N; j++) {
PISLAM_UNROLL
      for (int k = j; k < N; k++) {
        A[j][k] = S[o], A[k][j] = S[o];
        o++;
      }
    }
  }
  const double s = 1.0 + lambda;
PISLAM_UNROLL
  for (int j = 0; j < N; j++) A[j][j] = A[j][j] * s, b[j] = -S[N * (N + 1) / 2 + j];
  if (pin_last) {
PISLAM_UNROLL
    for (int j = 0; j < N - 1; j++) A[j][N - 1] = 0.0, A[N - 1][j] = 0.0;
    A[N - 1][N - 1] = 1.0, b[N - 1] = 0.0;
  }
  bool ok = true;
PISLAM_UNROLL
  for (int c = 0; c < N; c++) {
    ok = ok && A[c][c] > 0.0;
PISLAM_UNROLL
    for (int r = c + 1; r < N; r++) {
      const double f = A[r][c] / A[c][c];
PISLAM_UNROLL
      for (int j = c + 1; j < N; j++) A[r][j] = A[r][j] - f * A[c][j];
      b[r] = b[r] - f * b[c];
    }
  }
PISLAM_UNROLL
  for (int r = N - 1; r >= 0; r--) {
    double t = b[r];
PISLAM_UNROLL
    for (int j = r + 1; j < N; j++) t = t - A[r][j] * d[j];
    d[r] = t / A[r][r];
    ok = ok && finite_d(d[r]);
  }
  return ok;
}

// The Cayley map of the rotation vector d[0..2]: Q = ((1 - n) I + 2 a a' + 2 [a]x) / (1 + n) with a = d / 2, n = a'a.
PISLAM_HD void cayley(const double *d, double *Q) {
  const double a0 = d[0] * 0.5, a1 = d[1] * 0.5, a2 = d[2] * 0.5;
  const double n = (a0 * a0 + a1 * a1) + a2 * a2;
  const double m = 1.0 - n, den = 1.0 + n;
  Q[0] = (m + 2.0 * (a0 * a0)) / den, Q[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den, Q[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  Q[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den, Q[4] = (m + 2.0 * (a1 * a1)) / den, Q[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  Q[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den, Q[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den, Q[8] = (m + 2.0 * (a2 * a2)) / den;
}

// The Cayley retraction of T by d = (omega, upsilon): R' = Q R, t' = Q t + upsilon.
PISLAM_HD void retract(const double *T, const double *d, double *Tn) {
  double Q[9];
  cayley(d, Q);
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) Tn[3 * i + j] = (Q[3 * i] * T[j] + Q[3 * i + 1] * T[3 + j]) + Q[3 * i + 2] * T[6 + j];
    Tn[9 + i] = ((Q[3 * i] * T[9] + Q[3 * i + 1] * T[10]) + Q[3 * i + 2] * T[11]) + d[3 + i];
  }
}

// One frame as the call reads it.
struct Frame {
  const float *pose_in, *cam, *xw;             // [12], [5], [n][3]
  const int32_t *obs;                          // [n][3]
  const uint8_t *level;                        // [n] or null
  const float *inv_sigma2;                     // [nlevels] or null with level == null
  int nlevels;
  uint32_t n;                                  // already psm::clamp_count(count, stride)
};

using Params = prf::Params;

// What the Levenberg rule needs of the call (prf::Lm, pislam_refine_math.h).
struct Rule {
  static constexpr int STATE = 12, DIM = 6, TERMS = pq::TERMS, RHO = 27;
  static PISLAM_HD bool solve(const double *S, double lambda, double *d) { return solve_n<6>(S, lambda, d); }
  static PISLAM_HD void retract(const double *T, const double *d, double *Tn) { pq::retract(T, d, Tn); }
};
using Lm = prf::Lm<Rule>;

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one frame (the probe; never the library's hot path) ---------------

// The frame as prf::host_refine sees it.  A pass reads the pose, then the camera.
struct Problem : Rule {
  static constexpr int SUMS = pq::SUMS, BCAST = 12 + 5;
  Frame F;
  uint32_t n;
  explicit Problem(const Frame &F_) : F(F_), n(F_.n) {}

  bool ok() const {
    bool fin = true;
    for (int i = 0; i < 12; i++) fin = fin && finite_f(F.pose_in[i]);
    for (int i = 0; i < 5; i++) fin = fin && finite_f(F.cam[i]);
    return fin;
  }
  void inputs(float *in, float *W) const {
    for (int i = 0; i < 12; i++) in[i] = F.pose_in[i], W[i] = F.pose_in[i];
    for (int i = 0; i < 5; i++) W[12 + i] = F.cam[i];
  }
  static void pass_words(const double *T, float *W) {
    for (int i = 0; i < 12; i++) W[i] = (float)T[i];
  }
  // Observation i of a pass at W: its active flag (set anew on classification) and what it adds to its partial sums:
  // the 28 terms, then the count, then chi2.
  void one(const float *W, uint32_t i, bool classify, bool robust, uint8_t *active, double *a) const {
    float w = 1.0f;
    bool dead = false;
    if (F.level) {
      if (F.level[i] < F.nlevels) w = F.inv_sigma2[F.level[i]];
      else dead = true;
    }
    const int32_t *o = F.obs + 3 * (size_t)i;
    const float *X = F.xw + 3 * (size_t)i;
    const bool stereo = o[2] != MONO;
    float t[TERMS], chi2 = 0.0f;
    bool live = false;
    if (!dead && (classify || *active))
      live = obs_terms(W, W + 12, X[0], X[1], X[2], obs_px(o[0]), obs_px(o[1]), stereo ? obs_px(o[2]) : 0.0f, stereo, w,
                       robust, t, &chi2);
    if (classify) *active = live && chi2 <= (stereo ? TH_STEREO : TH_MONO);
    if (!live || !*active) return;
    for (int k = 0; k < TERMS; k++) a[k] += (double)t[k];
    a[28] += 1.0;
    a[29] += (double)chi2;
  }
};
using Result = prf::Result<Problem>;

inline void host_frame(const Frame &F, const Params &P, Result *R, uint8_t *inlier) {
  prf::host_refine(Problem(F), P, R, inlier);
}
#endif

}  // namespace pq
