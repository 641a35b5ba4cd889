// pislam_sim3_refine_math.h — the arithmetic of pislam_sim3_refine_batch (include/pislam_hip.h: that comment is the
// contract), stated ONCE for the device kernel (pislam_sim3_refine_kernels.h) and for a plain C++ compiler (tools/probes/
// sim3_refine_host_check.cpp): the two sides of a match and their 36 terms in binary32, the 7 x 7 solve, the retraction
// of a similarity in binary64, what the Levenberg rule of pislam_refine_math.h needs of the call (Rule) and, for the
// host's serial form of the whole procedure there (prf::host_refine), the pair as a Problem.  A match, its camera points
// and a side's projection are those of pislam_sim3_math.h; the elimination and the Cayley map are those of
// pislam_pose_math.h.  Every operation is written out
// one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_sim3_math.h"

namespace s3r {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int DIM = 7;                         // the increment: omega, upsilon, sigma
constexpr int TERMS = 36;                      // per side: 28 upper-triangle terms, 7 gradient terms, rho
constexpr int SUMS = 38;                       // + the number of active matches that are not dead, + their chi2
constexpr int STATE = 13;                      // R row-major, t, s
constexpr int MAX_STRIDE = pq::MAX_STRIDE;
constexpr int MAX_LEVELS = pq::MAX_LEVELS;

struct Params {
  int rounds, iters, huber_rounds, min_obs;
  float th2;
  int fixed_scale;
  double eps;
};

// sim_in, cam1, cam2 as the call accepts them.
PISLAM_HD bool sim_ok(const float *sim) {
  bool ok = sim[12] > 0.0f;
PISLAM_UNROLL
  for (int i = 0; i < STATE; i++) ok = ok && finite_f(sim[i]);
  return ok;
}

// The similarity of a pass: the binary64 state rounded, then is = 1 / s (the 14 words of s3m's stored form).
PISLAM_HD void pass_words(const double *T, float *Sf) {
PISLAM_UNROLL
  for (int i = 0; i < STATE; i++) Sf[i] = (float)T[i];
  Sf[13] = fdiv(1.0f, Sf[12]);
}

// Both sides of a match under Sf.  False: the match is dead (nothing is written).
PISLAM_HD bool sides(const float *Sf, const s3m::Cam &C1, const s3m::Cam &C2, const s3m::Match &m, s3m::Side *f, s3m::Side *b) {
  if (!m.live) return false;
  float pa[3], pb[3];
  s3m::camera_points(Sf, m, pa, pb);
  if (!s3m::side_at(C1, pa[0], pa[1], pa[2], m.u1, m.v1, m.w1, f)) return false;
  return s3m::side_at(C2, pb[0], pb[1], pb[2], m.u2, m.v2, m.w2, b);
}

// The 36 terms of a side from its two Jacobian rows, with the side's own Huber weight (delta^2 = th2).
PISLAM_HD void row_terms(const float (&Ju)[DIM], const float (&Jv)[DIM], const s3m::Side &p, float w, bool robust, float th2,
                         float *t) {
  float wr = w, rho = p.chi2;
  if (robust && p.chi2 > th2) {
    const float k = fsqrt(fdiv(th2, p.chi2));
    wr = w * k;
    rho = (p.chi2 * k) * 2.0f - th2;
  }
  int o = 0;
PISLAM_UNROLL
  for (int j = 0; j < DIM; j++) {
PISLAM_UNROLL
    for (int k = j; k < DIM; k++) t[o++] = (Ju[j] * Ju[k] + Jv[j] * Jv[k]) * wr;
  }
PISLAM_UNROLL
  for (int j = 0; j < DIM; j++) t[28 + j] = (Ju[j] * p.eu + Jv[j] * p.ev) * wr;
  t[35] = rho;
}

// The forward side (camera 1): the pose call's monocular rows, and a scale column of zeros.
PISLAM_HD void forward_terms(const s3m::Cam &C, const s3m::Side &p, float w, bool robust, float th2, float *t) {
  const float a = C.fx * p.iz, b = C.fy * p.iz;
  const float pxy = p.px * p.py;
  float Ju[DIM], Jv[DIM];
  Ju[0] = pxy * C.fx, Ju[1] = -((1.0f + p.px * p.px) * C.fx), Ju[2] = p.py * C.fx, Ju[3] = -a, Ju[4] = 0.0f, Ju[5] = p.px * a;
  Jv[0] = (1.0f + p.py * p.py) * C.fy, Jv[1] = -(pxy * C.fy), Jv[2] = -(p.px * C.fy), Jv[3] = 0.0f, Jv[4] = -b, Jv[5] = p.py * b;
  Ju[6] = 0.0f, Jv[6] = 0.0f;
  row_terms(Ju, Jv, p, w, robust, th2, t);
}

// The backward side (camera 2): db = is R'(X1 x omega - upsilon - sigma X1), column by column, through the pinhole
// derivative at b.
PISLAM_HD void backward_terms(const float *Sf, const s3m::Cam &C, const float (&X)[3], const s3m::Side &p, float w, bool robust,
                              float th2, float *t) {
  const float a = C.fx * p.iz, b = C.fy * p.iz, is = Sf[13];
  float W[DIM][3];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    const float r0 = Sf[i], r1 = Sf[3 + i], r2 = Sf[6 + i];  // column i of R
    W[0][i] = r1 * X[2] - r2 * X[1];
    W[1][i] = r2 * X[0] - r0 * X[2];
    W[2][i] = r0 * X[1] - r1 * X[0];
    W[3][i] = -r0, W[4][i] = -r1, W[5][i] = -r2;
    W[6][i] = -((r0 * X[0] + r1 * X[1]) + r2 * X[2]);
  }
  float Ju[DIM], Jv[DIM];
PISLAM_UNROLL
  for (int c = 0; c < DIM; c++) {
    const float d0 = W[c][0] * is, d1 = W[c][1] * is, d2 = W[c][2] * is;
    Ju[c] = -(a * (d0 - p.px * d2));
    Jv[c] = -(b * (d1 - p.py * d2));
  }
  row_terms(Ju, Jv, p, w, robust, th2, t);
}

// The left increment d = (omega, upsilon, sigma) on T = (R, t, s): R' = Q R, t' = k (Q t) + upsilon, s' = k s with the
// Cayley Q and k = (2 + sigma) / (2 - sigma).
PISLAM_HD void retract(const double *T, const double *d, double *Tn) {
  double Q[9];
  pq::cayley(d, Q);
  const double k = (2.0 + d[6]) / (2.0 - d[6]);
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) Tn[3 * i + j] = (Q[3 * i] * T[j] + Q[3 * i + 1] * T[3 + j]) + Q[3 * i + 2] * T[6 + j];
    Tn[9 + i] = k * ((Q[3 * i] * T[9] + Q[3 * i + 1] * T[10]) + Q[3 * i + 2] * T[11]) + d[3 + i];
  }
  Tn[12] = k * T[12];
}

// One pair as the call reads it.
struct Pair {
  const float *sim_in;                         // [13]
  s3m::Pair m;                                 // the matches as the RANSAC call reads them (b is not used)
  const uint8_t *mask;                         // [n] or null
};

// What the Levenberg rule needs of the call (prf::Lm, pislam_refine_math.h).
struct Rule {
  static constexpr int STATE = s3r::STATE, DIM = s3r::DIM, TERMS = s3r::TERMS, RHO = 35;
  bool fixed_scale;
  // A fixed scale pins sigma to 0; |sigma| < 2 keeps the scale factor of the retraction positive and finite.
  PISLAM_HD bool solve(const double *S, double lambda, double *d) const {
    return pq::solve_n<DIM>(S, lambda, d, fixed_scale) && fabs(d[6]) < 2.0;
  }
  static PISLAM_HD void retract(const double *T, const double *d, double *Tn) { s3r::retract(T, d, Tn); }
};
using Lm = prf::Lm<Rule>;

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one pair (the probe; never the library's hot path) ----------------

// The pair as prf::host_refine sees it.  A pass reads the similarity in s3m's stored form (R, t, s, 1 / s), then the
// two cameras.
struct Problem : Rule {
  static constexpr int SUMS = s3r::SUMS, BCAST = s3m::WORDS + 10;
  Pair F;
  uint32_t n;
  float th2;
  Problem(const Pair &F_, const Params &P) : Rule{P.fixed_scale != 0}, F(F_), n(F_.m.n), th2(P.th2) {}

  bool ok() const { return sim_ok(F.sim_in) && s3m::cam_ok(F.m.cam1) && s3m::cam_ok(F.m.cam2); }
  void inputs(float *in, float *W) const {
    for (int i = 0; i < STATE; i++) in[i] = F.sim_in[i], W[i] = F.sim_in[i];
    W[13] = fdiv(1.0f, W[12]);
    for (int i = 0; i < 5; i++) W[s3m::WORDS + i] = F.m.cam1[i], W[s3m::WORDS + 5 + i] = F.m.cam2[i];
  }
  static void pass_words(const double *T, float *W) { s3r::pass_words(T, W); }
  // Match i of a pass at W: its active flag (set anew on classification) and what it adds to its partial sums: the 36
  // forward terms, then the 36 backward terms, then the count, the forward chi2, the backward chi2.
  void one(const float *W, uint32_t i, bool classify, bool robust, uint8_t *active, double *a) const {
    const s3m::Pair &M = F.m;
    const s3m::Cam C1 = s3m::make_cam(W + s3m::WORDS), C2 = s3m::make_cam(W + s3m::WORDS + 5);
    s3m::Match m = s3m::match(M.x1 + 3 * (size_t)i, M.x2 + 3 * (size_t)i, M.obs1 + 3 * (size_t)i, M.obs2 + 3 * (size_t)i,
                              M.level1 ? M.level1 + i : nullptr, M.level1 ? M.level2 + i : nullptr, M.inv_sigma2, M.nlevels);
    if (F.mask && !F.mask[i]) m.live = false;
    s3m::Side f{}, b{};
    bool live = false;
    if (classify || *active) live = sides(W, C1, C2, m, &f, &b);
    if (classify) *active = live && f.chi2 <= th2 && b.chi2 <= th2;
    if (!live || !*active) return;
    float t[TERMS];
    forward_terms(C1, f, m.w1, robust, th2, t);
    for (int k = 0; k < TERMS; k++) a[k] += (double)t[k];
    backward_terms(W, C2, m.X1, b, m.w2, robust, th2, t);
    for (int k = 0; k < TERMS; k++) a[k] += (double)t[k];
    a[36] += 1.0;
    a[37] += (double)f.chi2;
    a[37] += (double)b.chi2;
  }
};
using Result = prf::Result<Problem>;

inline void host_pair(const Pair &F, const Params &P, Result *R, uint8_t *inlier) {
  prf::host_refine(Problem(F, P), P, R, inlier);
}
#endif

}  // namespace s3r
