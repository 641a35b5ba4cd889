// pislam_refine_math.h — what pislam_pose_refine_batch and pislam_sim3_refine_batch share, for the device and for a
// plain C++ compiler: the parameters, the Levenberg rule of one round as a state machine (prf::Lm: lane 0 of both
// kernels and the host run it) and, for the host only, one pass with the contract's tree order and the whole call for
// one element run serially (prf::host_refine, the probes under tools/probes).  A call's *_math.h supplies a RULE:
//   STATE, DIM, TERMS, RHO the words of the state (12 or 13) and of the increment (6 or 7), the sums the rule reads (the
//                          upper triangle, the gradient, rho at index RHO = TERMS - 1)
//   solve(S, lambda, d)    the damped normal equations; false: no step at this lambda
//   retract(T, d, Tt)      the state T moved by the increment d
// and, for the host's driver, a PROBLEM derived from it:
//   SUMS, BCAST            all the sums of a pass (TERMS, the count of active items that are not dead, their chi2); the
//                          floats a pass reads beside the items (pass_words' words, then the call's cameras)
//   n, ok()                the element's clamped count; the inputs pass the call's finiteness and sign tests
//   inputs(in, W)          the state as the call received it, and the BCAST floats of the first pass
//   pass_words(T, W)       the binary64 state as the floats of a pass
//   one(W, i, classify, robust, &active, acc)
//                          item i at W: its active flag, set anew on classification, and what it then adds to acc
// Every operation of the rule is written out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_scalar_math.h"

namespace prf {

constexpr int PARTIALS = 256;
constexpr int MAX_STRIDE = 16384;
constexpr double LAMBDA_0 = 0x1p-10, LAMBDA_MIN = 0x1p-30, LAMBDA_MAX = 0x1p20;

struct Params {
  int rounds, iters, huber_rounds, min_obs;
  double eps;
};

// The damping of the Levenberg rule: down after a step that lowered F, up after one that did not or a failed solve.
PISLAM_HD double lambda_down(double lambda) { return fmax(lambda * 0.25, LAMBDA_MIN); }
PISLAM_HD double lambda_up(double lambda) { return fmin(8.0 * lambda, LAMBDA_MAX); }

// The Levenberg rule of one round, as a state machine around the passes over the items: begin() takes the sums at the
// round's state, next() asks for the next trial state (false: the round is over), trial() takes the sums at it.
template <class RULE>
struct Lm {
  static constexpr int STATE = RULE::STATE, DIM = RULE::DIM, TERMS = RULE::TERMS, RHO = RULE::RHO;
  double T[STATE], Tt[STATE], S[TERMS];
  double lambda, dmax;
  int it;
  bool over;

  PISLAM_HD void begin(const double *sums) {
PISLAM_UNROLL
    for (int i = 0; i < TERMS; i++) S[i] = sums[i];
    lambda = LAMBDA_0, it = 0, over = false;
  }
  PISLAM_HD bool next(const RULE &R, int iters) {
    while (!over && it < iters) {
      it++;
      double d[DIM];
      if (!R.solve(S, lambda, d)) {
        lambda = lambda_up(lambda);
        continue;
      }
      RULE::retract(T, d, Tt);
      dmax = 0.0;
PISLAM_UNROLL
      for (int j = 0; j < DIM; j++) dmax = fmax(dmax, fabs(d[j]));
      return true;
    }
    return false;
  }
  PISLAM_HD void trial(const double *sums, double eps) {
    if (sums[RHO] < S[RHO]) {
PISLAM_UNROLL
      for (int i = 0; i < STATE; i++) T[i] = Tt[i];
PISLAM_UNROLL
      for (int i = 0; i < TERMS; i++) S[i] = sums[i];
      lambda = lambda_down(lambda);
    } else {
      lambda = lambda_up(lambda);
    }
    if (dmax <= eps) over = true;
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one element (the probes; never the library's hot path) ------------

template <class PROBLEM>
struct Result {
  float state[PROBLEM::STATE];
  uint32_t ninliers, status;
  double cost;
};

// One pass: the SUMS sums at W in the contract's tree order.  classify: the active flags (and `inlier`) are set anew.
template <class PROBLEM>
inline void host_pass(const PROBLEM &P, const float (&W)[PROBLEM::BCAST], bool classify, bool robust, uint8_t *active,
                      double *sums) {
  constexpr int SUMS = PROBLEM::SUMS;
  static thread_local double p[PARTIALS][SUMS];
  for (int q = 0; q < PARTIALS; q++)
    for (int t = 0; t < SUMS; t++) p[q][t] = 0.0;
  for (uint32_t i = 0; i < P.n; i++) P.one(W, i, classify, robust, &active[i], p[i % PARTIALS]);
  for (int h = PARTIALS / 2; h >= 1; h /= 2)
    for (int q = 0; q < h; q++)
      for (int t = 0; t < SUMS; t++) p[q][t] += p[q + h][t];
  for (int t = 0; t < SUMS; t++) sums[t] = p[0][t];
}

template <class PROBLEM, class PARAMS>
inline void host_refine(const PROBLEM &P, const PARAMS &prm, Result<PROBLEM> *R, uint8_t *inlier) {
  constexpr int STATE = PROBLEM::STATE, SUMS = PROBLEM::SUMS;
  float in[STATE], W[PROBLEM::BCAST];
  P.inputs(in, W);
  for (uint32_t i = 0; i < P.n; i++) inlier[i] = 0;
  for (int i = 0; i < STATE; i++) R->state[i] = in[i];
  R->ninliers = 0, R->cost = 0.0;
  if (!P.ok()) {
    R->status = 2;
    return;
  }
  if (P.n < (uint32_t)prm.min_obs) {
    R->status = 1;
    return;
  }
  Lm<typename PROBLEM::Rule> L;
  double sums[SUMS];
  uint32_t evals = 0, code = 0;
  for (int i = 0; i < STATE; i++) L.T[i] = (double)in[i];
  uint8_t *active = inlier;                    // the mask is the active set
  for (uint32_t i = 0; i < P.n; i++) active[i] = 1;
  host_pass(P, W, false, 0 < prm.huber_rounds, active, sums);
  evals++;
  for (int r = 0; r < prm.rounds; r++) {
    L.begin(sums);
    while (L.next(P, prm.iters)) {
      PROBLEM::pass_words(L.Tt, W);
      host_pass(P, W, false, r < prm.huber_rounds, active, sums);
      evals++;
      L.trial(sums, prm.eps);
    }
    PROBLEM::pass_words(L.T, W);
    host_pass(P, W, true, r + 1 < prm.huber_rounds, active, sums);
    evals++;
    R->ninliers = (uint32_t)sums[SUMS - 2], R->cost = sums[SUMS - 1];
    if (r + 1 < prm.rounds && R->ninliers < (uint32_t)prm.min_obs) {
      code = 1;
      break;
    }
  }
  for (int i = 0; i < STATE; i++) R->state[i] = (float)L.T[i];
  R->status = code | evals << 8;
}
#endif

}  // namespace prf
