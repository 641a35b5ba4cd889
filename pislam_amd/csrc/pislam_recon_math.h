// pislam_recon_math.h — the arithmetic of pislam_two_view_reconstruct_batch (include/pislam_hip.h: that comment is the
// contract), stated ONCE for the device kernel (pislam_recon_kernels.h) and for a plain C++ compiler (tools/probes/
// recon_host_check.cpp): a pair's constants, a match's coordinates, one match under one candidate motion in binary32,
// the choice in integers, and, for the host only, the whole call for one pair run serially.  Every operation is written
// out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_scalar_math.h"

namespace prm {

using psm::clamp_q8;
using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_CAND = 8;
constexpr int MAX_STRIDE = 16384;
constexpr uint32_t GOOD = 1, PARALLAX = 2, POINT = 4;        // the flags of a match under a candidate

enum Code { OK = 0, FEW = 1, AMBIGUOUS = 2, LOW_PARALLAX = 3, NO_INPUT = 4 };

struct Params {
  int32_t ncand, sigma_q8;
  float cos_parallax, cos_point;
  int32_t min_good, min_good_pct, similar_pct, parallax_rank;
};

PISLAM_HD bool params_ok(const Params &p) {
  return p.ncand >= 1 && p.ncand <= MAX_CAND && p.sigma_q8 >= 1 && p.sigma_q8 <= 4096 && p.cos_parallax > 0.0f &&
         p.cos_parallax <= 1.0f && p.cos_point > 0.0f && p.cos_point <= 1.0f && p.min_good >= 1 &&
         p.min_good <= MAX_STRIDE && p.min_good_pct >= 0 && p.min_good_pct <= 100 && p.similar_pct >= 1 &&
         p.similar_pct <= 100 && p.parallax_rank >= 1 && p.parallax_rank <= MAX_STRIDE;
}

PISLAM_HD float px(int32_t q8) { return (float)clamp_q8(q8) * (1.0f / 256.0f); }   // exact

// What a pair's matches share.  False: cam is not finite, or fx == 0 or fy == 0 (code 4).
struct Pair {
  float fx, fy, cx, cy, ifx, ify, th2;
};
PISLAM_HD bool pair_setup(const float *cam, int32_t sigma_q8, Pair *P) {
  P->fx = cam[0], P->fy = cam[1], P->cx = cam[2], P->cy = cam[3];
  P->ifx = fdiv(1.0f, P->fx), P->ify = fdiv(1.0f, P->fy);
  const float sg = (float)sigma_q8 * (1.0f / 256.0f);
  P->th2 = (sg * sg) * 4.0f;
  return finite_f(P->fx) && finite_f(P->fy) && finite_f(P->cx) && finite_f(P->cy) && P->fx != 0.0f && P->fy != 0.0f;
}

struct Match {
  float u1, v1, u2, v2, x1, y1, x2, y2, bb;
};
PISLAM_HD Match match_setup(const Pair &P, int32_t xq1, int32_t yq1, int32_t xq2, int32_t yq2) {
  Match m;
  m.u1 = px(xq1), m.v1 = px(yq1), m.u2 = px(xq2), m.v2 = px(yq2);
  m.x1 = (m.u1 - P.cx) * P.ifx, m.y1 = (m.v1 - P.cy) * P.ify;
  m.x2 = (m.u2 - P.cx) * P.ifx, m.y2 = (m.v2 - P.cy) * P.ify;
  m.bb = (m.x2 * m.x2 + m.y2 * m.y2) + 1.0f;
  return m;
}

PISLAM_HD bool cand_finite(const float *c) {
  bool ok = true;
  for (int i = 0; i < 12; i++) ok = ok && finite_f(c[i]);
  return ok;
}

// One match under the candidate c (r0 .. r8, t0 .. t2, every entry finite): its flags, and in X the midpoint of the two
// rays' closest points in frame 1.
PISLAM_HD uint32_t evaluate(const float *c, const Pair &P, const Match &m, float cos_parallax, float cos_point, float *X) {
  const float x1 = m.x1, y1 = m.y1, x2 = m.x2, y2 = m.y2;
  const float t0 = c[9], t1 = c[10], t2 = c[11];
  const float a0 = (c[0] * x1 + c[1] * y1) + c[2];
  const float a1 = (c[3] * x1 + c[4] * y1) + c[5];
  const float a2 = (c[6] * x1 + c[7] * y1) + c[8];
  const float n0 = a1 - a2 * y2, n1 = a2 * x2 - a0, n2 = a0 * y2 - a1 * x2;
  const float nn = (n0 * n0 + n1 * n1) + n2 * n2;
  const float p0 = y2 * t2 - t1, p1 = t0 - x2 * t2, p2 = x2 * t1 - y2 * t0;
  const float q0 = a1 * t2 - a2 * t1, q1 = a2 * t0 - a0 * t2, q2 = a0 * t1 - a1 * t0;
  const float z1 = fdiv((p0 * n0 + p1 * n1) + p2 * n2, nn);
  const float z2 = fdiv((q0 * n0 + q1 * n1) + q2 * n2, nn);
  const float g0 = z2 * x2 - t0, g1 = z2 * y2 - t1, g2 = z2 - t2;
  const float h0 = (c[0] * g0 + c[3] * g1) + c[6] * g2;
  const float h1 = (c[1] * g0 + c[4] * g1) + c[7] * g2;
  const float h2 = (c[2] * g0 + c[5] * g1) + c[8] * g2;
  const float X0 = (z1 * x1 + h0) * 0.5f, X1 = (z1 * y1 + h1) * 0.5f, X2 = (z1 + h2) * 0.5f;
  const float Y0 = ((c[0] * X0 + c[1] * X1) + c[2] * X2) + t0;
  const float Y1 = ((c[3] * X0 + c[4] * X1) + c[5] * X2) + t1;
  const float Y2 = ((c[6] * X0 + c[7] * X1) + c[8] * X2) + t2;
  const float cs = fdiv((a0 * x2 + a1 * y2) + a2, fsqrt(((a0 * a0 + a1 * a1) + a2 * a2) * m.bb));
  X[0] = X0, X[1] = X1, X[2] = X2;
  if (!(finite_f(X0) && finite_f(X1) && finite_f(X2) && finite_f(Y0) && finite_f(Y1) && finite_f(Y2))) return 0;
  const bool is_point = cs < cos_point;                       // false for a NaN
  if ((X2 <= 0.0f || Y2 <= 0.0f) && is_point) return 0;        // a point at infinity stays, whatever its depth's sign
  const float i1 = fdiv(1.0f, X2);
  const float eu1 = m.u1 - (P.fx * (X0 * i1) + P.cx), ev1 = m.v1 - (P.fy * (X1 * i1) + P.cy);
  const float e1 = eu1 * eu1 + ev1 * ev1;
  const float i2 = fdiv(1.0f, Y2);
  const float eu2 = m.u2 - (P.fx * (Y0 * i2) + P.cx), ev2 = m.v2 - (P.fy * (Y1 * i2) + P.cy);
  const float e2 = eu2 * eu2 + ev2 * ev2;
  if (!(e1 <= P.th2 && e2 <= P.th2)) return 0;                // a NaN fails
  return GOOD | (cs < cos_parallax ? PARALLAX : 0u) | (is_point ? POINT : 0u);
}

// The choice of a pair from its integer counts: G[c] good matches and Pc[c] of them with parallax under candidate c,
// N used matches.  Returns the code; *cbest is the smallest c of the largest G.
PISLAM_HD uint32_t choose(const uint32_t *G, const uint32_t *Pc, const Params &p, uint32_t N, bool cam_ok, int *cbest) {
  uint32_t gmax = 0, g2 = 0;
  int cb = 0;
  for (int c = 0; c < p.ncand; c++)
    if (G[c] > gmax) gmax = G[c], cb = c;
  for (int c = 0; c < p.ncand; c++)
    if (c != cb && G[c] > g2) g2 = G[c];
  *cbest = cb;
  if (N == 0 || !cam_ok) return NO_INPUT;
  if (gmax < (uint32_t)p.min_good || 100u * gmax < (uint32_t)p.min_good_pct * N) return FEW;
  if (100u * g2 >= (uint32_t)p.similar_pct * gmax) return AMBIGUOUS;
  const uint32_t rank = (uint32_t)p.parallax_rank < gmax ? (uint32_t)p.parallax_rank : gmax;
  if (Pc[cb] < rank) return LOW_PARALLAX;
  return OK;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one pair (the probe; never the library's hot path) ----------------

struct PairIn {
  const int32_t *p1, *p2;                      // [n][2]
  const uint8_t *mask;                         // [n] or null
  const float *cam, *cand;                     // [4], [ncand][12]
  uint32_t n;                                  // already psm::clamp_count(count, stride)
};
struct PairOut {
  int32_t best;
  uint32_t status, ngood[MAX_CAND], npar[MAX_CAND];
  float pose[12];
};

inline void host_pair(const PairIn &I, const Params &p, PairOut *O, float *xw, uint8_t *point) {
  Pair P;
  const bool cam_ok = pair_setup(I.cam, p.sigma_q8, &P);
  uint32_t G[MAX_CAND] = {0}, Pc[MAX_CAND] = {0}, N = 0;
  for (uint32_t i = 0; i < I.n; i++) {
    point[i] = 0, xw[3 * (size_t)i] = xw[3 * (size_t)i + 1] = xw[3 * (size_t)i + 2] = 0.0f;
    if (I.mask && !I.mask[i]) continue;
    N++;
    if (!cam_ok) continue;
    const Match m = match_setup(P, I.p1[2 * (size_t)i], I.p1[2 * (size_t)i + 1], I.p2[2 * (size_t)i], I.p2[2 * (size_t)i + 1]);
    for (int c = 0; c < p.ncand; c++) {
      const float *cd = I.cand + 12 * (size_t)c;
      float X[3];
      const uint32_t f = cand_finite(cd) ? evaluate(cd, P, m, p.cos_parallax, p.cos_point, X) : 0u;
      G[c] += f & GOOD, Pc[c] += (f & PARALLAX) >> 1;
    }
  }
  int cb = 0;
  const uint32_t code = choose(G, Pc, p, N, cam_ok, &cb);
  O->status = code | (uint32_t)cb << 8, O->best = code == OK ? cb : -1;
  for (int c = 0; c < MAX_CAND; c++) O->ngood[c] = code == NO_INPUT ? 0 : G[c], O->npar[c] = code == NO_INPUT ? 0 : Pc[c];
  for (int k = 0; k < 12; k++) O->pose[k] = code == OK ? I.cand[12 * (size_t)cb + k] : 0.0f;
  if (code != OK) return;
  const float *cd = I.cand + 12 * (size_t)cb;
  for (uint32_t i = 0; i < I.n; i++) {
    if (I.mask && !I.mask[i]) continue;
    const Match m = match_setup(P, I.p1[2 * (size_t)i], I.p1[2 * (size_t)i + 1], I.p2[2 * (size_t)i], I.p2[2 * (size_t)i + 1]);
    float X[3];
    if (evaluate(cd, P, m, p.cos_parallax, p.cos_point, X) & POINT)
      point[i] = 1, xw[3 * (size_t)i] = X[0], xw[3 * (size_t)i + 1] = X[1], xw[3 * (size_t)i + 2] = X[2];
  }
}
#endif

}  // namespace prm
