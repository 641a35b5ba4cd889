// pislam_sim3_math.h — the arithmetic of pislam_sim3_ransac_batch (include/pislam_hip.h: that comment is the contract),
// stated ONCE for the device kernel (pislam_sim3_kernels.h) and for a plain C++ compiler (tools/probes/
// sim3_host_check.cpp): the camera test, a match as the call reads it, Horn's closed-form absolute orientation on three
// points with its 4 x 4 eigenvector by cyclic Jacobi, the two-sided chi2 and score of a match under a similarity, the
// pair as the RANSAC skeleton sees it (pislam_ransac_math.h) and, for the host only, the whole call for one pair run
// serially.  The sampler and the observation's constants are those of pislam_geom_math.h and pislam_pose_math.h.
// Every operation is written out one rounding at a time; build with -ffp-contract=off.  Static indices only: the Jacobi
// pivots are template parameters and the choice of the eigenvector is a running best, so on the device the solver
// stays in VGPRs.
#pragma once
#include "pislam_geom_math.h"
#include "pislam_pose_math.h"

namespace s3m {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_HYP = pgm::MAX_HYP;
constexpr int MAX_STRIDE = pq::MAX_STRIDE;
constexpr int MAX_LEVELS = pq::MAX_LEVELS;
constexpr int SAMPLE = 3;
constexpr int SWEEPS = 4;                      // cyclic Jacobi sweeps, all of them taken
constexpr float TH = 9.210f;                   // chi-square, 2 degrees of freedom, 1 % (ORB-SLAM's Sim3Solver)
constexpr int WORDS = 14;                      // a hypothesis: R row-major, t, s, is = 1 / s
constexpr int OUT_WORDS = 13;                  // sim_out: R row-major, t, s

// A camera as the scoring uses it.  bf is read for the finiteness test only.
struct Cam {
  float fx, fy, cx, cy;
};
PISLAM_HD bool cam_ok(const float *cam) {
  bool ok = cam[0] != 0.0f && cam[1] != 0.0f;
PISLAM_UNROLL
  for (int i = 0; i < 5; i++) ok = ok && finite_f(cam[i]);
  return ok;
}
PISLAM_HD Cam make_cam(const float *cam) { return Cam{cam[0], cam[1], cam[2], cam[3]}; }

// A match as the call reads it.  live: both levels have a weight (always, without the level arrays).
struct Match {
  float X1[3], X2[3], u1, v1, u2, v2, w1, w2;
  bool live;
};
PISLAM_HD Match match(const float *x1, const float *x2, const int32_t *q1, const int32_t *q2, const uint8_t *level1,
                      const uint8_t *level2, const float *inv_sigma2, int nlevels) {
  Match m;
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) m.X1[i] = x1[i], m.X2[i] = x2[i];
  m.u1 = pq::obs_px(q1[0]), m.v1 = pq::obs_px(q1[1]);
  m.u2 = pq::obs_px(q2[0]), m.v2 = pq::obs_px(q2[1]);
  m.w1 = 1.0f, m.w2 = 1.0f, m.live = true;
  if (level1) {
    const int l1 = *level1, l2 = *level2;
    m.live = l1 < nlevels && l2 < nlevels;
    if (m.live) m.w1 = inv_sigma2[l1], m.w2 = inv_sigma2[l2];
  }
  return m;
}

PISLAM_HD float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One Jacobi rotation of the symmetric a on the pivot (P, Q), accumulated into the columns of v.
template <int P, int Q>
PISLAM_HD void jacobi(float (&a)[4][4], float (&v)[4][4]) {
  const float apq = a[P][Q];
  if (apq == 0.0f) return;
  const float th = fdiv(a[Q][Q] - a[P][P], 2.0f * apq);
  const float den = fabsf(th) + fsqrt(th * th + 1.0f);       // th * th = inf for a tiny pivot: t = 0, the identity
  const float t = fdiv(th >= 0.0f ? 1.0f : -1.0f, den);
  const float c = fdiv(1.0f, fsqrt(t * t + 1.0f));
  const float s = t * c;
PISLAM_UNROLL
  for (int k = 0; k < 4; k++) {                              // the columns P and Q
    const float x = a[k][P], y = a[k][Q];
    a[k][P] = c * x - s * y, a[k][Q] = s * x + c * y;
  }
PISLAM_UNROLL
  for (int k = 0; k < 4; k++) {                              // the rows P and Q
    const float x = a[P][k], y = a[Q][k];
    a[P][k] = c * x - s * y, a[Q][k] = s * x + c * y;
  }
PISLAM_UNROLL
  for (int k = 0; k < 4; k++) {
    const float x = v[k][P], y = v[k][Q];
    v[k][P] = c * x - s * y, v[k][Q] = s * x + c * y;
  }
}

// The similarity X1 = s R X2 + t of three matches (Horn 1987): S = (R row-major, t, s, 1 / s).  False: invalid.
PISLAM_HD bool solve(const Match &m0, const Match &m1, const Match &m2, bool fixed_scale, float (&S)[WORDS]) {
  float O1[3], O2[3], p1[3][3], p2[3][3];                    // p[j] = the centred point of draw j
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    O1[i] = fdiv((m0.X1[i] + m1.X1[i]) + m2.X1[i], 3.0f);
    O2[i] = fdiv((m0.X2[i] + m1.X2[i]) + m2.X2[i], 3.0f);
    p1[0][i] = m0.X1[i] - O1[i], p1[1][i] = m1.X1[i] - O1[i], p1[2][i] = m2.X1[i] - O1[i];
    p2[0][i] = m0.X2[i] - O2[i], p2[1][i] = m1.X2[i] - O2[i], p2[2][i] = m2.X2[i] - O2[i];
  }
  float M[3][3];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) M[i][j] = (p2[0][i] * p1[0][j] + p2[1][i] * p1[1][j]) + p2[2][i] * p1[2][j];
  }
  float a[4][4], v[4][4];
  a[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  a[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  a[2][2] = (M[1][1] - M[0][0]) - M[2][2];
  a[3][3] = (M[2][2] - M[0][0]) - M[1][1];
  a[0][1] = a[1][0] = M[1][2] - M[2][1];
  a[0][2] = a[2][0] = M[2][0] - M[0][2];
  a[0][3] = a[3][0] = M[0][1] - M[1][0];
  a[1][2] = a[2][1] = M[0][1] + M[1][0];
  a[1][3] = a[3][1] = M[2][0] + M[0][2];
  a[2][3] = a[3][2] = M[1][2] + M[2][1];
PISLAM_UNROLL
  for (int i = 0; i < 4; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0f : 0.0f;
  }
  for (int sweep = 0; sweep < SWEEPS; sweep++) {
    jacobi<0, 1>(a, v), jacobi<0, 2>(a, v), jacobi<0, 3>(a, v);
    jacobi<1, 2>(a, v), jacobi<1, 3>(a, v), jacobi<2, 3>(a, v);
  }
  float d = a[0][0], q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
PISLAM_UNROLL
  for (int j = 1; j < 4; j++) {
    const bool take = a[j][j] > d;                           // strict: the lowest index wins a tie
    d = take ? a[j][j] : d;
PISLAM_UNROLL
    for (int i = 0; i < 4; i++) q[i] = take ? v[i][j] : q[i];
  }
  const float rn = fdiv(1.0f, fsqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]));
  const float w = q[0] * rn, x = q[1] * rn, y = q[2] * rn, z = q[3] * rn;
  const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  const float xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  float R[3][3];
  R[0][0] = ((ww + xx) - yy) - zz, R[0][1] = 2.0f * (xy - wz), R[0][2] = 2.0f * (xz + wy);
  R[1][0] = 2.0f * (xy + wz), R[1][1] = ((ww - xx) + yy) - zz, R[1][2] = 2.0f * (yz - wx);
  R[2][0] = 2.0f * (xz - wy), R[2][1] = 2.0f * (yz + wx), R[2][2] = ((ww - xx) - yy) + zz;
  float s = 1.0f;
  if (!fixed_scale) {
    float g[3][3];                                           // g[j] = R p2[j]
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) {
PISLAM_UNROLL
      for (int i = 0; i < 3; i++) g[j][i] = (R[i][0] * p2[j][0] + R[i][1] * p2[j][1]) + R[i][2] * p2[j][2];
    }
    const float nom = (dot3(p1[0], g[0]) + dot3(p1[1], g[1])) + dot3(p1[2], g[2]);
    const float den = (dot3(p2[0], p2[0]) + dot3(p2[1], p2[1])) + dot3(p2[2], p2[2]);
    s = fdiv(nom, den);
  }
  bool ok = s > 0.0f && finite_f(s);
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) S[3 * i + j] = R[i][j], ok = ok && finite_f(R[i][j]);
    S[9 + i] = O1[i] - s * ((R[i][0] * O2[0] + R[i][1] * O2[1]) + R[i][2] * O2[2]);
    ok = ok && finite_f(S[9 + i]);
  }
  S[12] = s, S[13] = fdiv(1.0f, s);
  return ok;
}

// Hypothesis k of pair b.  fetch(i) is match i of the pair.
template <class FETCH>
PISLAM_HD bool hypothesis(const FETCH &fetch, uint32_t n, uint32_t seed, uint32_t b, uint32_t k, bool fixed_scale,
                          float (&S)[WORDS]) {
  uint32_t draw[SAMPLE];
  pgm::sample<SAMPLE>(seed, b, k, n, draw);
  return solve(fetch(draw[0]), fetch(draw[1]), fetch(draw[2]), fixed_scale, S);
}

// The pixel (u, v) against the projection of the camera point (x, y, z): the pose call's monocular arithmetic, with the
// intermediates a Jacobian needs (pislam_sim3_refine_math.h).  False: dead (nothing is written).
struct Side {
  float iz, px, py, eu, ev, chi2;
};
PISLAM_HD bool side_at(const Cam &C, float x, float y, float z, float u, float v, float w, Side *out) {
  if (!(z >= pq::Z_MIN)) return false;
  const float iz = fdiv(1.0f, z);
  const float px = x * iz, py = y * iz;
  const float pu = C.fx * px + C.cx, pv = C.fy * py + C.cy;
  const float eu = u - pu, ev = v - pv;
  const float chi2 = (eu * eu + ev * ev) * w;
  if (!finite_f(chi2)) return false;
  *out = Side{iz, px, py, eu, ev, chi2};
  return true;
}
PISLAM_HD bool chi2_at(const Cam &C, float x, float y, float z, float u, float v, float w, float *chi2_out) {
  Side s;
  if (!side_at(C, x, y, z, u, v, w, &s)) return false;
  *chi2_out = s.chi2;
  return true;
}

// The two camera points of a match under S = (R, t, s, 1 / s): a = s (R X2) + t in camera 1, b = (R'(X1 - t)) / s in
// camera 2.
PISLAM_HD void camera_points(const float *S, const Match &m, float (&a)[3], float (&b)[3]) {
  float d[3];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    a[i] = S[12] * ((S[3 * i] * m.X2[0] + S[3 * i + 1] * m.X2[1]) + S[3 * i + 2] * m.X2[2]) + S[9 + i];
    d[i] = m.X1[i] - S[9 + i];
  }
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) b[i] = ((S[i] * d[0] + S[3 + i] * d[1]) + S[6 + i] * d[2]) * S[13];
}

// What one match adds to a hypothesis's score; *inl = it is an inlier.
PISLAM_HD uint32_t score(const float (&S)[WORDS], const Cam &C1, const Cam &C2, const Match &m, bool *inl) {
  *inl = false;
  if (!m.live) return 0u;
  float a[3], b[3];
  camera_points(S, m, a, b);
  float c1 = 0.0f, c2 = 0.0f;
  if (!chi2_at(C1, a[0], a[1], a[2], m.u1, m.v1, m.w1, &c1)) return 0u;
  if (!chi2_at(C2, b[0], b[1], b[2], m.u2, m.v2, m.w2, &c2)) return 0u;
  if (!(c1 < TH && c2 < TH)) return 0u;
  *inl = true;
  return (uint32_t)floorf((TH - c1) * 256.0f) + (uint32_t)floorf((TH - c2) * 256.0f);
}

// One pair as the call reads it.
struct Pair {
  const float *cam1, *cam2, *x1, *x2;          // [5], [5], [n][3], [n][3]
  const int32_t *obs1, *obs2;                  // [n][3]
  const uint8_t *level1, *level2;              // [n] or both null
  const float *inv_sigma2;                     // [nlevels] or null without levels
  int nlevels;
  uint32_t n;                                  // already psm::clamp_count(count, stride)
  uint32_t b;                                  // the pair's index in the batch: the sampler hashes it
};

// The pair as the RANSAC skeleton sees it (pislam_ransac_math.h).
struct Problem {
  static constexpr int WORDS = s3m::WORDS;
  using Item = Match;
  Pair F;
  Cam C1, C2;
  uint32_t seed, n;
  bool fixed_scale, cam_ok, have;
  PISLAM_HD Problem(const Pair &F_, uint32_t seed_, bool fixed_scale_)
      : F(F_), seed(seed_), n(F_.n), fixed_scale(fixed_scale_) {
    float cam1[5], cam2[5];
PISLAM_UNROLL
    for (int i = 0; i < 5; i++) cam1[i] = F.cam1[i], cam2[i] = F.cam2[i];
    cam_ok = s3m::cam_ok(cam1) && s3m::cam_ok(cam2), C1 = make_cam(cam1), C2 = make_cam(cam2);
    have = cam_ok && n >= (uint32_t)SAMPLE;
  }
  PISLAM_HD Match item(uint32_t i) const {
    return match(F.x1 + 3 * (size_t)i, F.x2 + 3 * (size_t)i, F.obs1 + 3 * (size_t)i, F.obs2 + 3 * (size_t)i,
                 F.level1 ? F.level1 + i : nullptr, F.level1 ? F.level2 + i : nullptr, F.inv_sigma2, F.nlevels);
  }
  PISLAM_HD bool hypothesis(uint32_t k, float (&S)[WORDS]) const {
    const Problem &P = *this;
    return s3m::hypothesis([&P](uint32_t i) { return P.item(i); }, n, seed, F.b, k, fixed_scale, S);
  }
  PISLAM_HD uint32_t score(const float (&S)[WORDS], const Match &m, bool *inl) const {
    return s3m::score(S, C1, C2, m, inl);
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one pair (the probe; never the library's hot path) ----------------

struct Result {
  int32_t best;
  uint32_t score, ninliers, status;
  float sim[OUT_WORDS];
};

inline void host_pair(const Pair &F, int hypotheses, uint32_t seed, int min_inliers, bool fixed_scale, Result *R,
                      uint8_t *inlier) {
  const Problem P(F, seed, fixed_scale);
  float S[WORDS] = {0};
  const prk::Outcome O = prk::host_ransac(P, hypotheses, S, inlier);
  R->best = O.best, R->score = O.score, R->ninliers = O.ninliers, R->status = prk::status(O, P.cam_ok, min_inliers);
  for (int i = 0; i < OUT_WORDS; i++) R->sim[i] = O.best < 0 ? 0.0f : S[i];
}
#endif

}  // namespace s3m
