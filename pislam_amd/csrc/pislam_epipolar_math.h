// pislam_epipolar_math.h — the geometric test of pislam_match_hamming_epipolar_batch (include/pislam_hip.h: that comment
// is the contract), stated ONCE for the device kernels (pislam_epipolar_kernels.h) and for a plain C++ compiler
// (tools/probes/epipolar_host_check.cpp): how an observation is read, the epipolar line of a query in image 2, the
// distance test of a train keypoint against it and the disc around the epipole; and, for the host only, the fundamental
// matrix and the epipole of a key-frame pair from its poses (pislam_epipolar_from_poses: binary64, stated to a
// tolerance).  Every binary32 operation is written out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_pose_math.h"

namespace pem {

using psm::finite_f;

constexpr int MAX_LEVELS = 16;

// The host tables and the parameter struct as the kernels carry them (by value: a captured graph keeps its own copy).
struct Tables {
  float level_sigma2[MAX_LEVELS], level_scale[MAX_LEVELS];
  int32_t nlevels;
};
struct Params {
  float chi2, epipole_r2;
};

PISLAM_HD bool params_ok(const Params &p) { return p.chi2 > 0.0f && p.epipole_r2 >= 0.0f; }   // a NaN fails; +inf passes

// A pair takes part when the nine words of its fundamental matrix are finite.
PISLAM_HD bool f_ok(const float *F) {
  bool ok = true;
PISLAM_UNROLL
  for (int i = 0; i < 9; i++) ok = ok && finite_f(F[i]);
  return ok;
}

// A keypoint as the matcher reads it from an observation (u, v, u_right) in Q8: the pose call's pixels, and whether it
// is monocular.
PISLAM_HD float px(int32_t q8) { return pq::obs_px(q8); }
PISLAM_HD bool mono(int32_t ur_q8) { return ur_q8 == pq::MONO; }

// The epipolar line of the query (u1, v1) in image 2: l = F' (u1, v1, 1).
struct Line {
  float a, b, c, den;
};
PISLAM_HD Line line(const float *F, float u1, float v1) {
  Line l;
  l.a = (u1 * F[0] + v1 * F[3]) + F[6];
  l.b = (u1 * F[1] + v1 * F[4]) + F[7];
  l.c = (u1 * F[2] + v1 * F[5]) + F[8];
  l.den = l.a * l.a + l.b * l.b;
  return l;
}

// The bounds of a train level: chi2 * level_sigma2[l] and epipole_r2 * level_scale[l].
PISLAM_HD float line_bound(const Params &p, const Tables &t, int l) { return p.chi2 * t.level_sigma2[l]; }
PISLAM_HD float disc_bound(const Params &p, const Tables &t, int l) { return p.epipole_r2 * t.level_scale[l]; }

// The squared distance of (u2, v2) to the line against the bound, without a division: false for a NaN and for den == 0.
PISLAM_HD bool near_line(const Line &l, float u2, float v2, float bound) {
  const float num = (l.a * u2 + l.b * v2) + l.c;
  return num * num < bound * l.den;
}

// Inside the disc around the epipole: false for an epipole that is not finite.
PISLAM_HD bool in_disc(float ex, float ey, float u2, float v2, float bound) {
  const float dx = ex - u2, dy = ey - v2;
  return dx * dx + dy * dy < bound;
}

// The geometric half of the candidate rule for a query with a line and a train keypoint on a valid level.
PISLAM_HD bool candidate(const Line &l, bool qmono, float ex, float ey, float u2, float v2, bool tmono, float lbound,
                         float dbound) {
  if (!near_line(l, u2, v2, lbound)) return false;
  return !(qmono && tmono && in_disc(ex, ey, u2, v2, dbound));
}

// ---- the host's helper: F12 and the epipole from two poses (binary64, one final rounding to binary32) ----------------

// pose: r0..r8 row-major, then t (Xc = R Xw + t); cam: fx, fy, cx, cy.  f12: x1' F12 x2 = 0 in level-0 pixels, row-major
// (ORB-SLAM's ComputeF12: K1^-T [t12]x R12 K2^-1 with R12 = R1 R2', t12 = t1 - R12 t2); epipole: the centre of camera 1
// projected into image 2, as it comes out (not finite when the centre lies in camera 2's focal plane).  False: a NULL
// pointer, an input that is not finite, or an fx or fy equal to 0.
inline bool epipolar_from_poses(const float *pose1, const float *pose2, const float *cam1, const float *cam2, float *f12,
                                float *epipole) {
  if (!pose1 || !pose2 || !cam1 || !cam2 || !f12 || !epipole) return false;
  for (int i = 0; i < 12; i++)
    if (!finite_f(pose1[i]) || !finite_f(pose2[i])) return false;
  for (int i = 0; i < 4; i++)
    if (!finite_f(cam1[i]) || !finite_f(cam2[i])) return false;
  if (cam1[0] == 0.0f || cam1[1] == 0.0f || cam2[0] == 0.0f || cam2[1] == 0.0f) return false;
  double R1[9], R2[9], t1[3], t2[3], R12[9], t12[3];
  for (int i = 0; i < 9; i++) R1[i] = pose1[i], R2[i] = pose2[i];
  for (int i = 0; i < 3; i++) t1[i] = pose1[9 + i], t2[i] = pose2[9 + i];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R12[3 * i + j] = R1[3 * i] * R2[3 * j] + R1[3 * i + 1] * R2[3 * j + 1] + R1[3 * i + 2] * R2[3 * j + 2];
  for (int i = 0; i < 3; i++) t12[i] = t1[i] - (R12[3 * i] * t2[0] + R12[3 * i + 1] * t2[1] + R12[3 * i + 2] * t2[2]);
  const double S[9] = {0.0, -t12[2], t12[1], t12[2], 0.0, -t12[0], -t12[1], t12[0], 0.0};   // [t12]x
  double E[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) E[3 * i + j] = S[3 * i] * R12[j] + S[3 * i + 1] * R12[3 + j] + S[3 * i + 2] * R12[6 + j];
  // K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]
  const double A[9] = {1.0 / cam1[0], 0.0, -(double)cam1[2] / cam1[0], 0.0, 1.0 / cam1[1], -(double)cam1[3] / cam1[1], 0.0, 0.0, 1.0};
  const double B[9] = {1.0 / cam2[0], 0.0, -(double)cam2[2] / cam2[0], 0.0, 1.0 / cam2[1], -(double)cam2[3] / cam2[1], 0.0, 0.0, 1.0};
  double AE[9];                                // K1^-T E
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) AE[3 * i + j] = A[i] * E[j] + A[3 + i] * E[3 + j] + A[6 + i] * E[6 + j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      f12[3 * i + j] = (float)(AE[3 * i] * B[j] + AE[3 * i + 1] * B[3 + j] + AE[3 * i + 2] * B[6 + j]);
  // the centre of camera 1 in camera 2: R2 (-R1' t1) + t2
  double O1[3], C[3];
  for (int j = 0; j < 3; j++) O1[j] = -(R1[j] * t1[0] + R1[3 + j] * t1[1] + R1[6 + j] * t1[2]);
  for (int i = 0; i < 3; i++) C[i] = R2[3 * i] * O1[0] + R2[3 * i + 1] * O1[1] + R2[3 * i + 2] * O1[2] + t2[i];
  epipole[0] = (float)(cam2[0] * C[0] / C[2] + cam2[2]);
  epipole[1] = (float)(cam2[1] * C[1] / C[2] + cam2[3]);
  return true;
}

}  // namespace pem
