// pislam_mappoint_math.h — the arithmetic of pislam_triangulate_batch (include/pislam_hip.h: that comment is the
// contract), stated ONCE for the device kernel (pislam_mappoint_kernels.h) and for a plain C++ compiler (tools/probes/
// mappoint_host_check.cpp): what a key-frame pair's slots share, and one slot from its two observations to the status,
// the world point, the normal and the distance range.  The closest points of the two rays and their midpoint are the
// reconstruction contract's (prm::evaluate), written out here with the two cameras apart and without its reprojection,
// which knows no bf.  Every operation is written out one rounding at a time; build with -ffp-contract=off.  The level
// tables are only ever indexed by the counter of a loop over the levels, the entry of a slot's own level is picked by a
// select, so on the device nothing goes through scratch.
#pragma once
#include "pislam_pose_math.h"

namespace pmp {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_LEVELS = 16;
constexpr int MAX_STRIDE = 16384;

// The status of a slot: the first test that failed.
enum Status : uint8_t { OK = 0, NO_LEVEL = 1, LOW_PARALLAX = 2, NOT_FINITE = 3, DEPTH1 = 4, DEPTH2 = 5, REPROJ1 = 6,
                        REPROJ2 = 7, SCALE = 8, PAIR = 9 };
// How the point of a slot was made (the probe prints it; the library does not hand it out).
enum Mode : uint8_t { NONE = 0, TRIANGULATE = 1, STEREO1 = 2, STEREO2 = 3 };

// The host tables and the parameter struct as the kernel carries them (by value: a captured graph keeps its own copy).
struct Tables {
  float level_scale[MAX_LEVELS], level_sigma2[MAX_LEVELS];
  int32_t nlevels;
};
struct Params {
  float cos_min_parallax, chi2_mono, chi2_stereo, ratio_factor;
};

PISLAM_HD bool params_ok(const Params &p) {
  return finite_f(p.cos_min_parallax) && p.chi2_mono > 0.0f && finite_f(p.chi2_mono) && p.chi2_stereo > 0.0f &&
         finite_f(p.chi2_stereo) && p.ratio_factor > 0.0f && finite_f(p.ratio_factor);
}

// Entry l < nlevels of a table, without a variable index.
PISLAM_HD float pick(const float *tab, int nlevels, int l) {
  float v = tab[0];
  for (int k = 1; k < nlevels; k++) v = k == l ? tab[k] : v;
  return v;
}

// What the slots of a pair share.
struct Pair {
  float R1[9], t1[3], R2[9], t2[3];            // the two poses, world to camera
  float c[12];                                 // R21 row-major, then t21: X2 = R21 X1 + t21
  float O1[3], O2[3];                          // the camera centres in the world
  float cam1[5], cam2[5];                      // fx, fy, cx, cy, bf
  float ifx1, ify1, ifx2, ify2, hb1, hb2;      // hb = half the stereo baseline
};

// False: a pose or camera word is not finite, or an fx or fy is 0 (every slot gets PAIR; *P is then not to be used).
PISLAM_HD bool pair_setup(const float *pose1, const float *pose2, const float *cam1, const float *cam2, Pair *P) {
  bool ok = true;
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) ok = ok && finite_f(pose1[i]) && finite_f(pose2[i]);
PISLAM_UNROLL
  for (int i = 0; i < 5; i++) ok = ok && finite_f(cam1[i]) && finite_f(cam2[i]);
  ok = ok && cam1[0] != 0.0f && cam1[1] != 0.0f && cam2[0] != 0.0f && cam2[1] != 0.0f;
PISLAM_UNROLL
  for (int i = 0; i < 9; i++) P->R1[i] = pose1[i], P->R2[i] = pose2[i];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) P->t1[i] = pose1[9 + i], P->t2[i] = pose2[9 + i];
PISLAM_UNROLL
  for (int i = 0; i < 5; i++) P->cam1[i] = cam1[i], P->cam2[i] = cam2[i];
  const float *R1 = P->R1, *R2 = P->R2, *t1 = P->t1, *t2 = P->t2;
PISLAM_UNROLL
  for (int i = 0; i < 3; i++)
PISLAM_UNROLL
    for (int j = 0; j < 3; j++)
      P->c[3 * i + j] = (R2[3 * i] * R1[3 * j] + R2[3 * i + 1] * R1[3 * j + 1]) + R2[3 * i + 2] * R1[3 * j + 2];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++)
    P->c[9 + i] = t2[i] - ((P->c[3 * i] * t1[0] + P->c[3 * i + 1] * t1[1]) + P->c[3 * i + 2] * t1[2]);
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
    P->O1[j] = -((R1[j] * t1[0] + R1[3 + j] * t1[1]) + R1[6 + j] * t1[2]);
    P->O2[j] = -((R2[j] * t2[0] + R2[3 + j] * t2[1]) + R2[6 + j] * t2[2]);
  }
  P->ifx1 = fdiv(1.0f, cam1[0]), P->ify1 = fdiv(1.0f, cam1[1]);
  P->ifx2 = fdiv(1.0f, cam2[0]), P->ify2 = fdiv(1.0f, cam2[1]);
  P->hb1 = fdiv(cam1[4], cam1[0]) * 0.5f, P->hb2 = fdiv(cam2[4], cam2[0]) * 0.5f;
  return ok;
}

// One side's observation as the slot reads it.
struct Side {
  float u, v, ur, x, y, zs, cs;                // pixels, normalised coordinates, stereo depth and parallax cosine
  bool stereo;
};
PISLAM_HD Side side_setup(const int32_t *obs, const float *cam, float ifx, float ify, float hb) {
  Side s;
  s.u = pq::obs_px(obs[0]), s.v = pq::obs_px(obs[1]), s.ur = pq::obs_px(obs[2]);
  s.x = (s.u - cam[2]) * ifx, s.y = (s.v - cam[3]) * ify;
  const float d = s.u - s.ur;
  s.stereo = obs[2] != pq::MONO && d > 0.0f;
  s.zs = fdiv(cam[4], d);
  const float zz = s.zs * s.zs, hh = hb * hb;
  s.cs = fdiv(zz - hh, zz + hh);               // cos(2 atan(hb / zs))
  return s;
}

// A frame-k point to the world: R' (X - t).
PISLAM_HD void to_world(const float *R, const float *t, const float *X, float *Xw) {
  const float e0 = X[0] - t[0], e1 = X[1] - t[1], e2 = X[2] - t[2];
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) Xw[j] = (R[j] * e0 + R[3 + j] * e1) + R[6 + j] * e2;
}

// The world point through one pose against one side's observation: 0 ok, 1 the depth is not > 0, 2 the reprojection
// error is above the side's bound.
PISLAM_HD int side_check(const float *R, const float *t, const float *cam, const Side &s, const float *Xw, float bound_mono,
                         float bound_stereo) {
  const float X = Xw[0], Y = Xw[1], Z = Xw[2];
  const float x = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
  const float y = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
  const float z = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
  if (!(z > 0.0f)) return 1;                   // a NaN fails
  const float iz = fdiv(1.0f, z);
  const float px = x * iz, py = y * iz;
  const float pu = cam[0] * px + cam[2], pv = cam[1] * py + cam[3];
  const float eu = s.u - pu, ev = s.v - pv;
  float e2 = eu * eu + ev * ev;
  if (s.stereo) {
    const float er = s.ur - (pu - cam[4] * iz);
    e2 = e2 + er * er;
  }
  return e2 <= (s.stereo ? bound_stereo : bound_mono) ? 0 : 2;   // a NaN fails
}

struct Slot {
  uint8_t status, mode;
  float xw[3], normal[3], drange[2];           // zeros unless status is OK
};

// One slot of a pair whose pair_setup returned true.
PISLAM_HD Slot slot(const Pair &P, const int32_t *obs1, const int32_t *obs2, int l1, int l2, const Tables &tab,
                    const Params &p) {
  Slot o{NO_LEVEL, NONE, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f}};
  // 1. the levels
  if (l1 >= tab.nlevels || l2 >= tab.nlevels) return o;
  // 2. the two rays and their cosine
  Side s1 = side_setup(obs1, P.cam1, P.ifx1, P.ify1, P.hb1), s2 = side_setup(obs2, P.cam2, P.ifx2, P.ify2, P.hb2);
  const float *c = P.c;
  const float x1 = s1.x, y1 = s1.y, x2 = s2.x, y2 = s2.y;
  const float bb = (x2 * x2 + y2 * y2) + 1.0f;
  const float a0 = (c[0] * x1 + c[1] * y1) + c[2];
  const float a1 = (c[3] * x1 + c[4] * y1) + c[5];
  const float a2 = (c[6] * x1 + c[7] * y1) + c[8];
  const float cs = fdiv((a0 * x2 + a1 * y2) + a2, fsqrt(((a0 * a0 + a1 * a1) + a2 * a2) * bb));
  // 3. the stereo parallax of each side (a monocular side never limits)
  const float cs1 = s1.stereo ? s1.cs : cs + 1.0f, cs2 = s2.stereo ? s2.cs : cs + 1.0f;
  // 4. the mode
  const float mn = cs2 < cs1 ? cs2 : cs1;
  float X[3], Xw[3];
  if (cs < mn && cs > 0.0f && (s1.stereo || s2.stereo || cs < p.cos_min_parallax)) {
    // 5. the midpoint of the rays' closest points, in frame 1
    o.mode = TRIANGULATE;
    const float t0 = c[9], t1 = c[10], t2 = c[11];
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
    X[0] = (z1 * x1 + h0) * 0.5f, X[1] = (z1 * y1 + h1) * 0.5f, X[2] = (z1 + h2) * 0.5f;
    to_world(P.R1, P.t1, X, Xw);
  } else if (s1.stereo && cs1 < cs2) {
    o.mode = STEREO1;
    X[0] = x1 * s1.zs, X[1] = y1 * s1.zs, X[2] = s1.zs;
    to_world(P.R1, P.t1, X, Xw);
  } else if (s2.stereo && cs2 < cs1) {
    o.mode = STEREO2;
    X[0] = x2 * s2.zs, X[1] = y2 * s2.zs, X[2] = s2.zs;
    to_world(P.R2, P.t2, X, Xw);
  } else {
    o.status = LOW_PARALLAX;
    return o;
  }
  o.status = NOT_FINITE;
  if (!(finite_f(Xw[0]) && finite_f(Xw[1]) && finite_f(Xw[2]))) return o;
  // 6, 7. depth and reprojection in both key frames
  const float sg1 = pick(tab.level_sigma2, tab.nlevels, l1), sg2 = pick(tab.level_sigma2, tab.nlevels, l2);
  const int k1 = side_check(P.R1, P.t1, P.cam1, s1, Xw, p.chi2_mono * sg1, p.chi2_stereo * sg1);
  const int k2 = side_check(P.R2, P.t2, P.cam2, s2, Xw, p.chi2_mono * sg2, p.chi2_stereo * sg2);
  o.status = k1 == 1 ? DEPTH1 : (k2 == 1 ? DEPTH2 : (k1 == 2 ? REPROJ1 : (k2 == 2 ? REPROJ2 : SCALE)));
  if (o.status != SCALE) return o;
  // 8. scale consistency
  const float e0 = Xw[0] - P.O1[0], e1 = Xw[1] - P.O1[1], e2 = Xw[2] - P.O1[2];
  const float f0 = Xw[0] - P.O2[0], f1 = Xw[1] - P.O2[1], f2 = Xw[2] - P.O2[2];
  const float d1 = fsqrt((e0 * e0 + e1 * e1) + e2 * e2), d2 = fsqrt((f0 * f0 + f1 * f1) + f2 * f2);
  const float ls1 = pick(tab.level_scale, tab.nlevels, l1), ls2 = pick(tab.level_scale, tab.nlevels, l2);
  const float r1 = d1 * ls1, r2 = d2 * ls2;
  if (d1 == 0.0f || d2 == 0.0f) return o;
  if (!((d2 * p.ratio_factor) * ls2 >= r1 && r2 <= r1 * p.ratio_factor)) return o;   // a NaN fails
  // the point, and what pislam_match_projection_batch reads of it in map mode
  o.status = OK;
  o.xw[0] = Xw[0], o.xw[1] = Xw[1], o.xw[2] = Xw[2];
  const float w0 = fdiv(e0, d1) + fdiv(f0, d2), w1 = fdiv(e1, d1) + fdiv(f1, d2), w2 = fdiv(e2, d1) + fdiv(f2, d2);
  const float wn = fsqrt((w0 * w0 + w1 * w1) + w2 * w2);
  o.normal[0] = fdiv(w0, wn), o.normal[1] = fdiv(w1, wn), o.normal[2] = fdiv(w2, wn);
  o.drange[0] = fdiv(r1, pick(tab.level_scale, tab.nlevels, tab.nlevels - 1)), o.drange[1] = r1;
  return o;
}

}  // namespace pmp
