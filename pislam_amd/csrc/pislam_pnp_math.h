// pislam_pnp_math.h — the arithmetic of pislam_pnp_ransac_batch (include/pislam_hip.h: that comment is the contract),
// stated ONCE for the device kernel (pislam_pnp_kernels.h) and for a plain C++ compiler (tools/probes/
// pnp_host_check.cpp): the camera test, an observation as the call reads it, its chi2 and score under a pose, the
// bearing, the P3P solver (Lambda Twist: Persson & Nordberg, ECCV 2018) with the choice among its solutions, the frame
// as the RANSAC skeleton sees it (pislam_ransac_math.h) and, for the host only, the whole call for one frame run
// serially.  The sampler and the observation's constants are those of pislam_geom_math.h and pislam_pose_math.h.
// Every operation is written out one rounding at a time; build with -ffp-contract=off.  Static indices only: the solver
// keeps a running best over its (at most four) solutions and never indexes an array with a runtime value, so on the
// device it stays in VGPRs.
#pragma once
#include "pislam_geom_math.h"
#include "pislam_pose_math.h"

namespace pnm {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_HYP = pgm::MAX_HYP;
constexpr int MAX_STRIDE = pq::MAX_STRIDE;
constexpr int MAX_LEVELS = pq::MAX_LEVELS;
constexpr int SAMPLE = 4;                      // draws 0..2 make the minimal problem, draw 3 chooses among its solutions
constexpr int NEWTON = 12;                     // steps on the cubic, all of them taken
constexpr int REFINE = 5;                      // Gauss-Newton steps on the depths, all of them taken
constexpr float TH = pq::TH_MONO;

// The camera as the solver and the scoring use it.  bf is read for the finiteness test only.
struct Cam {
  float fx, fy, cx, cy, ifx, ify;
};
PISLAM_HD bool cam_ok(const float *cam) {
  bool ok = cam[0] != 0.0f && cam[1] != 0.0f;
PISLAM_UNROLL
  for (int i = 0; i < 5; i++) ok = ok && finite_f(cam[i]);
  return ok;
}
PISLAM_HD Cam make_cam(const float *cam) {
  return Cam{cam[0], cam[1], cam[2], cam[3], fdiv(1.0f, cam[0]), fdiv(1.0f, cam[1])};
}

// An observation as the call reads it.  live: its level has a weight (always, without a level table).
struct Obs {
  float X, Y, Z, u, v, w;
  bool live;
};
PISLAM_HD Obs obs(const float *xw, const int32_t *q8, const uint8_t *level, const float *inv_sigma2, int nlevels) {
  Obs o;
  o.X = xw[0], o.Y = xw[1], o.Z = xw[2];
  o.u = pq::obs_px(q8[0]), o.v = pq::obs_px(q8[1]);
  o.w = 1.0f, o.live = true;
  if (level) {
    const int l = *level;
    o.live = l < nlevels;
    if (o.live) o.w = inv_sigma2[l];
  }
  return o;
}

// chi2 of one observation under the pose T (r0..r8 row-major, then t): the pose call's monocular arithmetic.  False:
// dead (nothing is written).
PISLAM_HD bool chi2_at(const float (&T)[12], const Cam &C, const Obs &o, float *chi2_out) {
  if (!o.live) return false;
  const float x = ((T[0] * o.X + T[1] * o.Y) + T[2] * o.Z) + T[9];
  const float y = ((T[3] * o.X + T[4] * o.Y) + T[5] * o.Z) + T[10];
  const float z = ((T[6] * o.X + T[7] * o.Y) + T[8] * o.Z) + T[11];
  if (!(z >= pq::Z_MIN)) return false;
  const float iz = fdiv(1.0f, z);
  const float px = x * iz, py = y * iz;
  const float pu = C.fx * px + C.cx, pv = C.fy * py + C.cy;
  const float eu = o.u - pu, ev = o.v - pv;
  const float chi2 = (eu * eu + ev * ev) * o.w;
  if (!finite_f(chi2)) return false;
  *chi2_out = chi2;
  return true;
}

// What one observation adds to a hypothesis's score; *inl = it is an inlier.
PISLAM_HD uint32_t score(const float (&T)[12], const Cam &C, const Obs &o, bool *inl) {
  float c = 0.0f;
  const bool in = chi2_at(T, C, o, &c) && c < TH;
  *inl = in;
  return in ? (uint32_t)floorf((TH - c) * 256.0f) : 0u;
}

PISLAM_HD float dot3(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PISLAM_HD void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

PISLAM_HD void bearing(const Cam &C, float u, float v, float (&y)[3]) {
  const float xn = (u - C.cx) * C.ifx, yn = (v - C.cy) * C.ify;
  const float r = fdiv(1.0f, fsqrt((xn * xn + yn * yn) + 1.0f));
  y[0] = xn * r, y[1] = yn * r, y[2] = r;
}

// One real root of r^3 + b r^2 + c r + d.
PISLAM_HD float cubic_root(float b, float c, float d) {
  const float bb = b * b, c3 = 3.0f * c;
  float r;
  if (bb >= c3) {                                            // two stationary points
    const float v = fsqrt(bb - c3);
    const float t1 = fdiv(-b - v, 3.0f);
    const float k1 = ((t1 + b) * t1 + c) * t1 + d;
    if (k1 > 0.0f) {
      r = t1 - fsqrt(fdiv(-k1, 3.0f * t1 + b));
    } else {
      const float t2 = fdiv(-b + v, 3.0f);
      const float k2 = ((t2 + b) * t2 + c) * t2 + d;
      r = t2 + fsqrt(fdiv(-k2, 3.0f * t2 + b));
    }
  } else {
    r = fdiv(-b, 3.0f);
    if (fabsf((3.0f * r + 2.0f * b) * r + c) < 1e-4f) r = r + 1.0f;
  }
  for (int i = 0; i < NEWTON; i++) {
    const float f = ((r + b) * r + c) * r + d;
    const float fp = (3.0f * r + 2.0f * b) * r + c;
    if (fp != 0.0f) r = r - fdiv(f, fp);
  }
  return r;
}

// The unit eigenvector (a1, a2, 1) * rn of the symmetric A for its eigenvalue e.
PISLAM_HD void eigenvector(float e, float A00, float A01, float A02, float A11, float A12, float x01, float prec0, float prec1,
                           float (&v)[3]) {
  const float tmp = fdiv(1.0f, ((e * (A00 + A11) - A00 * A11) - e * e) + x01);
  const float a1 = -((e * A02 + prec0) * tmp), a2 = -((e * A12 + prec1) * tmp);
  const float rn = fdiv(1.0f, fsqrt((a1 * a1 + a2 * a2) + 1.0f));
  v[0] = a1 * rn, v[1] = a2 * rn, v[2] = rn;
}

struct Solver {
  Cam C;
  Obs o4;
  float y1[3], y2[3], y3[3], x1[3];
  float a12, a13, a23, b12, b13, b23;
  float Xi[9];
  float best;                                  // the smallest chi2 of draw 3 so far
  bool found;
  float T[12];

  // One solution of the depth quadratic: the depths, their refinement, the pose, its chi2 on draw 3.
  PISLAM_HD void candidate(float w0, float w1, float tau) {
    if (!(tau > 0.0f)) return;
    const float d = fdiv(a23, tau * (b23 + tau) + 1.0f);
    if (!(d > 0.0f)) return;
    float l2 = fsqrt(d);
    float l3 = tau * l2;
    float l1 = w0 * l2 + w1 * l3;
    if (!(l1 >= 0.0f)) return;
    for (int i = 0; i < REFINE; i++) {
      const float r1 = ((l1 * l1 + l2 * l2) + (b12 * l1) * l2) - a12;
      const float r2 = ((l1 * l1 + l3 * l3) + (b13 * l1) * l3) - a13;
      const float r3 = ((l2 * l2 + l3 * l3) + (b23 * l2) * l3) - a23;
      const float v0 = 2.0f * l1 + b12 * l2, v1 = 2.0f * l2 + b12 * l1;
      const float v3 = 2.0f * l1 + b13 * l3, v5 = 2.0f * l3 + b13 * l1;
      const float v7 = 2.0f * l2 + b23 * l3, v8 = 2.0f * l3 + b23 * l2;
      const float idet = fdiv(1.0f, -((v0 * v5) * v7) - (v1 * v3) * v8);
      const float n1 = ((v1 * v5) * r3 - (v5 * v7) * r1) - (v1 * v8) * r2;
      const float n2 = ((v0 * v8) * r2 - (v3 * v8) * r1) - (v0 * v5) * r3;
      const float n3 = ((v3 * v7) * r1 - (v0 * v7) * r2) - (v1 * v3) * r3;
      l1 = l1 - n1 * idet, l2 = l2 - n2 * idet, l3 = l3 - n3 * idet;
    }
    float ry1[3], e1[3], e2[3], e3[3];
PISLAM_UNROLL
    for (int i = 0; i < 3; i++) {
      ry1[i] = l1 * y1[i];
      e1[i] = ry1[i] - l2 * y2[i];
      e2[i] = ry1[i] - l3 * y3[i];
    }
    cross3(e1, e2, e3);
    float P[12];
    bool fin = true;
PISLAM_UNROLL
    for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
      for (int j = 0; j < 3; j++) P[3 * i + j] = (e1[i] * Xi[j] + e2[i] * Xi[3 + j]) + e3[i] * Xi[6 + j];
      P[9 + i] = ry1[i] - ((P[3 * i] * x1[0] + P[3 * i + 1] * x1[1]) + P[3 * i + 2] * x1[2]);
    }
PISLAM_UNROLL
    for (int i = 0; i < 12; i++) fin = fin && finite_f(P[i]);
    float c = 0.0f;
    if (!fin || !chi2_at(P, C, o4, &c) || !(c < best)) return;
    best = c, found = true;
PISLAM_UNROLL
    for (int i = 0; i < 12; i++) T[i] = P[i];
  }

  // The two solutions for one sign of v.
  PISLAM_HD void branch(float s, float V00, float V10, float V20, float V01, float V11, float V21) {
    const float w2 = fdiv(1.0f, s * V01 - V00);
    const float w0 = (V10 - s * V11) * w2, w1 = (V20 - s * V21) * w2;
    const float qa = fdiv(1.0f, (((a13 - a12) * w1) * w1 - (a12 * b13) * w1) - a12);
    const float qb = (((a13 * b12) * w1 - (a12 * b13) * w0) - ((2.0f * w0) * w1) * (a12 - a13)) * qa;
    const float qc = ((((a13 - a12) * w0) * w0 + (a13 * b12) * w0) + a13) * qa;
    const float disc = qb * qb - 4.0f * qc;
    if (!(disc >= 0.0f)) return;
    const float sq = fsqrt(disc);
    candidate(w0, w1, (-qb + sq) * 0.5f);
    candidate(w0, w1, (-qb - sq) * 0.5f);
  }
};

// The pose of the minimal problem (o1, o2, o3) that fits o4 best; false: the hypothesis is invalid.
PISLAM_HD bool solve(const Cam &C, const Obs &o1, const Obs &o2, const Obs &o3, const Obs &o4, float (&T)[12]) {
  Solver S;
  S.C = C, S.o4 = o4, S.best = __builtin_inff(), S.found = false;
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) S.T[i] = 0.0f;
  bearing(C, o1.u, o1.v, S.y1), bearing(C, o2.u, o2.v, S.y2), bearing(C, o3.u, o3.v, S.y3);
  S.x1[0] = o1.X, S.x1[1] = o1.Y, S.x1[2] = o1.Z;
  const float b12 = -2.0f * dot3(S.y1, S.y2), b13 = -2.0f * dot3(S.y1, S.y3), b23 = -2.0f * dot3(S.y2, S.y3);
  float d12[3], d13[3], d23[3], nx[3];
  d12[0] = o1.X - o2.X, d12[1] = o1.Y - o2.Y, d12[2] = o1.Z - o2.Z;
  d13[0] = o1.X - o3.X, d13[1] = o1.Y - o3.Y, d13[2] = o1.Z - o3.Z;
  d23[0] = o2.X - o3.X, d23[1] = o2.Y - o3.Y, d23[2] = o2.Z - o3.Z;
  const float a12 = dot3(d12, d12), a13 = dot3(d13, d13), a23 = dot3(d23, d23);
  S.a12 = a12, S.a13 = a13, S.a23 = a23, S.b12 = b12, S.b13 = b13, S.b23 = b23;
  const float c12 = -0.5f * b12, c23 = -0.5f * b23, c31 = -0.5f * b13;
  const float s12 = 1.0f - c12 * c12, s23 = 1.0f - c23 * c23, s31 = 1.0f - c31 * c31;
  const float blob = (c12 * c23) * c31 - 1.0f;
  const float p3 = a13 * (a23 * s31 - a13 * s23);
  const float p2 = (((2.0f * blob) * a23) * a13 + (a13 * (2.0f * a12 + a13)) * s23) + (a23 * (a23 - a12)) * s31;
  const float p1 = ((a23 * (a13 - a23)) * s12 - (a12 * a12) * s23) - (2.0f * a12) * (blob * a23 + a13 * s23);
  const float p0 = a12 * (a12 * s23 - a23 * s12);
  if (p3 == 0.0f) return false;
  const float ip = fdiv(1.0f, p3);
  const float g = cubic_root(p2 * ip, p1 * ip, p0 * ip);

  const float A00 = a23 * (1.0f - g), A01 = (a23 * b12) * 0.5f, A02 = ((a23 * b13) * g) * -0.5f;
  const float A11 = (a23 - a12) + a13 * g, A12 = (b23 * (a13 * g - a12)) * 0.5f, A22 = g * (a13 - a23) - a12;
  // the two eigenvalues that are not 0: the roots of e^2 + eb e + ec, the larger magnitude first
  const float x01 = A01 * A01;
  const float eb = (-A00 - A11) - A22;
  const float ec = (((-x01 - A02 * A02) - A12 * A12) + A00 * (A11 + A22)) + A11 * A22;
  float disc = eb * eb - 4.0f * ec;
  if (!(disc > 0.0f)) disc = 0.0f;
  const float sq = fsqrt(disc);
  const float L0 = (eb < 0.0f ? -eb + sq : -eb - sq) * 0.5f;
  const float L1 = fdiv(ec, L0);
  const float prec0 = A01 * A12 - A02 * A11, prec1 = A01 * A02 - A00 * A12;
  float va[3], vb[3];
  eigenvector(L0, A00, A01, A02, A11, A12, x01, prec0, prec1, va);
  eigenvector(L1, A00, A01, A02, A11, A12, x01, prec0, prec1, vb);
  const float q = fdiv(-L1, L0);
  const float v = q > 0.0f ? fsqrt(q) : 0.0f;

  // the inverse of X = [d12, d13, d12 x d13] (columns) by cofactors
  cross3(d12, d13, nx);
  {
    const float m00 = d12[0], m01 = d13[0], m02 = nx[0], m10 = d12[1], m11 = d13[1], m12 = nx[1];
    const float m20 = d12[2], m21 = d13[2], m22 = nx[2];
    const float i00 = m11 * m22 - m12 * m21, i01 = m02 * m21 - m01 * m22, i02 = m01 * m12 - m02 * m11;
    const float i10 = m12 * m20 - m10 * m22, i11 = m00 * m22 - m02 * m20, i12 = m02 * m10 - m00 * m12;
    const float i20 = m10 * m21 - m11 * m20, i21 = m01 * m20 - m00 * m21, i22 = m00 * m11 - m01 * m10;
    const float idet = fdiv(1.0f, (m00 * i00 + m01 * i10) + m02 * i20);
    S.Xi[0] = i00 * idet, S.Xi[1] = i01 * idet, S.Xi[2] = i02 * idet;
    S.Xi[3] = i10 * idet, S.Xi[4] = i11 * idet, S.Xi[5] = i12 * idet;
    S.Xi[6] = i20 * idet, S.Xi[7] = i21 * idet, S.Xi[8] = i22 * idet;
  }
  S.branch(v, va[0], va[1], va[2], vb[0], vb[1], vb[2]);
  S.branch(-v, va[0], va[1], va[2], vb[0], vb[1], vb[2]);
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) T[i] = S.T[i];
  return S.found;
}

// Hypothesis k of frame b: its pose; false when invalid.  fetch(i) is observation i of the frame.
template <class FETCH>
PISLAM_HD bool hypothesis(const Cam &C, const FETCH &fetch, uint32_t n, uint32_t seed, uint32_t b, uint32_t k, float (&T)[12]) {
  uint32_t draw[SAMPLE];
  pgm::sample<SAMPLE>(seed, b, k, n, draw);
  return solve(C, fetch(draw[0]), fetch(draw[1]), fetch(draw[2]), fetch(draw[3]), T);
}

// One frame as the call reads it.
struct Frame {
  const float *cam, *xw;                       // [5], [n][3]
  const int32_t *obs;                          // [n][3]
  const uint8_t *level;                        // [n] or null
  const float *inv_sigma2;                     // [nlevels] or null with level == null
  int nlevels;
  uint32_t n;                                  // already psm::clamp_count(count, stride)
  uint32_t b;                                  // the frame's index in the batch: the sampler hashes it
};

// The frame as the RANSAC skeleton sees it (pislam_ransac_math.h).
struct Problem {
  static constexpr int WORDS = 12;
  using Item = Obs;
  Frame F;
  Cam C;
  uint32_t seed, n;
  bool cam_ok, have;
  PISLAM_HD Problem(const Frame &F_, uint32_t seed_) : F(F_), seed(seed_), n(F_.n) {
    float cam[5];
PISLAM_UNROLL
    for (int i = 0; i < 5; i++) cam[i] = F.cam[i];
    cam_ok = pnm::cam_ok(cam), C = make_cam(cam);
    have = cam_ok && n >= (uint32_t)SAMPLE;
  }
  PISLAM_HD Obs item(uint32_t i) const {
    return obs(F.xw + 3 * (size_t)i, F.obs + 3 * (size_t)i, F.level ? F.level + i : nullptr, F.inv_sigma2, F.nlevels);
  }
  PISLAM_HD bool hypothesis(uint32_t k, float (&T)[12]) const {
    const Problem &P = *this;
    return pnm::hypothesis(C, [&P](uint32_t i) { return P.item(i); }, n, seed, F.b, k, T);
  }
  PISLAM_HD uint32_t score(const float (&T)[12], const Obs &o, bool *inl) const { return pnm::score(T, C, o, inl); }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one frame (the probe; never the library's hot path) ---------------

struct Result {
  int32_t best;
  uint32_t score, ninliers, status;
  float pose[12];
};

inline void host_frame(const Frame &F, int hypotheses, uint32_t seed, int min_inliers, Result *R, uint8_t *inlier) {
  const Problem P(F, seed);
  float T[12] = {0};
  const prk::Outcome O = prk::host_ransac(P, hypotheses, T, inlier);
  R->best = O.best, R->score = O.score, R->ninliers = O.ninliers, R->status = prk::status(O, P.cam_ok, min_inliers);
  for (int i = 0; i < 12; i++) R->pose[i] = O.best < 0 ? 0.0f : T[i];
}
#endif

}  // namespace pnm
