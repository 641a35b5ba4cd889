// pislam_geom_host.h — the host half of the two-view calls (pislam_two_view_denormalise, pislam_two_view_decompose;
// include/pislam_hip.h).  Host only, no HIP: a plain C++ translation unit can include it (a sanitizer build of a small
// driver, for instance).
#pragma once

#include <math.h>
#include <stdint.h>

namespace pgh {

// out = T2' * Fn * T1 (model 0) or inverse(T2) * Hn * T1 (model 1) in double, T = [s 0 -Sx k; 0 s -Sy k; 0 0 1] with
// k = 2 n n / D and s = 256 n k.  False for a bad argument.
inline bool two_view_denormalise(int model, const float *model_n, const int64_t *st, double out[9]) {
  if ((model != 0 && model != 1) || !model_n || !st || !out) return false;
  const int64_t n = st[0];
  if (n < 1 || st[3] < 1 || st[6] < 1) return false;
  double s[2], tx[2], ty[2];
  for (int i = 0; i < 2; i++) {
    const double k = 2.0 * (double)n * (double)n / (double)st[3 + 3 * i];
    s[i] = 256.0 * (double)n * k, tx[i] = -(double)st[1 + 3 * i] * k, ty[i] = -(double)st[2 + 3 * i] * k;
  }
  double m[9], r[9];
  for (int i = 0; i < 9; i++) m[i] = (double)model_n[i];
  // r = M * T1: the columns of M scaled, the last column picks up the translation
  for (int i = 0; i < 3; i++) {
    r[3 * i + 0] = m[3 * i + 0] * s[0];
    r[3 * i + 1] = m[3 * i + 1] * s[0];
    r[3 * i + 2] = m[3 * i + 0] * tx[0] + m[3 * i + 1] * ty[0] + m[3 * i + 2];
  }
  if (model == 0) {
    // T2' * r: rows 0 and 1 scaled, row 2 = tx * row 0 + ty * row 1 + row 2
    for (int j = 0; j < 3; j++) {
      out[0 + j] = s[1] * r[0 + j];
      out[3 + j] = s[1] * r[3 + j];
      out[6 + j] = tx[1] * r[0 + j] + ty[1] * r[3 + j] + r[6 + j];
    }
  } else {
    // inverse(T2) = [1/s 0 -tx/s; 0 1/s -ty/s; 0 0 1]
    for (int j = 0; j < 3; j++) {
      out[0 + j] = (r[0 + j] - tx[1] * r[6 + j]) / s[1];
      out[3 + j] = (r[3 + j] - ty[1] * r[6 + j]) / s[1];
      out[6 + j] = r[6 + j];
    }
  }
  return true;
}

// ---- pislam_two_view_decompose ---------------------------------------------------------------------------------------

// A = U diag(d) V' for a 3 x 3 matrix (row-major), d0 >= d1 >= d2 >= 0, U and V orthogonal: one-sided Jacobi (Hestenes)
// on the columns of W = A V, a fixed number of sweeps at most.  The column of U that belongs to the smallest singular
// value is the cross product of the other two (with the sign of W's column), so a singular A has an orthogonal U too.
inline void svd3(const double *A, double *U, double *d, double *V) {
  double W[9], Vt[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; i++) W[i] = A[i];
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++) {
      for (int q = p + 1; q < 3; q++) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < 3; i++)
          alpha += W[3 * i + p] * W[3 * i + p], beta += W[3 * i + q] * W[3 * i + q], gamma += W[3 * i + p] * W[3 * i + q];
        if (gamma == 0.0 || fabs(gamma) <= 1e-16 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; i++) {
          const double wp = W[3 * i + p], wq = W[3 * i + q], vp = Vt[3 * i + p], vq = Vt[3 * i + q];
          W[3 * i + p] = c * wp - s * wq, W[3 * i + q] = s * wp + c * wq;
          Vt[3 * i + p] = c * vp - s * vq, Vt[3 * i + q] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double nrm[3];
  int o[3] = {0, 1, 2};
  for (int j = 0; j < 3; j++) nrm[j] = sqrt(W[j] * W[j] + W[3 + j] * W[3 + j] + W[6 + j] * W[6 + j]);
  for (int a = 0; a < 2; a++)
    for (int b = 0; b < 2 - a; b++)
      if (nrm[o[b]] < nrm[o[b + 1]]) {
        const int t = o[b];
        o[b] = o[b + 1], o[b + 1] = t;
      }
  for (int j = 0; j < 3; j++) {
    d[j] = nrm[o[j]];
    for (int i = 0; i < 3; i++) V[3 * i + j] = Vt[3 * i + o[j]];
  }
  // U: the two large columns normalised (the second made orthogonal to the first once more), the third their cross product
  double u0[3], u1[3], u2[3];
  for (int i = 0; i < 3; i++) u0[i] = d[0] > 0 ? W[3 * i + o[0]] / d[0] : (i == 0), u1[i] = W[3 * i + o[1]];
  const double dot = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
  for (int i = 0; i < 3; i++) u1[i] -= dot * u0[i];
  double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  if (!(n1 > 1e-300)) {                        // rank below 2: any unit vector orthogonal to u0
    const int k = fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2]) ? 0 : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
    double e[3] = {0, 0, 0};
    e[k] = 1.0;
    for (int i = 0; i < 3; i++) u1[i] = e[i] - u0[k] * u0[i];
    n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
  }
  for (int i = 0; i < 3; i++) u1[i] /= n1;
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  const double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  const double sgn = u2[0] * W[o[2]] + u2[1] * W[3 + o[2]] + u2[2] * W[6 + o[2]] < 0 ? -1.0 : 1.0;
  for (int i = 0; i < 3; i++) U[3 * i] = u0[i], U[3 * i + 1] = u1[i], U[3 * i + 2] = sgn * u2[i] / n2;
}

inline void mul3(const double *A, const double *B, double *C) {       // C = A B
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
inline void mul3t(const double *A, const double *B, double *C) {      // C = A B'
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
inline double det3(const double *A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// One candidate, checked in double and stored as floats.  False: R is not a rotation to 1e-12, or t has no direction.
inline bool store_motion(const double *R, const double *t, float *out) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double g = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0);
      if (!(fabs(g) <= 1e-12)) return false;
    }
  if (!(fabs(det3(R) - 1.0) <= 1e-12)) return false;
  const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  if (!(n > 0.0) || !(n < HUGE_VAL)) return false;
  for (int i = 0; i < 9; i++) out[i] = (float)R[i];
  for (int i = 0; i < 3; i++) out[9 + i] = (float)(t[i] / n);
  return true;
}

// The candidate motions of a pixel matrix (include/pislam_hip.h).  False for a bad argument; *ncand = 0 for a
// degenerate decomposition.
inline bool two_view_decompose(int model, const double *m, const double *cam, float *cand, int *ncand) {
  if ((model != 0 && model != 1) || !m || !cam || !cand || !ncand) return false;
  for (int i = 0; i < 9; i++)
    if (!(fabs(m[i]) < HUGE_VAL)) return false;
  for (int i = 0; i < 4; i++)
    if (!(fabs(cam[i]) < HUGE_VAL)) return false;
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  if (fx == 0.0 || fy == 0.0) return false;
  const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
  const double Ki[9] = {1.0 / fx, 0, -cx / fx, 0, 1.0 / fy, -cy / fy, 0, 0, 1};
  for (int i = 0; i < 8 * 12; i++) cand[i] = 0.0f;
  *ncand = 0;
  double A[9], T[9], U[9], V[9], d[3], R[9], t[3];
  if (model == 0) {
    const double Kt[9] = {fx, 0, 0, 0, fy, 0, cx, cy, 1};
    mul3(Kt, m, T), mul3(T, K, A);
  } else {
    mul3(Ki, m, T), mul3(T, K, A);
  }
  for (int i = 0; i < 9; i++)
    if (!(fabs(A[i]) < HUGE_VAL)) return false;
  svd3(A, U, d, V);
  int k = 0;
  bool ok = true;
  if (model == 0) {
    if (!(d[1] > 0.0)) return true;            // rank below 2: no essential matrix
    const double Wm[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    double R1[9], R2[9];
    mul3(U, Wm, T), mul3t(T, V, R1);
    mul3(U, Wt, T), mul3t(T, V, R2);
    if (det3(R1) < 0)
      for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    if (det3(R2) < 0)
      for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    for (int sgn = 0; sgn < 2; sgn++) {
      for (int i = 0; i < 3; i++) t[i] = sgn ? -U[3 * i + 2] : U[3 * i + 2];
      ok = ok && store_motion(R1, t, cand + 12 * k++);
      ok = ok && store_motion(R2, t, cand + 12 * k++);
    }
  } else {
    const double d1 = d[0], d2 = d[1], d3 = d[2];
    if (!(d3 > 0.0) || d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return true;
    const double s = det3(U) * det3(V);
    const double a1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), a3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const double root = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
    const double e1[4] = {1, 1, -1, -1}, e3[4] = {1, -1, 1, -1};
    for (int neg = 0; neg < 2; neg++) {
      const double den = ((neg ? d1 - d3 : d1 + d3) * d2);
      const double sn = root / den, cs = (neg ? d1 * d3 - d2 * d2 : d2 * d2 + d1 * d3) / den;
      for (int i = 0; i < 4; i++) {
        const double x1 = e1[i] * a1, x3 = e3[i] * a3, si = e1[i] * e3[i] * sn;
        double Rp[9] = {cs, 0, -si, 0, 1, 0, si, 0, cs};
        if (neg) Rp[2] = si, Rp[4] = -1.0, Rp[8] = -cs;
        mul3(U, Rp, T), mul3t(T, V, R);
        for (int j = 0; j < 9; j++) R[j] *= s;
        const double tp[3] = {x1, 0.0, neg ? x3 : -x3};
        for (int j = 0; j < 3; j++) t[j] = U[3 * j] * tp[0] + U[3 * j + 2] * tp[2];
        ok = ok && store_motion(R, t, cand + 12 * k++);
      }
    }
  }
  if (!ok) {
    for (int i = 0; i < 8 * 12; i++) cand[i] = 0.0f;
    return true;
  }
  *ncand = k;
  return true;
}

}  // namespace pgh
