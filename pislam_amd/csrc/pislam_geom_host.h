// pislam_geom_host.h — the host half of the two-view call (pislam_two_view_denormalise; include/pislam_hip.h).  Host
// only, no HIP: a plain C++ translation unit can include it (a sanitizer build of a small driver, for instance).
#pragma once

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

}  // namespace pgh
