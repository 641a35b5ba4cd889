// Host check of the two-view call's host half (pislam_amd/csrc/pislam_geom_host.h: pgh::two_view_denormalise), on the
// CPU only.  Random models and statistics: the result is checked against plain 3 x 3 matrix products written out here
// (T2' * M * T1 and inverse(T2) * M * T1 with the inverse written out as a matrix), and every refused argument.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I pislam_amd/csrc tools/probes/two_view_host_check.cpp -o tools/probes/_bin/two_view_host_check && tools/probes/_bin/two_view_host_check
#include <math.h>
#include <stdio.h>
#include <random>
#include <vector>
#include "pislam_geom_host.h"

static void mul(const double *a, const double *b, double *c) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

int main() {
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> val(-2.0, 2.0);
  int bad = 0;
  for (int it = 0; it < 20000; it++) {
    // heap copies of exactly the sizes the function may touch: a read or write past them is an ASan report
    std::vector<float> m(9);
    std::vector<int64_t> st(8);
    std::vector<double> out(9);
    for (auto &v : m) v = (float)val(rng);
    m[8] = 1.0f;
    const int64_t n = 1 + (int64_t)(rng() % 16384);
    st[0] = n;
    for (int i = 0; i < 2; i++) {
      st[1 + 3 * i] = (int64_t)(rng() % (1ull << 35)) - (1ll << 34);
      st[2 + 3 * i] = (int64_t)(rng() % (1ull << 35)) - (1ll << 34);
      st[3 + 3 * i] = 1 + (int64_t)(rng() % (it % 7 == 0 ? 4ull : 1ull << 50));
    }
    st[7] = 0;
    const int model = it & 1;
    if (!pgh::two_view_denormalise(model, m.data(), st.data(), out.data())) return printf("refused case %d\n", it), 1;
    double T[2][9], M[9], R[9], W[9];
    for (int i = 0; i < 2; i++) {
      const double k = 2.0 * (double)n * (double)n / (double)st[3 + 3 * i], s = 256.0 * (double)n * k;
      const double t[9] = {s, 0, -(double)st[1 + 3 * i] * k, 0, s, -(double)st[2 + 3 * i] * k, 0, 0, 1};
      for (int j = 0; j < 9; j++) T[i][j] = t[j];
    }
    for (int j = 0; j < 9; j++) M[j] = (double)m[j];
    mul(M, T[0], R);                                        // M * T1
    // the left factor written out as a matrix; the tolerance is relative to the magnitude of the terms of each sum
    const double s2 = T[1][0], tx = T[1][2], ty = T[1][5];
    const double T2t[9] = {s2, 0, 0, 0, s2, 0, tx, ty, 1};
    const double T2i[9] = {1 / s2, 0, -tx / s2, 0, 1 / s2, -ty / s2, 0, 0, 1};
    const double *L = model == 0 ? T2t : T2i;
    mul(L, R, W);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double mag = fabs(L[3 * i] * R[j]) + fabs(L[3 * i + 1] * R[3 + j]) + fabs(L[3 * i + 2] * R[6 + j]);
        bad += !(fabs(W[3 * i + j] - out[3 * i + j]) <= 1e-14 * mag);
      }
  }
  float m[9] = {0};
  int64_t st[8] = {5, 0, 0, 10, 0, 0, 10, 0};
  double out[9];
  bad += !pgh::two_view_denormalise(0, m, st, out);
  bad += pgh::two_view_denormalise(2, m, st, out) || pgh::two_view_denormalise(-1, m, st, out);
  bad += pgh::two_view_denormalise(0, nullptr, st, out) || pgh::two_view_denormalise(0, m, nullptr, out) ||
         pgh::two_view_denormalise(0, m, st, nullptr);
  for (int i : {0, 3, 6}) {
    int64_t s2[8];
    for (int j = 0; j < 8; j++) s2[j] = st[j];
    s2[i] = 0;
    bad += pgh::two_view_denormalise(1, m, s2, out);
    s2[i] = -3;
    bad += pgh::two_view_denormalise(1, m, s2, out);
  }
  printf("two_view_host_check: %d mismatches\n", bad);
  return bad != 0;
}
