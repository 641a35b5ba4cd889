// pislam_geom_math.h — the arithmetic of pislam_two_view_ransac_batch (include/pislam_hip.h: that comment is the
// contract), stated ONCE for the device kernel (pislam_geom_kernels.h) and for a plain C++ compiler (tools/probes/
// ransac_host_check.cpp): a pair's normalisation, the counter-based sampler, the 8 x 9 system and its elimination, the
// two chi-square forms in binary32, the integer score, the pair as the RANSAC skeleton sees it (pislam_ransac_math.h,
// which holds the best-of rule and the serial form of the steps), and, for the host only, the whole call for one pair
// run serially.  Every operation is written out one rounding at a time; build with -ffp-contract=off.
#pragma once
#include <stdlib.h>
#include "pislam_ransac_math.h"

namespace pgm {

constexpr int MAX_HYP = prk::MAX_HYP;
constexpr int MAX_STRIDE = 16384;
constexpr float PIVOT_MIN = 0x1p-20f;
constexpr float TH_SCORE = 5.991f;
constexpr float TH_FUND = 3.841f, TH_HOMOG = 5.991f;         // chi-square, 1 and 2 degrees of freedom
constexpr int sample_size(int model) { return model == 0 ? 8 : 4; }

PISLAM_HD float sigma_px(int32_t sigma_q8) { return (float)sigma_q8 / 256.0f; }   // exact: below 2^13 over a power of two

PISLAM_HD constexpr uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
PISLAM_HD constexpr uint32_t hash(uint32_t seed, uint32_t b, uint32_t k, uint32_t j) {
  uint32_t h = mix32(seed + 0x9e3779b9u * b);
  h = mix32(h ^ (0x85ebca6bu * (k + 1u)));
  return mix32(h ^ (0xc2b2ae35u * (j + 1u)));
}

// A match as the call reads it: the Q8 coordinates in both images, clamped.
struct Match {
  int32_t x1, y1, x2, y2;
};
PISLAM_HD Match match(int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
  return Match{psm::clamp_q8(x1), psm::clamp_q8(y1), psm::clamp_q8(x2), psm::clamp_q8(y2)};
}

// One pair's normalisation: integer centre, one scale per image.
struct Norm {
  long long sx1, sy1, sx2, sy2;
  int32_t n;
  float k1, k2;
};
// What a point adds to its image's D.
PISLAM_HD long long spread(int32_t n, int32_t x, int32_t y, long long sx, long long sy) {
  return llabs((long long)n * x - sx) + llabs((long long)n * y - sy);
}
PISLAM_HD float scale(int32_t n, long long D) { return (float)(2 * n * n) / (float)D; }   // n <= 16384: 2 n n <= 2^29
// The chi-square weight of the image with the scale k: 1 / (256 n k sigma)^2.
PISLAM_HD float weight(int32_t n, float k, float sigma) {
  const float t = ((256.0f * (float)n) * k) * sigma;
  return 1.0f / (t * t);
}

struct Point {
  float x1, y1, x2, y2;
};
PISLAM_HD Point point(const Norm &N, const Match &m) {
  Point P;
  P.x1 = (float)((long long)N.n * m.x1 - N.sx1) * N.k1;
  P.y1 = (float)((long long)N.n * m.y1 - N.sy1) * N.k1;
  P.x2 = (float)((long long)N.n * m.x2 - N.sx2) * N.k2;
  P.y2 = (float)((long long)N.n * m.y2 - N.sy2) * N.k2;
  return P;
}

// The m distinct indices of hypothesis k in draw order; `sorted` is the ascending copy that later draws step over.
template <int M>
PISLAM_HD void sample(uint32_t seed, uint32_t b, uint32_t k, uint32_t n, uint32_t (&draw)[M]) {
  uint32_t sorted[M];
PISLAM_UNROLL
  for (int j = 0; j < M; j++) {
    uint32_t r = (uint32_t)(((uint64_t)hash(seed, b, k, (uint32_t)j) * (n - (uint32_t)j)) >> 32);
PISLAM_UNROLL
    for (int t = 0; t < j; t++) r += r >= sorted[t] ? 1u : 0u;
    draw[j] = r;
    uint32_t v = r;
PISLAM_UNROLL
    for (int t = 0; t < j; t++) {
      const uint32_t lo = sorted[t] < v ? sorted[t] : v, hi = sorted[t] < v ? v : sorted[t];
      sorted[t] = lo, v = hi;
    }
    sorted[j] = v;
  }
}

// Gaussian elimination with partial pivoting on [A | b] (8 x 9), back substitution into x.  False: a pivot below
// PIVOT_MIN (or a NaN) or a solution that is not finite.  Static indices only.
PISLAM_HD bool solve(float (&A)[8][9], float (&x)[8]) {
  bool ok = true;
PISLAM_UNROLL
  for (int c = 0; c < 8; c++) {
PISLAM_UNROLL
    for (int r = c + 1; r < 8; r++) {
      const bool s = fabsf(A[r][c]) > fabsf(A[c][c]);        // strict: row c ends as the first row of largest magnitude
PISLAM_UNROLL
      for (int j = c; j < 9; j++) {
        const float t = A[c][j], u = A[r][j];
        A[c][j] = s ? u : t;
        A[r][j] = s ? t : u;
      }
    }
    ok = ok && fabsf(A[c][c]) >= PIVOT_MIN;                  // false for a NaN
    const float inv = 1.0f / A[c][c];
PISLAM_UNROLL
    for (int r = c + 1; r < 8; r++) {
      const float f = A[r][c] * inv;
PISLAM_UNROLL
      for (int j = c + 1; j < 9; j++) A[r][j] = A[r][j] - f * A[c][j];
    }
  }
PISLAM_UNROLL
  for (int r = 7; r >= 0; r--) {
    float s = A[r][8];
PISLAM_UNROLL
    for (int j = r + 1; j < 8; j++) s = s - A[r][j] * x[j];
    x[r] = s / A[r][r];
    ok = ok && psm::finite_f(x[r]);
  }
  return ok;
}

// Hypothesis k of pair b: its 8 unknowns; false when invalid.  fetch(i) is match i of the pair.
template <int MODEL, class FETCH>
PISLAM_HD bool hypothesis(const Norm &N, const FETCH &fetch, uint32_t seed, uint32_t b, uint32_t k, float (&x)[8]) {
  constexpr int M = sample_size(MODEL);
  uint32_t draw[M];
  sample<M>(seed, b, k, (uint32_t)N.n, draw);
  float A[8][9];
PISLAM_UNROLL
  for (int j = 0; j < M; j++) {
    const Point P = point(N, fetch(draw[j]));
    if (MODEL == 0) {
      A[j][0] = P.x2 * P.x1, A[j][1] = P.x2 * P.y1, A[j][2] = P.x2;
      A[j][3] = P.y2 * P.x1, A[j][4] = P.y2 * P.y1, A[j][5] = P.y2;
      A[j][6] = P.x1, A[j][7] = P.y1, A[j][8] = -1.0f;
    } else {
      float *u = A[2 * j], *v = A[2 * j + 1];
      u[0] = P.x1, u[1] = P.y1, u[2] = 1.0f, u[3] = 0.0f, u[4] = 0.0f, u[5] = 0.0f;
      u[6] = -(P.x2 * P.x1), u[7] = -(P.x2 * P.y1), u[8] = P.x2;
      v[0] = 0.0f, v[1] = 0.0f, v[2] = 0.0f, v[3] = P.x1, v[4] = P.y1, v[5] = 1.0f;
      v[6] = -(P.y2 * P.x1), v[7] = -(P.y2 * P.y1), v[8] = P.y2;
    }
  }
  return solve(A, x);
}

// chi2 of the distance of (xb, yb) to the line m * (xa, ya, 1).
PISLAM_HD float line_chi(const float (&m)[9], float xa, float ya, float xb, float yb, float w) {
  const float a = (m[0] * xa + m[1] * ya) + m[2];
  const float b = (m[3] * xa + m[4] * ya) + m[5];
  const float c = (m[6] * xa + m[7] * ya) + m[8];
  const float num = (a * xb + b * yb) + c;
  return ((num * num) / (a * a + b * b)) * w;
}
// chi2 of the distance of (xb, yb) to the image of (xa, ya) under m.
PISLAM_HD float transfer_chi(const float (&m)[9], float xa, float ya, float xb, float yb, float w) {
  const float inv = 1.0f / ((m[6] * xa + m[7] * ya) + m[8]);
  const float u = ((m[0] * xa + m[1] * ya) + m[2]) * inv;
  const float v = ((m[3] * xa + m[4] * ya) + m[5]) * inv;
  const float du = xb - u, dv = yb - v;
  return (du * du + dv * dv) * w;
}

// A model ready for scoring: f (last entry 1) and its second matrix: the transpose of F, the adjugate of H.
template <int MODEL>
struct Model {
  float f[9], g[9];
  PISLAM_HD explicit Model(const float *x) {
PISLAM_UNROLL
    for (int i = 0; i < 8; i++) f[i] = x[i];
    f[8] = 1.0f;
    if (MODEL == 0) {
PISLAM_UNROLL
      for (int i = 0; i < 9; i++) g[i] = f[3 * (i % 3) + i / 3];
    } else {
      g[0] = f[4] * f[8] - f[5] * f[7], g[1] = f[2] * f[7] - f[1] * f[8], g[2] = f[1] * f[5] - f[2] * f[4];
      g[3] = f[5] * f[6] - f[3] * f[8], g[4] = f[0] * f[8] - f[2] * f[6], g[5] = f[2] * f[3] - f[0] * f[5];
      g[6] = f[3] * f[7] - f[4] * f[6], g[7] = f[1] * f[6] - f[0] * f[7], g[8] = f[0] * f[4] - f[1] * f[3];
    }
  }
};

// One match under one model: what it adds to the score; *inl = both directions pass.
template <int MODEL>
PISLAM_HD uint32_t score(const Model<MODEL> &m, const Point &P, float w1, float w2, bool *inl) {
  constexpr float th = MODEL == 0 ? TH_FUND : TH_HOMOG;
  float ca, cb;
  if (MODEL == 0) {
    ca = line_chi(m.f, P.x1, P.y1, P.x2, P.y2, w2);
    cb = line_chi(m.g, P.x2, P.y2, P.x1, P.y1, w1);
  } else {
    ca = transfer_chi(m.f, P.x1, P.y1, P.x2, P.y2, w2);
    cb = transfer_chi(m.g, P.x2, P.y2, P.x1, P.y1, w1);
  }
  const bool oka = ca < th, okb = cb < th;                   // false for a NaN
  uint32_t s = 0;
  if (oka) s += (uint32_t)floorf((TH_SCORE - ca) * 256.0f);
  if (okb) s += (uint32_t)floorf((TH_SCORE - cb) * 256.0f);
  *inl = oka && okb;
  return s;
}

// One pair as the call reads it.
struct PairIn {
  const int32_t *p1, *p2;                      // [n][2]
  uint32_t n;                                  // already psm::clamp_count(count, stride)
  uint32_t b;                                  // the pair's index in the batch: the sampler hashes it
};
PISLAM_HD Match match_at(const PairIn &I, uint32_t i) {
  return match(I.p1[2 * (size_t)i], I.p1[2 * (size_t)i + 1], I.p2[2 * (size_t)i], I.p2[2 * (size_t)i + 1]);
}

// The pair as the RANSAC skeleton sees it (pislam_ransac_math.h), from its integer sums: N with n and the four
// coordinate sums, D1 and D2 the two spreads.
template <int MODEL>
struct Problem {
  static constexpr int WORDS = 8;
  using Item = Point;
  PairIn I;
  Norm N;
  float w1, w2;
  uint32_t seed, n;
  bool have;
  PISLAM_HD Problem(const PairIn &I_, const Norm &N_, long long D1, long long D2, float sigma, uint32_t seed_)
      : I(I_), N(N_), w1(0.0f), w2(0.0f), seed(seed_), n(I_.n) {
    have = n >= (uint32_t)sample_size(MODEL) && D1 != 0 && D2 != 0;
    if (have) {
      N.k1 = scale(N.n, D1), N.k2 = scale(N.n, D2);
      w1 = weight(N.n, N.k1, sigma), w2 = weight(N.n, N.k2, sigma);
    }
  }
  PISLAM_HD Point item(uint32_t i) const { return point(N, match_at(I, i)); }
  PISLAM_HD bool hypothesis(uint32_t k, float (&x)[8]) const {
    const PairIn &J = I;
    return pgm::hypothesis<MODEL>(N, [&J](uint32_t i) { return match_at(J, i); }, seed, I.b, k, x);
  }
  PISLAM_HD uint32_t score(const float (&x)[8], const Point &P, bool *inl) const {
    return pgm::score<MODEL>(Model<MODEL>(x), P, w1, w2, inl);
  }
};
PISLAM_HD void stats_row(const Norm &N, long long D1, long long D2, long long *st) {
  st[0] = N.n, st[1] = N.sx1, st[2] = N.sy1, st[3] = D1, st[4] = N.sx2, st[5] = N.sy2, st[6] = D2, st[7] = 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one pair (the probe; never the library's hot path) ----------------

struct PairOut {
  int32_t best;
  uint32_t score, ninliers;
  float model_n[9];
  long long stats[8];
};

template <int MODEL>
inline void host_pair(const PairIn &I, int hypotheses, uint32_t seed, int32_t sigma_q8, PairOut *O, uint8_t *inlier) {
  Norm N{};
  N.n = (int32_t)I.n;
  for (uint32_t i = 0; i < I.n; i++) {
    const Match m = match_at(I, i);
    N.sx1 += m.x1, N.sy1 += m.y1, N.sx2 += m.x2, N.sy2 += m.y2;
  }
  long long D1 = 0, D2 = 0;
  for (uint32_t i = 0; i < I.n; i++) {
    const Match m = match_at(I, i);
    D1 += spread(N.n, m.x1, m.y1, N.sx1, N.sy1), D2 += spread(N.n, m.x2, m.y2, N.sx2, N.sy2);
  }
  stats_row(N, D1, D2, O->stats);
  float x[8] = {0};
  const Problem<MODEL> P(I, N, D1, D2, sigma_px(sigma_q8), seed);
  const prk::Outcome R = prk::host_ransac(P, hypotheses, x, inlier);
  O->best = R.best, O->score = R.score, O->ninliers = R.ninliers;
  for (int i = 0; i < 9; i++) O->model_n[i] = R.best < 0 ? 0.0f : i < 8 ? x[i] : 1.0f;
}
#endif

}  // namespace pgm
