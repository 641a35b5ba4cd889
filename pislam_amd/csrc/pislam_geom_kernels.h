// pislam_geom_kernels.h — batched two-view RANSAC on the device (pislam_two_view_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a fundamental matrix or a homography per pair of matched point lists, scored the way
// ORB-SLAM's Initializer scores them.  The header comment is the contract; every binary32 operation below is written
// out one rounding at a time and the library is built with -ffp-contract=off, so a restatement in plain float32
// scalars reproduces every output word.
//
// One workgroup of TV_THREADS works on a pair, then on the pair TV_GRID_CAP further on, and so on; one launch per call,
// no workspace.  Per pair:
//   1. integer sums: Sx, Sy of both images, then D of both images (64-bit LDS atomics: any order gives the same sum);
//   2. one LANE per hypothesis: counter-based sampling, the 8 x 9 system in registers, Gaussian elimination with
//      partial pivoting.  Every index into the system is a compile-time constant (the loops are unrolled and a row
//      swap is a chain of selects), so it never leaves the VGPRs: no scratch.  The 8 unknowns go to LDS;
//   3. scoring with one MATCH per lane: a wave holds 64 matches' normalised coordinates in registers and walks over
//      all hypotheses (the model is an LDS broadcast read), integer wave sum, one LDS atomic add per wave and
//      hypothesis;
//   4. the best score (64-bit LDS atomic max over score << 10 | 1023 - k: the smallest k wins a tie);
//   5. one more pass over the matches with the winning model for the mask, through the SAME scoring routine.
#pragma once

namespace pg {

constexpr int TV_THREADS = 512;                // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs
constexpr int TV_WAVES = TV_THREADS / 64;
constexpr int TV_MAX_HYP = 1024;
constexpr int TV_MAX_STRIDE = 16384;
constexpr int TV_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes
constexpr int32_t TV_COORD_MAX = 1 << 20;
constexpr float TV_PIVOT_MIN = 0x1p-20f;
constexpr float TV_TH_SCORE = 5.991f;
constexpr uint32_t TV_COUNT_INVALID = 0xffffffffu;

// In front of a loop that must stay one copy: unrolled or interleaved copies of the hypothesis loop (the loop vectoriser
// interleaves by two on its own) hold twice the state and spill SGPRs.
#define TV_ROLLED _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")

struct TvArgs {
  const int32_t *p1, *p2;                      // [batch][stride][2]
  const uint32_t *counts;
  size_t stride;
  int batch, hypotheses;
  uint32_t seed;
  float sigma;                                 // float(sigma_q8) / 256.0f, computed on the host (exact)
  int32_t *best;
  uint32_t *score, *ninliers;
  uint8_t *inlier;                             // [batch][stride]
  float *model_n;                              // [batch][9]
  long long *stats;                            // [batch][8]
};

__host__ __device__ constexpr uint32_t tv_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ constexpr uint32_t tv_hash(uint32_t seed, uint32_t b, uint32_t k, uint32_t j) {
  uint32_t h = tv_mix32(seed + 0x9e3779b9u * b);
  h = tv_mix32(h ^ (0x85ebca6bu * (k + 1u)));
  return tv_mix32(h ^ (0xc2b2ae35u * (j + 1u)));
}

__device__ __forceinline__ int32_t tv_clamp(int32_t v) { return min(max(v, -TV_COORD_MAX), TV_COORD_MAX); }

// One pair's normalisation: integer centre, one scale per image.
struct TvNorm {
  long long sx1, sy1, sx2, sy2;
  int32_t n;
  float k1, k2;
};
struct TvPoint {
  float x1, y1, x2, y2;
};
__device__ __forceinline__ TvPoint tv_point(const TvNorm &N, const int32_t *p1, const int32_t *p2, uint32_t i) {
  const int2 a = *(const int2 *)(p1 + 2 * (size_t)i), b = *(const int2 *)(p2 + 2 * (size_t)i);
  TvPoint P;
  P.x1 = (float)((long long)N.n * tv_clamp(a.x) - N.sx1) * N.k1;
  P.y1 = (float)((long long)N.n * tv_clamp(a.y) - N.sy1) * N.k1;
  P.x2 = (float)((long long)N.n * tv_clamp(b.x) - N.sx2) * N.k2;
  P.y2 = (float)((long long)N.n * tv_clamp(b.y) - N.sy2) * N.k2;
  return P;
}

// The m distinct indices of hypothesis k in draw order; `sorted` is the ascending copy that later draws step over.
template <int M>
__device__ __forceinline__ void tv_sample(uint32_t seed, uint32_t b, uint32_t k, uint32_t n, uint32_t (&draw)[M]) {
  uint32_t sorted[M];
#pragma unroll
  for (int j = 0; j < M; j++) {
    uint32_t r = __umulhi(tv_hash(seed, b, k, (uint32_t)j), n - (uint32_t)j);
#pragma unroll
    for (int t = 0; t < j; t++) r += r >= sorted[t] ? 1u : 0u;
    draw[j] = r;
    uint32_t v = r;
#pragma unroll
    for (int t = 0; t < j; t++) {
      const uint32_t lo = min(sorted[t], v), hi = max(sorted[t], v);
      sorted[t] = lo, v = hi;
    }
    sorted[j] = v;
  }
}

// Gaussian elimination with partial pivoting on [A | b] (8 x 9), back substitution into x.  False: a pivot below
// TV_PIVOT_MIN (or a NaN) or a solution that is not finite.  Static indices only.
__device__ __forceinline__ bool tv_solve(float (&A)[8][9], float (&x)[8]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; c++) {
#pragma unroll
    for (int r = c + 1; r < 8; r++) {
      const bool s = fabsf(A[r][c]) > fabsf(A[c][c]);        // strict: row c ends as the first row of largest magnitude
#pragma unroll
      for (int j = c; j < 9; j++) {
        const float t = A[c][j], u = A[r][j];
        A[c][j] = s ? u : t;
        A[r][j] = s ? t : u;
      }
    }
    ok = ok && fabsf(A[c][c]) >= TV_PIVOT_MIN;               // false for a NaN
    const float inv = 1.0f / A[c][c];
#pragma unroll
    for (int r = c + 1; r < 8; r++) {
      const float f = A[r][c] * inv;
#pragma unroll
      for (int j = c + 1; j < 9; j++) A[r][j] = A[r][j] - f * A[c][j];
    }
  }
#pragma unroll
  for (int r = 7; r >= 0; r--) {
    float s = A[r][8];
#pragma unroll
    for (int j = r + 1; j < 8; j++) s = s - A[r][j] * x[j];
    x[r] = s / A[r][r];
    ok = ok && fabsf(x[r]) < __builtin_inff();               // finite: neither infinite nor a NaN
  }
  return ok;
}

// Hypothesis k of pair b: its 8 unknowns; false when invalid.
template <int MODEL>
__device__ __forceinline__ bool tv_hypothesis(const TvNorm &N, const int32_t *p1, const int32_t *p2, uint32_t seed,
                                              uint32_t b, uint32_t k, float (&x)[8]) {
  constexpr int M = MODEL == 0 ? 8 : 4;
  uint32_t draw[M];
  tv_sample<M>(seed, b, k, (uint32_t)N.n, draw);
  float A[8][9];
#pragma unroll
  for (int j = 0; j < M; j++) {
    const TvPoint P = tv_point(N, p1, p2, draw[j]);
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
  return tv_solve(A, x);
}

// chi2 of the distance of (xb, yb) to the line m * (xa, ya, 1).
__device__ __forceinline__ float tv_line_chi(const float (&m)[9], float xa, float ya, float xb, float yb, float w) {
  const float a = (m[0] * xa + m[1] * ya) + m[2];
  const float b = (m[3] * xa + m[4] * ya) + m[5];
  const float c = (m[6] * xa + m[7] * ya) + m[8];
  const float num = (a * xb + b * yb) + c;
  return ((num * num) / (a * a + b * b)) * w;
}
// chi2 of the distance of (xb, yb) to the image of (xa, ya) under m.
__device__ __forceinline__ float tv_transfer_chi(const float (&m)[9], float xa, float ya, float xb, float yb, float w) {
  const float inv = 1.0f / ((m[6] * xa + m[7] * ya) + m[8]);
  const float u = ((m[0] * xa + m[1] * ya) + m[2]) * inv;
  const float v = ((m[3] * xa + m[4] * ya) + m[5]) * inv;
  const float du = xb - u, dv = yb - v;
  return (du * du + dv * dv) * w;
}

// The sum of v over a full wave (all 64 lanes active), the same in every lane: four DPP steps leave each row of 16
// lanes with its own sum (xor 1, xor 2 inside the quads, then mirrored halves of 8 and of 16, whose partners hold equal
// partial sums by then), four lane reads add the rows.  (Six __shfl_xor steps are six LDS permutes and their address
// arithmetic, a third of the scoring loop.)
__device__ __forceinline__ uint32_t tv_wave_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_mov_dpp(x, 0xb1, 0xf, 0xf, true);    // quad_perm [1, 0, 3, 2]
  x += __builtin_amdgcn_mov_dpp(x, 0x4e, 0xf, 0xf, true);    // quad_perm [2, 3, 0, 1]
  x += __builtin_amdgcn_mov_dpp(x, 0x141, 0xf, 0xf, true);   // row_half_mirror
  x += __builtin_amdgcn_mov_dpp(x, 0x140, 0xf, 0xf, true);   // row_mirror
  return (uint32_t)(__builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
                    __builtin_amdgcn_readlane(x, 48));
}

// A model ready for scoring: f (last entry 1) and its second matrix: the transpose of F, the adjugate of H.
template <int MODEL>
struct TvModel {
  float f[9], g[9];
  __device__ __forceinline__ explicit TvModel(const float *x) {
#pragma unroll
    for (int i = 0; i < 8; i++) f[i] = x[i];
    f[8] = 1.0f;
    if (MODEL == 0) {
#pragma unroll
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
__device__ __forceinline__ uint32_t tv_score(const TvModel<MODEL> &m, const TvPoint &P, float w1, float w2, bool *inl) {
  constexpr float th = MODEL == 0 ? 3.841f : 5.991f;
  float ca, cb;
  if (MODEL == 0) {
    ca = tv_line_chi(m.f, P.x1, P.y1, P.x2, P.y2, w2);
    cb = tv_line_chi(m.g, P.x2, P.y2, P.x1, P.y1, w1);
  } else {
    ca = tv_transfer_chi(m.f, P.x1, P.y1, P.x2, P.y2, w2);
    cb = tv_transfer_chi(m.g, P.x2, P.y2, P.x1, P.y1, w1);
  }
  const bool oka = ca < th, okb = cb < th;                   // false for a NaN
  uint32_t s = 0;
  if (oka) s += (uint32_t)floorf((TV_TH_SCORE - ca) * 256.0f);
  if (okb) s += (uint32_t)floorf((TV_TH_SCORE - cb) * 256.0f);
  *inl = oka && okb;
  return s;
}

template <int MODEL>
__global__ __launch_bounds__(TV_THREADS) void k_two_view(const TvArgs A) {
  constexpr uint32_t M = MODEL == 0 ? 8 : 4;
  __shared__ float s_model[TV_MAX_HYP][8];                   // 32 KB
  __shared__ uint32_t s_score[TV_MAX_HYP];
  __shared__ uint8_t s_valid[TV_MAX_HYP];
  __shared__ unsigned long long s_sum[6];                    // Sx1, Sy1, Sx2, Sy2, D1, D2 (two's complement)
  __shared__ unsigned long long s_best;
  __shared__ uint32_t s_ninl;

  TV_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    // The thread's index is made opaque once per pair: otherwise every per-thread predicate below (tid < 6, tid == 0,
    // tid < hypotheses, ...) is hoisted over this loop and held in an SGPR pair for the whole kernel, and they spilled.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * A.stride;
    const int32_t *p1 = A.p1 + 2 * row, *p2 = A.p2 + 2 * row;
    uint8_t *inlier = A.inlier + row;
    uint32_t n = A.counts[b];
    n = n == TV_COUNT_INVALID ? 0u : (n < A.stride ? n : (uint32_t)A.stride);
    if (tid < 6) s_sum[tid] = 0;
    if (tid == 0) s_best = 0, s_ninl = 0;
    __syncthreads();

    // ---- 1. integer sums ----
    {
      long long a[4] = {0, 0, 0, 0};
      TV_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) {
        const int2 u = *(const int2 *)(p1 + 2 * (size_t)i), v = *(const int2 *)(p2 + 2 * (size_t)i);
        a[0] += tv_clamp(u.x), a[1] += tv_clamp(u.y), a[2] += tv_clamp(v.x), a[3] += tv_clamp(v.y);
      }
      if ((uint32_t)tid < n) {
#pragma unroll
        for (int c = 0; c < 4; c++) atomicAdd(&s_sum[c], (unsigned long long)a[c]);
      }
    }
    __syncthreads();
    TvNorm N;
    N.n = (int32_t)n, N.sx1 = (long long)s_sum[0], N.sy1 = (long long)s_sum[1], N.sx2 = (long long)s_sum[2], N.sy2 = (long long)s_sum[3];
    {
      long long d1 = 0, d2 = 0;
      TV_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) {
        const int2 u = *(const int2 *)(p1 + 2 * (size_t)i), v = *(const int2 *)(p2 + 2 * (size_t)i);
        d1 += llabs((long long)N.n * tv_clamp(u.x) - N.sx1) + llabs((long long)N.n * tv_clamp(u.y) - N.sy1);
        d2 += llabs((long long)N.n * tv_clamp(v.x) - N.sx2) + llabs((long long)N.n * tv_clamp(v.y) - N.sy2);
      }
      if ((uint32_t)tid < n) atomicAdd(&s_sum[4], (unsigned long long)d1), atomicAdd(&s_sum[5], (unsigned long long)d2);
    }
    __syncthreads();
    const long long D1 = (long long)s_sum[4], D2 = (long long)s_sum[5];
    if (tid == 0) {
      long long *st = A.stats + 8 * (size_t)b;
      st[0] = N.n, st[1] = N.sx1, st[2] = N.sy1, st[3] = D1, st[4] = N.sx2, st[5] = N.sy2, st[6] = D2, st[7] = 0;
    }
    bool have = n >= M && D1 != 0 && D2 != 0;                // uniform over the workgroup
    float w1 = 0.0f, w2 = 0.0f;
    if (have) {
      const float nn = (float)(2 * N.n * N.n);               // n <= 16384: 2 n n <= 2^29
      N.k1 = nn / (float)D1, N.k2 = nn / (float)D2;
      const float t1 = ((256.0f * (float)N.n) * N.k1) * A.sigma, t2 = ((256.0f * (float)N.n) * N.k2) * A.sigma;
      w1 = 1.0f / (t1 * t1), w2 = 1.0f / (t2 * t2);

      // ---- 2. one lane per hypothesis: sample and solve ----
      TV_ROLLED
      for (int k = tid; k < A.hypotheses; k += TV_THREADS) {
        float x[8];
        const bool ok = tv_hypothesis<MODEL>(N, p1, p2, A.seed, b, (uint32_t)k, x);
        *(float4 *)&s_model[k][0] = make_float4(x[0], x[1], x[2], x[3]);
        *(float4 *)&s_model[k][4] = make_float4(x[4], x[5], x[6], x[7]);
        s_valid[k] = ok ? 1 : 0;
        s_score[k] = 0;
      }
      __syncthreads();

      // ---- 3. one match per lane, all hypotheses ----
      TV_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * TV_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const TvPoint P = tv_point(N, p1, p2, live ? i : i0);
        TV_ROLLED
        for (int k = 0; k < A.hypotheses; k++) {
          if (!s_valid[k]) continue;                         // uniform
          const TvModel<MODEL> m(&s_model[k][0]);
          bool inl;
          const uint32_t s = tv_score<MODEL>(m, P, w1, w2, &inl);
          const uint32_t sum = tv_wave_sum(live ? s : 0u);   // wave-uniform
          if (lane == 0 && sum) atomicAdd(&s_score[k], sum);
        }
      }
      __syncthreads();

      // ---- 4. the best ----
      TV_ROLLED
      for (int k = tid; k < A.hypotheses; k += TV_THREADS) {
        const uint32_t s = s_score[k];
        if (s) atomicMax(&s_best, ((unsigned long long)s << 10) | (unsigned long long)(TV_MAX_HYP - 1 - k));
      }
      __syncthreads();
      have = s_best != 0;
    }

    // ---- 5. the mask and the outputs ----
    if (have) {
      const int kb = TV_MAX_HYP - 1 - (int)(s_best & (TV_MAX_HYP - 1));
      const TvModel<MODEL> m(&s_model[kb][0]);
      TV_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * TV_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const TvPoint P = tv_point(N, p1, p2, live ? i : i0);
        bool inl;
        (void)tv_score<MODEL>(m, P, w1, w2, &inl);
        inl = inl && live;
        if (live) inlier[i] = inl ? 1 : 0;
        const uint64_t mask = __ballot(inl);
        if (lane == 0 && mask) atomicAdd(&s_ninl, (uint32_t)__popcll(mask));
      }
      __syncthreads();
      if (tid == 0) A.best[b] = kb, A.score[b] = (uint32_t)(s_best >> 10), A.ninliers[b] = s_ninl;
      if (tid < 9) A.model_n[9 * (size_t)b + tid] = tid < 8 ? s_model[kb][tid] : 1.0f;
    } else {
      TV_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) inlier[i] = 0;
      if (tid == 0) A.best[b] = -1, A.score[b] = 0, A.ninliers[b] = 0;
      if (tid < 9) A.model_n[9 * (size_t)b + tid] = 0.0f;
    }
    __syncthreads();                                         // the next pair clears what this one still reads
  }
}

}  // namespace pg
