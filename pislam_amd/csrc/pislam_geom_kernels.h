// pislam_geom_kernels.h — batched two-view RANSAC on the device (pislam_two_view_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a fundamental matrix or a homography per pair of matched point lists, scored the way
// ORB-SLAM's Initializer scores them.  The header comment is the contract; the arithmetic lives once in
// pislam_geom_math.h, for this kernel and for the host probe: what stays here is the threads' share of the work, the
// loads, the LDS atomics and the order of the five steps.
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
#include "pislam_dev.h"
#include "pislam_geom_math.h"

namespace pg {

constexpr int TV_THREADS = 512;                // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs
constexpr int TV_WAVES = TV_THREADS / 64;
constexpr int TV_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes

struct TvArgs {
  const int32_t *p1, *p2;                      // [batch][stride][2]
  const uint32_t *counts;
  size_t stride;
  int batch, hypotheses;
  uint32_t seed;
  float sigma;                                 // pgm::sigma_px(sigma_q8), computed on the host (exact)
  int32_t *best;
  uint32_t *score, *ninliers;
  uint8_t *inlier;                             // [batch][stride]
  float *model_n;                              // [batch][9]
  long long *stats;                            // [batch][8]
};

// Match i of a pair: two 8-byte loads.
__device__ __forceinline__ pgm::Match tv_load(const int32_t *p1, const int32_t *p2, uint32_t i) {
  const int2 a = *(const int2 *)(p1 + 2 * (size_t)i), b = *(const int2 *)(p2 + 2 * (size_t)i);
  return pgm::match(a.x, a.y, b.x, b.y);
}

template <int MODEL>
__global__ __launch_bounds__(TV_THREADS) void k_two_view(const TvArgs A) {
  constexpr uint32_t M = pgm::sample_size(MODEL);
  __shared__ float s_model[pgm::MAX_HYP][8];                 // 32 KB
  __shared__ uint32_t s_score[pgm::MAX_HYP];
  __shared__ uint8_t s_valid[pgm::MAX_HYP];
  __shared__ unsigned long long s_sum[6];                    // Sx1, Sy1, Sx2, Sy2, D1, D2 (two's complement)
  __shared__ unsigned long long s_best;
  __shared__ uint32_t s_ninl;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    // The thread's index is made opaque once per pair: otherwise every per-thread predicate below (tid < 6, tid == 0,
    // tid < hypotheses, ...) is hoisted over this loop and held in an SGPR pair for the whole kernel, and they spilled.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * A.stride;
    const int32_t *p1 = A.p1 + 2 * row, *p2 = A.p2 + 2 * row;
    uint8_t *inlier = A.inlier + row;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    const auto fetch = [p1, p2](uint32_t i) { return tv_load(p1, p2, i); };
    if (tid < 6) s_sum[tid] = 0;
    if (tid == 0) s_best = 0, s_ninl = 0;
    __syncthreads();

    // ---- 1. integer sums ----
    {
      long long a[4] = {0, 0, 0, 0};
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) {
        const pgm::Match m = fetch(i);
        a[0] += m.x1, a[1] += m.y1, a[2] += m.x2, a[3] += m.y2;
      }
      if ((uint32_t)tid < n) {
#pragma unroll
        for (int c = 0; c < 4; c++) atomicAdd(&s_sum[c], (unsigned long long)a[c]);
      }
    }
    __syncthreads();
    pgm::Norm N;
    N.n = (int32_t)n, N.sx1 = (long long)s_sum[0], N.sy1 = (long long)s_sum[1], N.sx2 = (long long)s_sum[2], N.sy2 = (long long)s_sum[3];
    {
      long long d1 = 0, d2 = 0;
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) {
        const pgm::Match m = fetch(i);
        d1 += pgm::spread(N.n, m.x1, m.y1, N.sx1, N.sy1), d2 += pgm::spread(N.n, m.x2, m.y2, N.sx2, N.sy2);
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
      N.k1 = pgm::scale(N.n, D1), N.k2 = pgm::scale(N.n, D2);
      w1 = pgm::weight(N.n, N.k1, A.sigma), w2 = pgm::weight(N.n, N.k2, A.sigma);

      // ---- 2. one lane per hypothesis: sample and solve ----
      PISLAM_ROLLED
      for (int k = tid; k < A.hypotheses; k += TV_THREADS) {
        float x[8];
        const bool ok = pgm::hypothesis<MODEL>(N, fetch, A.seed, b, (uint32_t)k, x);
        *(float4 *)&s_model[k][0] = make_float4(x[0], x[1], x[2], x[3]);
        *(float4 *)&s_model[k][4] = make_float4(x[4], x[5], x[6], x[7]);
        s_valid[k] = ok ? 1 : 0;
        s_score[k] = 0;
      }
      __syncthreads();

      // ---- 3. one match per lane, all hypotheses ----
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * TV_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const pgm::Point P = pgm::point(N, fetch(live ? i : i0));
        PISLAM_ROLLED
        for (int k = 0; k < A.hypotheses; k++) {
          if (!s_valid[k]) continue;                         // uniform
          const pgm::Model<MODEL> m(&s_model[k][0]);
          bool inl;
          const uint32_t s = pgm::score<MODEL>(m, P, w1, w2, &inl);
          const uint32_t sum = pdev::wave_sum_dpp(live ? s : 0u);   // wave-uniform
          if (lane == 0 && sum) atomicAdd(&s_score[k], sum);
        }
      }
      __syncthreads();

      // ---- 4. the best ----
      PISLAM_ROLLED
      for (int k = tid; k < A.hypotheses; k += TV_THREADS) {
        const uint32_t s = s_score[k];
        if (s) atomicMax(&s_best, pgm::best_key(s, k));
      }
      __syncthreads();
      have = s_best != 0;
    }

    // ---- 5. the mask and the outputs ----
    if (have) {
      const int kb = pgm::key_hypothesis(s_best);
      const pgm::Model<MODEL> m(&s_model[kb][0]);
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * TV_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const pgm::Point P = pgm::point(N, fetch(live ? i : i0));
        bool inl;
        (void)pgm::score<MODEL>(m, P, w1, w2, &inl);
        inl = inl && live;
        if (live) inlier[i] = inl ? 1 : 0;
        const uint64_t mask = __ballot(inl);
        if (lane == 0 && mask) atomicAdd(&s_ninl, (uint32_t)__popcll(mask));
      }
      __syncthreads();
      if (tid == 0) A.best[b] = kb, A.score[b] = pgm::key_score(s_best), A.ninliers[b] = s_ninl;
      if (tid < 9) A.model_n[9 * (size_t)b + tid] = tid < 8 ? s_model[kb][tid] : 1.0f;
    } else {
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += TV_THREADS) inlier[i] = 0;
      if (tid == 0) A.best[b] = -1, A.score[b] = 0, A.ninliers[b] = 0;
      if (tid < 9) A.model_n[9 * (size_t)b + tid] = 0.0f;
    }
    __syncthreads();                                         // the next pair clears what this one still reads
  }
}

}  // namespace pg
