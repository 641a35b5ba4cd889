// pislam_sim3_kernels.h — batched Sim(3) RANSAC on the device (pislam_sim3_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a similarity per (key frame, loop candidate) pair from 3D-3D matches, by Horn's closed form on
// minimal samples, scored by reprojection into both images.  The header comment is the contract; the arithmetic lives
// once in pislam_sim3_math.h, for this kernel and for the host probe: what stays here is the threads' share of the
// work, the loads, the LDS atomics and the order of the four steps.
//
// One workgroup of S3_THREADS works on a pair, then on the pair S3_GRID_CAP further on, and so on; one launch per call,
// no workspace.  Per pair:
//   1. one LANE per hypothesis: counter-based sampling and Horn's solver (the 4 x 4 eigenvector by cyclic Jacobi with
//      static indices only, so it never leaves the VGPRs).  The hypothesis's 14 words (R, t, s, 1 / s) go to LDS in a
//      record of 16;
//   2. scoring with one MATCH per lane: a wave holds 64 matches' points, pixels and weights in registers and walks over
//      all hypotheses (the record is an LDS broadcast read), integer wave sum, one LDS atomic add per wave and
//      hypothesis;
//   3. the best score (64-bit LDS atomic max over score << 10 | 1023 - k: the smallest k wins a tie);
//   4. one more pass over the matches with the winning similarity for the mask, through the SAME scoring routine.
#pragma once
#include "pislam_dev.h"
#include "pislam_sim3_math.h"

namespace s3 {

constexpr int S3_THREADS = 512;                // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs
constexpr int S3_WAVES = S3_THREADS / 64;
constexpr int S3_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes
constexpr int S3_RECORD = 16;                  // words of a hypothesis in LDS: s3m::WORDS, padded to four float4

struct S3Args {
  const float *cam1, *cam2, *x1, *x2;          // [batch][5] twice, [batch][stride][3] twice
  const int32_t *obs1, *obs2;                  // [batch][stride][3]
  const uint8_t *level1, *level2;              // [batch][stride], or both null
  const uint32_t *counts;
  size_t stride;
  int batch, hypotheses, nlevels, min_inliers, fixed_scale;
  uint32_t seed;
  float inv_sigma2[s3m::MAX_LEVELS];
  int32_t *best;
  uint32_t *score, *ninliers;
  uint8_t *inlier;                             // [batch][stride]
  float *sim_out;                              // [batch][13]
  uint32_t *status;
};

__device__ __forceinline__ void load_record(const float (*rec)[S3_RECORD], int k, float (&S)[s3m::WORDS]) {
  const float4 a = *(const float4 *)&rec[k][0], b = *(const float4 *)&rec[k][4], c = *(const float4 *)&rec[k][8];
  const float2 d = *(const float2 *)&rec[k][12];
  S[0] = a.x, S[1] = a.y, S[2] = a.z, S[3] = a.w, S[4] = b.x, S[5] = b.y, S[6] = b.z, S[7] = b.w;
  S[8] = c.x, S[9] = c.y, S[10] = c.z, S[11] = c.w, S[12] = d.x, S[13] = d.y;
}

__global__ __launch_bounds__(S3_THREADS) void k_sim3_ransac(const S3Args A) {
  __shared__ __attribute__((aligned(16))) float s_rec[s3m::MAX_HYP][S3_RECORD];   // 64 KB
  __shared__ uint32_t s_score[s3m::MAX_HYP];
  __shared__ uint8_t s_valid[s3m::MAX_HYP];
  __shared__ unsigned long long s_best;
  __shared__ uint32_t s_ninl, s_nvalid;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    // The thread's index is made opaque once per pair: otherwise every per-thread predicate below is hoisted over this
    // loop and held in an SGPR pair for the whole kernel (see pg::k_two_view).
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * A.stride;
    const float *x1 = A.x1 + 3 * row, *x2 = A.x2 + 3 * row;
    const int32_t *o1 = A.obs1 + 3 * row, *o2 = A.obs2 + 3 * row;
    const uint8_t *l1 = A.level1 ? A.level1 + row : nullptr, *l2 = A.level1 ? A.level2 + row : nullptr;
    uint8_t *inlier = A.inlier + row;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    const float *tab = A.inv_sigma2;
    const int nlevels = A.nlevels;
    const bool fixed = A.fixed_scale != 0;
    const auto fetch = [x1, x2, o1, o2, l1, l2, tab, nlevels](uint32_t i) {
      return s3m::match(x1 + 3 * (size_t)i, x2 + 3 * (size_t)i, o1 + 3 * (size_t)i, o2 + 3 * (size_t)i,
                        l1 ? l1 + i : nullptr, l1 ? l2 + i : nullptr, tab, nlevels);
    };
    float cam1[5], cam2[5];
#pragma unroll
    for (int i = 0; i < 5; i++) cam1[i] = A.cam1[5 * (size_t)b + i], cam2[i] = A.cam2[5 * (size_t)b + i];
    const bool cam_ok = s3m::cam_ok(cam1) && s3m::cam_ok(cam2);   // uniform over the workgroup
    const s3m::Cam C1 = s3m::make_cam(cam1), C2 = s3m::make_cam(cam2);
    if (tid == 0) s_best = 0, s_ninl = 0, s_nvalid = 0;
    __syncthreads();

    bool have = cam_ok && n >= (uint32_t)s3m::SAMPLE;
    if (have) {
      // ---- 1. one lane per hypothesis: sample, solve ----
      PISLAM_ROLLED
      for (int k0 = 64 * wave; k0 < A.hypotheses; k0 += S3_THREADS) {
        const int k = k0 + lane;
        bool ok = false;
        if (k < A.hypotheses) {
          float S[s3m::WORDS];
          ok = s3m::hypothesis(fetch, n, A.seed, b, (uint32_t)k, fixed, S);
          *(float4 *)&s_rec[k][0] = make_float4(S[0], S[1], S[2], S[3]);
          *(float4 *)&s_rec[k][4] = make_float4(S[4], S[5], S[6], S[7]);
          *(float4 *)&s_rec[k][8] = make_float4(S[8], S[9], S[10], S[11]);
          *(float2 *)&s_rec[k][12] = make_float2(S[12], S[13]);
          s_valid[k] = ok ? 1 : 0;
          s_score[k] = 0;
        }
        const uint64_t mask = __ballot(ok);
        if (lane == 0 && mask) atomicAdd(&s_nvalid, (uint32_t)__popcll(mask));
      }
      __syncthreads();

      // ---- 2. one match per lane, all hypotheses ----
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * S3_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const s3m::Match m = fetch(live ? i : i0);
        PISLAM_ROLLED
        for (int k = 0; k < A.hypotheses; k++) {
          if (!s_valid[k]) continue;                         // uniform
          float S[s3m::WORDS];
          load_record(s_rec, k, S);
          bool inl;
          const uint32_t s = s3m::score(S, C1, C2, m, &inl);
          const uint32_t sum = pdev::wave_sum_dpp(live ? s : 0u);   // wave-uniform
          if (lane == 0 && sum) atomicAdd(&s_score[k], sum);
        }
      }
      __syncthreads();

      // ---- 3. the best ----
      PISLAM_ROLLED
      for (int k = tid; k < A.hypotheses; k += S3_THREADS) {
        const uint32_t s = s_score[k];
        if (s) atomicMax(&s_best, pgm::best_key(s, k));
      }
      __syncthreads();
      have = s_best != 0;
    }

    // ---- 4. the mask and the outputs ----
    const uint32_t nvalid = s_nvalid;
    float *sim = A.sim_out + s3m::OUT_WORDS * (size_t)b;
    if (have) {
      const int kb = pgm::key_hypothesis(s_best);
      float S[s3m::WORDS];
      load_record(s_rec, kb, S);
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * S3_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const s3m::Match m = fetch(live ? i : i0);
        bool inl;
        (void)s3m::score(S, C1, C2, m, &inl);
        inl = inl && live;
        if (live) inlier[i] = inl ? 1 : 0;
        const uint64_t mask = __ballot(inl);
        if (lane == 0 && mask) atomicAdd(&s_ninl, (uint32_t)__popcll(mask));
      }
      __syncthreads();
      if (tid == 0) {
        const uint32_t ninl = s_ninl;
        A.best[b] = kb, A.score[b] = pgm::key_score(s_best), A.ninliers[b] = ninl;
        A.status[b] = (ninl < (uint32_t)A.min_inliers ? 1u : 0u) | nvalid << 8;
      }
      if (tid < s3m::OUT_WORDS) sim[tid] = s_rec[kb][tid];
    } else {
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += S3_THREADS) inlier[i] = 0;
      if (tid == 0) {
        A.best[b] = -1, A.score[b] = 0, A.ninliers[b] = 0;
        A.status[b] = cam_ok ? (2u | nvalid << 8) : 3u;
      }
      if (tid < s3m::OUT_WORDS) sim[tid] = 0.0f;
    }
    __syncthreads();                                         // the next pair clears what this one still reads
  }
}

}  // namespace s3
