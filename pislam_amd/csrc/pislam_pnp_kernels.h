// pislam_pnp_kernels.h — batched absolute-pose RANSAC on the device (pislam_pnp_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a camera pose per frame from 3D-2D matches, by P3P on minimal samples, scored with the pose
// call's monocular chi2.  The header comment is the contract; the arithmetic lives once in pislam_pnp_math.h, for this
// kernel and for the host probe: what stays here is the threads' share of the work, the loads, the LDS atomics and the
// order of the four steps.
//
// One workgroup of PN_THREADS works on a frame, then on the frame PN_GRID_CAP further on, and so on; one launch per
// call, no workspace.  Per frame:
//   1. one LANE per hypothesis: counter-based sampling, the P3P solver, the choice among its solutions by the fourth
//      draw.  The solver has static indices only, so it never leaves the VGPRs.  The twelve pose words go to LDS;
//   2. scoring with one OBSERVATION per lane: a wave holds 64 observations' point, pixel and weight in registers and
//      walks over all hypotheses (the pose is an LDS broadcast read), integer wave sum, one LDS atomic add per wave and
//      hypothesis;
//   3. the best score (64-bit LDS atomic max over score << 10 | 1023 - k: the smallest k wins a tie);
//   4. one more pass over the observations with the winning pose for the mask, through the SAME scoring routine.
#pragma once
#include "pislam_dev.h"
#include "pislam_pnp_math.h"

namespace pn {

constexpr int PN_THREADS = 512;                // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs
constexpr int PN_WAVES = PN_THREADS / 64;
constexpr int PN_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes

struct PnArgs {
  const float *cam, *xw;                       // [batch][5], [batch][stride][3]
  const int32_t *obs;                          // [batch][stride][3]
  const uint8_t *level;                        // [batch][stride] or null
  const uint32_t *counts;
  size_t stride;
  int batch, hypotheses, nlevels, min_inliers;
  uint32_t seed;
  float inv_sigma2[pnm::MAX_LEVELS];
  int32_t *best;
  uint32_t *score, *ninliers;
  uint8_t *inlier;                             // [batch][stride]
  float *pose_out;                             // [batch][12]
  uint32_t *status;
};

__global__ __launch_bounds__(PN_THREADS) void k_pnp_ransac(const PnArgs A) {
  __shared__ float s_pose[pnm::MAX_HYP][12];                 // 48 KB
  __shared__ uint32_t s_score[pnm::MAX_HYP];
  __shared__ uint8_t s_valid[pnm::MAX_HYP];
  __shared__ unsigned long long s_best;
  __shared__ uint32_t s_ninl, s_nvalid;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    // The thread's index is made opaque once per frame: otherwise every per-thread predicate below is hoisted over
    // this loop and held in an SGPR pair for the whole kernel (see pg::k_two_view).
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * A.stride;
    const float *xw = A.xw + 3 * row;
    const int32_t *ob = A.obs + 3 * row;
    const uint8_t *lv = A.level ? A.level + row : nullptr;
    uint8_t *inlier = A.inlier + row;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    const float *tab = A.inv_sigma2;
    const int nlevels = A.nlevels;
    const auto fetch = [xw, ob, lv, tab, nlevels](uint32_t i) {
      return pnm::obs(xw + 3 * (size_t)i, ob + 3 * (size_t)i, lv ? lv + i : nullptr, tab, nlevels);
    };
    float cam[5];
#pragma unroll
    for (int i = 0; i < 5; i++) cam[i] = A.cam[5 * (size_t)b + i];
    const bool cam_ok = pnm::cam_ok(cam);                    // uniform over the workgroup
    const pnm::Cam C = pnm::make_cam(cam);
    if (tid == 0) s_best = 0, s_ninl = 0, s_nvalid = 0;
    __syncthreads();

    bool have = cam_ok && n >= (uint32_t)pnm::SAMPLE;
    if (have) {
      // ---- 1. one lane per hypothesis: sample, solve, choose ----
      PISLAM_ROLLED
      for (int k0 = 64 * wave; k0 < A.hypotheses; k0 += PN_THREADS) {
        const int k = k0 + lane;
        bool ok = false;
        if (k < A.hypotheses) {
          float T[12];
          ok = pnm::hypothesis(C, fetch, n, A.seed, b, (uint32_t)k, T);
          *(float4 *)&s_pose[k][0] = make_float4(T[0], T[1], T[2], T[3]);
          *(float4 *)&s_pose[k][4] = make_float4(T[4], T[5], T[6], T[7]);
          *(float4 *)&s_pose[k][8] = make_float4(T[8], T[9], T[10], T[11]);
          s_valid[k] = ok ? 1 : 0;
          s_score[k] = 0;
        }
        const uint64_t mask = __ballot(ok);
        if (lane == 0 && mask) atomicAdd(&s_nvalid, (uint32_t)__popcll(mask));
      }
      __syncthreads();

      // ---- 2. one observation per lane, all hypotheses ----
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * PN_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const pnm::Obs o = fetch(live ? i : i0);
        PISLAM_ROLLED
        for (int k = 0; k < A.hypotheses; k++) {
          if (!s_valid[k]) continue;                         // uniform
          float T[12];
          const float4 t0 = *(const float4 *)&s_pose[k][0], t1 = *(const float4 *)&s_pose[k][4], t2 = *(const float4 *)&s_pose[k][8];
          T[0] = t0.x, T[1] = t0.y, T[2] = t0.z, T[3] = t0.w, T[4] = t1.x, T[5] = t1.y, T[6] = t1.z, T[7] = t1.w;
          T[8] = t2.x, T[9] = t2.y, T[10] = t2.z, T[11] = t2.w;
          bool inl;
          const uint32_t s = pnm::score(T, C, o, &inl);
          const uint32_t sum = pdev::wave_sum_dpp(live ? s : 0u);   // wave-uniform
          if (lane == 0 && sum) atomicAdd(&s_score[k], sum);
        }
      }
      __syncthreads();

      // ---- 3. the best ----
      PISLAM_ROLLED
      for (int k = tid; k < A.hypotheses; k += PN_THREADS) {
        const uint32_t s = s_score[k];
        if (s) atomicMax(&s_best, pgm::best_key(s, k));
      }
      __syncthreads();
      have = s_best != 0;
    }

    // ---- 4. the mask and the outputs ----
    const uint32_t nvalid = s_nvalid;
    if (have) {
      const int kb = pgm::key_hypothesis(s_best);
      float T[12];
#pragma unroll
      for (int i = 0; i < 12; i++) T[i] = s_pose[kb][i];
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * PN_WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const pnm::Obs o = fetch(live ? i : i0);
        bool inl;
        (void)pnm::score(T, C, o, &inl);
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
      if (tid < 12) A.pose_out[12 * (size_t)b + tid] = s_pose[kb][tid];
    } else {
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += PN_THREADS) inlier[i] = 0;
      if (tid == 0) {
        A.best[b] = -1, A.score[b] = 0, A.ninliers[b] = 0;
        A.status[b] = cam_ok ? (2u | nvalid << 8) : 3u;
      }
      if (tid < 12) A.pose_out[12 * (size_t)b + tid] = 0.0f;
    }
    __syncthreads();                                         // the next frame clears what this one still reads
  }
}

}  // namespace pn
