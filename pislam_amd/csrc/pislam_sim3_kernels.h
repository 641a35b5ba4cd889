// pislam_sim3_kernels.h — batched Sim(3) RANSAC on the device (pislam_sim3_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a similarity per (key frame, loop candidate) pair from 3D-3D matches, by Horn's closed form on
// minimal samples, scored by reprojection into both images.  The header comment is the contract; the arithmetic lives
// once in pislam_sim3_math.h, for this kernel and for the host probe, and the steps of the RANSAC with their barriers
// in pislam_ransac_kernels.h.  What stays here is the call's own: the pair's row of every array, and the outputs with
// the status word.  A hypothesis is 14 words (R, t, s, 1 / s) in an LDS record of 16; the first 13 are sim_out.
#pragma once
#include "pislam_ransac_kernels.h"
#include "pislam_sim3_math.h"

namespace s3 {

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

struct Call {
  using Problem = s3m::Problem;
  static constexpr bool SETUP_SYNCS = false, COUNTS_VALID = true;
  uint8_t *inlier;
  Problem P;

  static __device__ __forceinline__ s3m::Pair pair(const S3Args &A, uint32_t b) {
    const size_t row = (size_t)b * A.stride;
    return s3m::Pair{A.cam1 + 5 * (size_t)b, A.cam2 + 5 * (size_t)b, A.x1 + 3 * row, A.x2 + 3 * row,
                     A.obs1 + 3 * row, A.obs2 + 3 * row, A.level1 ? A.level1 + row : nullptr,
                     A.level1 ? A.level2 + row : nullptr, A.inv_sigma2, A.nlevels,
                     psm::clamp_count(A.counts[b], A.stride), b};
  }
  __device__ __forceinline__ Call(const S3Args &A, uint32_t b, int)
      : inlier(A.inlier + (size_t)b * A.stride), P(pair(A, b), A.seed, A.fixed_scale != 0) {}

  __device__ __forceinline__ void finish(const S3Args &A, uint32_t b, int tid, const prk::Outcome &O,
                                         const float (*rec)[16]) const {
    if (tid == 0) {
      A.best[b] = O.best, A.score[b] = O.score, A.ninliers[b] = O.ninliers;
      A.status[b] = prk::status(O, P.cam_ok, A.min_inliers);
    }
    if (tid < s3m::OUT_WORDS) A.sim_out[s3m::OUT_WORDS * (size_t)b + tid] = O.best < 0 ? 0.0f : rec[O.best][tid];
  }
};

__global__ __launch_bounds__(prk::THREADS) void k_sim3_ransac(const S3Args A) { prk::ransac_batch<Call>(A); }

}  // namespace s3
