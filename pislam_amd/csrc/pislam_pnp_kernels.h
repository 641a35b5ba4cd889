// pislam_pnp_kernels.h — batched absolute-pose RANSAC on the device (pislam_pnp_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a camera pose per frame from 3D-2D matches, by P3P on minimal samples, scored with the pose
// call's monocular chi2.  The header comment is the contract; the arithmetic lives once in pislam_pnp_math.h, for this
// kernel and for the host probe, and the steps of the RANSAC with their barriers in pislam_ransac_kernels.h.  What
// stays here is the call's own: the frame's row of every array, and the outputs with the status word.  A hypothesis is
// the twelve pose words; the fourth draw chooses among the solver's solutions.
#pragma once
#include "pislam_ransac_kernels.h"
#include "pislam_pnp_math.h"

namespace pn {

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

struct Call {
  using Problem = pnm::Problem;
  static constexpr bool SETUP_SYNCS = false, COUNTS_VALID = true;
  uint8_t *inlier;
  Problem P;

  static __device__ __forceinline__ pnm::Frame frame(const PnArgs &A, uint32_t b) {
    const size_t row = (size_t)b * A.stride;
    return pnm::Frame{A.cam + 5 * (size_t)b, A.xw + 3 * row, A.obs + 3 * row, A.level ? A.level + row : nullptr,
                      A.inv_sigma2, A.nlevels, psm::clamp_count(A.counts[b], A.stride), b};
  }
  __device__ __forceinline__ Call(const PnArgs &A, uint32_t b, int)
      : inlier(A.inlier + (size_t)b * A.stride), P(frame(A, b), A.seed) {}

  __device__ __forceinline__ void finish(const PnArgs &A, uint32_t b, int tid, const prk::Outcome &O,
                                         const float (*rec)[12]) const {
    if (tid == 0) {
      A.best[b] = O.best, A.score[b] = O.score, A.ninliers[b] = O.ninliers;
      A.status[b] = prk::status(O, P.cam_ok, A.min_inliers);
    }
    if (tid < 12) A.pose_out[12 * (size_t)b + tid] = O.best < 0 ? 0.0f : rec[O.best][tid];
  }
};

__global__ __launch_bounds__(prk::THREADS) void k_pnp_ransac(const PnArgs A) { prk::ransac_batch<Call>(A); }

}  // namespace pn
