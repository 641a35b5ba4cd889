// pislam_refine_kernels.h — what the two Levenberg refinement kernels (po::k_pose_refine in pislam_pose_kernels.h,
// sr::k_sim3_refine in pislam_sim3_refine_kernels.h) share on the device beside the Levenberg rule
// of pislam_refine_math.h (prf::Lm, run by lane 0): the launch shape, the partial sum a thread owns, the contract's tree
// over the partial sums and the refused element.  One workgroup of THREADS runs the whole call for a batch element in
// one launch, then the element GRID_CAP further on.  No workspace.
#pragma once
#include "pislam_dev.h"
#include "pislam_refine_math.h"

namespace prf {

constexpr int THREADS = 256;
constexpr int GRID_CAP = 1024;                 // workgroups per launch; a larger batch is walked in passes

// The contract's partial sum of thread (wave, lane): q = wave * 4 + lane / 16 + 16 * rev4(lane % 16), that is the items
// q, q + 256, q + 512, ... in ascending order.  The bits are laid out so that the halving tree's steps 128, 64, 32, 16
// are the lane exchanges xor 1, 2, 4, 8 inside a row of 16 lanes and the steps 8, 4, 2, 1 combine the 16 row sums.
__device__ __forceinline__ uint32_t partial_of(int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t l4 = (uint32_t)lane & 15u;
  const uint32_t rev = (l4 & 1u) << 3 | (l4 & 2u) << 1 | (l4 & 4u) >> 1 | (l4 & 8u) >> 3;
  return (uint32_t)wave << 2 | (uint32_t)lane >> 4 | rev << 4;
}

// The tree over the 256 partial sums of each of SUMS sums: leaves them in S (ends with a barrier).
template <int SUMS>
__device__ __forceinline__ void tree_sums(double (&acc)[SUMS], int tid, double (*part)[16], double *S) {
  // steps 128, 64, 32, 16 inside the rows of 16 lanes (every lane is active here; four DPP moves, both partners add) ...
#pragma unroll
  for (int k = 0; k < SUMS; k++) acc[k] = pdev::row16_sum(acc[k]);
  if ((tid & 15) == 0) {
#pragma unroll
    for (int k = 0; k < SUMS; k++) part[k][tid >> 4] = acc[k];   // row tid / 16 = wave * 4 + lane / 16 = q % 16
  }
  __syncthreads();
  // ... steps 8, 4, 2, 1 over the 16 row sums through LDS, one sum per lane
  if (tid < SUMS) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = part[tid][j];
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1) {
#pragma unroll
      for (int j = 0; j < h; j++) v[j] += v[j + h];
    }
    S[tid] = v[0];
  }
  __syncthreads();
}

// The refused element b (a bad input: status 2; fewer than min_obs items: status 1): its mask is cleared and its state
// copied out.  v is the thread's word of the state as the call received it (threads below STATE).
template <int STATE, class ARGS>
__device__ __forceinline__ void refuse(const ARGS &A, uint32_t b, int tid, uint32_t n, uint8_t *inlier, float *out, float v,
                                       bool fin) {
  PISLAM_ROLLED
  for (uint32_t i = tid; i < n; i += THREADS) inlier[i] = 0;
  if (tid < STATE) out[STATE * (size_t)b + tid] = v;
  if (tid == 0) A.ninliers[b] = 0, A.cost[b] = 0.0, A.status[b] = fin ? 1u : 2u;
}

}  // namespace prf
