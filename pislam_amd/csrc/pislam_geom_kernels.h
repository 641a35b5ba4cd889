// pislam_geom_kernels.h — batched two-view RANSAC on the device (pislam_two_view_ransac_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): a fundamental matrix or a homography per pair of matched point lists, scored the way
// ORB-SLAM's Initializer scores them.  The header comment is the contract; the arithmetic lives once in
// pislam_geom_math.h, for this kernel and for the host probe, and the steps of the RANSAC with their barriers in
// pislam_ransac_kernels.h.  What stays here is the call's own: in front of the skeleton the pair's integer sums (Sx,
// Sy of both images, then D of both images; 64-bit LDS atomics: any order gives the same sum) with the `stats` row,
// behind it the outputs.  A hypothesis is the 8 unknowns of the 8 x 9 system, solved in registers.
#pragma once
#include "pislam_ransac_kernels.h"
#include "pislam_geom_math.h"

namespace pg {

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

template <int MODEL>
struct Call {
  using Problem = pgm::Problem<MODEL>;
  static constexpr bool SETUP_SYNCS = true;                  // the three barriers of the sums
  // The call has no status word and ignores the count.  H takes it all the same, in the form PnP and Sim(3) have; F
  // does not: with the ballot in its hypothesis loop F measured 1.75 % slower on pairs of 1000 matches, H without it
  // 1.0 % slower, each with its scoring loop unchanged (docs/experiments.md AE).
  static constexpr bool COUNTS_VALID = MODEL != 0;
  uint8_t *inlier;
  Problem P;

  // The integer sums of pair b, three barriers, and the problem they make.
  static __device__ __forceinline__ Problem sums(const TvArgs &A, uint32_t b, int tid) {
    __shared__ unsigned long long s_sum[6];                  // Sx1, Sy1, Sx2, Sy2, D1, D2 (two's complement)
    const size_t row = (size_t)b * A.stride;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    const pgm::PairIn I{A.p1 + 2 * row, A.p2 + 2 * row, n, b};
    if (tid < 6) s_sum[tid] = 0;
    __syncthreads();
    {
      long long a[4] = {0, 0, 0, 0};
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += prk::THREADS) {
        const pgm::Match m = pgm::match_at(I, i);
        a[0] += m.x1, a[1] += m.y1, a[2] += m.x2, a[3] += m.y2;
      }
      if ((uint32_t)tid < n) {
#pragma unroll
        for (int c = 0; c < 4; c++) atomicAdd(&s_sum[c], (unsigned long long)a[c]);
      }
    }
    __syncthreads();
    pgm::Norm N;
    N.n = (int32_t)n, N.sx1 = (long long)s_sum[0], N.sy1 = (long long)s_sum[1];
    N.sx2 = (long long)s_sum[2], N.sy2 = (long long)s_sum[3];
    {
      long long d1 = 0, d2 = 0;
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += prk::THREADS) {
        const pgm::Match m = pgm::match_at(I, i);
        d1 += pgm::spread(N.n, m.x1, m.y1, N.sx1, N.sy1), d2 += pgm::spread(N.n, m.x2, m.y2, N.sx2, N.sy2);
      }
      if ((uint32_t)tid < n) atomicAdd(&s_sum[4], (unsigned long long)d1), atomicAdd(&s_sum[5], (unsigned long long)d2);
    }
    __syncthreads();
    const long long D1 = (long long)s_sum[4], D2 = (long long)s_sum[5];
    if (tid == 0) pgm::stats_row(N, D1, D2, A.stats + 8 * (size_t)b);
    return Problem(I, N, D1, D2, A.sigma, A.seed);
  }

  __device__ __forceinline__ Call(const TvArgs &A, uint32_t b, int tid)
      : inlier(A.inlier + (size_t)b * A.stride), P(sums(A, b, tid)) {}

  __device__ __forceinline__ void finish(const TvArgs &A, uint32_t b, int tid, const prk::Outcome &O,
                                         const float (*rec)[8]) const {
    if (tid == 0) A.best[b] = O.best, A.score[b] = O.score, A.ninliers[b] = O.ninliers;
    if (tid < 9) A.model_n[9 * (size_t)b + tid] = O.best < 0 ? 0.0f : tid < 8 ? rec[O.best][tid] : 1.0f;
  }
};

template <int MODEL>
__global__ __launch_bounds__(prk::THREADS) void k_two_view(const TvArgs A) {
  prk::ransac_batch<Call<MODEL>>(A);
}
// F (the 8 x 9 system of eight matches) is stated to run at 3 waves per SIMD: left to itself the scheduler squeezes its
// wave-wise hypothesis loop into a fourth wave's registers and pays with 24 SGPRs spilled to VGPR lanes.
template <>
inline __global__ __launch_bounds__(prk::THREADS)
__attribute__((amdgpu_waves_per_eu(3, 3))) void k_two_view<0>(const TvArgs A) {
  prk::ransac_batch<Call<0>>(A);
}

}  // namespace pg
