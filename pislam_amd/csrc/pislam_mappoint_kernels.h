// pislam_mappoint_kernels.h — new map points from the selected matches of two key frames on the device
// (pislam_triangulate_batch; include/pislam_hip.h), after ORB-SLAM's
// LocalMapping::CreateNewMapPoints.  The header comment is the contract; the arithmetic is stated once, in
// pislam_mappoint_math.h, for this kernel and for the host probe.
//
// One workgroup of MP_THREADS = 256 runs a pair, then the pair MP_GRID_CAP further on.  No workspace.
//   * Thread 0 makes the pair's constants (R21, t21, the two camera centres, the inverse focal lengths and half
//     baselines: a hundred operations) once, into LDS; every lane copies them to registers after the barrier.
//   * One lane works on a slot: two 12-byte observations and two level bytes in, pmp::slot, 12 to 33 bytes out.  No
//     float crosses a lane.  The level tables and the parameters travel by value in the kernel arguments.
//   * npoints is an integer: the lanes count their status-0 slots, the wave sums by DPP, the four waves through LDS.
#pragma once
#include "pislam_dev.h"
#include "pislam_mappoint_math.h"

namespace pmk {

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / 64;
constexpr int MP_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes

struct MpArgs {
  const float *pose1, *pose2, *cam1, *cam2;
  const int32_t *obs1, *obs2;
  const uint8_t *level1, *level2;
  const uint32_t *counts;
  size_t stride;
  int batch;
  pmp::Tables tab;
  pmp::Params p;
  float *xw;
  uint8_t *status;
  float *normal, *drange;                      // each may be null
  uint32_t *npoints;
};

__global__ __launch_bounds__(MP_THREADS) void k_triangulate(const MpArgs A) {
  __shared__ pmp::Pair s_pair;
  __shared__ uint32_t s_ok;
  __shared__ uint32_t s_cnt[MP_WAVES];

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * A.stride;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    if (tid == 0)
      s_ok = pmp::pair_setup(A.pose1 + 12 * (size_t)b, A.pose2 + 12 * (size_t)b, A.cam1 + 5 * (size_t)b,
                             A.cam2 + 5 * (size_t)b, &s_pair) ? 1u : 0u;
    __syncthreads();
    const bool pair_ok = s_ok != 0;
    const pmp::Pair P = s_pair;
    uint32_t good = 0;
    PISLAM_ROLLED
    for (uint32_t i = tid; i < n; i += MP_THREADS) {
      const size_t o = row + i;
      pmp::Slot s{pmp::PAIR, pmp::NONE, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f}};
      if (pair_ok) {
        int32_t o1[3], o2[3];
#pragma unroll
        for (int k = 0; k < 3; k++) o1[k] = A.obs1[3 * o + k], o2[k] = A.obs2[3 * o + k];
        s = pmp::slot(P, o1, o2, (int)A.level1[o], (int)A.level2[o], A.tab, A.p);
      }
      good += s.status == pmp::OK ? 1u : 0u;
      A.status[o] = s.status;
#pragma unroll
      for (int k = 0; k < 3; k++) A.xw[3 * o + k] = s.xw[k];
      if (A.normal) {
#pragma unroll
        for (int k = 0; k < 3; k++) A.normal[3 * o + k] = s.normal[k];
      }
      if (A.drange) A.drange[2 * o] = s.drange[0], A.drange[2 * o + 1] = s.drange[1];
    }
    const uint32_t w = pdev::wave_sum_dpp(good);
    if (lane == 0) s_cnt[wave] = w;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0;
#pragma unroll
      for (int k = 0; k < MP_WAVES; k++) t += s_cnt[k];
      A.npoints[b] = t;
    }
    __syncthreads();                           // the next pair rewrites what this one still reads
  }
}

}  // namespace pmk
