// pislam_mapupdate_kernels.h — the batched map-point update on the device (pislam_map_points_update_batch; include/
// pislam_hip.h), after ORB-SLAM's MapPoint::UpdateNormalAndDepth and
// MapPoint::ComputeDistinctiveDescriptors.  The header comment is the contract; the rules are stated once, in
// pislam_mapupdate_math.h, for these kernels and for the host probe.  No workspace: the map's flag lives in status[b],
// which the call zeroes with an asynchronous memset first.
//
// k_mapupdate_check: one thread per observation slot of the batch, walked in grid passes.  The thread checks its own
//   observation against the one before it; a violation stores 3 into status[b] (every writer stores the same word).
// k_mapupdate_points: one WAVE per chunk of 64 consecutive points of a map, walked in grid passes; lane q is point
//   64 c + q.  A valid list is ascending in obs_pt, so a point's observers are a segment that two binary searches find
//   (the second is the neighbour lane's first): no counter, no atomic, nothing to zero.  The lane writes nobs and first,
//   walks its observers in list order for the geometry (pmu::geometry) and writes normal, drange and pt_status.
//   Then the descriptors of the chunk's tracks of at most 64 observers: the observers of consecutive points are
//   consecutive in the list, so the wave takes as many whole tracks as fit its 64 lanes at a time (PACKS), lane l being
//   list slot s0 + l with its descriptor in eight registers.  Step j gives every lane the descriptor of observer j of its
//   own track through eight __shfl (the source lane differs from track to track, so it is no uniform lane read), eight
//   XORs and popcounts, and the lane keeps the distance in its own column of the wave's LDS tile (uint16 [64][64], row
//   j, column lane: no lane ever reads another lane's column, so the tile needs no barrier).  The median is pmu::rank_select over that column, the choice a minimum of pmu::choice_key over
//   the track through lane reads, and the winning lane stores its registers.  A map of two-observer points fills 64 of
//   64 lanes.
// k_mapupdate_long: the tracks of more than 64 observers, one workgroup each.  A workgroup scans 256 points at a time
//   for such tracks (nobs, which the kernel before it wrote); for one, thread t takes the rows t, t + 256, ..: its own
//   descriptor in registers, the others through loads whose address is the same in every lane, the distances recomputed
//   in each of the nine steps of pmu::rank_select (a row of 4096 distances per thread fits nowhere), the minimum key
//   through lane exchange and LDS.
#pragma once
#include "pislam_dev.h"
#include "pislam_mapupdate_math.h"

namespace pmuk {

constexpr int MU_THREADS = 256;                // the workgroup of all three kernels
constexpr int MU_WAVES = MU_THREADS / 64;
constexpr int MU_GRID_CAP = 1024;              // workgroups per launch of each kernel; more work is walked in passes
constexpr int MU_CHUNK = 64;                   // points per wave of k_mapupdate_points
constexpr int MU_WAVE_TRACK = 64;              // the longest track that a wave takes; a longer one takes a workgroup

struct MuArgs {
  const int32_t *obs_pt, *counts, *kf_counts;
  const uint16_t *obs_kf, *ref;                // ref or null
  const uint8_t *obs_level;
  const uint32_t *obs_desc, *pt_counts;        // obs_desc or null
  const float *poses, *xw;
  size_t kf_stride, stride, pt_stride, batch;
  pmu::Tables tab;
  float *normal, *drange;                      // each may be null
  uint32_t *desc;                              // or null
  int32_t *nobs, *first, *status;              // first or null
  uint8_t *pt_status;
};

__device__ __forceinline__ pmu::Map mu_map(const MuArgs &A, size_t b) {
  const size_t row = b * A.stride, pts = b * A.pt_stride;
  pmu::Map M;
  M.obs_pt = A.obs_pt + row, M.obs_kf = A.obs_kf + row, M.obs_level = A.obs_level + row;
  M.obs_desc = A.obs_desc ? A.obs_desc + row * pmu::WORDS : nullptr;
  M.poses = A.poses + b * A.kf_stride * 12, M.xw = A.xw + pts * 3, M.ref = A.ref ? A.ref + pts : nullptr;
  M.count = A.counts[b], M.stride = (int64_t)A.stride, M.nk = A.kf_counts[b], M.kf_stride = (int64_t)A.kf_stride;
  M.npt = (int64_t)A.pt_counts[b], M.pt_stride = (int64_t)A.pt_stride;
  return M;
}

__global__ __launch_bounds__(MU_THREADS) void k_mapupdate_check(const MuArgs A) {
  const size_t step = (size_t)gridDim.x * MU_THREADS, total = A.batch * A.stride;
  PISLAM_ROLLED
  for (size_t o = (size_t)blockIdx.x * MU_THREADS + threadIdx.x; o < total; o += step) {
    const size_t b = o / A.stride;
    const int64_t i = (int64_t)(o - b * A.stride);
    const pmu::Map M = mu_map(A, b);
    if (!pmu::shape_ok(M)) {
      if (i == 0) A.status[b] = 3;
      continue;
    }
    if (i < M.count && !pmu::obs_ok(M, i)) A.status[b] = 3;
  }
}

__global__ __launch_bounds__(MU_THREADS) void k_mapupdate_points(const MuArgs A) {
  __shared__ uint16_t s_row[MU_WAVES][MU_WAVE_TRACK * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint16_t *row = s_row[wave];
  const size_t chunks = (A.pt_stride + MU_CHUNK - 1) / MU_CHUNK, items = A.batch * chunks;
  PISLAM_ROLLED
  for (size_t item = (size_t)blockIdx.x * MU_WAVES + wave; item < items; item += (size_t)gridDim.x * MU_WAVES) {
    const size_t b = item / chunks, c = item - b * chunks;
    const pmu::Map M = mu_map(A, b);
    // (status[b] holds 0 or the 3 of the check, or already what this computes from it: the test reads the same)
    const int32_t code = pmu::status_of(A.status[b] == 3, M);
    if (c == 0 && lane == 0) A.status[b] = code;
    const int64_t p = (int64_t)(c * MU_CHUNK) + lane, npw = pmu::points_written(M);
    const bool live = p < npw;
    const size_t gp = b * A.pt_stride + (size_t)p;
    if (code != 0) {                           // (the same for the whole wave)
      if (live) {
        A.nobs[gp] = 0, A.pt_status[gp] = pmu::NO_OBSERVERS;
        if (A.first) A.first[gp] = -1;
      }
      continue;
    }
    // a lane beyond the map's points reads as an empty track behind the list
    const int32_t cnt = (int32_t)M.count;
    const int32_t lb = live ? pmu::segment_begin(M.obs_pt, M.count, p) : cnt;
    const int32_t nxt = __shfl_down(lb, 1);
    const int32_t end = lane < 63 ? nxt : (p + 1 < npw ? pmu::segment_begin(M.obs_pt, M.count, p + 1) : cnt);
    const int32_t n = end - lb;
    if (live) {
      A.nobs[gp] = n;
      if (A.first) A.first[gp] = n ? lb : -1;
      if (n == 0) {
        A.pt_status[gp] = pmu::NO_OBSERVERS;
      } else {
        const pmu::Geo g = pmu::geometry(M, A.tab, p, lb, n);
        A.pt_status[gp] = g.status;
        if (A.normal) A.normal[3 * gp] = g.normal[0], A.normal[3 * gp + 1] = g.normal[1], A.normal[3 * gp + 2] = g.normal[2];
        if (A.drange) A.drange[2 * gp] = g.drange[0], A.drange[2 * gp + 1] = g.drange[1];
      }
    }
    if (!A.desc) continue;
    // the descriptors: packs of whole tracks, at most 64 observers together
    PISLAM_ROLLED
    for (int q0 = 0; q0 < MU_CHUNK;) {
      const int32_t s0 = __shfl(lb, q0);
      const uint64_t fits = __ballot(lane >= q0 && end - s0 <= MU_WAVE_TRACK) >> q0;
      const int take = ~fits ? __builtin_ctzll(~fits) : 64;    // tracks q0 .. q0 + take - 1 (end ascends with the lane)
      if (take == 0) {                         // a long track: k_mapupdate_long's
        q0++;
        continue;
      }
      const int32_t total = __shfl(end, q0 + take - 1) - s0;
      q0 += take;
      if (total == 0) continue;
      const bool act = lane < total;
      const int32_t slot = s0 + (act ? lane : 0);
      const int32_t q = M.obs_pt[slot] - (int32_t)(c * MU_CHUNK);      // the lane's own track, a lane of this wave
      const int32_t start = __shfl(lb, q) - s0, nn = __shfl(n, q);      // its first lane and its length
      uint32_t own[pmu::WORDS];
#pragma unroll
      for (int k = 0; k < pmu::WORDS; k++) own[k] = M.obs_desc[(size_t)slot * pmu::WORDS + k];
      int steps = 0;
      PISLAM_ROLLED
      for (;; steps++) {
        const bool in = act && steps < nn;
        if (!__ballot(in)) break;
        const int src = in ? start + steps : lane;
        uint32_t d = 0;
#pragma unroll
        for (int k = 0; k < pmu::WORDS; k++) d += (uint32_t)__popc(own[k] ^ (uint32_t)__shfl((int)own[k], src));
        if (in) row[steps * 64 + lane] = (uint16_t)d;
      }
      uint32_t key = pmu::KEY_NONE;
      if (act) {
        const uint32_t med = pmu::rank_select((uint32_t)nn, pmu::median_rank((uint32_t)nn),
                                              [&](uint32_t j) { return (uint32_t)row[j * 64 + lane]; });
        key = pmu::choice_key(med, (uint32_t)(lane - start));
      }
      uint32_t best = pmu::KEY_NONE;
      PISLAM_ROLLED
      for (int j = 0; j < steps; j++) {
        const bool in = act && j < nn;
        const uint32_t other = (uint32_t)__shfl((int)key, in ? start + j : lane);
        best = in && other < best ? other : best;
      }
      if (act && (int32_t)pmu::key_observer(best) == lane - start) {
        uint32_t *out = A.desc + (b * A.pt_stride + (size_t)(c * MU_CHUNK) + (size_t)q) * pmu::WORDS;
#pragma unroll
        for (int k = 0; k < pmu::WORDS; k++) out[k] = own[k];
      }
    }
  }
}

__global__ __launch_bounds__(MU_THREADS) void k_mapupdate_long(const MuArgs A) {
  __shared__ int32_t s_n[MU_THREADS], s_first[MU_THREADS];
  __shared__ uint32_t s_key[MU_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t chunks = (A.pt_stride + MU_THREADS - 1) / MU_THREADS, items = A.batch * chunks;
  PISLAM_ROLLED
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t b = item / chunks, c = item - b * chunks;
    const pmu::Map M = mu_map(A, b);
    if (A.status[b] != 0) continue;            // (final by now, and the same for the whole workgroup)
    const int64_t p = (int64_t)(c * MU_THREADS) + tid;
    int32_t n = 0, f = 0;
    if (p < pmu::points_written(M)) {
      n = A.nobs[b * A.pt_stride + (size_t)p];
      if (n > MU_WAVE_TRACK) f = pmu::segment_begin(M.obs_pt, M.count, p);
    }
    if (__syncthreads_count(n > MU_WAVE_TRACK) == 0) continue;
    s_n[tid] = n, s_first[tid] = f;
    __syncthreads();
    PISLAM_ROLLED
    for (int t = 0; t < MU_THREADS; t++) {
      const int32_t nn = s_n[t];
      if (nn <= MU_WAVE_TRACK) continue;       // (the same for the whole workgroup)
      const uint32_t *D = M.obs_desc + (size_t)s_first[t] * pmu::WORDS;
      uint32_t best = pmu::KEY_NONE;
      PISLAM_ROLLED
      for (int32_t i = tid; i < nn; i += MU_THREADS) {
        uint32_t own[pmu::WORDS];
#pragma unroll
        for (int k = 0; k < pmu::WORDS; k++) own[k] = D[(size_t)i * pmu::WORDS + k];
        const uint32_t med = pmu::rank_select((uint32_t)nn, pmu::median_rank((uint32_t)nn),
                                              [&](uint32_t j) { return pmu::hamming(own, D + (size_t)j * pmu::WORDS); });
        const uint32_t key = pmu::choice_key(med, (uint32_t)i);
        best = key < best ? key : best;
      }
#pragma unroll
      for (int h = 32; h >= 1; h >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, h);
        best = o < best ? o : best;
      }
      if (lane == 0) s_key[wave] = best;
      __syncthreads();
#pragma unroll
      for (int v = 0; v < MU_WAVES; v++) best = s_key[v] < best ? s_key[v] : best;
      if (tid < pmu::WORDS)
        A.desc[(b * A.pt_stride + c * MU_THREADS + (size_t)t) * pmu::WORDS + tid] =
            D[(size_t)pmu::key_observer(best) * pmu::WORDS + tid];
      __syncthreads();                         // the next track rewrites the keys
    }
    __syncthreads();                           // the next chunk rewrites the lengths
  }
}

}  // namespace pmuk
