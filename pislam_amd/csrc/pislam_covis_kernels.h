// pislam_covis_kernels.h — the batched covisibility graph on the device (pislam_covisibility_batch; include/
// pislam_hip.h), after ORB-SLAM's KeyFrame::UpdateConnections, the spanning tree it fixes at a key
// frame's first call, and the statistic of LocalMapping::KeyFrameCulling.  The header comment is the contract; the rules
// are stated once, in pislam_covis_math.h, for these kernels and for the host probe.
//
// k_covis_count: one thread per observation slot of the batch, walked in grid passes.  The thread checks its own
//   observation against the one before it (a violation raises the map's flag: every writer stores the same word), then
//   adds what pcv::count_obs says with integer atomics into the map's dense matrix and its two counters in the context's
//   workspace, which the call zeroed.  Integer addition commutes, so the order of arrival cannot change a word.
// k_covis_rows: one workgroup per (map, key frame), walked in grid passes.  It reads row k of the matrix (contiguous),
//   finds the parent and the fallback as maxima of pcv::pick_of, compacts the qualifying entries into LDS with wave64
//   ballots (the order of the compaction is arbitrary: the keys are distinct and the sort makes the order definite),
//   sorts them as 64-bit keys and writes the row.
//   * The bitonic network is padded to the power of two at or above the row's count (at least 64), not to kf_stride.
//   * Steps with a stride of 64 keys or more go through LDS: the 32 lanes of a ds_read_b64 group touch 32 consecutive
//     keys, which are the 64 banks once each.  Steps with a stride below 64 would put lane t and lane t + 16 on the same
//     banks; each lane takes one key instead (consecutive: conflict free), exchanges it with lane ^ stride, and all the
//     steps from 32 down to 1 run in registers between one read and one write.
//   * LDS is sized by the launch (8 bytes per key of kf_stride rounded up to a power of two, at least 64) and the
//     workgroup has 64, 128 or 256 threads by kf_stride, so the rows of small maps share a compute unit.
#pragma once
#include "pislam_dev.h"
#include "pislam_covis_math.h"

namespace pcvk {

constexpr int CV_THREADS = 256;                // the count kernel's workgroup, and the row kernel's largest
constexpr int CV_GRID_CAP = 1024;              // workgroups per launch of either kernel; more work is walked in passes

struct CvArgs {
  const int32_t *obs_pt, *counts, *kf_counts;
  const uint16_t *obs_kf;
  const uint8_t *obs_level, *cull_mask;        // or null
  size_t kf_stride, stride, nb_stride, batch;
  pcv::Params p;
  uint16_t *nb_idx, *parent;
  int32_t *nb_weight, *nb_count, *kf_points, *kf_redundant, *status;
  pcv::Ws ws;
};

__device__ __forceinline__ pcv::Map cv_map(const CvArgs &A, size_t b) {
  const size_t row = b * A.stride;
  pcv::Map M;
  M.obs_pt = A.obs_pt + row, M.obs_kf = A.obs_kf + row;
  M.obs_level = A.obs_level ? A.obs_level + row : nullptr, M.cull_mask = A.cull_mask ? A.cull_mask + row : nullptr;
  M.count = A.counts[b], M.stride = (int64_t)A.stride, M.nk = A.kf_counts[b], M.kf_stride = (int64_t)A.kf_stride;
  return M;
}

__global__ __launch_bounds__(CV_THREADS) void k_covis_count(const CvArgs A) {
  const size_t step = (size_t)gridDim.x * CV_THREADS, total = A.batch * A.stride, ks = A.kf_stride;
  const auto add = [](uint32_t *p) { atomicAdd(p, 1u); };
  PISLAM_ROLLED
  for (size_t o = (size_t)blockIdx.x * CV_THREADS + threadIdx.x; o < total; o += step) {
    const size_t b = o / A.stride;
    const int64_t i = (int64_t)(o - b * A.stride);
    const pcv::Map M = cv_map(A, b);
    if (!pcv::shape_ok(M)) {
      if (i == 0) A.ws.bad[b] = 1u;
      continue;
    }
    if (i >= M.count) continue;
    if (!pcv::obs_ok(M, i)) {                  // (before anything is indexed by this observation's key frame)
      A.ws.bad[b] = 1u;
      continue;
    }
    pcv::count_obs(M, A.p, i, A.ws.W + b * ks * ks, A.ws.pts + b * ks, A.ws.red + b * ks, add);
  }
}

__device__ __forceinline__ uint64_t cv_shfl_xor(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t cv_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Ascending bitonic sort of keys[0, N) in LDS, N a power of two >= 64, by a workgroup of T threads (T a multiple of 64).
// Begins after and ends with a barrier.
__device__ __forceinline__ void cv_sort(uint64_t *keys, uint32_t N, uint32_t T, uint32_t tid) {
  PISLAM_ROLLED
  for (uint32_t k2 = 2; k2 <= N; k2 <<= 1) {
    uint32_t j = k2 >> 1;
    PISLAM_ROLLED
    for (; j >= 64; j >>= 1) {
      PISLAM_ROLLED
      for (uint32_t t = tid; t < N / 2; t += T) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = keys[i], c = keys[l];
        if ((a > c) == ((i & k2) == 0)) keys[i] = c, keys[l] = a;
      }
      __syncthreads();
    }
    PISLAM_ROLLED
    for (uint32_t e = tid; e < N; e += T) {    // (N is a multiple of 64: a wave is in or out as a whole)
      uint64_t v = keys[e];
      PISLAM_ROLLED
      for (uint32_t jj = j; jj >= 1; jj >>= 1) {
        const uint64_t p = cv_shfl_xor(v, (int)jj);
        const bool low = ((e & jj) == 0) == ((e & k2) == 0);
        v = low ? (v < p ? v : p) : (v > p ? v : p);
      }
      keys[e] = v;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CV_THREADS) void k_covis_rows(const CvArgs A) {
  extern __shared__ uint64_t cv_keys[];        // the launch gives 8 bytes per key of kf_stride rounded up (>= 64 keys)
  __shared__ uint64_t s_pick[2][CV_THREADS / 64];
  __shared__ uint32_t s_n;
  const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = T >> 6;
  const size_t ks = A.kf_stride, items = A.batch * ks;
  PISLAM_ROLLED
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t b = item / ks;
    const uint32_t k = (uint32_t)(item - b * ks);
    const pcv::Map M = cv_map(A, b);
    const int32_t code = pcv::status_of(A.ws.bad[b] != 0u, M);
    if (tid == 0 && k == 0) A.status[b] = code;
    if (code != 0 || (int64_t)k >= M.nk) {     // (the same for the whole workgroup: no barrier is skipped by a part of it)
      if (tid == 0) A.nb_count[item] = 0, A.parent[item] = pcv::NO_PARENT, A.kf_points[item] = 0, A.kf_redundant[item] = 0;
      continue;
    }
    const uint32_t nk = (uint32_t)M.nk;
    const uint32_t *row = A.ws.W + item * ks;
    if (tid == 0) s_n = 0;
    __syncthreads();
    uint64_t par = 0, fb = 0;
    PISLAM_ROLLED
    for (uint32_t j0 = 0; j0 < nk; j0 += T) {  // (every lane stays in the loop: the ballot and the broadcast need them)
      const uint32_t j = j0 + tid, w = (j < nk && j != k) ? row[j] : 0u;
      if (pcv::fallback_candidate(w, j, k)) fb = cv_max(fb, pcv::pick_of(w, j));
      if (pcv::parent_candidate(w, j, k)) par = cv_max(par, pcv::pick_of(w, j));
      const bool q = w > 0 && pcv::qualifies(w, A.p.min_weight);
      const uint64_t m = __ballot(q);
      uint32_t base = 0;
      if (lane == 0 && m) base = atomicAdd(&s_n, (uint32_t)__popcll(m));
      base = (uint32_t)__shfl((int)base, 0);
      if (q) cv_keys[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = pcv::sort_key(w, j);
    }
    PISLAM_ROLLED
    for (int h = 32; h >= 1; h >>= 1) par = cv_max(par, cv_shfl_xor(par, h)), fb = cv_max(fb, cv_shfl_xor(fb, h));
    if (lane == 0) s_pick[0][wave] = par, s_pick[1][wave] = fb;
    __syncthreads();
    PISLAM_ROLLED
    for (uint32_t v = 0; v < waves; v++) par = cv_max(par, s_pick[0][v]), fb = cv_max(fb, s_pick[1][v]);
    uint32_t n = s_n;
    if (n == 0 && fb) {                        // nobody qualifies: the best one does
      if (tid == 0) cv_keys[0] = pcv::sort_key(pcv::pick_weight(fb), pcv::pick_index(fb));
      n = 1;
    }
    if (n > 1) {
      uint32_t N = 64;
      while (N < n) N <<= 1;
      PISLAM_ROLLED
      for (uint32_t e = n + tid; e < N; e += T) cv_keys[e] = pcv::KEY_PAD;
      __syncthreads();
      cv_sort(cv_keys, N, T, tid);
    } else {
      __syncthreads();
    }
    const uint32_t nw = n < A.nb_stride ? n : (uint32_t)A.nb_stride;
    PISLAM_ROLLED
    for (uint32_t r = tid; r < nw; r += T) {
      const uint64_t key = cv_keys[r];
      A.nb_idx[item * A.nb_stride + r] = pcv::key_index(key), A.nb_weight[item * A.nb_stride + r] = pcv::key_weight(key);
    }
    if (tid == 0) {
      A.nb_count[item] = (int32_t)n, A.parent[item] = par ? (uint16_t)pcv::pick_index(par) : pcv::NO_PARENT;
      A.kf_points[item] = (int32_t)A.ws.pts[item], A.kf_redundant[item] = (int32_t)A.ws.red[item];
    }
    __syncthreads();                           // the next row rewrites the keys and the counter
  }
}

}  // namespace pcvk
