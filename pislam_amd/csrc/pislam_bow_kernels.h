// Bag-of-words quantisation and word-guided matching (include/pislam_hip.h): a descriptor is
// dropped down a vocabulary tree of cluster centres to a leaf (its word); a pyramid's sorted multiset of words is its
// bag-of-words vector; two pyramids are matched only between descriptors whose words share an ancestor (a group).
// The reference ships neither a vocabulary nor a matcher: the semantics are this library's own.  Four kernels:
//   k_bow_descend   BOW_LPD lanes per descriptor (the descriptor in registers), all levels in one launch.  A step reads
//                   ONE run of child records: lane c takes children c and c + BOW_LPD, loads each child's descriptor and
//                   its (first, count) record at once (the addresses only depend on the parent), XOR-popcounts, and the
//                   lanes min-reduce dist << 8 | child with xor-shuffles; the winner's record travels with its key, so a
//                   level costs one dependent load latency, not two.  No LDS, no branches around the loads.
//   k_bow_vector    one workgroup per pyramid: bitonic sort of the words in LDS, run heads flagged and scanned, the
//                   distinct words and their run lengths written in ascending order.
//   k_bow_index     one workgroup per pair: pm::lds_counting_sort (the sort of pm::k_scaled_index) with the train entry's
//                   group id as the bin (ids at or above ngroups are not indexed).
//   k_match_bow     pm::WIN_LPQ lanes per query walking the one run of its group, (best, second) on dist << 16 | index
//                   kept, merged and stored by the functions the window matchers use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pislam_match_kernels.h"

namespace pb {

constexpr int BOW_MAX_CHILDREN = 32;
constexpr int BOW_MAX_DEPTH = 16;
constexpr int BOW_LPD = 16;                          // lanes per descriptor: children c and c + 16
constexpr int BOW_THREADS = 256;
constexpr int BOW_DPW = BOW_THREADS / BOW_LPD;       // descriptors per workgroup pass
constexpr int BOW_VEC_MAX = 16384;                   // k_bow_vector: keys of one pyramid in LDS (64 KiB)
constexpr int BOW_VEC_THREADS = 1024;
constexpr int BOW_MAX_GROUPS = pm::WIN_MAX_CELLS;    // LDS histogram of k_bow_index

// Node record (host: pislam_vocab_create).  Inner node: x = first child, y = child count (1..32).  Leaf: x = word id,
// y = group id << 8 (the count bits are 0).
__device__ __forceinline__ uint32_t bow_count(uint2 m) { return m.y & 0xffu; }

// grid (descriptor tiles, batch), BOW_THREADS threads; desc [batch][stride][WORDS]; node_desc [nnodes][WORDS] (256-byte
// aligned base), node_meta [nnodes]; outputs [batch][stride], group / wdist may be null.  The host validated the tree:
// every child range lies inside [1, nnodes) and no path is longer than BOW_MAX_DEPTH.
template <int WORDS>
__global__ __launch_bounds__(BOW_THREADS) void k_bow_descend(const uint32_t *__restrict__ node_desc,
                                                             const uint2 *__restrict__ node_meta,
                                                             const uint32_t *__restrict__ desc,
                                                             const uint32_t *__restrict__ count, size_t stride,
                                                             uint32_t *__restrict__ word, uint32_t *__restrict__ group,
                                                             uint32_t *__restrict__ wdist) {
  const int b = blockIdx.y;
  const uint32_t n = pm::win_count(count[b], stride);
  const uint32_t sub = threadIdx.x % BOW_LPD;
  const uint2 root = node_meta[0];
  for (uint32_t q0 = blockIdx.x * (uint32_t)BOW_DPW; q0 < n; q0 += gridDim.x * (uint32_t)BOW_DPW) {
    const uint32_t i = q0 + threadIdx.x / BOW_LPD;
    const size_t o = (size_t)b * stride + i;
    uint32_t qd[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; w++) qd[w] = 0;
    uint2 m = make_uint2(0u, 0u);                      // past the count: a leaf, no step
    if (i < n) {
      const uint32_t *qp = desc + o * WORDS;
#pragma unroll
      for (int w = 0; w < WORDS; w++) qd[w] = qp[w];
      m = root;
    }
    uint32_t key = 0;
    // (the lanes of a descriptor hold the same m, so they leave the loop together and the shuffles stay among them)
    for (int step = 0; step < BOW_MAX_DEPTH && bow_count(m) != 0; step++) {
      const uint32_t first = m.x, cnt = bow_count(m);
      // both children's records are always loaded (a lane past the count re-reads the last child): no branch between
      // the four loads, all in flight together
      const uint32_t c0 = sub, c1 = sub + BOW_LPD;
      const uint32_t n0 = first + min(c0, cnt - 1), n1 = first + min(c1, cnt - 1);
      const uint2 m0 = node_meta[n0], m1 = node_meta[n1];
      const uint32_t d0 = pm::win_popc<WORDS>(qd, node_desc + (size_t)n0 * WORDS);
      const uint32_t d1 = pm::win_popc<WORDS>(qd, node_desc + (size_t)n1 * WORDS);
      const uint32_t k0 = c0 < cnt ? (d0 << 8) | c0 : 0xffffffffu;
      const uint32_t k1 = c1 < cnt ? (d1 << 8) | c1 : 0xffffffffu;
      key = min(k0, k1);                               // (keys are unique per child: ties go to the smallest child)
      m = k1 < k0 ? m1 : m0;
#pragma unroll
      for (int s = 1; s < BOW_LPD; s <<= 1) {
        const uint32_t ok = __shfl_xor(key, s, 64), ox = __shfl_xor(m.x, s, 64), oy = __shfl_xor(m.y, s, 64);
        if (ok < key) key = ok, m = make_uint2(ox, oy);
      }
    }
    if (sub == 0 && i < n) {
      word[o] = m.x;
      if (group) group[o] = m.y >> 8;
      if (wdist) wdist[o] = key >> 8;
    }
  }
}

// grid (batch), BOW_VEC_THREADS threads; word [batch][stride], stride <= BOW_VEC_MAX; bow_word / bow_tf [batch][stride],
// bow_n [batch].  Slots at and beyond bow_n[b] are not written.
__global__ __launch_bounds__(BOW_VEC_THREADS) void k_bow_vector(const uint32_t *__restrict__ word,
                                                                const uint32_t *__restrict__ count, size_t stride,
                                                                uint32_t *__restrict__ bow_word,
                                                                uint32_t *__restrict__ bow_tf,
                                                                uint32_t *__restrict__ bow_n) {
  __shared__ uint32_t key[BOW_VEC_MAX];
  __shared__ uint16_t start[BOW_VEC_MAX];                // first sorted position of the run with a given rank
  __shared__ uint32_t wave_sum[BOW_VEC_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t n = pm::win_count(count[b], stride);
  if (n == 0) {
    if (tid == 0) bow_n[b] = 0;
    return;
  }
  // the smallest power of two that holds the words; the padding sorts to the end (a word of the same value as the
  // padding is indistinguishable from it, so the first n sorted slots are the words whatever they are)
  uint32_t N = 2;
  while (N < n) N <<= 1;
  const uint32_t *wp = word + (size_t)b * stride;
  for (uint32_t i = tid; i < N; i += BOW_VEC_THREADS) key[i] = i < n ? wp[i] : 0xffffffffu;
  __syncthreads();
  for (uint32_t k = 2; k <= N; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < N / 2; t += BOW_VEC_THREADS) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint32_t a = key[lo], c = key[hi];
        if ((a > c) == ((lo & k) == 0)) key[lo] = c, key[hi] = a;
      }
      __syncthreads();
    }
  }
  // run heads: every thread counts those of a contiguous chunk, the chunk sums are scanned across the workgroup
  const uint32_t chunk = (n + BOW_VEC_THREADS - 1) / BOW_VEC_THREADS;
  const uint32_t i0 = min(tid * chunk, n), i1 = min(i0 + chunk, n);
  uint32_t s = 0;
  for (uint32_t i = i0; i < i1; i++) s += (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
  uint32_t total;
  uint32_t rank = pm::block_scan<BOW_VEC_THREADS>(s, wave_sum, &total);
  uint32_t *ow = bow_word + (size_t)b * stride, *ot = bow_tf + (size_t)b * stride;
  for (uint32_t i = i0; i < i1; i++) {
    if (i == 0 || key[i] != key[i - 1]) {
      ow[rank] = key[i];
      start[rank] = (uint16_t)i;
      rank++;
    }
  }
  __syncthreads();
  for (uint32_t r = tid; r < total; r += BOW_VEC_THREADS) ot[r] = (r + 1 < total ? (uint32_t)start[r + 1] : n) - start[r];
  if (tid == 0) bow_n[b] = total;
}

// grid (batch), pm::WIN_INDEX_THREADS threads.  tgroup [batch][t_stride]; grp_off [batch][ngroups + 1],
// ent_idx [batch][t_stride] = original index, ent_desc [batch][t_stride][words], both sorted by group:
// pm::lds_counting_sort with the group id as the bin, as pm::k_scaled_index runs it with the cell.  Scatter order inside
// a group varies between runs; the match results do not (the key is unique per index).
__global__ __launch_bounds__(pm::WIN_INDEX_THREADS) void k_bow_index(uint32_t ngroups, int words,
                                                                     const uint32_t *__restrict__ tgroup,
                                                                     const uint32_t *__restrict__ tdesc,
                                                                     const uint32_t *__restrict__ tcount, size_t t_stride,
                                                                     uint32_t *__restrict__ grp_off,
                                                                     uint32_t *__restrict__ ent_idx,
                                                                     uint32_t *__restrict__ ent_desc) {
  __shared__ uint32_t hist[BOW_MAX_GROUPS];
  __shared__ uint32_t wave_sum[pm::WIN_INDEX_THREADS / 64];
  const int b = blockIdx.x;
  const uint32_t *gp = tgroup + (size_t)b * t_stride;
  const uint32_t *dp = tdesc + (size_t)b * t_stride * words;
  uint32_t *ip = ent_idx + (size_t)b * t_stride;
  uint32_t *ep = ent_desc + (size_t)b * t_stride * words;
  pm::lds_counting_sort<pm::WIN_INDEX_THREADS>(
      ngroups, pm::win_count(tcount[b], t_stride), hist, wave_sum, grp_off + (size_t)b * (ngroups + 1),
      [&](uint32_t j) {
        const uint32_t g = gp[j];
        return g < ngroups ? (int32_t)g : -1;
      },
      [&](uint32_t slot, uint32_t j) {
        ip[slot] = j;
        for (int w = 0; w < words; w++) ep[(size_t)slot * words + w] = dp[(size_t)j * words + w];
      });
}

// grid (query tiles, batch), pm::WIN_THREADS threads; q_stride / t_stride in entries; outputs [batch][q_stride].
template <int WORDS>
__global__ __launch_bounds__(pm::WIN_THREADS) void k_match_bow(uint32_t ngroups, const uint32_t *__restrict__ qdesc,
                                                               const uint32_t *__restrict__ qgroup,
                                                               const uint32_t *__restrict__ qcount, size_t q_stride,
                                                               size_t t_stride, const uint32_t *__restrict__ grp_off,
                                                               const uint32_t *__restrict__ ent_idx,
                                                               const uint32_t *__restrict__ ent_desc,
                                                               int32_t *__restrict__ idx, uint32_t *__restrict__ dist,
                                                               uint32_t *__restrict__ dist2) {
  const int b = blockIdx.y;
  const uint32_t nq = pm::win_count(qcount[b], q_stride);
  const uint32_t sub = threadIdx.x % pm::WIN_LPQ;
  const uint32_t *off = grp_off + (size_t)b * (ngroups + 1);
  const uint32_t *ip = ent_idx + (size_t)b * t_stride;
  const uint32_t *ep = ent_desc + (size_t)b * t_stride * WORDS;
  for (uint32_t q0 = blockIdx.x * (uint32_t)pm::WIN_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)pm::WIN_QPW) {
    const uint32_t i = q0 + threadIdx.x / pm::WIN_LPQ;
    const size_t o = (size_t)b * q_stride + i;
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    uint32_t e = 0, e1 = 0;                             // the run of the query's group (empty: past the count, no group)
    const uint32_t *qp = nullptr;
    if (i < nq) {
      const uint32_t g = qgroup[o];
      if (g < ngroups) {
        e = off[g] + sub, e1 = off[g + 1];
        qp = qdesc + o * WORDS;
      }
    }
    uint32_t qd[WORDS];
    pm::load_query<WORDS>(qd, qp);
    for (; e < e1; e += pm::WIN_LPQ)
      pm::pair_push(best, second, (pm::win_popc<WORDS>(qd, ep + (size_t)e * WORDS) << 16) | ip[e]);
    pm::pair_merge_lanes<pm::WIN_LPQ>(best, second);
    if (sub == 0 && i < nq) pm::store_match(o, best, second, idx, dist, dist2);
  }
}

}  // namespace pb
