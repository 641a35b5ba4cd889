// pislam_select_kernels.h — match selection on the device (pislam_match_select_batch; include/pislam_hip.h, DESIGN.md
// section 5.5): distance threshold, ratio test, cross-check, one-to-one claim and ORB-SLAM's rotation histogram over
// the idx / dist / dist2 arrays of any matcher, compacted into pair lists.  Integers only.
//
// One workgroup of SEL_THREADS per pair, one launch per call, no workspace.  Three walks over the pair's queries:
//   1. (rot_keep > 0) the histogram of the survivors of tests 1-5;  one wave ranks the 30 bins into a keep mask;
//   2. the compaction walk in blocks of SEL_THREADS queries: status, ballot / popcount prefix per wave, wave offsets
//      over the workgroup, sel_q / sel_t in ascending query order.
// Tests 1-4 are a pure function of the inputs (sel_early) and are recomputed wherever a query is looked at again, so
// no pass can decide them differently.  Test 5 (uniqueness) is a table of SEL_SLOTS uint32 minima in LDS over one
// chunk of SEL_SLOTS train indices, keys dist << 23 | i (dist <= 256 < 2^9, i < 2^22: exact), filled by atomicMin by
// ONE routine (sel_table) that every walk goes through; a query has lost when its chunk's slot holds another key.
// With nt <= SEL_SLOTS (the usual 1-4 k keypoints) the table is built once per call.  A pair with more train entries
// has 2-4 chunks: walk 1 builds each once; walk 2 builds a chunk again for every query block that has a proposal in
// it and finds another chunk loaded — nq / SEL_THREADS further fills of the table in the worst case.
#pragma once

namespace ps {

constexpr int SEL_THREADS = 1024;              // 16 waves
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_SLOTS = 16384;               // uint32 minima: 64 KB, two workgroups per CU
constexpr int SEL_SLOT_BITS = 14;
constexpr int SEL_BINS = 30;                   // ORB-SLAM's HISTO_LENGTH; the library's angle is one of 30 bins of 12 degrees
constexpr uint32_t SEL_NONE = 0xffffffffu;
constexpr size_t SEL_LDS_BYTES = sizeof(uint32_t) * (SEL_SLOTS + 32 + SEL_WAVES + 1);   // table, histogram, wave sums, keep mask

struct SelArgs {
  int32_t max_dist;
  uint32_t ratio_num, ratio_den;               // ratio_den 0: off
  int32_t unique, rot_keep, rot_min_pct;
  const int32_t *idx;
  const uint32_t *dist, *dist2;                // dist2 may be null (ratio_den is 0 then)
  const uint32_t *qcounts, *tcounts;
  const int32_t *back_idx;                     // or null
  const uint8_t *qangle, *tangle;              // both null iff rot_keep == 0
  size_t q_stride, t_stride;
  int32_t *sel_q, *sel_t;
  uint32_t *nsel;
  uint8_t *status;                             // or null
  uint32_t *rot_hist;                          // or null
};

// One pair's rows.
struct SelPair {
  const int32_t *idx;
  const uint32_t *dist, *dist2;
  const int32_t *back;
  uint32_t nq, nt;
};

// Tests 1-4 of query i < nq: the status (0 = a proposal) with its train index and key.
__device__ __forceinline__ uint32_t sel_early(const SelArgs &A, const SelPair &P, uint32_t i, uint32_t *j_out, uint32_t *key) {
  const int32_t j = P.idx[i];
  *j_out = (uint32_t)j;
  if (j < 0 || (uint32_t)j >= P.nt) return 1;
  const uint32_t d = P.dist[i];
  *key = (d << 23) | i;
  if (d > (uint32_t)A.max_dist) return 2;
  if (A.ratio_den) {
    const uint32_t d2 = P.dist2[i];
    if (d2 != SEL_NONE && (uint64_t)d * A.ratio_den >= (uint64_t)d2 * A.ratio_num) return 3;
  }
  if (P.back && P.back[j] != (int32_t)i) return 4;
  return 0;
}

// Makes the table hold the minima of chunk c (train indices c * SEL_SLOTS ...).  Uniform over the workgroup.
__device__ __forceinline__ void sel_table(const SelArgs &A, const SelPair &P, uint32_t *tab, int c, int *loaded) {
  if (*loaded == c) return;
  __syncthreads();                                           // the previous chunk's readers are done
  const uint32_t base = (uint32_t)c << SEL_SLOT_BITS;
  const uint32_t used = min(P.nt - base, (uint32_t)SEL_SLOTS);
  for (uint32_t s = threadIdx.x; s < used; s += SEL_THREADS) tab[s] = SEL_NONE;   // consecutive dwords: no bank conflict
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < P.nq; i += SEL_THREADS) {
    const int32_t j = P.idx[i];
    if (j < 0 || (uint32_t)j >= P.nt || ((uint32_t)j >> SEL_SLOT_BITS) != (uint32_t)c) continue;
    uint32_t jj, key;
    if (sel_early(A, P, i, &jj, &key) == 0) atomicMin(&tab[jj & (SEL_SLOTS - 1)], key);
  }
  __syncthreads();
  *loaded = c;
}

__global__ __launch_bounds__(SEL_THREADS) void k_match_select(const SelArgs A) {
  extern __shared__ uint32_t sel_lds[];
  uint32_t *tab = sel_lds;                                   // [SEL_SLOTS]
  uint32_t *hist = sel_lds + SEL_SLOTS;                      // [32]
  uint32_t *wsum = hist + 32;                                // [SEL_WAVES]
  uint32_t *keep_lds = wsum + SEL_WAVES;                     // [1]
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t nq = A.qcounts[b], nt = A.tcounts[b];
  nq = nq == SEL_NONE ? 0u : (nq < A.q_stride ? nq : (uint32_t)A.q_stride);   // PISLAM_COUNT_INVALID counts as 0
  nt = nt == SEL_NONE ? 0u : (nt < A.t_stride ? nt : (uint32_t)A.t_stride);
  const size_t qo = (size_t)b * A.q_stride, to = (size_t)b * A.t_stride;
  SelPair P;
  P.idx = A.idx + qo, P.dist = A.dist + qo, P.dist2 = A.dist2 ? A.dist2 + qo : nullptr;
  P.back = A.back_idx ? A.back_idx + to : nullptr;
  P.nq = nq, P.nt = nt;
  const uint8_t *qa = A.qangle ? A.qangle + qo : nullptr, *ta = A.tangle ? A.tangle + to : nullptr;
  const int nchunks = A.unique ? (int)((nt + SEL_SLOTS - 1) >> SEL_SLOT_BITS) : 0;   // 0: no table at all
  int loaded = -1;

  if (tid < 32) hist[tid] = 0;
  if (tid == 0) *keep_lds = 0;
  __syncthreads();

  // ---- walk 1: the histogram of the survivors of tests 1-5 ----
  if (A.rot_keep > 0) {
    for (int c = 0; c < max(nchunks, 1); c++) {
      if (nchunks) sel_table(A, P, tab, c, &loaded);
      for (uint32_t i = tid; i < nq; i += SEL_THREADS) {
        uint32_t j, key;
        if (sel_early(A, P, i, &j, &key) != 0) continue;
        if (nchunks && ((j >> SEL_SLOT_BITS) != (uint32_t)c || tab[j & (SEL_SLOTS - 1)] != key)) continue;
        const uint32_t a = qa[i], t = ta[j];
        if (a < SEL_BINS && t < SEL_BINS) atomicAdd(&hist[(a + SEL_BINS - t) % SEL_BINS], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {                                         // rank: lanes 0..29 count the bins that beat their own
      const uint32_t h = lane < SEL_BINS ? hist[lane] : 0u;
      uint32_t rank = 0, top = 0;
      for (int k = 0; k < SEL_BINS; k++) {
        const uint32_t hk = (uint32_t)__shfl((int)h, k, 64);
        rank += (hk > h || (hk == h && k < lane)) ? 1u : 0u;
        top = max(top, hk);
      }
      const bool keep = lane < SEL_BINS && rank < (uint32_t)A.rot_keep && h >= 1 &&
                        (uint64_t)100 * h >= (uint64_t)A.rot_min_pct * top;
      const uint64_t m = __ballot(keep);
      if (lane == 0) *keep_lds = (uint32_t)m;
    }
    __syncthreads();
  }
  if (A.rot_hist && tid < SEL_BINS) A.rot_hist[(size_t)b * SEL_BINS + tid] = hist[tid];
  const uint32_t keep_mask = *keep_lds;

  // ---- walk 2: status and compaction, ascending ----
  uint32_t out = 0;                                          // selected so far (uniform)
  for (uint32_t i0 = 0; i0 < nq; i0 += SEL_THREADS) {
    const uint32_t i = i0 + tid;
    const bool valid = i < nq;
    uint32_t j = 0, key = 0, st = 0xff;
    if (valid) st = sel_early(A, P, i, &j, &key);
    for (int c = 0; c < nchunks; c++) {
      const bool mine = st == 0 && (j >> SEL_SLOT_BITS) == (uint32_t)c;
      if (!__syncthreads_or(mine)) continue;                 // (also the barrier between two chunks' readers)
      sel_table(A, P, tab, c, &loaded);
      if (mine && tab[j & (SEL_SLOTS - 1)] != key) st = 5;
    }
    if (st == 0 && A.rot_keep > 0) {
      const uint32_t a = qa[i], t = ta[j];
      if (a >= SEL_BINS || t >= SEL_BINS || !((keep_mask >> ((a + SEL_BINS - t) % SEL_BINS)) & 1u)) st = 6;
    }
    if (valid && A.status) A.status[qo + i] = (uint8_t)st;
    const uint64_t m = __ballot(st == 0);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int w = 0; w < SEL_WAVES; w++) {
      const uint32_t v = wsum[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    if (st == 0) {
      const size_t o = qo + out + before + (uint32_t)pdev::ballot_rank(m);
      A.sel_q[o] = (int32_t)i;
      A.sel_t[o] = (int32_t)j;
    }
    out += total;
    __syncthreads();                                         // wsum is written again
  }
  if (tid == 0) A.nsel[b] = out;
}

}  // namespace ps
