// pislam_ransac_kernels.h — the RANSAC skeleton of pislam_two_view_ransac_batch, pislam_pnp_ransac_batch and
// pislam_sim3_ransac_batch on the device, stated ONCE for the three kernels.  What differs
// between the calls is a PROBLEM type in the call's *_math.h (pislam_ransac_math.h lists what it supplies; the host
// probes run the same types through prk::host_ransac there).
//
// On the device one workgroup of THREADS works on a batch element, then on the element GRID_CAP further on, and so on;
// one launch per call, no workspace.  A CALL type (the call's *_kernels.h) adds what is the call's own: CALL(A, b, tid)
// is the set-up and holds the problem `P` and the element's `inlier` row (SETUP_SYNCS: it passes a barrier of its own,
// which then also orders the skeleton's clearing of its LDS words); finish(A, b, tid, outcome, rec) writes the outputs
// (rec: the records in LDS, rec[outcome.best] the winner's); COUNTS_VALID: the count of valid hypotheses is taken
// (without it outcome.nvalid is 0; only a call that ignores the count may go without).  Per element:
//   1. one LANE per hypothesis, wave by wave: the solver is reached with static indices only, so it never leaves the
//      VGPRs; the record goes to LDS (a row of WORDS rounded up to whole float4), a ballot counts the valid ones
//      (COUNTS_VALID);
//   2. scoring with one ITEM per lane: a wave holds 64 items in registers and walks over all hypotheses (the record is
//      an LDS broadcast read; the skip of an invalid one is uniform), integer wave sum, one LDS atomic add per wave and
//      hypothesis;
//   3. the best score: a 64-bit LDS atomic max over the keys;
//   4. one more pass over the items with the winning record for the mask, through the SAME score(); without a model
//      the mask is cleared.
// A barrier stands between the steps and one closes the element: the next element clears what this one still reads.
#pragma once
#include "pislam_dev.h"
#include "pislam_ransac_math.h"

namespace prk {

constexpr int THREADS = 512;                   // 8 waves: two per SIMD, so a lane may hold up to 256 VGPRs
constexpr int WAVES = THREADS / 64;
constexpr int GRID_CAP = 1024;                 // workgroups per launch; a larger batch is walked in passes

template <int WORDS>
struct Lds {
  static constexpr int RECORD = (WORDS + 3) & ~3;
  static_assert(WORDS % 4 == 0 || WORDS % 4 == 2, "a record is float4s and at most one float2");
  __attribute__((aligned(16))) float rec[MAX_HYP][RECORD];   // 32, 48 or 64 KB
  uint32_t score[MAX_HYP];
  uint8_t valid[MAX_HYP];
  unsigned long long best;
  uint32_t ninl, nvalid;
};

template <int WORDS>
__device__ __forceinline__ void store_record(float *row, const float (&r)[WORDS]) {
#pragma unroll
  for (int i = 0; i + 4 <= WORDS; i += 4) *(float4 *)&row[i] = make_float4(r[i], r[i + 1], r[i + 2], r[i + 3]);
  if (WORDS % 4) *(float2 *)&row[WORDS - 2] = make_float2(r[WORDS - 2], r[WORDS - 1]);
}
template <int WORDS>
__device__ __forceinline__ void load_record(const float *row, float (&r)[WORDS]) {
#pragma unroll
  for (int i = 0; i + 4 <= WORDS; i += 4) {
    const float4 v = *(const float4 *)&row[i];
    r[i] = v.x, r[i + 1] = v.y, r[i + 2] = v.z, r[i + 3] = v.w;
  }
  if (WORDS % 4) {
    const float2 v = *(const float2 *)&row[WORDS - 2];
    r[WORDS - 2] = v.x, r[WORDS - 1] = v.y;
  }
}

// The whole kernel: A has batch and hypotheses next to what CALL reads.
template <class CALL, class ARGS>
__device__ __forceinline__ void ransac_batch(const ARGS &A) {
  using Problem = typename CALL::Problem;
  constexpr int WORDS = Problem::WORDS;
  __shared__ Lds<WORDS> L;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    // The thread's index is made opaque once per element: otherwise every per-thread predicate below and in CALL
    // (tid == 0, tid < 12, ...) is hoisted over this loop and held in an SGPR pair for the whole kernel, and they
    // spilled.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) L.best = 0, L.ninl = 0, L.nvalid = 0;
    const CALL call(A, b, tid);
    const Problem &P = call.P;
    const uint32_t n = P.n;
    if (!CALL::SETUP_SYNCS) __syncthreads();                 // a set-up with barriers of its own has passed this one

    bool have = P.have;
    if (have) {
      // ---- 1. one lane per hypothesis ----
      PISLAM_ROLLED
      for (int k0 = 64 * wave; k0 < A.hypotheses; k0 += THREADS) {
        const int k = k0 + lane;
        bool ok = false;
        if (k < A.hypotheses) {
          float r[WORDS];
          ok = P.hypothesis((uint32_t)k, r);
          store_record(L.rec[k], r);
          L.valid[k] = ok ? 1 : 0;
          L.score[k] = 0;
        }
        if (CALL::COUNTS_VALID) {
          const uint64_t mask = __ballot(ok);
          if (lane == 0 && mask) atomicAdd(&L.nvalid, (uint32_t)__popcll(mask));
        }
      }
      __syncthreads();

      // ---- 2. one item per lane, all hypotheses ----
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const typename Problem::Item it = P.item(live ? i : i0);
        PISLAM_ROLLED
        for (int k = 0; k < A.hypotheses; k++) {
          if (!L.valid[k]) continue;                         // uniform
          float r[WORDS];
          load_record(L.rec[k], r);
          bool inl;
          const uint32_t s = P.score(r, it, &inl);
          const uint32_t sum = pdev::wave_sum_dpp(live ? s : 0u);   // wave-uniform
          if (lane == 0 && sum) atomicAdd(&L.score[k], sum);
        }
      }
      __syncthreads();

      // ---- 3. the best ----
      PISLAM_ROLLED
      for (int k = tid; k < A.hypotheses; k += THREADS) {
        const uint32_t s = L.score[k];
        if (s) atomicMax(&L.best, best_key(s, k));
      }
      __syncthreads();
      have = L.best != 0;
    }

    // ---- 4. the mask and the outputs ----
    const uint32_t nvalid = L.nvalid;
    if (have) {
      const int kb = key_hypothesis(L.best);
      float r[WORDS];
      load_record(L.rec[kb], r);
      PISLAM_ROLLED
      for (uint32_t i0 = 64u * wave; i0 < n; i0 += 64u * WAVES) {
        const uint32_t i = i0 + lane;
        const bool live = i < n;
        const typename Problem::Item it = P.item(live ? i : i0);
        bool inl;
        (void)P.score(r, it, &inl);
        inl = inl && live;
        if (live) call.inlier[i] = inl ? 1 : 0;
        const uint64_t mask = __ballot(inl);
        if (lane == 0 && mask) atomicAdd(&L.ninl, (uint32_t)__popcll(mask));
      }
      __syncthreads();
      call.finish(A, b, tid, Outcome{kb, key_score(L.best), L.ninl, nvalid}, L.rec);
    } else {
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += THREADS) call.inlier[i] = 0;
      call.finish(A, b, tid, Outcome{-1, 0, 0, nvalid}, L.rec);
    }
    __syncthreads();                                         // the next element clears what this one still reads
  }
}

}  // namespace prk
