// pislam_sim3_refine_kernels.h — batched Sim(3) refinement on the device (pislam_sim3_refine_batch; include/pislam_hip.h,
// DESIGN.md section 5.5): ORB-SLAM's OptimizeSim3 per (key frame, loop candidate) pair.  The header comment is the
// contract; the arithmetic is stated once, in pislam_sim3_refine_math.h and, the Levenberg rule, in
// pislam_refine_math.h, for this kernel and for the host probe.
//
// The shape is k_pose_refine's (pislam_pose_kernels.h): one workgroup runs the whole call for a pair in one launch, with
// the launch shape and the partial sum a thread owns of pislam_refine_kernels.h.  The tree and the refused pair are
// written out here: through prf::tree_sums or prf::refuse this kernel spills 16 or 18 SGPRs where it spilled 14
// (docs/experiments.md AF).
//   * A pair of at most SR_RES * 256 = 1024 matches is loaded once and stays in registers over all passes (12 floats
//     and a flag per match); a larger one is re-read (from L2) in every pass.  The active set is a bit mask per lane.
//   * A match's forward terms are added to the lane's 38 binary64 accumulators before its backward terms are computed:
//     36 terms are alive at a time, not 72, and the order of the additions is the contract's.
//   * Lane 0 runs the 7 x 7 solve, the retraction and the Levenberg rule (prf::Lm) on state kept in LDS and broadcasts
//     the next similarity as 14 floats (R, t, s, 1 / s): three barriers per pass.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_sim3_refine_math.h"

namespace sr {

constexpr int SR_RES = 4;                      // register-resident matches per lane
constexpr int SR_BCAST = s3m::WORDS + 10;      // the similarity of the pass, then the two cameras

struct SrArgs {
  const float *sim_in, *cam1, *cam2, *x1, *x2;
  const int32_t *obs1, *obs2;
  const uint8_t *level1, *level2, *mask;       // the levels both or neither; mask or null
  const uint32_t *counts;
  size_t stride;
  int batch, nlevels;
  float inv_sigma2[s3r::MAX_LEVELS];
  s3r::Params p;
  float *sim_out;
  uint8_t *inlier;
  uint32_t *ninliers, *status;
  double *cost;
};

struct SrPair {
  const float *x1, *x2;
  const int32_t *obs1, *obs2;
  const uint8_t *level1, *level2, *mask;
  uint8_t *inlier;
  uint32_t n;
};

// Match i as the passes see it: dead (live == false) beyond n, by a level or by the mask.
__device__ __forceinline__ s3m::Match sr_load(const SrArgs &A, const SrPair &F, uint32_t i) {
  s3m::Match m;
#pragma unroll
  for (int k = 0; k < 3; k++) m.X1[k] = 0.0f, m.X2[k] = 0.0f;
  m.u1 = m.v1 = m.u2 = m.v2 = 0.0f, m.w1 = m.w2 = 1.0f, m.live = false;
  if (i < F.n) {
    const float *tab = A.inv_sigma2;
    m = s3m::match(F.x1 + 3 * (size_t)i, F.x2 + 3 * (size_t)i, F.obs1 + 3 * (size_t)i, F.obs2 + 3 * (size_t)i,
                   F.level1 ? F.level1 + i : nullptr, F.level1 ? F.level2 + i : nullptr, tab, A.nlevels);
    if (F.mask && !F.mask[i]) m.live = false;
  }
  return m;
}

// One match of a pass: classification, the mask, the 38 per-lane partial sums.
__device__ __forceinline__ void sr_one(const s3m::Match &m, uint32_t i, int s, const float *Sf, const s3m::Cam &C1,
                                       const s3m::Cam &C2, float th2, bool classify, bool robust, uint64_t &active,
                                       uint8_t *inlier, double (&acc)[s3r::SUMS]) {
  const uint64_t bit = 1ull << s;
  if (!m.live) {                               // dead under every similarity
    if (classify) active &= ~bit, inlier[i] = 0;
    return;
  }
  if (!classify && !(active & bit)) return;
  s3m::Side f, b;
  const bool live = s3r::sides(Sf, C1, C2, m, &f, &b);
  if (classify) {
    const bool in = live && f.chi2 <= th2 && b.chi2 <= th2;
    active = in ? (active | bit) : (active & ~bit);
    inlier[i] = in ? 1 : 0;
  }
  if (live && (active & bit)) {
    float t[s3r::TERMS];
    s3r::forward_terms(C1, f, m.w1, robust, th2, t);
#pragma unroll
    for (int k = 0; k < s3r::TERMS; k++) acc[k] += (double)t[k];
    s3r::backward_terms(Sf, C2, m.X1, b, m.w2, robust, th2, t);
#pragma unroll
    for (int k = 0; k < s3r::TERMS; k++) acc[k] += (double)t[k];
    acc[36] += 1.0;
    acc[37] += (double)f.chi2;
    acc[37] += (double)b.chi2;
  }
}

// One pass over the pair's matches at the similarity s_bc: leaves the 38 sums in s_S (ends with a barrier).
template <bool RES>
__device__ __forceinline__ void sr_pass(const SrArgs &A, const SrPair &F, const s3m::Match (&r)[SR_RES], uint32_t q, int tid,
                                        const float *s_bc, double (*s_part)[16], double *s_S, bool classify, bool robust,
                                        uint64_t &active) {
  float Sf[s3m::WORDS], cam[10];
#pragma unroll
  for (int i = 0; i < s3m::WORDS; i++) Sf[i] = s_bc[i];
#pragma unroll
  for (int i = 0; i < 10; i++) cam[i] = s_bc[s3m::WORDS + i];
  const s3m::Cam C1 = s3m::make_cam(cam), C2 = s3m::make_cam(cam + 5);
  const float th2 = A.p.th2;
  double acc[s3r::SUMS];
#pragma unroll
  for (int k = 0; k < s3r::SUMS; k++) acc[k] = 0.0;
  if (RES) {
#pragma unroll
    for (int s = 0; s < SR_RES; s++) {
      const uint32_t i = q + 256u * (uint32_t)s;
      if (i < F.n) sr_one(r[s], i, s, Sf, C1, C2, th2, classify, robust, active, F.inlier, acc);
    }
  } else {
    PISLAM_ROLLED
    for (int s = 0; s < s3r::MAX_STRIDE / 256; s++) {
      const uint32_t i = q + 256u * (uint32_t)s;
      if (i < F.n) {
        const s3m::Match m = sr_load(A, F, i);
        sr_one(m, i, s, Sf, C1, C2, th2, classify, robust, active, F.inlier, acc);
      }
    }
  }
  // the tree: steps 128, 64, 32, 16 inside the rows of 16 lanes (every lane is active here) ...
#pragma unroll
  for (int k = 0; k < s3r::SUMS; k++) acc[k] = pdev::row16_sum(acc[k]);
  if ((tid & 15) == 0) {
#pragma unroll
    for (int k = 0; k < s3r::SUMS; k++) s_part[k][tid >> 4] = acc[k];   // row tid / 16 = wave * 4 + lane / 16 = q % 16
  }
  __syncthreads();
  // ... steps 8, 4, 2, 1 over the 16 row sums, one sum per lane
  if (tid < s3r::SUMS) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = s_part[tid][j];
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1) {
#pragma unroll
      for (int j = 0; j < h; j++) v[j] += v[j + h];
    }
    s_S[tid] = v[0];
  }
  __syncthreads();
}

template <bool RES>
__device__ __forceinline__ void sr_pair(const SrArgs &A, const SrPair &F, uint32_t b, int tid, uint32_t q, float *s_bc,
                                        double (*s_part)[16], double *s_S, s3r::Lm *s_lm, int *s_cmd) {
  s3m::Match r[SR_RES];
  if (RES) {
#pragma unroll
    for (int s = 0; s < SR_RES; s++) r[s] = sr_load(A, F, q + 256u * (uint32_t)s);
  }
  const int rounds = A.p.rounds, iters = A.p.iters, hr = A.p.huber_rounds;
  const bool fixed = A.p.fixed_scale != 0;
  uint64_t active = ~0ull;
  uint32_t evals = 1, code = 0, ninl = 0;
  double cost = 0.0;
  sr_pass<RES>(A, F, r, q, tid, s_bc, s_part, s_S, false, 0 < hr, active);
  PISLAM_ROLLED
  for (int rd = 0; rd < rounds; rd++) {
    if (tid == 0) s_lm->begin(s_S);
    PISLAM_ROLLED
    for (;;) {
      if (tid == 0) {
        const bool go = s_lm->next(s3r::Rule{fixed}, iters);
        *s_cmd = go ? 1 : 0;
        s3r::pass_words(go ? s_lm->Tt : s_lm->T, s_bc);
      }
      __syncthreads();
      if (!*s_cmd) break;
      sr_pass<RES>(A, F, r, q, tid, s_bc, s_part, s_S, false, rd < hr, active);
      evals++;
      if (tid == 0) s_lm->trial(s_S, A.p.eps);
    }
    sr_pass<RES>(A, F, r, q, tid, s_bc, s_part, s_S, true, rd + 1 < hr, active);
    evals++;
    ninl = (uint32_t)s_S[36], cost = s_S[37];
    if (rd + 1 < rounds && ninl < (uint32_t)A.p.min_obs) {
      code = 1;
      break;
    }
  }
  if (tid < s3r::STATE) A.sim_out[s3r::STATE * (size_t)b + tid] = (float)s_lm->T[tid];
  if (tid == 0) A.ninliers[b] = ninl, A.cost[b] = cost, A.status[b] = code | evals << 8;
}

__global__ __launch_bounds__(prf::THREADS) void k_sim3_refine(const SrArgs A) {
  __shared__ s3r::Lm s_lm;
  __shared__ double s_part[s3r::SUMS][16];
  __shared__ double s_S[s3r::SUMS + 2];
  __shared__ float s_bc[SR_BCAST];             // the similarity of the pass (R, t, s, 1 / s), then cam1 and cam2
  __shared__ int s_cmd;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));              // keeps the per-thread predicates out of SGPRs held over the loop
    const uint32_t q = prf::partial_of(tid);
    const size_t row = (size_t)b * A.stride;
    SrPair F;
    F.x1 = A.x1 + 3 * row, F.x2 = A.x2 + 3 * row, F.obs1 = A.obs1 + 3 * row, F.obs2 = A.obs2 + 3 * row;
    F.level1 = A.level1 ? A.level1 + row : nullptr, F.level2 = A.level1 ? A.level2 + row : nullptr;
    F.mask = A.mask ? A.mask + row : nullptr, F.inlier = A.inlier + row;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    F.n = n;
    // lanes 0 .. 12 hold sim_in, 13 .. 17 cam1, 18 .. 22 cam2; the broadcast keeps slot 13 for 1 / s
    float v = 1.0f;
    if (tid < 13) v = A.sim_in[s3r::STATE * (size_t)b + tid];
    else if (tid < 18) v = A.cam1[5 * (size_t)b + (tid - 13)];
    else if (tid < 23) v = A.cam2[5 * (size_t)b + (tid - 18)];
    if (tid < 23) s_bc[tid < 13 ? tid : tid + 1] = v;
    if (tid == 0) s_cmd = 1;
    __syncthreads();
    bool bad = !s3r::finite_f(v);
    bad = bad || (tid == 12 && !(v > 0.0f));                             // s > 0
    bad = bad || ((tid == 13 || tid == 14 || tid == 18 || tid == 19) && v == 0.0f);   // fx, fy
    if (tid < 23 && bad) s_cmd = 0;                                      // (every writer writes the same value)
    __syncthreads();
    const bool fin = s_cmd != 0;
    if (!fin || n < (uint32_t)A.p.min_obs) {
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += prf::THREADS) F.inlier[i] = 0;
      if (tid < s3r::STATE) A.sim_out[s3r::STATE * (size_t)b + tid] = v;
      if (tid == 0) A.ninliers[b] = 0, A.cost[b] = 0.0, A.status[b] = fin ? 1u : 2u;
    } else {
      if (tid < s3r::STATE) s_lm.T[tid] = (double)v;
      if (tid == 0) s_bc[13] = s3r::fdiv(1.0f, s_bc[12]);
      __syncthreads();
      if (n <= (uint32_t)(SR_RES * 256))
        sr_pair<true>(A, F, b, tid, q, s_bc, s_part, s_S, &s_lm, &s_cmd);
      else
        sr_pair<false>(A, F, b, tid, q, s_bc, s_part, s_S, &s_lm, &s_cmd);
    }
    __syncthreads();                                         // the next pair rewrites what this one still reads
  }
}

}  // namespace sr
