// pislam_pose_kernels.h — batched motion-only pose optimisation on the device (pislam_pose_refine_batch;
// include/pislam_hip.h).  The header comment is the contract; the arithmetic is stated once, in
// pislam_pose_math.h and, the Levenberg rule, in pislam_refine_math.h, for this kernel and for the host probe.
//
// One workgroup runs the whole call for a frame in one launch (all rounds, passes, solves and classifications).  The
// launch shape, the partial sum a thread owns, the tree and the refused frame are those of pislam_refine_kernels.h.
//   * A frame of at most PO_RES * 256 = 2048 observations is loaded once and stays in registers over all passes; a
//     larger one is re-read (from L2) in every pass.  The active set is a bit mask per lane either way.
//   * Lane 0 runs the solve, the retraction and the Levenberg rule (prf::Lm) on state kept in LDS and broadcasts the
//     next pose as 12 floats: three barriers per pass.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_pose_math.h"

namespace po {

constexpr int PO_RES = 8;                      // register-resident observations per lane

struct PoArgs {
  const float *pose_in, *cam, *xw;
  const int32_t *obs;
  const uint8_t *level;                        // or null
  const uint32_t *counts;
  size_t stride;
  int batch, nlevels;
  float inv_sigma2[pq::MAX_LEVELS];
  pq::Params p;
  float *pose_out;
  uint8_t *inlier;
  uint32_t *ninliers, *status;
  double *cost;
};

struct PoObs {
  float X, Y, Z, u, v, ur, w;
  uint32_t flags;                              // bit 0: present with a level in range, bit 1: stereo
};

struct PoFrame {
  const float *xw;
  const int32_t *obs;
  const uint8_t *level;
  uint8_t *inlier;
  uint32_t n;
};

__device__ __forceinline__ PoObs po_load(const PoArgs &A, const PoFrame &F, uint32_t i) {
  PoObs o;
  o.X = o.Y = o.Z = o.u = o.v = o.ur = 0.0f, o.w = 1.0f, o.flags = 0;
  if (i < F.n) {
    const float *x = F.xw + 3 * (size_t)i;
    const int32_t *q = F.obs + 3 * (size_t)i;
    o.X = x[0], o.Y = x[1], o.Z = x[2];
    const int32_t ur = q[2];
    o.u = pq::obs_px(q[0]), o.v = pq::obs_px(q[1]);
    o.flags = 1;
    if (ur != pq::MONO) o.ur = pq::obs_px(ur), o.flags |= 2;
    if (F.level) {
      const int l = F.level[i];
      const float *tab = A.inv_sigma2;
      if (l < A.nlevels) o.w = tab[l];
      else o.flags = 0;
    }
  }
  return o;
}

// One observation of a pass: classification, the mask, the 30 per-lane partial sums.
__device__ __forceinline__ void po_one(const PoObs &o, uint32_t i, int s, const float *Tf, const float *cam, bool classify,
                                       bool robust, uint64_t &active, uint8_t *inlier, double (&acc)[pq::SUMS]) {
  const uint64_t bit = 1ull << s;
  const bool stereo = (o.flags & 2) != 0;
  if (!(o.flags & 1)) {                        // dead by its level
    if (classify) active &= ~bit, inlier[i] = 0;
    return;
  }
  if (!classify && !(active & bit)) return;
  float t[pq::TERMS], chi2 = 0.0f;
  const bool live = pq::obs_terms(Tf, cam, o.X, o.Y, o.Z, o.u, o.v, o.ur, stereo, o.w, robust, t, &chi2);
  if (classify) {
    const bool in = live && chi2 <= (stereo ? pq::TH_STEREO : pq::TH_MONO);
    active = in ? (active | bit) : (active & ~bit);
    inlier[i] = in ? 1 : 0;
  }
  if (live && (active & bit)) {
#pragma unroll
    for (int k = 0; k < pq::TERMS; k++) acc[k] += (double)t[k];
    acc[28] += 1.0;
    acc[29] += (double)chi2;
  }
}

// One pass over the frame's observations at the pose s_Tf: leaves the 30 sums in s_S (ends with a barrier).
template <bool RES>
__device__ __forceinline__ void po_pass(const PoArgs &A, const PoFrame &F, const PoObs (&r)[PO_RES], uint32_t q, int tid,
                                        const float *s_Tf, double (*s_part)[16], double *s_S, bool classify, bool robust,
                                        uint64_t &active) {
  float Tf[12], cam[5];
#pragma unroll
  for (int i = 0; i < 12; i++) Tf[i] = s_Tf[i];
#pragma unroll
  for (int i = 0; i < 5; i++) cam[i] = s_Tf[12 + i];
  double acc[pq::SUMS];
#pragma unroll
  for (int k = 0; k < pq::SUMS; k++) acc[k] = 0.0;
  if (RES) {
#pragma unroll
    for (int s = 0; s < PO_RES; s++) {
      const uint32_t i = q + 256u * (uint32_t)s;
      if (i < F.n) po_one(r[s], i, s, Tf, cam, classify, robust, active, F.inlier, acc);
    }
  } else {
    PISLAM_ROLLED
    for (int s = 0; s < pq::MAX_STRIDE / 256; s++) {
      const uint32_t i = q + 256u * (uint32_t)s;
      if (i < F.n) {
        const PoObs o = po_load(A, F, i);
        po_one(o, i, s, Tf, cam, classify, robust, active, F.inlier, acc);
      }
    }
  }
  prf::tree_sums(acc, tid, s_part, s_S);
}

template <bool RES>
__device__ __forceinline__ void po_frame(const PoArgs &A, const PoFrame &F, uint32_t b, int tid, uint32_t q, float *s_Tf,
                                         double (*s_part)[16], double *s_S, pq::Lm *s_lm, int *s_cmd) {
  PoObs r[PO_RES];
  if (RES) {
#pragma unroll
    for (int s = 0; s < PO_RES; s++) r[s] = po_load(A, F, q + 256u * (uint32_t)s);
  }
  const int rounds = A.p.rounds, iters = A.p.iters, hr = A.p.huber_rounds;
  uint64_t active = ~0ull;
  uint32_t evals = 1, code = 0, ninl = 0;
  double cost = 0.0;
  po_pass<RES>(A, F, r, q, tid, s_Tf, s_part, s_S, false, 0 < hr, active);
  PISLAM_ROLLED
  for (int rd = 0; rd < rounds; rd++) {
    if (tid == 0) s_lm->begin(s_S);
    PISLAM_ROLLED
    for (;;) {
      if (tid == 0) {
        const bool go = s_lm->next(pq::Rule{}, iters);
        *s_cmd = go ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 12; i++) s_Tf[i] = (float)(go ? s_lm->Tt[i] : s_lm->T[i]);
      }
      __syncthreads();
      if (!*s_cmd) break;
      po_pass<RES>(A, F, r, q, tid, s_Tf, s_part, s_S, false, rd < hr, active);
      evals++;
      if (tid == 0) s_lm->trial(s_S, A.p.eps);
    }
    po_pass<RES>(A, F, r, q, tid, s_Tf, s_part, s_S, true, rd + 1 < hr, active);
    evals++;
    ninl = (uint32_t)s_S[28], cost = s_S[29];
    if (rd + 1 < rounds && ninl < (uint32_t)A.p.min_obs) {
      code = 1;
      break;
    }
  }
  if (tid < 12) A.pose_out[12 * (size_t)b + tid] = (float)s_lm->T[tid];
  if (tid == 0) A.ninliers[b] = ninl, A.cost[b] = cost, A.status[b] = code | evals << 8;
}

__global__ __launch_bounds__(prf::THREADS) void k_pose_refine(const PoArgs A) {
  __shared__ pq::Lm s_lm;
  __shared__ double s_part[pq::SUMS][16];
  __shared__ double s_S[pq::SUMS + 2];
  __shared__ float s_Tf[12 + 5];               // the pose of the pass, then the camera
  __shared__ int s_cmd;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));              // keeps the per-thread predicates out of SGPRs held over the loop
    const uint32_t q = prf::partial_of(tid);
    const size_t row = (size_t)b * A.stride;
    PoFrame F;
    F.xw = A.xw + 3 * row, F.obs = A.obs + 3 * row, F.level = A.level ? A.level + row : nullptr, F.inlier = A.inlier + row;
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    F.n = n;
    float v = 0.0f;
    if (tid < 12) v = A.pose_in[12 * (size_t)b + tid];
    else if (tid < 17) v = A.cam[5 * (size_t)b + (tid - 12)];
    if (tid < 17) s_Tf[tid] = v;
    if (tid == 0) s_cmd = 1;
    __syncthreads();
    if (tid < 17 && !pq::finite_f(v)) s_cmd = 0;             // (every writer writes the same value)
    __syncthreads();
    const bool fin = s_cmd != 0;
    if (!fin || n < (uint32_t)A.p.min_obs) {
      prf::refuse<12>(A, b, tid, n, F.inlier, A.pose_out, v, fin);
    } else {
      if (tid < 12) s_lm.T[tid] = (double)v;
      __syncthreads();
      if (n <= (uint32_t)(PO_RES * 256))
        po_frame<true>(A, F, b, tid, q, s_Tf, s_part, s_S, &s_lm, &s_cmd);
      else
        po_frame<false>(A, F, b, tid, q, s_Tf, s_part, s_S, &s_lm, &s_cmd);
    }
    __syncthreads();                                         // the next frame rewrites what this one still reads
  }
}

}  // namespace po
