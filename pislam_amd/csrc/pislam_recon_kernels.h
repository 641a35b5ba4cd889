// pislam_recon_kernels.h — batched two-view reconstruction on the device (pislam_two_view_reconstruct_batch;
// include/pislam_hip.h).  The header comment is the contract; the arithmetic is stated once, in
// pislam_recon_math.h, for this kernel and for the host probe.
//
// One workgroup of RC_THREADS = 256 runs a pair, then the pair RC_GRID_CAP further on.  No workspace.
//   * Pass 1 walks the pair's matches once, one match per lane and step, and evaluates every candidate on it.  The
//     candidates are the same for every lane: the loop over them is rolled and reads the twelve words of one at a time
//     from a wave-uniform address (three 16-byte loads that hit the cache), so the lanes hold one candidate, not eight.
//     (Moving the words to SGPRs with readfirstlane saved 2 VGPRs and spilled 4 SGPRs: not kept.)  A lane sees at most
//     16384 / 256 = 64 matches, so its 16 counters (good and parallax per candidate) are bytes of two 64-bit words; the
//     17th is the number of used matches.
//   * The counters are summed over the wave by DPP and over the four waves through LDS; lane 0 makes the choice.
//   * Pass 2 recomputes the winner only and writes xw / point (zeros where the pair has no winner).
#pragma once
#include "pislam_dev.h"
#include "pislam_recon_math.h"

namespace pr {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_GRID_CAP = 1024;              // workgroups per launch; a larger batch is walked in passes
constexpr int RC_COUNTERS = 2 * prm::MAX_CAND + 1;

struct RcArgs {
  const int32_t *p1, *p2;
  const uint32_t *counts;
  const uint8_t *mask;                         // or null
  const float *cam, *cand;
  size_t stride;
  int batch;
  prm::Params p;
  int32_t *best;
  uint32_t *status, *ngood, *npar;
  float *pose_out, *xw;
  uint8_t *point;
};

__device__ __forceinline__ prm::Match rc_match(const prm::Pair &P, const int32_t *p1, const int32_t *p2, uint32_t i) {
  const int2 u = *(const int2 *)(p1 + 2 * (size_t)i), v = *(const int2 *)(p2 + 2 * (size_t)i);
  return prm::match_setup(P, u.x, u.y, v.x, v.y);
}

__global__ __launch_bounds__(RC_THREADS) void k_reconstruct(const RcArgs A) {
  __shared__ uint32_t s_cnt[RC_WAVES][RC_COUNTERS];
  __shared__ uint32_t s_fin[prm::MAX_CAND];
  __shared__ uint32_t s_code, s_cbest;

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {   // b + 1024 fits 32 bits unsigned
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));              // keeps the per-thread predicates out of SGPRs held over the loop
    const int lane = tid & 63, wave = tid >> 6;
    const int ncand = A.p.ncand;
    const size_t row = (size_t)b * A.stride;
    const int32_t *p1 = A.p1 + 2 * row, *p2 = A.p2 + 2 * row;
    const uint8_t *mask = A.mask ? A.mask + row : nullptr;
    const float *cand = A.cand + 12 * ((size_t)b * (size_t)ncand);
    const uint32_t n = psm::clamp_count(A.counts[b], A.stride);
    prm::Pair P;
    const bool cam_ok = prm::pair_setup(A.cam + 4 * (size_t)b, A.p.sigma_q8, &P);
    if (tid < prm::MAX_CAND) s_fin[tid] = tid < ncand && prm::cand_finite(cand + 12 * tid) ? 1u : 0u;
    __syncthreads();
    uint32_t fin = 0;
#pragma unroll
    for (int c = 0; c < prm::MAX_CAND; c++) fin |= s_fin[c] << c;
    fin = (uint32_t)__builtin_amdgcn_readfirstlane((int)fin);

    // ---- pass 1: the counts ----
    unsigned long long good = 0, par = 0;      // a byte per candidate, at most 64 each
    uint32_t used = 0;
    PISLAM_ROLLED
    for (uint32_t i = tid; i < n; i += RC_THREADS) {
      if (mask && !mask[i]) continue;
      used++;
      if (!cam_ok) continue;
      const prm::Match m = rc_match(P, p1, p2, i);
      PISLAM_ROLLED
      for (int c = 0; c < ncand; c++) {
        if (!(fin >> c & 1u)) continue;
        const float *cd = cand + 12 * c;
        float C[12], X[3];
#pragma unroll
        for (int k = 0; k < 12; k++) C[k] = cd[k];
        const uint32_t f = prm::evaluate(C, P, m, A.p.cos_parallax, A.p.cos_point, X);
        good += (unsigned long long)(f & prm::GOOD) << (8 * c);
        par += (unsigned long long)((f & prm::PARALLAX) >> 1) << (8 * c);
      }
    }
#pragma unroll
    for (int c = 0; c < prm::MAX_CAND; c++) {
      const uint32_t g = pdev::wave_sum_dpp((uint32_t)(good >> (8 * c)) & 0xffu);
      const uint32_t q = pdev::wave_sum_dpp((uint32_t)(par >> (8 * c)) & 0xffu);
      if (lane == 0) s_cnt[wave][c] = g, s_cnt[wave][prm::MAX_CAND + c] = q;
    }
    {
      const uint32_t u = pdev::wave_sum_dpp(used);
      if (lane == 0) s_cnt[wave][2 * prm::MAX_CAND] = u;
    }
    __syncthreads();

    // ---- the choice ----
    if (tid == 0) {
      uint32_t t[RC_COUNTERS];
#pragma unroll
      for (int k = 0; k < RC_COUNTERS; k++) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < RC_WAVES; w++) s += s_cnt[w][k];
        t[k] = s;
      }
      int cb = 0;
      const uint32_t code = prm::choose(t, t + prm::MAX_CAND, A.p, t[2 * prm::MAX_CAND], cam_ok, &cb);
      s_code = code, s_cbest = (uint32_t)cb;
      A.status[b] = code | (uint32_t)cb << 8;
      A.best[b] = code == prm::OK ? cb : -1;
#pragma unroll
      for (int c = 0; c < prm::MAX_CAND; c++) {
        A.ngood[prm::MAX_CAND * (size_t)b + c] = code == prm::NO_INPUT ? 0u : t[c];
        A.npar[prm::MAX_CAND * (size_t)b + c] = code == prm::NO_INPUT ? 0u : t[prm::MAX_CAND + c];
      }
    }
    __syncthreads();
    const bool ok = s_code == prm::OK;
    const float *win = cand + 12 * (size_t)s_cbest;
    if (tid < 12) A.pose_out[12 * (size_t)b + tid] = ok ? win[tid] : 0.0f;

    // ---- pass 2: the winner's points ----
    {
      float C[12];
#pragma unroll
      for (int k = 0; k < 12; k++) C[k] = ok ? win[k] : 0.0f;
      float *xw = A.xw + 3 * row;
      uint8_t *point = A.point + row;
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += RC_THREADS) {
        float X[3] = {0.0f, 0.0f, 0.0f};
        bool is_point = false;
        if (ok && !(mask && !mask[i])) {
          const prm::Match m = rc_match(P, p1, p2, i);
          is_point = (prm::evaluate(C, P, m, A.p.cos_parallax, A.p.cos_point, X) & prm::POINT) != 0;
        }
        xw[3 * (size_t)i] = is_point ? X[0] : 0.0f;
        xw[3 * (size_t)i + 1] = is_point ? X[1] : 0.0f;
        xw[3 * (size_t)i + 2] = is_point ? X[2] : 0.0f;
        point[i] = is_point ? 1 : 0;
      }
    }
    __syncthreads();                           // the next pair rewrites what this one still reads
  }
}

}  // namespace pr
