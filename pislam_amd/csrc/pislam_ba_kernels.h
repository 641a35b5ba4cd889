// pislam_ba_kernels.h — batched local bundle adjustment on the device (pislam_local_ba_batch; include/pislam_hip.h,
// DESIGN.md section 5.5).  The header comment is the contract; the arithmetic is stated once, in pislam_ba_math.h, for
// this kernel and for the host probe.
//
// One workgroup runs the whole call for a window in one launch (all rounds, passes, solves and classifications), then
// the window GRID_CAP further on; the launch shape and the tree are those of pislam_refine_kernels.h.
//   * The reduced camera system (at most 96 x 96 and its right-hand side, binary64) and the free poses live in LDS; what
//     grows with the points and the observations (the point state, the two sets of terms a pass leaves, V'^-1's
//     factors, the rows of W V'^-1, the index) lives in the workgroup's slice of the context's workspace.
//   * Every sum has one owner and one sequential chain: a thread owns the points q, q + 256, ... (q = its partial of
//     the tree) in a pass, an entry of the reduced system in the Schur step, an entry of the trailing block in the
//     elimination (two barriers per pivot column) and a row in the back substitution (one barrier per unknown).
//   * Every thread follows the Levenberg rule on the same words (the sums come out of LDS), so nothing is broadcast.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_ba_math.h"

namespace pbk {

struct BaArgs {
  const float *poses, *cams, *xw;
  const uint32_t *kf_counts, *kf_free, *pt_counts, *counts;
  const int32_t *obs;
  const uint8_t *obs_kf;
  const uint16_t *obs_pt;
  const uint8_t *level;                        // or null
  size_t kf_stride, pt_stride, stride;
  int batch, nlevels;
  float inv_sigma2[pq::MAX_LEVELS];
  pba::Params p;
  float *poses_out, *xw_out;
  uint8_t *inlier;
  uint32_t *ninliers, *status;
  double *cost;
  char *ws;                                    // the workspace: ws_bytes(pt_stride, stride) per workgroup
};

// A workgroup's slice of the workspace.
struct BaWs {
  double *X[2], *V[2], *fac, *Y;               // the point state and sums of set 0 / 1; the factors; the rows of W V'^-1
  float *cam[2], *cross[2];
  uint32_t *pstart;
  uint16_t *slot, *klist;
  uint8_t *on[2], *held;
};

__host__ __device__ inline size_t ws_carve(char *base, size_t P, size_t N, BaWs *w) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = (char *)((uintptr_t)base + o);
    o += (bytes + 15) & ~(size_t)15;
    return p;
  };
  for (int s = 0; s < 2; s++) w->X[s] = (double *)take(8 * 3 * P), w->V[s] = (double *)take(8 * pba::PT * P);
  w->fac = (double *)take(8 * 9 * P), w->Y = (double *)take(8 * pba::CROSS * N);
  for (int s = 0; s < 2; s++) w->cam[s] = (float *)take(4 * pba::CAM * N), w->cross[s] = (float *)take(4 * pba::CROSS * N);
  w->pstart = (uint32_t *)take(4 * (P + 1));
  w->slot = (uint16_t *)take(2 * pba::MAX_FREE * P), w->klist = (uint16_t *)take(2 * N);
  for (int s = 0; s < 2; s++) w->on[s] = (uint8_t *)take(N);
  w->held = (uint8_t *)take(P);
  return (o + 255) & ~(size_t)255;
}
inline size_t ws_bytes(size_t P, size_t N) {
  BaWs w;
  return ws_carve(nullptr, P, N, &w);
}

struct BaLds {
  double A[pba::MAX_N * pba::LDA];             // the reduced system, its right-hand side at column MAX_N
  double T[2][pba::MAX_FREE * 12];             // the free poses of set 0 / 1
  double d[pba::MAX_N], f[pba::MAX_N], red[prf::THREADS], part[3][16], S[4];
  float Tf[pba::MAX_KF * 12], cam[pba::MAX_KF * 5];   // the poses of the pass (fixed ones as given), the cameras
  uint32_t kstart[pba::MAX_FREE + 1];
  int flag[2];
};

// One pass at set `set`'s state into that set: leaves (F, the contributing observations, their chi2) in L.S (ends with a
// barrier).
__device__ __forceinline__ void ba_pass(const pba::Window &W, const BaWs &ws, BaLds &L, int set, int tid, uint32_t q,
                                        uint8_t *active, bool classify, bool robust) {
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 12 * W.nfree; i += prf::THREADS) L.Tf[i] = (float)L.T[set][i];
  __syncthreads();
  double acc[3] = {0.0, 0.0, 0.0};
  PISLAM_ROLLED
  for (uint32_t p = q; p < W.npt; p += prf::THREADS) {
    const double *Xs = ws.X[set] + 3 * (size_t)p;
    const float Xf[3] = {(float)Xs[0], (float)Xs[1], (float)Xs[2]};
    double v[pba::PT], s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < pba::PT; j++) v[j] = 0.0;
    PISLAM_ROLLED
    for (uint32_t i = ws.pstart[p]; i < ws.pstart[p + 1]; i++) {
      const uint32_t k = W.kf[i];
      pba::ObsTerms t;
      const bool c = pba::pass_one(W, i, &L.Tf[12 * k], &L.cam[5 * k], Xf, classify, robust, &active[i], t);
      ws.on[set][i] = c;
      if (!c) continue;
#pragma unroll
      for (int j = 0; j < pba::PT; j++) v[j] = v[j] + (double)t.pt[j];
      s[0] = s[0] + (double)t.cam[27], s[1] = s[1] + 1.0, s[2] = s[2] + (double)t.chi2;
      if (k < W.nfree) {
        float *c_ = ws.cam[set] + pba::CAM * (size_t)i, *x_ = ws.cross[set] + pba::CROSS * (size_t)i;
#pragma unroll
        for (int j = 0; j < pba::CAM; j++) c_[j] = t.cam[j];
#pragma unroll
        for (int j = 0; j < pba::CROSS; j++) x_[j] = t.cross[j];
      }
    }
#pragma unroll
    for (int j = 0; j < pba::PT; j++) ws.V[set][pba::PT * (size_t)p + j] = v[j];
#pragma unroll
    for (int j = 0; j < 3; j++) acc[j] += s[j];
  }
  prf::tree_sums(acc, tid, L.part, L.S);
}

// One solve at lambda from set `set`: the trial state goes to the other set, *dmax is the largest |increment word|.
// False (the same for every thread): no step at this lambda.  Ends with a barrier.
__device__ __forceinline__ bool ba_step(const pba::Window &W, const BaWs &ws, BaLds &L, int set, int tid, double lambda,
                                        double *dmax) {
  const uint32_t nfree = W.nfree, npt = W.npt, N = 6 * nfree;
  const double s = 1.0 + lambda;
  const pba::Store S{ws.cam[set], ws.cross[set], ws.on[set], ws.V[set], ws.fac, ws.held, ws.Y,
                     ws.slot, ws.klist, L.kstart, W.pt};
  if (tid == 0) L.flag[1] = 0;
  PISLAM_ROLLED
  for (uint32_t p = tid; p < npt; p += prf::THREADS) {
    ws.held[p] = !pba::factor3(ws.V[set] + pba::PT * (size_t)p, s, ws.fac + 9 * (size_t)p);
    pba::point_rows(S, W.kf, nfree, p, ws.pstart[p], ws.pstart[p + 1], ws.Y);
  }
  __syncthreads();
  // the reduced system: an owner per entry of the upper block triangle and per right-hand side
  const uint32_t nent = 36 * (nfree * (nfree + 1) / 2);
  PISLAM_ROLLED
  for (uint32_t w = tid; w < nent + N; w += prf::THREADS) {
    if (w < nent) {
      uint32_t ki = 0, rem = w / 36;
      while (rem >= nfree - ki) rem -= nfree - ki, ki++;
      const uint32_t kj = ki + rem, ai = (w % 36) / 6, aj = w % 6;
      if (ki == kj && ai > aj) continue;
      const double v = pba::reduced_entry(S, (int)ki, (int)ai, (int)kj, (int)aj, s);
      const uint32_t i = 6 * ki + ai, j = 6 * kj + aj;
      L.A[pba::LDA * i + j] = v, L.A[pba::LDA * j + i] = v;
    } else {
      const uint32_t r = w - nent;
      L.A[pba::LDA * r + pba::MAX_N] = pba::reduced_rhs(S, (int)(r / 6), (int)(r % 6));
    }
  }
  __syncthreads();
  // the elimination: every entry update of a pivot column is independent of the others
  bool ok = true;
  PISLAM_ROLLED
  for (uint32_t c = 0; c < N; c++) {
    const double piv = L.A[pba::LDA * c + c];
    if (!(piv > 0.0)) {
      ok = false;
      break;
    }
    for (uint32_t r = c + 1 + tid; r < N; r += prf::THREADS) L.f[r] = L.A[pba::LDA * r + c] / piv;
    __syncthreads();
    const uint32_t m = N - c - 1;
    PISLAM_ROLLED
    for (uint32_t e = tid; e < m * (m + 1); e += prf::THREADS) {
      const uint32_t r = c + 1 + e / (m + 1), jj = e % (m + 1);
      const uint32_t j = jj < m ? c + 1 + jj : (uint32_t)pba::MAX_N;
      L.A[pba::LDA * r + j] = L.A[pba::LDA * r + j] - L.f[r] * L.A[pba::LDA * c + j];
    }
    __syncthreads();
  }
  if (!ok) return false;                       // (every thread read the same pivot after the same barrier)
  // the back substitution: row r's owner takes d_r out of the rows above as soon as it is known
  double t = (uint32_t)tid < N ? L.A[pba::LDA * tid + pba::MAX_N] : 0.0;
  PISLAM_ROLLED
  for (uint32_t r = N; r-- > 0;) {
    if ((uint32_t)tid == r) L.d[r] = t / L.A[pba::LDA * r + r];
    __syncthreads();
    if ((uint32_t)tid < r) t = t - L.A[pba::LDA * tid + r] * L.d[r];
  }
  double dm = 0.0;
  if ((uint32_t)tid < N) {
    if (!pba::finite_d(L.d[tid])) L.flag[1] = 1;
    dm = fabs(L.d[tid]);
  }
  PISLAM_ROLLED
  for (uint32_t p = tid; p < npt; p += prf::THREADS) {
    double dp[3];
    if (!pba::point_step(S, W.kf, nfree, p, ws.pstart[p], ws.pstart[p + 1], L.d, dp)) L.flag[1] = 1;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      ws.X[set ^ 1][3 * (size_t)p + j] = ws.X[set][3 * (size_t)p + j] + dp[j];
      dm = fmax(dm, fabs(dp[j]));
    }
  }
  if ((uint32_t)tid < nfree) pq::retract(&L.T[set][12 * tid], &L.d[6 * tid], &L.T[set ^ 1][12 * tid]);
  L.red[tid] = dm;
  __syncthreads();
  PISLAM_ROLLED
  for (int h = prf::THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) L.red[tid] = fmax(L.red[tid], L.red[tid + h]);
    __syncthreads();
  }
  const bool bad = L.flag[1] != 0;
  *dmax = L.red[0];
  __syncthreads();                             // the next step rewrites the flag and the maxima
  return !bad;
}

// The index of the window: a point's first observation, the observation of (point, free key frame), a free key frame's
// observations in ascending order.
__device__ __forceinline__ void ba_index(const pba::Window &W, const BaWs &ws, BaLds &L, int tid) {
  const uint32_t n = W.n, npt = W.npt, nfree = W.nfree;
  PISLAM_ROLLED
  for (uint32_t p = tid; p <= npt; p += prf::THREADS) ws.pstart[p] = p < npt ? pba::first_obs(W.pt, n, p) : n;
  PISLAM_ROLLED
  for (uint32_t e = tid; e < pba::MAX_FREE * npt; e += prf::THREADS) ws.slot[e] = pba::NO_OBS;
  __syncthreads();
  PISLAM_ROLLED
  for (uint32_t i = tid; i < n; i += prf::THREADS)
    if (W.kf[i] < nfree) ws.slot[pba::MAX_FREE * (size_t)W.pt[i] + W.kf[i]] = (uint16_t)i;
  __syncthreads();
  const uint32_t lane = (uint32_t)tid & 63u, wave = (uint32_t)tid >> 6;
  PISLAM_ROLLED
  for (uint32_t k = wave; k < nfree; k += prf::THREADS / 64) {   // (counts first: kstart[k + 1] holds key frame k's)
    uint32_t cnt = 0;
    PISLAM_ROLLED
    for (uint32_t base = 0; base < npt; base += 64) {
      const uint32_t p = base + lane;
      cnt += (uint32_t)__popcll(__ballot(p < npt && ws.slot[pba::MAX_FREE * (size_t)p + k] != pba::NO_OBS));
    }
    if (lane == 0) L.kstart[k + 1] = cnt;
  }
  if (tid == 0) L.kstart[0] = 0;
  __syncthreads();
  if (tid == 0) {
    PISLAM_ROLLED
    for (uint32_t k = 0; k < nfree; k++) L.kstart[k + 1] += L.kstart[k];
  }
  __syncthreads();
  PISLAM_ROLLED
  for (uint32_t k = wave; k < nfree; k += prf::THREADS / 64) {
    uint32_t off = L.kstart[k];
    PISLAM_ROLLED
    for (uint32_t base = 0; base < npt; base += 64) {
      const uint32_t p = base + lane;
      const uint16_t o = p < npt ? ws.slot[pba::MAX_FREE * (size_t)p + k] : pba::NO_OBS;
      const uint64_t m = __ballot(o != pba::NO_OBS);
      if (o != pba::NO_OBS) ws.klist[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = o;
      off += (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
}

// The window that runs: the call's rounds.  out: poses_out, xw_out of the window.
__device__ __forceinline__ void ba_window(const BaArgs &A, const pba::Window &W, const BaWs &ws, BaLds &L, uint32_t b, int tid,
                                          uint32_t q, float *pout, float *xout, uint8_t *inl) {
  const uint32_t n = W.n, nkf = W.nkf, npt = W.npt, nfree = W.nfree;
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 12 * nkf; i += prf::THREADS) L.Tf[i] = W.poses[i];
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 5 * nkf; i += prf::THREADS) L.cam[i] = W.cams[i];
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 12 * nfree; i += prf::THREADS) L.T[0][i] = (double)W.poses[i];
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 3 * npt; i += prf::THREADS) ws.X[0][i] = (double)W.xw[i];
  PISLAM_ROLLED
  for (uint32_t i = tid; i < n; i += prf::THREADS) inl[i] = 1;   // the mask is the active set
  ba_index(W, ws, L, tid);

  const int rounds = A.p.rounds, hr = A.p.huber_rounds;
  int set = 0;
  uint32_t evals = 1, code = 0, ninl = 0;
  double cost = 0.0;
  ba_pass(W, ws, L, set, tid, q, inl, false, 0 < hr);
  double F = L.S[0];
  PISLAM_ROLLED
  for (int rd = 0; rd < rounds; rd++) {
    double lambda = prf::LAMBDA_0;
    const int iters = A.p.iters[rd];
    PISLAM_ROLLED
    for (int it = 0; it < iters; it++) {
      double dmax;
      if (!ba_step(W, ws, L, set, tid, lambda, &dmax)) {
        lambda = prf::lambda_up(lambda);
        continue;
      }
      ba_pass(W, ws, L, set ^ 1, tid, q, inl, false, rd < hr);
      evals++;
      const double Ft = L.S[0];
      if (Ft < F) {
        F = Ft, set ^= 1;
        lambda = prf::lambda_down(lambda);
      } else {
        lambda = prf::lambda_up(lambda);
      }
      if (dmax <= A.p.eps) break;
    }
    ba_pass(W, ws, L, set, tid, q, inl, true, rd + 1 < hr);
    evals++;
    F = L.S[0], ninl = (uint32_t)L.S[1], cost = L.S[2];
    if (rd + 1 < rounds && ninl < (uint32_t)A.p.min_obs) {
      code = 1;
      break;
    }
  }
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 12 * nkf; i += prf::THREADS) pout[i] = i < 12 * nfree ? (float)L.T[set][i] : L.Tf[i];
  PISLAM_ROLLED
  for (uint32_t i = tid; i < 3 * npt; i += prf::THREADS) xout[i] = (float)ws.X[set][i];
  if (tid == 0) A.ninliers[b] = ninl, A.cost[b] = cost, A.status[b] = code | evals << 8;
}

__global__ __launch_bounds__(prf::THREADS) void k_local_ba(const BaArgs A) {
  __shared__ BaLds L;
  BaWs ws;
  ws_carve(A.ws + (size_t)blockIdx.x * ws_carve(nullptr, A.pt_stride, A.stride, &ws), A.pt_stride, A.stride, &ws);

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {
    const int tid = threadIdx.x;
    const uint32_t q = prf::partial_of(tid);
    const size_t krow = (size_t)b * A.kf_stride, prow = (size_t)b * A.pt_stride, row = (size_t)b * A.stride;
    pba::Window W;
    W.poses = A.poses + 12 * krow, W.cams = A.cams + 5 * krow, W.xw = A.xw + 3 * prow, W.obs = A.obs + 3 * row;
    W.kf = A.obs_kf + row, W.pt = A.obs_pt + row, W.level = A.level ? A.level + row : nullptr;
    W.inv_sigma2 = A.inv_sigma2, W.nlevels = A.nlevels;
    W.nkf = psm::clamp_count(A.kf_counts[b], A.kf_stride), W.npt = psm::clamp_count(A.pt_counts[b], A.pt_stride);
    W.n = psm::clamp_count(A.counts[b], A.stride), W.nfree = A.kf_free[b];
    float *pout = A.poses_out + 12 * krow, *xout = A.xw_out + 3 * prow;
    uint8_t *inl = A.inlier + row;
    const uint32_t n = W.n, nkf = W.nkf, npt = W.npt;

    if (tid == 0) L.flag[0] = 0, L.flag[1] = 0;
    __syncthreads();
    bool bad = W.nfree > (uint32_t)pba::MAX_FREE || W.nfree > nkf, inf = false;
    PISLAM_ROLLED
    for (uint32_t i = tid; i < n; i += prf::THREADS) bad = bad || !pba::obs_in_order(W, i);
    PISLAM_ROLLED
    for (uint32_t i = tid; i < 12 * nkf; i += prf::THREADS) inf = inf || !pba::finite_f(W.poses[i]);
    PISLAM_ROLLED
    for (uint32_t i = tid; i < 5 * nkf; i += prf::THREADS) inf = inf || !pba::finite_f(W.cams[i]);
    PISLAM_ROLLED
    for (uint32_t i = tid; i < 3 * npt; i += prf::THREADS) inf = inf || !pba::finite_f(W.xw[i]);
    if (bad) L.flag[0] = 1;                                  // (every writer writes the same value)
    if (inf) L.flag[1] = 1;
    __syncthreads();
    const uint32_t code = L.flag[0] ? 3u : (L.flag[1] ? 2u : (n < (uint32_t)A.p.min_obs ? 1u : 0u));
    __syncthreads();                                         // (ba_step rewrites flag[1])
    if (code) {                                              // the refused window: the inputs copied, the mask cleared
      PISLAM_ROLLED
      for (uint32_t i = tid; i < 12 * nkf; i += prf::THREADS) pout[i] = W.poses[i];
      PISLAM_ROLLED
      for (uint32_t i = tid; i < 3 * npt; i += prf::THREADS) xout[i] = W.xw[i];
      PISLAM_ROLLED
      for (uint32_t i = tid; i < n; i += prf::THREADS) inl[i] = 0;
      if (tid == 0) A.ninliers[b] = 0, A.cost[b] = 0.0, A.status[b] = code;
    } else {
      ba_window(A, W, ws, L, b, tid, q, pout, xout, inl);
    }
    __syncthreads();                                         // the next window rewrites what this one still reads
  }
}

}  // namespace pbk
