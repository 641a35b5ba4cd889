// pislam_gba_kernels.h — global bundle adjustment of whole maps on the device (pislam_global_ba_batch; include/
// pislam_hip.h).  The header comment is the contract; the arithmetic is stated once, in
// pislam_gba_math.h, for these kernels and for the host probe.
//
// Every phase of a call is ONE LAUNCH over all maps of the batch and all of their points, observations or key frames;
// the order of the launches on the context stream is the only synchronisation between workgroups: no cooperative launch,
// no grid-wide wait, no polling.  The host issues a fixed sequence from the parameters alone and reads nothing back; a
// map's control block (gba::Ctl, at the head of the workspace) tells every launch whether the map still has work for
// it, and a workgroup whose map is finished, converged or refused returns at once.
//   * a thread per point:      the pass (walks the point's observations), the point factors, t_p and q_p of a PCG
//                              iteration, the point step
//   * a wave per key frame:    the index check, the set-up sums and (S p)_k: lane q owns partial q of the 64, the partials
//                              are combined by halving with six lane exchanges, lane 0 finishes the key frame
//   * a workgroup per map:     the sums over points (256 partials, prf::tree_sums) and over key frames, the PCG scalars
//                              and the x, r, z, p updates of at most 4096 key frames, the Levenberg rule (thread 0)
// A launch walks (map, group of 256 items) pairs grid-stride, so the grid follows the strides of the maps, not the batch.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_gba_math.h"

namespace gbk {

constexpr int THREADS = prf::THREADS, WAVES = THREADS / 64;
constexpr size_t GRID_CAP = 1u << 16;          // workgroups per launch; more (map, group) pairs are walked in passes

struct GbaArgs {
  const float *poses, *cams, *xw;
  const int32_t *obs, *obs_pt, *counts, *kf_counts;
  const uint32_t *pt_counts, *kf_ptr, *kf_obs;
  const uint16_t *obs_kf;
  const uint8_t *level, *fixed;                // level: or null
  size_t kf_stride, pt_stride, stride, batch, ws_map;
  int nlevels;
  float inv_sigma2[pq::MAX_LEVELS];
  gba::Params p;
  float *poses_out, *xw_out;
  uint8_t *inlier;
  uint32_t *ninliers, *status, *work;          // work: or null
  double *cost;
  char *ws;                                    // batch control blocks of gba::CTL_BYTES, then a slice of ws_map per map
};

__device__ __forceinline__ void make_map(const GbaArgs &A, size_t b, gba::Map &M) {
  const size_t krow = b * A.kf_stride, prow = b * A.pt_stride, row = b * A.stride;
  M.poses = A.poses + 12 * krow, M.cams = A.cams + 5 * krow, M.xw = A.xw + 3 * prow;
  M.obs = A.obs + 3 * row, M.pt = A.obs_pt + row, M.kf = A.obs_kf + row;
  M.level = A.level ? A.level + row : nullptr, M.fixed = A.fixed + krow;
  M.kf_ptr = A.kf_ptr + b * (A.kf_stride + 1), M.kf_obs = A.kf_obs + row;
  M.W.poses = nullptr, M.W.cams = nullptr, M.W.xw = nullptr, M.W.kf = nullptr, M.W.pt = nullptr;
  M.W.obs = M.obs, M.W.level = M.level, M.W.inv_sigma2 = A.inv_sigma2, M.W.nlevels = A.nlevels;
  M.W.nkf = 0, M.W.nfree = 0, M.W.npt = 0, M.W.n = 0;
  gba::map_counts(M, A.counts[b], A.kf_counts[b], A.pt_counts[b], A.stride, A.kf_stride, A.pt_stride);
  gba::ws_carve(A.ws + A.batch * gba::CTL_BYTES + b * A.ws_map, A.kf_stride, A.pt_stride, A.stride, &M.ws);
  M.ctl = (gba::Ctl *)(A.ws + b * gba::CTL_BYTES);
}

// The map with set `set` of its state in place 0 and the other set in place 1: the phases then index the sets with
// constants, and the map stays in registers.
template <class T>
__device__ __forceinline__ void orient2(T *(&a)[2], bool swap) {
  T *const x = swap ? a[1] : a[0], *const y = swap ? a[0] : a[1];
  a[0] = x, a[1] = y;
}
__device__ __forceinline__ void orient(gba::Map &M, uint32_t set) {
  const bool swap = set != 0u;
  orient2(M.ws.T, swap), orient2(M.ws.Tf, swap), orient2(M.ws.X, swap), orient2(M.ws.V, swap);
  orient2(M.ws.cam, swap), orient2(M.ws.cross, swap), orient2(M.ws.on, swap);
}

// The (map, group) pairs of this workgroup: fn(M, b, first item of the group); `per_map` items in groups of `group`.
template <class FN>
__device__ __forceinline__ void for_groups(const GbaArgs &A, size_t per_map, size_t group, const FN &fn) {
  const size_t gpm = (per_map + group - 1) / group, total = A.batch * gpm;
  PISLAM_ROLLED
  for (size_t g = blockIdx.x; g < total; g += gridDim.x) {
    gba::Map M;
    make_map(A, g / gpm, M);
    fn(M, g / gpm, (g % gpm) * group);
  }
}
inline size_t groups_of(const GbaArgs &A, size_t per_map, size_t group) {
  return std::min<size_t>(A.batch * ((per_map + group - 1) / group), GRID_CAP);
}

// The 64 partials of SUMS sums, one set per lane, combined by halving (32, 16, .. 1): lane 0 holds the sums.  Both
// partners of a step add, and addition is commutative, so lane q < h holds p[q] + p[q + h] after step h.
template <int SUMS>
__device__ __forceinline__ void wave_halve(double *acc) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
    for (int t = 0; t < SUMS; t++) acc[t] = acc[t] + __shfl_xor(acc[t], h, 64);
  }
}

// ---- the checks, the control block, the state ------------------------------------------------------------------------

// Item i < stride: observation i; item stride + p: point p.
__global__ __launch_bounds__(THREADS) void k_gba_check_items(const GbaArgs A) {
  for_groups(A, A.stride + A.pt_stride, THREADS, [&](gba::Map &M, size_t, size_t first) {
    if (!M.shaped) return;
    const size_t item = first + threadIdx.x;
    if (item < A.stride) {
      if (item < M.n && !gba::obs_in_order(M, (uint32_t)item)) M.ctl->bad3 = 1;
    } else if (item - A.stride < M.npt) {
      if (!gba::pt_words_ok(M, (uint32_t)(item - A.stride))) M.ctl->bad2 = 1;
    }
  });
}

// A wave per key frame: its range and entries of the index, its words, whether it is free.
__global__ __launch_bounds__(THREADS) void k_gba_check_kf(const GbaArgs A) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for_groups(A, A.kf_stride, WAVES, [&](gba::Map &M, size_t, size_t first) {
    const size_t k = first + wave;
    if (!M.shaped || k >= M.nk) return;
    if (!gba::kf_range_ok(M, (uint32_t)k)) {                 // (the same for every lane of the wave)
      M.ctl->bad3 = 1;
    } else {
      bool ok = true;
      const uint32_t e1 = M.kf_ptr[k + 1];
      PISLAM_ROLLED
      for (uint32_t j = M.kf_ptr[k] + lane; j < e1; j += 64) ok = ok && gba::kf_entry_ok(M, (uint32_t)k, j);
      if (!ok) M.ctl->bad3 = 1;
    }
    if (lane == 0) {
      if (!gba::kf_words_ok(M, (uint32_t)k)) M.ctl->bad2 = 1;
      if (!M.fixed[k]) M.ctl->any_free = 1;
    }
  });
}

__global__ __launch_bounds__(THREADS) void k_gba_begin(const GbaArgs A) {
  for_groups(A, 1, 1, [&](gba::Map &M, size_t, size_t) {
    if (threadIdx.x == 0) gba::ctl_begin(M, *M.ctl, A.p.ba.min_obs);
  });
}

// Items: the key frames, then the points 0 .. pt_stride (pstart has one word more), then the observations.
__global__ __launch_bounds__(THREADS) void k_gba_load(const GbaArgs A) {
  for_groups(A, A.kf_stride + A.pt_stride + 1 + A.stride, THREADS, [&](gba::Map &M, size_t b, size_t first) {
    if (M.ctl->done) return;
    size_t item = first + threadIdx.x;
    if (item < A.kf_stride) {
      if (item < M.nk) gba::load_kf(M, (uint32_t)item);
      return;
    }
    item -= A.kf_stride;
    if (item <= A.pt_stride) {
      if (item <= M.npt) gba::load_pt(M, (uint32_t)item);
      return;
    }
    item -= A.pt_stride + 1;
    if (item < M.n) A.inlier[b * A.stride + item] = 1;       // the mask is the active set
  });
}

// ---- a pass and what follows it ---------------------------------------------------------------------------------------

enum : int { FIRST = 0, TRIAL = 1, CLASSIFY = 2 };

__global__ __launch_bounds__(THREADS) void k_gba_pass(const GbaArgs A, int mode, int robust) {
  for_groups(A, A.pt_stride, THREADS, [&](gba::Map &M, size_t b, size_t first) {
    const gba::Ctl &C = *M.ctl;
    if (mode == TRIAL ? !gba::trial_live(C) : C.done != 0u) return;
    const size_t p = first + threadIdx.x;
    if (p >= M.npt) return;
    orient(M, C.set ^ (mode == TRIAL ? 1u : 0u));
    gba::pass_point(M, 0, (uint32_t)p, mode == CLASSIFY, robust != 0, A.inlier + b * A.stride);
  });
}

// A workgroup per map: the sums of the pass over the points, then the rule.  r: the round (CLASSIFY).
__global__ __launch_bounds__(THREADS) void k_gba_decide(const GbaArgs A, int mode, int r) {
  __shared__ double part[3][16], S[4];
  const int tid = threadIdx.x;
  const uint32_t q = prf::partial_of(tid);
  for_groups(A, 1, 1, [&](gba::Map &M, size_t, size_t) {
    gba::Ctl &C = *M.ctl;
    const bool live = mode == TRIAL ? gba::iter_live(C) : C.done == 0u;
    const bool summed = mode == TRIAL ? gba::trial_live(C) : live;
    __syncthreads();                                         // (thread 0 rewrites what the others have just read)
    if (!live) return;
    if (summed) {
      double acc[3] = {0.0, 0.0, 0.0};
      PISLAM_ROLLED
      for (uint32_t p = q; p < M.npt; p += prf::PARTIALS) {
#pragma unroll
        for (int j = 0; j < 3; j++) acc[j] += M.ws.sub[3 * (size_t)p + j];
      }
      prf::tree_sums(acc, tid, part, S);
    }
    if (tid == 0) {
      if (mode == FIRST) gba::ctl_first(C, S);
      else if (mode == TRIAL) gba::ctl_trial(C, S, A.p.ba.eps);
      else gba::ctl_classify(C, S, r, A.p.ba.rounds, A.p.ba.min_obs);
    }
    __syncthreads();                                         // (the next map of this workgroup rewrites S)
  });
}

// ---- a solve ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void k_gba_factor(const GbaArgs A) {
  for_groups(A, A.pt_stride, THREADS, [&](gba::Map &M, size_t, size_t first) {
    const gba::Ctl &C = *M.ctl;
    if (!gba::iter_live(C)) return;
    const size_t p = first + threadIdx.x;
    orient(M, C.set);
    if (p < M.npt) gba::point_factor(M, 0, (uint32_t)p, 1.0 + C.lambda);
  });
}

__global__ __launch_bounds__(THREADS) void k_gba_kf_setup(const GbaArgs A) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for_groups(A, A.kf_stride, WAVES, [&](gba::Map &M, size_t, size_t first) {
    gba::Ctl &C = *M.ctl;
    const size_t k = first + wave;
    if (!gba::iter_live(C) || k >= M.nk || M.fixed[k]) return;
    orient(M, C.set);
    double acc[gba::SETUP_SUMS];
    gba::kf_setup_partial(M, 0, (uint32_t)k, lane, acc);
    wave_halve<gba::SETUP_SUMS>(acc);
    if (lane == 0 && !gba::kf_setup_finish(M, (uint32_t)k, 1.0 + C.lambda, acc)) C.solve_fail = 1;
  });
}

// The sum over the free key frames of fn(k): 256 partials by k mod 256, then the tree; the same in every thread.
template <class FN>
__device__ __forceinline__ double kf_sum(const gba::Map &M, int tid, uint32_t q, double (*part)[16], double *S, const FN &fn) {
  double acc[1] = {0.0};
  PISLAM_ROLLED
  for (uint32_t k = q; k < M.nk; k += prf::PARTIALS)
    if (!M.fixed[k]) acc[0] += fn(k);
  prf::tree_sums(acc, tid, part, S);
  const double v = S[0];
  __syncthreads();                                           // (the next sum rewrites S)
  return v;
}

__global__ __launch_bounds__(THREADS) void k_gba_cg_begin(const GbaArgs A) {
  __shared__ double part[1][16], S[1];
  const int tid = threadIdx.x;
  const uint32_t q = prf::partial_of(tid);
  for_groups(A, 1, 1, [&](gba::Map &M, size_t, size_t) {
    gba::Ctl &C = *M.ctl;
    const bool live = gba::iter_live(C);
    __syncthreads();
    if (!live) return;
    const double rz = kf_sum(M, tid, q, part, S, [&](uint32_t k) { return M.ws.dot[k]; });
    if (tid == 0) gba::ctl_cg_begin(C, rz, A.p.cg_tol);
  });
}

__global__ __launch_bounds__(THREADS) void k_gba_cg_point(const GbaArgs A) {
  for_groups(A, A.pt_stride, THREADS, [&](gba::Map &M, size_t, size_t first) {
    const gba::Ctl &C = *M.ctl;
    if (!gba::cg_live(C)) return;
    const size_t p = first + threadIdx.x;
    orient(M, C.set);
    if (p < M.npt) gba::cg_point(M, 0, (uint32_t)p);
  });
}

__global__ __launch_bounds__(THREADS) void k_gba_cg_kf(const GbaArgs A) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for_groups(A, A.kf_stride, WAVES, [&](gba::Map &M, size_t, size_t first) {
    const gba::Ctl &C = *M.ctl;
    const size_t k = first + wave;
    if (!gba::cg_live(C) || k >= M.nk || M.fixed[k]) return;
    orient(M, C.set);
    double acc[gba::DIM];
    gba::kf_sp_partial(M, 0, (uint32_t)k, lane, acc);
    wave_halve<gba::DIM>(acc);
    if (lane == 0) gba::kf_sp_finish(M, (uint32_t)k, acc);
  });
}

// The scalars of an iteration and the vectors that hang on them: pAp, alpha, x, r, z, rz, beta, p.
__global__ __launch_bounds__(THREADS) void k_gba_cg_scalar(const GbaArgs A) {
  __shared__ double part[1][16], S[1], sc[2];
  const int tid = threadIdx.x;
  const uint32_t q = prf::partial_of(tid);
  for_groups(A, 1, 1, [&](gba::Map &M, size_t, size_t) {
    gba::Ctl &C = *M.ctl;
    const bool live = gba::cg_live(C);
    __syncthreads();
    if (!live) return;
    const double pAp = kf_sum(M, tid, q, part, S, [&](uint32_t k) { return gba::kf_pap(M, k); });
    if (tid == 0) {
      double alpha = 0.0;
      sc[1] = gba::ctl_cg_alpha(C, pAp, &alpha) ? 1.0 : 0.0;
      sc[0] = alpha;
    }
    __syncthreads();
    const double alpha = sc[0];
    const bool ok = sc[1] != 0.0;
    __syncthreads();
    if (!ok) return;
    const double rz1 = kf_sum(M, tid, q, part, S, [&](uint32_t k) { return gba::kf_update(M, k, alpha); });
    if (tid == 0) sc[0] = gba::ctl_cg_beta(C, rz1, A.p.cg_iters);
    __syncthreads();
    const double beta = sc[0];
    PISLAM_ROLLED
    for (uint32_t k = q; k < M.nk; k += prf::PARTIALS)
      if (!M.fixed[k]) gba::kf_p(M, k, beta);
    __syncthreads();
  });
}

// Item p < pt_stride: the step of point p; item pt_stride + k: the step of key frame k.
__global__ __launch_bounds__(THREADS) void k_gba_step(const GbaArgs A) {
  for_groups(A, A.pt_stride + A.kf_stride, THREADS, [&](gba::Map &M, size_t, size_t first) {
    gba::Ctl &C = *M.ctl;
    if (!gba::step_live(C)) return;                          // (the same for the whole workgroup)
    const size_t item = first + threadIdx.x;
    orient(M, C.set);
    const int set = 0;
    double dm = 0.0;
    bool ok = true;
    if (item < A.pt_stride) {
      if (item < M.npt) ok = gba::point_step(M, set, (uint32_t)item, &dm);
    } else {
      const size_t k = item - A.pt_stride;
      if (k < M.nk && !M.fixed[k]) ok = gba::kf_step(M, set, (uint32_t)k, &dm);
    }
    if (!ok) C.step_bad = 1, dm = 0.0;
    PISLAM_ROLLED
    for (int o = 32; o >= 1; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o, 64));
    // a maximum of non-negative finite doubles is the maximum of their bit patterns
    if ((threadIdx.x & 63) == 0 && dm > 0.0) atomicMax((unsigned long long *)&C.dmax, (unsigned long long)__double_as_longlong(dm));
  });
}

// ---- the outputs -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void k_gba_out(const GbaArgs A) {
  size_t per_map = 12 * A.kf_stride > 3 * A.pt_stride ? 12 * A.kf_stride : 3 * A.pt_stride;
  per_map = per_map > A.stride ? per_map : A.stride;
  for_groups(A, per_map, THREADS, [&](gba::Map &M, size_t b, size_t first) {
    const gba::Ctl &C = *M.ctl;
    const bool ran = C.evals != 0u;
    orient(M, C.set);
    const size_t i = first + threadIdx.x;
    if (i < 12 * (size_t)M.nk) {
      const size_t o = 12 * b * A.kf_stride + i;
      A.poses_out[o] = ran && !M.fixed[i / 12] ? (float)M.ws.T[0][i] : A.poses[o];
    }
    if (i < 3 * (size_t)M.npt) {
      const size_t o = 3 * b * A.pt_stride + i;
      A.xw_out[o] = ran ? (float)M.ws.X[0][i] : A.xw[o];
    }
    if (!ran && i < M.n) A.inlier[b * A.stride + i] = 0;
    if (i == 0) {
      A.ninliers[b] = C.ninl, A.cost[b] = C.cost, A.status[b] = C.code | C.evals << 8;
      if (A.work) A.work[2 * b] = C.solves, A.work[2 * b + 1] = C.cg_total;
    }
  });
}

}  // namespace gbk
