// pislam_graph_kernels.h — batched essential-graph optimisation and map-point correction on the device
// (pislam_pose_graph_batch, pislam_map_points_correct_batch; include/pislam_hip.h), after
// ORB-SLAM's Optimizer::OptimizeEssentialGraph and the end of LoopClosing::CorrectLoop.  The header comments are the
// contract; the arithmetic is stated once, in pislam_graph_math.h, for these kernels and for the host probe.
//
// k_pose_graph: one workgroup runs the whole call for a graph in one launch (the checks, every evaluation, every solve
// with all its conjugate-gradient iterations), then the graph GRID_CAP further on; the launch shape and the tree are
// those of pislam_refine_kernels.h.
//   * The state does not fit in LDS at the limits (4096 vertices are 416 KiB a set): the two sets of similarities, the
//     edge errors, the terms J'u of every incidence entry, the factored blocks and the five vectors of the conjugate gradients live in the workgroup's slice of
//     the context's workspace, which a graph rereads from L2.  LDS holds the tree's partial sums, the maxima and flags.
//   * Every sum has one owner and one sequential chain: an edge belongs to a thread in the edge phases (any thread: an
//     edge phase only writes the edge's own words), a vertex to the thread of its partial q = k mod 256 in every vertex
//     phase, so a vertex's words never cross a thread between the barriers of a solve.
//   * Every thread follows the Levenberg rule and the stopping rules of the solve on the same words (the sums come out
//     of LDS), so nothing is broadcast and every barrier is met by the whole workgroup.
// k_map_points_correct: one thread per point, no LDS, walked over the batch in grid passes.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_graph_math.h"

namespace pgk {

struct PgArgs {
  const float *sims, *meas, *weight;           // weight or null
  const uint8_t *fixed;
  const uint32_t *v_counts, *e_counts, *edges, *inc_ptr, *inc;
  size_t v_stride, e_stride;
  int batch;
  pgr::Params p;
  float *sims_out;
  double *cost;
  uint32_t *status;
  char *ws;                                    // the workspace: pgr::ws_bytes(v_stride, e_stride) per workgroup
};

struct PgLds {
  double part[1][16], S[4], red[prf::THREADS];
  int flag[4];                                 // malformed, bad values or a failed step, some vertex fixed, some vertex free
};

// The sum over the owned free vertices of fn(k) through the tree (ends with a barrier).
template <class FN>
__device__ __forceinline__ double pg_vertex_sum(const pgr::Graph &G, PgLds &L, int tid, uint32_t q, const FN &fn) {
  double acc[1] = {0.0};
  PISLAM_ROLLED
  for (uint32_t k = q; k < G.nv; k += prf::THREADS)
    if (!G.fixed[k]) acc[0] += fn(k);
  prf::tree_sums(acc, tid, L.part, L.S);
  return L.S[0];
}

// F at set `set`'s state; *adm: every edge is admissible.  Ends with a barrier; flag[1] is left raised when not.
__device__ __forceinline__ double pg_eval(const pgr::Graph &G, PgLds &L, int set, int tid, uint32_t q, bool *adm) {
  double acc[1] = {0.0};
  bool ok = true;
  PISLAM_ROLLED
  for (uint32_t e = q; e < G.ne; e += prf::THREADS) {
    double f;
    ok = pgr::edge_eval(G, set, e, &f) && ok;
    acc[0] += f;
  }
  if (!ok) L.flag[1] = 1;                      // (every writer writes the same value)
  prf::tree_sums(acc, tid, L.part, L.S);
  *adm = L.flag[1] == 0;
  return L.S[0];
}

// One solve at lambda from set `set`: the trial state goes to the other set, *dmax is the largest |increment word|.
// False (the same for every thread): no step at this lambda.  flag[1] is 0 on entry and on return; ends with a barrier.
__device__ __forceinline__ bool pg_solve(const pgr::Graph &G, const pgr::Params &P, PgLds &L, int set, int tid, uint32_t q,
                                         double lambda, double *dmax) {
  const double s = 1.0 + lambda;
  double rz = pg_vertex_sum(G, L, tid, q, [&](uint32_t k) {
    double d;
    if (!pgr::vertex_setup(G, set, k, s, &d)) L.flag[1] = 1;
    return d;
  });
  bool ok = L.flag[1] == 0;                    // (raised before the barriers of the tree)
  __syncthreads();                             // the retractions raise it again: not before every thread has read it
  const double thr = (P.cg_tol * P.cg_tol) * rz;
  PISLAM_ROLLED
  for (int n = 0; ok && n < P.cg_iters; n++) {
    if (rz <= thr) break;
    PISLAM_ROLLED
    for (uint32_t e = tid; e < G.ne; e += prf::THREADS) pgr::edge_v(G, set, e);
    __syncthreads();
    const double pAp = pg_vertex_sum(G, L, tid, q, [&](uint32_t k) { return pgr::vertex_ap(G, k, lambda); });
    if (!(pAp > 0.0)) {
      ok = false;
      break;
    }
    const double alpha = rz / pAp;
    const double rz1 = pg_vertex_sum(G, L, tid, q, [&](uint32_t k) { return pgr::vertex_update(G, k, alpha); });
    const double beta = rz1 / rz;
    PISLAM_ROLLED
    for (uint32_t k = q; k < G.nv; k += prf::THREADS)
      if (!G.fixed[k]) pgr::vertex_p(G, k, beta);
    rz = rz1;
    __syncthreads();                           // the next edge phase reads every p
  }
  double dm = 0.0;
  if (ok) {
    PISLAM_ROLLED
    for (uint32_t k = q; k < G.nv; k += prf::THREADS) {
      if (G.fixed[k]) continue;
      double m;
      if (!pgr::vertex_retract(G, set, k, &m)) L.flag[1] = 1;
      dm = fmax(dm, m);
    }
  }
  L.red[tid] = dm;
  __syncthreads();
  PISLAM_ROLLED
  for (int h = prf::THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) L.red[tid] = fmax(L.red[tid], L.red[tid + h]);
    __syncthreads();
  }
  ok = ok && L.flag[1] == 0;
  *dmax = L.red[0];
  __syncthreads();                             // the flag and the maxima are rewritten from here on
  if (tid == 0) L.flag[1] = 0;
  __syncthreads();
  return ok;
}

__global__ __launch_bounds__(prf::THREADS) void k_pose_graph(const PgArgs A) {
  __shared__ PgLds L;
  pgr::Ws ws;
  pgr::ws_carve(A.ws + (size_t)blockIdx.x * pgr::ws_carve(nullptr, A.v_stride, A.e_stride, &ws), A.v_stride, A.e_stride, &ws);

  PISLAM_ROLLED
  for (uint32_t b = blockIdx.x; b < (uint32_t)A.batch; b += gridDim.x) {
    const int tid = threadIdx.x;
    const uint32_t q = prf::partial_of(tid);
    const size_t vrow = (size_t)b * A.v_stride, erow = (size_t)b * A.e_stride;
    pgr::Graph G;
    G.sims = A.sims + pgr::STATE * vrow, G.meas = A.meas + pgr::STATE * erow;
    G.weight = A.weight ? A.weight + erow : nullptr, G.fixed = A.fixed + vrow;
    G.edges = A.edges + 2 * erow, G.inc_ptr = A.inc_ptr + (size_t)b * (A.v_stride + 1), G.inc = A.inc + 2 * erow;
    G.nv = psm::clamp_count(A.v_counts[b], A.v_stride), G.ne = psm::clamp_count(A.e_counts[b], A.e_stride);
    G.ws = ws;
    const uint32_t nv = G.nv, ne = G.ne;
    float *out = A.sims_out + pgr::STATE * vrow;

    if (tid < 4) L.flag[tid] = 0;
    __syncthreads();
    bool bad = false;
    PISLAM_ROLLED
    for (uint32_t e = tid; e < ne; e += prf::THREADS) bad = bad || !pgr::edge_in_order(G, e);
    PISLAM_ROLLED
    for (uint32_t k = tid; k < nv; k += prf::THREADS) L.flag[G.fixed[k] ? 2 : 3] = 1;
    if (bad) L.flag[0] = 1;                                  // (every writer writes the same value)
    __syncthreads();
    // (the entries of the index are looked up in `edges`: only once every edge is known to name two vertices)
    bad = L.flag[0] != 0;
    __syncthreads();
    if (!bad) {
      PISLAM_ROLLED
      for (uint32_t k = tid; k < nv; k += prf::THREADS) bad = bad || !pgr::vertex_in_order(G, k);
      if (bad) L.flag[0] = 1;
    }
    __syncthreads();
    uint32_t code = L.flag[0] || !L.flag[2] ? 3u : 0u;
    const bool any_free = L.flag[3] != 0;
    double F = 0.0;
    if (!code) {
      bool inf = false;
      PISLAM_ROLLED
      for (uint32_t k = tid; k < nv; k += prf::THREADS) {
        inf = inf || !pgr::sim_words_ok(G.sims + pgr::STATE * (size_t)k);
        pgr::vertex_load(G, k);
      }
      PISLAM_ROLLED
      for (uint32_t e = tid; e < ne; e += prf::THREADS) inf = inf || !pgr::edge_words_ok(G, e);
      if (inf) L.flag[1] = 1;
      __syncthreads();
      bool adm;
      F = pg_eval(G, L, 0, tid, q, &adm);
      code = !adm ? 2u : ((ne == 0 || !any_free) ? 1u : 0u);
      __syncthreads();
      if (tid == 0) L.flag[1] = 0;
      __syncthreads();
    }
    if (code) {                                              // the refused graph: the inputs copied
      PISLAM_ROLLED
      for (uint32_t i = tid; i < pgr::STATE * nv; i += prf::THREADS) out[i] = G.sims[i];
      if (tid == 0) A.cost[b] = 0.0, A.status[b] = code;
    } else {
      int set = 0;
      uint32_t evals = 1;
      double lambda = prf::LAMBDA_0;
      PISLAM_ROLLED
      for (int it = 0; it < A.p.iters; it++) {
        double dmax;
        if (!pg_solve(G, A.p, L, set, tid, q, lambda, &dmax)) {
          lambda = prf::lambda_up(lambda);
          continue;
        }
        bool adm;
        const double Ft = pg_eval(G, L, set ^ 1, tid, q, &adm);
        evals++;
        __syncthreads();
        if (tid == 0) L.flag[1] = 0;
        __syncthreads();
        if (!adm) {
          lambda = prf::lambda_up(lambda);
          continue;
        }
        if (Ft < F) {
          F = Ft, set ^= 1;
          lambda = prf::lambda_down(lambda);
        } else {
          lambda = prf::lambda_up(lambda);
        }
        if (dmax <= A.p.eps) break;
      }
      PISLAM_ROLLED
      for (uint32_t i = tid; i < pgr::STATE * nv; i += prf::THREADS) out[i] = (float)ws.S[set][i];
      if (tid == 0) A.cost[b] = F, A.status[b] = evals << 8;
    }
    __syncthreads();                                         // the next graph rewrites what this one still reads
  }
}

// ---- map points moved with their reference key frames -----------------------------------------------------------------

constexpr int MC_THREADS = 256;
constexpr int MC_GRID_CAP = 1024;              // workgroups per launch; more points are walked in passes

struct McArgs {
  const float *xw, *sims_old, *sims_new;
  const uint16_t *ref;
  const uint32_t *pt_counts, *v_counts;
  size_t pt_stride, v_stride, total;           // total = batch * pt_stride
  float *xw_out;
  uint8_t *status;
};

__global__ __launch_bounds__(MC_THREADS) void k_map_points_correct(const McArgs A) {
  const size_t step = (size_t)gridDim.x * MC_THREADS;
  PISLAM_ROLLED
  for (size_t o = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; o < A.total; o += step) {
    const size_t b = o / A.pt_stride, i = o - b * A.pt_stride;
    if (i >= psm::clamp_count(A.pt_counts[b], A.pt_stride)) continue;
    const uint32_t nv = psm::clamp_count(A.v_counts[b], A.v_stride), k = A.ref[o];
    const float X[3] = {A.xw[3 * o], A.xw[3 * o + 1], A.xw[3 * o + 2]};
    float Y[3] = {X[0], X[1], X[2]};
    bool ok = k < nv;
    if (ok) {
      const size_t v = pgr::STATE * (b * A.v_stride + k);
      ok = pgr::correct_point(A.sims_old + v, A.sims_new + v, X, Y);
    }
    A.xw_out[3 * o] = Y[0], A.xw_out[3 * o + 1] = Y[1], A.xw_out[3 * o + 2] = Y[2];
    A.status[o] = ok ? 0 : 1;
  }
}

}  // namespace pgk
