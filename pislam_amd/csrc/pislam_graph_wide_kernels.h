// pislam_graph_wide_kernels.h — essential-graph optimisation of large graphs across workgroups
// (pislam_pose_graph_wide_batch; include/pislam_hip.h).  The contract is the comment of
// pislam_pose_graph_batch; the arithmetic is stated once, in pislam_graph_math.h, for k_pose_graph, for these kernels
// and for the host probes.  The outputs are those of k_pose_graph bit for bit: every sum keeps its owner's order.
//
// Every phase of a call is ONE LAUNCH over all graphs of the batch and all of their edges or vertices; the order of the
// launches on the context stream is the only synchronisation between workgroups: no cooperative launch, no grid-wide
// wait, no polling.  The host issues a fixed sequence from the parameters alone and reads nothing back; a graph's
// control block (pgw::Ctl, at the head of the workspace) tells every launch whether the graph still has work for it,
// and a workgroup whose graph is refused, finished or past its solve's stopping rule returns at once.
//   * a thread per edge:       edge_in_order, edge_words_ok, edge_eval (the edge's term of F goes to f[e]), edge_v
//   * a thread per vertex:     vertex_in_order, vertex_load, vertex_setup, vertex_ap, vertex_update, vertex_p,
//                              vertex_retract; the term the vertex would have added goes to t[k] (a fixed vertex
//                              stores nothing)
//   * a workgroup per graph:   thread t adds the terms of partial prf::partial_of(t) in ascending index, then
//                              prf::tree_sums (pg_vertex_sum's and pg_eval's order); thread 0 applies the conjugate-
//                              gradient scalars, the stopping rules and the Levenberg rule to the control block
// A launch walks (graph, group of 256 items) pairs grid-stride, so the grid follows the strides, not the batch.  No
// launch reads a word of the control block that the same launch writes: the flags a phase raises are read by the next.
#pragma once
#include "pislam_refine_kernels.h"
#include "pislam_graph_math.h"

namespace pgw {

constexpr int THREADS = prf::THREADS;
constexpr size_t GRID_CAP = 1u << 16;          // workgroups per launch; more (graph, group) pairs are walked in passes
constexpr size_t MAX_V = 65536, MAX_E = 1u << 20;
constexpr size_t CTL_BYTES = 256;              // a control block's place at the head of the workspace

struct Ctl {
  uint32_t bad3, bad2, any_fixed, any_free;    // raised by the checks: malformed, a bad value or an inadmissible input
  uint32_t code, done, set, evals, solves, cg_total;
  uint32_t solve_fail, step_bad, inadm, cg_live;   // of the solve under way; cg_live: the next iteration runs
  double lambda, F, rz, thr, alpha, beta, dmax;
};
static_assert(sizeof(Ctl) <= CTL_BYTES, "the control block outgrew its place");

// The launches of a call: the checks, the load, the first evaluation and its rule; per Levenberg iteration the set-up,
// the start of the conjugate gradients, six launches an iteration, the retraction, the evaluation and the rule; the
// outputs.
inline long long launch_count(const pgr::Params &p) { return 5 + (long long)p.iters * (5 + 6 * (long long)p.cg_iters); }

// A graph's slice: pgr::ws_carve's arrays, then f[e_stride] (an edge's term of F) and t[v_stride] (a vertex's term).
inline size_t ws_graph_bytes(size_t V, size_t E) {
  return pgr::ws_bytes(V, E) + ((8 * ((E + 1) & ~(size_t)1) + 8 * V + 255) & ~(size_t)255);
}

struct WideArgs {
  const float *sims, *meas, *weight;           // weight or null
  const uint8_t *fixed;
  const uint32_t *v_counts, *e_counts, *edges, *inc_ptr, *inc;
  size_t v_stride, e_stride, batch, ws_graph;
  pgr::Params p;
  float *sims_out;
  double *cost;
  uint32_t *status, *work;                     // work: or null
  char *ws;                                    // batch control blocks of CTL_BYTES, then a slice of ws_graph per graph
};

struct Wide {
  pgr::Graph G;
  Ctl *ctl;
  double *f, *t;
};

__device__ __forceinline__ void make_graph(const WideArgs &A, size_t b, Wide &W) {
  const size_t vrow = b * A.v_stride, erow = b * A.e_stride;
  pgr::Graph &G = W.G;
  G.sims = A.sims + pgr::STATE * vrow, G.meas = A.meas + pgr::STATE * erow;
  G.weight = A.weight ? A.weight + erow : nullptr, G.fixed = A.fixed + vrow;
  G.edges = A.edges + 2 * erow, G.inc_ptr = A.inc_ptr + b * (A.v_stride + 1), G.inc = A.inc + 2 * erow;
  G.nv = psm::clamp_count(A.v_counts[b], A.v_stride), G.ne = psm::clamp_count(A.e_counts[b], A.e_stride);
  char *slice = A.ws + A.batch * CTL_BYTES + b * A.ws_graph;
  const size_t o = pgr::ws_carve(slice, A.v_stride, A.e_stride, &G.ws);
  W.f = (double *)(slice + o), W.t = W.f + ((A.e_stride + 1) & ~(size_t)1);
  W.ctl = (Ctl *)(A.ws + b * CTL_BYTES);
}

// The graph with set `set` of its state in place 0 and the other set in place 1: the phases then index the sets with
// constants, and the graph stays in registers.
__device__ __forceinline__ void orient(pgr::Graph &G, uint32_t set) {
  const bool swap = set != 0u;
  double *const s0 = swap ? G.ws.S[1] : G.ws.S[0], *const s1 = swap ? G.ws.S[0] : G.ws.S[1];
  double *const e0 = swap ? G.ws.E[1] : G.ws.E[0], *const e1 = swap ? G.ws.E[0] : G.ws.E[1];
  G.ws.S[0] = s0, G.ws.S[1] = s1, G.ws.E[0] = e0, G.ws.E[1] = e1;
}

// The (graph, group) pairs of this workgroup: fn(W, b, first item of the group); `per_graph` items in groups of `group`.
template <class FN>
__device__ __forceinline__ void for_groups(const WideArgs &A, size_t per_graph, size_t group, const FN &fn) {
  const size_t gpg = (per_graph + group - 1) / group, total = A.batch * gpg;
  PISLAM_ROLLED
  for (size_t g = blockIdx.x; g < total; g += gridDim.x) {
    Wide W;
    make_graph(A, g / gpg, W);
    fn(W, g / gpg, (g % gpg) * group);
  }
}
inline size_t groups_of(const WideArgs &A, size_t per_graph, size_t group) {
  return std::min<size_t>(A.batch * ((per_graph + group - 1) / group), GRID_CAP);
}

// ---- what a launch asks of the control block ------------------------------------------------------------------------

__device__ __forceinline__ bool malformed(const Ctl &C) { return C.bad3 != 0u || C.any_fixed == 0u; }
__device__ __forceinline__ bool iter_live(const Ctl &C) { return !C.done; }
__device__ __forceinline__ bool step_live(const Ctl &C) { return !C.done && !C.solve_fail; }
__device__ __forceinline__ bool cg_live(const Ctl &C) { return step_live(C) && C.cg_live; }
__device__ __forceinline__ bool trial_live(const Ctl &C) { return step_live(C) && !C.step_bad; }

__device__ __forceinline__ void ctl_next_solve(Ctl &C) { C.solve_fail = 0, C.step_bad = 0, C.inadm = 0, C.cg_live = 0, C.dmax = 0.0; }

// The refusals in the contract's order, or the start of the round.
__device__ __forceinline__ void ctl_first(Ctl &C, uint32_t ne, double F) {
  C.code = malformed(C) ? 3u : (C.bad2 ? 2u : ((ne == 0u || !C.any_free) ? 1u : 0u));
  C.done = C.code != 0u;
  C.F = 0.0, C.evals = 0, C.set = 0, C.solves = 0, C.cg_total = 0, C.lambda = prf::LAMBDA_0;
  if (!C.done) C.F = F, C.evals = 1;
  ctl_next_solve(C);
}

// The Levenberg rule after an iteration: Ft is the trial state's F where trial_live.
__device__ __forceinline__ void ctl_trial(Ctl &C, double Ft, double eps) {
  if (trial_live(C)) {
    C.evals++;
    if (C.inadm) {
      C.lambda = prf::lambda_up(C.lambda);
    } else {
      if (Ft < C.F) C.F = Ft, C.set ^= 1u, C.lambda = prf::lambda_down(C.lambda);
      else C.lambda = prf::lambda_up(C.lambda);
      if (C.dmax <= eps) C.done = 1;
    }
  } else {
    C.lambda = prf::lambda_up(C.lambda);
  }
  ctl_next_solve(C);
}

// ---- the checks, the state ------------------------------------------------------------------------------------------

// Item e < e_stride: edge e; item e_stride + k: vertex k.
__global__ __launch_bounds__(THREADS) void k_pgw_check(const WideArgs A) {
  for_groups(A, A.e_stride + A.v_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    const pgr::Graph &G = W.G;
    Ctl &C = *W.ctl;
    const size_t item = first + threadIdx.x;
    if (item < A.e_stride) {
      if (item < G.ne && !pgr::edge_in_order(G, (uint32_t)item)) C.bad3 = 1;
    } else if (item - A.e_stride < G.nv) {
      const uint32_t k = (uint32_t)(item - A.e_stride);
      if (!pgr::vertex_in_order(G, k)) C.bad3 = 1;
      if (G.fixed[k]) C.any_fixed = 1;
      else C.any_free = 1;
    }
  });
}

// Item k < v_stride: vertex k; item v_stride + e: edge e.
__global__ __launch_bounds__(THREADS) void k_pgw_load(const WideArgs A) {
  for_groups(A, A.v_stride + A.e_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    const pgr::Graph &G = W.G;
    Ctl &C = *W.ctl;
    if (malformed(C)) return;
    const size_t item = first + threadIdx.x;
    if (item < A.v_stride) {
      if (item >= G.nv) return;
      if (!pgr::sim_words_ok(G.sims + pgr::STATE * item)) C.bad2 = 1;
      pgr::vertex_load(G, (uint32_t)item);
    } else if (item - A.v_stride < G.ne) {
      if (!pgr::edge_words_ok(G, (uint32_t)(item - A.v_stride))) C.bad2 = 1;
    }
  });
}

// ---- an evaluation of F and the rule that follows it ------------------------------------------------------------------

enum : int { FIRST = 0, TRIAL = 1 };

__global__ __launch_bounds__(THREADS) void k_pgw_eval(const WideArgs A, int mode) {
  for_groups(A, A.e_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    Ctl &C = *W.ctl;
    if (mode == TRIAL ? !trial_live(C) : malformed(C)) return;
    const size_t e = first + threadIdx.x;
    if (e >= W.G.ne) return;
    orient(W.G, mode == TRIAL ? C.set ^ 1u : 0u);
    double f;
    const bool ok = pgr::edge_eval(W.G, 0, (uint32_t)e, &f);
    W.f[e] = f;
    if (!ok) (mode == TRIAL ? C.inadm : C.bad2) = 1;
  });
}

// The sum of n terms in the contract's order: partial q takes q, q + 256, ..; then the tree.  The same in every thread.
// skip: or null; a term whose skip byte is nonzero is not added.
__device__ __forceinline__ double ordered_sum(const double *term, const uint8_t *skip, uint32_t n, int tid, uint32_t q,
                                              double (*part)[16], double *S) {
  double acc[1] = {0.0};
  PISLAM_ROLLED
  for (uint32_t i = q; i < n; i += prf::PARTIALS)
    if (!skip || !skip[i]) acc[0] += term[i];
  prf::tree_sums(acc, tid, part, S);
  const double v = S[0];
  __syncthreads();                                           // (the next sum rewrites S)
  return v;
}

__global__ __launch_bounds__(THREADS) void k_pgw_decide(const WideArgs A, int mode) {
  __shared__ double part[1][16], S[1];
  const int tid = threadIdx.x;
  const uint32_t q = prf::partial_of(tid);
  for_groups(A, 1, 1, [&](Wide &W, size_t, size_t) {
    Ctl &C = *W.ctl;
    const bool live = mode == FIRST || iter_live(C);
    const bool summed = mode == FIRST ? !malformed(C) : trial_live(C);
    __syncthreads();                                         // (thread 0 rewrites what the others have just read)
    if (!live) return;
    double F = 0.0;
    if (summed) F = ordered_sum(W.f, nullptr, W.G.ne, tid, q, part, S);
    if (tid == 0) {
      if (mode == FIRST) ctl_first(C, W.G.ne, F);
      else ctl_trial(C, F, A.p.eps);
    }
    __syncthreads();
  });
}

// ---- a solve ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void k_pgw_setup(const WideArgs A) {
  for_groups(A, A.v_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    Ctl &C = *W.ctl;
    if (!iter_live(C)) return;
    const size_t k = first + threadIdx.x;
    if (k >= W.G.nv || W.G.fixed[k]) return;
    orient(W.G, C.set);
    double d;
    const bool ok = pgr::vertex_setup(W.G, 0, (uint32_t)k, 1.0 + C.lambda, &d);
    W.t[k] = d;
    if (!ok) C.solve_fail = 1;
  });
}

enum : int { BEGIN = 0, ALPHA = 1, BETA = 2 };

// The scalars of the conjugate gradients.  BEGIN: rz, thr; ALPHA: pAp, alpha; BETA (iteration n): rz', beta.
__global__ __launch_bounds__(THREADS) void k_pgw_cg_scalar(const WideArgs A, int mode, int n) {
  __shared__ double part[1][16], S[1];
  const int tid = threadIdx.x;
  const uint32_t q = prf::partial_of(tid);
  for_groups(A, 1, 1, [&](Wide &W, size_t, size_t) {
    Ctl &C = *W.ctl;
    const bool live = mode == BEGIN ? iter_live(C) : cg_live(C);
    const bool summed = mode == BEGIN ? step_live(C) : live;
    __syncthreads();
    if (!live) return;
    double s = 0.0;
    if (summed) s = ordered_sum(W.t, W.G.fixed, W.G.nv, tid, q, part, S);
    if (tid == 0) {
      bool next = false;
      if (mode == BEGIN) {
        C.solves++;
        if (summed) C.rz = s, C.thr = (A.p.cg_tol * A.p.cg_tol) * s, next = true;
      } else if (mode == ALPHA) {
        if (!(s > 0.0)) C.solve_fail = 1;
        else C.alpha = C.rz / s;
      } else {
        C.beta = s / C.rz, C.rz = s;
        next = n + 1 < A.p.cg_iters;
      }
      if (mode != ALPHA) {                                   // the stopping rule of the iteration that would follow
        C.cg_live = next && !(C.rz <= C.thr);
        if (C.cg_live) C.cg_total++;
      }
    }
    __syncthreads();
  });
}

__global__ __launch_bounds__(THREADS) void k_pgw_edge_v(const WideArgs A) {
  for_groups(A, A.e_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    const Ctl &C = *W.ctl;
    if (!cg_live(C)) return;
    const size_t e = first + threadIdx.x;
    if (e >= W.G.ne) return;
    orient(W.G, C.set);
    pgr::edge_v(W.G, 0, (uint32_t)e);
  });
}

enum : int { AP = 0, UPDATE = 1, P = 2 };

// A free vertex's step of an iteration.  P is skipped after the last iteration of a solve: nothing reads that p.
__global__ __launch_bounds__(THREADS) void k_pgw_cg_vertex(const WideArgs A, int mode) {
  for_groups(A, A.v_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    const Ctl &C = *W.ctl;
    if (!cg_live(C)) return;
    const size_t k = first + threadIdx.x;
    if (k >= W.G.nv || W.G.fixed[k]) return;
    if (mode == AP) W.t[k] = pgr::vertex_ap(W.G, (uint32_t)k, C.lambda);
    else if (mode == UPDATE) W.t[k] = pgr::vertex_update(W.G, (uint32_t)k, C.alpha);
    else pgr::vertex_p(W.G, (uint32_t)k, C.beta);
  });
}

__global__ __launch_bounds__(THREADS) void k_pgw_retract(const WideArgs A) {
  for_groups(A, A.v_stride, THREADS, [&](Wide &W, size_t, size_t first) {
    Ctl &C = *W.ctl;
    if (!step_live(C)) return;                               // (the same for the whole workgroup)
    const size_t k = first + threadIdx.x;
    double dm = 0.0;
    if (k < W.G.nv && !W.G.fixed[k]) {
      orient(W.G, C.set);
      if (!pgr::vertex_retract(W.G, 0, (uint32_t)k, &dm)) C.step_bad = 1, dm = 0.0;
    }
    PISLAM_ROLLED
    for (int o = 32; o >= 1; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o, 64));
    // a maximum of non-negative finite doubles is the maximum of their bit patterns
    if ((threadIdx.x & 63) == 0 && dm > 0.0) atomicMax((unsigned long long *)&C.dmax, (unsigned long long)__double_as_longlong(dm));
  });
}

// ---- the outputs -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void k_pgw_out(const WideArgs A) {
  for_groups(A, pgr::STATE * A.v_stride, THREADS, [&](Wide &W, size_t b, size_t first) {
    const Ctl &C = *W.ctl;
    const size_t i = first + threadIdx.x;
    if (i < pgr::STATE * (size_t)W.G.nv) {
      const size_t o = pgr::STATE * b * A.v_stride + i;
      A.sims_out[o] = C.code ? A.sims[o] : (float)W.G.ws.S[C.set ? 1 : 0][i];
    }
    if (i == 0) {
      A.cost[b] = C.F, A.status[b] = C.code | C.evals << 8;
      if (A.work) A.work[2 * b] = C.solves, A.work[2 * b + 1] = C.cg_total;
    }
  });
}

}  // namespace pgw
