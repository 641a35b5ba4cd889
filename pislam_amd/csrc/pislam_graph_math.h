// pislam_graph_math.h — the arithmetic of pislam_pose_graph_batch and pislam_map_points_correct_batch (include/
// pislam_hip.h: those comments are the contract), stated ONCE for the device kernels (pislam_graph_kernels.h, and
// pislam_graph_wide_kernels.h for pislam_pose_graph_wide_batch) and for a plain C++ compiler (tools/probes/
// graph_host_check.cpp, graph_wide_host_check.cpp): composition and error of an edge, the rational residual, the
// structured Jacobians applied to a 7-vector and as a diagonal block, the pivot-free 7 x 7 factorisation, the steps of
// the block-Jacobi preconditioned conjugate gradients as the owner of an edge or of a vertex takes them, the workspace
// slice of a graph and, for the host only, the whole call for one graph run serially.  The retraction is
// s3r::retract, the damping prf::lambda_down / prf::lambda_up.  Everything is binary64; every operation is written out
// one rounding at a time; build with -ffp-contract=off.
#pragma once
#include "pislam_sim3_refine_math.h"

namespace pgr {

using psm::finite_d;
using psm::finite_f;

constexpr int MAX_V = 4096, MAX_E = 16384;      // of pislam_pose_graph_batch (the wide call: pgw::MAX_V, pgw::MAX_E)
constexpr int STATE = 13, DIM = 7, TRI = 28, FAC = 49;
constexpr double ROT_MIN = 0x1p-10;            // an edge is admissible while 1 + tr R_E exceeds this

struct Params {
  int iters, cg_iters;
  double cg_tol, eps;
};

PISLAM_HD void load13(const float *a, double *d) {
PISLAM_UNROLL
  for (int i = 0; i < STATE; i++) d[i] = (double)a[i];
}

// C = A o B for similarities (R, t, s): R_C = R_A R_B, t_C = s_A (R_A t_B) + t_A, s_C = s_A s_B.
PISLAM_HD void compose(const double *A, const double *B, double *C) {
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
    C[9 + i] = A[12] * ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i];
  }
  C[12] = A[12] * B[12];
}

// E = M o S_i o S_j^-1 through G = M o S_i: R_E = R_G R_j', s_E = s_G / s_j, t_E = t_G - s_E (R_E t_j).
PISLAM_HD void edge_error(const double *M, const double *Si, const double *Sj, double *E) {
  double G[STATE];
  compose(M, Si, G);
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++)
      E[3 * i + j] = (G[3 * i] * Sj[3 * j] + G[3 * i + 1] * Sj[3 * j + 1]) + G[3 * i + 2] * Sj[3 * j + 2];
  }
  E[12] = G[12] / Sj[12];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++)
    E[9 + i] = G[9 + i] - E[12] * ((E[3 * i] * Sj[9] + E[3 * i + 1] * Sj[10]) + E[3 * i + 2] * Sj[11]);
}

// r = (omega, upsilon, sigma) of E: the inverse of the retraction at the identity.  False: inadmissible.
PISLAM_HD bool residual(const double *E, double *r) {
  const double c = 1.0 + ((E[0] + E[4]) + E[8]);
  if (!(c > ROT_MIN)) return false;
  r[0] = (2.0 * (E[7] - E[5])) / c;
  r[1] = (2.0 * (E[2] - E[6])) / c;
  r[2] = (2.0 * (E[3] - E[1])) / c;
  r[3] = E[9], r[4] = E[10], r[5] = E[11];
  r[6] = (2.0 * (E[12] - 1.0)) / (E[12] + 1.0);
  return true;
}

PISLAM_HD double dot7(const double *a, const double *b) {
  return (((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]) + a[6] * b[6];
}

// J_i p: with a = R_M omega and c = t_M - t_E it is (a, (c x a + s_M (R_M upsilon)) - sigma c, sigma).
PISLAM_HD void apply_ji(const double *E, const double *M, const double *p, double *o) {
  double a[3], b[3], c[3];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    a[i] = (M[3 * i] * p[0] + M[3 * i + 1] * p[1]) + M[3 * i + 2] * p[2];
    b[i] = M[12] * ((M[3 * i] * p[3] + M[3 * i + 1] * p[4]) + M[3 * i + 2] * p[5]);
    c[i] = M[9 + i] - E[9 + i];
  }
  o[0] = a[0], o[1] = a[1], o[2] = a[2];
  o[3] = ((c[1] * a[2] - c[2] * a[1]) + b[0]) - p[6] * c[0];
  o[4] = ((c[2] * a[0] - c[0] * a[2]) + b[1]) - p[6] * c[1];
  o[5] = ((c[0] * a[1] - c[1] * a[0]) + b[2]) - p[6] * c[2];
  o[6] = p[6];
}

// J_j p = -(R_E omega, s_E (R_E upsilon), sigma).
PISLAM_HD void apply_jj(const double *E, const double *p, double *o) {
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    o[i] = -((E[3 * i] * p[0] + E[3 * i + 1] * p[1]) + E[3 * i + 2] * p[2]);
    o[3 + i] = -(E[12] * ((E[3 * i] * p[3] + E[3 * i + 1] * p[4]) + E[3 * i + 2] * p[5]));
  }
  o[6] = -p[6];
}

// J_i' u = (R_M' (u_w - c x u_v), s_M (R_M' u_v), u_s - c . u_v).
PISLAM_HD void apply_jit(const double *E, const double *M, const double *u, double *o) {
  double c[3], v[3];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) c[i] = M[9 + i] - E[9 + i];
  v[0] = u[0] - (c[1] * u[5] - c[2] * u[4]);
  v[1] = u[1] - (c[2] * u[3] - c[0] * u[5]);
  v[2] = u[2] - (c[0] * u[4] - c[1] * u[3]);
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    o[i] = (M[i] * v[0] + M[3 + i] * v[1]) + M[6 + i] * v[2];
    o[3 + i] = M[12] * ((M[i] * u[3] + M[3 + i] * u[4]) + M[6 + i] * u[5]);
  }
  o[6] = u[6] - ((c[0] * u[3] + c[1] * u[4]) + c[2] * u[5]);
}

// J_j' u = -(R_E' u_w, s_E (R_E' u_v), u_s).
PISLAM_HD void apply_jjt(const double *E, const double *u, double *o) {
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    o[i] = -((E[i] * u[0] + E[3 + i] * u[1]) + E[6 + i] * u[2]);
    o[3 + i] = -(E[12] * ((E[i] * u[3] + E[3 + i] * u[4]) + E[6 + i] * u[5]));
  }
  o[6] = -u[6];
}

// The Jacobian of side 0 (J_i) or 1 (J_j) as a dense 7 x 7 matrix, row-major.
PISLAM_HD void jacobian(int side, const double *E, const double *M, double *J) {
PISLAM_UNROLL
  for (int i = 0; i < FAC; i++) J[i] = 0.0;
  if (side == 0) {
    const double c0 = M[9] - E[9], c1 = M[10] - E[10], c2 = M[11] - E[11];
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) {
      J[j] = M[j], J[7 + j] = M[3 + j], J[14 + j] = M[6 + j];
      J[21 + j] = c1 * M[6 + j] - c2 * M[3 + j];
      J[28 + j] = c2 * M[j] - c0 * M[6 + j];
      J[35 + j] = c0 * M[3 + j] - c1 * M[j];
      J[21 + 3 + j] = M[12] * M[j], J[28 + 3 + j] = M[12] * M[3 + j], J[35 + 3 + j] = M[12] * M[6 + j];
    }
    J[21 + 6] = -c0, J[28 + 6] = -c1, J[35 + 6] = -c2;
    J[48] = 1.0;
  } else {
PISLAM_UNROLL
    for (int i = 0; i < 3; i++) {
PISLAM_UNROLL
      for (int j = 0; j < 3; j++) J[7 * i + j] = -E[3 * i + j], J[7 * (3 + i) + 3 + j] = -(E[12] * E[3 * i + j]);
    }
    J[48] = -1.0;
  }
}

// H = H + w J'J on the upper triangle, row by row: an entry is the sum over the rows of J in ascending order, times w.
PISLAM_HD void block_add(const double *J, double w, double *H) {
  int o = 0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) {
PISLAM_UNROLL
    for (int b = a; b < DIM; b++) {
      double h = J[a] * J[b];
PISLAM_UNROLL
      for (int k = 1; k < DIM; k++) h = h + J[7 * k + a] * J[7 * k + b];
      H[o] = H[o] + w * h;
      o++;
    }
  }
}

// The damped block (H's diagonal times s = 1.0 + lambda) eliminated without pivoting, as pq::solve_n does it: fac holds
// the upper triangle of the eliminated matrix and, below the diagonal, the multipliers.  False: a pivot that is not > 0.
PISLAM_HD bool factor7(const double *H, double s, double *fac) {
  {
    int o = 0;
PISLAM_UNROLL
    for (int j = 0; j < DIM; j++) {
PISLAM_UNROLL
      for (int k = j; k < DIM; k++) {
        fac[7 * j + k] = H[o], fac[7 * k + j] = H[o];
        o++;
      }
    }
  }
PISLAM_UNROLL
  for (int j = 0; j < DIM; j++) fac[8 * j] = fac[8 * j] * s;
  bool ok = true;
PISLAM_UNROLL
  for (int c = 0; c < DIM; c++) {
    ok = ok && fac[8 * c] > 0.0;
PISLAM_UNROLL
    for (int r = c + 1; r < DIM; r++) {
      const double f = fac[7 * r + c] / fac[8 * c];
PISLAM_UNROLL
      for (int j = c + 1; j < DIM; j++) fac[7 * r + j] = fac[7 * r + j] - f * fac[7 * c + j];
      fac[7 * r + c] = f;
    }
  }
  return ok;
}

// x = (the factored block)^-1 b.
PISLAM_HD void sol7(const double *fac, const double *b_in, double *x) {
  double b[DIM];
PISLAM_UNROLL
  for (int i = 0; i < DIM; i++) b[i] = b_in[i];
PISLAM_UNROLL
  for (int c = 0; c < DIM; c++) {
PISLAM_UNROLL
    for (int r = c + 1; r < DIM; r++) b[r] = b[r] - fac[7 * r + c] * b[c];
  }
PISLAM_UNROLL
  for (int r = DIM - 1; r >= 0; r--) {
    double t = b[r];
PISLAM_UNROLL
    for (int j = r + 1; j < DIM; j++) t = t - fac[7 * r + j] * x[j];
    x[r] = t / fac[8 * r];
  }
}

// ---- a graph and its slice of the workspace -------------------------------------------------------------------------

struct Ws {
  double *S[2], *E[2];                         // the similarities and the edge errors of set 0 / 1
  double *v, *fac, *diag, *x, *r, *z, *p, *Ap; // per incidence entry (in the index's order): J'u; per vertex
  uint32_t *pos;                               // the place of entry edge << 1 | side in the index
};

PISLAM_HD size_t ws_carve(char *base, size_t V, size_t N, Ws *w) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = (char *)((uintptr_t)base + o);
    o += (bytes + 15) & ~(size_t)15;
    return (double *)p;
  };
  for (int s = 0; s < 2; s++) w->S[s] = take(8 * STATE * V), w->E[s] = take(8 * STATE * N);
  w->v = take(8 * DIM * 2 * N), w->fac = take(8 * FAC * V), w->diag = take(8 * DIM * V);
  w->x = take(8 * DIM * V), w->r = take(8 * DIM * V), w->z = take(8 * DIM * V), w->p = take(8 * DIM * V);
  w->Ap = take(8 * DIM * V);
  w->pos = (uint32_t *)take(4 * 2 * N);
  return (o + 255) & ~(size_t)255;
}
inline size_t ws_bytes(size_t V, size_t N) {
  Ws w;
  return ws_carve(nullptr, V, N, &w);
}

// One graph as the call reads it, with its slice.
struct Graph {
  const float *sims, *meas, *weight;           // [nv][13], [ne][13], [ne] or null
  const uint8_t *fixed;                        // [nv]
  const uint32_t *edges, *inc_ptr, *inc;       // [ne][2], [nv + 1], [2 ne]
  uint32_t nv, ne;                             // already psm::clamp_count(count, stride)
  Ws ws;
};

PISLAM_HD double edge_weight(const Graph &G, uint32_t e) { return G.weight ? (double)G.weight[e] : 1.0; }

// The structure of edge e and of vertex k's incidence entries.  False: the graph is malformed (code 3).
PISLAM_HD bool edge_in_order(const Graph &G, uint32_t e) {
  const uint32_t i = G.edges[2 * (size_t)e], j = G.edges[2 * (size_t)e + 1];
  return i < G.nv && j < G.nv && i != j;
}
PISLAM_HD bool vertex_in_order(const Graph &G, uint32_t k) {
  const uint32_t a = G.inc_ptr[k], b = G.inc_ptr[k + 1], top = 2u * G.ne;
  if (a > b || b > top || (k == 0 && a != 0u) || (k + 1 == G.nv && b != top)) return false;
  bool ok = true;
  for (uint32_t n = a; n < b; n++) {
    const uint32_t ent = G.inc[n];
    ok = ok && (ent >> 1) < G.ne && G.edges[2 * (size_t)(ent >> 1) + (ent & 1u)] == k;
    ok = ok && (n == a || G.inc[n - 1] < ent);
  }
  return ok;
}

// The words of vertex k and of edge e pass the call's finiteness and sign tests.
PISLAM_HD bool sim_words_ok(const float *s) {
  bool ok = s[12] > 0.0f;
PISLAM_UNROLL
  for (int i = 0; i < STATE; i++) ok = ok && finite_f(s[i]);
  return ok;
}
PISLAM_HD bool edge_words_ok(const Graph &G, uint32_t e) {
  bool ok = sim_words_ok(G.meas + STATE * (size_t)e);
  if (G.weight) ok = ok && finite_f(G.weight[e]) && G.weight[e] >= 0.0f;
  return ok;
}

// Vertex k as the call starts: both sets of the state are double(input); p_k = +0.0, which a fixed vertex keeps; where
// its entries stand in the (checked) index.
PISLAM_HD void vertex_load(const Graph &G, uint32_t k) {
  for (uint32_t n = G.inc_ptr[k]; n < G.inc_ptr[k + 1]; n++) G.ws.pos[G.inc[n]] = n;
  load13(G.sims + STATE * (size_t)k, G.ws.S[0] + STATE * (size_t)k);
  load13(G.sims + STATE * (size_t)k, G.ws.S[1] + STATE * (size_t)k);
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) G.ws.p[DIM * (size_t)k + a] = 0.0;
}

// Edge e at set `set`'s state: E_e into that set; *f = w_e (r . r).  False: inadmissible.
PISLAM_HD bool edge_eval(const Graph &G, int set, uint32_t e, double *f) {
  double M[STATE], E[STATE], r[DIM];
  load13(G.meas + STATE * (size_t)e, M);
  const uint32_t i = G.edges[2 * (size_t)e], j = G.edges[2 * (size_t)e + 1];
  edge_error(M, G.ws.S[set] + STATE * (size_t)i, G.ws.S[set] + STATE * (size_t)j, E);
  double *out = G.ws.E[set] + STATE * (size_t)e;
PISLAM_UNROLL
  for (int k = 0; k < STATE; k++) out[k] = E[k];
  *f = 0.0;
  if (!residual(E, r)) return false;
  *f = edge_weight(G, e) * dot7(r, r);
  return true;
}

// The free vertex k before the first iteration of a solve at s = 1.0 + lambda: its block and gradient over its entries
// in ascending order, the factors, r = -g, z, p = z, x = 0; *rz = r . z.  False: a pivot that is not > 0.
PISLAM_HD bool vertex_setup(const Graph &G, int set, uint32_t k, double s, double *rz) {
  double H[TRI], g[DIM];
PISLAM_UNROLL
  for (int a = 0; a < TRI; a++) H[a] = 0.0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) g[a] = 0.0;
  for (uint32_t n = G.inc_ptr[k]; n < G.inc_ptr[k + 1]; n++) {
    const uint32_t ent = G.inc[n], e = ent >> 1;
    const double *E = G.ws.E[set] + STATE * (size_t)e;
    double M[STATE], J[FAC], r[DIM], t[DIM], v[DIM];
    load13(G.meas + STATE * (size_t)e, M);
    const double w = edge_weight(G, e);
    jacobian((int)(ent & 1u), E, M, J);
    block_add(J, w, H);
    residual(E, r);
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) t[a] = w * r[a];
    if (ent & 1u) apply_jjt(E, t, v);
    else apply_jit(E, M, t, v);
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) g[a] = g[a] + v[a];
  }
  double *fac = G.ws.fac + FAC * (size_t)k, *diag = G.ws.diag + DIM * (size_t)k;
  {
    int o = 0;
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) diag[a] = H[o], o += DIM - a;
  }
  const bool ok = factor7(H, s, fac);
  double *x = G.ws.x + DIM * (size_t)k, *r = G.ws.r + DIM * (size_t)k, *z = G.ws.z + DIM * (size_t)k;
  double *p = G.ws.p + DIM * (size_t)k;
  double rr[DIM], zz[DIM];
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) rr[a] = -g[a];
  sol7(fac, rr, zz);
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) x[a] = 0.0, r[a] = rr[a], z[a] = zz[a], p[a] = zz[a];
  *rz = dot7(rr, zz);
  return ok;
}

// u_e = w_e (J_i p_i + J_j p_j); p of a fixed vertex is 0.  What the edge's two vertices will add, J_i' u_e and J_j' u_e,
// goes to the places of its two entries in the index, so that a vertex reads its terms in one contiguous run.
PISLAM_HD void edge_v(const Graph &G, int set, uint32_t e) {
  const double *E = G.ws.E[set] + STATE * (size_t)e;
  double M[STATE], a[DIM], b[DIM];
  load13(G.meas + STATE * (size_t)e, M);
  const uint32_t i = G.edges[2 * (size_t)e], j = G.edges[2 * (size_t)e + 1];
  apply_ji(E, M, G.ws.p + DIM * (size_t)i, a);
  apply_jj(E, G.ws.p + DIM * (size_t)j, b);
  const double w = edge_weight(G, e);
  double u[DIM], vi[DIM], vj[DIM];
PISLAM_UNROLL
  for (int k = 0; k < DIM; k++) u[k] = w * (a[k] + b[k]);
  apply_jit(E, M, u, vi);
  apply_jjt(E, u, vj);
  double *oi = G.ws.v + DIM * (size_t)G.ws.pos[2 * (size_t)e], *oj = G.ws.v + DIM * (size_t)G.ws.pos[2 * (size_t)e + 1];
PISLAM_UNROLL
  for (int k = 0; k < DIM; k++) oi[k] = vi[k], oj[k] = vj[k];
}

// (A p)_k of the free vertex k over its entries in ascending order, plus lambda diag p_k; returns p_k . (A p)_k.
PISLAM_HD double vertex_ap(const Graph &G, uint32_t k, double lambda) {
  double s[DIM];
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) s[a] = 0.0;
  const uint32_t n0 = G.inc_ptr[k], n1 = G.inc_ptr[k + 1];
  for (uint32_t n = n0; n < n1; n++) {
    const double *v = G.ws.v + DIM * (size_t)n;
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) s[a] = s[a] + v[a];
  }
  const double *diag = G.ws.diag + DIM * (size_t)k, *p = G.ws.p + DIM * (size_t)k;
  double *Ap = G.ws.Ap + DIM * (size_t)k;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) s[a] = s[a] + (lambda * diag[a]) * p[a], Ap[a] = s[a];
  return dot7(p, s);
}

// x_k = x_k + alpha p_k, r_k = r_k - alpha (A p)_k, z_k = block^-1 r_k; returns r_k . z_k.
PISLAM_HD double vertex_update(const Graph &G, uint32_t k, double alpha) {
  double *x = G.ws.x + DIM * (size_t)k, *r = G.ws.r + DIM * (size_t)k, *z = G.ws.z + DIM * (size_t)k;
  const double *p = G.ws.p + DIM * (size_t)k, *Ap = G.ws.Ap + DIM * (size_t)k;
  double rr[DIM], zz[DIM];
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) x[a] = x[a] + alpha * p[a], rr[a] = r[a] - alpha * Ap[a];
  sol7(G.ws.fac + FAC * (size_t)k, rr, zz);
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) r[a] = rr[a], z[a] = zz[a];
  return dot7(rr, zz);
}

// p_k = z_k + beta p_k.
PISLAM_HD void vertex_p(const Graph &G, uint32_t k, double beta) {
  const double *z = G.ws.z + DIM * (size_t)k;
  double *p = G.ws.p + DIM * (size_t)k;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) p[a] = z[a] + beta * p[a];
}

// The trial similarity of the free vertex k into the other set; *dm = its largest |increment word|.  False: a word of
// the increment is not finite or |sigma| < 2 is false (the scale factor of the retraction must stay positive).
PISLAM_HD bool vertex_retract(const Graph &G, int set, uint32_t k, double *dm) {
  const double *d = G.ws.x + DIM * (size_t)k;
  bool ok = fabs(d[6]) < 2.0;
  double m = 0.0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) ok = ok && finite_d(d[a]), m = fmax(m, fabs(d[a]));
  *dm = m;
  s3r::retract(G.ws.S[set] + STATE * (size_t)k, d, G.ws.S[set ^ 1] + STATE * (size_t)k);
  return ok;
}

// ---- pislam_map_points_correct_batch: one point ---------------------------------------------------------------------

// X' = S_new^-1(S_old(X)) in binary64, rounded once.  False: a word of the result is not finite (out is not written).
PISLAM_HD bool correct_point(const float *so, const float *sn, const float *X, float *out) {
  double A[STATE], B[STATE], c[3], d[3];
  load13(so, A), load13(sn, B);
  const double x0 = (double)X[0], x1 = (double)X[1], x2 = (double)X[2];
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    c[i] = A[12] * ((A[3 * i] * x0 + A[3 * i + 1] * x1) + A[3 * i + 2] * x2) + A[9 + i];
    d[i] = c[i] - B[9 + i];
  }
  float y[3];
  bool ok = true;
PISLAM_UNROLL
  for (int i = 0; i < 3; i++) {
    y[i] = (float)(((B[i] * d[0] + B[3 + i] * d[1]) + B[6 + i] * d[2]) / B[12]);
    ok = ok && finite_f(y[i]);
  }
  if (!ok) return false;
  out[0] = y[0], out[1] = y[1], out[2] = y[2];
  return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one graph (the probe; never the library's hot path) ---------------

struct Result {
  uint32_t status, cg_total, solves;           // cg_total: conjugate-gradient iterations over the `solves` solves begun
  double cost;
};

inline double host_tree(double *p) {
  for (int h = prf::PARTIALS / 2; h >= 1; h /= 2)
    for (int q = 0; q < h; q++) p[q] += p[q + h];
  return p[0];
}

// F at set `set`'s state.  False: inadmissible.
inline bool host_eval(const Graph &G, int set, double *F) {
  double p[prf::PARTIALS] = {0.0};
  bool ok = true;
  for (uint32_t e = 0; e < G.ne; e++) {
    double f;
    ok = edge_eval(G, set, e, &f) && ok;
    p[e % prf::PARTIALS] += f;
  }
  *F = host_tree(p);
  return ok;
}

// The sum over the free vertices of fn(k) in the contract's order.
template <class FN>
inline double host_vertex_sum(const Graph &G, const FN &fn) {
  double p[prf::PARTIALS] = {0.0};
  for (uint32_t k = 0; k < G.nv; k++)
    if (!G.fixed[k]) p[k % prf::PARTIALS] += fn(k);
  return host_tree(p);
}

// One solve at lambda from set `set`: the trial state goes to the other set.  False: no step at this lambda.
inline bool host_solve(const Graph &G, const Params &P, int set, double lambda, double *dmax, uint32_t *cg) {
  bool ok = true;
  double rz = host_vertex_sum(G, [&](uint32_t k) {
    double d;
    ok = vertex_setup(G, set, k, 1.0 + lambda, &d) && ok;
    return d;
  });
  if (!ok) return false;
  const double thr = (P.cg_tol * P.cg_tol) * rz;
  for (int n = 0; n < P.cg_iters; n++) {
    if (rz <= thr) break;
    (*cg)++;
    for (uint32_t e = 0; e < G.ne; e++) edge_v(G, set, e);
    const double pAp = host_vertex_sum(G, [&](uint32_t k) { return vertex_ap(G, k, lambda); });
    if (!(pAp > 0.0)) return false;
    const double alpha = rz / pAp;
    const double rz1 = host_vertex_sum(G, [&](uint32_t k) { return vertex_update(G, k, alpha); });
    const double beta = rz1 / rz;
    for (uint32_t k = 0; k < G.nv; k++)
      if (!G.fixed[k]) vertex_p(G, k, beta);
    rz = rz1;
  }
  *dmax = 0.0;
  for (uint32_t k = 0; k < G.nv; k++) {
    if (G.fixed[k]) continue;
    double dm;
    ok = vertex_retract(G, set, k, &dm) && ok;
    *dmax = fmax(*dmax, dm);
  }
  return ok;
}

// The whole call for one graph; G.ws is a slice of ws_bytes(nv, ne) (or larger strides).
inline void host_graph(const Graph &G, const Params &P, float *sims_out, Result *R) {
  R->cost = 0.0, R->cg_total = 0, R->solves = 0;
  auto refuse = [&](uint32_t code) {
    for (size_t i = 0; i < STATE * (size_t)G.nv; i++) sims_out[i] = G.sims[i];
    R->status = code;
  };
  bool bad = false, any_fixed = false, any_free = false;
  for (uint32_t e = 0; e < G.ne; e++) bad = bad || !edge_in_order(G, e);
  for (uint32_t k = 0; k < G.nv; k++) {
    bad = bad || !vertex_in_order(G, k);
    (G.fixed[k] ? any_fixed : any_free) = true;
  }
  if (bad || !any_fixed) return refuse(3);
  bool inf = false;
  for (uint32_t k = 0; k < G.nv; k++) {
    inf = inf || !sim_words_ok(G.sims + STATE * (size_t)k);
    vertex_load(G, k);
  }
  for (uint32_t e = 0; e < G.ne; e++) inf = inf || !edge_words_ok(G, e);
  int set = 0;
  double F;
  const bool adm = host_eval(G, set, &F);
  if (inf || !adm) return refuse(2);
  if (G.ne == 0 || !any_free) return refuse(1);
  uint32_t evals = 1;
  double lambda = prf::LAMBDA_0;
  for (int it = 0; it < P.iters; it++) {
    double dmax, Ft;
    R->solves++;
    if (!host_solve(G, P, set, lambda, &dmax, &R->cg_total)) {
      lambda = prf::lambda_up(lambda);
      continue;
    }
    const bool ok = host_eval(G, set ^ 1, &Ft);
    evals++;
    if (!ok) {
      lambda = prf::lambda_up(lambda);
      continue;
    }
    if (Ft < F) {
      F = Ft, set ^= 1;
      lambda = prf::lambda_down(lambda);
    } else {
      lambda = prf::lambda_up(lambda);
    }
    if (dmax <= P.eps) break;
  }
  for (size_t i = 0; i < STATE * (size_t)G.nv; i++) sims_out[i] = (float)G.ws.S[set][i];
  R->cost = F, R->status = evals << 8;
}
#endif

}  // namespace pgr
