// pislam_gba_math.h — the arithmetic of pislam_global_ba_batch (include/pislam_hip.h: that comment is the contract), stated
// ONCE for the device kernels (pislam_gba_kernels.h) and for a plain C++ compiler (tools/probes/gba_host_check.cpp): what
// the owner of an observation, of a point, of a key frame's partial sum and of a key frame does in every phase, the
// Levenberg rule on a map's control block, the map's slice of the workspace and, for the host only, the whole call for
// one map run serially in the order of the launches (gba::host_map).  One observation, the point blocks and their
// solves are the local bundle adjustment's (pba::pass_one, pba::factor3, pba::solve3), the damping is prf::lambda_down /
// prf::lambda_up, the retraction pq::retract.  Every operation is written out one rounding at a time; build with
// -ffp-contract=off.
#pragma once
#include <vector>
#include "pislam_ba_math.h"

namespace gba {

using psm::finite_d;
using psm::finite_f;

constexpr int MAX_KF = 4096, MAX_ROUNDS = pba::MAX_ROUNDS, MAX_ITERS = 32, MAX_CG = 256;
constexpr size_t MAX_PTS = (size_t)1 << 22, MAX_STRIDE = (size_t)1 << 24;
constexpr int CAM = pba::CAM, CROSS = pba::CROSS, PT = pba::PT;
constexpr int KPART = 64;                      // partial sums of a key frame's entries: one per lane of its wave
constexpr int TRI = 21, DIM = 6, FAC = 36;
constexpr int SETUP_SUMS = CAM + TRI + DIM;    // H_k 21, g_k 6; the Schur terms of the block 21 and of the right-hand side 6

struct Params {
  pba::Params ba;
  int cg_iters;
  double cg_tol;
};

// A map's control block: what the launches of a call hand to one another.  Written by ONE thread of the map's own
// workgroup in the begin, scalar and decide phases; the flags bad3, bad2, any_free, solve_fail and step_bad are raised
// (to 1, by any number of writers) in the phases between, and dmax is raised by a maximum.
struct Ctl {
  double S[3];                                 // (F, the contributing observations, their chi2) at the current state
  double lambda, rz, thr, cost;
  double dmax;                                 // the largest |increment word| of a step (a maximum: no order; >= +0.0)
  uint32_t bad3, bad2, any_free;
  uint32_t done, code, evals, ninl, set;       // done: refused, or ended: every later launch returns at once
  uint32_t round_over, solve_fail, step_bad, cg_live;
  uint32_t solves, cg_total, cg_last, fails;   // solves begun, PCG iterations of all solves and of the last one, solves
  uint32_t rejects, pad;                       //   or steps that failed, steps that did not lower F
};

// A map's slice of the workspace.
struct Ws {
  double *T[2], *Hd, *fac, *x, *r, *z, *p, *Sp, *dot;   // per key frame: the poses of set 0 / 1, H' (21), the factors of S_kk
  float *Tf[2];                                //   and the PCG vectors; the poses of a pass as binary32 words
  double *X[2], *V[2], *sub, *pfac, *q;        // per point: state, sums (V 6, g 3) of set 0 / 1, (rho, n, c), factors, q_p
  uint32_t *pstart;                            // [P + 1]: a point's first observation
  uint8_t *held;
  float *cam[2], *cross[2];                    // per observation, set 0 / 1
  uint8_t *on[2];
};

PISLAM_HD size_t ws_carve(char *base, size_t K, size_t P, size_t N, Ws *w) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = (char *)((uintptr_t)base + o);
    o += (bytes + 15) & ~(size_t)15;
    return p;
  };
  for (int s = 0; s < 2; s++) w->T[s] = (double *)take(8 * 12 * K), w->Tf[s] = (float *)take(4 * 12 * K);
  w->Hd = (double *)take(8 * TRI * K), w->fac = (double *)take(8 * FAC * K);
  w->x = (double *)take(8 * DIM * K), w->r = (double *)take(8 * DIM * K), w->z = (double *)take(8 * DIM * K);
  w->p = (double *)take(8 * DIM * K), w->Sp = (double *)take(8 * DIM * K), w->dot = (double *)take(8 * K);
  for (int s = 0; s < 2; s++) w->X[s] = (double *)take(8 * 3 * P), w->V[s] = (double *)take(8 * PT * P);
  w->sub = (double *)take(8 * 3 * P), w->pfac = (double *)take(8 * 9 * P), w->q = (double *)take(8 * 3 * P);
  w->pstart = (uint32_t *)take(4 * (P + 1));
  w->held = (uint8_t *)take(P);
  for (int s = 0; s < 2; s++) {
    w->cam[s] = (float *)take(4 * CAM * N), w->cross[s] = (float *)take(4 * CROSS * N);
    w->on[s] = (uint8_t *)take(N);
  }
  return (o + 255) & ~(size_t)255;
}
inline size_t ws_bytes(size_t K, size_t P, size_t N) {
  Ws w;
  return ws_carve(nullptr, K, P, N, &w);
}
constexpr size_t CTL_BYTES = 256;              // a control block's place at the head of the workspace
static_assert(sizeof(Ctl) <= CTL_BYTES, "the control block outgrew its place");

// One map as the call reads it, with its slice and its control block.
struct Map {
  const float *poses, *cams, *xw;              // [nk][12], [nk][5], [npt][3]
  const int32_t *obs, *pt;                     // [n][3], [n]
  const uint16_t *kf;                          // [n]
  const uint8_t *level, *fixed;                // [n] or null, [nk]
  const uint32_t *kf_ptr, *kf_obs;             // [nk + 1], [n]
  pba::Window W;                               // what pba::pass_one reads: obs, level, the level table
  uint32_t nk, npt, n;                         // nk, n: 0 if the count is out of range (then `shaped` is false)
  bool shaped;
  Ws ws;
  Ctl *ctl;
};

// The signed counts of a map, checked as the covisibility call checks them; pt_counts clamped as the local call does.
PISLAM_HD void map_counts(Map &M, int32_t count, int32_t kf_count, uint32_t pt_count, size_t stride, size_t kf_stride,
                          size_t pt_stride) {
  M.shaped = count >= 0 && (size_t)count <= stride && kf_count >= 0 && (size_t)kf_count <= kf_stride;
  M.n = M.shaped ? (uint32_t)count : 0u, M.nk = M.shaped ? (uint32_t)kf_count : 0u;
  M.npt = psm::clamp_count(pt_count, pt_stride);
}

// ---- the checks (code 3, code 2) ------------------------------------------------------------------------------------

// Observation i exists in the map and comes after observation i - 1.
PISLAM_HD bool obs_in_order(const Map &M, uint32_t i) {
  if (M.kf[i] >= M.nk || M.pt[i] < 0 || (uint32_t)M.pt[i] >= M.npt) return false;
  if (i == 0) return true;
  return M.pt[i] > M.pt[i - 1] || (M.pt[i] == M.pt[i - 1] && M.kf[i] > M.kf[i - 1]);
}
// Key frame k's range of the index, and entry j of it.
PISLAM_HD bool kf_range_ok(const Map &M, uint32_t k) {
  const uint32_t a = M.kf_ptr[k], b = M.kf_ptr[k + 1];
  return a <= b && b <= M.n && (k != 0 || a == 0u) && (k + 1 != M.nk || b == M.n);
}
PISLAM_HD bool kf_entry_ok(const Map &M, uint32_t k, uint32_t j) {
  const uint32_t e = M.kf_obs[j];
  return e < M.n && M.kf[e] == k && (j == M.kf_ptr[k] || M.kf_obs[j - 1] < e);
}
PISLAM_HD bool kf_words_ok(const Map &M, uint32_t k) {
  bool ok = true;
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) ok = ok && finite_f(M.poses[12 * (size_t)k + i]);
PISLAM_UNROLL
  for (int i = 0; i < 5; i++) ok = ok && finite_f(M.cams[5 * (size_t)k + i]);
  return ok;
}
PISLAM_HD bool pt_words_ok(const Map &M, uint32_t p) {
  const float *x = M.xw + 3 * (size_t)p;
  return finite_f(x[0]) && finite_f(x[1]) && finite_f(x[2]);
}

// The refusal of a map from its flags: code 3, then 2, then 1; 0: the map runs.
PISLAM_HD uint32_t refusal(const Map &M, const Ctl &C, int min_obs) {
  if (!M.shaped || C.bad3) return 3u;
  if (C.bad2) return 2u;
  return M.n < (uint32_t)min_obs || !C.any_free ? 1u : 0u;
}

// ---- the state as the call starts -----------------------------------------------------------------------------------

PISLAM_HD void load_kf(const Map &M, uint32_t k) {
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) {
    const float v = M.poses[12 * (size_t)k + i];
    M.ws.T[0][12 * (size_t)k + i] = (double)v, M.ws.T[1][12 * (size_t)k + i] = (double)v;
    M.ws.Tf[0][12 * (size_t)k + i] = v, M.ws.Tf[1][12 * (size_t)k + i] = v;
  }
}
// First observation of point p: the lower bound of p in the ascending pt[0 .. n).
PISLAM_HD uint32_t first_obs(const Map &M, uint32_t p) {
  uint32_t lo = 0, hi = M.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)M.pt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// p <= npt: pstart[npt] = n.
PISLAM_HD void load_pt(const Map &M, uint32_t p) {
  M.ws.pstart[p] = p < M.npt ? first_obs(M, p) : M.n;
  if (p < M.npt) {
PISLAM_UNROLL
    for (int j = 0; j < 3; j++) M.ws.X[0][3 * (size_t)p + j] = (double)M.xw[3 * (size_t)p + j];
  }
}

// ---- a pass: the owner of point p -----------------------------------------------------------------------------------

PISLAM_HD void pass_point(const Map &M, int set, uint32_t p, bool classify, bool robust, uint8_t *active) {
  const double *Xs = M.ws.X[set] + 3 * (size_t)p;
  const float Xf[3] = {(float)Xs[0], (float)Xs[1], (float)Xs[2]};
  double v[PT], s[3] = {0.0, 0.0, 0.0};
PISLAM_UNROLL
  for (int j = 0; j < PT; j++) v[j] = 0.0;
  const uint32_t i1 = M.ws.pstart[p + 1];
  for (uint32_t i = M.ws.pstart[p]; i < i1; i++) {
    const uint32_t k = M.kf[i];
    pba::ObsTerms t;
    const bool c = pba::pass_one(M.W, i, M.ws.Tf[set] + 12 * (size_t)k, M.cams + 5 * (size_t)k, Xf, classify, robust, &active[i], t);
    M.ws.on[set][i] = c;
    if (!c) continue;
PISLAM_UNROLL
    for (int j = 0; j < PT; j++) v[j] = v[j] + (double)t.pt[j];
    s[0] = s[0] + (double)t.cam[27], s[1] = s[1] + 1.0, s[2] = s[2] + (double)t.chi2;
    if (!M.fixed[k]) {
      float *c_ = M.ws.cam[set] + CAM * (size_t)i, *x_ = M.ws.cross[set] + CROSS * (size_t)i;
PISLAM_UNROLL
      for (int j = 0; j < CAM; j++) c_[j] = t.cam[j];
PISLAM_UNROLL
      for (int j = 0; j < CROSS; j++) x_[j] = t.cross[j];
    }
  }
PISLAM_UNROLL
  for (int j = 0; j < PT; j++) M.ws.V[set][PT * (size_t)p + j] = v[j];
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) M.ws.sub[3 * (size_t)p + j] = s[j];
}

// ---- a solve at s = 1.0 + lambda ------------------------------------------------------------------------------------

PISLAM_HD void point_factor(const Map &M, int set, uint32_t p, double s) {
  M.ws.held[p] = !pba::factor3(M.ws.V[set] + PT * (size_t)p, s, M.ws.pfac + 9 * (size_t)p);
}

PISLAM_HD double dot6(const double *a, const double *b) {
  return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

// The 6 x 6 block B (upper triangle, row by row) eliminated without pivoting, as pq::solve_n does it: fac holds the
// upper triangle of the eliminated matrix and, below the diagonal, the multipliers.  False: a pivot that is not > 0.
PISLAM_HD bool factor6(const double *B, double *fac) {
  {
    int o = 0;
PISLAM_UNROLL
    for (int j = 0; j < DIM; j++) {
PISLAM_UNROLL
      for (int k = j; k < DIM; k++) {
        fac[6 * j + k] = B[o], fac[6 * k + j] = B[o];
        o++;
      }
    }
  }
  bool ok = true;
PISLAM_UNROLL
  for (int c = 0; c < DIM; c++) {
    ok = ok && fac[7 * c] > 0.0;
PISLAM_UNROLL
    for (int r = c + 1; r < DIM; r++) {
      const double f = fac[6 * r + c] / fac[7 * c];
PISLAM_UNROLL
      for (int j = c + 1; j < DIM; j++) fac[6 * r + j] = fac[6 * r + j] - f * fac[6 * c + j];
      fac[6 * r + c] = f;
    }
  }
  return ok;
}
PISLAM_HD void sol6(const double *fac, const double *b_in, double *x) {
  double b[DIM];
PISLAM_UNROLL
  for (int i = 0; i < DIM; i++) b[i] = b_in[i];
PISLAM_UNROLL
  for (int c = 0; c < DIM; c++) {
PISLAM_UNROLL
    for (int r = c + 1; r < DIM; r++) b[r] = b[r] - fac[6 * r + c] * b[c];
  }
PISLAM_UNROLL
  for (int r = DIM - 1; r >= 0; r--) {
    double t = b[r];
PISLAM_UNROLL
    for (int j = r + 1; j < DIM; j++) t = t - fac[6 * r + j] * x[j];
    x[r] = t / fac[7 * r];
  }
}

// Entry j of a key frame's list as the Schur sums read it: the observation o; it takes part (it contributes and its
// point is not held); its point.
PISLAM_HD bool schur_entry(const Map &M, int set, uint32_t j, uint32_t *o, uint32_t *p) {
  *o = M.kf_obs[j];
  *p = (uint32_t)M.pt[*o];
  return M.ws.on[set][*o] && !M.ws.held[*p];
}

// Partial q of the free key frame k's set-up sums: its entries at the places q, q + 64, ... in ascending order, from
// +0.0.  acc[0 .. 26]: H_k, g_k over the contributing entries; acc[27 .. 47]: the upper triangle of sum W V'^-1 W' and
// acc[48 .. 53]: sum W V'^-1 g_p over the entries that take part.
PISLAM_HD void kf_setup_partial(const Map &M, int set, uint32_t k, uint32_t q, double *acc) {
PISLAM_UNROLL
  for (int t = 0; t < SETUP_SUMS; t++) acc[t] = 0.0;
  const uint32_t e1 = M.kf_ptr[k + 1];
  for (uint32_t j = M.kf_ptr[k] + q; j < e1; j += KPART) {
    uint32_t o, p;
    const bool part = schur_entry(M, set, j, &o, &p);
    if (!M.ws.on[set][o]) continue;
    const float *c = M.ws.cam[set] + CAM * (size_t)o;
PISLAM_UNROLL
    for (int t = 0; t < CAM; t++) acc[t] = acc[t] + (double)c[t];
    if (!part) continue;
    const float *wf = M.ws.cross[set] + CROSS * (size_t)o;
    const double *F = M.ws.pfac + 9 * (size_t)p, *g = M.ws.V[set] + PT * (size_t)p + 6;
    double w[CROSS], y[CROSS];
PISLAM_UNROLL
    for (int t = 0; t < CROSS; t++) w[t] = (double)wf[t];
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) pba::solve3(F, w[3 * a], w[3 * a + 1], w[3 * a + 2], y + 3 * a);
    int t = CAM;
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++) {
PISLAM_UNROLL
      for (int b = a; b < DIM; b++) {
        acc[t] = acc[t] + ((y[3 * a] * w[3 * b] + y[3 * a + 1] * w[3 * b + 1]) + y[3 * a + 2] * w[3 * b + 2]);
        t++;
      }
    }
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++)
      acc[CAM + TRI + a] = acc[CAM + TRI + a] + ((y[3 * a] * g[0] + y[3 * a + 1] * g[1]) + y[3 * a + 2] * g[2]);
  }
}
// The free key frame k from its combined set-up sums: H' = H_k with its diagonal times s, the block S_kk = H' - sum and
// its factors, r = (-g_k) + sum, z = Sol_k(r), p = z, x = 0, dot = r . z.  False: a pivot that is not > 0.
PISLAM_HD bool kf_setup_finish(const Map &M, uint32_t k, double s, const double *sums) {
  double Hd[TRI], B[TRI], r[DIM], z[DIM];
  int o = 0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) {
PISLAM_UNROLL
    for (int b = a; b < DIM; b++) {
      Hd[o] = a == b ? sums[o] * s : sums[o];
      B[o] = Hd[o] - sums[CAM + o];
      o++;
    }
  }
  double *fac = M.ws.fac + FAC * (size_t)k;
  const bool ok = factor6(B, fac);
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) r[a] = -sums[TRI + a] + sums[CAM + TRI + a];
  sol6(fac, r, z);
PISLAM_UNROLL
  for (int t = 0; t < TRI; t++) M.ws.Hd[TRI * (size_t)k + t] = Hd[t];
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) {
    M.ws.x[DIM * (size_t)k + a] = 0.0, M.ws.r[DIM * (size_t)k + a] = r[a];
    M.ws.z[DIM * (size_t)k + a] = z[a], M.ws.p[DIM * (size_t)k + a] = z[a];
  }
  M.ws.dot[k] = dot6(r, z);
  return ok;
}

// W_o' e for the columns j = 0..2 of an observation's cross terms: b_j = b_j + sign * (the six products from the left).
PISLAM_HD void cross_t(const float *w, const double *e, double sign, double *b) {
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
    const double t = (((((double)w[j] * e[0] + (double)w[3 + j] * e[1]) + (double)w[6 + j] * e[2]) + (double)w[9 + j] * e[3]) +
                      (double)w[12 + j] * e[4]) + (double)w[15 + j] * e[5];
    b[j] = sign > 0.0 ? b[j] + t : b[j] - t;
  }
}

// One PCG iteration, the owner of point p: t_p over its contributing observations of free key frames, q_p = Sol_p(t_p).
PISLAM_HD void cg_point(const Map &M, int set, uint32_t p) {
  double t[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  if (!M.ws.held[p]) {
    const uint32_t i1 = M.ws.pstart[p + 1];
    for (uint32_t i = M.ws.pstart[p]; i < i1; i++) {
      const uint32_t k = M.kf[i];
      if (!M.ws.on[set][i] || M.fixed[k]) continue;
      cross_t(M.ws.cross[set] + CROSS * (size_t)i, M.ws.p + DIM * (size_t)k, 1.0, t);
    }
    pba::solve3(M.ws.pfac + 9 * (size_t)p, t[0], t[1], t[2], q);
  }
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) M.ws.q[3 * (size_t)p + j] = q[j];
}

// Partial q of sum W_o q_p over the free key frame k's entries that take part.
PISLAM_HD void kf_sp_partial(const Map &M, int set, uint32_t k, uint32_t q, double *acc) {
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) acc[a] = 0.0;
  const uint32_t e1 = M.kf_ptr[k + 1];
  for (uint32_t j = M.kf_ptr[k] + q; j < e1; j += KPART) {
    uint32_t o, p;
    if (!schur_entry(M, set, j, &o, &p)) continue;
    const float *w = M.ws.cross[set] + CROSS * (size_t)o;
    const double *qp = M.ws.q + 3 * (size_t)p;
PISLAM_UNROLL
    for (int a = 0; a < DIM; a++)
      acc[a] = acc[a] + (((double)w[3 * a] * qp[0] + (double)w[3 * a + 1] * qp[1]) + (double)w[3 * a + 2] * qp[2]);
  }
}
// (S p)_k = H'_k p_k - sum.
PISLAM_HD void kf_sp_finish(const Map &M, uint32_t k, const double *sums) {
  const double *Hd = M.ws.Hd + TRI * (size_t)k, *p = M.ws.p + DIM * (size_t)k;
  double H[DIM][DIM];
  int o = 0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) {
PISLAM_UNROLL
    for (int b = a; b < DIM; b++) {
      H[a][b] = Hd[o], H[b][a] = Hd[o];
      o++;
    }
  }
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) M.ws.Sp[DIM * (size_t)k + a] = dot6(H[a], p) - sums[a];
}

PISLAM_HD double kf_pap(const Map &M, uint32_t k) { return dot6(M.ws.p + DIM * (size_t)k, M.ws.Sp + DIM * (size_t)k); }
// x_k = x_k + alpha p_k, r_k = r_k - alpha (S p)_k, z_k = Sol_k(r_k); returns r_k . z_k.
PISLAM_HD double kf_update(const Map &M, uint32_t k, double alpha) {
  double *x = M.ws.x + DIM * (size_t)k, *r = M.ws.r + DIM * (size_t)k, *z = M.ws.z + DIM * (size_t)k;
  const double *p = M.ws.p + DIM * (size_t)k, *Sp = M.ws.Sp + DIM * (size_t)k;
  double rr[DIM], zz[DIM];
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) x[a] = x[a] + alpha * p[a], rr[a] = r[a] - alpha * Sp[a];
  sol6(M.ws.fac + FAC * (size_t)k, rr, zz);
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) r[a] = rr[a], z[a] = zz[a];
  return dot6(rr, zz);
}
PISLAM_HD void kf_p(const Map &M, uint32_t k, double beta) {
  const double *z = M.ws.z + DIM * (size_t)k;
  double *p = M.ws.p + DIM * (size_t)k;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) p[a] = z[a] + beta * p[a];
}

// The step of the free key frame k: d = x_k, the trial pose into the other set.  False: a word of d is not finite.
PISLAM_HD bool kf_step(const Map &M, int set, uint32_t k, double *dm) {
  const double *d = M.ws.x + DIM * (size_t)k;
  bool ok = true;
  double m = 0.0;
PISLAM_UNROLL
  for (int a = 0; a < DIM; a++) ok = ok && finite_d(d[a]), m = fmax(m, fabs(d[a]));
  *dm = m;
  double Tn[12];
  pq::retract(M.ws.T[set] + 12 * (size_t)k, d, Tn);
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) M.ws.T[set ^ 1][12 * (size_t)k + i] = Tn[i], M.ws.Tf[set ^ 1][12 * (size_t)k + i] = (float)Tn[i];
  return ok;
}
// The step of point p: dp = Sol_p(-g_p - W_p' d), the trial point into the other set.  False: a word is not finite.
PISLAM_HD bool point_step(const Map &M, int set, uint32_t p, double *dm) {
  double dp[3] = {0.0, 0.0, 0.0};
  if (!M.ws.held[p]) {
    const double *g = M.ws.V[set] + PT * (size_t)p + 6;
    double b[3] = {-g[0], -g[1], -g[2]};
    const uint32_t i1 = M.ws.pstart[p + 1];
    for (uint32_t i = M.ws.pstart[p]; i < i1; i++) {
      const uint32_t k = M.kf[i];
      if (!M.ws.on[set][i] || M.fixed[k]) continue;
      cross_t(M.ws.cross[set] + CROSS * (size_t)i, M.ws.x + DIM * (size_t)k, -1.0, b);
    }
    pba::solve3(M.ws.pfac + 9 * (size_t)p, b[0], b[1], b[2], dp);
  }
  double m = 0.0;
PISLAM_UNROLL
  for (int j = 0; j < 3; j++) {
    M.ws.X[set ^ 1][3 * (size_t)p + j] = M.ws.X[set][3 * (size_t)p + j] + dp[j];
    m = fmax(m, fabs(dp[j]));
  }
  *dm = m;
  return finite_d(dp[0]) && finite_d(dp[1]) && finite_d(dp[2]);
}

// ---- the rule on the control block (one thread of the map) ----------------------------------------------------------

// Which launches find work.
PISLAM_HD bool iter_live(const Ctl &C) { return !C.done && !C.round_over; }
PISLAM_HD bool cg_live(const Ctl &C) { return iter_live(C) && C.cg_live && !C.solve_fail; }
PISLAM_HD bool step_live(const Ctl &C) { return iter_live(C) && !C.solve_fail; }
PISLAM_HD bool trial_live(const Ctl &C) { return step_live(C) && !C.step_bad; }

PISLAM_HD void ctl_next_solve(Ctl &C) { C.solve_fail = 0, C.step_bad = 0, C.dmax = 0.0, C.cg_live = 0; }

// After the checks.
PISLAM_HD void ctl_begin(const Map &M, Ctl &C, int min_obs) {
  C.code = refusal(M, C, min_obs);
  C.done = C.code != 0u;
  C.evals = 0, C.ninl = 0, C.set = 0, C.round_over = 0, C.cost = 0.0, C.lambda = prf::LAMBDA_0;
  C.solves = 0, C.cg_total = 0, C.cg_last = 0, C.fails = 0, C.rejects = 0;
  ctl_next_solve(C);
}
// After the first pass.
PISLAM_HD void ctl_first(Ctl &C, const double *sums) {
  C.S[0] = sums[0], C.S[1] = sums[1], C.S[2] = sums[2];
  C.evals = 1;
}
// After the set-up of a solve: rz is the key-frame sum of r . z.
PISLAM_HD void ctl_cg_begin(Ctl &C, double rz, double cg_tol) {
  C.solves++, C.cg_last = 0;
  C.rz = rz, C.thr = (cg_tol * cg_tol) * rz;
  C.cg_live = !C.solve_fail && !(rz <= C.thr);
}
// The scalars of one PCG iteration.  alpha from pAp (false: the solve fails); then beta from the new rz.
PISLAM_HD bool ctl_cg_alpha(Ctl &C, double pAp, double *alpha) {
  C.cg_total++, C.cg_last++;
  if (!(pAp > 0.0)) {
    C.solve_fail = 1, C.cg_live = 0;
    return false;
  }
  *alpha = C.rz / pAp;
  return true;
}
PISLAM_HD double ctl_cg_beta(Ctl &C, double rz1, int cg_iters) {
  const double beta = rz1 / C.rz;
  C.rz = rz1;
  if ((int)C.cg_last >= cg_iters || rz1 <= C.thr) C.cg_live = 0;
  return beta;
}
// After the pass at the trial state (sums), or after a solve or a step that failed.
PISLAM_HD void ctl_trial(Ctl &C, const double *sums, double eps) {
  if (C.solve_fail || C.step_bad) {
    C.lambda = prf::lambda_up(C.lambda);
    C.fails++;
  } else {
    C.evals++;
    if (sums[0] < C.S[0]) {
      C.S[0] = sums[0], C.S[1] = sums[1], C.S[2] = sums[2];
      C.set ^= 1u;
      C.lambda = prf::lambda_down(C.lambda);
    } else {
      C.lambda = prf::lambda_up(C.lambda);
      C.rejects++;
    }
    if (C.dmax <= eps) C.round_over = 1;
  }
  ctl_next_solve(C);
}
// After the classifying pass of round r.
PISLAM_HD void ctl_classify(Ctl &C, const double *sums, int r, int rounds, int min_obs) {
  C.S[0] = sums[0], C.S[1] = sums[1], C.S[2] = sums[2];
  C.evals++;
  C.ninl = (uint32_t)sums[1], C.cost = sums[2];
  C.round_over = 0, C.lambda = prf::LAMBDA_0;
  ctl_next_solve(C);
  if (r + 1 == rounds) C.done = 1;
  else if (C.ninl < (uint32_t)min_obs) C.code = 1, C.done = 1;
}

// The launches of a call with these parameters (the checks, the state, the first pass and the outputs included).
inline long long launch_count(const pba::Params &p, int cg_iters) {
  long long n = 7;                             // two checks, begin, load, pass, decide; at the end the outputs
  for (int r = 0; r < p.rounds; r++) n += (long long)p.iters[r] * (6 + 3 * (long long)cg_iters) + 2;
  return n;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's serial form of the whole call for one map (the probe; never the library's hot path) -----------------

struct Result {
  uint32_t ninliers, status, solves, cg_total, fails, rejects, held;   // held: the most points held in a solve
  double cost;
};

inline double host_tree(double *p, int n) {
  for (int h = n / 2; h >= 1; h /= 2)
    for (int q = 0; q < h; q++) p[q] += p[q + h];
  return p[0];
}
inline void host_point_sums(const Map &M, double *sums) {
  static thread_local double part[3][prf::PARTIALS];
  for (int j = 0; j < 3; j++)
    for (int q = 0; q < prf::PARTIALS; q++) part[j][q] = 0.0;
  for (uint32_t p = 0; p < M.npt; p++)
    for (int j = 0; j < 3; j++) part[j][p % prf::PARTIALS] += M.ws.sub[3 * (size_t)p + j];
  for (int j = 0; j < 3; j++) sums[j] = host_tree(part[j], prf::PARTIALS);
}
template <class FN>
inline double host_kf_sum(const Map &M, const FN &fn) {
  double part[prf::PARTIALS] = {0.0};
  for (uint32_t k = 0; k < M.nk; k++)
    if (!M.fixed[k]) part[k % prf::PARTIALS] += fn(k);
  return host_tree(part, prf::PARTIALS);
}
// The 64 partials of a key frame's sums, combined by halving.
template <int SUMS, class FN>
inline void host_kf_partials(const FN &fn, double *sums) {
  static thread_local double part[SUMS][KPART];
  for (uint32_t q = 0; q < (uint32_t)KPART; q++) {
    double acc[SUMS];
    fn(q, acc);
    for (int t = 0; t < SUMS; t++) part[t][q] = acc[t];
  }
  for (int t = 0; t < SUMS; t++) sums[t] = host_tree(part[t], KPART);
}

// The whole call for one map, phase by phase as the launches run; M.ws is a slice of ws_bytes(nk, npt, n) or larger,
// M.ctl a zeroed control block.  poses_out [nk][12], xw_out [npt][3], inlier [n]; cg_log (or null) receives the PCG
// iterations of every solve begun.
inline void host_map(const Map &M, const Params &P, float *poses_out, float *xw_out, uint8_t *inlier, Result *R,
                     std::vector<uint32_t> *cg_log = nullptr) {
  Ctl &C = *M.ctl;
  R->held = 0;
  // the checks
  if (M.shaped) {
    for (uint32_t i = 0; i < M.n; i++)
      if (!obs_in_order(M, i)) C.bad3 = 1;
    for (uint32_t p = 0; p < M.npt; p++)
      if (!pt_words_ok(M, p)) C.bad2 = 1;
    for (uint32_t k = 0; k < M.nk; k++) {
      if (!kf_range_ok(M, k)) {
        C.bad3 = 1;
      } else {
        for (uint32_t j = M.kf_ptr[k]; j < M.kf_ptr[k + 1]; j++)
          if (!kf_entry_ok(M, k, j)) C.bad3 = 1;
      }
      if (!kf_words_ok(M, k)) C.bad2 = 1;
      if (!M.fixed[k]) C.any_free = 1;
    }
  }
  ctl_begin(M, C, P.ba.min_obs);
  double sums[3];
  auto pass = [&](int set, bool classify, bool robust) {
    for (uint32_t p = 0; p < M.npt; p++) pass_point(M, set, p, classify, robust, inlier);
    host_point_sums(M, sums);
  };
  if (!C.done) {
    for (uint32_t k = 0; k < M.nk; k++) load_kf(M, k);
    for (uint32_t p = 0; p <= M.npt; p++) load_pt(M, p);
    for (uint32_t i = 0; i < M.n; i++) inlier[i] = 1;
    pass((int)C.set, false, 0 < P.ba.huber_rounds);
    ctl_first(C, sums);
  }
  for (int r = 0; r < P.ba.rounds; r++) {
    for (int it = 0; it < P.ba.iters[r]; it++) {
      if (!iter_live(C)) continue;
      const int set = (int)C.set;
      const double s = 1.0 + C.lambda;
      uint32_t held = 0;
      for (uint32_t p = 0; p < M.npt; p++) point_factor(M, set, p, s), held += M.ws.held[p];
      R->held = held > R->held ? held : R->held;
      for (uint32_t k = 0; k < M.nk; k++) {
        if (M.fixed[k]) continue;
        double su[SETUP_SUMS];
        host_kf_partials<SETUP_SUMS>([&](uint32_t q, double *acc) { kf_setup_partial(M, set, k, q, acc); }, su);
        if (!kf_setup_finish(M, k, s, su)) C.solve_fail = 1;
      }
      ctl_cg_begin(C, host_kf_sum(M, [&](uint32_t k) { return M.ws.dot[k]; }), P.cg_tol);
      for (int n = 0; n < P.cg_iters; n++) {
        if (!cg_live(C)) continue;
        for (uint32_t p = 0; p < M.npt; p++) cg_point(M, set, p);
        for (uint32_t k = 0; k < M.nk; k++) {
          if (M.fixed[k]) continue;
          double su[DIM];
          host_kf_partials<DIM>([&](uint32_t q, double *acc) { kf_sp_partial(M, set, k, q, acc); }, su);
          kf_sp_finish(M, k, su);
        }
        double alpha;
        if (!ctl_cg_alpha(C, host_kf_sum(M, [&](uint32_t k) { return kf_pap(M, k); }), &alpha)) continue;
        const double beta = ctl_cg_beta(C, host_kf_sum(M, [&](uint32_t k) { return kf_update(M, k, alpha); }), P.cg_iters);
        for (uint32_t k = 0; k < M.nk; k++)
          if (!M.fixed[k]) kf_p(M, k, beta);
      }
      if (cg_log) cg_log->push_back(C.cg_last);
      if (step_live(C)) {
        double dmax = 0.0, dm;
        for (uint32_t p = 0; p < M.npt; p++) {
          if (!point_step(M, set, p, &dm)) C.step_bad = 1;
          else dmax = fmax(dmax, dm);
        }
        for (uint32_t k = 0; k < M.nk; k++) {
          if (M.fixed[k]) continue;
          if (!kf_step(M, set, k, &dm)) C.step_bad = 1;
          else dmax = fmax(dmax, dm);
        }
        C.dmax = dmax;
      }
      if (trial_live(C)) pass(set ^ 1, false, r < P.ba.huber_rounds);
      ctl_trial(C, sums, P.ba.eps);
    }
    if (!C.done) {
      pass((int)C.set, true, r + 1 < P.ba.huber_rounds);
      ctl_classify(C, sums, r, P.ba.rounds, P.ba.min_obs);
    }
  }
  // the outputs
  const bool ran = C.evals != 0;
  for (uint32_t k = 0; k < M.nk; k++)
    for (int i = 0; i < 12; i++)
      poses_out[12 * (size_t)k + i] = ran && !M.fixed[k] ? (float)M.ws.T[C.set][12 * (size_t)k + i] : M.poses[12 * (size_t)k + i];
  for (size_t i = 0; i < 3 * (size_t)M.npt; i++) xw_out[i] = ran ? (float)M.ws.X[C.set][i] : M.xw[i];
  if (!ran)
    for (uint32_t i = 0; i < M.n; i++) inlier[i] = 0;
  R->ninliers = C.ninl, R->cost = C.cost, R->status = C.code | C.evals << 8;
  R->solves = C.solves, R->cg_total = C.cg_total, R->fails = C.fails, R->rejects = C.rejects;
}
#endif

}  // namespace gba
