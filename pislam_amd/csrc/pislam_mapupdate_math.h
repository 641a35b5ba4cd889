// pislam_mapupdate_math.h — the rules of pislam_map_points_update_batch (include/pislam_hip.h: that comment is the
// contract), stated ONCE for the device kernels (pislam_mapupdate_kernels.h) and for a plain C++ compiler (tools/probes/
// mapupdate_host_check.cpp): when a map's lists are valid, where a point's observers lie in the list, the geometry of one
// point (mean viewing direction, reference observer, distance range), the Hamming distance, the element of a given rank
// of a row of distances without a sort, the key that picks the representative descriptor and, for the host only, the
// whole call for one map run serially.  The float operations are written out one rounding at a time; build with
// -ffp-contract=off.  The level table is only ever indexed by a loop counter, so on the device nothing goes through
// scratch.
#pragma once
#include "pislam_scalar_math.h"

namespace pmu {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_KF = 4096;                   // == the covisibility call's limit
constexpr int MAX_LEVELS = 16;
constexpr int WORDS = 8;                       // 32-bit words of a descriptor
constexpr int MAX_DIST = 32 * WORDS;           // the largest Hamming distance
constexpr int RANK_STEPS = 9;                  // halvings of [0, MAX_DIST]: 257 values

// The status of a point; of 3, 4 and 2 the first that applies.
enum PtStatus : uint8_t { OK = 0, NO_OBSERVERS = 1, REF_REPLACED = 2, GEOMETRY = 3, NO_LEVEL = 4 };

// The host table as the kernels carry it (by value: a captured graph keeps its own copy).
struct Tables {
  float level_scale[MAX_LEVELS];
  int32_t nlevels;
};

// One map of a batch as the call is given it: count, nk and npt are the words of counts[b], kf_counts[b] and
// pt_counts[b], unclamped.
struct Map {
  const int32_t *obs_pt;
  const uint16_t *obs_kf;
  const uint8_t *obs_level;
  const uint32_t *obs_desc;                    // or null
  const float *poses, *xw;
  const uint16_t *ref;                         // or null
  int64_t count, stride, nk, kf_stride, npt, pt_stride;
};

// ---- the validity of a map -------------------------------------------------------------------------------------------

PISLAM_HD bool shape_ok(const Map &M) {
  return M.count >= 0 && M.count <= M.stride && M.nk >= 0 && M.nk <= M.kf_stride && M.npt <= M.pt_stride;
}

// Observation i < count of a map whose shape is ok: its key frame and its point exist, and it comes strictly behind
// observation i - 1 in (obs_pt, obs_kf).
PISLAM_HD bool obs_ok(const Map &M, int64_t i) {
  const int32_t pt = M.obs_pt[i];
  const uint32_t kf = M.obs_kf[i];
  if (pt < 0 || (int64_t)pt >= M.npt || (int64_t)kf >= M.nk) return false;
  if (i == 0) return true;
  const int32_t pp = M.obs_pt[i - 1];
  return pp < pt || (pp == pt && (uint32_t)M.obs_kf[i - 1] < kf);
}

// The status of a map: 3 malformed, 1 nothing to do, 0 ok.
PISLAM_HD int32_t status_of(bool malformed, const Map &M) { return malformed ? 3 : ((M.npt == 0 || M.count == 0) ? 1 : 0); }

// The points of a map that the call writes: p < points_written.
PISLAM_HD int64_t points_written(const Map &M) { return M.npt < M.pt_stride ? M.npt : M.pt_stride; }

// The list index of the first observation whose point is >= p, in a valid list (ascending obs_pt): the observers of p
// are [segment_begin(p), segment_begin(p + 1)).
PISLAM_HD int32_t segment_begin(const int32_t *obs_pt, int64_t count, int64_t p) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)obs_pt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return (int32_t)lo;
}

// ---- the geometry of one point ---------------------------------------------------------------------------------------

// Entry l < nlevels of the table, without a variable index.
PISLAM_HD float pick(const Tables &tab, int l) {
  float v = tab.level_scale[0];
  for (int k = 1; k < MAX_LEVELS; k++) v = (k < tab.nlevels && k == l) ? tab.level_scale[k] : v;
  return v;
}

struct Geo {
  uint8_t status;                              // OK, REF_REPLACED, GEOMETRY or NO_LEVEL
  float normal[3], drange[2];
};

// Point p of a valid map with its n >= 1 observers at [first, first + n).
PISLAM_HD Geo geometry(const Map &M, const Tables &tab, int64_t p, int64_t first, int64_t n) {
  Geo g{OK, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f}};
  const float X0 = M.xw[3 * p], X1 = M.xw[3 * p + 1], X2 = M.xw[3 * p + 2];
  bool bad = !(finite_f(X0) && finite_f(X1) && finite_f(X2));
  const uint32_t want = M.ref ? (uint32_t)M.ref[p] : 0u;
  bool found = !M.ref;                         // without ref the first observer is the reference
  float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, dr = 0.0f;
  int lr = 0;
  for (int64_t i = 0; i < n; i++) {
    const uint32_t kf = M.obs_kf[first + i];
    const float *P = M.poses + 12 * (size_t)kf;
    float R[9], t[3];
PISLAM_UNROLL
    for (int k = 0; k < 9; k++) R[k] = P[k], bad = bad || !finite_f(R[k]);
PISLAM_UNROLL
    for (int k = 0; k < 3; k++) t[k] = P[9 + k], bad = bad || !finite_f(t[k]);
    const float O0 = -((R[0] * t[0] + R[3] * t[1]) + R[6] * t[2]);
    const float O1 = -((R[1] * t[0] + R[4] * t[1]) + R[7] * t[2]);
    const float O2 = -((R[2] * t[0] + R[5] * t[1]) + R[8] * t[2]);
    const float e0 = X0 - O0, e1 = X1 - O1, e2 = X2 - O2;
    const float d = fsqrt((e0 * e0 + e1 * e1) + e2 * e2);
    bad = bad || d == 0.0f;
    const float u0 = fdiv(e0, d), u1 = fdiv(e1, d), u2 = fdiv(e2, d);
    if (i == 0) w0 = u0, w1 = u1, w2 = u2;
    else w0 = w0 + u0, w1 = w1 + u1, w2 = w2 + u2;
    const bool is_ref = M.ref ? (!found && kf == want) : i == 0;
    if (i == 0 || is_ref) dr = d, lr = (int)M.obs_level[first + i];
    found = found || is_ref;
  }
  const float wn = fsqrt((w0 * w0 + w1 * w1) + w2 * w2);
  bad = bad || wn == 0.0f;
  const float n0 = fdiv(w0, wn), n1 = fdiv(w1, wn), n2 = fdiv(w2, wn);
  bad = bad || !(finite_f(n0) && finite_f(n1) && finite_f(n2));
  const bool level_ok = lr < tab.nlevels;
  const float r = dr * pick(tab, lr);
  const float lo = fdiv(r, pick(tab, tab.nlevels - 1));
  bad = bad || (level_ok && !(finite_f(r) && finite_f(lo)));
  if (bad) {
    g.status = GEOMETRY;
    return g;
  }
  g.normal[0] = n0, g.normal[1] = n1, g.normal[2] = n2;
  if (level_ok) g.drange[0] = lo, g.drange[1] = r;
  g.status = !level_ok ? NO_LEVEL : (found ? OK : REF_REPLACED);
  return g;
}

// ---- the representative descriptor ---------------------------------------------------------------------------------------

PISLAM_HD uint32_t hamming(const uint32_t *a, const uint32_t *b) {
  uint32_t d = 0;
PISLAM_UNROLL
  for (int k = 0; k < WORDS; k++) d += (uint32_t)__builtin_popcount(a[k] ^ b[k]);
  return d;
}

// The index of the median of a row of n distances sorted ascending (ORB-SLAM's vDists[0.5*(N-1)]).
PISLAM_HD uint32_t median_rank(uint32_t n) { return (n - 1u) >> 1; }

// The element with index k < n of the row dist(0) .. dist(n - 1) sorted ascending, without a sort: the smallest value v
// in [0, MAX_DIST] with at least k + 1 elements <= v, by RANK_STEPS halvings with one count each.  (Once lo == hi the
// count at lo passes, so the surplus steps change nothing: every row takes the same number of steps.)
template <class ROW>
PISLAM_HD uint32_t rank_select(uint32_t n, uint32_t k, const ROW &dist) {
  uint32_t lo = 0, hi = MAX_DIST;
  for (int s = 0; s < RANK_STEPS; s++) {
    const uint32_t mid = (lo + hi) >> 1;
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < n; j++) cnt += dist(j) <= mid ? 1u : 0u;
    const bool enough = cnt >= k + 1u;
    hi = enough ? mid : hi;
    lo = enough ? lo : mid + 1u;
  }
  return lo;
}

// "The smallest median, the first observer on a tie" as a minimum: the key of observer i < 4096 with median med.
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;
PISLAM_HD uint32_t choice_key(uint32_t med, uint32_t i) { return (med << 12) | i; }
PISLAM_HD uint32_t key_observer(uint32_t key) { return key & 0xFFFu; }

}  // namespace pmu

#if !defined(__HIPCC__)
// ---- the host only: the whole call for one map, serially -----------------------------------------------------------------
namespace pmu {

// Outputs as the call's rows of one map (normal, drange, desc and first may be null); what the call does not write keeps
// what it held.
inline void host_map(const Map &M, const Tables &tab, float *normal, float *drange, uint32_t *desc, int32_t *nobs,
                     int32_t *first, uint8_t *pt_status, int32_t *status) {
  bool bad = !shape_ok(M);
  if (!bad)
    for (int64_t i = 0; i < M.count; i++) bad = bad || !obs_ok(M, i);
  *status = status_of(bad, M);
  const int64_t npw = points_written(M);
  for (int64_t p = 0; p < npw; p++) {
    nobs[p] = 0, pt_status[p] = NO_OBSERVERS;
    if (first) first[p] = -1;
    if (*status != 0) continue;
    const int32_t f = segment_begin(M.obs_pt, M.count, p), n = segment_begin(M.obs_pt, M.count, p + 1) - f;
    nobs[p] = n;
    if (n == 0) continue;
    if (first) first[p] = f;
    const Geo g = geometry(M, tab, p, f, n);
    pt_status[p] = g.status;
    for (int k = 0; k < 3 && normal; k++) normal[3 * p + k] = g.normal[k];
    for (int k = 0; k < 2 && drange; k++) drange[2 * p + k] = g.drange[k];
    if (!desc) continue;
    const uint32_t *D = M.obs_desc + (size_t)f * WORDS;
    uint32_t best = KEY_NONE;
    for (int32_t i = 0; i < n; i++) {
      const uint32_t *own = D + (size_t)i * WORDS;
      const uint32_t med = rank_select((uint32_t)n, median_rank((uint32_t)n),
                                       [&](uint32_t j) { return hamming(own, D + (size_t)j * WORDS); });
      const uint32_t key = choice_key(med, (uint32_t)i);
      best = key < best ? key : best;
    }
    for (int k = 0; k < WORDS; k++) desc[(size_t)p * WORDS + k] = D[(size_t)key_observer(best) * WORDS + k];
  }
}

}  // namespace pmu
#endif
