// pislam_covis_math.h — the rules of pislam_covisibility_batch (include/pislam_hip.h: that comment is the contract),
// stated ONCE for the device kernels (pislam_covis_kernels.h) and for a plain C++ compiler (tools/probes/
// covis_host_check.cpp): when a list of observations is valid, what one observation adds to the weight matrix and to
// the culling statistic, when a key frame qualifies as a neighbour and the fallback, the sort key of a neighbour row,
// the parent rule, the redundancy predicate, the workspace of a batch and, for the host only, the whole call for one map
// run serially.  Everything is integer arithmetic: nothing here rounds.
#pragma once
#include "pislam_scalar_math.h"

namespace pcv {

constexpr int MAX_KF = 4096;                   // == the pose graph's vertex limit
constexpr uint16_t NO_PARENT = 0xFFFF;
constexpr uint64_t KEY_PAD = ~0ull;            // sorts behind every key of a neighbour (a neighbour's weight is >= 1)

struct Params {
  int32_t min_weight, cull_min_observers, cull_level_slack;
};

// One map of a batch as the call is given it: count and nk are the words of counts[b] and kf_counts[b], unclamped.
struct Map {
  const int32_t *obs_pt;
  const uint16_t *obs_kf;
  const uint8_t *obs_level, *cull_mask;        // or null
  int64_t count, stride, nk, kf_stride;
};

// ---- the validity of a list ------------------------------------------------------------------------------------------

PISLAM_HD bool shape_ok(const Map &M) { return M.count >= 0 && M.count <= M.stride && M.nk >= 0 && M.nk <= M.kf_stride; }

// Observation i < count of a map whose shape is ok: its key frame exists, its point is not negative, and it comes
// strictly behind observation i - 1 in (obs_pt, obs_kf).
PISLAM_HD bool obs_ok(const Map &M, int64_t i) {
  const int32_t pt = M.obs_pt[i];
  const uint32_t kf = M.obs_kf[i];
  if (pt < 0 || (int64_t)kf >= M.nk) return false;
  if (i == 0) return true;
  const int32_t pp = M.obs_pt[i - 1];
  return pp < pt || (pp == pt && (uint32_t)M.obs_kf[i - 1] < kf);
}

// ---- the culling statistic -------------------------------------------------------------------------------------------

PISLAM_HD int32_t level_of(const Map &M, int64_t i) { return M.obs_level ? (int32_t)M.obs_level[i] : 0; }
PISLAM_HD bool is_subject(const Map &M, int64_t i) { return !M.cull_mask || M.cull_mask[i] != 0; }
// Observer o of a point counts for the subject `own` of the same point (ORB-SLAM: scaleLeveli <= scaleLevel + 1).
PISLAM_HD bool observer_counts(int32_t level_o, int32_t level_own, int32_t slack) { return level_o <= level_own + slack; }
PISLAM_HD bool is_redundant(int32_t observers, int32_t min_observers) { return observers >= min_observers; }

// What observation i of a valid prefix adds: 1 to W[kf_i][kf_j] and W[kf_j][kf_i] for every LATER observation j of the
// same point (so every pair of a point is added once, by its earlier member), 1 to pts[kf_i] if i is a subject and 1 to
// red[kf_i] if enough of the point's other observers count.  The caller has checked obs_ok(M, i).  The walks stop where
// the key frames stop ascending, so a malformed list costs at most nk steps each way and indexes nothing outside the
// matrix: such a map is flagged by the thread of the offending observation and its matrix is never read.
template <class ADD>
PISLAM_HD void count_obs(const Map &M, const Params &P, int64_t i, uint32_t *W, uint32_t *pts, uint32_t *red,
                         const ADD &add) {
  const int32_t pt = M.obs_pt[i], own = level_of(M, i);
  const uint32_t k = M.obs_kf[i];
  const size_t ks = (size_t)M.kf_stride;
  const bool subject = is_subject(M, i);
  int32_t others = 0;
  uint32_t last = k;
  for (int64_t j = i + 1; j < M.count && M.obs_pt[j] == pt; j++) {
    const uint32_t kj = M.obs_kf[j];
    if (kj <= last || (int64_t)kj >= M.nk) break;
    last = kj;
    add(&W[(size_t)k * ks + kj]);
    add(&W[(size_t)kj * ks + k]);
    others += observer_counts(level_of(M, j), own, P.cull_level_slack) ? 1 : 0;
  }
  if (!subject) return;
  last = k;
  for (int64_t j = i - 1; j >= 0 && M.obs_pt[j] == pt; j--) {
    const uint32_t kj = M.obs_kf[j];
    if (kj >= last) break;
    last = kj;
    others += observer_counts(level_of(M, j), own, P.cull_level_slack) ? 1 : 0;
  }
  add(&pts[k]);
  if (is_redundant(others, P.cull_min_observers)) add(&red[k]);
}

// ---- a key frame's row -----------------------------------------------------------------------------------------------

PISLAM_HD bool qualifies(uint32_t w, int32_t min_weight) { return w >= (uint32_t)min_weight; }

// Ascending keys are a row's order: weight descending, index ascending on equal weight.  The weight keeps its 32 bits.
PISLAM_HD uint64_t sort_key(uint32_t w, uint32_t j) { return ((uint64_t)(~w) << 16) | j; }
PISLAM_HD uint16_t key_index(uint64_t key) { return (uint16_t)(key & 0xFFFFu); }
PISLAM_HD int32_t key_weight(uint64_t key) { return (int32_t)~(uint32_t)(key >> 16); }

// "The largest weight, the smallest index on a tie" as a maximum: the pick of (w > 0, j); 0 is "none".  The parent of k
// is the largest pick over j < k, the fallback neighbour the largest pick over j != k.
PISLAM_HD uint64_t pick_of(uint32_t w, uint32_t j) { return ((uint64_t)w << 16) | (0xFFFFu - j); }
PISLAM_HD uint32_t pick_index(uint64_t pick) { return 0xFFFFu - (uint32_t)(pick & 0xFFFFu); }
PISLAM_HD uint32_t pick_weight(uint64_t pick) { return (uint32_t)(pick >> 16); }
PISLAM_HD bool parent_candidate(uint32_t w, uint32_t j, uint32_t k) { return w > 0 && j < k; }
PISLAM_HD bool fallback_candidate(uint32_t w, uint32_t j, uint32_t k) { return w > 0 && j != k; }

// The status of a map: 3 malformed, 1 nothing to do, 0 ok.
PISLAM_HD int32_t status_of(bool malformed, const Map &M) { return malformed ? 3 : ((M.nk == 0 || M.count == 0) ? 1 : 0); }

// ---- the workspace of a batch: W [batch][ks][ks], pts [batch][ks], red [batch][ks], bad [batch], all uint32 --------------

struct Ws {
  uint32_t *W, *pts, *red, *bad;
};
PISLAM_HD size_t ws_bytes(size_t kf_stride, size_t batch) { return 4 * batch * (kf_stride * kf_stride + 2 * kf_stride + 1); }
PISLAM_HD void ws_carve(void *base, size_t kf_stride, size_t batch, Ws *ws) {
  ws->W = (uint32_t *)base;
  ws->pts = ws->W + batch * kf_stride * kf_stride;
  ws->red = ws->pts + batch * kf_stride;
  ws->bad = ws->red + batch * kf_stride;
}

}  // namespace pcv

#if !defined(__HIPCC__)
// ---- the host only: the whole call for one map, serially -----------------------------------------------------------------
#include <algorithm>
#include <vector>

namespace pcv {

// Outputs as the call's rows of one map; nb_idx and nb_weight [kf_stride][nb_stride] keep what they held where the call
// does not write.
inline void host_map(const Map &M, const Params &P, size_t nb_stride, uint16_t *nb_idx, int32_t *nb_weight,
                     int32_t *nb_count, uint16_t *parent, int32_t *kf_points, int32_t *kf_redundant, int32_t *status) {
  const size_t ks = (size_t)M.kf_stride;
  std::vector<uint32_t> W(ks * ks, 0u), pts(ks, 0u), red(ks, 0u);
  bool bad = !shape_ok(M);
  if (!bad) {
    const auto add = [](uint32_t *p) { *p += 1; };
    for (int64_t i = 0; i < M.count; i++) {
      if (!obs_ok(M, i)) {
        bad = true;
        continue;
      }
      count_obs(M, P, i, W.data(), pts.data(), red.data(), add);
    }
  }
  *status = status_of(bad, M);
  std::vector<uint64_t> keys;
  for (size_t k = 0; k < ks; k++) {
    nb_count[k] = 0, parent[k] = NO_PARENT, kf_points[k] = 0, kf_redundant[k] = 0;
    if (*status != 0 || (int64_t)k >= M.nk) continue;
    uint64_t par = 0, fb = 0;
    keys.clear();
    for (uint32_t j = 0; j < (uint32_t)M.nk; j++) {
      const uint32_t w = j == k ? 0u : W[k * ks + j];
      if (parent_candidate(w, j, (uint32_t)k)) par = std::max(par, pick_of(w, j));
      if (fallback_candidate(w, j, (uint32_t)k)) fb = std::max(fb, pick_of(w, j));
      if (w > 0 && qualifies(w, P.min_weight)) keys.push_back(sort_key(w, j));
    }
    if (keys.empty() && fb) keys.push_back(sort_key(pick_weight(fb), pick_index(fb)));
    std::sort(keys.begin(), keys.end());
    for (size_t r = 0; r < keys.size() && r < nb_stride; r++)
      nb_idx[k * nb_stride + r] = key_index(keys[r]), nb_weight[k * nb_stride + r] = key_weight(keys[r]);
    nb_count[k] = (int32_t)keys.size();
    parent[k] = par ? (uint16_t)pick_index(par) : NO_PARENT;
    kf_points[k] = (int32_t)pts[k], kf_redundant[k] = (int32_t)red[k];
  }
}

}  // namespace pcv
#endif
