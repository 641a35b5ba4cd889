// Map-point search by projection (include/pislam_hip.h: pislam_match_projection_batch), after
// ORB-SLAM's ORBmatcher::SearchByProjection, and map-point fusion search (pislam_match_fuse_batch), after
// ORBmatcher::Fuse.  The train side is the scaled window matcher's: pm::k_scaled_index sorts the frame's keypoints into
// per-level cell grids in level-0 pixels.  The query side is new: a query is a 3D map point, not a keypoint.
//   k_match_projection   WIN_LPQ lanes per map point; blockIdx.y is the frame, so its pose and camera are wave-uniform
//                        loads.  Every lane of a query projects the point itself (pislam_project_math.h: a few dozen VALU
//                        operations, no shuffle, the same bits in all four lanes), then the wave-uniform loop over the
//                        plan's levels of k_match_scaled<.., false> walks the levels pl - level_below .. pl + level_above
//                        with the radius of the PREDICTED level and the viewing angle (pm::win_walk, pm::pair_push,
//                        pm::pair_merge_lanes).  For second_same_level the levels of the two winners are looked up from
//                        the caller's keypoint words afterwards (two loads in one lane of four).
//   k_match_fuse         the same body (match_projection<WORDS, true>) with a query mask and, per entry inside the integer
//                        window, the reprojection test pjm::fuse_ok before the popcount: the keypoint's (u, v, u_right)
//                        is gathered from the caller's tobs_q8 by the train index the entry carries (12 bytes, only for
//                        entries that passed the window test); inv_sigma2 of the level walked comes from the by-value
//                        table under the uniform level counter, the two bounds are kernel arguments.
// The level tables travel as kernel arguments and are indexed by uniform loop counters only.
#pragma once
#include "pislam_match_kernels.h"
#include "pislam_project_math.h"

namespace pj {

struct ProjArgs {
  const float *pose, *cam, *xw, *normal, *drange;        // normal / drange null: see pjm::project
  const uint8_t *qlevel;                                 // null in map mode
  const uint32_t *qdesc, *qcount, *tkp;
  size_t q_stride, t_stride;                             // in entries
  const uint32_t *cell_off;                              // pm::k_scaled_index's outputs
  const uint2 *ent_meta;
  const uint32_t *ent_desc;
  int32_t *idx;
  uint32_t *dist, *dist2;
  int32_t *pred;                                         // [batch][q_stride][2] or null
  uint8_t *plevel;                                       // [batch][q_stride] or null
};

// What the fuse call adds (by value: a captured graph keeps its own copy of the table and the bounds).
struct FuseArgs {
  const int32_t *tobs;                                   // [batch][t_stride][3]: u, v, u_right (Q8; pq::MONO: monocular)
  const uint8_t *qmask;                                  // [batch][q_stride] or null
  float inv_sigma2[pjm::MAX_LEVELS];
  float chi2_mono, chi2_stereo;
};

// The body of both kernels.  FUSE false: fz is never read.
template <int WORDS, bool FUSE>
__device__ __forceinline__ void match_projection(const pm::ScaledPlan P, const pjm::Tables tab, const pjm::Params prm,
                                                 const ProjArgs a, const FuseArgs fz) {
  const int b = blockIdx.y;
  const uint32_t nq = pm::win_count(a.qcount[b], a.q_stride);
  const uint32_t sub = threadIdx.x % pm::WIN_LPQ;
  const uint32_t *off_b = a.cell_off + (size_t)b * (P.ncells + 1);
  const uint2 *mp = a.ent_meta + (size_t)b * a.t_stride;
  const uint32_t *ep = a.ent_desc + (size_t)b * a.t_stride * WORDS;
  const uint32_t *kp = a.tkp + (size_t)b * a.t_stride;
  const int32_t *ob = nullptr;
  if constexpr (FUSE) ob = fz.tobs + (size_t)b * a.t_stride * 3;
  float T[12], C[5];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = a.pose[(size_t)b * 12 + k];
#pragma unroll
  for (int k = 0; k < 5; k++) C[k] = a.cam[(size_t)b * 5 + k];
  const bool frame = pjm::frame_ok(T, C);
  for (uint32_t q0 = blockIdx.x * (uint32_t)pm::WIN_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)pm::WIN_QPW) {
    const uint32_t i = q0 + threadIdx.x / pm::WIN_LPQ;
    const size_t o = (size_t)b * a.q_stride + i;
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    pjm::Query q{false, false, 0, 0, pjm::DEAD_LEVEL, 0};
    pjm::Pixel px{0.0f, 0.0f, 0.0f};
    const uint32_t *qp = nullptr;
    bool take = frame && i < nq;
    if constexpr (FUSE) take = take && (!fz.qmask || fz.qmask[o] != 0);
    if (take) {
      q = pjm::project(T, C, a.xw + o * 3, a.normal ? a.normal + o * 3 : nullptr, a.drange ? a.drange + o * 2 : nullptr,
                       a.qlevel ? (int)a.qlevel[o] : -1, tab, prm, FUSE ? &px : nullptr);
      if (q.live) qp = a.qdesc + o * WORDS;
    }
    uint32_t qd[WORDS];
    pm::load_query<WORDS>(qd, qp);
    const int32_t xc = q.xc, yc = q.yc, r = q.r;
    float wl = 0.0f;                                    // FUSE: inv_sigma2 of the level being walked (wave-uniform)
    auto visit = [&](uint32_t e, uint2 m) {
      const int32_t tx = (int32_t)(m.x >> 16), ty = (int32_t)(m.x & 0xffffu);
      if (abs(tx - xc) <= r && abs(ty - yc) <= r) {
        if constexpr (FUSE) {                           // geometry before the popcount: m.y < t_stride <= 65535
          const int32_t *t = ob + m.y * 3u;
          if (!pjm::fuse_ok(px, t[0], t[1], t[2], wl, fz.chi2_mono, fz.chi2_stereo)) return;
        }
        pm::pair_push(best, second, (pm::win_popc<WORDS>(qd, ep + (size_t)e * WORDS) << 16) | m.y);
      }
    };
    for (int l = 0; l < P.nlevels; l++) {               // wave-uniform: the level's fields are kernel-argument loads
      if (!q.live || l < q.pl - prm.level_below || l > q.pl + prm.level_above) continue;
      if constexpr (FUSE) wl = fz.inv_sigma2[l];
      pm::win_walk(P.lv[l], off_b, mp, sub, xc - r, xc + r, yc - r, yc + r, visit);
    }
    pm::pair_merge_lanes<pm::WIN_LPQ>(best, second);
    if (sub == 0 && i < nq) {
      if (prm.second_same_level && second != 0xffffffffu) {   // (both winners were indexed: each lies in a level)
        const uint32_t k1 = kp[best & 0xffffu], k2 = kp[second & 0xffffu];
        const int32_t l1 = pm::sc_level(P, (int32_t)((k1 >> 12) & 0xfffu), (int32_t)(k1 & 0xfffu)).level;
        const int32_t l2 = pm::sc_level(P, (int32_t)((k2 >> 12) & 0xfffu), (int32_t)(k2 & 0xfffu)).level;
        if (l1 != l2) second = 0xffffffffu;
      }
      pm::store_match(o, best, second, a.idx, a.dist, a.dist2);
      if (a.pred) a.pred[o * 2] = xc, a.pred[o * 2 + 1] = yc;
      if (a.plevel) a.plevel[o] = (uint8_t)q.pl;
    }
  }
}

// grid (query tiles, batch), WIN_THREADS threads.
template <int WORDS>
__global__ __launch_bounds__(pm::WIN_THREADS) void k_match_projection(pm::ScaledPlan P, pjm::Tables tab, pjm::Params prm,
                                                                      ProjArgs a) {
  match_projection<WORDS, false>(P, tab, prm, a, FuseArgs{});
}

template <int WORDS>
__global__ __launch_bounds__(pm::WIN_THREADS) void k_match_fuse(pm::ScaledPlan P, pjm::Tables tab, pjm::Params prm,
                                                                ProjArgs a, FuseArgs fz) {
  match_projection<WORDS, true>(P, tab, prm, a, fz);
}

}  // namespace pj
