// Epipolar search between two key frames (include/pislam_hip.h:
// pislam_match_hamming_epipolar_batch), after ORB-SLAM's ORBmatcher::SearchForTriangulation: the word-guided matcher
// (pislam_bow_kernels.h) with a geometric test on every candidate.  Two kernels, siblings of pb::k_bow_index and
// pb::k_match_bow:
//   k_epi_index        one workgroup per pair: pm::lds_counting_sort with the train entry's group id as the bin.  An entry
//                      whose mask byte is 0 or whose level is not in the tables is not indexed at all.  The scatter
//                      carries the entry's geometry next to its descriptor: 12 bytes, the index with the level and the
//                      monocular flag in one dword, u and v as the floats the test reads (the 8 bytes of two packed
//                      integers would have to be unpacked and converted per candidate; the index needs 16 bits of its
//                      own either way).
//   k_match_epipolar   pm::WIN_LPQ lanes per query walking the one run of its group.  The pair's fundamental matrix and
//                      epipole are wave-uniform loads; the query's line (a, b, c, den) is computed once, in registers, by
//                      every lane of the query (the same bits in all four).  The per-level bounds chi2 * level_sigma2[l]
//                      and epipole_r2 * level_scale[l] are made once per workgroup into LDS, where a lane reads the pair
//                      of its candidate's level.  A candidate's geometry is tested first and the descriptor of an entry
//                      that passes is the only one read (the other order was measured: DESIGN.md).
#pragma once
#include "pislam_epipolar_math.h"
#include "pislam_match_kernels.h"

namespace pe {

constexpr int EPI_MAX_GROUPS = pm::WIN_MAX_CELLS;    // LDS histogram of k_epi_index

struct Ent {                                         // a train entry of the index
  uint32_t tag;                                      // index | level << 16 | monocular << 24
  float u, v;
};
static_assert(sizeof(Ent) == 12, "the workspace is sized for 12 bytes per entry");

struct EpiArgs {
  uint32_t ngroups;
  const uint32_t *qdesc, *qgroup, *qcount;
  const int32_t *qobs;
  const uint8_t *qlevel, *qmask;                     // qmask / tmask may be null
  const uint32_t *tdesc, *tgroup, *tcount;
  const int32_t *tobs;
  const uint8_t *tlevel, *tmask;
  const float *f12, *epipole;
  size_t q_stride, t_stride;
  uint32_t *grp_off;                                 // the workspace
  Ent *ent;
  uint32_t *ent_desc;
  int32_t *idx;
  uint32_t *dist, *dist2;
};

// grid (batch), pm::WIN_INDEX_THREADS threads.
__global__ __launch_bounds__(pm::WIN_INDEX_THREADS) void k_epi_index(int words, int nlevels, EpiArgs a) {
  __shared__ uint32_t hist[EPI_MAX_GROUPS];
  __shared__ uint32_t wave_sum[pm::WIN_INDEX_THREADS / 64];
  const int b = blockIdx.x;
  const size_t row = (size_t)b * a.t_stride;
  const uint32_t *gp = a.tgroup + row;
  const uint32_t *dp = a.tdesc + row * words;
  const int32_t *op = a.tobs + row * 3;
  const uint8_t *lp = a.tlevel + row, *mp = a.tmask ? a.tmask + row : nullptr;
  Ent *ip = a.ent + row;
  uint32_t *ep = a.ent_desc + row * words;
  pm::lds_counting_sort<pm::WIN_INDEX_THREADS>(
      a.ngroups, pm::win_count(a.tcount[b], a.t_stride), hist, wave_sum, a.grp_off + (size_t)b * (a.ngroups + 1),
      [&](uint32_t j) {
        const uint32_t g = gp[j];
        return g < a.ngroups && (int)lp[j] < nlevels && (!mp || mp[j]) ? (int32_t)g : -1;
      },
      [&](uint32_t slot, uint32_t j) {
        Ent e;
        e.tag = j | (uint32_t)lp[j] << 16 | (pem::mono(op[3 * (size_t)j + 2]) ? 1u << 24 : 0u);
        e.u = pem::px(op[3 * (size_t)j]), e.v = pem::px(op[3 * (size_t)j + 1]);
        ip[slot] = e;
        for (int w = 0; w < words; w++) ep[(size_t)slot * words + w] = dp[(size_t)j * words + w];
      });
}

// grid (query tiles, batch), pm::WIN_THREADS threads; outputs [batch][q_stride].
template <int WORDS>
__global__ __launch_bounds__(pm::WIN_THREADS) void k_match_epipolar(pem::Tables tab, pem::Params prm, EpiArgs a) {
  __shared__ float s_line[pem::MAX_LEVELS], s_disc[pem::MAX_LEVELS];
  const int b = blockIdx.y;
  if (threadIdx.x == 0)
    for (int l = 0; l < tab.nlevels; l++) s_line[l] = pem::line_bound(prm, tab, l), s_disc[l] = pem::disc_bound(prm, tab, l);
  __syncthreads();
  const uint32_t nq = pm::win_count(a.qcount[b], a.q_stride);
  const uint32_t sub = threadIdx.x % pm::WIN_LPQ;
  const uint32_t *off = a.grp_off + (size_t)b * (a.ngroups + 1);
  const Ent *ip = a.ent + (size_t)b * a.t_stride;
  const uint32_t *ep = a.ent_desc + (size_t)b * a.t_stride * WORDS;
  float F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = a.f12[(size_t)b * 9 + k];
  const float ex = a.epipole[(size_t)b * 2], ey = a.epipole[(size_t)b * 2 + 1];
  const bool pair_ok = pem::f_ok(F);
  for (uint32_t q0 = blockIdx.x * (uint32_t)pm::WIN_QPW; q0 < nq; q0 += gridDim.x * (uint32_t)pm::WIN_QPW) {
    const uint32_t i = q0 + threadIdx.x / pm::WIN_LPQ;
    const size_t o = (size_t)b * a.q_stride + i;
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    uint32_t e = 0, e1 = 0;                             // the run of the query's group (empty: no part in the match)
    const uint32_t *qp = nullptr;
    pem::Line ln{0.0f, 0.0f, 0.0f, 0.0f};
    bool qmono = false;
    if (pair_ok && i < nq) {
      const uint32_t g = a.qgroup[o];
      if (g < a.ngroups && (int)a.qlevel[o] < tab.nlevels && (!a.qmask || a.qmask[o])) {
        e = off[g] + sub, e1 = off[g + 1];
        qp = a.qdesc + o * WORDS;
        ln = pem::line(F, pem::px(a.qobs[3 * o]), pem::px(a.qobs[3 * o + 1]));
        qmono = pem::mono(a.qobs[3 * o + 2]);
      }
    }
    uint32_t qd[WORDS];
    pm::load_query<WORDS>(qd, qp);
    for (; e < e1; e += pm::WIN_LPQ) {
      const Ent t = ip[e];
      const uint32_t lt = t.tag >> 16 & 0xffu;          // < nlevels: the index holds no other entry
      if (pem::candidate(ln, qmono, ex, ey, t.u, t.v, (t.tag >> 24 & 1u) != 0, s_line[lt], s_disc[lt]))
        pm::pair_push(best, second, (pm::win_popc<WORDS>(qd, ep + (size_t)e * WORDS) << 16) | (t.tag & 0xffffu));
    }
    pm::pair_merge_lanes<pm::WIN_LPQ>(best, second);
    if (sub == 0 && i < nq) pm::store_match(o, best, second, a.idx, a.dist, a.dist2);
  }
}

}  // namespace pe
