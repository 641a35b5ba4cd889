// pislam_ransac_math.h — what the RANSAC skeleton of pislam_two_view_ransac_batch, pislam_pnp_ransac_batch and
// pislam_sim3_ransac_batch (pislam_ransac_kernels.h: that comment describes the steps) states for the device and for a
// plain C++ compiler: the best-of key, the outcome it hands to a call's epilogue, the status word, and, for the host
// only, the skeleton run serially (prk::host_ransac, the probes under tools/probes).  A call's PROBLEM type, written
// PISLAM_HD in its *_math.h, is consumed by both forms:
//   WORDS                  the words of a hypothesis (8, 12 or 14)
//   Item, item(i)          what scoring needs of match / observation i, and how to fetch it
//   n, have                the element's clamped count; false when the element cannot have a model (both uniform)
//   hypothesis(k, rec)     hypothesis k: its WORDS words; false when invalid
//   score(rec, item, &inl) what the item adds to the integer score of rec; *inl = it is an inlier
// The best-of rule is one integer: the largest key wins, that is the largest score and, on a tie, the smallest k.
#pragma once
#include "pislam_scalar_math.h"

namespace prk {

constexpr int MAX_HYP = 1024;

// A score of 0 never competes, so a key of 0 means "no model".
PISLAM_HD unsigned long long best_key(uint32_t s, int k) {
  return ((unsigned long long)s << 10) | (unsigned long long)(MAX_HYP - 1 - k);
}
PISLAM_HD int key_hypothesis(unsigned long long key) { return MAX_HYP - 1 - (int)(key & (MAX_HYP - 1)); }
PISLAM_HD uint32_t key_score(unsigned long long key) { return (uint32_t)(key >> 10); }

// What the skeleton hands to the call's epilogue, uniform over the workgroup.  best: the winning hypothesis or -1.
struct Outcome {
  int32_t best;
  uint32_t score, ninliers, nvalid;
};

// The status word of the calls that test a camera (PnP, Sim(3)): 0 a model, 1 one with fewer than min_inliers, 2 none,
// 3 a bad camera; the count of valid hypotheses from bit 8 on.
PISLAM_HD uint32_t status(const Outcome &O, bool cam_ok, int min_inliers) {
  if (O.best >= 0) return (O.ninliers < (uint32_t)min_inliers ? 1u : 0u) | O.nvalid << 8;
  return cam_ok ? (2u | O.nvalid << 8) : 3u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host's serial form (the probes; never the library's hot path).  rec: the winning record, when there is one.
template <class PROBLEM>
inline Outcome host_ransac(const PROBLEM &P, int hypotheses, float (&rec)[PROBLEM::WORDS], uint8_t *inlier) {
  Outcome O{-1, 0, 0, 0};
  for (uint32_t i = 0; i < P.n; i++) inlier[i] = 0;
  if (!P.have) return O;
  unsigned long long best = 0;
  for (int k = 0; k < hypotheses; k++) {
    float r[PROBLEM::WORDS];
    if (!P.hypothesis((uint32_t)k, r)) continue;
    O.nvalid++;
    uint32_t s = 0;
    for (uint32_t i = 0; i < P.n; i++) {
      bool inl;
      s += P.score(r, P.item(i), &inl);
    }
    if (s && best_key(s, k) > best) {
      best = best_key(s, k);
      for (int i = 0; i < PROBLEM::WORDS; i++) rec[i] = r[i];
    }
  }
  if (!best) return O;
  for (uint32_t i = 0; i < P.n; i++) {
    bool inl;
    (void)P.score(rec, P.item(i), &inl);
    inlier[i] = inl ? 1 : 0, O.ninliers += inl ? 1u : 0u;
  }
  O.best = key_hypothesis(best), O.score = key_score(best);
  return O;
}
#endif

}  // namespace prk
