// pislam_project_math.h — the query-side arithmetic of pislam_match_projection_batch (include/pislam_hip.h: that comment
// is the contract), stated ONCE for the device kernel (pislam_project_kernels.h) and for a plain C++ compiler
// (tools/probes/project_host_check.cpp): the frame test, the projection of a map point through the pose (the pose call's
// monocular arithmetic, pnm::chi2_at), the image bounds and the window centre, the distance and viewing-angle tests, the
// predicted level and the radius; and, for pislam_match_fuse_batch (tools/probes/fuse_host_check.cpp), the reprojection
// test of one candidate keypoint (fuse_ok).  Every operation is written out one rounding at a time; build with
// -ffp-contract=off.
// The level tables are only ever indexed by the counter of a loop over the levels (uniform across a wave: scalar loads of
// kernel arguments), the entry of a query's own level is picked by a select, so on the device nothing goes through
// scratch.
#pragma once
#include "pislam_pnp_math.h"

namespace pjm {

using psm::fdiv;
using psm::finite_f;
using psm::fsqrt;

constexpr int MAX_LEVELS = 16;
constexpr float Z_MIN = pq::Z_MIN;             // 2^-10, the pose call's
constexpr float BOUND_LIMIT = 1048576.0f;      // the image bounds lie within +- 2^20
constexpr int32_t MAX_RADIUS = 65535;
constexpr uint8_t DEAD_LEVEL = 0xff;           // plevel of a dead query

// The host tables and the parameter struct as the kernel carries them (by value: a captured graph keeps its own copy).
struct Tables {
  float level_scale[MAX_LEVELS];
  int32_t radius_far[MAX_LEVELS], radius_near[MAX_LEVELS];   // (radius_near NULL: a copy of radius_far)
  int32_t nlevels;
};
struct Params {
  float min_x, max_x, min_y, max_y, cos_min, cos_near;
  int32_t level_below, level_above, second_same_level;
};

// A frame is live when its 12 pose words are finite and its camera passes the absolute-pose call's test.
PISLAM_HD bool frame_ok(const float *pose, const float *cam) {
  bool ok = pnm::cam_ok(cam);
PISLAM_UNROLL
  for (int i = 0; i < 12; i++) ok = ok && finite_f(pose[i]);
  return ok;
}

// What the match needs of a query.  Dead: xc = yc = 0, pl = DEAD_LEVEL, r = 0, near false.
struct Query {
  bool live, near;
  int32_t xc, yc, pl, r;
};

// The unrounded projection of a live query, for the fuse call's reprojection test: pu, pv and pur = pu - bf * iz.
struct Pixel {
  float pu, pv, pur;
};

// Steps 1-6 of the contract for one map point of a live frame.  T: the pose (r0..r8 row-major, then t), cam: fx, fy,
// cx, cy (bf is read only when pix is given), xw: the point. Map mode: drange = (dmin, dmax), normal or null, qlevel < 0.
// Level mode: drange and normal null, qlevel = the query's level (0..255).  pix (optional): the pixel of a query that
// passed steps 1-2, unwritten otherwise.
PISLAM_HD Query project(const float (&T)[12], const float (&cam)[5], const float *xw, const float *normal,
                        const float *drange, int qlevel, const Tables &tab, const Params &p, Pixel *pix = nullptr) {
  Query q{false, false, 0, 0, DEAD_LEVEL, 0};
  const float X = xw[0], Y = xw[1], Z = xw[2];
  // 1. the camera point and its pixel
  const float x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9];
  const float y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10];
  const float z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11];
  bool live = z >= Z_MIN;
  const float iz = fdiv(1.0f, z);
  const float px = x * iz, py = y * iz;
  const float pu = cam[0] * px + cam[2], pv = cam[1] * py + cam[3];
  // 2. the image bounds (every comparison is false for a NaN) and the window centre
  live = live & (pu >= p.min_x) & (pu <= p.max_x) & (pv >= p.min_y) & (pv <= p.max_y);
  if (!live) return q;
  if (pix) *pix = Pixel{pu, pv, pu - cam[4] * iz};
  const int32_t xc = (int32_t)floorf(pu + 0.5f), yc = (int32_t)floorf(pv + 0.5f);   // |pu|, |pv| <= 2^20: no overflow
  int32_t pl = 0;
  bool near = false;
  if (drange) {
    // 3. the distance
    const float dmin = drange[0], dmax = drange[1];
    const float d = fsqrt((x * x + y * y) + z * z);
    live = (dmin <= d) & (d <= dmax);
    // 4. the viewing angle
    if (normal) {
      const float n0 = normal[0], n1 = normal[1], n2 = normal[2];
      const float nc0 = (T[0] * n0 + T[1] * n1) + T[2] * n2;
      const float nc1 = (T[3] * n0 + T[4] * n1) + T[5] * n2;
      const float nc2 = (T[6] * n0 + T[7] * n1) + T[8] * n2;
      const float c = (x * nc0 + y * nc1) + z * nc2;
      live = live & (c >= p.cos_min * d);
      near = c > p.cos_near * d;
    }
    // 5. the predicted level: the levels l below the last with d * level_scale[l] < dmax
    for (int l = 0; l < tab.nlevels - 1; l++) pl += (d * tab.level_scale[l] < dmax) ? 1 : 0;
  } else {
    pl = qlevel;
    live = pl < tab.nlevels;
  }
  if (!live) return q;
  // 6. the radius of that level
  int32_t r = 0;
  for (int l = 0; l < tab.nlevels; l++) {
    const int32_t rl = near ? tab.radius_near[l] : tab.radius_far[l];
    r = l == pl ? rl : r;
  }
  return Query{true, near, xc, yc, pl, r};
}

// The fuse call's reprojection test of one candidate keypoint: (u, v, ur) its Q8 observation words (the pose call's
// clamp and conversion; ur == pq::MONO: monocular), w = inv_sigma2 of the keypoint's level.  A NaN fails; with both
// bounds +inf every candidate of a live query passes (no NaN can arise: pu, pv, bf and iz are finite).
PISLAM_HD bool fuse_ok(const Pixel &p, int32_t u, int32_t v, int32_t ur, float w, float chi2_mono, float chi2_stereo) {
  const float ex = p.pu - pq::obs_px(u), ey = p.pv - pq::obs_px(v);
  const float e2 = ex * ex + ey * ey;
  if (ur == pq::MONO) return e2 * w <= chi2_mono;
  const float er = p.pur - pq::obs_px(ur);
  return (e2 + er * er) * w <= chi2_stereo;
}

}  // namespace pjm
