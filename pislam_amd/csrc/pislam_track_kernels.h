// Pyramidal Lucas-Kanade tracking and sub-pixel match refinement (the contract is the comment
// above pislam_track_lk_batch in include/pislam_hip.h).  Included by pislam_hip.hip only.
//
//   k_track_lk<W>   one wave per point, LK_PPW points per workgroup pass; the waves of a workgroup never meet (no
//                   workgroup barrier), so each runs its own chain and its own number of iterations.
//                     template   the (2W+3)^2 Q5 samples around p go to the wave's slice of LDS, LK 64 lanes abreast
//                     window     window pixel k = lane + 64 j (j < LK_SLOTS<W>: one pixel per lane up to W = 3, four
//                                at W = 7) keeps its T, gx, gy in registers for the whole level
//                     sums       A11, A12, A22 once per level, b1, b2 and sad once per iteration, by xor butterflies:
//                                every lane holds the totals, so every lane runs the same 64-bit solve and nothing
//                                is broadcast; code, it and the level are wave uniform
//                   The bilinear weights are the same for every pixel of a window (the offsets are whole pixels), so a
//                   sample is four byte loads and four multiply-adds.
//   k_lk_count      one workgroup per pair: ntracked[b] = the points with code 0.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace pt {

constexpr int LK_MAX_LEVELS = 16;
constexpr int LK_MAX_W = 7;                            // win_radius limit
constexpr int LK_THREADS = 256;
constexpr int LK_PPW = LK_THREADS / 64;                // points per workgroup pass: one per wave
constexpr int LK_T_SLOTS = 292;                        // (2 * LK_MAX_W + 3)^2 = 289 halfwords, rounded up to 8 bytes
constexpr int LK_COUNT_THREADS = 256;
constexpr int32_t LK_COORD_MAX = 1 << 20;              // points and guesses are clamped to +- this
constexpr int32_t LK_MAP_MAX = 1 << 22;                // positions mapped between levels are clamped to +- this

struct LkLevel {
  int32_t col0, row0, width, height;                   // rectangle inside the stacked pyramid
  int32_t scale;                                       // level-0 pixels per level pixel, Q16
};

struct LkArgs {                                        // passed by value (kernel arguments: a captured graph keeps its own copy)
  LkLevel lv[LK_MAX_LEVELS];
  int32_t nlevels, max_iters, eps_q8, max_step_q8, level_step, max_coarse, min_eig, max_err;
  const uint8_t *prev, *next;                          // pair b at + b * pyramid_stride, rows of vstep bytes
  int32_t vstep;
  size_t pyramid_stride;
  const int32_t *pts;                                  // [batch][stride][2]
  const uint32_t *counts;                              // [batch]
  const int32_t *guess;                                // [batch][stride][2] or null; may be next_q8
  size_t stride;
  int32_t *next_q8;                                    // [batch][stride][2]
  uint32_t *status, *err;                              // [batch][stride]
};

#if defined(__HIPCC__)

// A count as the call reads it: PISLAM_COUNT_INVALID is 0.
__device__ __forceinline__ uint32_t lk_count(uint32_t c, size_t stride) {
  return c == 0xffffffffu ? 0u : (uint32_t)min((size_t)c, stride);
}

// Orders one wave's LDS traffic: the lanes of a wave run in lockstep and the LDS serves a wave's instructions in
// order, so only the compiler has to be kept from moving accesses across this point.
__device__ __forceinline__ void lk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int32_t lk_uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t lk_floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// A coordinate on a level of scale `from` on a level of scale `to`: floor((u * from + floor(to / 2)) / to), clamped.
// |u| <= 2^22 and from <= 2^20: the product stays below 2^43.
__device__ __forceinline__ int32_t lk_map(int32_t u, int32_t from, int32_t to) {
  const int64_t v = lk_floordiv((int64_t)u * from + (to >> 1), to);
  return (int32_t)max((int64_t)-LK_MAP_MAX, min((int64_t)LK_MAP_MAX, v));
}

__device__ __forceinline__ bool lk_inside(int32_t x, int32_t y, int32_t m, int32_t width, int32_t height) {
  const int32_t x0 = x >> 8, y0 = y >> 8;
  return (x0 - m >= 0) & (y0 - m >= 0) & (x0 + m + 1 <= width - 1) & (y0 + m + 1 <= height - 1);
}

// The four bilinear weights of a Q8 position's fraction and the Q5 sample at a whole-pixel offset from it.
struct LkTaps {
  uint32_t w00, w01, w10, w11;
  __device__ LkTaps(int32_t x, int32_t y) {
    const uint32_t ax = (uint32_t)(x & 255), ay = (uint32_t)(y & 255);
    w00 = (256 - ax) * (256 - ay), w01 = ax * (256 - ay), w10 = (256 - ax) * ay, w11 = ax * ay;
  }
  // r: the byte at (x0 + dx, y0 + dy)
  __device__ __forceinline__ int32_t at(const uint8_t *r, int32_t vstep) const {
    return (int32_t)((w00 * r[0] + w01 * r[1] + w10 * r[vstep] + w11 * r[vstep + 1] + 1024u) >> 11);
  }
};

// One axis of the step: floor((-64 n + floor(det / 2)) / det) clamped to +- lim, with |n| < 2^60 and 0 < det < 2^56.
// n = k det + rem (0 <= rem < det) gives step = -64 k + floor((floor(det / 2) - 64 rem) / det), the second term in
// [-64, 0]: beyond |k| = 128 the clamp (lim <= 4096) decides, below it everything fits easily.
__device__ __forceinline__ int32_t lk_step(int64_t n, int64_t det, int32_t lim) {
  const int64_t k = lk_floordiv(n, det), rem = n - k * det;
  if (k > 128) return -lim;
  if (k < -128) return lim;
  const int64_t s = -64 * k + lk_floordiv((det >> 1) - 64 * rem, det);
  return (int32_t)max((int64_t)-lim, min((int64_t)lim, s));
}

struct LkResult {
  int32_t code, qx, qy, it;
  uint32_t sad;
};

// The level procedure on one level of both images (pl / nl: the level's byte (0, 0)), p and q level-local Q8; `own`
// applies the max_err test.  tm: the wave's LDS slice.  Everything but the window pixels is wave uniform.
template <int W>
__device__ __forceinline__ LkResult lk_level(const LkArgs &a, const uint8_t *__restrict__ pl, const uint8_t *__restrict__ nl,
                                             int32_t width, int32_t height, int32_t px, int32_t py, int32_t qx, int32_t qy,
                                             bool own, uint16_t *tm, uint32_t lane) {
  constexpr int S = 2 * W + 3, D = 2 * W + 1, N = D * D, SLOTS = (N + 63) / 64;
  const int32_t vstep = a.vstep;
  LkResult res{1, qx, qy, 0, 0xffffffffu};
  if (!lk_inside(px, py, W + 1, width, height)) return res;
  // template: (2W+3)^2 samples around p
  {
    const LkTaps taps(px, py);
    const uint8_t *c = pl + (ptrdiff_t)((py >> 8) - (W + 1)) * vstep + ((px >> 8) - (W + 1));
    lk_wave_sync();                                      // (the previous level's reads of tm are done)
#pragma unroll
    for (int k0 = 0; k0 < S * S; k0 += 64) {
      const uint32_t k = (uint32_t)k0 + lane;
      if (k < (uint32_t)(S * S)) tm[k] = (uint16_t)taps.at(c + (ptrdiff_t)(k / S) * vstep + (k % S), vstep);
    }
    lk_wave_sync();
  }
  // this lane's window pixels: T, gx, gy (zero past the window) and the offset of the pixel's tap in the next image
  int32_t T[SLOTS], gx[SLOTS], gy[SLOTS], off[SLOTS];
  int32_t a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
  for (int j = 0; j < SLOTS; j++) {
    const uint32_t k = (uint32_t)(64 * j) + lane;
    const bool in = k < (uint32_t)N;
    const uint32_t wx = in ? k % D : 0u, wy = in ? k / D : 0u, c = (wy + 1) * S + wx + 1;
    T[j] = in ? (int32_t)tm[c] : 0;
    gx[j] = in ? ((int32_t)tm[c + 1] - (int32_t)tm[c - 1] + 4) >> 3 : 0;
    gy[j] = in ? ((int32_t)tm[c + S] - (int32_t)tm[c - S] + 4) >> 3 : 0;
    off[j] = in ? ((int32_t)wy - W) * vstep + ((int32_t)wx - W) : 0x7fffffff;
    a11 += gx[j] * gx[j], a12 += gx[j] * gy[j], a22 += gy[j] * gy[j];
  }
  const int64_t A11 = pdev::wave_sum(a11), A12 = pdev::wave_sum(a12), A22 = pdev::wave_sum(a22);
  const int64_t t = (int64_t)a.min_eig * N, det = A11 * A22 - A12 * A12;
  res.code = 2;
  if (!(det > 0 && A11 + A22 >= 2 * t && (A11 - t) * (A22 - t) - A12 * A12 >= 0)) return res;
  res.code = 3;
  if (!lk_inside(qx, qy, W, width, height)) return res;
  // r at q for this lane's pixels; returns the lane's share of sad, adds to b1 / b2
  auto residual = [&](int32_t x, int32_t y, int32_t &b1, int32_t &b2) {
    const LkTaps taps(x, y);
    const uint8_t *c = nl + (ptrdiff_t)(y >> 8) * vstep + (x >> 8);
    int32_t sad = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
      if (off[j] != 0x7fffffff) {
        const int32_t r = taps.at(c + off[j], vstep) - T[j];
        sad += abs(r), b1 += r * gx[j], b2 += r * gy[j];
      }
    }
    return sad;
  };
  int32_t it = 0;
  for (;;) {
    int32_t b1 = 0, b2 = 0;
    const int32_t s = residual(qx, qy, b1, b2);
    res.sad = (uint32_t)pdev::wave_sum(s);
    if (it == a.max_iters) {
      res.code = 0;
      break;
    }
    const int64_t B1 = pdev::wave_sum(b1), B2 = pdev::wave_sum(b2);
    const int32_t sx = lk_uniform(lk_step(A22 * B1 - A12 * B2, det, a.max_step_q8));
    const int32_t sy = lk_uniform(lk_step(A11 * B2 - A12 * B1, det, a.max_step_q8));
    it++;
    if (!lk_inside(qx + sx, qy + sy, W, width, height)) break;          // code 3, q kept
    qx += sx, qy += sy;
    if (abs(sx) <= a.eps_q8 && abs(sy) <= a.eps_q8) {
      int32_t u1 = 0, u2 = 0;
      res.sad = (uint32_t)pdev::wave_sum(residual(qx, qy, u1, u2));
      res.code = 0;
      break;
    }
  }
  res.qx = qx, res.qy = qy, res.it = it;
  if (res.code != 0) res.sad = 0xffffffffu;
  else if (own && a.max_err > 0 && (uint64_t)res.sad > (uint64_t)a.max_err * N) res.code = 4;
  return res;
}

// The fields of level c, picked by selects in a wave-uniform loop over the kernel arguments (no indexing of the
// table by a register).
__device__ __forceinline__ LkLevel lk_pick(const LkArgs &a, int32_t c) {
  LkLevel h{0, 0, 0, 0, 65536};
  for (int l = 0; l < a.nlevels; l++)
    if (l == c) h = a.lv[l];
  return h;
}

// One point: its level, the chain of coarser levels, the own level, the outputs.
template <int W>
__device__ __forceinline__ void lk_point(const LkArgs &a, const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                         size_t o, uint16_t *tm, uint32_t lane) {
  const int32_t x = max(-LK_COORD_MAX, min(LK_COORD_MAX, a.pts[2 * o])), y = max(-LK_COORD_MAX, min(LK_COORD_MAX, a.pts[2 * o + 1]));
  int32_t qx = x, qy = y;
  if (a.guess) {
    qx = max(-LK_COORD_MAX, min(LK_COORD_MAX, a.guess[2 * o]));
    qy = max(-LK_COORD_MAX, min(LK_COORD_MAX, a.guess[2 * o + 1]));
  }
  int32_t l = -1;
  LkLevel own{0, 0, 0, 0, 65536};
  for (int k = 0; k < a.nlevels; k++) {
    const LkLevel L = a.lv[k];
    if (((uint32_t)((x >> 8) - L.col0) < (uint32_t)L.width) & ((uint32_t)((y >> 8) - L.row0) < (uint32_t)L.height)) l = k, own = L;
  }
  l = lk_uniform(l);
  LkResult r{1, qx, qy, 0, 0xffffffffu};
  if (l >= 0) {
    const int32_t px = x - 256 * own.col0, py = y - 256 * own.row0;
    qx -= 256 * own.col0, qy -= 256 * own.row0;
    const int32_t M = min(a.max_coarse, (a.nlevels - 1 - l) / a.level_step);
    for (int32_t m = M; m > 0; m--) {
      const LkLevel C = lk_pick(a, l + m * a.level_step);
      const size_t org = (size_t)C.row0 * a.vstep + C.col0;
      const LkResult rc = lk_level<W>(a, prev + org, next + org, C.width, C.height, lk_map(px, own.scale, C.scale),
                                      lk_map(py, own.scale, C.scale), lk_map(qx, own.scale, C.scale),
                                      lk_map(qy, own.scale, C.scale), false, tm, lane);
      if (lk_uniform(rc.code) == 0) qx = lk_map(rc.qx, C.scale, own.scale), qy = lk_map(rc.qy, C.scale, own.scale);
    }
    const size_t org = (size_t)own.row0 * a.vstep + own.col0;
    r = lk_level<W>(a, prev + org, next + org, own.width, own.height, px, py, qx, qy, true, tm, lane);
    r.qx += 256 * own.col0, r.qy += 256 * own.row0;
  }
  if (lane == 0) {
    a.next_q8[2 * o] = r.qx, a.next_q8[2 * o + 1] = r.qy;
    a.status[o] = (uint32_t)r.code | (uint32_t)r.it << 8;
    a.err[o] = r.sad;
  }
}

// grid (point tiles, pairs), LK_THREADS threads; the pointers of `a` are those of the launch's first pair.
template <int W>
__global__ __launch_bounds__(LK_THREADS) void k_track_lk(LkArgs a) {
  __shared__ uint16_t tmpl[LK_PPW][LK_T_SLOTS];
  const size_t b = blockIdx.y;
  const uint32_t wave = (uint32_t)lk_uniform((int32_t)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t n = lk_count(a.counts[b], a.stride);
  const uint8_t *prev = a.prev + b * a.pyramid_stride, *next = a.next + b * a.pyramid_stride;
  for (uint32_t i = blockIdx.x * (uint32_t)LK_PPW + wave; i < n; i += gridDim.x * (uint32_t)LK_PPW)
    lk_point<W>(a, prev, next, b * a.stride + i, tmpl[wave], lane);
}

// grid (pairs), LK_COUNT_THREADS threads.
__global__ __launch_bounds__(LK_COUNT_THREADS) void k_lk_count(const uint32_t *__restrict__ counts, size_t stride,
                                                               const uint32_t *__restrict__ status,
                                                               uint32_t *__restrict__ ntracked) {
  __shared__ uint32_t part[LK_COUNT_THREADS / 64];
  const size_t b = blockIdx.x;
  const uint32_t n = lk_count(counts[b], stride);
  int32_t mine = 0;
  for (uint32_t i = threadIdx.x; i < n; i += LK_COUNT_THREADS) mine += (status[b * stride + i] & 0xffu) == 0u;
  mine = pdev::wave_sum(mine);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = (uint32_t)mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int k = 0; k < LK_COUNT_THREADS / 64; k++) s += part[k];
    ntracked[b] = s;
  }
}

#endif  // __HIPCC__

}  // namespace pt
