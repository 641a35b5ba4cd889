// pislam_warp_kernels.h — the fixed-point mesh warp (pislam_warp_batch; include/pislam_hip.h, DESIGN.md section
// 5.5): lens undistortion and stereo rectification of a batch of 8-bit frames through a coarse grid of Q8 source
// coordinates, bilinear in 1/32 pixel.  Integers only; the statement in the header is the contract.
//
// One workgroup of THREADS per TW x TH output tile, grid = tiles x batch, one launch per call, no workspace.  A lane
// produces four adjacent outputs of two rows 16 apart and stores one dword each (bytes at a ragged right edge or an
// unaligned destination).  The tile's record (pislam_warp_plan.h, made once per warp on the host) is the source
// bounding box of all its taps:
//   staged  the box goes into LDS with coalesced aligned dword loads (bytes where a dword would leave the row's
//           src_width bytes: nothing outside the source rectangle is read) and the taps are byte reads from LDS;
//           a row lies at the alignment it has in memory, rows box_pitch() apart (an odd number of dwords);
//   direct  the taps are byte loads from global memory through the caches: boxes beyond LDS_BYTES, or option
//           "warp_direct".
// Both paths run the same arithmetic on the same bytes.  The mesh is read from global memory: with cells of four
// pixels or more a lane's four outputs share one cell (eight node loads per lane and row, most of them the
// neighbouring lanes' addresses), and a VGA mesh at log_cell 3 is 40 KB, resident in L2.
#pragma once

#include "pislam_warp_plan.h"

namespace pw {

struct WarpArgs {
  const Tile *tiles;
  const int32_t *mesh_x, *mesh_y;              // [mesh_h][mesh_w]
  int32_t mesh_w, log_cell, width, height, src_width, src_height, border, tiles_x, direct;
  const uint8_t *src;
  int32_t src_vstep;
  size_t src_stride;
  uint8_t *dst;
  int32_t dst_vstep;
  size_t dst_stride;
};

// (misalignment of a box row in memory: the low bits of its first byte's address)
__device__ inline uint32_t row_mis(uint32_t src_lo, int v, int vstep, int bx0) {
  return (src_lo + (uint32_t)(v & 3) * (uint32_t)(vstep & 3) + (uint32_t)bx0) & 3u;
}

// Nodes and everything interpolated from them fit 24 signed bits, weights 7: the products are the full-rate 24-bit
// multiply (a 32-bit one issues at a quarter of the rate, and the kernel is bound by its integer arithmetic).
__device__ inline int lerp_q8(int m0, int m1, int f, int C, int lc) { return (__mul24(m0, C - f) + __mul24(m1, f) + (C >> 1)) >> lc; }

// the source coordinate of output pixel (x, y) on one axis
__device__ inline int mesh_coord(const int32_t *m, int mesh_w, int lc, int x, int y) {
  const int C = 1 << lc, fx = x & (C - 1), fy = y & (C - 1);
  const int32_t *r0 = m + (size_t)(y >> lc) * mesh_w + (x >> lc), *r1 = r0 + mesh_w;
  return lerp_q8(lerp_q8(r0[0], r0[1], fx, C, lc), lerp_q8(r1[0], r1[1], fx, C, lc), fy, C, lc);
}

template <bool STAGED>
struct Source {
  const uint8_t *g;                            // the frame (direct), or the LDS box (staged)
  uint32_t src_lo;
  int vstep, sw, sh, border, bx0, by0, pitch;

  // where row v's column 0 lies, as an offset from g (valid for 0 <= v < sh only)
  __device__ ptrdiff_t row(int v) const {
    if (STAGED) return (ptrdiff_t)(__mul24(v - by0, pitch) + (int)row_mis(src_lo, v, vstep, bx0) - bx0);
    return (ptrdiff_t)v * (ptrdiff_t)vstep;
  }
  __device__ uint32_t sample(int sx_q8, int sy_q8) const {
    const int s5x = (sx_q8 + 4) >> 3, s5y = (sy_q8 + 4) >> 3;
    const int x0 = s5x >> 5, ax = s5x & 31, y0 = s5y >> 5, ay = s5y & 31;
    const bool cx0 = (unsigned)x0 < (unsigned)sw, cx1 = (unsigned)(x0 + 1) < (unsigned)sw;
    uint32_t p00 = border, p01 = border, p10 = border, p11 = border;
    if ((unsigned)y0 < (unsigned)sh) {
      const ptrdiff_t r = row(y0) + x0;
      if (cx0) p00 = g[r];
      if (cx1) p01 = g[r + 1];
    }
    if ((unsigned)(y0 + 1) < (unsigned)sh) {
      const ptrdiff_t r = row(y0 + 1) + x0;
      if (cx0) p10 = g[r];
      if (cx1) p11 = g[r + 1];
    }
    const uint32_t top = __umul24(32 - ax, p00) + __umul24(ax, p01), bot = __umul24(32 - ax, p10) + __umul24(ax, p11);
    return (__umul24(32 - ay, top) + __umul24(ay, bot) + 512) >> 10;
  }
};

template <bool STAGED>
__device__ inline void warp_rows(const WarpArgs &a, const Source<STAGED> &S, uint8_t *d, int tx0, int ty0) {
  const int lc = a.log_cell, C = 1 << lc;
  const int x = tx0 + (int)(threadIdx.x & 15) * 4;
  if (x >= a.width) return;
  const int n = min(4, a.width - x);
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int y = ty0 + (int)(threadIdx.x >> 4) + 16 * pass;
    if (y >= a.height) break;
    uint32_t out[4] = {0, 0, 0, 0};
    if (lc >= 2) {                               // the four outputs share a cell: its nodes are loaded once
      const size_t k = (size_t)(y >> lc) * a.mesh_w + (x >> lc);
      const int fy = y & (C - 1), fx0 = x & (C - 1);
      const int x00 = a.mesh_x[k], x01 = a.mesh_x[k + 1], x10 = a.mesh_x[k + a.mesh_w], x11 = a.mesh_x[k + a.mesh_w + 1];
      const int y00 = a.mesh_y[k], y01 = a.mesh_y[k + 1], y10 = a.mesh_y[k + a.mesh_w], y11 = a.mesh_y[k + a.mesh_w + 1];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (q >= n) break;
        const int fx = fx0 + q;
        const int sx = lerp_q8(lerp_q8(x00, x01, fx, C, lc), lerp_q8(x10, x11, fx, C, lc), fy, C, lc);
        const int sy = lerp_q8(lerp_q8(y00, y01, fx, C, lc), lerp_q8(y10, y11, fx, C, lc), fy, C, lc);
        out[q] = S.sample(sx, sy);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (q >= n) break;
        out[q] = S.sample(mesh_coord(a.mesh_x, a.mesh_w, lc, x + q, y), mesh_coord(a.mesh_y, a.mesh_w, lc, x + q, y));
      }
    }
    uint8_t *p = d + (size_t)y * (size_t)a.dst_vstep + x;
    if (n == 4 && ((uintptr_t)p & 3) == 0) {
      *(uint32_t *)p = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    } else {
      for (int q = 0; q < n; q++) p[q] = (uint8_t)out[q];
    }
  }
}

__global__ __launch_bounds__(THREADS) void k_warp(const WarpArgs a) {
  __shared__ uint32_t box[LDS_BYTES / 4];
  const Tile t = a.tiles[blockIdx.x];
  const int tx0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * TW, ty0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * TH;
  const uint8_t *s = a.src + (size_t)blockIdx.y * a.src_stride;
  uint8_t *d = a.dst + (size_t)blockIdx.y * a.dst_stride;
  const uint32_t src_lo = (uint32_t)(uintptr_t)s;
  if (t.bw >= 0 && !a.direct) {
    const int pitch = box_pitch(t.bw), pd = pitch >> 2;
    for (int k = (int)threadIdx.x; k < pd * t.bh; k += THREADS) {
      const int r = k / pd, c = k - r * pd, v = t.by0 + r;
      // LDS dword c of row r = the four bytes at column o of source row v, o = bx0 - mis + 4 c (an aligned address)
      const int o = t.bx0 - (int)row_mis(src_lo, v, a.src_vstep, t.bx0) + 4 * c;
      const uint8_t *p = s + ((ptrdiff_t)v * (ptrdiff_t)a.src_vstep + o);
      uint32_t w = 0;
      if (o >= 0 && o + 4 <= a.src_width) {
        w = *(const uint32_t *)p;
      } else {
        for (int q = 0; q < 4; q++)
          if (o + q >= 0 && o + q < a.src_width) w |= (uint32_t)p[q] << (8 * q);
      }
      box[k] = w;
    }
    __syncthreads();
    const Source<true> S{(const uint8_t *)box, src_lo, a.src_vstep, a.src_width, a.src_height, a.border, t.bx0, t.by0, pitch};
    warp_rows<true>(a, S, d, tx0, ty0);
  } else {
    const Source<false> S{s, src_lo, a.src_vstep, a.src_width, a.src_height, a.border, 0, 0, 0};
    warp_rows<false>(a, S, d, tx0, ty0);
  }
}

}  // namespace pw
