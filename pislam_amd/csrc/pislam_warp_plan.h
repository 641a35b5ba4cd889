// pislam_warp_plan.h — the host half of the mesh warp (pislam_warp_*; include/pislam_hip.h):
// the limits, the mesh dimensions and the tile plan pislam_warp_create makes once per warp.  Plain C++ without a HIP
// type, so that it also compiles with a host compiler alone; pislam_warp_kernels.h reads the same constants and the
// same Tile record.
//
// The output is cut into TW x TH tiles, one workgroup each.  A tile's record is the bounding box of every source
// byte its taps can touch, clipped to the source rectangle.  The box follows from the minimum and maximum of the
// tile's nodes per axis: an interpolated coordinate is a rounded weighted mean of integers, so it never leaves the
// range of its four nodes, and (s + 4) >> 3 >> 5 is monotone.  A box that fits LDS_BYTES is staged; a larger one
// (strong minification, a mesh of wild content) sends the tile down the direct path (bw = -1).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__
#else
#define PW_HD
#endif

namespace pw {

constexpr int TW = 64, TH = 32;                // outputs per workgroup
constexpr int THREADS = 256;                   // four adjacent outputs per lane, two rows 16 apart
constexpr int LDS_BYTES = 16384;               // source box per workgroup: eight workgroups per CU keep 128 of its 160 KiB
constexpr int MAX_LOG_CELL = 6;
constexpr int MAX_OUT = 4096, MAX_SRC = 16384;
constexpr int32_t NODE_LO = -(1 << 23), NODE_HI = (1 << 23) - 1;

struct Tile {
  int32_t bx0, by0;                            // first source column / row of the box
  int32_t bw, bh;                              // its extent; 0 x 0: every tap is border; bw < 0: direct path
};

// Bytes per LDS row of a box bw wide: up to 3 bytes in front (rows start on the aligned dword below their first
// byte), whole dwords, and an odd number of them so that consecutive rows start on different banks.
PW_HD inline int box_pitch(int bw) { return (((bw + 6) >> 2) | 1) << 2; }

// x0 (or y0) of the sampling statement for a Q8 coordinate
PW_HD inline int tap0(int s_q8) { return ((s_q8 + 4) >> 3) >> 5; }

inline bool mesh_dims(int width, int height, int log_cell, int32_t *mesh_w, int32_t *mesh_h) {
  if (width < 1 || width > MAX_OUT || height < 1 || height > MAX_OUT || log_cell < 0 || log_cell > MAX_LOG_CELL) return false;
  if (mesh_w) *mesh_w = ((width - 1) >> log_cell) + 2;
  if (mesh_h) *mesh_h = ((height - 1) >> log_cell) + 2;
  return true;
}

// nullptr, or what is wrong with the arguments of pislam_warp_create
inline const char *check_create(int width, int height, int src_width, int src_height, int log_cell, const int32_t *mesh_x,
                                const int32_t *mesh_y, int border) {
  if (width < 1 || width > MAX_OUT || height < 1 || height > MAX_OUT) return "width and height must be 1..4096";
  if (src_width < 1 || src_width > MAX_SRC || src_height < 1 || src_height > MAX_SRC) return "src_width and src_height must be 1..16384";
  if (log_cell < 0 || log_cell > MAX_LOG_CELL) return "log_cell must be 0..6";
  if (border < 0 || border > 255) return "border must be 0..255";
  if (!mesh_x || !mesh_y) return "null mesh";
  int32_t mw = 0, mh = 0;
  mesh_dims(width, height, log_cell, &mw, &mh);
  // a dense mesh's last node column and row carry weight 0 everywhere: supplied, never looked at
  const int uw = log_cell ? mw : mw - 1, uh = log_cell ? mh : mh - 1;
  for (int j = 0; j < uh; j++)
    for (int i = 0; i < uw; i++) {
      const size_t k = (size_t)j * mw + i;
      if (mesh_x[k] < NODE_LO || mesh_x[k] > NODE_HI || mesh_y[k] < NODE_LO || mesh_y[k] > NODE_HI)
        return "every mesh node must lie in [-2^23, 2^23)";
    }
  return nullptr;
}

struct Plan {
  std::vector<Tile> tiles;
  int tiles_x = 0, tiles_y = 0, staged = 0, direct = 0;
};

// arguments as check_create accepted them
inline Plan make_plan(int width, int height, int src_width, int src_height, int log_cell, const int32_t *mesh_x,
                      const int32_t *mesh_y) {
  Plan p;
  int32_t mw = 0, mh = 0;
  mesh_dims(width, height, log_cell, &mw, &mh);
  p.tiles_x = (width + TW - 1) / TW, p.tiles_y = (height + TH - 1) / TH;
  p.tiles.resize((size_t)p.tiles_x * p.tiles_y);
  const int last = log_cell ? 1 : 0;           // (dense: the node after a tile's last pixel has weight 0)
  for (int ty = 0; ty < p.tiles_y; ty++)
    for (int tx = 0; tx < p.tiles_x; tx++) {
      const int x0 = tx * TW, x1 = std::min(x0 + TW, width) - 1, y0 = ty * TH, y1 = std::min(y0 + TH, height) - 1;
      const int i0 = x0 >> log_cell, i1 = (x1 >> log_cell) + last, j0 = y0 >> log_cell, j1 = (y1 >> log_cell) + last;
      int32_t xlo = NODE_HI, xhi = NODE_LO, ylo = NODE_HI, yhi = NODE_LO;
      for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
          const size_t k = (size_t)j * mw + i;
          xlo = std::min(xlo, mesh_x[k]), xhi = std::max(xhi, mesh_x[k]);
          ylo = std::min(ylo, mesh_y[k]), yhi = std::max(yhi, mesh_y[k]);
        }
      const int bx0 = std::max(tap0(xlo), 0), bx1 = std::min(tap0(xhi) + 1, src_width - 1);
      const int by0 = std::max(tap0(ylo), 0), by1 = std::min(tap0(yhi) + 1, src_height - 1);
      Tile &t = p.tiles[(size_t)ty * p.tiles_x + tx];
      if (bx0 > bx1 || by0 > by1) {
        t = Tile{0, 0, 0, 0};
        p.staged++;
      } else if ((int64_t)box_pitch(bx1 - bx0 + 1) * (by1 - by0 + 1) <= LDS_BYTES) {
        t = Tile{bx0, by0, bx1 - bx0 + 1, by1 - by0 + 1};
        p.staged++;
      } else {
        t = Tile{bx0, by0, -1, -1};
        p.direct++;
      }
    }
  return p;
}

// nullptr, or what is wrong with the per-call arguments of pislam_warp_batch (pointer kinds are the caller's to check)
inline const char *check_batch(int width, int height, int src_width, int src_height, const void *src, int src_vstep,
                               size_t src_stride, const void *dst, int dst_vstep, size_t dst_stride, int batch) {
  if (batch < 0) return "negative batch";
  if (src_vstep < src_width) return "src_vstep must be at least src_width";
  if (dst_vstep < width) return "dst_vstep must be at least width";
  if (batch == 0) return nullptr;
  if (!src || !dst) return "null frames";
  // the byte ranges the call reads and writes (size_t arithmetic: strides may push a batch past 4 GiB)
  const size_t s_len = (size_t)(batch - 1) * src_stride + (size_t)(src_height - 1) * (size_t)src_vstep + (size_t)src_width;
  const size_t d_len = (size_t)(batch - 1) * dst_stride + (size_t)(height - 1) * (size_t)dst_vstep + (size_t)width;
  const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
  if (s < d + d_len && d < s + s_len) return "src and dst overlap";
  return nullptr;
}

}  // namespace pw
