// Host emulation of pw::k_warp (pislam_amd/csrc/pislam_warp_kernels.h) for the sanitizers, on the CPU only: the kernel
// header compiled as plain C++, a tile's threads run one after another, twice (the first sweep fills the LDS box, the
// second computes with it complete), staged and direct, against a per-pixel int64 restatement of include/pislam_hip.h.
// Source row padding and the bytes around the frame are poisoned, so a staging load that leaves a row is reported.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -I pislam_amd/csrc tools/probes/warp_host_check.cpp -o tools/probes/_bin/warp_host_check && tools/probes/_bin/warp_host_check
#include <sanitizer/asan_interface.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>
#define __device__
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
struct D3 { unsigned x, y, z; };
static D3 threadIdx, blockIdx;
static void __syncthreads() {}
using std::min;
static int __mul24(int a, int b) { return (int)((int64_t)((int32_t)((uint32_t)a << 8) >> 8) * (int64_t)((int32_t)((uint32_t)b << 8) >> 8)); }
static unsigned __umul24(unsigned a, unsigned b) { return (unsigned)((uint64_t)(a & 0xffffff) * (uint64_t)(b & 0xffffff)); }
#include "pislam_warp_kernels.h"

static int64_t fl(int64_t a, int s) { return a >> s; }
static int ref_pixel(const std::vector<int32_t> &mx, const std::vector<int32_t> &my, int mw, int lc, int x, int y, const uint8_t *s,
                     int vstep, int sw, int sh, int border) {
  const int C = 1 << lc, i = x >> lc, fx = x & (C - 1), j = y >> lc, fy = y & (C - 1);
  auto co = [&](const std::vector<int32_t> &m) {
    int64_t a = fl((int64_t)m[j * mw + i] * (C - fx) + (int64_t)m[j * mw + i + 1] * fx + (C >> 1), lc);
    int64_t b = fl((int64_t)m[(j + 1) * mw + i] * (C - fx) + (int64_t)m[(j + 1) * mw + i + 1] * fx + (C >> 1), lc);
    return fl(a * (C - fy) + b * fy + (C >> 1), lc);
  };
  int64_t s5x = fl(co(mx) + 4, 3), s5y = fl(co(my) + 4, 3);
  int64_t x0 = fl(s5x, 5), ax = s5x & 31, y0 = fl(s5y, 5), ay = s5y & 31;
  auto S = [&](int64_t u, int64_t v) -> int64_t { return (u >= 0 && u < sw && v >= 0 && v < sh) ? s[v * vstep + u] : border; };
  return (int)(((32 - ax) * (32 - ay) * S(x0, y0) + ax * (32 - ay) * S(x0 + 1, y0) + (32 - ax) * ay * S(x0, y0 + 1) +
                ax * ay * S(x0 + 1, y0 + 1) + 512) >> 10);
}

static int run_case(int W, int H, int SW, int SH, int lc, int kind, int border, int pad, int misalign, unsigned seed) {
  std::mt19937 rng(seed);
  int32_t mw, mh;
  pw::mesh_dims(W, H, lc, &mw, &mh);
  std::vector<int32_t> mx((size_t)mw * mh), my((size_t)mw * mh);
  const int C = 1 << lc;
  for (int j = 0; j < mh; j++)
    for (int i = 0; i < mw; i++) {
      int64_t x = (int64_t)i * C, y = (int64_t)j * C, vx, vy;
      switch (kind) {
        case 0: vx = 256 * x, vy = 256 * y; break;                                     // identity
        case 1: vx = 300 * x + 20 * y - 700 + (int)(rng() % 1025) - 512, vy = 250 * y - 10 * x - 300 + (int)(rng() % 1025) - 512; break;
        case 2: vx = 2048 * x, vy = 2048 * y; break;                                    // 8x minify
        case 3: vx = (rng() & 1) ? pw::NODE_LO : pw::NODE_HI, vy = (rng() & 1) ? pw::NODE_LO : pw::NODE_HI; break;
        case 4: vx = 256 * x - 128, vy = 256 * y - 128; break;                          // -0.5 px
        default: vx = 256 * x + 256 * (SW - W) + 100, vy = 256 * y + 37; break;         // near the right end
      }
      mx[(size_t)j * mw + i] = (int32_t)std::max<int64_t>(pw::NODE_LO, std::min<int64_t>(pw::NODE_HI, vx));
      my[(size_t)j * mw + i] = (int32_t)std::max<int64_t>(pw::NODE_LO, std::min<int64_t>(pw::NODE_HI, vy));
    }
  if (lc == 0) {                                 // ignored nodes: garbage
    for (int j = 0; j < mh; j++) mx[(size_t)j * mw + mw - 1] = 0x7fffffff, my[(size_t)j * mw + mw - 1] = -0x7fffffff;
    for (int i = 0; i < mw; i++) mx[(size_t)(mh - 1) * mw + i] = 0x7fffffff, my[(size_t)(mh - 1) * mw + i] = -0x7fffffff;
  }
  if (pw::check_create(W, H, SW, SH, lc, mx.data(), my.data(), border)) { printf("check_create refused\n"); return 1; }
  pw::Plan plan = pw::make_plan(W, H, SW, SH, lc, mx.data(), my.data());
  const int svs = SW + pad, dvs = W + pad;
  const size_t sbytes = (size_t)(SH - 1) * svs + SW, dbytes = (size_t)(H - 1) * dvs + W;
  uint8_t *sraw = (uint8_t *)malloc(sbytes + 8), *draw = (uint8_t *)malloc(dbytes + 8), *d2 = (uint8_t *)malloc(dbytes + 8);
  uint8_t *s = sraw + misalign, *d = draw + misalign, *dd = d2 + misalign;
  for (size_t k = 0; k < sbytes; k++) s[k] = (uint8_t)rng();
  memset(draw, 0xEE, dbytes + 8), memset(d2, 0xEE, dbytes + 8);
  for (int v = 0; v + 1 < SH && pad; v++) ASAN_POISON_MEMORY_REGION(s + (size_t)v * svs + SW, pad);
  if (misalign) ASAN_POISON_MEMORY_REGION(sraw, misalign);
  ASAN_POISON_MEMORY_REGION(s + sbytes, 8 - misalign);
  int bad = 0;
  for (int direct = 0; direct < 2; direct++) {
    pw::WarpArgs a{};
    a.tiles = plan.tiles.data(), a.mesh_x = mx.data(), a.mesh_y = my.data();
    a.mesh_w = mw, a.log_cell = lc, a.width = W, a.height = H, a.src_width = SW, a.src_height = SH, a.border = border;
    a.tiles_x = plan.tiles_x, a.direct = direct, a.src = s, a.src_vstep = svs, a.dst = direct ? dd : d, a.dst_vstep = dvs;
    for (unsigned t = 0; t < plan.tiles.size(); t++)
      for (int sweep = 0; sweep < 2; sweep++)
        for (unsigned th = 0; th < pw::THREADS; th++) {
          blockIdx.x = t, blockIdx.y = 0, threadIdx.x = th;
          pw::k_warp(a);
        }
    uint8_t *o = direct ? dd : d;
    for (int y = 0; y < H; y++)
      for (int x = 0; x < dvs && (size_t)y * dvs + x < dbytes; x++) {
        const int want = x < W ? ref_pixel(mx, my, mw, lc, x, y, s, svs, SW, SH, border) : 0xEE;
        if (o[(size_t)y * dvs + x] != want) {
          if (bad++ < 5) printf("  mismatch direct=%d (%d,%d): got %d want %d\n", direct, x, y, o[(size_t)y * dvs + x], want);
        }
      }
  }
  ASAN_UNPOISON_MEMORY_REGION(sraw, sbytes + 8);
  printf("%s W%d H%d SW%d SH%d lc%d kind%d pad%d mis%d: tiles %zu staged %d direct %d\n", bad ? "FAIL" : "ok  ", W, H, SW, SH, lc, kind, pad,
         misalign, plan.tiles.size(), plan.staged, plan.direct);
  free(sraw), free(draw), free(d2);
  return bad != 0;
}

int main() {
  int bad = 0;
  const int shapes[][4] = {{1, 1, 1, 1}, {64, 32, 64, 32}, {65, 33, 70, 40}, {70, 37, 90, 50}, {200, 90, 211, 97}};
  unsigned seed = 1;
  for (auto &sh : shapes)
    for (int lc : {0, 1, 2, 3, 6})
      for (int kind : {0, 1, 4})
        for (int pad : {0, 5, 21})
          bad += run_case(sh[0], sh[1], sh[2], sh[3], lc, kind, 0xA5, pad, pad ? 3 : 0, seed++);
  bad += run_case(80, 50, 640, 400, 3, 2, 7, 3, 1, seed++);
  bad += run_case(80, 50, 640, 400, 0, 2, 7, 0, 0, seed++);
  bad += run_case(1, 1, 1, 1, 0, 3, 9, 0, 0, seed++);
  bad += run_case(70, 37, 90, 50, 3, 3, 9, 2, 2, seed++);
  bad += run_case(130, 2, 16384, 2, 3, 5, 9, 1, 1, seed++);
  bad += run_case(4096, 1, 300, 7, 6, 1, 9, 1, 1, seed++);
  bad += run_case(1, 4096, 7, 300, 5, 1, 9, 1, 1, seed++);
  printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
