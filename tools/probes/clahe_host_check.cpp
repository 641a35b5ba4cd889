// Host emulation of pc::k_clahe_luts and pc::k_clahe_apply (pislam_amd/csrc/pislam_clahe_kernels.h) for the sanitizers,
// on the CPU only: the kernel header compiled as plain C++, a workgroup's 256 threads run as 256 host threads (one set per launch) that meet
// at a barrier for __syncthreads and for every shuffle, against a per-tile / per-pixel int64 restatement of
// include/pislam_hip.h.  Source row padding and the bytes around the frame are poisoned, so a load that leaves the
// width x height rectangle is reported; the destination and the tables are compared whole, sentinel included.
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -I pislam_amd/csrc tools/probes/clahe_host_check.cpp -o tools/probes/_bin/clahe_host_check && tools/probes/_bin/clahe_host_check
#include <pthread.h>
#include <sanitizer/asan_interface.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <thread>
#include <vector>
#define __HIPCC__ 1
#define __host__
#define __device__
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
struct D3 { unsigned x, y, z; };
static thread_local D3 threadIdx, blockIdx;
static pthread_barrier_t g_barrier;
static uint32_t g_xchg[256];
static void __syncthreads() { pthread_barrier_wait(&g_barrier); }
static uint32_t exchange(uint32_t x, int from) {
  g_xchg[threadIdx.x] = x;
  __syncthreads();
  const uint32_t v = g_xchg[from];
  __syncthreads();
  return v;
}
static uint32_t __shfl_xor(uint32_t x, int d, int) { return exchange(x, (int)threadIdx.x ^ d); }
static uint32_t __shfl_up(uint32_t x, int d, int) { return exchange(x, ((int)threadIdx.x & 63) >= d ? (int)threadIdx.x - d : (int)threadIdx.x); }
static uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
using std::max;
using std::min;
static unsigned __umul24(unsigned a, unsigned b) { return (unsigned)((uint64_t)(a & 0xffffff) * (uint64_t)(b & 0xffffff)); }
#include "pislam_clahe_kernels.h"

template <typename K>
static void run_grid(K kernel, const pc::Args &a, unsigned gx) {
  pthread_barrier_init(&g_barrier, nullptr, pc::THREADS);
  std::vector<std::thread> ts;
  for (unsigned t = 0; t < (unsigned)pc::THREADS; t++)
    ts.emplace_back([=] {
      for (unsigned b = 0; b < gx; b++) {
        blockIdx.x = b, blockIdx.y = 0, threadIdx.x = t;
        kernel(a);
        __syncthreads();                         // (the next workgroup reuses the LDS)
      }
    });
  for (auto &t : ts) t.join();
  pthread_barrier_destroy(&g_barrier);
}

static int refl(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

// the header's table of one tile
static void ref_lut(const uint8_t *s, int vstep, int W, int H, int tw, int th, int tx, int ty, int clip_q8, uint8_t *lut) {
  int64_t h[256] = {0}, area = (int64_t)tw * th;
  for (int y = ty * th; y < (ty + 1) * th; y++)
    for (int x = tx * tw; x < (tx + 1) * tw; x++) h[s[(size_t)refl(y, H) * vstep + refl(x, W)]]++;
  if (clip_q8 > 0) {
    const int64_t clip = std::max<int64_t>(((int64_t)clip_q8 * area) >> 16, 1);
    int64_t excess = 0;
    for (int v = 0; v < 256; v++) excess += std::max<int64_t>(h[v] - clip, 0), h[v] = std::min(h[v], clip);
    const int64_t q = excess / 256, res = excess % 256;
    for (int v = 0; v < 256; v++) h[v] += q;
    if (res > 0) {
      const int64_t step = std::max<int64_t>(256 / res, 1);
      for (int v = 0; v < 256; v++)
        if (v % step == 0 && v / step < res) h[v]++;
    }
  }
  int64_t cdf = 0;
  for (int v = 0; v < 256; v++) cdf += h[v], lut[v] = (uint8_t)std::min<int64_t>(255, (255 * cdf + (area >> 1)) / area);
}

static int64_t floordiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static int ref_pixel(const uint8_t *L, int tiles_x, int tiles_y, int tw, int th, int x, int y, int v) {
  const int64_t fx = 2 * x - tw, fy = 2 * y - th;
  int64_t tx1 = floordiv(fx, 2 * tw), ty1 = floordiv(fy, 2 * th);
  const int64_t wx2 = fx - 2 * tw * tx1, wx1 = 2 * tw - wx2, wy2 = fy - 2 * th * ty1, wy1 = 2 * th - wy2;
  int64_t tx2 = std::min<int64_t>(tx1 + 1, tiles_x - 1), ty2 = std::min<int64_t>(ty1 + 1, tiles_y - 1);
  tx1 = std::max<int64_t>(tx1, 0), ty1 = std::max<int64_t>(ty1, 0);
  auto T = [&](int64_t ty, int64_t tx) -> int64_t { return L[((size_t)ty * tiles_x + tx) * 256 + v]; };
  const int64_t S = wy1 * (wx1 * T(ty1, tx1) + wx2 * T(ty1, tx2)) + wy2 * (wx1 * T(ty2, tx1) + wx2 * T(ty2, tx2));
  const int64_t D = 4 * (int64_t)tw * th;
  return (int)((S + (D >> 1)) / D);
}

// kind: 0 random, 1 low contrast, 2 constant, 3 two-valued; tables: 0 computed, 1 random bytes, 2 checkerboard 0 / 255
static int run_case(int W, int H, int tiles_x, int tiles_y, int clip_q8, int kind, int tables, int pad, int dpad, int misalign,
                    bool in_place, unsigned seed) {
  std::mt19937 rng(seed);
  if (pc::check_params(W, H, tiles_x, tiles_y, clip_q8)) { printf("check_params refused\n"); return 1; }
  pc::Args g = pc::geometry(W, H, tiles_x, tiles_y, clip_q8);
  const int svs = W + pad, dvs = in_place ? svs : W + dpad;
  const size_t sbytes = (size_t)(H - 1) * svs + W, dbytes = (size_t)(H - 1) * dvs + W, lbytes = (size_t)tiles_x * tiles_y * 256;
  uint8_t *sraw = (uint8_t *)malloc(sbytes + 8), *draw = (uint8_t *)malloc(dbytes + 8);
  uint8_t *s = sraw + misalign, *d = draw + (in_place ? misalign : (misalign + 1) & 3);
  std::vector<uint8_t> keep(sbytes), luts(lbytes + 2, 0xEE), want_l(lbytes);
  memset(sraw, 0x5B, sbytes + 8), memset(draw, 0xEE, dbytes + 8);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      uint8_t v = (uint8_t)rng();
      if (kind == 1) v = (uint8_t)((v / 32) * 3 + 100);
      if (kind == 2) v = 77;
      if (kind == 3) v = (v & 1) ? 200 : 13;
      s[(size_t)y * svs + x] = v;
    }
  memcpy(keep.data(), s, sbytes);
  for (int tyy = 0; tyy < tiles_y; tyy++)
    for (int txx = 0; txx < tiles_x; txx++) {
      uint8_t *t = &want_l[((size_t)tyy * tiles_x + txx) * 256];
      if (tables == 0) ref_lut(s, svs, W, H, g.tw, g.th, txx, tyy, clip_q8, t);
      for (int v = 0; v < 256 && tables; v++) t[v] = tables == 1 ? (uint8_t)rng() : (uint8_t)(((txx + tyy) & 1) ? 255 : 0);
    }
  auto poison = [&] {
    for (int v = 0; v + 1 < H && pad; v++) ASAN_POISON_MEMORY_REGION(s + (size_t)v * svs + W, pad);
    if (misalign) ASAN_POISON_MEMORY_REGION(sraw, misalign);
    ASAN_POISON_MEMORY_REGION(s + sbytes, 8 - misalign);
  };
  poison();
  int bad = 0;
  for (int variant = 0; variant < 2; variant++) {
    if (in_place && variant) {                   // (the first variant's output lies in the source)
      ASAN_UNPOISON_MEMORY_REGION(sraw, sbytes + 8);
      for (int y = 0; y < H; y++) memcpy(s + (size_t)y * svs, keep.data() + (size_t)y * svs, W);
      poison();
    }
    pc::Args a = g;
    a.src = s, a.src_vstep = svs, a.luts = luts.data() + 1;        // (the tables at an odd address)
    if (tables == 0) {
      std::fill(luts.begin(), luts.end(), 0xEE);
      if (variant) run_grid(pc::k_clahe_luts<true>, a, tiles_x * tiles_y);
      else run_grid(pc::k_clahe_luts<false>, a, tiles_x * tiles_y);
      if (luts[0] != 0xEE || luts[lbytes + 1] != 0xEE) bad++, printf("  table sentinel overwritten\n");
      for (size_t k = 0; k < lbytes; k++)
        if (luts[k + 1] != want_l[k] && bad++ < 5) printf("  table %zu bin %zu: got %d want %d\n", k >> 8, k & 255, luts[k + 1], want_l[k]);
    } else {
      memcpy(luts.data() + 1, want_l.data(), lbytes);
    }
    uint8_t *o = in_place ? s : d;
    if (!in_place) memset(draw, 0xEE, dbytes + 8);
    a.dst = o, a.dst_vstep = dvs;
    const unsigned gx = (unsigned)(a.cells_x * a.cells_y * a.chunks);
    if (variant) run_grid(pc::k_clahe_apply<true>, a, gx);
    else run_grid(pc::k_clahe_apply<false>, a, gx);
    if (in_place) ASAN_UNPOISON_MEMORY_REGION(sraw, sbytes + 8);
    const uint8_t *base = in_place ? sraw : draw;
    const size_t off = (size_t)(o - base);
    for (size_t k = 0; k < dbytes + 8; k++) {
      int want = in_place ? 0x5B : 0xEE;
      if (k >= off && k - off < dbytes) {
        const int y = (int)((k - off) / dvs), x = (int)((k - off) % dvs);
        if (x < W) want = ref_pixel(want_l.data(), tiles_x, tiles_y, g.tw, g.th, x, y, keep[(size_t)y * svs + x]);
      }
      if (base[k] != want && bad++ < 5) printf("  byte %zu (variant %d): got %d want %d\n", k, variant, base[k], want);
    }
  }
  ASAN_UNPOISON_MEMORY_REGION(sraw, sbytes + 8);
  printf("%s %dx%d tiles %dx%d clip_q8 %d kind %d tables %d pad %d/%d mis %d%s: cells %dx%d x %d\n", bad ? "FAIL" : "ok  ", W, H, tiles_x,
         tiles_y, clip_q8, kind, tables, pad, dpad, misalign, in_place ? " in place" : "", g.cells_x, g.cells_y, g.chunks);
  free(sraw), free(draw);
  return bad != 0;
}

int main() {
  int bad = 0;
  unsigned seed = 1;
  const int shapes[][5] = {{37, 23, 4, 3, 768},  {64, 48, 8, 8, 768},    {5, 5, 5, 5, 256},  {1, 1, 1, 1, 0},   {33, 20, 2, 7, 0},
                           {100, 60, 3, 2, 768}, {100, 60, 3, 2, 65535}, {19, 7, 10, 4, 40}, {257, 1, 1, 1, 1}, {258, 1, 1, 1, 1},
                           {300, 40, 1, 1, 300}};
  for (auto &sh : shapes)
    for (int kind : {0, 1, 2, 3})
      bad += run_case(sh[0], sh[1], sh[2], sh[3], sh[4], kind, 0, kind ? 5 : 0, kind == 1 ? 2 : 5, kind, kind == 3, seed++);
  bad += run_case(67, 35, 32, 32, 5000, 0, 0, 3, 1, 1, false, seed++);
  for (int tables : {1, 2}) {
    bad += run_case(37, 23, 4, 3, 0, 0, tables, 3, 6, 1, false, seed++);
    bad += run_case(64, 48, 8, 8, 0, 0, tables, 0, 0, 0, true, seed++);
    bad += run_case(4096, 8, 4, 1, 0, 0, tables, 1, 2, 3, false, seed++);
  }
  bad += run_case(4096, 4, 32, 1, 768, 0, 0, 0, 0, 0, false, seed++);
  bad += run_case(4, 4096, 1, 32, 768, 0, 0, 3, 1, 2, false, seed++);
  bad += run_case(2048, 512, 1, 1, 768, 2, 0, 0, 0, 0, false, seed++);
  printf(bad ? "FAILED %d\n" : "all ok\n", bad);
  return bad != 0;
}
