// pislam_clahe_kernels.h — contrast-limited adaptive histogram equalisation (pislam_clahe_*; include/pislam_hip.h,
// DESIGN.md section 5.5): the step between pislam_warp_batch and pislam_pyramid_build_batch.  Integers only; the
// statement in the header is the contract.
//
// Two kernels, no workspace (the caller owns the tables):
//   k_clahe_luts   one workgroup per (tile, frame): the tile's histogram of the reflect-101 extended frame, counted
//                  into one LDS sub-histogram per wave, then clip, closed-form redistribution, a 256-entry scan and
//                  the table, one bin per thread.
//   k_clahe_apply  one workgroup per piece of a blend cell (the rectangle between neighbouring tile centres, half
//                  cells at the frame edges): exactly four tables, uniform tile indices, four pixels per lane and step.
// Both walk rows in "slots": the aligned dwords that cover a span of columns [c0, c1) of one row.  A slot that lies
// wholly inside the span is one dword load; the ragged ends are bytes.  Nothing outside [c0, c1) is read, so nothing
// outside the width x height rectangle is, row padding included.  A reflected part of a tile is just another span of
// the same row (a histogram does not care about order).
//
// The first part (limits, geometry, argument checks) is plain C++ without a HIP type.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define PC_HD __host__ __device__
#else
#define PC_HD
#endif

namespace pc {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_DIM = 4096, MAX_TILES = 32, MAX_CLIP_Q8 = 65535;
constexpr int64_t MAX_AREA = 1 << 20;
constexpr int APPLY_PX = 8192;                 // pixels per apply workgroup (a VGA 8 x 8 blend cell, 80 x 60, is one)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// nullptr, or what is wrong with a pislam_clahe_params
inline const char *check_params(int width, int height, int tiles_x, int tiles_y, int clip_q8) {
  if (width < 1 || width > MAX_DIM || height < 1 || height > MAX_DIM) return "width and height must be 1..4096";
  if (tiles_x < 1 || tiles_x > std::min(MAX_TILES, width)) return "tiles_x must be 1..min(32, width)";
  if (tiles_y < 1 || tiles_y > std::min(MAX_TILES, height)) return "tiles_y must be 1..min(32, height)";
  if ((int64_t)cdiv(width, tiles_x) * cdiv(height, tiles_y) > MAX_AREA) return "a tile may hold at most 2^20 pixels";
  if (clip_q8 < 0 || clip_q8 > MAX_CLIP_Q8) return "clip_q8 must be 0..65535";
  return nullptr;
}

// first column of blend cell c along an axis of tile size t: the first x with floor((2 x - t) / (2 t)) == c - 1
PC_HD inline int cell_start(int c, int t) { return c ? (t * (2 * c - 1) + 1) >> 1 : 0; }

// blend cells that hold a pixel along an axis of n pixels (at most tiles + 1)
inline int cell_count(int n, int tiles, int t) {
  int c = 1;
  while (c <= tiles && cell_start(c, t) < n) c++;
  return c;
}

struct Args {
  const uint8_t *src;
  size_t src_stride;
  uint8_t *dst;
  size_t dst_stride;
  uint8_t *luts;                               // [batch][tiles_y][tiles_x][256]
  int32_t src_vstep, dst_vstep, width, height, tiles_x, tiles_y, tw, th;
  uint32_t area, clip;                         // clip == 0: no clipping
  int32_t cells_x, cells_y, rows_per_wg, chunks;
  uint32_t d;                                  // 4 * tw * th
  float inv_d;
};

// (params as check_params accepted them)
inline Args geometry(int width, int height, int tiles_x, int tiles_y, int clip_q8) {
  Args a{};
  a.width = width, a.height = height, a.tiles_x = tiles_x, a.tiles_y = tiles_y;
  a.tw = cdiv(width, tiles_x), a.th = cdiv(height, tiles_y);
  a.area = (uint32_t)a.tw * (uint32_t)a.th;
  a.clip = clip_q8 ? (uint32_t)std::max<int64_t>(((int64_t)clip_q8 * (int64_t)a.area) >> 16, 1) : 0u;
  a.cells_x = cell_count(width, tiles_x, a.tw), a.cells_y = cell_count(height, tiles_y, a.th);
  a.rows_per_wg = std::max(1, std::min(a.th, APPLY_PX / a.tw));
  a.chunks = cdiv(a.th, a.rows_per_wg);
  a.d = 4u * a.area;
  a.inv_d = (float)(1.0 / (double)a.d);
  return a;
}

struct Range {
  uintptr_t p;
  size_t n;
};
inline bool overlap(Range a, Range b) { return a.n && b.n && a.p < b.p + b.n && b.p < a.p + a.n; }
inline Range frames_range(const void *p, int width, int height, int vstep, size_t stride, int batch) {
  return Range{(uintptr_t)p, (size_t)(batch - 1) * stride + (size_t)(height - 1) * (size_t)vstep + (size_t)width};
}

// nullptr, or what is wrong with the per-call arguments (pointer kinds are the caller's to check).  src, dst or luts
// may be NULL where the call does not use them (vstep 0 then).
inline const char *check_call(int width, int height, size_t lut_bytes, const void *src, int src_vstep, size_t src_stride,
                              const void *dst, int dst_vstep, size_t dst_stride, const void *luts, int batch, bool use_src,
                              bool use_dst) {
  if (batch < 0) return "negative batch";
  if (use_src && src_vstep < width) return "src_vstep must be at least width";
  if (use_dst && dst_vstep < width) return "dst_vstep must be at least width";
  if (batch == 0) return nullptr;
  if ((use_src && !src) || (use_dst && !dst) || !luts) return "null pointer";
  const Range s = use_src ? frames_range(src, width, height, src_vstep, src_stride, batch) : Range{0, 0};
  const Range d = use_dst ? frames_range(dst, width, height, dst_vstep, dst_stride, batch) : Range{0, 0};
  const Range l{(uintptr_t)luts, (size_t)batch * lut_bytes};
  const bool in_place = use_src && use_dst && src == dst && src_vstep == dst_vstep && src_stride == dst_stride;
  if (!in_place && overlap(s, d)) return "src and dst overlap (only dst == src with the same steps is allowed)";
  if (overlap(s, l) || overlap(d, l)) return "luts overlaps the frames";
  return nullptr;
}

#if defined(__HIPCC__)

// A walk over rows x slots, 256 threads abreast: thread t starts at item t and advances by THREADS without dividing.
struct Walk {
  int r, s, dr, ds, sp;
  __device__ Walk(int slots_per_row) : sp(slots_per_row) {
    r = (int)threadIdx.x / sp, s = (int)threadIdx.x - r * sp;
    dr = THREADS / sp, ds = THREADS - dr * sp;
  }
  __device__ void next() {
    r += dr, s += ds;
    if (s >= sp) s -= sp, r++;
  }
};

// slots that cover n columns at any alignment (0 for an empty span)
__device__ inline int slots_of(int n) { return n > 0 ? (n + 6) >> 2 : 0; }

// The four bytes of a dword into a wave's sub-histogram.  COMBINE adds equal bytes of the dword in one atomic: on a
// constant tile, where every lane of every wave hits one bin, that is a quarter of the serialised LDS adds.
template <bool COMBINE>
__device__ inline void count4(uint32_t *h, uint32_t w) {
  const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
  if (!COMBINE) {
    atomicAdd(&h[b0], 1u), atomicAdd(&h[b1], 1u), atomicAdd(&h[b2], 1u), atomicAdd(&h[b3], 1u);
    return;
  }
  const bool e10 = b1 == b0, e20 = b2 == b0, e30 = b3 == b0, e21 = b2 == b1, e31 = b3 == b1, e32 = b3 == b2;
  atomicAdd(&h[b0], 1u + e10 + e20 + e30);
  if (!e10) atomicAdd(&h[b1], 1u + e21 + e31);
  if (!e20 && !e21) atomicAdd(&h[b2], 1u + e32);
  if (!e30 && !e31 && !e32) atomicAdd(&h[b3], 1u);
}

__device__ inline uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

template <bool COMBINE>
__global__ __launch_bounds__(THREADS) void k_clahe_luts(const Args a) {
  __shared__ uint32_t hist[WAVES][256];
  __shared__ uint32_t excess[WAVES], total[WAVES];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
  const uint8_t *s = a.src + (size_t)blockIdx.y * a.src_stride;
#pragma unroll
  for (int w = 0; w < WAVES; w++) hist[w][tid] = 0;
  __syncthreads();

  // The tile's columns of the extended frame: [x0, x0 + tw) below `width` as they are, the rest reflected, which is the
  // span [2 (width - 1) - (x0 + tw - 1), 2 (width - 1) - max(x0, width)] of the same row.
  const int x0 = tx * a.tw, x1 = x0 + a.tw;
  const int a0 = x0, a1 = min(x1, a.width);
  const int nb = max(x1 - max(x0, a.width), 0), b0 = 2 * (a.width - 1) - (x1 - 1), b1 = b0 + nb;
  const int sa = slots_of(a1 - a0), sb = slots_of(nb);
  uint32_t *h = hist[wave];
  for (Walk k(sa + sb); k.r < a.th; k.next()) {
    const int ey = ty * a.th + k.r, ry = ey < a.height ? ey : 2 * (a.height - 1) - ey;
    const bool first = k.s < sa;
    const int c0 = first ? a0 : b0, c1 = first ? a1 : b1;
    const uint8_t *row = s + (size_t)ry * (size_t)a.src_vstep;
    const int o = c0 - (int)((uintptr_t)(row + c0) & 3) + 4 * (first ? k.s : k.s - sa);
    if (o >= c0 && o + 4 <= c1) {
      count4<COMBINE>(h, *(const uint32_t *)(row + o));
    } else {
      for (int q = 0; q < 4; q++)
        if (o + q >= c0 && o + q < c1) atomicAdd(&h[row[o + q]], 1u);
    }
  }
  __syncthreads();

  // one bin per thread from here on
  uint32_t hv = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) hv += hist[w][tid];
  if (a.clip) {
    const uint32_t over = wave_sum(hv > a.clip ? hv - a.clip : 0u);
    if (lane == 0) excess[wave] = over;
    __syncthreads();
    uint32_t ex = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) ex += excess[w];
    hv = min(hv, a.clip) + (ex >> 8);
    const uint32_t res = ex & 255u;
    if (res) {
      const uint32_t step = 256u / res, v = (uint32_t)tid;     // (res <= 255: step >= 1)
      if (v % step == 0 && v / step < res) hv++;
    }
  }
  uint32_t cdf = hv;                            // inclusive scan: within the wave, then the waves before it
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(cdf, d, 64);
    if (lane >= d) cdf += t;
  }
  if (lane == 63) total[wave] = cdf;
  __syncthreads();
  for (int w = 0; w < wave; w++) cdf += total[w];
  // 255 * cdf + area / 2 < 2^28 + 2^19: 32 bits hold it; one division per thread and tile
  const uint32_t lut = min(255u, (255u * cdf + (a.area >> 1)) / a.area);
  uint8_t *out = a.luts + ((size_t)blockIdx.y * (size_t)(a.tiles_x * a.tiles_y) + blockIdx.x) * 256;
  out[tid] = (uint8_t)lut;
}

// One output pixel.  t holds L[ty1][tx1][v], L[ty1][tx2][v], L[ty2][tx1][v], L[ty2][tx2][v] from the low byte up.
//
// The division.  n = S + D / 2 with S <= 255 D and D = 4 tw th <= 2^22, so n < 2^30 and the quotient is at most 255.
// q0 = trunc(float(n) * inv_d): the conversion of n, the host's rounding of 1 / D and the product are each off by at
// most 2^-24 relative, so the estimate is within 256 * 2^-22 = 2^-14 of n / D and q0 is the true quotient or one off
// either way.  The remainder r = n - q0 * D (|r| < 2 D, exact in 32 bits; q0 <= 256 and D < 2^24 fit the 24-bit
// multiply) says which: r < 0 takes one off, r >= D adds one.  The result is floor(n / D) for every n the limits admit.
__device__ inline uint32_t blend(uint32_t t, int wx1, int wx2, int wy1, int wy2, uint32_t d, float inv_d) {
  const uint32_t top = __umul24(wx1, t & 255u) + __umul24(wx2, (t >> 8) & 255u);
  const uint32_t bot = __umul24(wx1, (t >> 16) & 255u) + __umul24(wx2, t >> 24);
  const uint32_t n = __umul24(wy1, top) + __umul24(wy2, bot) + (d >> 1);   // top, bot < 2^21, wy <= 2^13, n < 2^30
  uint32_t q = (uint32_t)((float)n * inv_d);
  const int r = (int)n - (int)__umul24(q, d);
  if (r < 0) q--;
  else if (r >= (int)d) q++;
  return q;
}

template <bool LDS_TABLES>
__global__ __launch_bounds__(THREADS) void k_clahe_apply(const Args a) {
  __shared__ uint32_t quad[256];
  const int tid = (int)threadIdx.x;
  const int chunk = (int)(blockIdx.x % (unsigned)a.chunks), cell = (int)(blockIdx.x / (unsigned)a.chunks);
  const int cx = cell % a.cells_x, cy = cell / a.cells_x;
  const int xs = cell_start(cx, a.tw), xe = min(cell_start(cx + 1, a.tw), a.width);
  const int ys = cell_start(cy, a.th) + chunk * a.rows_per_wg;
  const int ye = min(min(cell_start(cy + 1, a.th), a.height), ys + a.rows_per_wg);
  if (ys >= ye) return;                         // (a half cell at the frame edge has fewer pieces; uniform)
  const int tx1 = max(cx - 1, 0), tx2 = min(cx, a.tiles_x - 1), ty1 = max(cy - 1, 0), ty2 = min(cy, a.tiles_y - 1);
  const uint8_t *L = a.luts + (size_t)blockIdx.y * (size_t)(a.tiles_x * a.tiles_y) * 256;
  const uint8_t *l11 = L + (size_t)(ty1 * a.tiles_x + tx1) * 256, *l12 = L + (size_t)(ty1 * a.tiles_x + tx2) * 256;
  const uint8_t *l21 = L + (size_t)(ty2 * a.tiles_x + tx1) * 256, *l22 = L + (size_t)(ty2 * a.tiles_x + tx2) * 256;
  if (LDS_TABLES) {                             // the four tables interleaved: one LDS dword per pixel
    quad[tid] = (uint32_t)l11[tid] | ((uint32_t)l12[tid] << 8) | ((uint32_t)l21[tid] << 16) | ((uint32_t)l22[tid] << 24);
    __syncthreads();
  }
  auto look = [&](uint32_t v) -> uint32_t {
    if (LDS_TABLES) return quad[v];
    return (uint32_t)l11[v] | ((uint32_t)l12[v] << 8) | ((uint32_t)l21[v] << 16) | ((uint32_t)l22[v] << 24);
  };
  const uint8_t *s = a.src + (size_t)blockIdx.y * a.src_stride;
  uint8_t *dp = a.dst + (size_t)blockIdx.y * a.dst_stride;
  // wx2 = 2 x - tw - 2 tw (cx - 1) = 2 x - kx, wx1 = 2 tw - wx2; likewise in y
  const int kx = a.tw * (2 * cx - 1), ky = a.th * (2 * cy - 1), tw2 = 2 * a.tw, th2 = 2 * a.th;
  for (Walk k(slots_of(xe - xs)); k.r < ye - ys; k.next()) {
    const int y = ys + k.r, wy2 = 2 * y - ky, wy1 = th2 - wy2;
    const uint8_t *srow = s + (size_t)y * (size_t)a.src_vstep;
    uint8_t *drow = dp + (size_t)y * (size_t)a.dst_vstep;
    const int o = xs - (int)((uintptr_t)(srow + xs) & 3) + 4 * k.s;
    if (o >= xs && o + 4 <= xe) {
      const uint32_t w = *(const uint32_t *)(srow + o);
      uint32_t out = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int wx2 = 2 * (o + q) - kx;
        out |= blend(look((w >> (8 * q)) & 255u), tw2 - wx2, wx2, wy1, wy2, a.d, a.inv_d) << (8 * q);
      }
      if (((uintptr_t)(drow + o) & 3) == 0) {
        *(uint32_t *)(drow + o) = out;
      } else {
        for (int q = 0; q < 4; q++) drow[o + q] = (uint8_t)(out >> (8 * q));
      }
    } else {
      for (int q = 0; q < 4; q++) {
        const int x = o + q;
        if (x < xs || x >= xe) continue;
        const int wx2 = 2 * x - kx;
        drow[x] = (uint8_t)blend(look(srow[x]), tw2 - wx2, wx2, wy1, wy2, a.d, a.inv_d);
      }
    }
  }
}

#endif  // __HIPCC__

}  // namespace pc
