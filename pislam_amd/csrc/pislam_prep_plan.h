// pislam_prep_plan.h — the host half of the pyramid build (pislam_pyramid_layout, pislam_pyramid_build_batch,
// the bilinear reductions; include/pislam_hip.h): the geometry of a reduction step, the level
// table, and the plan pislam_pyramid_build_batch makes once per call — what it refuses, the margins it zeroes, which
// kernel each reduction takes and, for the one-launch build, the workgroup ranges and band counters of every level.
// Plain C++ without a HIP type, so that it also compiles with a host compiler alone (tools/probes/prep_host_check.cpp);
// pislam_prep_kernels.h reads the same structs and constants.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/pislam_hip.h"

#if defined(__HIPCC__)
#define PP_HD __host__ __device__
#else
#define PP_HD
#endif

namespace pp {

// ---- a reduction step: N x N source pixels become M x M (Bilinear.h:28-30,153) ----
struct Reduction {
  int N, M;
  int blocks(int x) const { return (x + N - 1) / N; }    // blocks that cover x pixels
  int padded(int x) const { return blocks(x) * N; }      // pixels the reduction reads (Bilinear.h:32,155 padding)
  int written(int x) const { return blocks(x) * M; }     // pixels it writes: whole blocks
  int reduced(int x) const { return x * M / N; }         // size of the next level: round down (Bilinear.h:34-35,157-158)
};
// step code 1 = bilinear7_8; 2 (the builder: anything else) = bilinear13_16
PP_HD inline Reduction reduction(int step) { return step == 1 ? Reduction{8, 7} : Reduction{16, 13}; }

// k_bilinear4 loads 16 bytes per block row for four blocks at once: the last group's loads must stay in the row
inline bool quad_loads_fit(int nbx, int N, int vstep) { return (ptrdiff_t)((nbx + 3) / 4) * 4 * N <= vstep; }
// Does the 4-block kernel (k_bilinear4) apply?  Addresses are given modulo 16.
inline bool quad_kernel_applies(unsigned src_mod16, unsigned dst_mod16, int vstep_src, int vstep_dst, size_t stride_src,
                                size_t stride_dst, int nbx, int N) {
  return src_mod16 % 16 == 0 && dst_mod16 % 4 == 0 && vstep_src % 16 == 0 && vstep_dst % 4 == 0 && stride_src % 16 == 0 &&
         stride_dst % 4 == 0 && quad_loads_fit(nbx, N, vstep_src);
}

// ---- k_zero_margins (pislam_prep_kernels.h) ----
struct ZeroPlan {
  int nlevels, vstep;
  int row0[16], ww[16], wh[16], slot_rows[16];
};
constexpr int ZM_COLS = 32, ZM_ROWS = 16;

// ---- k_bilinear_chain (pislam_prep_kernels.h) ----
constexpr int CH_BAND = 16;
struct ChainPlan {
  int nlevels, vstep, batch, bands_per_frame;
  int groups;                  // ceil(batch / 8) groups of eight frames (frame = 8 g + b % 8)
  int wg0[17];                 // first workgroup of level l (1 .. nlevels-1), multiples of 8; wg0[nlevels] = grid size
  // (Launch order: level-major.  Ordering by diagonals d = g + l - 1 — group g's level l + 1 one step behind its level l, so
  //  that the small levels of the early groups run beside the big levels of the late ones instead of all at the end — was
  //  measured: 202 us per 64-frame build against 166: consumers then sit right behind their producers in the dispatch order,
  //  and a waiting workgroup holds a slot.)
  int wpf[16];                 // workgroups per frame of level l
  int kind[16];                // the reduction INTO level l: 1 = 7/8, 2 = 13/16
  int row0[16];                // pyramid row of level l
  int sw[16], sh[16];          // width / height of level l - 1 (the source of the reduction into level l)
  int nq[16], oh[16];          // level l: items per output row, output rows written
  int band0[16];               // index (within a frame's block) of level l's first band counter
};
// ctr: [batch][bands_per_frame] band counters (rounded up to a 128-byte line), then — every word on a 128-byte line of its
// own (CH_LINE dwords apart) — [0] sticky fault (a wait timed out / a frame met two XCDs), [1] shards complete,
// [2 .. 2 + CH_SHARDS) workgroups done per shard, [2 + CH_SHARDS ..) the XCD of each frame + 1 (0 = not yet known).  All
// zero between launches (the fault word: until the host has seen it).
// (Measured, 64 720p frames: ONE done counter next to the fault word every poller reads and the per-frame XCD words every
//  workgroup reads made the kernel 837 us; without the done counter 134 us — 12 500 returning atomics on a line that 12 500
//  other accesses want.  Hence the shards and the lines.)
constexpr int CH_LINE = 32, CH_SHARDS = 64;
PP_HD constexpr size_t chain_tail_ofs(size_t batch, size_t bands_per_frame) {
  return (batch * bands_per_frame + CH_LINE - 1) / CH_LINE * CH_LINE;
}
PP_HD constexpr size_t chain_words(size_t batch, size_t bands_per_frame, size_t groups) {
  return chain_tail_ofs(batch, bands_per_frame) + (2 + CH_SHARDS + 8 * groups) * CH_LINE;
}

// ---- pislam_pyramid_layout ----
inline int layout(int width, int height, int nlevels, const int32_t *steps, int vstep_min, pislam_level *levels, int32_t *vstep,
                  int32_t *rows) {
  if (width <= 0 || height <= 0 || nlevels < 1 || nlevels > 16 || !levels || (nlevels > 1 && !steps))
    return PISLAM_ERR_INVALID;
  int w = width, h = height, row = 0, maxcols = width;
  for (int l = 0; l < nlevels; l++) {
    int written = 0;                       // rows the reduction INTO this level writes (whole 7x7 / 13x13 blocks)
    if (l > 0) {
      if (steps[l - 1] != 1 && steps[l - 1] != 2) return PISLAM_ERR_INVALID;
      const Reduction r = reduction(steps[l - 1]);
      written = r.written(h);
      maxcols = std::max(maxcols, r.written(w));
      w = r.reduced(w);
      h = r.reduced(h);
    }
    if (w < 3 || h < 3) return PISLAM_ERR_INVALID;
    levels[l].width = w;
    levels[l].height = h;
    levels[l].row0 = row;
    levels[l].col0 = 0;
    // the slot holds the padding rows the next reduction reads (the larger block, whichever step follows) and every
    // row the reduction into this level writes
    row += std::max(reduction(2).padded(h), written);
  }
  if (vstep) *vstep = std::max(vstep_min, (maxcols + 15) / 16 * 16);
  if (rows) *rows = row;
  return PISLAM_OK;
}

// ---- pislam_pyramid_build_batch ----
constexpr const char *HOST_POINTERS = "the pyramid builder takes device pointers only";

// nullptr, or what is wrong with the flags and the arguments that can be judged without looking at the level table
inline const char *check_build_call(int nlevels, const int32_t *steps, const pislam_level *levels, const void *frames,
                                    const void *pyramids, int batch, int flags) {
  // (ABI 1 took `blur` = any non-zero value here: unknown bits are refused, not silently read as flags)
  if (flags & ~(PISLAM_BUILD_BLUR | PISLAM_BUILD_MARGINS_CLEAN | PISLAM_BUILD_CHECK_MARGINS)) return "unknown PISLAM_BUILD_* flag bits";
  if (!levels || !frames || !pyramids || batch <= 0 || nlevels < 1 || nlevels > 16 || (nlevels > 1 && !steps)) return "bad argument";
  return nullptr;
}

struct ReductionPlan {         // level l -> level l + 1
  int step;                    // its code
  size_t src_ofs, dst_ofs;     // byte offsets of the two levels in a pyramid
  int width, height;           // of the source level
  int ow, oh;                  // columns and rows written: whole blocks
  bool quad;                   // k_bilinear4 applies (else k_bilinear)
};

struct BuildPlan {
  const char *refusal;         // nullptr, or why the call is refused (PISLAM_ERR_INVALID); the rest is then undefined
  bool margins;                // the margins pass runs (zeroing or checking): Z is filled, else all zero
  ZeroPlan Z;
  ReductionPlan red[15];
  bool chain;                  // all reductions as one launch of k_bilinear_chain
  ChainPlan C;                 // filled as far as the chain stayed eligible, all zero if it was not wanted
  unsigned chain_grid;         // workgroups and counter words of that launch (0 without it)
  size_t chain_words;
};

// Arguments as check_build_call accepted them.  pyramids_mod16: the destination's address modulo 16; chain_wanted: the
// context asks for the one-launch build (it still needs three levels and k_bilinear4's fast path on every one of them).
inline BuildPlan make_build_plan(int nlevels, const int32_t *steps, const pislam_level *levels, int frame_vstep, size_t frame_stride,
                                 int batch, int vstep, int rows, size_t pyramid_stride, int flags, unsigned pyramids_mod16,
                                 bool chain_wanted) {
  BuildPlan P;
  memset(&P, 0, sizeof(P));
  auto refuse = [&P](const char *why) {
    P.refusal = why;
    return P;
  };
  for (int l = 0; l < nlevels; l++) {
    const Reduction r = l + 1 < nlevels ? reduction(steps[l]) : Reduction{1, 1};
    if (levels[l].col0 != 0 || r.padded(levels[l].width) > vstep || levels[l].row0 + r.padded(levels[l].height) > rows ||
        pyramid_stride < (size_t)rows * vstep)
      return refuse("level (with its bilinear padding) does not fit the pyramid buffer");
  }
  for (int l = 0; l + 1 < nlevels; l++) {           // whole output blocks must land inside the next level's slot
    const Reduction r = reduction(steps[l]);
    ReductionPlan &R = P.red[l];
    R.step = steps[l];
    R.src_ofs = (size_t)levels[l].row0 * vstep;
    R.dst_ofs = (size_t)levels[l + 1].row0 * vstep;
    R.width = levels[l].width, R.height = levels[l].height;
    R.ow = r.written(R.width), R.oh = r.written(R.height);
    R.quad = quad_kernel_applies(pyramids_mod16 + (unsigned)(R.src_ofs % 16), pyramids_mod16 + (unsigned)(R.dst_ofs % 16), vstep, vstep,
                                 pyramid_stride, pyramid_stride, r.blocks(R.width), r.N);
    const int slot_end = l + 2 < nlevels ? levels[l + 2].row0 : rows;
    if (R.ow > vstep || levels[l + 1].row0 + R.oh > slot_end)
      return refuse("a reduction's output blocks overrun the next level's slot (use pislam_pyramid_layout)");
  }
  if (levels[0].width > frame_vstep || frame_stride < (size_t)levels[0].height * frame_vstep) return refuse("frame buffer too small");
  // the rectangle of each slot the build rewrites: level 0, then every reduction's whole output blocks
  P.margins = !(flags & PISLAM_BUILD_MARGINS_CLEAN) || (flags & PISLAM_BUILD_CHECK_MARGINS);
  if (P.margins) {
    P.Z.nlevels = nlevels;
    P.Z.vstep = vstep;
    for (int l = 0; l < nlevels; l++) {
      P.Z.row0[l] = levels[l].row0;
      P.Z.slot_rows[l] = (l + 1 < nlevels ? levels[l + 1].row0 : rows) - levels[l].row0;
      P.Z.ww[l] = l ? P.red[l - 1].ow : levels[0].width;
      P.Z.wh[l] = l ? P.red[l - 1].oh : levels[0].height;
    }
  }
  P.chain = chain_wanted && nlevels >= 3;
  if (!P.chain) return P;
  ChainPlan &C = P.C;
  P.chain = pyramids_mod16 % 16 == 0 && vstep % 16 == 0 && pyramid_stride % 16 == 0;   // k_bilinear4's fast path, every level
  C.nlevels = nlevels;
  C.vstep = vstep;
  C.batch = batch;
  C.groups = (batch + 7) / 8;
  long wg = 0;
  int bands = 0;
  for (int l = 1; l < nlevels && P.chain; l++) {
    const Reduction r = reduction(steps[l - 1]);
    const ReductionPlan &R = P.red[l - 1];
    if (!quad_loads_fit(r.blocks(R.width), r.N, vstep)) P.chain = false;
    C.kind[l] = R.step;
    C.row0[l] = levels[l].row0;
    C.sw[l] = R.width;
    C.sh[l] = R.height;
    C.nq[l] = (r.blocks(R.width) + 3) / 4;
    C.oh[l] = R.oh;
    C.wpf[l] = (C.nq[l] * C.oh[l] + 255) / 256;
    C.wg0[l] = (int)wg;
    wg += 8L * C.wpf[l] * C.groups;                 // (frame = 8 g + b % 8: one XCD per frame, see the kernel)
    C.band0[l] = bands;
    bands += (C.oh[l] + CH_BAND - 1) / CH_BAND;
  }
  C.row0[0] = levels[0].row0;
  C.bands_per_frame = bands;
  C.wg0[nlevels] = (int)wg;
  if (wg > 0x3fffffffL) P.chain = false;
  if (P.chain) {
    P.chain_grid = (unsigned)wg;
    P.chain_words = chain_words((size_t)batch, (size_t)bands, (size_t)C.groups);
  }
  return P;
}

}  // namespace pp
