// pislam_frontend_plan.h — the host half of the front end (pislam_orb_frontend_batch, pislam_frontend_reserve,
// pislam_debug_build_plan; include/pislam_hip.h, DESIGN.md sections 5.1 and 5.3): the integer options of a context, the
// plan structs the kernels of pislam_fused_kernels.h take by value, and the planner that fills them — what a batch call is
// refused for, its strip plan, sub-batches, bucket selection plan and unit table, every LDS size, and the invariants the
// kernels rely on.  Plain C++ without a HIP type or a context, so that it also compiles with a host compiler alone
// (tools/probes/frontend_host_check.cpp); pislam_fused_kernels.h reads the same structs and constants.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/pislam_hip.h"

#if defined(__HIPCC__)
#define FP_HD __host__ __device__
#else
#define FP_HD
#endif

// development switch (tools/ab_build.sh -D...): the default is the product
#ifndef PISLAM_ORB_PITCH_DW
#define PISLAM_ORB_PITCH_DW 12   // dwords per ORB patch row in LDS (12 = round 1-5: 48-byte rows skewed by a dword per 8 rows)
#endif

namespace pf {

// ---- the strip plan (pf::k_fused_strips, k_fused_overflow, k_gather, k_gather_orb, k_frame take a FusedParams by value) ----
constexpr int MAX_ORDER = 160;              // runs per pyramid the launch-order table holds
constexpr int MAX_LEVELS = 24;              // plan entries: levels, wide ones cut into x-tiles (see FusedLevel::gn)
constexpr int WAVES = 4;               // waves per strip workgroup
constexpr int NT = WAVES * 64;         // threads per strip workgroup
constexpr int QCAP_G = 128;            // 4-pixel groups that passed the SAD prefilter (< 64 before a <= 64 push)
constexpr int QCAP_F = 192;            // FAST candidates (< 64 before a <= 128 half-push)
constexpr int QCAP = QCAP_G + QCAP_F;  // dwords of private queue space per wave
constexpr int QH_SHARED = 1024;        // workgroup-shared queue of corners awaiting their Harris score (a 28-row
                                       // strip of a textured photo holds up to ~900: the reference's demo image)
constexpr int QN_SHARED = 512;         // plain layout only: queue of pixels with a non-zero score (NMS candidates)
constexpr int QS_SHARED = 256;         // survivors of one strip awaiting their rank
constexpr int SHARED_Q = QH_SHARED + QN_SHARED;
constexpr int NMS_SCRATCH = 3 * QS_SHARED;   // dwords: survivors, their keys (then ranks), bucket keep flags (in the idle per-wave queues)
static_assert(NMS_SCRATCH <= WAVES * QCAP, "NMS scratch must fit the per-wave queue area");
static_assert(QS_SHARED <= NT, "one survivor per thread (ranks are held in a register across a barrier)");

struct FusedLevel {
  int w, h;          // level size
  int row0, col0;    // position in the stacked pyramid
  int R;             // strip height (even)
  int nstrips;       // strips in this level
  int strip0;        // index of the level's first strip within the pyramid
  int slot0;         // staging slot (in keypoints) of the level's first strip
  int nbx;           // 2x2 blocks per block-row
  int xend;          // one past the last classified column (Fast.h:61,149)
  int pitch;         // LDS SCORE tile pitch in bytes (multiple of 16): the score tile spans the full level width
  int tpitch;        // LDS IMAGE tile pitch in bytes (multiple of 16) = classified columns + halo
  int nruns, run0;   // runs (= workgroups) of this level: run_len consecutive strips each
  int apad;          // ALIAS layout: bytes between the per-wave queues and the image tile (multiple of 16)
  int qh;            // ALIAS layout: entries of the shared corner queue (>= QH_SHARED: the plan hands the LDS
                     // a level's narrower tiles leave under the residency budget to its queue)
  int tbytes;        // plain layout: bytes reserved for the image tile = max((R+10)*tpitch, the scan
                     // fallbacks' survivor / per-cell buffers — larger only with narrow x-tiles)
  uint32_t vpr_recip; // ceil(2^32 / (tpitch/16)): row = umulhi(i, vpr_recip) for a vector index i < 2^16
  uint32_t tp_recip;  // ceil(2^32 / tpitch): tile row of a byte offset k < 2^16 into the tile = umulhi(k, tp_recip)
  // A plan entry is a whole pyramid level, or one X-TILE of a wide level: a column range handled by its own
  // workgroups like a level of its own (w / col0 describe the tile plus a halo of real image columns in place
  // of the border), so that the LDS footprint — and with it the number of resident workgroups — does not grow
  // with the level width.  Tiles classify and score a few columns beyond the blocks they own (the NMS of a
  // boundary block reads its neighbours' scores), emit only the blocks whose origin lies in [ex0, ex1), and
  // k_gather_orb merges the tiles' per-strip lists back into the level's block-raster order.
  int ex0, ex1;      // block origins (entry-relative x) this entry emits: [ex0, ex1)   (whole level: [B, w-B))
  int xscore;        // entry-relative x of the level's w-B: columns at / beyond it keep 0xff (Fast.h:172)
  int gfirst, gn;    // the entries gfirst .. gfirst+gn-1 are the tiles of this entry's level (same R, nstrips)
};

struct FusedParams {
  int nlevels, strips_per_pyr, slots_per_pyr;
  int runs_per_pyr, run_len;   // a workgroup walks run_len consecutive strips of one level (see k_fused_strips)
  int vstep, rows, border, thr;
  int32_t hthr;
  int batch;
  int lbs, limit;    // fastExtract logBucketSize (0 = none; fused path: 2..5) and bucketLimit
  int words;         // orbCompute words (descriptor dwords per keypoint)
  int orb_in_strip;  // ALIAS + 16-byte-aligned kernels: strips describe their own keypoints (strip_body phase E)
  int order_n;       // > 0: the launch order of a pyramid's runs is order[] (longest first)
  int dump_score;    // debug: also write the score tile to the HBM score map
  int ablate;        // profiling only: bit0 stop after staging, bit1 pretest only, bit2 no Harris, bit3 no NMS
  FusedLevel lv[MAX_LEVELS];
  // Runs of one pyramid in launch order, longest (estimated) first, so that the short ones fill the tail of
  // the launch (longest-processing-time-first list scheduling); plans with more runs keep entry order.
  uint32_t order[MAX_ORDER];                       // entry << 16 | run inside the entry (dwords: scalar loads)
};

// ---- the LDS patch of the gather + ORB kernel (pf::k_gather_orb) ----
constexpr int OWAVES = 4;                           // waves per k_gather_orb workgroup
// One 48-byte window per patch row.  Default layout (PISLAM_ORB_PITCH_DW 12): rows 12 dwords apart, skewed by one dword per
// 8 rows — the 9 row reads of the moments (lane = row) are conflict-free (a pitch of 12 dwords alone puts rows r, r+8, r+16,
// r+24 on the same banks), and so are the three dword stores that park a 12-byte piece (lanes = (row, piece): 12 row + 3
// piece + i hits 32 different banks for the 8 rows x 4 pieces of a half-wave).  With the 16-byte chunks of rounds 2-5 the
// four stores of a chunk fell on 8 banks (4-way: 5.6 M of the kernel's 13.8 M conflict cycles per launch, 1.5 M now); rows 13
// dwords apart (PISLAM_ORB_PITCH_DW 13, round 6) cured that at the price of 1 KB more LDS per workgroup and were not kept.
constexpr int ORB_PITCH = 4 * PISLAM_ORB_PITCH_DW;
FP_HD constexpr int orb_row_ofs(int r) { return PISLAM_ORB_PITCH_DW == 12 ? r * 48 + 4 * (r >> 3) : r * ORB_PITCH; }
// 31 rows (the idle lane's row 31 reads harmless bytes of whatever follows) + slack for the byte shift, a multiple of 16
constexpr int ORB_PATCH_BYTES = PISLAM_ORB_PITCH_DW == 12 ? 32 * 48 + 32 : (31 * ORB_PITCH + 4 + 15) / 16 * 16;

// ---- the bucket selection pass (pf::k_bucket_select) ----
struct SelectPlan {
  int nlevels, lbs, limit, border;
  int units_per_pyr, uslots_per_pyr;
  int row0[16], col0[16], h[16];      // the level (not its tiles)
  int g0[16], gn[16];                 // its plan entries in the strip plan
  int unit0[16], nunits[16];          // its units (cell rows)
  int cap[16], uslot0[16];            // slots per unit (buckets x limit), first slot of the level
  int nb_max;                         // most buckets of any level (the dense path's LDS counters: 2 x nb_max dwords per wave)
};
// (k_bucket_select takes FusedParams + SelectPlan + four pointers by value: the kernel-argument segment holds 4 KiB)
static_assert(sizeof(FusedParams) + sizeof(SelectPlan) + 5 * sizeof(void *) <= 4096, "k_bucket_select's arguments exceed the 4 KiB kernarg segment");
constexpr int SEL_WAVES = 4;
constexpr int SEL_NB = 1024;                         // buckets per cell row the dense path's LDS counters hold (the host checks)
// The unit table (host-built, one record of SEL_REC dwords per unit = (level, cell row)): everything the fast path needs to
// know about a unit arrives with ONE scalar load — until round 5 a wave found its level by a loop of dependent scalar
// loads over the plan, and the strips overlapping its rows by two software divisions per x-tile with more plan loads
// in between: the kernel is a single round of resident waves, its duration IS that chain.
//   [0] lists overlapping the unit (0xffffffff: more than SEL_ML: the generic path), [1] level, [2] cell row,
//   [3] first output slot (uslot0 + cell row * cap), [4] row0 + B, [5] col0 + B (stacked coordinates of the level's first
//   block origin), [8 ..] staging slot of list j, [16 ..] strip-count index of list j.
constexpr int SEL_REC = 24, SEL_ML = 6;

// Small shared state of the gather + ORB role, carved from the FRONT of the dynamic LDS (not static: the strip
// role's 5-workgroups-per-CU budget has no room for another 300 static bytes).
struct OrbShared {
  uint32_t wsum[4];
  uint32_t carry, ntodo, flag, pad;
  uint8_t rtab[256];                                // vrecpe estimate table (256 threads: one entry each)
};
FP_HD constexpr size_t orb_lds_bytes(int strips_per_pyr, size_t per_max) {
  return sizeof(OrbShared) + (size_t)OWAVES * 2 * ORB_PATCH_BYTES + sizeof(uint32_t) * (((size_t)strips_per_pyr + 1 + 3) & ~(size_t)3) +
         sizeof(uint32_t) * (((size_t)strips_per_pyr + 3) & ~(size_t)3) +   // where each strip's list starts in the staging buffer
         sizeof(uint32_t) * 2 * per_max;            // keypoints to describe here and their final positions
}

// pf::k_frame's hand-over counters (the kernel's comment says what each word holds)
constexpr int FRAME_SYNC_PYR = 8, FRAME_SYNC_DONE = 8, FRAME_SYNC_POISON = 9, FRAME_SYNC_WORDS = 12;

}  // namespace pf

namespace fp {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

constexpr int MAX_SUB = 16;             // most sub-batches of a fused batch call (option "sub_batches")

// ---- the integer options of a context (pislam_ctx_set_option), and the two facts about the device the planner reads ----
struct Options {
  int num_cus = 0;
  int lanes_in_flight = 1;   // > 1: this context is a lane of a pislam_pipeline of that depth (other batches' kernels share the GPU)
  int frame_test = 0;        // test hook: bit 0 = one strip workgroup skips its release, bits 8.. = log2 poll limit
  int build_chain = 0;       // 1: pislam_pyramid_build_batch runs levels 1.. as ONE launch (pp::k_bilinear_chain); 0 (default): one
                             // launch per level — measured faster: 150 against 166 us per 64 720p frames (docs/experiments.md)
  int pipeline = 0;          // 0 auto, 1 staged (one launch group per level), 2 fused strips
  int dump_score = 0;        // fused pipeline: also materialise the score map (parity hook)
  int strip_rows = 0;        // fused pipeline: strip height override (0 = heuristic)
  int ablate = 0;            // profiling only: skip phases of the fused kernel (results invalid)
  int bucket_round_up = 0;   // profiling: bucket mode always rounds the strip height up to whole bucket rows (round-2 rule)
  int orb_chunks = 0;        // fused pipeline: workgroups per pyramid in k_gather_orb (0 = heuristic)
  int repeat_strips = 1;     // profiling: launch the strip kernel n times inside the stage-0 event bracket
  int alias = 1;             // fused pipeline: score tile laid over the dead image rows (0 = separate tiles)
  int run_len = 0;           // fused pipeline: strips per workgroup run (0 = default, 1 = independent strips)
  int lds_pad = 0;           // profiling only: extra dynamic LDS bytes per strip workgroup
  int wgs_per_cu = 0;        // fused pipeline: if > 0, size strip heights for this many workgroups per CU
  int strip_px = 16384;      // profiling: pixels per strip the height heuristic aims at
  int strip_rows_max = 0;    // profiling: upper bound of the heuristic strip height (0 = rule in build_fused_plan)
  int run_order = 1;         // fused pipeline: launch a pyramid's runs longest first (0: in entry order)
  int tile_cols = 0;         // fused pipeline: levels with more classified columns are cut into x-tiles (0 = 704, < 0 = never)
  int bucket_select = 1;     // fused pipeline, buckets: 1 = strips as without buckets + pf::k_bucket_select (default), 0 = the strips select (round 1-3)
  int frame = 1;             // fused pipeline: small batches run as ONE launch (pf::k_frame): 1 = batches of 1 or 2 pyramids, n = up to n (<= 8), 0 = never
  int orb_in_strip = 0;      // fused pipeline: 1 = strips describe their own keypoints (measured slower: DESIGN.md §8), 0 = k_gather_orb describes all
  int match_mfma = 1;        // matcher on the matrix cores (0: the VALU popcount kernel)
  int warp_direct = 0;       // mesh warp: 1 = every tile takes the direct path (taps from global memory), 0 = by the tile plan
  int clahe_combine = 1;     // CLAHE table kernel: 1 = equal bytes of a lane's dword share one LDS atomic, 0 = one atomic per pixel
  int clahe_lut_global = 0;  // CLAHE apply kernel: 1 = the four tables are read from global memory per pixel, 0 = staged in LDS
  int dist_rccl_single = 0;  // test hook: pislam_dist_init(world = 1) still creates a (1-rank) RCCL communicator
  int sub_batches = 1;       // 1 = one launch group (default), n = n sub-batches, 0 = by bytes per sub-batch
  int sub_mb = 0;            // auto rule: target MiB of pyramids per sub-batch (0 = default)
};

// The options that are one int member: accepted range [lo, hi] with the message of a value outside it (no message: every
// value is accepted), then what is stored (no normaliser: the value itself).
struct OptionDef {
  const char *key;
  int Options::*member;
  int lo, hi;
  const char *range_error;
  int (*stored)(int);
};
inline int as_flag(int v) { return v != 0; }
inline int at_least_0(int v) { return std::max(0, v); }
inline const OptionDef OPTIONS[] = {
    {"pipeline", &Options::pipeline, 0, 2, "pipeline must be 0 (auto), 1 (staged) or 2 (fused)", nullptr},
    {"dump_score", &Options::dump_score, 0, 0, nullptr, as_flag},
    {"repeat_strips", &Options::repeat_strips, 1, 64, "repeat_strips must be 1..64", nullptr},
    {"alias", &Options::alias, 0, 0, nullptr, as_flag},
    {"run_len", &Options::run_len, 0, 64, "run_len must be 0 (default) .. 64", nullptr},
    {"lds_pad", &Options::lds_pad, 0, 0, nullptr, at_least_0},
    {"wgs_per_cu", &Options::wgs_per_cu, 0, 8, "wgs_per_cu must be 0..8", nullptr},
    {"match_mfma", &Options::match_mfma, 0, 0, nullptr, as_flag},
    {"warp_direct", &Options::warp_direct, 0, 1, "warp_direct must be 0 or 1", nullptr},
    {"clahe_combine", &Options::clahe_combine, 0, 1, "clahe_combine must be 0 or 1", nullptr},
    {"clahe_lut_global", &Options::clahe_lut_global, 0, 1, "clahe_lut_global must be 0 or 1", nullptr},
    {"run_order", &Options::run_order, 0, 0, nullptr, as_flag},
    {"strip_px", &Options::strip_px, 0, 0, nullptr, [](int v) { return std::max(4096, v); }},
    {"strip_rows_max", &Options::strip_rows_max, 0, 0, nullptr, [](int v) { return v <= 0 ? 0 : std::max(16, std::min(64, v & ~1)); }},
    // 0: never one launch; 1 (default): batches of 1 or 2 pyramids; n = 2..8: batches of up to n
    {"frame", &Options::frame, 0, 8, "frame must be 0..8", nullptr},
    // test hook of the one-launch path's bounded wait (see pf::k_frame `test`)
    {"frame_test", &Options::frame_test, 0, 0, nullptr, nullptr},
    // pyramid build: 1 = levels 1.. in ONE launch (pp::k_bilinear_chain), 0 (default) one launch per level
    {"build_chain", &Options::build_chain, 0, 0, nullptr, as_flag},
    {"orb_in_strip", &Options::orb_in_strip, 0, 0, nullptr, as_flag},
    {"bucket_select", &Options::bucket_select, 0, 0, nullptr, as_flag},
    {"dist_rccl_single", &Options::dist_rccl_single, 0, 0, nullptr, as_flag},
    {"bucket_round_up", &Options::bucket_round_up, 0, 0, nullptr, as_flag},
    {"orb_chunks", &Options::orb_chunks, 0, 1024, "orb_chunks must be 0..1024", nullptr},
    {"sub_batches", &Options::sub_batches, 0, MAX_SUB, "sub_batches must be 0 (auto) .. 16", nullptr},
    {"sub_mb", &Options::sub_mb, 0, 0, nullptr, at_least_0},
    {"ablate", &Options::ablate, 0, 0, nullptr, nullptr},
};

// Sets option `key`.  False: `key` is no option of this struct.  True: *refusal is nullptr and the value is stored, or says
// why it is not.
inline bool set_option(Options &o, const char *key, int value, const char **refusal) {
  *refusal = nullptr;
  for (const OptionDef &d : OPTIONS) {
    if (strcmp(key, d.key)) continue;
    if (d.range_error && (value < d.lo || value > d.hi)) *refusal = d.range_error;
    else o.*d.member = d.stored ? d.stored(value) : value;
    return true;
  }
  // the two whose range is no interval
  if (!strcmp(key, "tile_cols")) {
    if (value > 0 && value < 64) *refusal = "tile_cols must be 0 (default), < 0 (never) or >= 64";
    else o.tile_cols = value;
  } else if (!strcmp(key, "strip_rows")) {
    if (value < 0 || value > 64 || (value & 1)) *refusal = "strip_rows must be even, 0..64";
    else o.strip_rows = value;
  } else {
    return false;
  }
  return true;
}

// ---- what a batch call is refused for before anything is planned ----
// nullptr, or why (the caller reports PISLAM_ERR_INVALID with this text): the convention of every function here that refuses.
inline const char *check_params(const pislam_frontend_params *p, const pislam_level *lv, int batch) {
  if (!p || !lv) return "null params";
  if (batch <= 0) return "batch must be positive";
  if (p->vstep <= 0 || p->rows <= 0 || p->nlevels < 1 || p->nlevels > 16)
    return "bad vstep/rows/nlevels";
  if (p->border < 16) return "ORB needs border >= 16 (Fast.h:46-49)";
  if (p->words < 1 || p->words > 8) return "words must be 1..8";
  if (p->log_bucket_size < 0 || p->log_bucket_size > 8 || p->bucket_limit < 1 || p->bucket_limit > 64)
    return "bad bucket parameters";
  if (p->max_keypoints < 1) return "max_keypoints must be positive";
  for (int l = 0; l < p->nlevels; l++) {
    if (lv[l].width <= 0 || lv[l].height <= 0 || lv[l].row0 < 0 || lv[l].col0 < 0 ||
        lv[l].col0 + lv[l].width > p->vstep || lv[l].row0 + lv[l].height > p->rows)
      return "level does not fit the pyramid buffer";
    if (lv[l].row0 + lv[l].height > 4096 || lv[l].col0 + lv[l].width > 4096)
      return "stacked coordinates exceed 12 bits (Util.h:27-29)";
  }
  return nullptr;
}

// ---- the strip plan of the fused pipeline (build_fused_plan) ----
// LDS figures every step of the plan, the launcher and the plan's invariant checks share.
constexpr long CU_LDS = 160 * 1024;          // LDS of a CU: `wgs` resident workgroups have CU_LDS / wgs bytes each
constexpr size_t LDS_CAP = 150 * 1024;       // most dynamic LDS a launch may ask for
constexpr size_t LDS_OPT_IN = 64 * 1024;     // more than this: the kernel's hipFuncAttributeMaxDynamicSharedMemorySize is raised first
// Queue bytes of a strip workgroup: the per-wave queues, plus the shared queues the two layouts differ in — ALIAS keeps one
// corner queue (QH_SHARED entries at least: FusedLevel::qh), the plain layout the corner queue and the NMS candidates'.
constexpr long WAVE_QUEUE_BYTES = (long)pf::WAVES * pf::QCAP * 4;
constexpr long QUEUE_BYTES_ALIAS = WAVE_QUEUE_BYTES + pf::QH_SHARED * 4;
constexpr long QUEUE_BYTES_PLAIN = WAVE_QUEUE_BYTES + pf::SHARED_Q * 4;
// What a workgroup's dynamic LDS may take for `wgs` of them to stay resident on a CU.
// (margin of 1280 B: static LDS + allocation granule — with 512 B the kernel measurably lost its 5th workgroup)
inline long residency_budget(int wgs) { return CU_LDS / wgs - 1280; }
// Residency target of the heuristic: 5 workgroups per CU.  (A search over 5 / 4 / 3 per CU with a cost model
// "pixels * (R + 4) / R / measured throughput at that residency" was tried for the 1280-wide levels of BASELINE
// config 4 — 12-row strips at 4 per CU instead of 16 rows at 3 — and measured no better: 1.24 vs 1.21 ms at
// batch 256; forcing 5 per CU with 8-row strips and no halo carry gave 1.16 ms.  Option "wgs_per_cu" overrides.)
inline int alias_wgs(const Options &o) { return o.wgs_per_cu > 0 ? o.wgs_per_cu : 5; }
// Strips a resident slot (5 per CU) works through in a launch of `batch` pyramids.
inline double strips_per_slot(const Options &o, int strips, int batch) {
  return (double)strips * batch / (5.0 * std::max(1, o.num_cus));
}

inline int classified_end(int border, int nx) { return border + 16 * cdiv(nx, 16); }   // FusedLevel::xend for nx columns inside the border
inline int score_pitch(int xend) { return (xend + 4 + 15) & ~15; }                     // FusedLevel::pitch
// LDS pitch of an image tile row that stages columns [xbase, xend + 8), xbase = (border - 4) & ~15: a multiple of 16 bytes.
// (An ODD number of 16-byte vectors — consecutive rows 4 banks apart instead of column x of every row in one bank at VGA
// level 0's 640 bytes — was measured in round 4: bit-exact, the strip kernel within 0.5 % either way: the per-candidate
// reads' bank conflicts, 45 % of its LDS cycles, come from the candidates' random columns, not from the row pitch.)
inline int tile_pitch(int border, int xend) { return (xend - border + ((border - 4) & 15) + 4 + 8 + 15) & ~15; }

// Step 1, plan entries: a level, or the x-tiles of a wide level (pf::FusedLevel: w, h, row0, col0, ex0, ex1, xscore, gfirst,
// gn).  A level with more than `tile_max` classified columns is cut into tiles of T block-origin columns (T a multiple of
// 32: tiles start on bucket boundaries for every fused bucket size); tile t > 0 starts HALO = 32 columns to the left of its
// first block origin, so that, seen as a level of its own with the same border B, it classifies and scores the columns its
// boundary blocks' NMS reads, and every tile but the last ends 2 columns past its last owned block origin.
// False: more entries than a plan holds.
inline bool plan_entries(const Options &o, const pislam_frontend_params *p, const pislam_level *lv, pf::FusedParams *F) {
  const int B = p->border, HALO = 32;
  const int tile_max = o.tile_cols > 0 ? o.tile_cols : (o.tile_cols < 0 ? 1 << 30 : 704);
  int n = 0;
  for (int l = 0; l < p->nlevels; l++) {
    const int w = lv[l].width, nx = w - 2 * B, ny = lv[l].height - 2 * B;
    int nt = 1;
    // tiles of ~448 owned columns: with the 32-column halo a tile row is two full 256-pixel prefilter steps,
    // and its strips reach the full 28 rows at 5 workgroups per CU (1280x960 batch 256: 0.94 ms with three
    // 416-column tiles at level 0 against 1.01 ms with two of 624)
    if (nx > 0 && ny > 0 && 16 * cdiv(nx, 16) > tile_max)
      nt = std::max(2, tile_max >= 640 ? (nx + 224) / 448 : cdiv(nx, std::max(64, tile_max)));
    const int T = nt > 1 ? (cdiv(nx, nt) + 31) & ~31 : 0;
    nt = nt > 1 ? cdiv(nx, T) : 1;
    if (n + nt > pf::MAX_LEVELS) {
      memset(F->lv, 0, sizeof(F->lv));                 // (a refused plan holds no entries, not the first few)
      return false;
    }
    const int g0 = n;
    for (int t = 0; t < nt; t++) {
      pf::FusedLevel &L = F->lv[n++];
      const int o = t == 0 ? 0 : t * T - HALO;                           // level column of the entry's origin
      const int E = nt == 1 ? w - B : std::min(B + (t + 1) * T, w - B);  // one past the last owned block origin (level x)
      L.w = t == nt - 1 ? w - o : E - o + 2 + B;
      L.h = lv[l].height;
      L.row0 = lv[l].row0;
      L.col0 = lv[l].col0 + o;
      L.ex0 = t == 0 ? B : B + HALO;
      L.ex1 = E - o;
      L.xscore = (w - B) - o;
      L.gfirst = g0;
      L.gn = nt;
    }
  }
  F->nlevels = n;
  return true;
}

// The widest entry of entry e's level: all tiles of a level must cut the same strips, so its strip height comes from this one.
inline int widest_tile(const pf::FusedParams &F, int e) {
  int w = 0;
  for (int t = F.lv[e].gfirst; t < F.lv[e].gfirst + F.lv[e].gn; t++) w = std::max(w, F.lv[t].w);
  return w;
}

// Step 2, the strip height of a level whose widest entry has w columns (rows_max: build_fused_plan's cap).  Four rules, in
// this precedence: option "strip_rows"; the ALIAS layout's residency rule; the generic 8k-pixel rule; and, where the strips
// select per bucket themselves (lbs != 0), rounding to whole bucket rows on top of whichever rule gave the height.
inline int strip_height(const Options &o, const pislam_frontend_params *p, int lbs, int w, int rows_max) {
  const int xend = classified_end(p->border, w - 2 * p->border), tpitch = tile_pitch(p->border, xend);
  const int wgs = alias_wgs(o);
  int R = o.strip_rows;
  if (R == 0 && o.alias) {
    // ALIAS layout under a residency target of `wgs` workgroups per CU: ~16k pixels per strip, 16..rows_max rows, capped so
    // that queues + tile + the minimum shared queue fit CU_LDS / wgs where 16 rows allow it (VGA at 5 per CU: 24 rows at
    // level 0, 28 below; measured 0.293 ms vs 0.311 ms with 16-row strips).
    const int rcap = (int)((CU_LDS / wgs - QUEUE_BYTES_ALIAS) / tpitch - 10) & ~1;
    if (wgs == 5 || rcap >= 10)                        // (else: an explicit residency request falls back to the generic rule)
      R = std::max(16, std::min(std::min(rows_max, std::max(16, (o.strip_px / w) & ~1)), rcap));
  }
  if (R == 0) {
    R = (8192 / w) & ~1;                               // ~8k pixels per strip ...
    R = std::min(32, std::max(16, R));
    if (o.wgs_per_cu > 0) {                       // ... capped so that tiles + queues fit CU_LDS / wgs_per_cu
      const long budget = CU_LDS / o.wgs_per_cu, pitch = score_pitch(xend);
      if (budget > QUEUE_BYTES_PLAIN + 13 * pitch)
        R = std::max(8, std::min(R, (int)(((budget - QUEUE_BYTES_PLAIN) / pitch - 13) / 2) & ~1));
    }
  }
  if (lbs) {                                           // (selection inside the strips:) strips hold whole bucket rows
    const int bs = 1 << lbs;
    if (o.strip_rows == 0 && o.alias) {
      // heuristic height: round UP to whole bucket rows (16-px buckets: 32-row strips — measured 0.315 ms
      // vs 0.371 ms with 16-row strips) where that still fits the residency budget, DOWN on the levels where it
      // does not: the launch has ONE LDS size, a single level over the budget costs every level its fifth workgroup
      const int up = std::min(std::max(bs, 32), ((R + bs - 1) / bs) * bs), down = std::max(bs, (R / bs) * bs);
      const long need = QUEUE_BYTES_ALIAS + (long)(up + 10) * tpitch;
      R = (o.bucket_round_up || need <= residency_budget(wgs)) ? up : down;
    } else
      R = std::max(bs, (R / bs) * bs);
  }
  return R;
}

// Step 3, the LDS of an entry whose R, nbx and xend are set: pitches, the reciprocals the kernel divides by them with, and
// what a workgroup of this entry needs in the plain layout (tbytes) and in the ALIAS layout (apad, qh at `wgs` per CU),
// raising the launch's *lds and *lds_alias to it.
inline void level_lds(int border, int wgs, pf::FusedLevel &L, size_t *lds, size_t *lds_alias) {
  const int R = L.R;
  L.pitch = score_pitch(L.xend);
  L.tpitch = tile_pitch(border, L.xend);
  L.vpr_recip = (uint32_t)(((1ull << 32) + (L.tpitch / 16) - 1) / (L.tpitch / 16));
  L.tp_recip = (uint32_t)(((1ull << 32) + L.tpitch - 1) / L.tpitch);
  // scan fallbacks reuse the image tile: row buffers of R/2 x nbx dwords, or per-cell results (<= one
  // dword per block) + per-cell counts (<= a quarter of that: a cell holds >= 2x2 blocks)
  L.tbytes = std::max((R + 10) * L.tpitch, (((R / 2) * L.nbx * 5 + 64) + 15) & ~15);
  *lds = std::max(*lds, (size_t)L.tbytes + (size_t)(R + 3) * L.pitch + (size_t)QUEUE_BYTES_PLAIN);
  // ALIAS layout: the score tile (R+3 rows) is laid over [NMS scratch end, image row R): pad the
  // per-wave queue area when that span is too short (levels wider than ~680 columns)
  // ... and the ORB phase's 8 patches + vrecpe table are laid over the same span (strip_body phase E)
  const long need = std::max((long)pf::NMS_SCRATCH * 4 + (long)(R + 3) * L.pitch,
                             (long)pf::NMS_SCRATCH * 4 + (long)pf::WAVES * 2 * pf::ORB_PATCH_BYTES + 256);
  const long have = WAVE_QUEUE_BYTES + (long)R * L.tpitch;
  L.apad = need > have ? (int)((need - have + 15) & ~15L) : 0;
  // one shared queue in this layout: at least QH_SHARED entries, and whatever LDS the level's tile
  // leaves under the residency budget (narrow levels of a textured photo are the dense ones)
  const long fixed = WAVE_QUEUE_BYTES + L.apad + (long)(R + 10) * L.tpitch;
  const long spare = (residency_budget(wgs) - fixed) / 4;
  L.qh = (int)std::min<long>(4096, std::max<long>(pf::QH_SHARED, spare & ~3L));
  *lds_alias = std::max(*lds_alias, (size_t)fixed + (size_t)L.qh * 4);
}

// Step 4, the run length.  Runs: a workgroup walks run_len consecutive strips of a level (halo carried in LDS).  Longer runs
// save the duplicated halo work but leave fewer, longer workgroups for the dispatcher to balance over the 5 resident
// slots per CU.  Measured (strip kernel, ms): VGA batch 256 (15 strips per slot): 0.236 / 0.231 / 0.233 / 0.243 /
// 0.242 / 0.235 / 0.231 / 0.229 / 0.229 / 0.243 for run_len 1 / 2 / 3 / 4 / 5 / 6 / 8 / 10 / 12 / 16 — the carry is
// worth ~3 % at best and the curve is dispatch-quantisation noise; 720p batch 64 (10 strips per slot): 0.208 /
// 0.207 / 0.216 / 0.227 / 0.238 for 1..5; 1280x960 batch 256 (54 per slot): 1.029 / 1.018 / 1.012 / 1.044 / 1.053 /
// 1.010 for 4 / 5 / 6 / 7 / 8..10 / 12, batch 64: 0.278 / 0.307 / 0.376 for 2 / 3 / 8; VGA batch 32, 64: 1 is best.
// Rule: ~6.5 workgroups per resident slot, at most 8 strips per run.  (List-scheduling and processor-sharing
// simulations of one XCD were tried as a predictor: neither tracks the measured 2-3 % structure.)
// With the runs of a pyramid launched longest first (order_runs) the curve flattens: VGA batch 256
// 0.232 / 0.222 / 0.220 / 0.224 / 0.222 / 0.233 for run_len 1 / 2 / 3 / 4 / 6 / 8; 1280x960 batch 256 0.920 / 0.898 /
// 0.899 / 0.889 / 0.889 for 2 / 4 / 6 / 8 / 12; 720p batch 64 0.191 / 0.191 / 0.197 / 0.206 for 1 / 2 / 3 / 4.
inline int run_length(const Options &o, const pf::FusedParams &F, int strips, int batch) {
  if (o.run_len > 0) return o.run_len;
  // Round 5 (strips of a run follow each other without a barrier): one call at a time the rule stands (VGA batch 256: strip
  // kernel 0.164 / 0.166 / 0.171 ms for run_len 2 / 3 / 4), but as a LANE of a pipeline — other batches' kernels fill the
  // tail of the launch — longer runs win: whole step 0.2233 / 0.2208 / 0.2203 ms for 2 / 3 / 4 (720p batch 64: 0.2974 /
  // 0.2954 for 2 / 3; demo photo x 256: 0.3242 / 0.3208 for 2 / 4).  Lanes aim at ~3.25 workgroups per slot.
  const double per_wg = o.lanes_in_flight > 1 ? 3.25 : 6.5;
  const int by_slot = std::max(1, std::min(8, (int)(strips_per_slot(o, strips, batch) / per_wg + 0.5)));
  if (o.lanes_in_flight <= 1) return by_slot;
  // Round 6, lanes only: the LONGEST runs that still leave the launch 0.6 workgroups per resident slot (5 per CU) — whole
  // levels per workgroup where the batch is large enough.  Re-swept after the pretest change, pipelined step in ms for
  // run_len default (the rule above) / 12 / 16 / 24 / 32 / 64: VGA batch 256 0.2117 / 0.2087 / 0.2062 / 0.2072 / 0.2063 / 0.2068
  // (8 whole-level runs per pyramid = 1.6 per slot); demo photo 0.3169 / 0.3153 / 0.3153 / 0.3144 / 0.3143 / 0.3140; 1280x960
  // 0.6692 / 0.6674 / 0.6628 / 0.6637 / 0.6517 / 0.6531; 720p build batch 64 0.2865 / 0.2759 / 0.2671 / 0.2581 / 0.2589 / 0.2590
  // (15 runs per pyramid = 0.75 per slot); bucket mode 0.2334 / 0.2293 / 0.2285 / 0.2281 / 0.2287 / 0.2277 — and where the
  // launch gets too few workgroups it turns: VGA batch 64 0.0646 / 0.0631 (0.6 per slot) / 0.0681 (0.5) / 0.0720; batch 16
  // 0.0208 / 0.0425.  The strip kernel ALONE is slower with long runs (0.156 -> 0.159-0.162 ms: a longer tail); on a lane
  // another batch's kernels run in that tail, and a long run stages its halo once and prefetches every strip but the first.
  const long want = (long)(0.6 * 5.0 * std::max(1, o.num_cus));
  int longest = 1;
  for (int l = 0; l < F.nlevels; l++) longest = std::max(longest, F.lv[l].nstrips);
  longest = std::min(longest, 64);                     // (option range; k_frame keeps a 64-bit mask of a run's strips)
  for (int rl = longest; rl > by_slot; rl--) {
    long r = 0;
    for (int l = 0; l < F.nlevels; l++) r += cdiv(F.lv[l].nstrips, rl);
    if (r * batch >= want && r <= pf::MAX_ORDER) return rl;
  }
  return by_slot;
}

// Step 5, the launch order of a pyramid's runs: estimated cost (pixels + a fixed share per strip), longest first — the
// longest-processing-time-first rule of list scheduling: workgroups are dispatched in blockIdx order to the
// 5 resident slots per CU, so the short runs of the small levels fill the tail of the launch.  Entry order
// (level by level) interleaves short last-runs of big levels with long runs of the next level: VGA batch 256
// 0.232 -> 0.222 ms, 1280x960 batch 256 0.927 -> 0.895 ms.  Plans with more runs than order[] holds keep entry order.
inline void order_runs(const Options &o, pf::FusedParams *F) {
  F->order_n = 0;
  if (F->runs_per_pyr <= 0 || F->runs_per_pyr > pf::MAX_ORDER || !o.run_order) return;
  struct RunCost {
    double cost;
    int entry, run;
  };
  std::vector<RunCost> rc;
  for (int l = 0; l < F->nlevels; l++) {
    const pf::FusedLevel &L = F->lv[l];
    const int ny = L.h - 2 * F->border;
    for (int r = 0; r < L.nruns; r++) {
      double cst = 0;
      for (int sidx = r * F->run_len; sidx < std::min((r + 1) * F->run_len, L.nstrips); sidx++)
        cst += 1.6 * L.w * std::min(L.R, ny - sidx * L.R) + 6000.0;
      rc.push_back({cst, l, r});
    }
  }
  std::stable_sort(rc.begin(), rc.end(), [](const RunCost &a, const RunCost &b) { return a.cost > b.cost; });
  for (size_t i = 0; i < rc.size(); i++) F->order[i] = ((uint32_t)rc[i].entry << 16) | (uint32_t)rc[i].run;
  F->order_n = (int)rc.size();
}

// The strip plan for heuristic strip heights of at most rows_max rows: the five steps above.  False: no strip plan for
// these parameters (the staged pipeline takes the call).
inline bool build_fused_plan_rows(const Options &o, const pislam_frontend_params *p, const pislam_level *lv,
                           int batch, int rows_max, pf::FusedParams *F, size_t *lds_bytes, size_t *lds_alias_bytes) {
  if (p->nlevels > pf::MAX_LEVELS) return false;
  memset(F, 0, sizeof(*F));
  F->vstep = p->vstep;
  F->rows = p->rows;
  F->border = p->border;
  F->thr = p->fast_threshold & 0xff;
  F->hthr = p->harris_threshold;
  F->batch = batch;
  F->dump_score = o.dump_score;
  F->lbs = p->log_bucket_size;
  F->limit = p->bucket_limit;
  F->words = p->words;
  F->orb_in_strip = o.orb_in_strip;
  // Buckets (fastExtract<.., logBucketSize, bucketLimit>): by default the strips run exactly as without buckets (F->lbs = 0:
  // any strip height, the plain kernels) and pf::k_bucket_select applies the per-cell top-`limit` between the strip kernel and
  // the gather (run_fused); option "bucket_select" 0 keeps the selection inside the strips (rounds 1-3: strips cut on bucket
  // rows, cells of 4..32 px).
  bool select = p->log_bucket_size != 0 && o.bucket_select;
  for (int l = 0; l < p->nlevels && select; l++)
    if (lv[l].width - 2 * p->border > 0 && ((lv[l].width - 2 * p->border - 1) >> p->log_bucket_size) + 1 > pf::SEL_NB) select = false;
  if (select) {
    F->lbs = 0;
    F->orb_in_strip = 0;
  }
  // fused bucket mode inside the strips: cells of 4..32 px (they must fit a strip and the per-wave scratch)
  if (F->lbs != 0 && (p->log_bucket_size < 2 || p->log_bucket_size > 5)) return false;
  F->ablate = o.ablate;
  if (!plan_entries(o, p, lv, F)) return false;
  int strips = 0, slots = 0, runs = 0;
  size_t lds = 0, lds_alias = 0;
  for (int l = 0; l < F->nlevels; l++) {
    pf::FusedLevel &L = F->lv[l];
    const int nx = L.w - 2 * p->border, ny = L.h - 2 * p->border;
    L.strip0 = strips;
    L.slot0 = slots;
    if (nx <= 0 || ny <= 0) {   // nothing to extract on this level (Fast.h loops do not run)
      L.R = 16;                 // (nstrips and nbx stay 0)
      L.xend = p->border;
      L.pitch = 16;
      continue;
    }
    L.R = strip_height(o, p, F->lbs, widest_tile(*F, l), rows_max);
    L.nstrips = cdiv(ny, L.R);
    L.nbx = (nx + 1) / 2;
    L.xend = classified_end(p->border, nx);
    level_lds(p->border, alias_wgs(o), L, &lds, &lds_alias);
    strips += L.nstrips;
    slots += L.nstrips * (L.R / 2) * L.nbx;
  }
  F->run_len = run_length(o, *F, strips, batch);
  for (int l = 0; l < F->nlevels; l++) {
    F->lv[l].run0 = runs;
    F->lv[l].nruns = cdiv(F->lv[l].nstrips, F->run_len);
    runs += F->lv[l].nruns;
  }
  F->strips_per_pyr = strips;
  F->runs_per_pyr = runs;
  F->slots_per_pyr = slots;
  order_runs(o, F);
  *lds_bytes = lds;
  *lds_alias_bytes = lds_alias + (size_t)o.lds_pad;   // profiling: opt_lds_pad lowers the residency artificially
  if ((size_t)p->rows * p->vstep > 0x7fffffffu) return false;   // 32-bit byte offsets inside a pyramid
  return lds <= LDS_CAP;          // (strips == 0: no level holds a classifiable pixel — the caller writes zero counts)
}

// Cap of the heuristic strip height.  Every strip pays a fixed share (set-up, barriers, the halo carried through
// LDS, the ragged last wave step of each phase), so the narrow levels want strips as tall as the prefetch
// registers allow (R * pitch <= 16 KiB) — but only when the launch has plenty of workgroups per resident slot;
// a small launch is balanced better by more, shorter strips.  Measured, strip kernel alone (ms) for caps 28 / 36 /
// 44 / 56 / 64: VGA batch 256 (15 strips per slot at cap 28) 0.221 / 0.212 / 0.209 / 0.207 / 0.211; 1280x960 batch
// 256 (54 per slot) 0.885 / 0.857 / 0.861 / 0.861; 720p batch 64 (10 per slot): whole step 0.337 / 0.346 / 0.346 /
// 0.344.  Rule: cap 56 from 12 strips per slot on, 28 below.  Option "strip_rows_max" overrides.
inline bool build_fused_plan(const Options &o, const pislam_frontend_params *p, const pislam_level *lv, int batch,
                      pf::FusedParams *F, size_t *lds_bytes, size_t *lds_alias_bytes) {
  if (o.strip_rows_max > 0)
    return build_fused_plan_rows(o, p, lv, batch, o.strip_rows_max, F, lds_bytes, lds_alias_bytes);
  if (!build_fused_plan_rows(o, p, lv, batch, 28, F, lds_bytes, lds_alias_bytes)) return false;
  if (strips_per_slot(o, F->strips_per_pyr, batch) < 12.0) return true;
  pf::FusedParams tall;
  size_t l0 = 0, l1 = 0;
  if (build_fused_plan_rows(o, p, lv, batch, 56, &tall, &l0, &l1)) {
    *F = tall;
    *lds_bytes = l0;
    *lds_alias_bytes = l1;
  }
  return true;
}

// Sub-batches of a fused batch call (option "sub_batches", default 1 = one launch group): the strip kernels of the
// sub-batches run back to back on the context stream, overflow pass + gather/ORB of sub-batch i on the context's
// second stream under the strip kernel of sub-batch i+1 (fork / join by events inside the call).  MEASURED AND
// NOT THE DEFAULT (MI355X, VGA batch 256, one call at a time): 0.286 ms with one launch group, 0.326 / 0.360 / 0.367
// / 0.466 ms with 2 / 3 / 4 / 6 sub-batches — a strip launch of 128 pyramids takes 0.121 ms, not half of 0.206: every
// launch ends in its own tail of partly filled CUs and the serialised launches add ~18 us each, more than the
// overlap wins back (1280x960: 1.23 -> 1.36 ms with 4).  What does pay is whole batches in flight on separate
// contexts (bench.py --streams, tools/pislam_demo --streams: 0.252 ms).  `0` = the MiB-per-sub-batch rule below.
inline int choose_sub_batches(const Options &o, const pislam_frontend_params *p, int batch) {
  if (o.dump_score || o.ablate || o.pipeline == 1) return 1;
  int n = o.sub_batches;
  if (n == 0) {
    const double mb = (double)p->rows * p->vstep * batch / (1024.0 * 1024.0);
    const double target = o.sub_mb > 0 ? o.sub_mb : 128.0;
    n = (int)(mb / target + 0.5);
    n = std::min(n, batch / 16);
  }
  return std::max(1, std::min(std::min(n, batch), MAX_SUB));
}

// The bucket selection pass (pf::k_bucket_select) and the UNIT plan the gather runs on when the strips run as without buckets
// (build_fused_plan): one "strip" per (level, cell row), `buckets x limit` slots each, lists final (lbs != 0, no tiles:
// the gather concatenates).  Part of the call's plan (plan_frontend).
inline const char *build_select_plan(const pislam_frontend_params *p, const pf::FusedParams &Fplan, pf::SelectPlan *Qp,
                                     pf::FusedParams *Up) {
  pf::SelectPlan &Q = *Qp;
  pf::FusedParams &U = *Up;
  memset(&Q, 0, sizeof(Q));
  memset(&U, 0, sizeof(U));
  const int lbs = p->log_bucket_size, bs = 1 << lbs, B = p->border;
  Q.lbs = lbs;
  Q.limit = p->bucket_limit;
  Q.border = B;
  int nreal = 0;
  for (int e = 0; e < Fplan.nlevels; e++) {
    if (Fplan.lv[e].gfirst != e) continue;           // (the tiles of a level follow its first entry)
    if (nreal >= 16) return "too many levels for the bucket selection pass";
    const int l = nreal++;
    const int gn = std::max(1, Fplan.lv[e].gn);
    const pf::FusedLevel &last = Fplan.lv[e + gn - 1];
    const int wl = last.col0 + last.w - Fplan.lv[e].col0, hl = Fplan.lv[e].h;       // the level's own size
    const int nx = wl - 2 * B, ny = hl - 2 * B;
    Q.row0[l] = Fplan.lv[e].row0;
    Q.col0[l] = Fplan.lv[e].col0;
    Q.h[l] = hl;
    Q.g0[l] = e;
    Q.gn[l] = gn;
    Q.unit0[l] = Q.units_per_pyr;
    Q.nunits[l] = (nx > 0 && ny > 0) ? cdiv(ny, bs) : 0;
    Q.cap[l] = (nx > 0 ? ((nx - 1) >> lbs) + 1 : 1) * p->bucket_limit;             // Fast.h:201 numBuckets x bucketLimit
    Q.uslot0[l] = Q.uslots_per_pyr;
    Q.nb_max = std::max(Q.nb_max, Q.cap[l] / p->bucket_limit);
    Q.units_per_pyr += Q.nunits[l];
    Q.uslots_per_pyr += Q.nunits[l] * Q.cap[l];
    pf::FusedLevel &ul = U.lv[l];
    ul.w = wl;
    ul.h = hl;
    ul.row0 = Q.row0[l];
    ul.col0 = Q.col0[l];
    ul.R = 2;                                        // strip_slot_of: slot0 + s * (R >> 1) * nbx
    ul.nbx = Q.cap[l];
    ul.nstrips = Q.nunits[l];
    ul.strip0 = Q.unit0[l];
    ul.slot0 = Q.uslot0[l];
    ul.gfirst = l;
    ul.gn = 1;
  }
  Q.nlevels = nreal;
  U.nlevels = nreal;
  U.strips_per_pyr = Q.units_per_pyr;
  U.slots_per_pyr = Q.uslots_per_pyr;
  U.vstep = p->vstep;
  U.rows = p->rows;
  U.border = B;
  U.lbs = lbs;
  U.limit = p->bucket_limit;
  U.words = p->words;
  U.ablate = Fplan.ablate;
  if (Q.units_per_pyr == 0) return "no extractable level";
  return nullptr;
}

// The unit table of the bucket selection pass (pf::k_bucket_select reads one record per unit instead of walking the plan):
// built on the host from the strip plan and the selection plan (never empty); its device copy comes from plan_table().
inline std::vector<uint32_t> unit_table(const pislam_frontend_params *p, const pf::FusedParams &F, const pf::SelectPlan &Q) {
  std::vector<uint32_t> t((size_t)Q.units_per_pyr * pf::SEL_REC, 0u);
  const int B = p->border, lbs = p->log_bucket_size, bs = 1 << lbs;
  for (int l = 0; l < Q.nlevels; l++)
    for (int cr = 0; cr < Q.nunits[l]; cr++) {
      uint32_t *r = &t[(size_t)(Q.unit0[l] + cr) * pf::SEL_REC];
      const int y0 = B + (cr << lbs), y1 = std::min(y0 + bs, Q.h[l] - B);
      int nl = 0;
      for (int k = 0; k < Q.gn[l]; k++) {
        const pf::FusedLevel &E = F.lv[Q.g0[l] + k];
        const int s_lo = (y0 - B) / E.R, s_hi = std::min((y1 - 1 - B) / E.R, E.nstrips - 1);
        for (int sidx = s_lo; sidx <= s_hi; sidx++, nl++)
          if (nl < pf::SEL_ML) {
            r[8 + nl] = (uint32_t)(E.slot0 + sidx * (E.R >> 1) * E.nbx);
            r[16 + nl] = (uint32_t)(E.strip0 + sidx);
          }
      }
      r[0] = nl <= pf::SEL_ML ? (uint32_t)nl : 0xffffffffu;
      r[1] = (uint32_t)l;
      r[2] = (uint32_t)cr;
      r[3] = (uint32_t)(Q.uslot0[l] + cr * Q.cap[l]);
      r[4] = (uint32_t)(Q.row0[l] + B);
      r[5] = (uint32_t)(Q.col0[l] + B);
    }
  return t;
}

// The one-launch path (pf::k_frame) takes batches of up to FRAME_MAX_BATCH pyramids: three launch floors are most of such
// a call (one VGA pyramid: 31 us in three launches, 15 us of it work), and its gather + ORB workgroups — which wait inside
// the grid for their pyramid's strips — stay a small fraction of an XCD's resident slots even with several such launches
// in flight (at most 128 per launch).
constexpr int FRAME_MAX_BATCH = 8;                                  // what option "frame" can be raised to
constexpr int FRAME_DEFAULT_BATCH = 2;                              // measured: one launch wins for 1 and 2 pyramids per call
inline int frame_max_batch(const Options &o) { return o.frame <= 0 ? 0 : o.frame == 1 ? FRAME_DEFAULT_BATCH : std::min(o.frame, FRAME_MAX_BATCH); }
static_assert(FRAME_MAX_BATCH <= pf::FRAME_SYNC_PYR, "k_frame's hand-over counters");

// What a front-end batch call decides from the shape and the options (plan_frontend, host only): reserve_frontend sizes the
// workspace from it and run_fused launches from it (pislam_hip.hip): after a reserve the call allocates nothing and can be
// captured into a hipGraph.
struct FrontendPlan {
  bool fused = false;                 // false: the staged pipeline (option "pipeline" 1, or no strip plan for the shape)
  int nsub = 1, submax = 0;           // sub-batches, pyramids in the largest one
  pf::FusedParams F{};                // the strip plan, built for submax pyramids (strips_per_pyr == 0: nothing to extract)
  size_t lds = 0, lds_alias = 0, klds = 0;   // strip kernel LDS bytes: plain layout, ALIAS layout, the layout it runs with
  bool sel = false;                   // the bucket selection pass: build_select_plan's two plans, the unit table
  pf::SelectPlan Q{};
  pf::FusedParams U{};
  std::vector<uint32_t> utab;
  size_t sel_lds = 0, glds = 0;       // LDS bytes of k_bucket_select and of k_gather
  bool alias = false;                 // ALIAS layout: one overflow list of ovf_stride dwords per sub-batch
  size_t ovf_stride = 0, sdesc_per_pyr = 0;
  bool generic_orb = false;           // k_gather + per-keypoint k_orb instead of k_gather_orb
  bool frame = false;                 // the one-launch path (pf::k_frame), as far as the shape and the options decide
  int nch = 0, fch = 0;               // ORB workgroups per pyramid of k_gather_orb and of k_frame
  size_t per_max = 0, olds = 0, fper = 0, flds = 0;   // keypoints per workgroup and LDS bytes of the two
};

// The plan of a batch call (parameters checked).  Refuses (see check_params) only where build_select_plan does, with `fused`
// and F already set.
inline const char *plan_frontend(const Options &o, const pislam_frontend_params *p, const pislam_level *lv, int batch, FrontendPlan *P) {
  P->nsub = choose_sub_batches(o, p, batch);
  P->submax = batch / P->nsub + (batch % P->nsub ? 1 : 0);
  P->fused = o.pipeline != 1 && build_fused_plan(o, p, lv, P->submax, &P->F, &P->lds, &P->lds_alias);
  const pf::FusedParams &F = P->F;
  const int S = F.strips_per_pyr, nsub = P->nsub, submax = P->submax;
  if (!P->fused || S == 0) return nullptr;
  P->sel = p->log_bucket_size != 0 && F.lbs == 0;
  if (P->sel) {
    if (const char *why = build_select_plan(p, F, &P->Q, &P->U)) return why;
    P->utab = unit_table(p, F, P->Q);
    P->sel_lds = sizeof(uint32_t) * pf::SEL_WAVES * (64 + 2 * (size_t)P->Q.nb_max);
  }
  const int Sg = P->sel ? P->Q.units_per_pyr : S;   // "strips" of the plan the gather runs on
  // descriptor staging: QS_SHARED slots of `words` dwords per strip (ALIAS strips hold at most QS_SHARED survivors)
  // (only strips that describe their own keypoints write there: option "orb_in_strip")
  P->sdesc_per_pyr = F.orb_in_strip ? (size_t)S * pf::QS_SHARED * (size_t)p->words : 0;
  // ALIAS layout (score tile laid over the dead image rows, 26 KB instead of 39 KB of LDS per workgroup
  // at VGA): the default.  Its overflow list (strips with overflowing queues) is drained by
  // k_fused_overflow right after; the gather kernel empties the list for the next step.
  P->alias = o.alias && submax <= 65535 && S <= 65535;
  P->ovf_stride = 2 + (size_t)S * submax;
  P->klds = P->alias ? P->lds_alias : P->lds;
  // k_gather_orb's 48-byte row windows assume a row-independent byte shift (vstep % 16 == 0) and
  // 32-bit byte offsets inside a pyramid; other layouts take the generic gather + per-keypoint ORB kernels.
  P->generic_orb = p->vstep % 16 != 0 || (size_t)p->rows * p->vstep > 0x7fffffffu;
  P->glds = sizeof(uint32_t) * (Sg + 1);
  // gather + orbCompute in one launch: (chunks, pyramids) workgroups
  // Workgroups per pyramid: one per ~70 k classified pixels (keypoint counts are not known to the host; ~70-100
  // keypoints per workgroup measured best: VGA, 981 keypoints: 14 = 21 chunks > 7, 28; 1280x960, 4389 keypoints: 42-49
  // chunks 0.36 ms against 0.41 ms with 14), at least 16 for small batches, and such that the grid is a whole number
  // of "waves" of resident workgroups (7 per CU: 64 VGPRs, 13.5 KB LDS) — batch 256: 14 chunks = 2 x 1792 workgroups
  // measured 0.079 ms against 0.085 ms with 16 (2.3 waves: the last one 30 % full).
  if (!P->generic_orb) {
    long px = 0;
    for (int l = 0; l < F.nlevels; l++) px += (long)(F.lv[l].ex1 - F.lv[l].ex0) * F.lv[l].nstrips * F.lv[l].R;
    const int by_px = (int)(px / 70000);
    int nch = std::min(64, submax >= 128 ? std::max(8, by_px) : std::max(by_px, std::max(16, 4096 / submax)));
    if (nsub == 1) {
      const long slots = 7L * std::max(1, o.num_cus);
      long best = nch, bestd = 1L << 40;
      for (long m = 1; m <= 64; m++) {
        const long cand = m * slots / submax;
        if (cand < 4 || cand > 64) continue;
        const long d = std::labs(cand - nch);
        if (d < bestd) {
          bestd = d;
          best = cand;
        }
      }
      nch = (int)best;
    } else {
      // pipelined sub-batches: the kernel shares the GPU with the next sub-batch's strip kernel, whole "waves" of
      // resident workgroups mean nothing there — one workgroup per ~70 k pixels
      nch = std::min(64, std::max(8, by_px));
    }
    P->nch = o.orb_chunks > 0 ? o.orb_chunks : nch;
    P->per_max = ((size_t)p->max_keypoints + P->nch - 1) / P->nch;
    P->olds = pf::orb_lds_bytes(Sg, P->per_max);
  }
  // The one-launch path.  Occupancy gate: the gather + ORB workgroups WAIT inside the grid.  With `lanes_in_flight` such
  // launches on the device at most lanes x batch x fch of them are resident, an eighth per XCD; they must stay a small
  // fraction (a quarter) of the workgroups an XCD holds with this launch's LDS footprint (96 VGPRs: five 4-wave workgroups
  // per CU at most), so that strip workgroups always find a slot.
  if (P->alias && !P->sel && F.lbs == 0 && !F.dump_score && !F.ablate && !P->generic_orb && nsub == 1 && !F.orb_in_strip &&
      o.repeat_strips <= 1 && batch <= frame_max_batch(o)) {
    P->fch = o.orb_chunks > 0 ? std::min(o.orb_chunks, 128) : std::min(64, std::max(16, 128 / batch));
    P->fper = ((size_t)p->max_keypoints + P->fch - 1) / P->fch;
    P->flds = std::max(std::max(P->lds_alias, P->lds), pf::orb_lds_bytes(S, P->fper));
    const long wg_per_cu = std::max<long>(1, std::min<long>(5, CU_LDS / (long)std::max<size_t>(P->flds, 1)));
    const long slots_per_xcd = wg_per_cu * std::max(1, o.num_cus / 8);
    const long waiting_per_xcd = ((long)std::max(1, o.lanes_in_flight) * batch * P->fch + 7) / 8;
    P->frame = P->flds <= LDS_CAP && 4 * waiting_per_xcd <= slots_per_xcd;
  }
  return nullptr;
}

// The invariants of a plan the kernels rely on (pislam_debug_build_plan checks every plan it builds): what is violated, or
// nullptr.  The strip plan first; the selection plan's are a second function because plan_frontend may have refused it.
inline const char *strip_plan_violation(const FrontendPlan &P, const pislam_frontend_params *p) {
  const pf::FusedParams &F = P.F;
  if (F.nlevels < 1 || F.nlevels > pf::MAX_LEVELS) return "entries";
  int strips = 0, slots = 0, runs = 0;
  for (int l = 0; l < F.nlevels; l++) {
    const pf::FusedLevel &L = F.lv[l];
    if (L.strip0 != strips || L.slot0 != slots || L.run0 != runs) return "prefix sums";
    if (L.nstrips < 0 || (L.nstrips > 0 && (L.R < 2 || (L.R & 1)))) return "strip height";
    if (L.nstrips > 0) {
      if (L.col0 < 0 || L.row0 < 0 || L.col0 + L.w > p->vstep || L.row0 + L.h > p->rows) return "entry outside the pyramid";
      if (L.tpitch % 16 || L.pitch % 16 || L.tpitch <= 0) return "pitch";
      if ((L.R + 10) * L.tpitch > (int)LDS_CAP) return "tile larger than the LDS";
      if (L.gfirst < 0 || L.gfirst > l || L.gn < 1 || L.gfirst + L.gn > F.nlevels) return "tile group";
      if (L.ex0 < p->border || L.ex1 > L.w || L.ex0 > L.ex1) return "owned columns";
      if (cdiv(L.nstrips, F.run_len) != L.nruns) return "runs";
      if ((uint64_t)L.vpr_recip * (uint64_t)(L.tpitch / 16) < (1ull << 32)) return "vpr_recip";
      if ((uint64_t)L.tp_recip * (uint64_t)L.tpitch < (1ull << 32)) return "tp_recip";
      if (L.qh < pf::QH_SHARED) return "corner queue";
    }
    strips += L.nstrips;
    slots += L.nstrips * (L.R / 2) * L.nbx;
    runs += L.nruns;
  }
  if (strips != F.strips_per_pyr || slots != F.slots_per_pyr || runs != F.runs_per_pyr) return "totals";
  if (F.order_n) {
    if (F.order_n != runs || runs > pf::MAX_ORDER) return "order size";
    std::vector<int> seen((size_t)runs, 0);
    for (int i = 0; i < F.order_n; i++) {
      const int e = (int)(F.order[i] >> 16), r = (int)(F.order[i] & 0xffff);
      if (e >= F.nlevels || r >= F.lv[e].nruns) return "order entry";
      seen[(size_t)(F.lv[e].run0 + r)]++;
    }
    for (int v : seen)
      if (v != 1) return "order is not a permutation of the runs";
  }
  if (P.lds_alias > (size_t)CU_LDS) return "aliased LDS size";
  return nullptr;
}

inline const char *select_plan_violation(const FrontendPlan &P, const pislam_frontend_params *p) {
  const pf::SelectPlan &Q = P.Q;
  int units = 0, uslots = 0;
  for (int l = 0; l < Q.nlevels; l++) {
    if (Q.unit0[l] != units || Q.uslot0[l] != uslots) return "selection plan prefix sums";
    if (Q.g0[l] < 0 || Q.g0[l] + Q.gn[l] > P.F.nlevels) return "selection plan entries";
    if (Q.cap[l] / p->bucket_limit > pf::SEL_NB) return "more buckets than the selection pass holds";
    units += Q.nunits[l];
    uslots += Q.nunits[l] * Q.cap[l];
  }
  if (units != Q.units_per_pyr || uslots != Q.uslots_per_pyr) return "selection plan totals";
  return nullptr;
}

// ---- a plan as one line of text (tools/probes/frontend_host_check.cpp --dump, tests/golden/frontend_plans.json) ----
inline uint64_t fnv1a(const void *p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
  return h;
}
// The refusal text or "ok"; every scalar of the plan: fused nsub submax lds lds_alias klds sel sel_lds glds alias ovf_stride
// sdesc_per_pyr generic_orb frame nch fch per_max olds fper flds; FNV-1a-64 of the bytes of F, Q and U; length:hash of the
// unit table.  NUL-terminated.  A refused plan is hashed as far as it got.
inline std::vector<char> plan_digest(const char *refusal, const FrontendPlan &P) {
  std::vector<char> s;
  auto text = [&s](const char *t) { s.insert(s.end(), t, t + strlen(t)); };
  auto number = [&s](uint64_t v, unsigned base) {
    char digits[24];
    int n = 0;
    do digits[n++] = "0123456789abcdef"[v % base];
    while (v /= base);
    while (n) s.push_back(digits[--n]);
  };
  text(refusal ? refusal : "ok");
  const uint64_t scalars[] = {P.fused, (uint64_t)P.nsub, (uint64_t)P.submax, P.lds, P.lds_alias, P.klds, P.sel, P.sel_lds, P.glds, P.alias,
                              P.ovf_stride, P.sdesc_per_pyr, P.generic_orb, P.frame, (uint64_t)P.nch, (uint64_t)P.fch, P.per_max, P.olds,
                              P.fper, P.flds};
  for (uint64_t v : scalars) {
    text(" ");
    number(v, 10);
  }
  const uint64_t hashes[] = {fnv1a(&P.F, sizeof(P.F)), fnv1a(&P.Q, sizeof(P.Q)), fnv1a(&P.U, sizeof(P.U))};
  const char *const names[] = {" F=", " Q=", " U="};
  for (int i = 0; i < 3; i++) {
    text(names[i]);
    number(hashes[i], 16);
  }
  text(" utab=");
  number(P.utab.size(), 10);
  text(":");
  number(fnv1a(P.utab.data(), sizeof(uint32_t) * P.utab.size()), 16);
  s.push_back(0);
  return s;
}

}  // namespace fp
