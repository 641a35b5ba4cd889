/*
 * pislam_hip.h — C ABI of the MI355X-native PiSlam ORB front-end.
 *
 * This is the drop-in boundary: a plain-C shared library (libpislam_hip.so,
 * built from pislam_amd/csrc with hipcc for gfx950) whose entry points are
 * what the reference's header-only templates forward to.  The C++ headers in
 * include/pislam/ (Fast.h, Harris.h, Orb.h, Brief.h, Util.h) keep the
 * reference's names, template parameter lists and argument order and are thin
 * wrappers over the functions below; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns PISLAM_OK (0) or a negative PISLAM_ERR_* code;
 *     pislam_last_error(ctx) returns a static/ctx-owned message.
 *   - image / score-map pointers are row-major uint8 with a row stride of
 *     `vstep` bytes, exactly the reference's `uint8_t img[][vstep]`.
 *   - every data pointer may be a HOST pointer or a DEVICE pointer
 *     (hipPointerGetAttributes decides).  Host data is staged through
 *     ctx-owned device buffers; device data is used in place (zero copy).
 *   - all work is issued on the ctx's stream (default: the null stream);
 *     calls with host pointers synchronise before returning, calls with only
 *     device pointers are asynchronous on that stream unless noted.
 *   - there is NO CPU fallback: if no gfx950 device is usable the functions
 *     return PISLAM_ERR_HIP.
 */
#ifndef PISLAM_HIP_H_
#define PISLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PISLAM_OK 0
#define PISLAM_ERR_INVALID (-1) /* bad argument / violated precondition */
#define PISLAM_ERR_HIP (-2)     /* HIP runtime error (no device, launch failure, ...) */
#define PISLAM_ERR_NOMEM (-3)   /* device allocation failed */
#define PISLAM_ERR_DIST (-4)    /* RCCL unavailable or a collective failed */

/* 2: pislam_pyramid_build_batch takes a PISLAM_BUILD_* bitmask (ABI 1: `blur`, any non-zero value) and refuses
 *    unknown bits; pislam_dist_comm_count; option "own_stream" 1 creates a stream with DEFAULT flags (ordered
 *    with the legacy null stream), 2 a non-blocking one; options "sub_batches" / "sub_mb". */
#define PISLAM_ABI_VERSION 2

typedef struct pislam_ctx pislam_ctx;

/* ---- context ---------------------------------------------------------- */
int pislam_abi_version(void);
/* device < 0 selects the current HIP device. */
int pislam_ctx_create(int device, pislam_ctx **ctx);
int pislam_ctx_destroy(pislam_ctx *ctx);
/* hip_stream is a hipStream_t passed as void*; NULL = null stream. */
int pislam_ctx_set_stream(pislam_ctx *ctx, void *hip_stream);
/* Tuning / test hooks; results never depend on them.  Keys:
 *   "own_stream" issue on a stream created (and destroyed) by the context instead of the null stream: 1 = default flags
 *                (still ordered with work on the legacy null stream, like the null stream itself), 2 = hipStreamNonBlocking
 *                (device-pointer inputs must then be complete, or ordered by the caller, before a call); 0 = back to the null stream
 *   "sub_batches" fused batch path: 1 (default) one launch group; n <= 16: the batch is cut into n sub-batches whose overflow
 *                pass + gather/ORB kernels run on a context-owned second stream under the next sub-batch's strip kernel
 *                (fork / join by events inside the call; results and stream semantics unchanged; a call captured into a
 *                hipGraph runs its sub-batches in order on the context stream;
 *                measured slower than one launch group on MI355X — DESIGN.md); 0: by size ("sub_mb" MiB per sub-batch, 128)
 *   "pipeline"   0 auto, 1 staged (one launch group per reference call, HBM score map), 2 fused strips
 *   "dump_score" fused pipeline also materialises the score map (pislam_frontend_get_score_map)
 *   "strip_rows" fused strip height (0 = heuristic);  "run_len" strips per workgroup run (0 = by batch)
 *   "alias"      1 (default) score tile laid over the dead image rows + overflow pass, 0 separate tiles
 *   "orb_chunks" gather+ORB workgroups per pyramid
 *   "run_order"  1 (default) a pyramid's runs are launched longest first, 0 in level order
 *   "tile_cols"  levels with more classified columns are cut into x-tiles run by separate workgroups (0 = 704, < 0 never)
 *   "orb_in_strip" 1 strips describe their own keypoints right after their NMS, 0 (default) one gather+ORB pass describes all
 *   "bucket_select" fused batch path with log_bucket_size != 0: 1 (default) the strips run as without buckets and a selection
 *                pass between strip kernel and gather keeps each bucket's bucket_limit largest keypoints (log_bucket_size 1..8);
 *                0 the selection happens inside the strips (strips cut on bucket rows; log_bucket_size 2..5, others take the
 *                staged pipeline)
 *   "frame"      small batches run as ONE launch (strip workgroups, then the gather + ORB workgroups of the same grid behind an
 *                agent-scope hand-over; overflowed strips redone in place): 1 (default) batches of 1 or 2 pyramids, n = 2..8
 *                batches of up to n, 0 never (always strip kernel -> overflow pass -> gather + ORB); not with buckets
 *   "wgs_per_cu", "strip_px", "strip_rows_max", "lds_pad", "bucket_round_up", "repeat_strips", "ablate"  profiling only (ablate != 0 gives INVALID results by design)
 *   "match_mfma" 1 (default) pislam_match_hamming* run on the int8 matrix cores, 0 the VALU popcount kernel (same results)
 *   "warp_direct" 1 every tile of pislam_warp_batch takes its taps from global memory, 0 (default) tiles whose source box fits are staged in LDS
 *   "clahe_combine" 1 (default) pislam_clahe_luts_batch adds equal bytes of a lane's dword to the LDS histogram in one atomic, 0 one atomic per pixel (same results)
 *   "clahe_lut_global" 1 pislam_clahe_apply_batch reads its four tables from global memory per pixel, 0 (default) stages them in LDS (same results)
 *   "dist_rccl_single" test hook: pislam_dist_init(world = 1) still creates a 1-rank RCCL communicator */
int pislam_ctx_set_option(pislam_ctx *ctx, const char *key, int value);
int pislam_ctx_synchronize(pislam_ctx *ctx);
const char *pislam_last_error(const pislam_ctx *ctx);

/* ---- the four reference entry points (one pyramid level each) ---------- */

/* replaces pislam::fastDetect<vstep,border>(width,height,img,out,threshold)
 * — reference include/Fast.h:54-158.  FAST-9 segment test; writes 0xff/0x00
 * to out rows [border,height-border), columns [border, border+16*ceil((width-
 * 2*border)/16)), plus out[y][width]=out[y][width+1]=0 when width%16 != 0.
 * Nothing else in `out` is touched.  Requires border >= 3.  Like the
 * reference's 16-byte vectors, the over-classified columns are addressed
 * flat: when border + 16*ceil((width-2*border)/16) + 3 > vstep they continue
 * in the next row, and `img` must be readable up to byte
 * (height-border+2)*vstep + that column (a few bytes past height*vstep only
 * for border < 6 on a level as wide as vstep). */
int pislam_fast_detect(pislam_ctx *ctx, int vstep, int border, int width, int height,
                       const uint8_t *img, uint8_t *out, int threshold);

/* replaces pislam::fastScoreHarris<vstep,border>(width,height,img,threshold,out)
 * — reference include/Fast.h:166-180 (+ Harris.h:37-248).  Every non-zero
 * out[y][x], y in [border,height-border), x in [border,width-border) is
 * replaced by its 8-bit Harris log-score.  Requires border >= 4. */
int pislam_fast_score_harris(pislam_ctx *ctx, int vstep, int border, int width, int height,
                             const uint8_t *img, int32_t threshold, uint8_t *out);

/* replaces pislam::fastExtract<vstep,border,logBucketSize,bucketLimit>(width,
 * height,out,results) — reference include/Fast.h:196-355.  2x2-block non-max
 * suppression (+ optional per-bucket top-k).  Writes the packed keypoints
 * (score<<24 | x<<12 | y, level-relative, reference order) to results[0..cap)
 * and the number the reference would have appended to *count (it may exceed
 * `capacity`; only the first `capacity` are stored).  logBucketSize 0..8,
 * bucketLimit 1..64.  Synchronous (count is returned to the host). */
int pislam_fast_extract(pislam_ctx *ctx, int vstep, int border, int logBucketSize,
                        int bucketLimit, int width, int height, const uint8_t *out,
                        uint32_t *results, size_t capacity, size_t *count);

/* replaces pislam::orbCompute<vstep,words>(img,points,descriptors)
 * — reference include/Orb.h:396-441.  descriptors[i*words + j], i in [0,n).
 * `img` is the base of the (stacked) image the keypoint coordinates refer to;
 * with a host pointer only the byte hull the reference itself reads
 * (rows y-15..y+15, columns x-15..x+16 of every keypoint) is accessed.
 * words 1..8. */
int pislam_orb_compute(pislam_ctx *ctx, int vstep, int words, const uint8_t *img,
                       const uint32_t *points, size_t n, uint32_t *descriptors);

/* ---- the reference's public helpers (L1 primitives) -------------------- */

/* pislam::harrisScoreSobel<vstep>(img,x,y,threshold) — Harris.h:80-248.
 * Batched over n points; scores[i] for packed point i (x<<12|y, score ignored). */
int pislam_harris_score_points(pislam_ctx *ctx, int vstep, const uint8_t *img,
                               const uint32_t *points, size_t n, int32_t threshold,
                               uint8_t *scores);

/* pislam::orbCentroids<vstep>(img,points) — Orb.h:80-308.  centroids has
 * pislam_centroids_size(n) int32 in the reference's grouped layout
 * [x0 x1 x2 x3 y0 y1 y2 y3]..., padding slots zero. */
size_t pislam_centroids_size(size_t n);
int pislam_orb_centroids(pislam_ctx *ctx, int vstep, const uint8_t *img,
                         const uint32_t *points, size_t n, int32_t *centroids);

/* pislam::atan2(const std::vector<int32_t>&) — Orb.h:310-387.  n8 (multiple
 * of 8) int32 in the grouped layout -> n8/2 angle bins (0..29), padding slots
 * included, exactly like the reference. */
int pislam_orb_angles(pislam_ctx *ctx, const int32_t *centroids, size_t n8, uint8_t *angles);

/* pislam::briefDescribe<vstep,words>(img,x,y,rot,descriptor) — Brief.h:637-733,
 * batched: descriptors[i*words+j] for point i with rotation rots[i]. */
int pislam_brief_describe(pislam_ctx *ctx, int vstep, int words, const uint8_t *img,
                          const uint32_t *points, const uint8_t *rots, size_t n,
                          uint32_t *descriptors);

/* The rotated-BRIEF offset table int8[30][256][4] = (dx0,dy0,dx1,dy1) the
 * kernels use (behaviour of Brief.h:28-53); host memory, 30720 bytes. */
const int8_t *pislam_brief_table(void);

/* ---- image preparation ("next" tier) -------------------- */

/* replaces pislam::gaussian5x5<vstep>(width,height,img,out) — reference include/Gaussian.h:48.
 * Separable [1 4 6 4 1]/16 built from rounding halving adds, vertical then horizontal, reflect-101
 * borders: bit-exact to the reference's stated expectation (test/GaussianTest.cpp:159-215).
 * Writes the width x height region only; img == out (in place) is allowed. */
int pislam_gaussian5x5(pislam_ctx *ctx, int vstep, int width, int height, const uint8_t *img,
                       uint8_t *out);

/* replace pislam::bilinear7_8<vstep> / bilinear13_16<vstep>(width,height,img,out) — reference
 * include/Bilinear.h:42 / :165; arithmetic of test/BilinearTest.cpp:171-196 / :198-233.  The image
 * must be padded to a multiple of 8 / 16 in both dimensions (Bilinear.h:32,155); output dimensions
 * round down (floor(w*7/8) x floor(h*7/8), resp. 13/16); like the reference, whole 7x7 / 13x13
 * output blocks are written.  img == out is allowed. */
int pislam_bilinear7_8(pislam_ctx *ctx, int vstep, int width, int height, const uint8_t *img,
                       uint8_t *out);
int pislam_bilinear13_16(pislam_ctx *ctx, int vstep, int width, int height, const uint8_t *img,
                         uint8_t *out);

/* Lens undistortion and stereo rectification as a fixed-point mesh warp: the step in front
 * of pislam_pyramid_build_batch.  The matchers, pislam_match_stereo_batch in particular, assume undistorted
 * (rectified) pinhole images.  The reference ships nothing of the kind: the semantics are this library's own.
 *
 * An immutable warp object holds a coarse grid of source coordinates the caller computes from a calibration;
 * pislam_warp_batch resamples `batch` device-resident 8-bit frames through it, bilinearly, into `batch` output
 * frames.
 *
 * Mesh layout.  C = 1 << log_cell, 0 <= log_cell <= 6.  mesh_w = ((width - 1) >> log_cell) + 2, mesh_h likewise
 * (pislam_warp_mesh_dims; no context needed).  mesh_x and mesh_y are HOST int32 [mesh_h][mesh_w]; node (j, i) is the
 * source position of output pixel (i * C, j * C) in Q8: 256 is one source pixel, pixel centres lie at integers.
 * With log_cell == 0 the mesh is dense; its last node column and row carry weight 0, must still be supplied and
 * are ignored.
 *
 * Source coordinate of output pixel (x, y).  i = x >> log_cell, fx = x & (C - 1), j = y >> log_cell,
 * fy = y & (C - 1).  Per axis, with m the mesh:
 *   a    = (m[j][i]   * (C - fx) + m[j][i+1]   * fx + (C >> 1)) >> log_cell
 *   b    = (m[j+1][i] * (C - fx) + m[j+1][i+1] * fx + (C >> 1)) >> log_cell
 *   s_q8 = (a * (C - fy) + b * fy + (C >> 1)) >> log_cell
 * in signed 32-bit arithmetic; every >> is an arithmetic shift (floor).  Nothing overflows within the node range
 * below.
 *
 * Sampling.  s5 = (s_q8 + 4) >> 3, x0 = s5x >> 5, ax = s5x & 31, likewise y0 and ay (a position of -0.5 px is
 * x0 = -1, ax = 16).  S(u, v) = the source byte at src + b * src_stride + v * src_vstep + u when 0 <= u < src_width
 * and 0 <= v < src_height, otherwise `border`.
 *   out = ((32-ax)*(32-ay)*S(x0,y0) + ax*(32-ay)*S(x0+1,y0) + (32-ax)*ay*S(x0,y0+1) + ax*ay*S(x0+1,y0+1) + 512) >> 10
 * written to dst + b * dst_stride + y * dst_vstep + x.  Only the width x height bytes of each output frame are
 * written.  No source byte outside the src_width x src_height rectangle of a frame is read, row padding included.
 *
 * Limits: 1 <= width, height <= 4096 (outputs stay inside the 12-bit keypoint coordinates);
 * 1 <= src_width, src_height <= 16384; every node in [-2^23, 2^23); 0 <= border <= 255; src_vstep >= src_width and
 * dst_vstep >= width; batch >= 0 (batch == 0 is a no-op that returns PISLAM_OK); src and dst are device pointers
 * whose byte ranges do not overlap; the warp belongs to the context's device.  Anything else: PISLAM_ERR_INVALID,
 * before anything is launched or written.  Offsets use size_t arithmetic throughout: strides may push a batch past
 * 4 GiB.
 *
 * Lifetime and streams.  pislam_warp_create validates, plans, uploads on the context's device and stream and
 * synchronises, as pislam_vocab_create does; the host arrays are not referenced afterwards.  A warp is immutable and
 * may be used by any context of its device; destroy it after the work that uses it has completed.
 * pislam_warp_batch is asynchronous on the context stream, has no workspace and no host round trip, and can be
 * captured into a hipGraph as it is.
 *
 * The output is cut into tiles of 64 x 32 pixels, one workgroup each.  A tile whose source bounding box (from the
 * minimum and maximum of its nodes) fits the workgroup's LDS is staged there; any other tile takes its taps from
 * global memory (direct).  Option "warp_direct" 1 sends every tile down the direct path (0, the default: by the
 * plan; other values are refused); the results are the same.  pislam_warp_info: info[0] tiles, [1] tiles staged,
 * [2] tiles direct (as planned, whatever the option says), [3] LDS bytes per workgroup. */
typedef struct pislam_warp pislam_warp;
int pislam_warp_create(pislam_ctx *ctx, int width, int height, int src_width, int src_height, int log_cell,
                       const int32_t *mesh_x, const int32_t *mesh_y, int border, pislam_warp **warp);
int pislam_warp_destroy(pislam_warp *warp);
int pislam_warp_mesh_dims(int width, int height, int log_cell, int32_t *mesh_w, int32_t *mesh_h);
int pislam_warp_info(const pislam_warp *warp, int32_t info[4]);
int pislam_warp_batch(pislam_ctx *ctx, const pislam_warp *warp, const uint8_t *src, int src_vstep, size_t src_stride,
                      uint8_t *dst, int dst_vstep, size_t dst_stride, int batch);

/* Contrast-limited adaptive histogram equalisation (CLAHE): the step between
 * pislam_warp_batch and pislam_pyramid_build_batch for dim, hazy or unevenly lit frames (fast_threshold and
 * harris_threshold are absolute grey-level numbers).  The reference ships nothing of the kind: the semantics are this
 * library's own, after OpenCV's CLAHE but stated in integers from end to end.  This comment is the contract.
 *
 * Buffers.  Frame b is at src + b * src_stride, uint8 [height][src_vstep]; dst is laid out likewise.  luts is a device
 * buffer the caller supplies, uint8 [batch][tiles_y][tiles_x][256], pislam_clahe_lut_size(p) bytes per frame.
 * pislam_clahe_luts_batch computes the tables, pislam_clahe_apply_batch blends given tables into dst, and
 * pislam_clahe_batch is the first followed by the second on the context stream: its luts is both the scratch space
 * and an output the caller may inspect.  The caller owns luts, so there is no context workspace and no reserve call:
 * every call is asynchronous on the context stream, has no host round trip and can be captured into a hipGraph as
 * it is.
 *
 * With W = width, H = height, tw = ceil(W / tiles_x), th = ceil(H / tiles_y), area = tw * th:
 *
 * Extended frame.  E(x, y) = src[r(y, H)][r(x, W)] for 0 <= x < tw * tiles_x, 0 <= y < th * tiles_y, with r(i, n) = i
 * if i < n and 2 * (n - 1) - i otherwise (reflect-101; tiles_x <= W and tiles_y <= H keep r >= 0).  No byte outside
 * the W x H rectangle of a frame is read, row padding included.
 *
 * Histogram of tile (tx, ty).  h[v] = the number of pixels of E with value v in [tx * tw, (tx + 1) * tw) x
 * [ty * th, (ty + 1) * th); it sums to area.
 *
 * Clip (only if clip_q8 > 0).  clip = max((clip_q8 * area) >> 16, 1), computed in 64 bits.
 * excess = sum over v of max(h[v] - clip, 0); then h[v] = min(h[v], clip).  q = excess / 256, res = excess % 256.
 * Every bin gets + q.  If res > 0: step = 256 / res (floor; at least 1), and bin v gets + 1 iff v % step == 0 and
 * v / step < res.  (OpenCV's residual loop in closed form.  Bins may exceed clip afterwards, as in OpenCV.)
 *
 * Table.  lut[v] = min(255, (255 * cdf[v] + (area >> 1)) / area), cdf the inclusive prefix sum of h, floor division.
 *
 * Blend, for output pixel (x, y) with v = src[y][x] and L[ty][tx] the table of tile (tx, ty):
 *   fx = 2 * x - tw, tx1 = floor(fx / (2 * tw)) (-1 for fx < 0), wx2 = fx - 2 * tw * tx1 (0 <= wx2 < 2 * tw),
 *   wx1 = 2 * tw - wx2, tx2 = tx1 + 1; then tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1): the clamp does not change
 *   the weights.  Likewise fy, ty1, ty2, wy1, wy2 with th.
 *   S = wy1 * (wx1 * L[ty1][tx1][v] + wx2 * L[ty1][tx2][v]) + wy2 * (wx1 * L[ty2][tx1][v] + wx2 * L[ty2][tx2][v])
 *   D = 4 * tw * th, out = (S + (D >> 1)) / D, floor division.
 * Only the W x H bytes of each output frame are written.  pislam_clahe_apply_batch takes any table bytes, monotone
 * or not.
 *
 * Differences from OpenCV (by construction; OpenCV was not run against this): OpenCV rounds the table and the blend
 * in float (cvRound), this statement rounds half up in exact integers; OpenCV pads both axes whenever either does
 * not divide evenly, this statement pads each axis on its own.  The tile grid, the clip formula, the single-pass
 * redistribution and the x / tw - 0.5 tile coordinate follow OpenCV (ORB-SLAM3's createCLAHE(3.0, Size(8, 8)) is
 * tiles 8 x 8, clip_q8 768).
 *
 * Limits: 1 <= width, height <= 4096; 1 <= tiles_x <= min(32, width), 1 <= tiles_y <= min(32, height);
 * area <= 2^20 (so S + D / 2 < 2^32 and 255 * cdf < 2^28; a 4096 x 4096 frame needs at least 4 x 4 tiles);
 * 0 <= clip_q8 <= 65535; src_vstep >= width, dst_vstep >= width; batch >= 0 with no upper limit (batch == 0 is a
 * no-op that returns PISLAM_OK after the checks of p, batch and the steps; the data pointers are not looked at then
 * and may be NULL).  Offsets use size_t arithmetic throughout: strides may carry a batch past 4 GiB.  dst may be
 * exactly src (same pointer, same vstep, same stride: in place); any other overlap of the byte ranges of src, dst and
 * luts is refused.  src, dst and luts are device pointers; p is a host struct read during the call.  Any violation:
 * PISLAM_ERR_INVALID, before anything is launched or written.  pislam_clahe_lut_size needs no context and returns
 * 0 for an invalid p. */
typedef struct pislam_clahe_params {
  int32_t width, height;     /* frame size in pixels */
  int32_t tiles_x, tiles_y;  /* tile grid (OpenCV's tileGridSize; ORB-SLAM3: 8, 8) */
  int32_t clip_q8;           /* clip limit in Q8 (OpenCV's clipLimit * 256; ORB-SLAM3: 768); 0 = no clipping */
} pislam_clahe_params;
size_t pislam_clahe_lut_size(const pislam_clahe_params *p);
int pislam_clahe_luts_batch(pislam_ctx *ctx, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                            size_t src_stride, int batch, uint8_t *luts);
int pislam_clahe_apply_batch(pislam_ctx *ctx, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                             size_t src_stride, const uint8_t *luts, uint8_t *dst, int dst_vstep, size_t dst_stride,
                             int batch);
int pislam_clahe_batch(pislam_ctx *ctx, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                       size_t src_stride, uint8_t *dst, int dst_vstep, size_t dst_stride, int batch, uint8_t *luts);

/* ---- the measured path: a batch of stacked pyramids, device resident --- */

typedef struct pislam_level {
  int32_t width;  /* level width  (pixels)                                   */
  int32_t height; /* level height (rows)                                     */
  int32_t row0;   /* first row of the level inside the stacked pyramid       */
  int32_t col0;   /* first column (0 for the vertically stacked layout)      */
} pislam_level;

typedef struct pislam_frontend_params {
  int32_t vstep;            /* row stride in bytes (reference template vstep)  */
  int32_t rows;             /* rows per pyramid buffer                         */
  int32_t nlevels;          /* 1..16                                           */
  int32_t border;           /* reference template border (>= 16 for ORB)       */
  int32_t fast_threshold;   /* fastDetect threshold (demo: 20)                 */
  int32_t harris_threshold; /* fastScoreHarris threshold (demo: 1<<15)         */
  int32_t log_bucket_size;  /* fastExtract logBucketSize (0 = no buckets)      */
  int32_t bucket_limit;     /* fastExtract bucketLimit                         */
  int32_t words;            /* orbCompute words (1..8)                         */
  int32_t max_keypoints;    /* capacity per pyramid of keypoints/descriptors   */
} pislam_frontend_params;

/* On-GPU pyramid build (BASELINE config 5).  The reference ships no pyramid builder (README.md:28-31)
 * but provides the two reductions to build one from (Bilinear.h:28-30,153): level k+1 =
 * bilinear7_8 (steps[k] = 1) or bilinear13_16 (steps[k] = 2) of level k, level 0 = gaussian5x5 of the
 * frame (blur != 0) or the frame itself.  pislam_pyramid_layout computes the level table of a vertically
 * stacked pyramid (dimensions round down, every level's slot keeps the padding rows its reduction
 * reads); pislam_pyramid_build_batch fills `batch` pyramids from `batch` device-resident frames.
 * Every byte a consumer reads — the levels, the whole output blocks of each reduction, the next reduction's
 * block padding and FAST's right-edge columns (a margin of 32 columns / 16 rows around each level's
 * rewritten rectangle, zeroed on every call) — equals running the reference functions level by level on a
 * zero-initialised buffer; bytes beyond those margins are left untouched.
 * Layout of a build call (tests/test_build_layouts.py pins each of these, bit for bit, on whole allocations):
 *   frames   : frame b at frames + b*frame_stride, rows frame_vstep bytes apart; any frame_vstep >= width and any
 *              frame_stride >= height*frame_vstep.  Row padding and the gaps between frames are never read as pixels
 *              (the blur reflects at `width`).
 *   pyramids : pyramid b at pyramids + b*pyramid_stride, uint8 [rows][vstep]; any vstep that holds every level with
 *              its block padding (pislam_pyramid_layout's, or wider) and any pyramid_stride >= rows*vstep.  Gaps
 *              between pyramids are never written.
 *   Both bases may have any alignment, and the strides may exceed 4 GiB.  Alignment decides the speed, not the bytes:
 *   the blur stages a tile with 16-byte loads when the frame's address and frame_vstep are multiples of 16 (dwords
 *   when multiples of 4, else bytes), chosen per frame; a reduction takes the 4-block kernel when `pyramids`, vstep
 *   and pyramid_stride are multiples of 16 and vstep holds the level's blocks rounded up to groups of four (else a
 *   one-lane kernel), and the one-launch build (option "build_chain") needs that of every reduction.
 *   batch    : any positive int.  It goes into one grid dimension as it is (no walk in pieces of 65535, unlike the
 *              per-keypoint calls): HIP on gfx950 launches grids beyond 65535 in y and z, and a build of 65537 frames
 *              is part of the tests. */
int pislam_pyramid_layout(int width, int height, int nlevels, const int32_t *steps, int vstep_min,
                          pislam_level *levels, int32_t *vstep, int32_t *rows);
#define PISLAM_BUILD_BLUR 1          /* level 0 = gaussian5x5 of the frame (else the frame itself)              */
#define PISLAM_BUILD_MARGINS_CLEAN 2 /* the margins are already zero: this function filled `pyramids` before with */
                                     /* the same layout and nothing else wrote to it since — skip re-zeroing them */
#define PISLAM_BUILD_CHECK_MARGINS 4 /* debug, with MARGINS_CLEAN: verify that promise (synchronises; non-zero    */
                                     /* margin bytes -> PISLAM_ERR_INVALID).  Other bits are refused.             */
int pislam_pyramid_build_batch(pislam_ctx *ctx, int nlevels, const int32_t *steps, const pislam_level *levels,
                               const uint8_t *frames, int frame_vstep, size_t frame_stride, int batch,
                               uint8_t *pyramids, int vstep, int rows, size_t pyramid_stride, int flags);

/* Runs, for every pyramid b in [0,batch) and every level l (in order), the
 * call sequence of reference demo/demo.cpp:77-101 / README.md:67-82:
 *   fastDetect -> fastScoreHarris -> fastExtract (y += row0, x += col0)
 * then one orbCompute over the stacked image, entirely on the device.
 *   pyramids    : DEVICE, batch * pyramid_stride bytes, pyramid b at
 *                 pyramids + b*pyramid_stride, uint8 [rows][vstep]
 *   keypoints   : DEVICE uint32 [batch][max_keypoints]   (reference order)
 *   descriptors : DEVICE uint32 [batch][max_keypoints][words]
 *   counts      : DEVICE uint32 [batch]  = keypoints the reference would emit
 *                 (entries beyond max_keypoints are dropped, count is not clamped)
 * Asynchronous on the ctx stream; no host round trips; capturable in a hipGraph
 * after pislam_frontend_reserve() has sized the workspace. */
int pislam_orb_frontend_batch(pislam_ctx *ctx, const pislam_frontend_params *params,
                              const pislam_level *levels, const uint8_t *pyramids,
                              size_t pyramid_stride, int batch, uint32_t *keypoints,
                              uint32_t *descriptors, uint32_t *counts);

/* Pre-allocates the ctx workspace for the given shape (optional; the batch
 * call grows it on demand, which synchronises). */
int pislam_frontend_reserve(pislam_ctx *ctx, const pislam_frontend_params *params,
                            const pislam_level *levels, int batch);

/* Debug / parity hook: after pislam_orb_frontend_batch, copies the internal
 * score map of pyramid b (uint8 [rows][vstep], what the reference's `out`
 * holds after fastScoreHarris on every level) to dst (host or device).
 * Returns PISLAM_ERR_INVALID if the active pipeline does not materialise it. */
int pislam_frontend_get_score_map(pislam_ctx *ctx, int b, uint8_t *dst);

/* Elapsed milliseconds of the LAST pislam_orb_frontend_batch call on this ctx,
 * measured with hipEvents recorded on the ctx stream around its kernels
 * (total, and per internal stage — staged pipeline: 0 detect+score, 1 extract,
 * 2 orb; fused pipeline: 0 strip kernel (detect+score+extract), 1 overflow
 * pass, 2 gather+orb).
 * Synchronises on the end event. */
int pislam_frontend_last_timing(pislam_ctx *ctx, float *total_ms, float stage_ms[3]);

/* Diagnostics of the last pislam_orb_frontend_batch call on the fused pipeline:
 * stats[0] = strips whose on-chip queues overflowed (very dense corners) and
 * that were redone by the slower overflow pass, stats[1] = strips in the call.
 * Results are identical either way; a large ratio means the input is denser
 * than the fast path is sized for.  Synchronises the context stream. */
int pislam_frontend_last_stats(pislam_ctx *ctx, uint32_t stats[2]);

/* Which path the last pislam_orb_frontend_batch call on this context took (a bit mask; 0 before the first call).
 * Results are identical on every path; this is for tests, tuning and bug reports.  No synchronisation. */
#define PISLAM_PATH_STAGED 1u          /* one launch group per level (option "pipeline" 1, or a shape the strips cannot take) */
#define PISLAM_PATH_FUSED 2u           /* strip kernel -> overflow pass -> gather + ORB */
#define PISLAM_PATH_ONE_LAUNCH 4u      /* the same work as ONE launch (pf::k_frame): batches of 1 or 2 pyramids by default, option "frame" */
#define PISLAM_PATH_BUCKET_SELECT 8u   /* buckets applied by the selection pass between strips and gather (option "bucket_select" 1) */
#define PISLAM_PATH_BUCKETS_IN_STRIPS 16u /* buckets applied inside the strips (option "bucket_select" 0, or more buckets than the pass holds) */
#define PISLAM_PATH_GENERIC_ORB 32u    /* generic gather + per-keypoint ORB kernels (vstep % 16 != 0) */
#define PISLAM_PATH_FRAME_TIMED_OUT 64u /* an earlier one-launch call of this context timed out (reported then, see below): the
                                          context runs small batches as three launches now */
unsigned pislam_frontend_last_path(const pislam_ctx *ctx);
/* (On a pipeline lane the value is that of the lane's last call whether it ran eagerly or was replayed from its
 * hipGraph.  On PISLAM_PATH_ONE_LAUNCH calls pislam_frontend_last_timing reports the whole call as stage 0: stages 1, 2 = 0.)
 *
 * The one-launch path's safety net.  Inside pf::k_frame the gather + ORB workgroups wait for the strip workgroups of the
 * same grid; the library takes the path only while such waiting workgroups are a small fraction of the resident slots,
 * and the wait is bounded (~1 s).  Should it ever expire (nothing observed does this: CU masks, a debugger or a future
 * dispatcher could), the call does NOT return stale data silently:
 *   - counts[i] of every pyramid whose keypoints were not produced is PISLAM_COUNT_INVALID (no valid count can be);
 *   - the next call on the context (or on its pipeline lane), pislam_ctx_synchronize, pislam_pipeline_synchronize and
 *     pislam_frontend_last_stats return PISLAM_ERR_HIP once, with a message naming the time-out, after resetting the
 *     hand-over state; from then on the context runs small batches as three launches (PISLAM_PATH_FRAME_TIMED_OUT is set
 *     in pislam_frontend_last_path; graphs the pipeline captured with a one-launch node are dropped). */
#define PISLAM_COUNT_INVALID 0xffffffffu

/* Host only — no device, no allocation, no launch: build the strip plan (and the bucket selection plan) a batch call with
 * these parameters would run, with the planner the call itself uses (pislam_amd/csrc/pislam_frontend_plan.h), and check the
 * invariants the kernels rely on.  `options`: "key=value,key=value" with pislam_ctx_set_option keys (NULL / "": defaults;
 * own_stream is refused: it needs a device); num_cus <= 0: 256; lanes_in_flight: 1, or the depth of the pipeline the
 * call would be a lane of.  summary: [0] plan entries, [1] strips, [2] runs, [3] staging slots per pyramid, [4] strips per
 * run, [5] / [6] LDS bytes of the plain / aliased layout, [7] units of the bucket selection pass.  Returns
 * PISLAM_ERR_INVALID (message in `err`) when the parameters are refused or the staged pipeline would take the call. */
int pislam_debug_build_plan(const pislam_frontend_params *params, const pislam_level *levels, int batch, int num_cus,
                            int lanes_in_flight, const char *options, uint32_t summary[8], char *err, size_t err_cap);

/* ---- batches in flight ---------------------------------------------------
 * A pipeline = `depth` (1..8) contexts behind one object, each with its own workspace and non-blocking stream:
 * batch k runs on lane k % depth, so that the tail of one batch (partly filled CUs, the latency-bound gather+ORB
 * kernel, launch gaps) runs under the head of the next.  MI355X, 256 VGA pyramids per batch: 0.27 ms per batch
 * one call at a time, 0.23 ms with depth 3.  The reference loop (demo/demo.cpp:77-101: frames are independent)
 * becomes
 *     for each batch k:  pislam_pipeline_submit(pipe, ..., inputs_k, outputs_k, producer_stream, 1, &t[k]);
 *     before consuming outputs_k on stream s:  pislam_pipeline_wait(pipe, t[k], s);
 * submit: the lane's stream first waits (device side) for everything `input_stream` (hipStream_t as void*) holds
 * so far when order_after_input != 0 — the producer of `pyramids` — then runs pislam_orb_frontend_batch.  Outputs
 * of a batch must stay untouched until its ticket has been waited for; a lane's batches are ordered among
 * themselves.  pislam_pipeline_stream gives the lane's stream of a ticket (e.g. for
 * pislam_dist_allgather_counts_on), pislam_pipeline_lane its context (statistics).  A call that repeats exactly
 * (same buffers, same shape: a steady stream of batches) is replayed from a hipGraph from its third occurrence
 * on (option "graphs" 0 = always eager); pislam_pipeline_set_option applies any context option to every lane. */
typedef struct pislam_pipeline pislam_pipeline;
int pislam_pipeline_create(int device, int depth, pislam_pipeline **pipe);
int pislam_pipeline_destroy(pislam_pipeline *pipe);
int pislam_pipeline_depth(const pislam_pipeline *pipe);
int pislam_pipeline_set_option(pislam_pipeline *pipe, const char *key, int value);
int pislam_pipeline_reserve(pislam_pipeline *pipe, const pislam_frontend_params *params, const pislam_level *levels,
                            int batch);
int pislam_pipeline_submit(pislam_pipeline *pipe, const pislam_frontend_params *params, const pislam_level *levels,
                           const uint8_t *pyramids, size_t pyramid_stride, int batch, uint32_t *keypoints,
                           uint32_t *descriptors, uint32_t *counts, void *input_stream, int order_after_input,
                           uint64_t *ticket);
int pislam_pipeline_wait(pislam_pipeline *pipe, uint64_t ticket, void *stream);
int pislam_pipeline_synchronize(pislam_pipeline *pipe);
/* stats[0] batches submitted, [1] of them replayed from a hipGraph, [2] calls captured, [3] captures that failed
 * (such a call stays eager). */
int pislam_pipeline_stats(const pislam_pipeline *pipe, uint64_t stats[4]);
void *pislam_pipeline_stream(pislam_pipeline *pipe, uint64_t ticket);
pislam_ctx *pislam_pipeline_lane(pislam_pipeline *pipe, int lane);
const char *pislam_pipeline_last_error(const pislam_pipeline *pipe);

/* Measurement aid: the shader clock in GHz while the device is doing whatever else it is doing — one wave on the
 * context stream compares the shader cycle counter (s_memtime) with the constant 100 MHz counter
 * (s_memrealtime) over ~`micros` microseconds.  Synchronises.  bench.py prices the VALU issue rate with it. */
int pislam_debug_shader_clock(pislam_ctx *ctx, int micros, double *ghz);

/* ---- descriptor matching ---------------------------- */

/* The reference ships no matcher (README.md:125-128 only names matching as
 * the consumer of these descriptors), so there is no reference interface to
 * mirror: the semantics below are this library's own.
 *
 * Brute-force Hamming matching of `words`-dword binary descriptors
 * (words in {1,2,4,8}, as orbCompute produces them — Orb.h:396).  For every
 * query i: idx[i] = the train index with the smallest Hamming distance (ties:
 * the smallest index; -1 if nt == 0), dist[i] = that distance (0xffffffff if
 * nt == 0), dist2[i] = the smallest distance among all OTHER train descriptors
 * (0xffffffff if nt < 2; for a ratio test).  nt <= 65535.  Host or device
 * pointers. */
int pislam_match_hamming(pislam_ctx *ctx, int words, const uint32_t *query, size_t nq,
                         const uint32_t *train, size_t nt, int32_t *idx, uint32_t *dist,
                         uint32_t *dist2);

/* Batched form on device-resident front-end outputs: pair b matches the first
 * min(qcounts[b], q_stride) descriptors of query[b] against the first
 * min(tcounts[b], t_stride) of train[b] (layouts [batch][stride][words], the
 * descriptor / count arrays of pislam_orb_frontend_batch; strides in
 * descriptors, t_stride <= 65535).  Outputs are [batch][q_stride]; entries
 * at and beyond the pair's query count are not written.  Device pointers
 * only; asynchronous on the context stream. */
int pislam_match_hamming_batch(pislam_ctx *ctx, int words, const uint32_t *query,
                               const uint32_t *qcounts, size_t q_stride, const uint32_t *train,
                               const uint32_t *tcounts, size_t t_stride, int batch, int32_t *idx,
                               uint32_t *dist, uint32_t *dist2);

/* Spatially windowed form for frame-to-frame tracking (DESIGN.md, section
 * 5.5): pair b matches query i < nq_b = min(qcounts[b], q_stride) only against
 * the train entries j < nt_b = min(tcounts[b], t_stride) near its position
 * (a count of PISLAM_COUNT_INVALID counts as 0).  Positions are encodeFast
 * words of the stacked pyramid (x = (k >> 12) & 0xfff, y = k & 0xfff; score
 * bits ignored), keypoints [batch][stride] as pislam_orb_frontend_batch writes
 * them; the level of a position is the level whose rectangle
 * [col0, col0+width) x [row0, row0+height) holds it.  Train j is a candidate
 * for query i when both have a level, the same level l, and
 * |xq - xt| <= radius[l] and |yq - yt| <= radius[l] (a square window in that
 * level's pixels).  Outputs as pislam_match_hamming_batch, restricted to the
 * candidates: idx = the candidate with the smallest Hamming distance (ties:
 * the smallest train index; -1 without candidates), dist = that distance
 * (0xffffffff without candidates), dist2 = the smallest distance among the
 * other candidates (0xffffffff with fewer than 2); idx indexes the caller's
 * train array.  A query position in no level has no candidates.  Outputs are
 * [batch][q_stride]; entries at and beyond nq_b are not written.
 * words in {1,2,4,8}; 1 <= nlevels <= 16, level rectangles non-empty,
 * disjoint, inside 12-bit coordinates; 0 <= radius[l] <= 4095;
 * t_stride <= 65535.  Anything else: PISLAM_ERR_INVALID.  Device pointers
 * only, except `levels` and `radius` (host arrays, read during the call).
 * Asynchronous on the context stream.  The workspace lives in the context and
 * grows on demand, which synchronises; after pislam_match_window_reserve of
 * the same or a larger shape the call allocates nothing and never
 * synchronises, so it can be captured into a hipGraph. */
int pislam_match_window_reserve(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                                const int32_t *radius, size_t t_stride, int batch);
int pislam_match_hamming_window_batch(pislam_ctx *ctx, int words,
                                      const pislam_level *levels, int nlevels, const int32_t *radius,
                                      const uint32_t *qkp, const uint32_t *qdesc, const uint32_t *qcounts,
                                      size_t q_stride, const uint32_t *tkp, const uint32_t *tdesc,
                                      const uint32_t *tcounts, size_t t_stride, int batch, int32_t *idx,
                                      uint32_t *dist, uint32_t *dist2);

/* Scale-aware guided form: matching in level-0
 * coordinates across pyramid levels, around an optional predicted position.
 * Pairs, counts, keypoint words, descriptor and output layouts, and the level
 * of a position are those of pislam_match_hamming_window_batch.  A position
 * on level l with level-local u = x - col0, v = y - row0 maps to
 * X = (u * s_l + 32768) >> 16, Y = (v * s_l + 32768) >> 16 (unsigned 32-bit
 * arithmetic), s_l = scale_q16[l] = level-0 pixels per level-l pixel in Q16.
 * Window centre (Xc, Yc): the query's own mapped position when qpred is NULL,
 * else qpred[(b * q_stride + i) * 2 + {0, 1}] (device int32 level-0
 * coordinates, clamped to [-2^20, 2^20]).  Train j on level lt is a candidate
 * for query i on level lq when |lq - lt| <= level_span,
 * |Xc - Xt| <= radius0[lq] and |Yc - Yt| <= radius0[lq] (the radius is in
 * level-0 pixels and indexed by the query's level).  A query position in no
 * level has no candidates, with or without a prediction.  Outputs as
 * pislam_match_hamming_window_batch, restricted to these candidates (best on
 * dist << 16 | j: ties go to the smallest train index; idx -1 and dist
 * 0xffffffff without candidates; dist2 0xffffffff with fewer than 2); entries
 * at and beyond nq_b are not written.  With level_span 0, every scale 65536,
 * qpred NULL and radius0 = radius the outputs equal the windowed matcher's.
 * words in {1,2,4,8}; 1 <= nlevels <= 16, level rectangles non-empty,
 * disjoint, inside 12-bit coordinates; 0 <= radius0[l] <= 65535;
 * 0 <= level_span <= nlevels - 1; 1 <= scale_q16[l] <= 2^20 and every level's
 * mapped extent ((width - 1) * s_l + 32768) >> 16 (likewise height) <= 65535;
 * t_stride <= 65535.  Anything else, or a host pointer where a device pointer
 * is required: PISLAM_ERR_INVALID, before anything is launched or written.
 * Device pointers only (qpred may be NULL), except `levels`, `scale_q16` and
 * `radius0` (host arrays, read during the call: a captured graph keeps its own
 * copy).  Asynchronous on the context stream; the workspace is the context's
 * own (not the windowed matcher's) and grows on demand, which synchronises;
 * after pislam_match_scaled_window_reserve of the same or a larger shape the
 * call allocates nothing and never synchronises, so it can be captured into a
 * hipGraph. */
int pislam_match_scaled_window_reserve(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                                       const int32_t *scale_q16, const int32_t *radius0, int level_span,
                                       size_t t_stride, int batch);
int pislam_match_hamming_scaled_window_batch(pislam_ctx *ctx, int words,
                                             const pislam_level *levels, int nlevels,
                                             const int32_t *scale_q16, const int32_t *radius0, int level_span,
                                             const uint32_t *qkp, const uint32_t *qdesc, const uint32_t *qcounts,
                                             const int32_t *qpred, size_t q_stride,
                                             const uint32_t *tkp, const uint32_t *tdesc, const uint32_t *tcounts,
                                             size_t t_stride, int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2);

/* Map-point search by projection, after ORB-SLAM's
 * ORBmatcher::SearchByProjection (TrackWithMotionModel, TrackLocalMap,
 * relocalisation): the queries are 3D map points with a descriptor each, the
 * train side is a frame's keypoints.  Pair b is one frame.  The train side
 * (tkp, tdesc, tcounts, t_stride, levels, nlevels, scale_q16), the counts
 * (min(count, stride), PISLAM_COUNT_INVALID as 0), the level of a train
 * position and its Q16 mapping to level 0 (Xt, Yt) are exactly those of
 * pislam_match_hamming_scaled_window_batch.  Query side, per pair b:
 *   pose    float [batch][12]   r0..r8 row-major, then t: Xc = R Xw + t (the
 *                               pose_in of pislam_pose_refine_batch)
 *   cam     float [batch][5]    fx, fy, cx, cy, bf; bf is read for finiteness
 *                               only
 *   xw      float [batch][q_stride][3]      map points
 *   qdesc   uint32 [batch][q_stride][words]
 *   qcounts uint32 [batch]                  nq_b = min(qcounts[b], q_stride)
 * and the query's level from exactly one of two modes:
 *   map mode    drange float [batch][q_stride][2] = (dmin, dmax) is given and
 *               qlevel is NULL; normal float [batch][q_stride][3] is optional.
 *   level mode  qlevel uint8 [batch][q_stride] is given, drange and normal
 *               are NULL (the motion model, or any caller that knows the level).
 * Host tables of nlevels entries, read during the call and carried by value in
 * the kernel arguments (a captured graph keeps its own copy): level_scale
 * float (ORB-SLAM's mvScaleFactors), radius_far and radius_near int32 in
 * level-0 pixels; radius_near may be NULL, which means radius_far.
 *
 * A pair whose 12 pose words or 5 cam words are not all finite, or whose fx
 * or fy is 0, has every query dead.  Otherwise, per query i < nq_b, in
 * binary32 with one rounding per written operation, in this order (R = pose
 * words 0..8 row-major, t = words 9..11, (X, Y, Z) = xw):
 *  1. x = ((R0*X + R1*Y) + R2*Z) + t0,  y = ((R3*X + R4*Y) + R5*Z) + t1,
 *     z = ((R6*X + R7*Y) + R8*Z) + t2.  Dead unless z >= 2^-10.
 *     iz = 1.0f / z,  pu = fx*(x*iz) + cx,  pv = fy*(y*iz) + cy.
 *  2. Dead unless pu >= min_x & pu <= max_x & pv >= min_y & pv <= max_y
 *     (a NaN fails).  Centre xc = (int32)floorf(pu + 0.5f),
 *     yc = (int32)floorf(pv + 0.5f).
 *  3. Map mode only: d = sqrt((x*x + y*y) + z*z), correctly rounded.  Dead
 *     unless dmin <= d & d <= dmax.
 *  4. Only with normal n: nc_k = (R[3k]*n0 + R[3k+1]*n1) + R[3k+2]*n2,
 *     c = (x*nc0 + y*nc1) + z*nc2.  Dead unless c >= cos_min * d; NEAR when
 *     c > cos_near * d.  (No division and no camera centre: |Xc| is the
 *     distance to it.)  Without normal there is no test and no query is near.
 *  5. Predicted level.  Map mode: pl = the number of l in 0 .. nlevels - 2
 *     with d * level_scale[l] < dmax (ORB-SLAM's ceil(log(dmax / d) / log s)
 *     clamped to the level range, without a logarithm).  Level mode:
 *     pl = qlevel[i]; dead when pl >= nlevels.
 *  6. r = near ? radius_near[pl] : radius_far[pl].
 *  7. Train j on level lt is a candidate when pl - level_below <= lt <=
 *     pl + level_above, |xc - Xt| <= r and |yc - Yt| <= r.
 *  8. idx, dist, dist2 as the scaled matcher writes them, restricted to these
 *     candidates: best and second on dist << 16 | j (ties: the smallest train
 *     index), idx -1 and dist 0xffffffff without candidates, dist2 0xffffffff
 *     with fewer than 2.  With second_same_level 1, dist2 is 0xffffffff when
 *     the runner-up's level differs from the best's (ORB-SLAM applies the
 *     ratio test within a level only), so pislam_match_select_batch can be
 *     used as it is.  pred int32 [batch][q_stride][2] = (xc, yc) and plevel
 *     uint8 [batch][q_stride] = pl (ORB-SLAM's "visible" flag: 0xff for a dead
 *     query) may each be NULL.  A dead query writes idx -1, dist and dist2
 *     0xffffffff, pred (0, 0), plevel 0xff.  Entries at and beyond nq_b are
 *     not written.
 * No float is summed across queries: the results are bit-for-bit reproducible
 * and independent of the launch shape.
 *
 * Limits: words in {1,2,4,8}; levels, nlevels, scale_q16 and t_stride as the
 * scaled matcher's; radius_far / radius_near 0..65535; level_scale finite,
 * level_scale[0] > 0, non-decreasing; min_x, max_x, min_y, max_y finite, within
 * +-2^20, min <= max; level_below, level_above 0..nlevels-1; second_same_level
 * 0 or 1; cos_min, cos_near any value; q_stride < 2^31.  Offsets use size_t
 * arithmetic throughout.  Any violation, both or neither of drange / qlevel,
 * normal with qlevel, or a host pointer where a device pointer is required:
 * PISLAM_ERR_INVALID, before anything is launched or written.  Device pointers
 * only, except levels, scale_q16, level_scale, radius_far, radius_near and p
 * (host, read during the call).  Asynchronous on the context stream; the
 * workspace is the context's own for this call (not the scaled matcher's) and
 * grows on demand, which synchronises; after pislam_match_projection_reserve
 * of the same or a larger shape the call allocates nothing and never
 * synchronises, so it can be captured into a hipGraph.
 *
 * Not here: the stereo right-coordinate test of SearchByProjection, the
 * reprojection test of ORBmatcher::Fuse (pislam_match_fuse_batch, below, is
 * this call with that test; the replacement of map points stays with the
 * caller), and the rotation histogram, which pislam_match_select_batch applies
 * from angles. */
typedef struct pislam_projection_params {
  float min_x, max_x, min_y, max_y; /* image bounds of pu, pv (ORB-SLAM: mnMinX ..) */
  float cos_min;                    /* viewing-angle limit (ORB-SLAM: 0.5) */
  float cos_near;                   /* above it the near radius applies (ORB-SLAM: 0.998) */
  int32_t level_below;              /* 0..nlevels-1 (local map: 1) */
  int32_t level_above;              /* 0..nlevels-1 (local map: 0) */
  int32_t second_same_level;        /* 0 / 1 */
} pislam_projection_params;
int pislam_match_projection_reserve(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                                    const int32_t *scale_q16, const int32_t *radius_far, const int32_t *radius_near,
                                    int level_below, int level_above, size_t t_stride, int batch);
int pislam_match_projection_batch(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                                  const int32_t *scale_q16, const float *level_scale, const int32_t *radius_far,
                                  const int32_t *radius_near, const pislam_projection_params *p, const float *pose,
                                  const float *cam, const float *xw, const float *normal, const float *drange,
                                  const uint8_t *qlevel, const uint32_t *qdesc, const uint32_t *qcounts, size_t q_stride,
                                  const uint32_t *tkp, const uint32_t *tdesc, const uint32_t *tcounts, size_t t_stride,
                                  int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2, int32_t *pred,
                                  uint8_t *plevel);

/* Map-point fusion search, after ORB-SLAM's
 * ORBmatcher::Fuse (LocalMapping::SearchInNeighbors, LoopClosing::
 * SearchAndFuse): project map points into a key frame and find, for each, the
 * keypoint it should have been observed at.  It is
 * pislam_match_projection_batch plus a per-candidate reprojection test: every
 * argument of that call has the same meaning, layout, limits and NULL rules
 * here, both query modes and the same pislam_projection_params included.  In
 * addition:
 *   tobs_q8    int32 [batch][t_stride][3]  device: (u, v, u_right) of train
 *              keypoint j in Q8 level-0 pixels, read by
 *              pislam_match_hamming_epipolar_batch's rule: a word that is read
 *              is clamped to [-2^22, 2^22], then float(q) * (1.0f / 256.0f);
 *              u_right == INT32_MIN marks a monocular keypoint (u_right is
 *              then not converted).  Only rows of candidates by step 7 of the
 *              projection call are read.
 *   qmask      uint8 [batch][q_stride]  device, or NULL: 0 makes query i dead
 *              (ORB-SLAM's pMP->IsInKeyFrame(pKF) or isBad()).
 *   inv_sigma2 HOST float [nlevels], finite and > 0, carried by value in the
 *              kernel arguments (ORB-SLAM's mvInvLevelSigma2).
 *   f          HOST pislam_fuse_params: chi2_mono (ORB-SLAM: 5.99f) and
 *              chi2_stereo (7.8f), both > 0; +inf is allowed, a NaN is refused.
 *   cam        bf = cam[4] is read, not only tested for finiteness.
 * Per query i < nq_b, in binary32 with one rounding per written operation (no
 * fused multiply-add, no reciprocal approximation; a comparison with a NaN is
 * false), the projection call's steps 1-8 apply word for word, except:
 *  0. A query whose qmask byte is 0 is dead: idx -1, dist and dist2
 *     0xffffffff, pred (0, 0), plevel 0xff.
 *  1. also makes pur = pu - bf*iz.
 *  7. Train j on level lt is a candidate iff it is one by the projection
 *     call's step 7 AND passes the reprojection test with (u, v, r) its
 *     tobs_q8 words: ex = pu - u, ey = pv - v.
 *       Monocular (r == INT32_MIN): e2 = ex*ex + ey*ey; passes iff
 *         e2 * inv_sigma2[lt] <= chi2_mono.
 *       Otherwise: er = pur - r, e2 = (ex*ex + ey*ey) + er*er; passes iff
 *         e2 * inv_sigma2[lt] <= chi2_stereo.
 *     lt is the level the train keypoint's POSITION (tkp) lies in, the level
 *     whose cell grid the keypoint is indexed in.
 * Equivalence: with both bounds +inf and qmask NULL all five outputs equal
 * pislam_match_projection_batch's on the same inputs, whatever tobs_q8 holds:
 * for a live query pu and pv lie inside the bounds, bf and iz are finite, so
 * e2 * inv_sigma2[lt] is never a NaN, and inf <= inf is true.
 *
 * Limits, refusals (PISLAM_ERR_INVALID before anything is launched or
 * written: every refusal of the projection call, chi2_mono or chi2_stereo not
 * > 0, inv_sigma2 NULL, not finite or not > 0, f NULL, tobs_q8 NULL or a host
 * pointer, qmask a host pointer), size_t offsets and asynchrony are the
 * projection call's.  The workspace is the context's own for this call (not
 * the projection matcher's: a graph captured for either call survives a
 * reserve of the other) and grows on demand, which synchronises; after
 * pislam_match_fuse_reserve of the same or a larger shape the call allocates
 * nothing and never synchronises, so it can be captured into a hipGraph.
 * Fuse(pKF, Scw, ...) of loop closing is this call with the pose (R, t / s) of
 * the similarity and both bounds +inf (ORB-SLAM2 applies no chi-square test
 * there).
 *
 * Not here: what follows a match (add the observation, or replace the point
 * with fewer observations by the other: the map is the caller's), and the
 * stereo right-coordinate test of the motion-model SearchByProjection.  The
 * descriptor and normal updates of the fused points are
 * pislam_map_points_update_batch, below, on the map after the caller's edit. */
typedef struct pislam_fuse_params {
  float chi2_mono;   /* > 0, +inf allowed (ORB-SLAM: 5.99f) */
  float chi2_stereo; /* > 0, +inf allowed (ORB-SLAM: 7.8f) */
} pislam_fuse_params;
int pislam_match_fuse_reserve(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                              const int32_t *scale_q16, const int32_t *radius_far, const int32_t *radius_near,
                              int level_below, int level_above, size_t t_stride, int batch);
int pislam_match_fuse_batch(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                            const int32_t *scale_q16, const float *level_scale, const int32_t *radius_far,
                            const int32_t *radius_near, const pislam_projection_params *p, const float *inv_sigma2,
                            const pislam_fuse_params *f, const float *pose, const float *cam, const float *xw,
                            const float *normal, const float *drange, const uint8_t *qlevel, const uint8_t *qmask,
                            const uint32_t *qdesc, const uint32_t *qcounts, size_t q_stride, const uint32_t *tkp,
                            const uint32_t *tdesc, const int32_t *tobs_q8, const uint32_t *tcounts, size_t t_stride,
                            int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2, int32_t *pred, uint8_t *plevel);

/* Rectified stereo matching: left <-> right
 * correspondences of rectified stereo pairs with an SAD sub-pixel refinement,
 * after ORB-SLAM2's Frame::ComputeStereoMatches, stated in integers.  Pair b
 * is (left b, right b); the left list is the query, the right list the train.
 * Pairs, counts, keypoint words, descriptor layouts, PISLAM_COUNT_INVALID as
 * 0, the level of a position (the rectangle that holds it) and the Q16
 * mapping X = (u * s_l + 32768) >> 16 (u = x - col0, v = y - row0
 * level-local; likewise Y) are those of
 * pislam_match_hamming_scaled_window_batch.  Both pyramids share `levels`.
 *  1. Band search: right j on level lr is a candidate for left i on level ll
 *     when |ll - lr| <= level_span, |Yl - Yr| <= row_radius0[lr] (level-0
 *     pixels, indexed by the RIGHT level) and min_disp <= Xl - Xr <= max_disp
 *     (signed).  idx[i] = the best candidate on dist << 16 | j (ties: the
 *     smallest j; -1 without candidates), dist[i] = its Hamming distance
 *     (0xffffffff without).  Both are written whether or not the match is
 *     accepted below.
 *  2. Steps 3-6 run only when dist[i] <= max_hamming (ORB-SLAM2: < 75 for
 *     256-bit descriptors).
 *  3. SAD refinement on level ll of both images, w = sad_radius,
 *     L = search_radius.  The right centre column on level ll is
 *     ur0 = floor((Xr * 65536 + floor(s_ll / 2)) / s_ll) (64-bit; the right
 *     keypoint's own u when lr == ll and s >= 65536).  For inc in [-L, L]:
 *     sad(inc) = sum over |dx|, |dy| <= w of
 *       |(Lp(ul+dx, vl+dy) - Lp(ul, vl)) - (Rp(ur0+inc+dx, vl+dy) - Rp(ur0+inc, vl))|
 *     where Lp / Rp are the bytes at
 *     pyr + b * pyramid_stride + (row0 + v) * vstep + col0 + u (the right
 *     patch uses the left row vl: the pair is rectified).  The match is
 *     rejected when any pixel this would read, for any inc, lies outside level
 *     ll's rectangle (a complete check; ORB-SLAM2's covers part of the range).
 *     Otherwise ib = the inc of the smallest sad (ties: the smallest inc); the
 *     match is rejected when ib = -L or ib = +L.
 *  4. Sub-pixel fit: d1, d2, d3 = sad(ib-1), sad(ib), sad(ib+1),
 *     num = d1 - d3, den = 2 (d1 + d3 - 2 d2) >= 0; delta_q8 = 0 if den == 0,
 *     else floor((512 num + den) / (2 den)) (floor division, not C
 *     truncation; |delta_q8| <= 128).
 *  5. Disparity in level-0 pixels, Q8: dl_q8 = 256 (ul - ur0 - ib) - delta_q8,
 *     disp_q8 = floor((dl_q8 * s_ll + 32768) / 65536) (signed 64-bit).  The
 *     match is accepted iff 256 min_disp <= disp_q8 <= 256 max_disp; then
 *     disp_q8 = max(disp_q8, 1) (callers may divide by it; ORB-SLAM2 clamps to
 *     0.01 px) and sad[i] = sad(ib).
 *  6. Median filter (median_filter = 1): m = pair b's accepted SADs sorted
 *     ascending, element n / 2; every accepted match with 10 sad > 21 m
 *     (sad > 1.5 * 1.4 * m) is rejected.  ORB-SLAM2 rejects with >=, which
 *     with m = 0 (routine on clean or synthetic input) rejects everything; the
 *     strict > keeps the zero-SAD matches.
 *  7. A rejected match gets disp_q8 = -1 and sad = 0xffffffff.  nstereo[b]
 *     (optional, device) = the matches accepted after the filter.  Entries at
 *     and beyond the pair's left count are not written.
 * Outputs idx, dist, disp_q8, sad are [batch][l_stride].
 * Limits: words in {1,2,4,8}; 1 <= nlevels <= 16, level rectangles non-empty,
 * disjoint, inside [0, rows) x [0, vstep) and 12-bit coordinates;
 * 1 <= scale_q16[l] <= 2^20 and every mapped extent <= 65535 (as the scaled
 * window matcher); 0 <= row_radius0[l] <= 65535;
 * 0 <= level_span <= nlevels - 1; 0 <= min_disp <= max_disp <= 65535;
 * max_hamming >= 0; 1 <= sad_radius <= 7; 1 <= search_radius <= 8;
 * median_filter in {0, 1}; r_stride <= 65535.  Anything else, or a host
 * pointer where a device pointer is required: PISLAM_ERR_INVALID, before
 * anything is launched or written.  Device pointers only (nstereo may be
 * NULL), except `levels`, `scale_q16`, `row_radius0` and `p` (host, read
 * during the call: a captured graph keeps its own copy).  Asynchronous on the
 * context stream, no host round trip; the workspace is the context's own (not
 * either window matcher's) and grows on demand, which synchronises; after
 * pislam_match_stereo_reserve of the same or a larger shape the call
 * allocates nothing and never synchronises, so it can be captured into a
 * hipGraph. */
typedef struct pislam_stereo_params {
  int32_t level_span, min_disp, max_disp, max_hamming, sad_radius, search_radius, median_filter;
} pislam_stereo_params;
int pislam_match_stereo_reserve(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                                const int32_t *scale_q16, const int32_t *row_radius0, const pislam_stereo_params *p,
                                size_t r_stride, int batch);
int pislam_match_stereo_batch(pislam_ctx *ctx, int words, const pislam_level *levels, int nlevels,
                              const int32_t *scale_q16, const int32_t *row_radius0, const pislam_stereo_params *p,
                              const uint8_t *left_pyr, const uint8_t *right_pyr, int vstep, int rows,
                              size_t pyramid_stride,
                              const uint32_t *lkp, const uint32_t *ldesc, const uint32_t *lcounts, size_t l_stride,
                              const uint32_t *rkp, const uint32_t *rdesc, const uint32_t *rcounts, size_t r_stride,
                              int batch, int32_t *idx, uint32_t *dist, int32_t *disp_q8, uint32_t *sad,
                              uint32_t *nstereo);

/* ---- pyramidal Lucas-Kanade tracking and sub-pixel match refinement ------ */

/* The 2-D photometric step, with two uses.  Refinement: after any matcher and
 * pislam_match_select_batch, start at the matched keypoint's position and get the Q8 sub-pixel position in the next
 * frame.  Tracking: start at the previous position, or a prediction, and follow points coarse to fine through the
 * stacked pyramid, with no descriptors.  The reference ships nothing of the kind: the semantics are this library's own,
 * after the inverse-compositional Lucas-Kanade step (template gradients, as in Basalt's patch tracker; OpenCV's
 * calcOpticalFlowPyrLK was not run against this), stated in integers from end to end.  This comment is the contract.
 *
 * Buffers.  Pair b is (prev pyramid b, next pyramid b), both uint8 [rows][vstep] at + b * pyramid_stride, both sharing
 * `levels`.  pts_q8 and guess_q8 are device int32 [batch][stride][2] holding (x, y): stacked-pyramid coordinates in
 * Q8 (256 is one pixel, pixel centres lie at integers).  guess_q8 is optional: NULL means the guess is the point
 * itself.  n_b = min(counts[b], stride); PISLAM_COUNT_INVALID counts as 0; entries at and beyond n_b are not written.
 * Outputs: next_q8 [batch][stride][2], status and err [batch][stride], ntracked [batch] (optional, device).  levels,
 * scale_q16 and p are host arrays, read during the call (a captured graph keeps its own copy).
 *
 * Level and chain.  Point and guess coordinates are clamped to [-2^20, 2^20] first.  The point's level l is the
 * rectangle that holds (x >> 8, y >> 8); with no such rectangle status = 1, next_q8 = the guess, err = 0xffffffff.
 * Level-local coordinates: u = x - 256 * col0, v = y - 256 * row0 (the guess likewise, with level l's origin).  The
 * chain is c_m = l + m * level_step for m = M .. 0, M = min(max_coarse, (nlevels - 1 - l) / level_step).  A level-l
 * coordinate maps to level c, per axis in signed 64-bit with floor division, as
 *   u_c = floor((u_l * s_l + floor(s_c / 2)) / s_c),     s = scale_q16,
 * and back by the same formula with the roles exchanged; either result is clamped to [-2^22, 2^22] (no position that
 * far out is inside a level; with scale tables that really describe one pyramid the clamp is never reached).  q
 * starts as the guess.  For each coarse level (m > 0): map p and q to it and run the level procedure; if it ends with
 * code 0, map its q back to level l and replace q, otherwise q is unchanged.  The own level (m = 0) decides the
 * outputs.
 *
 * Level procedure, on a level of width W and height H with p and q level-local Q8, w = win_radius:
 *  1. Sampling.  With x0 = x >> 8, ax = x & 255, likewise y0 and ay (arithmetic shifts):
 *       Smp(x, y) = ((256-ax)*(256-ay)*B(x0,y0) + ax*(256-ay)*B(x0+1,y0) + (256-ax)*ay*B(x0,y0+1) + ax*ay*B(x0+1,y0+1)
 *                    + 1024) >> 11,
 *     Q5, 0..8160; B(x, y) is the level's byte at (row0 + y) * vstep + col0 + x.  inside(x, y, m) is true iff
 *     x0 - m >= 0, y0 - m >= 0, x0 + m + 1 <= W - 1 and y0 + m + 1 <= H - 1.  No byte outside the level's rectangle
 *     is ever read.
 *  2. Template (prev).  If !inside(p, w + 1) the code is 1.  T(dx, dy) = Smp(px + 256 dx, py + 256 dy) for
 *     |dx|, |dy| <= w + 1.  On the window |dx|, |dy| <= w: gx = (T(dx+1,dy) - T(dx-1,dy) + 4) >> 3 and
 *     gy = (T(dx,dy+1) - T(dx,dy-1) + 4) >> 3 (arithmetic shift; |g| <= 1020).  A11 = sum gx^2, A12 = sum gx gy,
 *     A22 = sum gy^2 (1020^2 * 225 < 2^28).
 *  3. Conditioning.  n = (2w+1)^2, t = min_eig * n, det = A11 * A22 - A12^2 (64 bits).  The code is 2 unless
 *     det > 0, A11 + A22 >= 2 t and (A11 - t) * (A22 - t) - A12^2 >= 0: lambda_min(A) >= t without a square root.
 *  4. Search (next).  If !inside(q, w) the code is 3.  it = 0, then loop:
 *       r = Smp(qx + 256 dx, qy + 256 dy) - T(dx, dy) over the window, sad = sum |r|.
 *       If it == max_iters: stop with code 0.
 *       b1 = sum r gx, b2 = sum r gy (8160 * 1020 * 225 < 2^31).  nx = A22 * b1 - A12 * b2, ny = A11 * b2 - A12 * b1.
 *       step per axis = floor((-64 * n_axis + floor(det / 2)) / det) in exact integers (-64 n does not fit 64 bits in
 *       the worst case, |n| < 2^60: the library splits n = k * det + rem and compares k with the clamp first), then
 *       clamped to +- max_step_q8.
 *       it += 1, q' = q + step.  If !inside(q', w): stop with code 3 and keep q.  Otherwise q = q'.
 *       If both |step| <= eps_q8: recompute sad at q and stop with code 0.
 *  5. Own level only: if the code is 0, max_err > 0 and sad > max_err * n, the code is 4.
 *
 * Outputs.  next_q8 = the final q on level l, back in stacked coordinates (+ 256 * col0, + 256 * row0): the q that
 * entered the level when the own level could not start (code 1 or 2), the last position that was inside when it
 * stopped on code 3.  status = code | it << 8, `it` the own level's iteration count (0 for codes 1 and 2); it ==
 * max_iters with code 0 means the limit was hit, which still counts as tracked, as in OpenCV.  err = sad for codes 0
 * and 4, else 0xffffffff.  ntracked[b] = the points of pair b with code 0.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= nlevels <= 16, level rectangles non-empty, disjoint,
 * inside [0, rows) x [0, vstep) and 12-bit coordinates, 1 <= scale_q16[l] <= 2^20 and every mapped extent <= 65535
 * (as pislam_match_stereo_batch); stride < 2^31; batch >= 0 with no upper limit (batch == 0 is a no-op that returns
 * PISLAM_OK after the checks of p, the tables, batch and stride; the data pointers are not looked at then).  Offsets
 * use size_t arithmetic throughout: strides may carry a batch past 4 GiB.  No output may overlap an input or another
 * output, except that next_q8 may be exactly guess_q8: each point reads its guess before it writes.  Any violation, or
 * a host pointer where a device pointer is required: PISLAM_ERR_INVALID, before anything is launched or written.
 * Asynchronous on the context stream; no workspace, no host round trip: the call can be captured into a hipGraph as
 * it is, so there is no reserve call. */
typedef struct pislam_lk_params {
  int32_t win_radius;   /* w: window (2w+1)^2, 1..7 */
  int32_t max_iters;    /* 1..32 */
  int32_t eps_q8;       /* stop when both |step| <= eps_q8, 0..255 */
  int32_t max_step_q8;  /* per-axis clamp of one step, 1..4096 */
  int32_t level_step;   /* distance between chain levels, 1..15 */
  int32_t max_coarse;   /* coarser levels used above the point's own, 0..15 */
  int32_t min_eig;      /* smallest eigenvalue of A per window pixel, >= 0, <= 2^20 */
  int32_t max_err;      /* mean |residual| limit (Q5 grey levels), 0 = no limit, <= 8160 */
} pislam_lk_params;
int pislam_track_lk_batch(pislam_ctx *ctx, const pislam_lk_params *p,
                          const pislam_level *levels, int nlevels, const int32_t *scale_q16,
                          const uint8_t *prev_pyr, const uint8_t *next_pyr, int vstep, int rows, size_t pyramid_stride,
                          const int32_t *pts_q8, const uint32_t *counts, const int32_t *guess_q8, size_t stride,
                          int batch, int32_t *next_q8, uint32_t *status, uint32_t *err, uint32_t *ntracked);

/* ---- bag of words: quantisation, vector, word-guided matching ----------- */

/* Matching without a position (relocalisation, loop closure, key frames
 * without a pose), after DBoW2 / ORB-SLAM's SearchByBoW, stated in integers
 * (DESIGN.md, section 5.5).  The reference ships neither a vocabulary nor a
 * matcher: the semantics are this library's own.
 *
 * The vocabulary is a rooted tree of `nnodes` cluster centres given by HOST
 * arrays: node_desc [nnodes][words], first_child [nnodes], child_count
 * [nnodes].  Node 0 is the root (its descriptor is ignored); the children of
 * node n are the nodes first_child[n] .. first_child[n] + child_count[n] - 1;
 * child_count[n] == 0 makes n a leaf (its first_child is ignored).
 * Refused with PISLAM_ERR_INVALID: words not in {1,2,4,8}; nnodes outside
 * 2 .. 2^24; a child_count outside 0 .. 32; the root a leaf; a child range that
 * leaves [1, nnodes), that does not lie strictly after its parent
 * (first_child[n] > n) or that overlaps another node's range; a node other
 * than the root that is nobody's child; a leaf deeper than 16 (root = depth
 * 0); group_depth outside 0 .. 16.
 *   Word id:  the leaves numbered 0 .. nwords - 1 in ascending node index.
 *   Group id: every node at depth group_depth and every leaf shallower than
 *             that, numbered 0 .. ngroups - 1 in ascending node index; the group
 *             of a word is the one of these nodes on its path.  (group_depth 0:
 *             one group, the root; a group_depth at or below the deepest leaf:
 *             groups = words.  ORB-SLAM's levelsup = 4 on its 10-ary, 6-level
 *             vocabulary is group_depth 2: 100 groups.)
 * pislam_vocab_create validates, repacks and uploads on the context's device
 * and stream and synchronises; the host arrays are not referenced afterwards.
 * A vocabulary is immutable and may be used by any context of the same device;
 * destroy it after the work that uses it has completed.  pislam_vocab_nwords /
 * _ngroups: the counts (PISLAM_ERR_INVALID for NULL). */
typedef struct pislam_vocab pislam_vocab;
int pislam_vocab_create(pislam_ctx *ctx, int words, int nnodes, const uint32_t *node_desc,
                        const int32_t *first_child, const int32_t *child_count, int group_depth,
                        pislam_vocab **vocab);
int pislam_vocab_destroy(pislam_vocab *vocab);
int pislam_vocab_nwords(const pislam_vocab *vocab);
int pislam_vocab_ngroups(const pislam_vocab *vocab);

/* Quantisation.  For pyramid b and every i < n_b = min(counts[b], stride)
 * (PISLAM_COUNT_INVALID counts as 0): start at the root; at an inner node n go
 * to the child c that minimises
 *   hamming(desc[b][i], node_desc[c]) << 8 | (c - first_child[n])
 * (ties: the smallest child index); stop at a leaf.  word[b][i] = the leaf's
 * word id, group[b][i] = its group id, wdist[b][i] = the Hamming distance to
 * the leaf's descriptor; group and wdist may each be NULL.  Layouts
 * [batch][stride]; desc [batch][stride][words] with the vocabulary's words, as
 * pislam_orb_frontend_batch writes it.  Entries at and beyond n_b are not
 * written.  Device pointers only; a host pointer, a NULL desc / counts / word or
 * a vocabulary of another device: PISLAM_ERR_INVALID before anything is
 * launched or written.  Asynchronous on the context stream; no workspace, so
 * the call can be captured into a hipGraph as it is. */
int pislam_bow_transform_batch(pislam_ctx *ctx, const pislam_vocab *vocab, const uint32_t *desc,
                               const uint32_t *counts, size_t stride, int batch,
                               uint32_t *word, uint32_t *group, uint32_t *wdist);

/* The bag-of-words vector.  bow_word[b][0 .. bow_n[b]) = the distinct values
 * of word[b][0 .. n_b) in ascending order, bow_tf[b][k] = how often
 * bow_word[b][k] occurs, bow_n[b] = their number; slots at and beyond bow_n[b]
 * are not written.  Layouts [batch][stride], bow_n [batch]; stride <= 16384
 * (one workgroup sorts a pyramid's words in LDS), more is refused.  Any uint32
 * is a word here.  Weights (idf), normalisation and scores are the caller's.
 * Device pointers only; asynchronous on the context stream; no workspace. */
int pislam_bow_vector_batch(pislam_ctx *ctx, const uint32_t *word, const uint32_t *counts, size_t stride, int batch,
                            uint32_t *bow_word, uint32_t *bow_tf, uint32_t *bow_n);

/* Word-guided matching.  Pairs, counts, descriptor and output layouts as
 * pislam_match_hamming_window_batch; qgroup [batch][q_stride] and tgroup
 * [batch][t_stride] are group ids as pislam_bow_transform_batch writes them.
 * Train j is a candidate for query i of the same pair iff
 * qgroup[b][i] == tgroup[b][j] and both are below ngroups; an id at or above
 * ngroups has no candidates and is not indexed.  Outputs as
 * pislam_match_hamming_window_batch, restricted to these candidates (best on
 * dist << 16 | j: ties go to the smallest train index; idx -1 and dist
 * 0xffffffff without candidates; dist2 0xffffffff with fewer than 2); entries
 * at and beyond nq_b are not written.  With ngroups 1 and every group 0 the
 * outputs equal pislam_match_hamming_batch's.
 * words in {1,2,4,8}; 1 <= ngroups <= 16384; t_stride <= 65535.  Anything
 * else, or a host pointer where a device pointer is required:
 * PISLAM_ERR_INVALID, before anything is launched or written.  Device
 * pointers only.  Asynchronous on the context stream; the workspace is the
 * context's own (no other matcher's) and grows on demand, which synchronises;
 * after pislam_match_bow_reserve of the same or a larger shape the call
 * allocates nothing and never synchronises, so it can be captured into a
 * hipGraph. */
int pislam_match_bow_reserve(pislam_ctx *ctx, int words, int ngroups, size_t t_stride, int batch);
int pislam_match_hamming_bow_batch(pislam_ctx *ctx, int words, int ngroups,
                                   const uint32_t *qdesc, const uint32_t *qgroup, const uint32_t *qcounts, size_t q_stride,
                                   const uint32_t *tdesc, const uint32_t *tgroup, const uint32_t *tcounts, size_t t_stride,
                                   int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2);

/* ---- after the match: angle bins and match selection --------------------- */

/* The rotation bin of every keypoint of a batch of pyramids (DESIGN.md,
 * section 5.5): what pislam_orb_frontend_batch computes for each keypoint
 * inside its descriptor pass and does not hand out.  The call covers pyramid b
 * (pyramids + b * pyramid_stride, uint8 [rows][vstep]) and every
 * i < n_b = min(counts[b], stride); PISLAM_COUNT_INVALID counts as 0.
 * angles[b][i] = the rotation bin, 0 .. 29 (12 degrees each), that orbCompute
 * uses for the position keypoints[b][i] (x = (k >> 12) & 0xfff, y = k & 0xfff;
 * score bits ignored) on pyramid b: the moments of Orb.h:80-308 over the
 * radius-15 circular patch, then the bin of Orb.h:310-387 — the same bits the
 * descriptor pass rotates its pattern by.  A position whose patch would leave
 * the buffer (x < 15, x > vstep - 16, y < 15 or y > rows - 16) gets 0xff; no
 * byte is read for it.  Entries at and beyond n_b are not written.
 * Layouts: keypoints uint32 [batch][stride] as pislam_orb_frontend_batch writes
 * them, angles uint8 [batch][stride].  Device pointers only: a host or NULL
 * pointer, batch < 0, vstep < 31, rows < 31 or stride >= 2^31:
 * PISLAM_ERR_INVALID, before anything is launched or written.  batch == 0 is a
 * no-op that returns PISLAM_OK.  Asynchronous on the context stream; no
 * workspace, so the call can be captured into a hipGraph as it is. */
int pislam_orb_angles_batch(pislam_ctx *ctx, const uint8_t *pyramids, int vstep, int rows, size_t pyramid_stride,
                            const uint32_t *keypoints, const uint32_t *counts, size_t stride, int batch,
                            uint8_t *angles);

/* Match selection: the four integer steps ORB-SLAM
 * runs after every search (SearchByBoW, SearchForInitialization,
 * SearchByProjection) — distance threshold, nearest-neighbour ratio,
 * one-to-one claim of a train descriptor, rotation-consistency histogram
 * (HISTO_LENGTH = 30, ComputeThreeMaxima, the 10 % rule) — and the compaction
 * of the survivors into pair lists, on the device.  The reference ships
 * nothing of the kind: the semantics are this library's own.
 *
 * Inputs.  idx, dist, dist2 are [batch][q_stride] as any matcher of this
 * library writes them; dist2 may be NULL (the stereo matcher has none),
 * ratio_den must then be 0.  back_idx is [batch][t_stride] or NULL: the idx of
 * the reverse match, train -> query (the caller runs any matcher with the roles
 * swapped).  qangle [batch][q_stride] and tangle [batch][t_stride] are uint8
 * as pislam_orb_angles_batch writes them; both must be non-NULL if and only if
 * rot_keep > 0.  nq_b / nt_b = qcounts[b] / tcounts[b] clamped to the strides;
 * PISLAM_COUNT_INVALID counts as 0.
 *
 * Steps.  Each query i < nq_b takes the FIRST test it fails; status[b][i]
 * records which.  With j = idx[b][i]:
 *  1. no match: j < 0 or j >= nt_b.
 *  2. distance: dist > max_dist.
 *  3. ratio: ratio_den > 0, dist2 != 0xffffffff and
 *     dist * ratio_den >= dist2 * ratio_num (64-bit).  A query without a second
 *     candidate (dist2 == 0xffffffff) passes.
 *  4. cross-check: back_idx != NULL and back_idx[b][j] != i.
 *  5. uniqueness: unique == 1 and another query that passed tests 1-4 has the
 *     same j with a smaller key dist << 32 | i: the smallest distance wins, ties
 *     go to the smallest query index.
 *  6. rotation: rot_keep > 0.  A survivor of tests 1-5 with qangle[i] >= 30 or
 *     tangle[j] >= 30 fails and is not counted.  Every other survivor counts
 *     into h[(qangle[i] - tangle[j] + 30) % 30].  The 30 bins are ranked by
 *     descending count, ties to the smaller bin; `top` is rank 0.  Bin k is kept
 *     iff rank(k) < rot_keep, h[k] >= 1 and 100 * h[k] >= rot_min_pct * h[top].
 *     A survivor whose bin is not kept fails.
 * Queries that fail nothing are selected: status 0.
 *
 * Outputs.  sel_q[b][0 .. nsel[b]) = the selected queries in ascending order,
 * sel_t their j, nsel[b] their number; sel_q / sel_t are [batch][q_stride] and
 * slots at and beyond nsel[b] are not written.  status (uint8
 * [batch][q_stride], optional) = 0 or the number of the failed test; entries at
 * and beyond nq_b are not written.  rot_hist (uint32 [batch][30], optional) = h
 * before pruning; every row is written in full, all zero when rot_keep == 0.
 * ORB-SLAM's settings are {50, 6..9, 10, 1, 3, 10}.  With {256, 0, 0, 0, 0, 0}
 * and back_idx NULL the selection is every query with a valid idx.
 *
 * Limits: t_stride <= 65535; 1 <= q_stride <= 2^22; 0 <= batch <= 65535; the
 * parameter ranges below.  Anything else, a host or NULL pointer where a device
 * pointer is required, or a violated NULL rule (dist2 against ratio_den, the
 * angles against rot_keep): PISLAM_ERR_INVALID, before anything is launched or
 * written.  `p` is a host struct, read during the call.  Asynchronous on the
 * context stream, no host round trip and no workspace: the call can be
 * captured into a hipGraph as it is, and no reserve function exists because
 * none is needed.  One workgroup selects a pair.  Its uniqueness table covers
 * 16384 train indices at a time: with nt_b <= 16384 it is filled once per call;
 * a larger nt_b is walked in 2 .. 4 chunks, and the compaction then fills a
 * chunk again for each block of 1024 queries that refers to it (slower, same
 * results). */
typedef struct pislam_select_params {
  int32_t max_dist;             /* keep dist <= max_dist; 0 .. 256                                             */
  int32_t ratio_num, ratio_den; /* keep dist * ratio_den < dist2 * ratio_num; ratio_den 0 = off;
                                   otherwise 1 <= ratio_num <= ratio_den <= 65535                              */
  int32_t unique;               /* 0 / 1: a train index is given to one query only                             */
  int32_t rot_keep;             /* 0 = no rotation check; 1 .. 30 = histogram bins kept (ORB-SLAM: 3)          */
  int32_t rot_min_pct;          /* 0 .. 100: a kept bin holds at least this share of the top bin (ORB-SLAM: 10) */
} pislam_select_params;
int pislam_match_select_batch(pislam_ctx *ctx, const pislam_select_params *p,
                              const int32_t *idx, const uint32_t *dist, const uint32_t *dist2,
                              const uint32_t *qcounts, size_t q_stride,
                              const uint32_t *tcounts, size_t t_stride,
                              const int32_t *back_idx, const uint8_t *qangle, const uint8_t *tangle, int batch,
                              int32_t *sel_q, int32_t *sel_t, uint32_t *nsel, uint8_t *status, uint32_t *rot_hist);

/* ---- bag of words: integer weights and the key-frame database ------------ */

/* Place recognition (relocalisation, loop detection), after DBoW2's
 * Database::query and ORB-SLAM's KeyFrameDatabase::Detect*Candidates, stated
 * in integers: the step between
 * pislam_bow_vector_batch and pislam_match_hamming_bow_batch.  The reference
 * ships nothing of the kind: the semantics are this library's own.
 *
 * Weights.  Inputs are what pislam_bow_vector_batch wrote ([batch][stride],
 * n_b = bow_n[b] clamped to stride, PISLAM_COUNT_INVALID counts as 0;
 * stride <= 16384).  idf is a DEVICE array [nwords] of the caller's
 * fixed-point idf (any scale; a value above 65535 counts as 65535); NULL means
 * 1 for every word.  With a_k = bow_tf[b][k] * idf[bow_word[b][k]] (0 for a word
 * >= nwords) and A = the sum of a_k over k < n_b, in 64 bits:
 *   bow_weight[b][k] = A == 0 ? 0 : (a_k << 24) / A      (floor; Q24)
 * so the weights of a frame sum to at most 2^24.  (The tf of a vector sum to at
 * most 16384, so a_k and A stay below 2^30; for other inputs the arithmetic is
 * modulo 2^64.)  Slots at and beyond n_b are not written.  Device pointers
 * only; asynchronous on the context stream; no workspace. */
int pislam_bow_weight_batch(pislam_ctx *ctx, const uint32_t *bow_word, const uint32_t *bow_tf, const uint32_t *bow_n,
                            size_t stride, int batch, const uint32_t *idf, uint32_t nwords, uint32_t *bow_weight);

/* The database holds up to `capacity` key frames (1 .. 2^20) of at most
 * `stride` entries (word, weight) each (1 .. 16384) over the words
 * 0 .. nwords - 1 (1 .. 2^24); capacity * stride <= 2^31.  All device memory
 * (20 bytes per entry of capacity * stride, 12 per word, 5 per key frame) is
 * allocated by pislam_bowdb_create on the context's device
 * (PISLAM_ERR_NOMEM when it cannot be had); nothing allocates later.  It may be
 * used by any context of that device, by one stream at a time.
 *   add     Frame b of the call becomes key frame id = size + b; ids are never
 *           reused; *first_id (HOST, may be NULL) = the first.  Inputs as the
 *           vector and weight calls write them; the add's stride may differ from
 *           the database's: a bow_n[b] above the database's stride is clamped to
 *           it (the first entries are kept).  An entry with a word >= nwords is
 *           stored but not indexed.  Entries need not be sorted.  The id count
 *           is host state: an add that would pass `capacity`, or any bad
 *           argument, returns PISLAM_ERR_INVALID before anything is launched
 *           and leaves the database as it was.  The inverted file (CSR over the
 *           words) is rebuilt by every add.
 *   remove  marks ids (HOST array) dead.  An unknown, already dead or repeated
 *           id: PISLAM_ERR_INVALID, nothing changed.  A dead key frame never
 *           appears in a result and does not count towards max_common.
 *   clear   empties the database and restarts ids at 0.
 *   size    ids handed out so far (removed ones included).
 * add, remove and clear are asynchronous on the context stream and ordered
 * against queries on it; they change host state and are not meant to be
 * captured into a hipGraph.  The number of key frames and the liveness flags
 * the QUERY reads live in device memory: a captured query replays against the
 * database as it is at replay time.  Destroy a database after the work that
 * uses it has completed. */
typedef struct pislam_bowdb pislam_bowdb;
int pislam_bowdb_create(pislam_ctx *ctx, uint32_t nwords, size_t stride, int capacity, pislam_bowdb **db);
int pislam_bowdb_destroy(pislam_bowdb *db);
int pislam_bowdb_size(const pislam_bowdb *db);
int pislam_bowdb_add_batch(pislam_ctx *ctx, pislam_bowdb *db, const uint32_t *bow_word, const uint32_t *bow_weight,
                           const uint32_t *bow_n, size_t stride, int batch, int32_t *first_id);
int pislam_bowdb_remove(pislam_ctx *ctx, pislam_bowdb *db, const int32_t *ids, int n);
int pislam_bowdb_clear(pislam_ctx *ctx, pislam_bowdb *db);

/* The query.  For query b (entries i < n_b of q_word / q_weight [batch][stride],
 * n_b = q_n[b] clamped to stride, stride <= 16384) and every key frame k, over
 * the words < nwords that both hold (query entry i, entry j of k):
 *   common[b][k] = the number of such words                         (<= 16384)
 *   score[b][k]  = the sum over them of min(q_weight[b][i], weight_k[j])  (<= 2^24)
 * score / 2^24 is DBoW2's L1 score 1 - 0.5 * |v/|v| - w/|w||_1 of the two tf-idf
 * vectors with every weight floored to Q24.
 *   eligible   k is alive and k < id_limit[b] (id_limit: DEVICE [batch] or NULL
 *              = every key frame; a limit <= 0: none).
 *   max_common[b] = the largest common[b][k] over eligible k (0 without one).
 *   candidate  k is eligible, common >= 1 and
 *              common * 100 >= min_common_pct * max_common[b]  (0 .. 100).
 *   top_id[b][0 .. topk) = the candidates by descending score, ties to the
 *              smaller id; top_score / top_common their values; with fewer than
 *              topk candidates the rest of the row is -1 / 0 / 0.  Every row is
 *              written in full.  topk 1 .. 64; layouts [batch][topk],
 *              max_common [batch].
 * These results are defined for frames, on both sides, whose words are
 * distinct and whose weights sum to at most 2^24: what the vector and weight
 * calls write.  For other inputs the VALUES are unspecified, but every access
 * stays in bounds and top_id holds -1 or an eligible id.
 * Device pointers only; batch 0 .. 65535; anything else, a NULL or host pointer
 * where a device pointer is required, or a database of another device:
 * PISLAM_ERR_INVALID before anything is launched or written.  Asynchronous on
 * the context stream.  The workspace is the context's own (no matcher's) and
 * grows on demand, which synchronises; after pislam_bowdb_query_reserve of the
 * same or a larger shape the call allocates nothing and can be captured into a
 * hipGraph together with the transform, vector, weight and guided match calls.
 * Workspace bytes (each term rounded up to 256), C = capacity rounded up to
 * even, S = ceil(capacity / 8192):
 *   batch * (6 * C + 4)  +  (S > 1 ? 12 * batch * S * topk : 0)
 * PISLAM_ERR_NOMEM when it cannot be had (the context's workspace is then
 * empty; a later, smaller call allocates again). */
int pislam_bowdb_query_reserve(pislam_ctx *ctx, const pislam_bowdb *db, int batch, int topk);
int pislam_bowdb_query_batch(pislam_ctx *ctx, const pislam_bowdb *db, const uint32_t *q_word, const uint32_t *q_weight,
                             const uint32_t *q_n, size_t stride, int batch, const int32_t *id_limit, int min_common_pct,
                             int topk, int32_t *top_id, uint32_t *top_score, uint32_t *top_common, uint32_t *max_common);

/* ---- two-view geometry: batched RANSAC for F and H ------------------------ */

/* Geometric verification of matched point lists: per pair, a fundamental matrix (model 0) or a
 * homography (model 1) by RANSAC over a FIXED number of hypotheses, scored as ORB-SLAM's Initializer scores them
 * (CheckFundamental / CheckHomography), with the inlier mask of the winner.  Run it once per model and compare the
 * scores (SH / (SH + SF)) to choose between them.  The reference ships nothing of the kind: the semantics are this
 * library's own, stated so that integers and individually rounded binary32 operations reproduce every output word.
 * This comment is the contract.  "float(v)" is the conversion of an integer to binary32, round to nearest even; every
 * +, -, *, / below on floats is ONE binary32 operation rounded to nearest even, in the order the parentheses give
 * (a + b + c means (a + b) + c); no fused multiply-add, no reciprocal or fast-division approximation, no square root;
 * denormals are kept.
 *
 * Inputs.  p1_q8, p2_q8: device int32 [batch][stride][2], (x, y) of match i of pair b in image 1 and image 2, level-0
 * pixels in Q8.  counts: device uint32 [batch]; n = min(counts[b], stride), PISLAM_COUNT_INVALID counts as 0.  Every
 * coordinate is clamped to [-2^20, 2^20] first.  m = 8 (model 0) or 4 (model 1) matches make a hypothesis.
 *
 * Normalisation, per image, in signed 64-bit integers: Sx = sum x_i, Sy = sum y_i, ex_i = n * x_i - Sx,
 * ey_i = n * y_i - Sy, D = sum |ex_i| + sum |ey_i| (below 2^53 for stride <= 16384).  With k = float(2 * n * n) /
 * float(D), the normalised point is (float(ex_i) * k, float(ey_i) * k); one scale per image, so a normalised distance
 * is a pixel distance times s = (256.0f * float(n)) * k.  Below, (x1, y1) and (x2, y2) are the normalised points of a
 * match, and w_I = 1.0f / (t_I * t_I) with t_I = s_I * (float(sigma_q8) / 256.0f) for image I = 1, 2.
 * n < m, D1 == 0 or D2 == 0: "no model" (see Outputs).
 *
 * Sampling.  mix(x) on uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   hash(b, k, j) = mix(mix(mix(seed + 0x9e3779b9 * b) ^ (0x85ebca6b * (k + 1))) ^ (0xc2b2ae35 * (j + 1)))   (mod 2^32)
 * Draw j = 0 .. m - 1 of hypothesis k of pair b: r = (hash(b, k, j) * (n - j)) >> 32 (64-bit product), then for every
 * index c drawn before, in ASCENDING order of c: if r >= c then r += 1.  The m indices are distinct, and n == m draws
 * every match.  Row order below is draw order.
 *
 * Solve.  An 8 x 9 system [A | b] whose unknowns are the first eight model entries, row-major; the ninth is 1.0f.
 *   model 0, one row per drawn match:  x2*x1, x2*y1, x2, y2*x1, y2*y1, y2, x1, y1 | -1.0f       (x2' F x1 = 0)
 *   model 1, two rows per drawn match: x1, y1, 1, 0, 0, 0, -(x2*x1), -(x2*y1) | x2
 *                                      0, 0, 0, x1, y1, 1, -(y2*x1), -(y2*y1) | y2              (x2 ~ H x1)
 * Gaussian elimination with partial pivoting, for c = 0 .. 7:
 *   for r = c+1 .. 7 in turn: if |A[r][c]| > |A[c][c]|, rows r and c are exchanged (so row c ends as the FIRST row of
 *     largest magnitude in column c; the rows passed over stay in the order this leaves them in);
 *   the hypothesis is invalid unless |A[c][c]| >= 2^-20 (a NaN fails);
 *   inv = 1.0f / A[c][c];  for r = c+1 .. 7: f = A[r][c] * inv;  for j = c+1 .. 8: A[r][j] = A[r][j] - f * A[c][j].
 * Back substitution, r = 7 .. 0: t = A[r][8]; for j = r+1 .. 7 ascending: t = t - A[r][j] * x[j];  x[r] = t / A[r][r].
 * The hypothesis is also invalid when an x[r] is not finite.  An invalid hypothesis scores 0.  F is NOT forced to
 * rank 2: a caller who decomposes it does that on the host, after refitting from the inliers.
 *
 * Scoring.  For a 3 x 3 matrix M (row-major m0 .. m8) and points (xa, ya), (xb, yb):
 *   line(M, a, b, w):     A = (m0*xa + m1*ya) + m2,  B = (m3*xa + m4*ya) + m5,  C = (m6*xa + m7*ya) + m8,
 *                         N = (A*xb + B*yb) + C,  chi2 = ((N*N) / (A*A + B*B)) * w
 *   transfer(M, a, b, w): I = 1.0f / ((m6*xa + m7*ya) + m8),  u = ((m0*xa + m1*ya) + m2) * I,
 *                         v = ((m3*xa + m4*ya) + m5) * I,  du = xb - u, dv = yb - v,  chi2 = (du*du + dv*dv) * w
 *   model 0: chi2_a = line(F, p1, p2, w_2), chi2_b = line(F transposed, p2, p1, w_1); th = 3.841f.
 *   model 1: chi2_a = transfer(H, p1, p2, w_2), chi2_b = transfer(G, p2, p1, w_1); th = 5.991f.  G is the adjugate of
 *     H (no division by the determinant): g0 = h4*h8 - h5*h7, g1 = h2*h7 - h1*h8, g2 = h1*h5 - h2*h4,
 *     g3 = h5*h6 - h3*h8, g4 = h0*h8 - h2*h6, g5 = h2*h3 - h0*h5, g6 = h3*h7 - h4*h6, g7 = h1*h6 - h0*h7,
 *     g8 = h0*h4 - h1*h3.
 * A direction passes when chi2 < th (a NaN fails) and then adds (uint32)floor((5.991f - chi2) * 256.0f) to the
 * hypothesis's score; a match is an inlier when both directions pass.  Scores are integer sums (at most
 * 2 * 1534 * 16384).  The hypothesis of largest score wins, ties go to the smallest k; a largest score of 0 is "no
 * model".  No float is ever summed across matches or hypotheses, so no result depends on an order of execution.
 *
 * Outputs, per pair, all device: best (int32) = the winning k, or -1 for "no model" (n < m, D == 0, every hypothesis
 * invalid, or no score above 0); score, ninliers (uint32; 0 for "no model"); inlier uint8 [batch][stride], 0 or 1 for
 * i < n (all 0 for "no model"), entries at and beyond n are not written; model_n float [batch][9], the winner in
 * NORMALISED coordinates, row-major, last entry 1.0f (nine zeros for "no model"); stats int64 [batch][8] =
 * {n, Sx1, Sy1, D1, Sx2, Sy2, D2, 0}, always written.
 *
 * pislam_two_view_denormalise (host only, pure, no context): the level-0-PIXEL matrix in double from one row of
 * model_n and of stats, out = T2' * Fn * T1 (model 0) or inverse(T2) * Hn * T1 (model 1), with
 * T = [s 0 -Sx*k; 0 s -Sy*k; 0 0 1], k = 2 n n / D and s = 256 n k in double.  PISLAM_ERR_INVALID for a NULL pointer,
 * a model other than 0 / 1, n < 1 or a D < 1.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, batch and stride; the pointers are not looked at then).
 * Offsets use size_t arithmetic throughout.  No output may overlap an input or another output.  Any violation, or a
 * NULL or host pointer where a device pointer is required: PISLAM_ERR_INVALID, before anything is launched or
 * written.  `p` is a host struct, read during the call.  Asynchronous on the context stream; no workspace (the models
 * of a pair live in LDS), no host round trip: the call can be captured into a hipGraph as it is, so there is no
 * reserve call.  One workgroup works on a pair; a batch above 1024 pairs is walked by the same 1024 workgroups in
 * passes. */
typedef struct pislam_two_view_params {
  int32_t model;       /* 0 = fundamental matrix (m = 8), 1 = homography (m = 4) */
  int32_t hypotheses;  /* 1..1024, all of them are evaluated (ORB-SLAM: 200) */
  uint32_t seed;       /* any */
  int32_t sigma_q8;    /* measurement sigma in Q8 level-0 pixels, 1..4096 (ORB-SLAM: 256) */
} pislam_two_view_params;
int pislam_two_view_ransac_batch(pislam_ctx *ctx, const pislam_two_view_params *p, const int32_t *p1_q8,
                                 const int32_t *p2_q8, const uint32_t *counts, size_t stride, int batch, int32_t *best,
                                 uint32_t *score, uint32_t *ninliers, uint8_t *inlier, float *model_n, int64_t *stats);
int pislam_two_view_denormalise(int model, const float *model_n, const int64_t *stats_row, double out[9]);

/* ---- two-view reconstruction: relative pose and map points ---------------- */

/* From a verified two-view model to the first map: what ORB-SLAM's Initializer does in
 * ReconstructF / ReconstructH with CheckRT, per pair of a batch: every used match is triangulated under every candidate
 * motion, the good points are counted, one motion is chosen or the pair is refused, and the winner's points are handed
 * back.  With ONE candidate (a known relative pose) it is the triangulation of local mapping between two key frames.
 * pislam_two_view_decompose (below) makes the candidates from F or H on the host.  The reference ships nothing of the
 * kind: the semantics are this library's own, stated so that integers and individually rounded binary32 operations
 * reproduce every output word.  This comment is the contract.  "float(v)" is the conversion of an integer to binary32;
 * every +, -, *, / and sqrt below on floats is ONE binary32 operation rounded to nearest even, in the order the
 * parentheses give; no fused multiply-add, no reciprocal or fast approximation: the division and the square root are
 * the correctly rounded ones; denormals are kept.
 *
 * Inputs, all device unless said.  p1_q8, p2_q8 (int32 [batch][stride][2]) and counts (uint32 [batch]) are the buffers
 * of pislam_two_view_ransac_batch: n = min(counts[b], stride), PISLAM_COUNT_INVALID counts as 0, every coordinate is
 * clamped to [-2^20, 2^20] first.
 *   mask   uint8 [batch][stride] or NULL.  Match i is USED iff i < n and (mask == NULL or mask[b][i] != 0); the RANSAC
 *          call's `inlier` fits as it is.  N = the number of used matches.
 *   cam    float [batch][4]: fx, fy, cx, cy in level-0 pixels; both images share the one camera.
 *   cand   float [batch][ncand][12]: r0 .. r8 row-major, then t0 .. t2, with X2 = R X1 + t (the layout of the pose
 *          call's pose_in, so pose_out can feed it directly).
 *
 * Per pair:   ifx = 1.0f / fx,  ify = 1.0f / fy,  sg = float(sigma_q8) * (1.0f / 256.0f),  th2 = (sg*sg) * 4.0f.
 * Per used match, with (xq1, yq1) and (xq2, yq2) its clamped coordinates in the two images:
 *   u1 = float(xq1) * (1.0f / 256.0f), and likewise v1, u2, v2 (exact)
 *   x1 = (u1 - cx)*ifx,  y1 = (v1 - cy)*ify,  x2 = (u2 - cx)*ifx,  y2 = (v2 - cy)*ify
 *   bb = (x2*x2 + y2*y2) + 1.0f
 * Per candidate (the closest points of the two rays, their midpoint, its two reprojections):
 *   a0 = (r0*x1 + r1*y1) + r2,  a1 = (r3*x1 + r4*y1) + r5,  a2 = (r6*x1 + r7*y1) + r8              a = R (x1, y1, 1)
 *   n0 = a1 - a2*y2,  n1 = a2*x2 - a0,  n2 = a0*y2 - a1*x2;   nn = (n0*n0 + n1*n1) + n2*n2        a x b, b = (x2, y2, 1)
 *   p0 = y2*t2 - t1,  p1 = t0 - x2*t2,  p2 = x2*t1 - y2*t0                                         b x t
 *   q0 = a1*t2 - a2*t1,  q1 = a2*t0 - a0*t2,  q2 = a0*t1 - a1*t0                                   a x t
 *   z1 = ((p0*n0 + p1*n1) + p2*n2) / nn,   z2 = ((q0*n0 + q1*n1) + q2*n2) / nn
 *   g0 = z2*x2 - t0,  g1 = z2*y2 - t1,  g2 = z2 - t2;   h_j = (r_(0+j)*g0 + r_(3+j)*g1) + r_(6+j)*g2   (j = 0, 1, 2: R' g)
 *   X = ((z1*x1 + h0)*0.5f, (z1*y1 + h1)*0.5f, (z1 + h2)*0.5f)                                     the point, frame 1
 *   Y_k = ((r_(3k)*X0 + r_(3k+1)*X1) + r_(3k+2)*X2) + t_k                                          the point, frame 2
 *   cs = ((a0*x2 + a1*y2) + a2) / sqrt(((a0*a0 + a1*a1) + a2*a2) * bb)                             cosine of the rays
 *   i1 = 1.0f / X2;  eu = u1 - (fx*(X0*i1) + cx),  ev = v1 - (fy*(X1*i1) + cy),  e1 = eu*eu + ev*ev
 *   i2 = 1.0f / Y2;  eu = u2 - (fx*(Y0*i2) + cx),  ev = v2 - (fy*(Y1*i2) + cy),  e2 = eu*eu + ev*ev
 * (R = I, t = (-1, 0, 0), (x1, y1) = (0, 0), (x2, y2) = (-0.5, 0) gives z1 = z2 = 2 and X = (0, 0, 2).)
 * The match is GOOD under the candidate iff every component of X and Y is finite, and NOT ((X2 <= 0.0f or Y2 <= 0.0f)
 * and cs < cos_point) (as in CheckRT, a point at infinity stays whatever the sign of its depth), and e1 <= th2 and
 * e2 <= th2 (a NaN fails).  A good match HAS PARALLAX iff cs < cos_parallax and is a POINT iff cs < cos_point.  A
 * candidate with an entry that is not finite has no good match.
 *
 * Counts and choice, integers only (no float is summed across matches, so no result depends on an order of
 * execution).  G_c = the number of used matches that are good under candidate c, P_c = those of them with parallax.
 * gmax = max G_c, cbest = the smallest c with G_c = gmax, g2 = the largest G_c over c != cbest (0 for ncand = 1).
 * The code is that of the first row that holds:
 *   4   N == 0, or cam is not finite, or fx == 0, or fy == 0 (nothing is evaluated: every count is 0)
 *   1   gmax < min_good, or 100*gmax < min_good_pct*N
 *   2   100*g2 >= similar_pct*gmax     (at exact equality ORB-SLAM's F path, which asks for more than 0.7 gmax in
 *                                       floats, accepts; this contract rejects)
 *   3   P_cbest < min(parallax_rank, gmax)     (ORB-SLAM's "the parallax_rank-th smallest cosine is below the
 *                                               threshold", as a count: no sort, no acos)
 *   0   otherwise
 *
 * Outputs, per pair, always written, all device: status uint32 [batch] = code | cbest << 8; best int32 [batch] =
 * cbest for code 0, else -1; ngood, npar uint32 [batch][8] = G_c, P_c (0 for c >= ncand, all 0 for code 4); pose_out
 * float [batch][12] = the twelve words of cand[b][cbest] for code 0, else twelve zeros; for i < n, point[b][i] = 1 and
 * xw[b][i] = X under cbest iff the code is 0, match i is used and it is a point under cbest, otherwise 0 and three
 * zeros (point uint8 [batch][stride], xw float [batch][stride][3]); entries at and beyond n are not written.
 *
 * pislam_two_view_decompose (host only, pure, no context; stated to a tolerance, not bit for bit): the candidate motions
 * of a pixel matrix m_px (pislam_two_view_denormalise's output, row-major) under cam = fx, fy, cx, cy, with a 3 x 3
 * singular value decomposition in double (one-sided Jacobi, at most 60 sweeps).  Model 0: E = K' F K = U S V'; the SVD
 * takes the place of the rank-2 projection.  t = the third column of U, R1 = U W V', R2 = U W' V' with W = [0 -1 0;
 * 1 0 0; 0 0 1], each negated if its determinant is negative; *ncand = 4: (R1, t), (R2, t), (R1, -t), (R2, -t), ORB-
 * SLAM's order (*ncand = 0 when E has fewer than two singular values above 0).  Model 1: the eight Faugeras-Lustman solutions of A = inverse(K) H K = U diag(d1, d2, d3) V' as ORB-
 * SLAM's ReconstructH lists them, s = det(U) det(V): with x1 = e1*sqrt((d1^2 - d2^2) / (d1^2 - d3^2)), x3 = e3*sqrt((d2^2
 * - d3^2) / (d1^2 - d3^2)) over (e1, e3) = (+, +), (+, -), (-, +), (-, -) and the sign e = e1*e3 of the sine: first the
 * four of d' = +d2, sin = e*sqrt((d1^2 - d2^2)(d2^2 - d3^2)) / ((d1 + d3) d2), cos = (d2^2 + d1 d3) / ((d1 + d3) d2),
 * R = s U [cos 0 -sin; 0 1 0; sin 0 cos] V', t = U (x1, 0, -x3); then the four of d' = -d2, sin = e*sqrt((d1^2 - d2^2)
 * (d2^2 - d3^2)) / ((d1 - d3) d2), cos = (d1 d3 - d2^2) / ((d1 - d3) d2), R = s U [cos 0 sin; 0 -1 0; sin 0 -cos] V',
 * t = U (x1, 0, x3).  Every t is scaled to unit length.  *ncand = 8, or 0 with PISLAM_OK when the decomposition is
 * degenerate: d1/d2 < 1.00001 or d2/d3 < 1.00001 (a pure rotation, or a plane through a camera centre).  Each R is
 * checked in double before it is stored as floats: an entry of R'R - I or det R - 1 above 1e-12 also gives *ncand = 0.
 * PISLAM_ERR_INVALID: a NULL pointer, a model other than 0 / 1, an entry of m_px or cam that is not finite, fx == 0 or
 * fy == 0.  cand has room for 8 candidates; the rows from *ncand on are zeroed.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, batch and stride; the pointers are not looked at then).
 * Offsets use size_t arithmetic throughout.  No output may overlap an input or another output.  Any violation, or a
 * NULL or host pointer where a device pointer is required (mask alone may be NULL): PISLAM_ERR_INVALID, before
 * anything is launched or written.  `p` is a host struct, read during the call.  Asynchronous on the context stream;
 * no workspace, no host round trip: the call can be captured into a hipGraph as it is, so there is no reserve call.
 * One workgroup works on a pair; a batch above 1024 pairs is walked by the same 1024 workgroups in passes. */
typedef struct pislam_reconstruct_params {
  int32_t ncand;          /* 1..8 candidate motions per pair */
  int32_t sigma_q8;       /* 1..4096, Q8 level-0 pixels (ORB-SLAM: 256) */
  float cos_parallax;     /* in (0,1]; a match has parallax iff cs < this (cos 1 deg = 0.99984770f) */
  float cos_point;        /* in (0,1]; a match yields a map point iff cs < this (ORB-SLAM: 0.99998f) */
  int32_t min_good;       /* 1..16384 (ORB-SLAM: 50) */
  int32_t min_good_pct;   /* 0..100 of the used matches (ORB-SLAM: 90) */
  int32_t similar_pct;    /* 1..100: ambiguous iff 100*g2 >= similar_pct*gmax (ORB-SLAM: 70 for F, 75 for H) */
  int32_t parallax_rank;  /* 1..16384 (ORB-SLAM: 51, i.e. index 50 of the sorted cosines) */
} pislam_reconstruct_params;
int pislam_two_view_reconstruct_batch(pislam_ctx *ctx, const pislam_reconstruct_params *p, const int32_t *p1_q8,
                                      const int32_t *p2_q8, const uint32_t *counts, const uint8_t *mask,
                                      const float *cam, const float *cand, size_t stride, int batch, int32_t *best,
                                      uint32_t *status, uint32_t *ngood, uint32_t *npar, float *pose_out, float *xw,
                                      uint8_t *point);
int pislam_two_view_decompose(int model, const double m_px[9], const double cam[4], float *cand, int *ncand);

/* ---- motion-only pose optimisation from 3D-2D matches --------------------- */

/* The camera pose of a frame from map points matched to its keypoints: what ORB-SLAM's
 * Optimizer::PoseOptimization computes with g2o, per frame of a batch, with the inlier mask.  The reference ships
 * nothing of the kind: the semantics are this library's own, stated so that individually rounded binary32 and binary64
 * operations reproduce every output word.  This comment is the contract.  On floats every +, -, *, / and sqrt below is
 * ONE operation of the stated format, rounded to nearest even, in the order the parentheses give (a + b + c means
 * (a + b) + c); no fused multiply-add, no reciprocal or fast approximation: the division and the square root are the
 * correctly rounded ones; denormals are kept.  "float(v)" converts to binary32 (round to nearest even), "double(v)"
 * converts a binary32 to binary64 (exact).
 *
 * Inputs, all device unless said.  Frame b has n = min(counts[b], stride) observations (counts: uint32 [batch],
 * PISLAM_COUNT_INVALID counts as 0).
 *   pose_in     float [batch][12]: r0 .. r8 row-major, then t0 .. t2; Xc = R Xw + t.
 *   cam         float [batch][5]: fx, fy, cx, cy, bf in level-0 pixels (bf = baseline * fx).
 *   xw          float [batch][stride][3]: the map points (X, Y, Z).
 *   obs_q8      int32 [batch][stride][3]: (u, v, u_right) in Q8 level-0 pixels, each clamped to [-2^22, 2^22] first and
 *               then float(q) * (1.0f / 256.0f) (exact).  u_right == INT32_MIN (tested before the clamp) marks a
 *               MONOCULAR observation (2 residual rows), any other value a STEREO one (3 rows).
 *   level       uint8 [batch][stride] or NULL.  NULL: w = 1.0f for every observation.  Otherwise w =
 *               inv_sigma2[level]; an observation whose level is >= nlevels is DEAD at every pose (it lives in device
 *               memory, so the host cannot refuse it).
 *   inv_sigma2  HOST float [nlevels], 1 <= nlevels <= 16, every entry finite and > 0, read during the call; not looked
 *               at (and nlevels ignored) when level is NULL.
 *
 * One observation at a pose, binary32.  The pose is the binary64 state (below) rounded: r_k = float(R_k),
 * t_k = float(t_k).
 *   x = ((r0*X + r1*Y) + r2*Z) + t0,  y = ((r3*X + r4*Y) + r5*Z) + t1,  z = ((r6*X + r7*Y) + r8*Z) + t2
 *   the observation is DEAD unless z >= 2^-10 (a NaN fails)
 *   iz = 1.0f / z,  px = x*iz,  py = y*iz,  pu = fx*px + cx,  pv = fy*py + cy
 *   eu = u - pu,  ev = v - pv;  stereo only: er = ur - (pu - bf*iz)
 *   chi2 = (eu*eu + ev*ev) * w        (monocular)         chi2 = ((eu*eu + ev*ev) + er*er) * w      (stereo)
 *   the observation is DEAD as well unless chi2 is finite (neither infinite nor a NaN)
 *   th = 5.991f (monocular), 7.815f (stereo)
 *   Huber with delta^2 = th, as in ORB-SLAM: if the pass is robust and chi2 > th:
 *       k = sqrt(th / chi2),  wr = w*k,  rho = (chi2*k)*2.0f - th;     otherwise wr = w, rho = chi2.
 * A dead observation contributes nothing and is an outlier.  Jacobian rows of the error for a left increment
 * d = (omega, upsilon), with a = fx*iz, b = fy*iz, c = bf*iz, pxy = px*py:
 *   Ju = [ pxy*fx, -((1.0f + px*px)*fx), py*fx, -a, 0.0f, px*a ]
 *   Jv = [ (1.0f + py*py)*fy, -(pxy*fy), -(px*fy), 0.0f, -b, py*b ]
 *   Jr = [ Ju0 - c*py, Ju1 + c*px, Ju2, Ju3, 0.0f, Ju5 - c*iz ]
 * The observation's 28 terms, in this order: for j = 0 .. 5, for k = j .. 5 (21 terms, the upper triangle row by row)
 *   H_jk = (Ju_j*Ju_k + Jv_j*Jv_k) * wr   or   ((Ju_j*Ju_k + Jv_j*Jv_k) + Jr_j*Jr_k) * wr   (stereo);
 * for j = 0 .. 5:  g_j = (Ju_j*eu + Jv_j*ev) * wr   or   ((Ju_j*eu + Jv_j*ev) + Jr_j*er) * wr;   then rho.
 * The products with the constant 0.0f entries are carried out like any other.
 *
 * A PASS evaluates every observation of the frame at one pose and sums, in binary64, the 28 terms of those that are
 * ACTIVE and not dead, and with them the number 1.0 and double(chi2) (the plain chi2) of each of these: 30 sums S_0 ..
 * S_29; S = (H, g, F = S_27, S_28, S_29).  The order is fixed and does not depend on the launch: 256 partial sums that
 * start at +0.0; partial i mod 256 takes double(term) of observation i, in ascending i; then the partials are combined
 * by halving: p[j] = p[j] + p[j + 128] for j < 128, then with 64, 32, 16, 8, 4, 2, 1; S is p[0].  (IEEE addition is
 * commutative, so an exchange between j and j xor h, in which both partners add, gives every lane the same bits as the
 * halving gives p[j mod h]: the kernel uses that.  Adding the +0.0 of an inactive or dead observation changes no
 * partial.)  No other float is ever summed across observations.  A CLASSIFYING pass first sets the active set anew from
 * EVERY observation: active iff not dead and chi2 <= th at the pass's pose (so an outlier can come back, as in
 * ORB-SLAM); it then sums over that new set.
 *
 * Per frame, binary64.  The state T = (R, t) is double(pose_in) and stays in binary64 for the whole call.
 *   Solve(S, lambda): A = the symmetric 6 x 6 matrix of the H sums, A_jj = H_jj * (1.0 + lambda), rhs_j = -g_j.
 *     Gaussian elimination WITHOUT pivoting, for c = 0 .. 5: the solve fails unless A[c][c] > 0 (a NaN fails); for
 *     r = c+1 .. 5: f = A[r][c] / A[c][c]; for j = c+1 .. 5: A[r][j] = A[r][j] - f*A[c][j]; rhs_r = rhs_r - f*rhs_c.
 *     Back substitution, r = 5 .. 0: s = rhs_r; for j = r+1 .. 5 ascending: s = s - A[r][j]*d_j;  d_r = s / A[r][r].
 *     The solve also fails when a d_r is not finite.
 *   Retract(T, d), the Cayley map (no sine or cosine): a = (d_0*0.5, d_1*0.5, d_2*0.5), n = (a0*a0 + a1*a1) + a2*a2,
 *     m = 1.0 - n, e = 1.0 + n, Q = ((1 - n) I + 2 a a' + 2 [a]x) / (1 + n) entry by entry:
 *       Q00 = (m + 2.0*(a0*a0))/e       Q01 = (2.0*(a0*a1) - 2.0*a2)/e   Q02 = (2.0*(a0*a2) + 2.0*a1)/e
 *       Q10 = (2.0*(a1*a0) + 2.0*a2)/e  Q11 = (m + 2.0*(a1*a1))/e        Q12 = (2.0*(a1*a2) - 2.0*a0)/e
 *       Q20 = (2.0*(a2*a0) - 2.0*a1)/e  Q21 = (2.0*(a2*a1) + 2.0*a0)/e   Q22 = (m + 2.0*(a2*a2))/e
 *     R'_ij = (Q_i0*R_0j + Q_i1*R_1j) + Q_i2*R_2j,   t'_i = ((Q_i0*t_0 + Q_i1*t_1) + Q_i2*t_2) + d_(3+i).
 *   A ROUND (Levenberg) starts from S at T over the current active set, lambda = 2^-10, and repeats up to `iters`
 *   times:  1. d = Solve(S, lambda);  2. on failure lambda = min(8.0*lambda, 2^20) and the iteration is spent;
 *   3. otherwise T' = Retract(T, d) and S' = a pass at T' (same active set, same robust flag);  4. if F' < F (false
 *   for a NaN): T = T', S = S', lambda = max(lambda*0.25, 2^-30), else lambda = min(8.0*lambda, 2^20);  5. either way
 *   the round ends when max_j |d_j| <= eps.  One pass per iteration.
 *   The call:  pose_in or cam not finite: code 2.  n < min_obs: code 1.  Otherwise every observation is active and a
 *   pass at T gives round 0 its S; the passes of round r are robust iff r < huber_rounds.  After round r a CLASSIFYING
 *   pass at T, robust iff r + 1 < huber_rounds, gives the inlier mask (= the new active set), ninliers = S_28 and
 *   cost = S_29, and its S is the start of round r + 1, which runs unless r + 1 == rounds (code 0) or ninliers <
 *   min_obs (code 1).  Unlike ORB-SLAM, a round continues from the pose the round before reached; it does not restart
 *   from the initial pose.
 *
 * Outputs, per frame, always written, all device.  pose_out float [batch][12] = float(T) (pose_in itself for code 2
 * and for a frame that never ran a round); it may be exactly pose_in.  inlier uint8 [batch][stride]: the last
 * classification, 0 or 1 for i < n (all 0 for a frame that never ran a round); entries at and beyond n are not written.
 * ninliers uint32 [batch].  cost double [batch]: the tree-ordered sum of the inliers' plain chi2 (0 without a round).
 * status uint32 [batch] = code | evaluations << 8, evaluations = the number of passes made; code 0: all rounds ran;
 * 1: stopped for min_obs, the pose is that of the last completed round, or pose_in; 2: pose_in or cam not finite.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, the table, batch and stride; the pointers are not looked
 * at then).  Offsets use size_t arithmetic throughout.  No output may overlap an input or another output, except that
 * pose_out may be pose_in.  Any violation, or a NULL or host pointer where a device pointer is required:
 * PISLAM_ERR_INVALID, before anything is launched or written.  `p` is a host struct, read during the call.
 * Asynchronous on the context stream; no workspace, no host round trip: the call can be captured into a hipGraph as it
 * is.  One workgroup runs a frame's whole call in one launch; a batch above 1024 frames is walked by the same 1024
 * workgroups in passes. */
typedef struct pislam_pose_params {
  int32_t rounds;        /* 1..8 (ORB-SLAM: 4) */
  int32_t iters;         /* 1..32 Levenberg iterations per round (ORB-SLAM: 10) */
  int32_t huber_rounds;  /* 0..rounds: rounds 0 .. huber_rounds - 1 are robust (ORB-SLAM: 3) */
  int32_t min_obs;       /* 3..16384 active observations needed to run a round (ORB-SLAM: 10) */
  double eps;            /* >= 0: a round ends when no |d_j| exceeds it (1e-6) */
} pislam_pose_params;
int pislam_pose_refine_batch(pislam_ctx *ctx, const pislam_pose_params *p, const float *pose_in, const float *cam,
                             const float *xw, const int32_t *obs_q8, const uint32_t *counts, const uint8_t *level,
                             const float *inv_sigma2, int nlevels, size_t stride, int batch, float *pose_out,
                             uint8_t *inlier, uint32_t *ninliers, double *cost, uint32_t *status);

/* ---- absolute pose from 3D-2D matches: P3P RANSAC ------------------------- */

/* A pose from nothing: what ORB-SLAM's relocalisation and loop closing do with their PnP
 * solver, per frame of a batch: minimal samples of three 3D-2D matches are solved for the camera pose (P3P in the
 * Lambda Twist formulation, Persson & Nordberg, ECCV 2018: nothing beyond + - * / and the square root), a fourth match
 * chooses among the solutions, every hypothesis is scored against every observation with the pose call's monocular
 * chi2, and the best one is handed back with its inlier mask.  The inputs are the pose call's buffers and pose_out is
 * its pose_in, so pislam_pose_refine_batch is the refit.  The reference ships nothing of the kind: the semantics are
 * this library's own, stated so that integers and individually rounded binary32 operations reproduce every output
 * word.  This comment is the contract.  Every +, -, *, / and sqrt below is ONE binary32 operation rounded to nearest
 * even, in the order the parentheses give (a + b + c means (a + b) + c, -a - b means (-a) - b); no fused multiply-add,
 * no reciprocal or fast approximation: the division and the square root are the correctly rounded ones; denormals are
 * kept.  A comparison with a NaN is false.
 *
 * Inputs: cam, xw, obs_q8, counts, level, inv_sigma2, nlevels exactly as in pislam_pose_refine_batch (same layouts,
 * same rules for level / inv_sigma2 / nlevels).  cam = (fx, fy, cx, cy, bf); bf is read for the finiteness test only.
 * (u, v) = (float(clamp(q, -2^22, 2^22)) * (1.0f/256.0f)) of the first two words of an observation; the third word is
 * ignored: every observation is monocular here.  n = min(counts[b], stride), PISLAM_COUNT_INVALID counts as 0.
 * w = 1.0f without a level table, else inv_sigma2[level]; an observation whose level is >= nlevels is DEAD under every
 * pose (as a sample of draws 0 .. 2 it is still used: only its point and pixel are read there).
 * ifx = 1.0f / fx, ify = 1.0f / fy.
 *
 * One observation under one pose T = (r0 .. r8 row-major, t0 .. t2), the pose call's monocular arithmetic:
 *   x = ((r0*X + r1*Y) + r2*Z) + t0,  y = ((r3*X + r4*Y) + r5*Z) + t1,  z = ((r6*X + r7*Y) + r8*Z) + t2
 *   dead unless z >= 2^-10;  iz = 1.0f / z,  pu = fx*(x*iz) + cx,  pv = fy*(y*iz) + cy,  eu = u - pu,  ev = v - pv
 *   chi2 = (eu*eu + ev*ev) * w;  dead unless chi2 is finite.
 * A live observation with chi2 < 5.991f is an INLIER and adds (uint32)floor((5.991f - chi2) * 256.0f) to the
 * hypothesis's integer score (at most 1533 * 16384).
 *
 * Sampling: the sampler of pislam_two_view_ransac_batch with m = 4, the same hash(seed; b, k, j) and draw order.  Draws
 * 0, 1, 2 are the minimal problem (points x1, x2, x3 with pixels (u_i, v_i)), draw 3 chooses among its solutions.
 * n < 4: no model.
 *
 * The solver.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2;  cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
 *  1. Bearings: xn = (u - cx) * ifx,  yn = (v - cy) * ify,  r = 1.0f / sqrt((xn*xn + yn*yn) + 1.0f),
 *     y_i = (xn*r, yn*r, r).
 *  2. b12 = -2.0f * dot(y1, y2),  b13 = -2.0f * dot(y1, y3),  b23 = -2.0f * dot(y2, y3);
 *     d12 = x1 - x2,  d13 = x1 - x3,  d23 = x2 - x3 (by component);  a_ij = dot(d_ij, d_ij);
 *     c12 = -0.5f * b12,  c23 = -0.5f * b23,  c31 = -0.5f * b13;  s12 = 1.0f - c12*c12,  s23, s31 alike;
 *     blob = (c12*c23)*c31 - 1.0f.
 *  3. p3 = a13 * (a23*s31 - a13*s23)
 *     p2 = (((2.0f*blob)*a23)*a13 + (a13*(2.0f*a12 + a13))*s23) + (a23*(a23 - a12))*s31
 *     p1 = ((a23*(a13 - a23))*s12 - (a12*a12)*s23) - (2.0f*a12)*(blob*a23 + a13*s23)
 *     p0 = a12 * (a12*s23 - a23*s12)
 *     p3 == 0: the hypothesis is invalid.  ip = 1.0f / p3;  B = p2*ip,  C = p1*ip,  D = p0*ip.
 *  4. One real root g of r^3 + B r^2 + C r + D.  h(t) = ((t + B)*t + C)*t + D,  h'(t) = (3.0f*t + 2.0f*B)*t + C.
 *     If B*B >= 3.0f*C:  v = sqrt(B*B - 3.0f*C),  t1 = (-B - v) / 3.0f,  k = h(t1);
 *       if k > 0: r = t1 - sqrt(-k / (3.0f*t1 + B));
 *       else t2 = (-B + v) / 3.0f,  k = h(t2),  r = t2 + sqrt(-k / (3.0f*t2 + B)).
 *     Otherwise r = -B / 3.0f, and if |h'(r)| < 1e-4f then r = r + 1.0f.
 *     Then 12 Newton steps, all of them taken: f = h(r), f' = h'(r), if f' != 0: r = r - f / f'.  g = r.
 *  5. A00 = a23*(1.0f - g),  A01 = (a23*b12)*0.5f,  A02 = ((a23*b13)*g)*(-0.5f),  A11 = (a23 - a12) + a13*g,
 *     A12 = (b23*(a13*g - a12))*0.5f,  A22 = g*(a13 - a23) - a12.  One eigenvalue of this symmetric matrix is 0; the
 *     other two are the roots of e^2 + eb e + ec:  x01 = A01*A01,  eb = (-A00 - A11) - A22,
 *     ec = (((-x01 - A02*A02) - A12*A12) + A00*(A11 + A22)) + A11*A22,  disc = eb*eb - 4.0f*ec, 0 unless disc > 0,
 *     L0 = ((eb < 0 ? -eb + sqrt(disc) : -eb - sqrt(disc))) * 0.5f (the larger magnitude),  L1 = ec / L0.
 *     Eigenvector of e (for L0: V0 = (V00, V10, V20); for L1: V1 = (V01, V11, V21)), with
 *     prec0 = A01*A12 - A02*A11,  prec1 = A01*A02 - A00*A12:
 *       tmp = 1.0f / (((e*(A00 + A11) - A00*A11) - e*e) + x01),  a1 = -((e*A02 + prec0)*tmp),
 *       a2 = -((e*A12 + prec1)*tmp),  rn = 1.0f / sqrt((a1*a1 + a2*a2) + 1.0f),  vector = (a1*rn, a2*rn, rn).
 *  6. q = -L1 / L0,  v = sqrt(q) if q > 0, else 0.  For s = +v, then s = -v:
 *       w2 = 1.0f / (s*V01 - V00),  w0 = (V10 - s*V11)*w2,  w1 = (V20 - s*V21)*w2
 *       qa = 1.0f / ((((a13 - a12)*w1)*w1 - (a12*b13)*w1) - a12)
 *       qb = (((a13*b12)*w1 - (a12*b13)*w0) - ((2.0f*w0)*w1)*(a12 - a13)) * qa
 *       qc = ((((a13 - a12)*w0)*w0 + (a13*b12)*w0) + a13) * qa
 *       disc = qb*qb - 4.0f*qc; nothing unless disc >= 0;  tau = (-qb + sqrt(disc))*0.5f, then (-qb - sqrt(disc))*0.5f.
 *     That is up to four candidates, numbered in this order.  A candidate exists when tau > 0,
 *     d = a23 / (tau*(b23 + tau) + 1.0f) > 0, and with l2 = sqrt(d), l3 = tau*l2, l1 = w0*l2 + w1*l3: l1 >= 0.
 *  7. 5 Gauss-Newton steps on (l1, l2, l3), all of them taken:
 *       r1 = ((l1*l1 + l2*l2) + (b12*l1)*l2) - a12,  r2 = ((l1*l1 + l3*l3) + (b13*l1)*l3) - a13,
 *       r3 = ((l2*l2 + l3*l3) + (b23*l2)*l3) - a23
 *       v0 = 2.0f*l1 + b12*l2,  v1 = 2.0f*l2 + b12*l1,  v3 = 2.0f*l1 + b13*l3,  v5 = 2.0f*l3 + b13*l1,
 *       v7 = 2.0f*l2 + b23*l3,  v8 = 2.0f*l3 + b23*l2,  idet = 1.0f / (-((v0*v5)*v7) - (v1*v3)*v8)
 *       n1 = ((v1*v5)*r3 - (v5*v7)*r1) - (v1*v8)*r2,  n2 = ((v0*v8)*r2 - (v3*v8)*r1) - (v0*v5)*r3,
 *       n3 = ((v3*v7)*r1 - (v0*v7)*r2) - (v1*v3)*r3;   l_i = l_i - n_i*idet  (all three from the old values).
 *  8. The inverse Xi of X = [d12, d13, nx = cross(d12, d13)] (columns; m_rc = entry of row r, column c) by cofactors:
 *       i00 = m11*m22 - m12*m21,  i01 = m02*m21 - m01*m22,  i02 = m01*m12 - m02*m11,
 *       i10 = m12*m20 - m10*m22,  i11 = m00*m22 - m02*m20,  i12 = m02*m10 - m00*m12,
 *       i20 = m10*m21 - m11*m20,  i21 = m01*m20 - m00*m21,  i22 = m00*m11 - m01*m10,
 *       idet = 1.0f / ((m00*i00 + m01*i10) + m02*i20),  Xi_rc = i_rc * idet.
 *     ry1 = l1*y1,  e1 = ry1 - l2*y2,  e2 = ry1 - l3*y3 (by component),  e3 = cross(e1, e2);
 *     R_ij = (e1_i*Xi_0j + e2_i*Xi_1j) + e3_i*Xi_2j,   t_i = ry1_i - ((R_i0*x1_0 + R_i1*x1_1) + R_i2*x1_2).
 *  9. A candidate with a pose entry that is not finite, or under whose pose draw 3 is dead, is dropped.  Of the others
 *     the one with the smallest chi2 of draw 3 is the hypothesis's pose (strict <: the lower number wins a tie).  The
 *     hypothesis is invalid when there is none.  (Collinear x1, x2, x3 end here: nx = 0 makes Xi not finite.)
 *
 * The best: the valid hypothesis of largest score wins, ties go to the smallest k; a largest score of 0 is "no model".
 * No float is ever summed across observations or hypotheses, so no result depends on an order of execution.
 *
 * Outputs, per frame, always written, all device.  best (int32) = the winning k, or -1.  score, ninliers (uint32; 0
 * without a model).  inlier uint8 [batch][stride]: 0 or 1 for i < n under the winning pose (all 0 without a model);
 * entries at and beyond n are not written.  pose_out float [batch][12] = the winner's (R row-major, t): the layout of
 * the pose call's pose_in; twelve zeros without a model.  status uint32 = code | valid_hypotheses << 8 (the number of
 * valid hypotheses among those evaluated; 0 when nothing is evaluated).  code 0: ok;  1: a model, but ninliers <
 * min_inliers (pose and mask are written all the same);  2: no model (n < 4, every hypothesis invalid, or no score
 * above 0);  3: cam not finite, fx == 0 or fy == 0: nothing is evaluated.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, the table, batch and stride; the pointers are not looked
 * at then).  Offsets use size_t arithmetic throughout.  No output may overlap an input or another output.  Any
 * violation, or a NULL or host pointer where a device pointer is required: PISLAM_ERR_INVALID, before anything is
 * launched or written.  `p` is a host struct, read during the call.  Asynchronous on the context stream; no workspace
 * (the poses of a frame's hypotheses live in LDS), no host round trip: the call can be captured into a hipGraph as it
 * is, so there is no reserve call.  One workgroup works on a frame; a batch above 1024 frames is walked by the same
 * 1024 workgroups in passes. */
typedef struct pislam_pnp_params {
  int32_t hypotheses;   /* 1..1024, all of them are evaluated */
  uint32_t seed;        /* any */
  int32_t min_inliers;  /* 4..16384 (ORB-SLAM: 10) */
} pislam_pnp_params;
int pislam_pnp_ransac_batch(pislam_ctx *ctx, const pislam_pnp_params *p, const float *cam, const float *xw,
                            const int32_t *obs_q8, const uint32_t *counts, const uint8_t *level,
                            const float *inv_sigma2, int nlevels, size_t stride, int batch, int32_t *best,
                            uint32_t *score, uint32_t *ninliers, uint8_t *inlier, float *pose_out, uint32_t *status);

/* ---- similarity from 3D-3D matches: Sim(3) RANSAC (Horn) ------------------ */

/* The loop-closing step: what ORB-SLAM's LoopClosing::ComputeSim3 asks of its Sim3Solver, per
 * (key frame, loop candidate) pair of a batch.  A monocular map drifts in scale, so the two key frames are related by a
 * similarity X1 = s R X2 + t, not by a rigid pose.  Minimal samples of three matched map points, each given in both
 * camera frames, are solved in closed form (Horn 1987, "Closed-form solution of absolute orientation using unit
 * quaternions"), every hypothesis is scored against every match by reprojection into BOTH images with the pose call's
 * monocular chi2, and the best one is handed back with its inlier mask.  The reference ships nothing of the kind: the
 * semantics are this library's own, stated so that integers and individually rounded binary32 operations reproduce
 * every output word.  This comment is the contract.  Every +, -, *, / and sqrt below is ONE binary32 operation rounded
 * to nearest even, in the order the parentheses give (a + b + c means (a + b) + c); no fused multiply-add, no
 * reciprocal or fast approximation: the division and the square root are the correctly rounded ones; denormals are
 * kept.  A comparison with a NaN is false.  Nothing but those five operations is used: no atan2, sin or cos (ORB-SLAM's
 * detour through the angle-axis form of the quaternion is not taken).
 *
 * Inputs, device unless said.  n = min(counts[b], stride), PISLAM_COUNT_INVALID counts as 0.  cam1, cam2 float
 * [batch][5] = (fx, fy, cx, cy, bf) as in pislam_pose_refine_batch; bf is read for the finiteness test only.  x1, x2
 * float [batch][stride][3]: match i's map point in camera 1's frame and in camera 2's frame.  obs1_q8, obs2_q8 int32
 * [batch][stride][3], the pose call's observation layout: (u, v) = (float(clamp(q, -2^22, 2^22)) * (1.0f/256.0f)) of
 * the first two words, the third word is ignored.  (ORB-SLAM compares with the points' own projections: a caller who
 * wants exactly that passes those.)  level1, level2 uint8 [batch][stride], both given or both NULL; with them
 * inv_sigma2 (HOST, nlevels entries) follows the pose call's rules, w1 = inv_sigma2[level1], w2 = inv_sigma2[level2],
 * and a match with a level >= nlevels on either side is DEAD under every hypothesis (as a sample it is still used:
 * only its points are read there); without them w1 = w2 = 1.0f.
 *
 * Sampling: the sampler of pislam_two_view_ransac_batch with m = 3, the same hash(seed; b, k, j) and draw order.
 * n < 3: no model.
 *
 * The solver, on the draws j = 0, 1, 2 with points P1_j (of x1) and P2_j (of x2).
 * dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
 *  1. Centroids, by component: O1 = ((P1_0 + P1_1) + P1_2) / 3.0f, O2 alike;  p1_j = P1_j - O1,  p2_j = P2_j - O2.
 *  2. M_ab = (p2_0[a]*p1_0[b] + p2_1[a]*p1_1[b]) + p2_2[a]*p1_2[b]   (a, b = 0 .. 2: the sum of p2 p1').
 *  3. The symmetric 4 x 4 matrix N:
 *       N00 = (M00 + M11) + M22,  N11 = (M00 - M11) - M22,  N22 = (M11 - M00) - M22,  N33 = (M22 - M00) - M11,
 *       N01 = M12 - M21,  N02 = M20 - M02,  N03 = M01 - M10,  N12 = M01 + M10,  N13 = M20 + M02,  N23 = M12 + M21,
 *     each stored at both places.  V = the 4 x 4 identity.
 *  4. Cyclic Jacobi: 4 sweeps, all of them taken (no convergence test); a sweep visits the pivots (p, q) = (0,1), (0,2),
 *     (0,3), (1,2), (1,3), (2,3) in this order.  A pivot with N_pq == 0 is skipped.  Otherwise
 *       th = (N_qq - N_pp) / (2.0f * N_pq),  tt = (th >= 0 ? 1.0f : -1.0f) / (|th| + sqrt(th*th + 1.0f)),
 *       c = 1.0f / sqrt(tt*tt + 1.0f),  sn = tt * c;
 *     then for k = 0 .. 3 (columns):  (N_kp, N_kq) = (c*N_kp - sn*N_kq,  sn*N_kp + c*N_kq)   (both from the old pair);
 *     then for k = 0 .. 3 (rows):     (N_pk, N_qk) = (c*N_pk - sn*N_qk,  sn*N_pk + c*N_qk);
 *     then for k = 0 .. 3 (vectors):  (V_kp, V_kq) = (c*V_kp - sn*V_kq,  sn*V_kp + c*V_kq).
 *     (All 16 entries of N are carried; the two triangles may differ in the last bit.  th*th overflows to infinity for
 *     a tiny pivot: tt = 0, the identity rotation, which is harmless and not branched round.)
 *  5. The quaternion is the column j of V with the largest N_jj after the last sweep (strict >: the lowest j wins a
 *     tie):  rn = 1.0f / sqrt(((V_0j*V_0j + V_1j*V_1j) + V_2j*V_2j) + V_3j*V_3j),  (w, x, y, z) = (V_0j*rn, .. V_3j*rn).
 *  6. R, entry by entry from the products ww = w*w, xx, yy, zz, xy, xz, yz, wx, wy, wz:
 *       R00 = ((ww + xx) - yy) - zz,  R01 = 2.0f*(xy - wz),         R02 = 2.0f*(xz + wy),
 *       R10 = 2.0f*(xy + wz),         R11 = ((ww - xx) + yy) - zz,  R12 = 2.0f*(yz - wx),
 *       R20 = 2.0f*(xz - wy),         R21 = 2.0f*(yz + wx),         R22 = ((ww - xx) - yy) + zz.
 *  7. Scale.  fixed_scale: s = 1.0f.  Otherwise (ORB-SLAM's asymmetric form) with g_j = R p2_j, that is
 *     g_j[i] = (Ri0*p2_j[0] + Ri1*p2_j[1]) + Ri2*p2_j[2]:
 *       s = ((dot(p1_0, g_0) + dot(p1_1, g_1)) + dot(p1_2, g_2)) / ((dot(p2_0, p2_0) + dot(p2_1, p2_1)) + dot(p2_2, p2_2)).
 *  8. t_i = O1_i - s * ((Ri0*O2_0 + Ri1*O2_1) + Ri2*O2_2);   is = 1.0f / s.
 *  9. The hypothesis is invalid when any of the 13 words R, t, s is not finite, or when s > 0 does not hold.
 *
 * Scoring, ORB-SLAM's CheckInliers: every match under every valid hypothesis, in the stored form (R, t, s, is).
 *   forward:   a_i = s * ((Ri0*X2_0 + Ri1*X2_1) + Ri2*X2_2) + t_i,       projected with cam1 against (u1, v1), w1;
 *   backward:  d = X1 - t,  b_i = ((R0i*d_0 + R1i*d_1) + R2i*d_2) * is,  projected with cam2 against (u2, v2), w2.
 * A side with the camera point (x, y, z), the pose call's monocular arithmetic:
 *   dead unless z >= 2^-10;  iz = 1.0f / z,  pu = fx*(x*iz) + cx,  pv = fy*(y*iz) + cy,  eu = u - pu,  ev = v - pv,
 *   chi2 = (eu*eu + ev*ev) * w;  dead unless chi2 is finite.
 * A match is an INLIER when both sides are live and chi2_1 < 9.210f and chi2_2 < 9.210f; it then adds
 * (uint32)floor((9.210f - chi2_1) * 256.0f) + (uint32)floor((9.210f - chi2_2) * 256.0f) to the hypothesis's integer
 * score (at most 2 * 2358 * 16384 < 2^27).
 *
 * The best: the valid hypothesis of largest score wins, ties go to the smallest k; a largest score of 0 is "no model".
 * No float is ever summed across matches or hypotheses, so no result depends on an order of execution or on the
 * launch shape.
 *
 * Outputs, per pair, always written, all device.  best (int32) = the winning k, or -1.  score, ninliers (uint32; 0
 * without a model).  inlier uint8 [batch][stride]: 0 or 1 for i < n under the winner (all 0 without a model); entries
 * at and beyond n are not written.  sim_out float [batch][13] = the winner's (R row-major, t, s); the first twelve
 * words are the layout of the pose call's pose_in, so a fixed-scale result feeds pislam_pose_refine_batch directly;
 * thirteen zeros without a model.  status uint32 = code | valid_hypotheses << 8 (the number of valid hypotheses among
 * those evaluated; 0 when nothing is evaluated).  code 0: ok;  1: a model, but ninliers < min_inliers (similarity and
 * mask are written all the same);  2: no model (n < 3, every hypothesis invalid, or no score above 0);  3: cam1 or cam2
 * not finite, or an fx or fy == 0: nothing is evaluated.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, the levels, the table, batch and stride; the other
 * pointers are not looked at then).  Offsets use size_t arithmetic throughout.  No output may overlap an input or
 * another output.  Any violation, one level pointer without the other, or a NULL or host pointer where a device
 * pointer is required: PISLAM_ERR_INVALID, before anything is launched or written.  `p` is a host struct, read during
 * the call.  Asynchronous on the context stream; no workspace (a pair's hypotheses live in LDS), no host round trip:
 * the call can be captured into a hipGraph as it is, so there is no reserve call.  One workgroup works on a pair; a
 * batch above 1024 pairs is walked by the same 1024 workgroups in passes.
 *
 * Not here: SearchBySim3, which pislam_match_hamming_scaled_window_batch with predicted centres covers, given this
 * call's output.  ORB-SLAM's 7-degree-of-freedom refinement of the result is pislam_sim3_refine_batch, below. */
typedef struct pislam_sim3_params {
  int32_t hypotheses;   /* 1..1024, all of them are evaluated (ORB-SLAM: up to 300) */
  uint32_t seed;        /* any */
  int32_t min_inliers;  /* 3..16384 (ORB-SLAM: 20) */
  int32_t fixed_scale;  /* 0 / 1: 1 forces s = 1.0f (stereo / RGB-D maps) */
} pislam_sim3_params;
int pislam_sim3_ransac_batch(pislam_ctx *ctx, const pislam_sim3_params *p, const float *cam1, const float *cam2,
                             const float *x1, const float *x2, const int32_t *obs1_q8, const int32_t *obs2_q8,
                             const uint32_t *counts, const uint8_t *level1, const uint8_t *level2,
                             const float *inv_sigma2, int nlevels, size_t stride, int batch, int32_t *best,
                             uint32_t *score, uint32_t *ninliers, uint8_t *inlier, float *sim_out, uint32_t *status);

/* ---- similarity refinement after the RANSAC: OptimizeSim3 ----------------- */

/* The last step of the loop-closing chain: what ORB-SLAM's Optimizer::OptimizeSim3 computes
 * with g2o, per (key frame, loop candidate) pair of a batch.  The similarity X1 = s R X2 + t that the RANSAC call found
 * on three points is refined over all its matches (or over those of a guided re-match) by minimising the robust
 * reprojection error in BOTH images; the map points stay fixed, as in ORB-SLAM.  LoopClosing::ComputeSim3 accepts a loop
 * on the number of inliers AFTER this step: that is `ninliers`.  The call is pislam_pose_refine_batch's procedure on a
 * 7-dimensional increment, and wherever this comment says "the pose call's" the words of that comment hold unchanged.
 * The reference ships nothing of the kind: the semantics are this library's own, stated so that individually rounded
 * binary32 and binary64 operations reproduce every output word.  This comment is the contract.  On floats every +, -, *,
 * / and sqrt below is ONE operation of the stated format, rounded to nearest even, in the order the parentheses give
 * (a + b + c means (a + b) + c); no fused multiply-add, no reciprocal or fast approximation; denormals are kept; no
 * transcendental function is used.  "float(v)" converts to binary32 (round to nearest even), "double(v)" converts a
 * binary32 to binary64 (exact).  A comparison with a NaN is false.
 *
 * Inputs, device unless said.  cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2, inv_sigma2 (HOST),
 * nlevels, stride, batch: pislam_sim3_ransac_batch's own buffers, read by its rules (n = min(counts[b], stride),
 * PISLAM_COUNT_INVALID counts as 0; (u, v) from the first two Q8 words; w1, w2 from the levels or 1.0f; a match with a
 * level >= nlevels on either side is DEAD under every similarity).
 *   sim_in  float [batch][13] = (R row-major, t, s): the RANSAC call's sim_out layout.
 *   mask    uint8 [batch][stride] or NULL.  A 0 makes match i DEAD under every similarity; any other value, or NULL,
 *           leaves it alone.  The RANSAC call's `inlier`, or the validity of a re-match, goes straight in.  Entries at
 *           and beyond n are not read.
 *
 * One match under one similarity, binary32.  The similarity of a pass is the binary64 state (below) rounded word by
 * word, R_ij = float(R_ij), t_i = float(t_i), s = float(s), and is = 1.0f / s.  With P = X1 and X = X2 of the match:
 *   forward:   a_i = s * ((Ri0*X_0 + Ri1*X_1) + Ri2*X_2) + t_i,          projected with cam1 against (u1, v1), w1;
 *   backward:  d = P - t,  b_i = ((R0i*d_0 + R1i*d_1) + R2i*d_2) * is,   projected with cam2 against (u2, v2), w2
 * (the RANSAC call's scoring arithmetic, to the letter).  A side with the camera point (x, y, z), the weight w and the
 * camera (fx, fy, cx, cy):
 *   dead unless z >= 2^-10;  iz = 1.0f / z,  px = x*iz,  py = y*iz,  pu = fx*px + cx,  pv = fy*py + cy,
 *   eu = u - pu,  ev = v - pv,  chi2 = (eu*eu + ev*ev) * w;  dead unless chi2 is finite.
 * A match is DEAD unless both sides are live; a dead match contributes nothing and is an outlier.  Each side carries
 * its own Huber weight with delta^2 = th2, the pose call's formula: if the pass is robust and chi2 > th2:
 *   k = sqrt(th2 / chi2),  wr = w*k,  rho = (chi2*k)*2.0f - th2;     otherwise wr = w, rho = chi2.
 *
 * The increment is a LEFT one, d = (omega_0..2, upsilon_0..2, sigma): S' = dS . S with dS = (Q(omega), upsilon,
 * k(sigma)), Q the pose call's Cayley map and k = (2 + sigma) / (2 - sigma), the Pade form of exp(sigma).  To first
 * order the forward camera point moves by da = omega x a + upsilon + sigma*a and the backward one by
 * db = is * R'(P x omega - upsilon - sigma*P).  Jacobian rows of the error (eu, ev) of a side, seven entries each:
 *   forward, with A = fx*iz, B = fy*iz, pxy = px*py (the pose call's monocular rows; the projection annihilates the
 *   scale column, sigma*a being along the ray, and that column is the constant 0.0f):
 *     Ju = [ pxy*fx, -((1.0f + px*px)*fx), py*fx, -A, 0.0f, px*A, 0.0f ]
 *     Jv = [ (1.0f + py*py)*fy, -(pxy*fy), -(px*fy), 0.0f, -B, py*B, 0.0f ]
 *   backward, with A = fx*iz, B = fy*iz of camera 2 at b: first the seven columns W_c of R'(P x e_c), -R'e_c, -R'P, for
 *   i = 0 .. 2 with (r0, r1, r2) = (R0i, R1i, R2i), column i of R:
 *     W_0i = r1*P_2 - r2*P_1,   W_1i = r2*P_0 - r0*P_2,   W_2i = r0*P_1 - r1*P_0,
 *     W_3i = -r0,  W_4i = -r1,  W_5i = -r2,   W_6i = -((r0*P_0 + r1*P_1) + r2*P_2);
 *   then for c = 0 .. 6:  D_ci = W_ci * is  (i = 0 .. 2),
 *     Ju_c = -(A * (D_c0 - px*D_c2)),   Jv_c = -(B * (D_c1 - py*D_c2)).
 * A side's 36 terms, in this order: for j = 0 .. 6, for k = j .. 6 (28 terms, the upper triangle row by row)
 *   H_jk = (Ju_j*Ju_k + Jv_j*Jv_k) * wr;   for j = 0 .. 6:  g_j = (Ju_j*eu + Jv_j*ev) * wr;   then rho.
 * The products with the constant 0.0f entries are carried out like any other.
 *
 * A PASS evaluates every match of the pair at one similarity and sums, in binary64, over the matches that are ACTIVE
 * and not dead: 38 sums S_0 .. S_37; S = (H, g, F = S_35, S_36, S_37).  The order is the pose call's: 256 partial sums
 * that start at +0.0; match i adds to partial i mod 256, in ascending i, first double(term) of each of its 36 forward
 * terms, then double(term) of each of its 36 backward terms (two additions to each of the sums 0 .. 35), then 1.0 to
 * sum 36, then double(chi2_1) and then double(chi2_2) to sum 37 (the plain chi2 of both sides); the partials are
 * combined by the pose call's halving tree (128, 64, 32, 16, 8, 4, 2, 1), unchanged; S is p[0].  No other float is ever
 * summed across matches.  A CLASSIFYING pass first sets the active set anew from EVERY match: active iff not dead and
 * chi2_1 <= th2 and chi2_2 <= th2 at the pass's similarity; it then sums over that new set.
 *
 * Per pair, binary64.  The state T = (R, t, s) is double(sim_in) and stays in binary64 for the whole call.
 *   Solve(S, lambda): the pose call's elimination on 7 x 7: A = the symmetric matrix of the H sums, A_jj = H_jj *
 *     (1.0 + lambda), rhs_j = -g_j.  With fixed_scale, row and column 6 are then replaced: A_j6 = A_6j = 0.0 for j < 6,
 *     A_66 = 1.0, rhs_6 = 0.0.  Gaussian elimination WITHOUT pivoting, for c = 0 .. 6: the solve fails unless
 *     A[c][c] > 0; for r = c+1 .. 6: f = A[r][c] / A[c][c]; for j = c+1 .. 6: A[r][j] = A[r][j] - f*A[c][j];
 *     rhs_r = rhs_r - f*rhs_c.  Back substitution, r = 6 .. 0: s = rhs_r; for j = r+1 .. 6 ascending: s = s - A[r][j]*d_j;
 *     d_r = s / A[r][r].  The solve also fails when a d_r is not finite, or unless |d_6| < 2.0.  (With fixed_scale
 *     d_6 = +0.0 and k = 1.0 exactly, so s stays double(sim_in[12]) bit for bit.)
 *   Retract(T, d): Q from (d_0, d_1, d_2) by the pose call's Cayley formulas;  k = (2.0 + d_6) / (2.0 - d_6);
 *     R'_ij = (Q_i0*R_0j + Q_i1*R_1j) + Q_i2*R_2j,   t'_i = k * ((Q_i0*t_0 + Q_i1*t_1) + Q_i2*t_2) + d_(3+i),
 *     s' = k * s.
 *   A ROUND is the pose call's Levenberg round, word for word, with this Solve, this Retract and F = S_35: lambda starts
 *   at 2^-10, up to `iters` iterations, a failed solve spends its iteration with lambda = min(8.0*lambda, 2^20), a trial
 *   is accepted iff F' < F (then lambda = max(lambda*0.25, 2^-30), else lambda = min(8.0*lambda, 2^20)), and the round
 *   ends when max_j |d_j| <= eps.  One pass per iteration.
 *   The call:  sim_in, cam1 or cam2 not finite, s > 0 false, or an fx or fy == 0: code 2.  n < min_obs: code 1.
 *   Otherwise every match is active and a pass at T gives round 0 its S; the passes of round r are robust iff
 *   r < huber_rounds.  After round r a CLASSIFYING pass at T, robust iff r + 1 < huber_rounds, gives the inlier mask
 *   (= the new active set), ninliers = S_36 and cost = S_37, and its S is the start of round r + 1, which runs unless
 *   r + 1 == rounds (code 0) or ninliers < min_obs (code 1).  A round continues from where the last ended.  (ORB-SLAM
 *   runs 5 iterations, removes the outliers and runs 10 or 5 more without the kernels; rounds = 2, iters = 5,
 *   huber_rounds = 2 keeps its kernels on and leaves the surplus iterations to the Levenberg stop.)
 *
 * Outputs, per pair, always written, all device.  sim_out float [batch][13] = float(T) (sim_in itself for code 2 and
 * for a pair that never ran a round); it may be exactly sim_in.  inlier uint8 [batch][stride]: the last classification,
 * 0 or 1 for i < n (all 0 for a pair that never ran a round); entries at and beyond n are not written.  ninliers uint32
 * [batch].  cost double [batch]: the tree-ordered sum of the inliers' plain chi2 of both sides (0 without a round).
 * status uint32 [batch] = code | evaluations << 8, evaluations = the number of passes made; code 0: all rounds ran;
 * 1: stopped for min_obs, the similarity is that of the last completed round, or sim_in; 2: as above.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, the levels, the table, batch and stride; the other
 * pointers are not looked at then).  Offsets use size_t arithmetic throughout.  No output may overlap an input or
 * another output, except that sim_out may be sim_in (so `inlier` is never `mask`).  Any violation, one level pointer
 * without the other, or a NULL or host pointer where a device pointer is required: PISLAM_ERR_INVALID, before anything
 * is launched or written.  `p` is a host struct, read during the call.  Asynchronous on the context stream; no
 * workspace, no host round trip: the call can be captured into a hipGraph as it is.  One workgroup runs a pair's whole
 * call in one launch; a batch above 1024 pairs is walked by the same 1024 workgroups in passes. */
typedef struct pislam_sim3_refine_params {
  int32_t rounds;        /* 1..8 (ORB-SLAM: 2) */
  int32_t iters;         /* 1..32 Levenberg iterations per round (ORB-SLAM: 5) */
  int32_t huber_rounds;  /* 0..rounds: rounds 0 .. huber_rounds - 1 are robust (ORB-SLAM: 2) */
  int32_t min_obs;       /* 3..16384 active matches needed to run a round (ORB-SLAM: 10) */
  float th2;             /* finite, > 0: the chi2 bound of one side and delta^2 of its Huber kernel (ORB-SLAM: 10.0f) */
  int32_t fixed_scale;   /* 0 / 1: 1 keeps s (stereo / RGB-D maps) */
  double eps;            /* >= 0: a round ends when no |d_j| exceeds it (1e-6) */
} pislam_sim3_refine_params;
int pislam_sim3_refine_batch(pislam_ctx *ctx, const pislam_sim3_refine_params *p, const float *sim_in, const float *cam1,
                             const float *cam2, const float *x1, const float *x2, const int32_t *obs1_q8,
                             const int32_t *obs2_q8, const uint32_t *counts, const uint8_t *level1, const uint8_t *level2,
                             const uint8_t *mask, const float *inv_sigma2, int nlevels, size_t stride, int batch,
                             float *sim_out, uint8_t *inlier, uint32_t *ninliers, double *cost, uint32_t *status);

/* ---- new map points from two key frames: the epipolar search -------------- */

/* The epipolar geometry of a key-frame pair (host only, pure, no context; stated to a tolerance, not bit for bit, like
 * pislam_two_view_decompose).  pose1, pose2: float [12], r0 .. r8 row-major, then t, Xc = R Xw + t (the pose call's
 * layout); cam1, cam2: float [4], fx, fy, cx, cy.  f12: float [9], row-major, with x1' F12 x2 = 0 for level-0 pixels x1 =
 * (u1, v1, 1) of key frame 1 and x2 of key frame 2: F12 = K1^-T [t12]x R12 K2^-1 with R12 = R1 R2', t12 = t1 - R12 t2
 * (ORB-SLAM's ComputeF12).  epipole: float [2], the centre of camera 1, -R1' t1, projected into image 2.  Everything is
 * computed in binary64 from the inputs converted exactly and rounded once to binary32: an entry of f12 is within one
 * binary32 ulp of the largest |entry| of the exact matrix, an epipole coordinate within one ulp of its own exact value.
 * An epipole behind camera 2 or at infinity is returned as it comes out: it may be infinite or a NaN, and that is legal
 * input below.  PISLAM_ERR_INVALID: a NULL pointer, an input that is not finite, or an fx or fy equal to 0. */
int pislam_epipolar_from_poses(const float *pose1, const float *pose2, const float *cam1, const float *cam2, float *f12,
                               float *epipole);

/* Epipolar search: ORB-SLAM's ORBmatcher::SearchForTriangulation without its selection tail,
 * which pislam_match_select_batch applies as it does for every matcher (the distance threshold too: ORB-SLAM tests it
 * before the geometry, and thresholding the best candidate gives the same winner).  It is the word-guided matcher with a
 * geometric test on every candidate: pairs, qdesc / tdesc, qgroup / tgroup, ngroups, counts and strides are exactly those
 * of pislam_match_hamming_bow_batch, and so are idx, dist and dist2 with their tie rule dist << 16 | j.  Pair b is (key
 * frame 1 = the query side, key frame 2 = the train side).  In addition, all device unless said:
 *   qobs_q8, tobs_q8  int32 [batch][stride][3]: (u, v, u_right) in Q8 level-0 pixels, read as pislam_pose_refine_batch
 *                     reads obs_q8: u and v clamped to [-2^22, 2^22], then float(q) * (1.0f / 256.0f) (exact); u_right
 *                     == INT32_MIN marks a MONOCULAR keypoint, nothing else of u_right is read.
 *   qlevel, tlevel    uint8 [batch][stride]: the pyramid level of each keypoint.
 *   qmask, tmask      uint8 [batch][stride] or NULL: a keypoint takes part iff its byte is non-zero ("has no map point
 *                     yet"); NULL: every keypoint takes part.
 *   f12, epipole      float [batch][9] and [batch][2], as pislam_epipolar_from_poses writes them.
 *   level_sigma2, level_scale   HOST float [nlevels], 1 <= nlevels <= 16, read during the call and carried by value in
 *                     the kernel arguments (a captured graph keeps its own copy).
 *   p                 HOST struct: chi2 (ORB-SLAM: 3.84f) and epipole_r2 (ORB-SLAM: 100.0f).
 * A pair whose nine f12 words are not all finite has no candidates.  In binary32, one rounding per written operation,
 * in the order the parentheses give, no fused multiply-add; every comparison is false for a NaN.  Per query i with the
 * pixel (u1, v1), once:
 *   a = (u1*F0 + v1*F3) + F6,  b = (u1*F1 + v1*F4) + F7,  c = (u1*F2 + v1*F5) + F8,  den = a*a + b*b
 * Train j with the pixel (u2, v2) on level lt = tlevel[j] is a candidate for query i iff
 *   qgroup[i] == tgroup[j] and both are below ngroups (the word-guided matcher's rule), and
 *   qmask is NULL or qmask[i] != 0, and tmask is NULL or tmask[j] != 0, and
 *   qlevel[i] < nlevels and lt < nlevels, and
 *   with num = (a*u2 + b*v2) + c:  num*num < (chi2*level_sigma2[lt])*den    (no division; den == 0 fails), and
 *   NOT (both keypoints are monocular and dx*dx + dy*dy < epipole_r2*level_scale[lt]), dx = ex - u2, dy = ey - v2,
 *   (ex, ey) = epipole (an epipole that is not finite excludes nothing).
 * Best and second are taken over these candidates only.  A query that takes no part (its mask byte is 0, its level or
 * group has no entry, its pair's f12 is not finite) writes idx -1 and dist and dist2 0xffffffff; entries at and beyond
 * nq_b are not written.  With chi2 = +inf, epipole_r2 = 0, NULL masks, every level below nlevels and a line with den > 0
 * (and num*num finite) for every query, the outputs equal pislam_match_hamming_bow_batch's word for word.
 * Limits: those of pislam_match_hamming_bow_batch (words in {1,2,4,8}; 1 <= ngroups <= 16384; t_stride <= 65535;
 * q_stride < 2^31; batch 0..65535); chi2 > 0 (+inf is allowed), epipole_r2 >= 0; level_sigma2 and level_scale finite
 * and > 0, level_scale non-decreasing.  Offsets use size_t arithmetic throughout.  Any violation, or a NULL or host
 * pointer where a device pointer is required (the masks alone may be NULL): PISLAM_ERR_INVALID, before anything is
 * launched or written.  Asynchronous on the context stream; the workspace is the context's own for this call (not the
 * word-guided matcher's) and grows on demand, which synchronises; after pislam_match_epipolar_reserve of the same or a
 * larger shape the call allocates nothing and never synchronises, so it can be captured into a hipGraph.
 *
 * Not here: the baseline test that skips a key-frame pair (the caller's), the rotation histogram and the uniqueness of
 * SearchForTriangulation's tail (pislam_match_select_batch), ORBmatcher::Fuse, which is pislam_match_fuse_batch, and
 * local bundle adjustment, which is pislam_local_ba_batch, below. */
typedef struct pislam_epipolar_params {
  float chi2;       /* > 0, +inf allowed: squared distance to the epipolar line in units of level_sigma2 (ORB-SLAM: 3.84f) */
  float epipole_r2; /* >= 0: two monocular keypoints are not matched this close to the epipole, times level_scale (100.0f) */
} pislam_epipolar_params;
int pislam_match_epipolar_reserve(pislam_ctx *ctx, int words, int ngroups, size_t t_stride, int batch);
int pislam_match_hamming_epipolar_batch(pislam_ctx *ctx, int words, int ngroups, const pislam_epipolar_params *p,
                                        const float *level_sigma2, const float *level_scale, int nlevels, const float *f12,
                                        const float *epipole, const uint32_t *qdesc, const uint32_t *qgroup,
                                        const int32_t *qobs_q8, const uint8_t *qlevel, const uint8_t *qmask,
                                        const uint32_t *qcounts, size_t q_stride, const uint32_t *tdesc,
                                        const uint32_t *tgroup, const int32_t *tobs_q8, const uint8_t *tlevel,
                                        const uint8_t *tmask, const uint32_t *tcounts, size_t t_stride, int batch,
                                        int32_t *idx, uint32_t *dist, uint32_t *dist2);

/* ---- new map points from two key frames: triangulation and stereo unprojection ---- */

/* The geometry of ORB-SLAM's LocalMapping::CreateNewMapPoints: per pair of key frames with
 * known poses, every selected match of two keypoints that have no map point yet becomes a map point or is refused.  The
 * point is triangulated, or unprojected from a stereo observation when that gives more parallax; it then has to lie in
 * front of both cameras, reproject within the per-level bound in both, and sit at distances that fit the two pyramid
 * levels.  The reference ships nothing of the kind: the semantics are this library's own, stated so that individually
 * rounded binary32 operations reproduce every output word.  This comment is the contract.  "float(v)" converts an
 * integer to binary32; every +, -, *, / and sqrt below is ONE binary32 operation rounded to nearest even, in the order
 * the parentheses give (a + b + c means (a + b) + c); no fused multiply-add, no reciprocal or fast approximation: the
 * division and the square root are the correctly rounded ones; denormals are kept.  Every comparison is false for a NaN.
 *
 * Inputs, all device unless said.  Pair b has n = min(counts[b], stride) slots (counts: uint32 [batch],
 * PISLAM_COUNT_INVALID counts as 0); slot s is one selected match.
 *   pose1, pose2    float [batch][12]: r0 .. r8 row-major, then t0 .. t2; Xc = R Xw + t (the pose call's layout).
 *   cam1, cam2      float [batch][5]: fx, fy, cx, cy, bf in level-0 pixels, one camera per key frame.
 *   obs1_q8, obs2_q8  int32 [batch][stride][3]: (u, v, u_right) in Q8 level-0 pixels, read exactly as
 *                   pislam_pose_refine_batch reads obs_q8: each clamped to [-2^22, 2^22], then float(q) * (1.0f / 256.0f)
 *                   (exact); u_right == INT32_MIN (tested before the clamp) marks a monocular keypoint.
 *   level1, level2  uint8 [batch][stride]: the pyramid level of each keypoint.
 *   level_scale, level_sigma2   HOST float [nlevels], 1 <= nlevels <= 16 (ORB-SLAM's mvScaleFactors and mvLevelSigma2),
 *                   read during the call and carried by value in the kernel arguments.
 *
 * Per pair, with R1, t1, R2, t2 the two poses and (fx_k, fy_k, cx_k, cy_k, bf_k) = cam_k:
 *   c_(3i+j) = (R2_(3i)*R1_(3j) + R2_(3i+1)*R1_(3j+1)) + R2_(3i+2)*R1_(3j+2)        R21 = R2 R1', row-major, i, j = 0..2
 *   c_(9+i)  = t2_i - ((c_(3i)*t1_0 + c_(3i+1)*t1_1) + c_(3i+2)*t1_2)               t21 = t2 - R21 t1
 *   O1_j = -((R1_j*t1_0 + R1_(3+j)*t1_1) + R1_(6+j)*t1_2), O2 likewise from R2, t2  the camera centres, -R' t
 *   ifx_k = 1.0f / fx_k,  ify_k = 1.0f / fy_k,  hb_k = (bf_k / fx_k) * 0.5f          (half the stereo baseline)
 * A pair with a pose or camera word that is not finite, or with an fx or fy equal to 0, gives every slot the status 9
 * and evaluates nothing.
 *
 * Per slot, `status` is the code of the first test that fails, or 0.  With l_k = level_k, (u_k, v_k, ur_k) the slot's
 * observation in key frame k:
 *  1. Status 1 (NO_LEVEL) if l_1 >= nlevels or l_2 >= nlevels.
 *  2. x_k = (u_k - cx_k)*ifx_k,  y_k = (v_k - cy_k)*ify_k;  bb = (x_2*x_2 + y_2*y_2) + 1.0f;
 *     a_i = (c_(3i)*x_1 + c_(3i+1)*y_1) + c_(3i+2)   (a = R21 (x_1, y_1, 1));
 *     cs = ((a_0*x_2 + a_1*y_2) + a_2) / sqrt(((a_0*a_0 + a_1*a_1) + a_2*a_2) * bb)     the cosine of the two rays
 *     (pislam_two_view_reconstruct_batch's formula, with each side's own camera).
 *  3. Side k is STEREO iff its u_right is not INT32_MIN and d_k = u_k - ur_k > 0.0f.  Then zs_k = bf_k / d_k and
 *     cs_k = (zs_k*zs_k - hb_k*hb_k) / (zs_k*zs_k + hb_k*hb_k)  (= cos(2 atan(hb_k / zs_k)), without a trigonometric
 *     call).  A side that is not stereo is monocular in every step below and has cs_k = cs + 1.0f.
 *  4. mn = cs_2 < cs_1 ? cs_2 : cs_1.  The mode is
 *       TRIANGULATE  iff cs < mn and cs > 0.0f and (side 1 is stereo or side 2 is stereo or cs < cos_min_parallax),
 *       else STEREO1 iff side 1 is stereo and cs_1 < cs_2,
 *       else STEREO2 iff side 2 is stereo and cs_2 < cs_1,
 *       else status 2 (LOW_PARALLAX).
 *  5. The point.  TRIANGULATE: the midpoint X of the two rays' closest points in frame 1, which is
 *     pislam_two_view_reconstruct_batch's n, nn, p, q, z1, z2, g, h and X word for word with r = c_0 .. c_8,
 *     t = c_9 .. c_11, (x1, y1) = (x_1, y_1), (x2, y2) = (x_2, y_2); then with e = X - t1 (three subtractions)
 *     Xw_j = (R1_j*e_0 + R1_(3+j)*e_1) + R1_(6+j)*e_2.  (Both poses the identity but t2 = (-1, 0, 0), both cameras
 *     (1, 1, 0, 0, 0), (u_1, v_1) = (0, 0), (u_2, v_2) = (-0.5, 0): z1 = z2 = 2 and Xw = (0, 0, 2).)
 *     STEREOk: X = (x_k*zs_k, y_k*zs_k, zs_k) in frame k, to the world the same way with Rk, tk.
 *     Status 3 (NOT_FINITE) unless the three words of Xw are finite.
 *  6. Through each pose: x = ((r0*Xw_0 + r1*Xw_1) + r2*Xw_2) + t0, y and z likewise (the pose call's).  Status 4
 *     (DEPTH1) unless z > 0.0f in key frame 1, else status 5 (DEPTH2) unless z > 0.0f in key frame 2.
 *  7. In each key frame iz = 1.0f / z, px = x*iz, py = y*iz, pu = fx*px + cx, pv = fy*py + cy, eu = u - pu,
 *     ev = v - pv, and on a stereo side er = ur - (pu - bf*iz) (the pose call's).  A monocular side passes iff
 *     eu*eu + ev*ev <= chi2_mono*level_sigma2[l], a stereo side iff (eu*eu + ev*ev) + er*er <=
 *     chi2_stereo*level_sigma2[l].  Status 6 (REPROJ1) unless side 1 passes, else status 7 (REPROJ2) unless side 2 does.
 *  8. e = Xw - O1, f = Xw - O2 (three subtractions each), d_1 = sqrt((e_0*e_0 + e_1*e_1) + e_2*e_2), d_2 likewise from
 *     f; r_1 = d_1*level_scale[l_1], r_2 = d_2*level_scale[l_2].  Status 8 (SCALE) if d_1 == 0.0f or d_2 == 0.0f, or
 *     unless (d_2*ratio_factor)*level_scale[l_2] >= r_1 and r_2 <= r_1*ratio_factor (ORB-SLAM's ratioDist against
 *     ratioOctave, the two divisions multiplied out).
 *
 * Outputs, device, written for every slot s < n and for no other:
 *   status  uint8 [batch][stride]
 *   xw      float [batch][stride][3]: Xw for status 0, else three zeros
 *   normal  float [batch][stride][3] or NULL: for status 0, w_j = e_j / d_1 + f_j / d_2,
 *           wn = sqrt((w_0*w_0 + w_1*w_1) + w_2*w_2), normal_j = w_j / wn (the mean viewing direction); else zeros
 *   drange  float [batch][stride][2] or NULL: for status 0, (r_1 / level_scale[nlevels - 1], r_1); else zeros
 *           (ORB-SLAM's UpdateNormalAndDepth for a point with two observations and key frame 1 as its reference: exactly
 *           the normal and drange that pislam_match_projection_batch reads in map mode)
 * and, per pair, always written: npoints uint32 [batch] = the number of status-0 slots, an integer count.  No float is
 * summed across slots: the results are bit-for-bit reproducible and independent of the launch shape.
 *
 * Limits: level_scale and level_sigma2 finite and > 0, level_scale non-decreasing; chi2_mono, chi2_stereo and
 * ratio_factor finite and > 0; cos_min_parallax finite; 1 <= stride <= 16384; batch >= 0 with no upper limit (batch ==
 * 0 is a no-op that returns PISLAM_OK after the checks of p, the tables, batch and stride; the pointers are not looked
 * at then).  Offsets use size_t arithmetic throughout.  No output may overlap an input or another output.  Any
 * violation, or a NULL or host pointer where a device pointer is required (normal and drange alone may be NULL):
 * PISLAM_ERR_INVALID, before anything is launched or written.  `p` and the tables are host memory, read during the
 * call.  Asynchronous on the context stream; no workspace, no host round trip: the call can be captured into a
 * hipGraph as it is, so there is no reserve call.  One lane works on a slot, one workgroup on a pair; a batch above
 * 1024 pairs is walked by the same 1024 workgroups in passes.
 *
 * Not here: the baseline test that skips a key-frame pair (the caller's), ORBmatcher::Fuse, the step after this one
 * (pislam_match_fuse_batch takes xw, normal and drange as they are), and local bundle adjustment, the step after that:
 * pislam_local_ba_batch, below, takes xw and the pose layout as they are.  (The matches come from
 * pislam_match_hamming_epipolar_batch.) */
typedef struct pislam_triangulate_params {
  float cos_min_parallax; /* finite; two monocular keypoints are triangulated iff cs < this (ORB-SLAM: 0.9998f) */
  float chi2_mono;        /* finite, > 0 (ORB-SLAM: 5.991f) */
  float chi2_stereo;      /* finite, > 0 (7.815f; ORB-SLAM uses 7.8f here) */
  float ratio_factor;     /* finite, > 0 (ORB-SLAM: 1.5f * the pyramid's scale factor) */
} pislam_triangulate_params;
int pislam_triangulate_batch(pislam_ctx *ctx, const pislam_triangulate_params *p, const float *pose1, const float *pose2,
                             const float *cam1, const float *cam2, const int32_t *obs1_q8, const int32_t *obs2_q8,
                             const uint8_t *level1, const uint8_t *level2, const uint32_t *counts,
                             const float *level_scale, const float *level_sigma2, int nlevels, size_t stride, int batch,
                             float *xw, uint8_t *status, float *normal, float *drange, uint32_t *npoints);

/* ---- local bundle adjustment: key-frame poses and map points together ---- */

/* What ORB-SLAM's Optimizer::LocalBundleAdjustment does, per WINDOW of a batch: the poses of
 * the window's free key frames and all of its map points are moved together so that the robust reprojection error of
 * every observation of a point in a key frame becomes minimal; the other key frames of the window are held fixed and
 * only anchor the points they see.  Levenberg on the Schur complement: the points are eliminated, a reduced system in
 * the 6 * kf_free camera unknowns is solved, the points follow.  The reference ships nothing of the kind: the semantics
 * are this library's own, stated so that individually rounded binary32 and binary64 operations reproduce every output
 * word.  This comment is the contract.  Every +, -, *, / and sqrt below is ONE binary32 or binary64 operation (as
 * marked) rounded to nearest even, NEVER fused into an FMA; the divisions and the square root are correctly rounded;
 * a NaN fails every comparison.  tests/test_local_ba.py restates it in numpy; tools/probes/ba_host_check.cpp compiles
 * the kernel's own arithmetic header (pislam_ba_math.h) for the host and runs a window serially.
 *
 * Inputs, all device, read only.  Window b has nkf = min(kf_counts[b], kf_stride) key frames, npt = min(pt_counts[b],
 * pt_stride) points and n = min(counts[b], stride) observations (PISLAM_COUNT_INVALID counts as 0); entries at and
 * beyond a count are never read.
 *   poses      float [batch][kf_stride][12]: per key frame R row-major, then t (Xc = R Xw + t): the pose call's layout
 *   cams       float [batch][kf_stride][5] = (fx, fy, cx, cy, bf), one camera per key frame
 *   kf_free    uint32 [batch]: key frames [0, kf_free) are optimised (FREE), the rest are held FIXED
 *   xw         float [batch][pt_stride][3]: the map points (pislam_triangulate_batch's xw goes in as it is)
 *   obs_q8     int32 [batch][stride][3], level uint8 [batch][stride] or NULL, inv_sigma2 HOST float [nlevels]: read
 *              exactly as pislam_pose_refine_batch reads them (u_right == INT32_MIN marks a monocular observation, a
 *              level >= nlevels makes the observation DEAD, NULL level: w = 1.0f)
 *   obs_kf     uint8 [batch][stride], obs_pt uint16 [batch][stride]: observation i is of point obs_pt[i] in key frame
 *              obs_kf[i].  The observations are SORTED by point and by key frame within a point: obs_pt is
 *              non-decreasing and obs_kf strictly increasing within a point (at most one observation per pair).
 *
 * One observation, binary32: exactly the pose call's, at r = float(R_k), t = float(t_k) of its key frame k (the state
 * rounded if k is free, the input if fixed), under cams[k], with (X, Y, Z) = float(state of its point): x, y, z, the
 * DEAD tests (z >= 2^-10, chi2 finite), iz, px, py, pu, pv, eu, ev, er, chi2, th, Huber's wr and rho, the rows Ju, Jv,
 * Jr and the 21 + 6 camera terms H_jk, g_j as stated there.  In addition the rows with respect to the point (minus the
 * projection's derivative times R; the products with the constant 0.0f entries are NOT carried out here), j = 0..2:
 *   Pu_j = Ju_3*r_(0j) + Ju_5*r_(2j),   Pv_j = Jv_4*r_(1j) + Jv_5*r_(2j),   Pr_j = Jr_3*r_(0j) + Jr_5*r_(2j)
 * (r_(ij) = r_(3i+j)), and from them, with "(+ ...)" for a stereo observation only, as in H_jk:
 *   cross terms, a = 0..5, j = 0..2:      W_aj = ((Ju_a*Pu_j + Jv_a*Pv_j) (+ Jr_a*Pr_j)) * wr
 *   point terms, j = 0..2, k = j..2:      V_jk = ((Pu_j*Pu_k + Pv_j*Pv_k) (+ Pr_j*Pr_k)) * wr
 *                j = 0..2:                gp_j = ((Pu_j*eu + Pv_j*ev) (+ Pr_j*er)) * wr
 *
 * A PASS evaluates the window at one state.  An observation CONTRIBUTES iff it is ACTIVE and not dead.  All sums are
 * binary64 sums of double(term), start at +0.0 and take the contributing observations only, in these orders, none of
 * which depends on the launch:
 *   per point p:           V_p (6), g_p (3), and (rho_p, n_p, c_p) = the sums of rho, of 1.0 and of chi2: over the
 *                          point's observations in ascending index
 *   F, the count, chi2:    256 partial sums; partial p mod 256 takes (rho_p, n_p, c_p) in ascending p; then the
 *                          partials are combined by halving as in the pose call (128, 64, .. 1): S = (F, S_1, S_2)
 *   per free key frame k:  H_k (21), g_k (6): over the key frame's observations in ascending index
 * The terms W of an observation are kept as binary32 words.  An observation of a fixed key frame adds to its point and
 * to F only.  A CLASSIFYING pass first sets the active set anew from EVERY observation (active iff not dead and chi2 <=
 * th), as in the pose call.
 *
 * A SOLVE at lambda, binary64, s = 1.0 + lambda, N = 6 * kf_free.
 *   Point blocks: a00 = V00*s, a01 = V01, a02 = V02, a11 = V11*s, a12 = V12, a22 = V22*s; eliminated without pivoting:
 *     f1 = a01/a00, f2 = a02/a00, b11 = a11 - f1*a01, b12 = a12 - f1*a02, b21 = a12 - f2*a01, b22 = a22 - f2*a02,
 *     f3 = b21/b11, c22 = b22 - f3*b12.  The point is HELD in this solve unless a00 > 0, b11 > 0 and c22 > 0.
 *     Sol(b0, b1, b2): b1 = b1 - f1*b0; b2 = b2 - f2*b0; b2 = b2 - f3*b1; x2 = b2/c22; x1 = (b1 - b12*x2)/b11;
 *     x0 = ((b0 - a01*x1) - a02*x2)/a00.
 *     HELD POINTS ARE THE NORMAL PATH, not an error: a point with no contributing observation (V = 0), or with too few
 *     to constrain it, is held; it takes no step and its terms leave the reduced system untouched.  After the first
 *     classification of a window with gross outliers such points are common.
 *   For each contributing observation o of a free key frame whose point p is not held, and each a: Y_o,a = Sol_p(
 *     double(W_a0), double(W_a1), double(W_a2)).
 *   The reduced system A d = rhs, for rows i = 6*ki + ai and columns j = 6*kj + aj >= i (A_ji = A_ij):
 *     A_ij starts at H_ki's sum (ai, aj) if ki == kj, times s if i == j, and at +0.0 if ki != kj; then, over the
 *     observations oi of key frame ki in ascending index (that is ascending point) that contribute, whose point p is not
 *     held and has a contributing observation oj in key frame kj:  A_ij = A_ij - ((y0*w0 + y1*w1) + y2*w2) with y =
 *     Y_oi,ai and w = double(W_aj,0..2 of oj).
 *     rhs_i starts at -g_ki[ai]; over the same observations oi:  rhs_i = rhs_i + ((y0*g0 + y1*g1) + y2*g2), g = g_p.
 *   Gaussian elimination WITHOUT pivoting, exactly as the pose call's: for c = 0 .. N-1 the solve fails unless A[c][c]
 *     > 0; for r > c: f = A[r][c]/A[c][c]; A[r][j] = A[r][j] - f*A[c][j] for j > c; rhs_r = rhs_r - f*rhs_c.
 *     Back substitution, r = N-1 .. 0:  d_r = rhs_r/A[r][r], then rhs_q = rhs_q - A[q][r]*d_r for every q < r.
 *   Points: a held point has dp = 0.  Otherwise b_j = -g_p[j]; over the point's contributing observations of free key
 *     frames k in ascending index, with e = d[6k .. 6k+5]:  b_j = b_j - (((((w_0j*e0 + w_1j*e1) + w_2j*e2) + w_3j*e3) +
 *     w_4j*e4) + w_5j*e5), w = double(W);  dp = Sol_p(b0, b1, b2).
 *   The solve fails as well when a word of d or of a dp is not finite.  dmax = the largest |word| of d and of all dp.
 *   Trial state: T'_k = Retract(T_k, d[6k .. 6k+5]), the pose call's Cayley retraction; X'_p = X_p + dp.
 *
 * Per window.  The state (the free poses, all points) is double(input) and stays in binary64 for the whole call.
 *   Refused on the device, in this order: code 3: kf_free > 16 or > nkf, an obs_kf >= nkf, an obs_pt >= npt, or the
 *   order above violated; code 2: a word of poses or cams below nkf, or of xw below npt, is not finite; code 1:
 *   n < min_obs.  Otherwise every observation is active and a pass gives round 0 its sums.  A ROUND is the pose call's
 *   Levenberg rule word for word (lambda = 2^-10; up to iters[r] iterations; a failed solve: lambda = min(8.0*lambda,
 *   2^20), the iteration is spent; otherwise one pass at the trial state, same active set, robust iff r < huber_rounds;
 *   F' < F: the trial state and its sums are taken, lambda = max(lambda*0.25, 2^-30), else lambda = min(8.0*lambda,
 *   2^20); the round ends when dmax <= eps).  After round r a CLASSIFYING pass, robust iff r + 1 < huber_rounds, gives
 *   the inlier mask (= the new active set), ninliers = S_1, cost = S_2 and the sums round r + 1 starts from, which runs
 *   unless r + 1 == rounds (code 0) or ninliers < min_obs (code 1).  A free key frame without a contributing
 *   observation makes every solve fail (its pivot is 0): the window then keeps its state, and ends with code 0 or 1.
 *
 * Outputs, per window, all device.  poses_out float [batch][kf_stride][12]: float(T_k) for a free key frame, the input
 * copied for a fixed one; xw_out float [batch][pt_stride][3] = float(X_p); inlier uint8 [batch][stride]: the last
 * classification; ninliers uint32, cost double, status uint32 [batch] = code | evaluations << 8 (evaluations = the
 * passes made).  For the codes 2 and 3, and for a window that never ran a round, the outputs are the inputs copied, the
 * mask is all 0, ninliers and cost are 0.  Entries at and beyond a count are never written.  poses_out may be exactly
 * poses and xw_out exactly xw (a window reads its inputs before it writes); no other overlap of an output with an input
 * or another output is allowed.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= kf_stride <= 32, 1 <= pt_stride <= 4096, 1 <= stride <=
 * 16384; batch >= 0 with no upper limit (batch == 0 is a no-op that returns PISLAM_OK after the checks of p, the table
 * and the shape).  Any violation, or a NULL or host pointer where a device pointer is required (level alone may be
 * NULL): PISLAM_ERR_INVALID, before anything is launched or written.  `p` and inv_sigma2 are host memory, read during
 * the call.  Asynchronous on the context stream.  The workspace (per workgroup: what grows with pt_stride and stride,
 * about 500 bytes per observation and 300 per point) belongs to the context and grows on demand, which synchronises;
 * after pislam_local_ba_reserve of the same or a larger shape the call allocates nothing and never synchronises, so it
 * can be captured into a hipGraph.  One workgroup runs a window's whole call in one launch; a batch above 1024 windows
 * is walked by the same 1024 workgroups in passes.
 *
 * Not here: ORBmatcher::Fuse (pislam_match_fuse_batch, which runs before this call so that a landmark is optimised
 * once), marginalisation, IMU terms; windows beyond the limits and whole maps are pislam_global_ba_batch's, below.  Which key frames form a
 * window (the key frame, its covisible neighbours, the key frames that see their points) is read off
 * pislam_covisibility_batch, below. */
typedef struct pislam_ba_params {
  int32_t rounds;        /* 1..4 (ORB-SLAM: 2) */
  int32_t iters[4];      /* 1..32 Levenberg iterations of round r, r < rounds (ORB-SLAM: 5, 10) */
  int32_t huber_rounds;  /* 0..rounds: rounds 0 .. huber_rounds - 1 are robust (ORB-SLAM: 1) */
  int32_t min_obs;       /* 1..16384 active observations needed to run a round */
  double eps;            /* >= 0: a round ends when no |increment word| exceeds it (1e-6) */
} pislam_ba_params;
int pislam_local_ba_reserve(pislam_ctx *ctx, size_t kf_stride, size_t pt_stride, size_t stride, int batch);
int pislam_local_ba_batch(pislam_ctx *ctx, const pislam_ba_params *p, const float *poses, const float *cams,
                          const uint32_t *kf_counts, const uint32_t *kf_free, const float *xw, const uint32_t *pt_counts,
                          const int32_t *obs_q8, const uint8_t *obs_kf, const uint16_t *obs_pt, const uint8_t *level,
                          const uint32_t *counts, const float *inv_sigma2, int nlevels, size_t kf_stride,
                          size_t pt_stride, size_t stride, int batch, float *poses_out, float *xw_out, uint8_t *inlier,
                          uint32_t *ninliers, double *cost, uint32_t *status);

/* ---- after a loop is accepted: essential-graph optimisation, map points moved ---- */

/* What ORB-SLAM's Optimizer::OptimizeEssentialGraph does, per GRAPH of a batch (one map, or
 * one loop hypothesis of one map): the FREE vertex similarities are moved so that the sum of the squared relative-Sim(3)
 * errors over the edges becomes minimal; the FIXED vertices (ORB-SLAM holds the loop key frame) are the gauge.
 * Levenberg; the damped normal equations are solved matrix-free by block-Jacobi preconditioned conjugate gradients.
 * The reference ships nothing of the kind: the semantics are this library's own.  This comment is the contract.
 * ALL arithmetic of this call is binary64: an input word v is converted exactly, double(v), an output is rounded once,
 * float(v).  Every +, -, *, / below is ONE binary64 operation rounded to nearest even, in the order the parentheses
 * give (a op b op c without parentheses is (a op b) op c), NEVER fused into an FMA; there is no transcendental
 * function; a NaN fails every comparison.  tests/test_pose_graph.py restates it in numpy; tools/probes/
 * graph_host_check.cpp compiles the kernel's own arithmetic header (pislam_graph_math.h) for the host and runs a graph
 * serially.
 *
 * Inputs, all device, read only.  Graph b has nv = min(v_counts[b], v_stride) vertices and ne = min(e_counts[b],
 * e_stride) edges (PISLAM_COUNT_INVALID counts as 0); entries at and beyond a count are never read.
 *   sims       float [batch][v_stride][13]: S_k = (R row-major, t, s), world to camera, Xc = s R Xw + t: the sim_out
 *              layout of pislam_sim3_ransac_batch and pislam_sim3_refine_batch
 *   fixed      uint8 [batch][v_stride]: nonzero = the vertex is held
 *   edges      uint32 [batch][e_stride][2] = (i, j): the vertex pair of edge e
 *   meas       float [batch][e_stride][13]: M_e, the measured S_j o S_i^-1 (ORB-SLAM's Sji)
 *   weight     float [batch][e_stride] or NULL: w_e, finite and >= 0; NULL: every w_e = 1.0 (ORB-SLAM: identity
 *              information)
 *   inc_ptr    uint32 [batch][v_stride + 1], inc uint32 [batch][2 * e_stride]: the incidence index.  Vertex k's ENTRIES
 *              are inc[inc_ptr[k] .. inc_ptr[k+1]); an entry is edge << 1 | side, side 0: k is the edge's i, side 1: its
 *              j.  The index is CONSISTENT iff inc_ptr[0] == 0, inc_ptr[k] <= inc_ptr[k+1], inc_ptr[nv] == 2 * ne, every
 *              entry of k names an edge < ne whose stated side is k, and the entries of a vertex are strictly ascending.
 *              Then every (edge, side) is an entry of exactly one vertex, and every per-vertex sum below has one owner
 *              and one order: ascending entries.
 *
 * Similarities.  A o B = (R_A R_B, s_A*(R_A t_B) + t_A, s_A*s_B), where a matrix product entry and a matrix-vector
 * entry is (x0*y0 + x1*y1) + x2*y2.  The ERROR of edge e at a state, with G = M_e o S_i:
 *   R_E = R_G R_j' (entry (a, b) = (G_a0*Rj_b0 + G_a1*Rj_b1) + G_a2*Rj_b2),  s_E = s_G / s_j,
 *   t_E = t_G - s_E*(R_E t_j)   (componentwise), that is E = M_e o S_i o S_j^-1.
 * The RESIDUAL r = (omega, upsilon, sigma) in R^7, with c = 1.0 + ((R_E00 + R_E11) + R_E22):
 *   omega = ((2.0*(R_E21 - R_E12))/c, (2.0*(R_E02 - R_E20))/c, (2.0*(R_E10 - R_E01))/c),  upsilon = t_E,
 *   sigma = (2.0*(s_E - 1.0))/(s_E + 1.0).
 * omega is the inverse of the pose call's Cayley map and sigma the inverse of the similarity refinement's factor
 * k(sigma) = (2 + sigma)/(2 - sigma), so r is the inverse of Retract at the identity: rational, no acos and no log, and
 * zero exactly when E is the identity.  It differs from g2o's Sim3 log in the terms of higher order in r only (the
 * rotation part is 2 tan(theta/2) against theta, the scale part 2 tanh(log(s)/2) against log s, the translation is not
 * multiplied by the inverse of the log's V matrix), which moves the minimiser of an inconsistent graph slightly and the
 * minimiser of a consistent one not at all.  The edge is ADMISSIBLE iff c > 2^-10 (a rotation error short of pi);
 * otherwise the state is INADMISSIBLE.  A dot product of two 7-vectors is ((((((a0*b0 + a1*b1) + a2*b2) + a3*b3) +
 * a4*b4) + a5*b5) + a6*b6).
 *   F = the sum over the edges of w_e*(r_e . r_e): 256 partial sums start at +0.0; partial e mod 256 takes its edges in
 *   ascending e; then the partials are combined by halving as in the pose call (128, 64, .. 1).
 *
 * The JACOBIANS of r_e with respect to the left increments d = (omega, upsilon, sigma) of S_i and S_j (S' = Retract(S,
 * d), pislam_sim3_refine_batch's Retract word for word: R' = Q R, t' = k*(Q t) + upsilon, s' = k*s), in closed form
 * from the 13 words of E and of M = M_e, with c = t_M - t_E:
 *   J_i d  = (a, ((c x a) + s_M*(R_M upsilon)) - sigma*c, sigma)  with a = R_M omega
 *   J_j d  = -(R_E omega, s_E*(R_E upsilon), sigma)
 *   J_i' u = (R_M' (u_w - (c x u_v)), s_M*(R_M' u_v), u_s - (c . u_v)),   J_j' u = -(R_E' u_w, s_E*(R_E' u_v), u_s)
 * (x: the cross product, each component one difference of two products; the sums of the upsilon row from the left).
 * The translation rows are the exact derivative at any E; the rotation and scale rows are exact to first order at
 * r = 0 (J_i = L_E Ad(M), J_j = -L_E Ad(E) with L_E the identity plus the upsilon-row terms -[t_E]x and t_E).  The
 * acceptance test on the exact F guards the approximation away from r = 0.  As a dense 7 x 7 matrix J_i has the rows
 * (R_M, 0, 0), ([c]x R_M, s_M*R_M, -c), (0, 0, 1.0) and J_j is -diag(R_E, s_E*R_E, 1.0), the other entries +0.0.
 *
 * A SOLVE at lambda of (J'WJ + lambda diag(J'WJ)) d = -J'W r in the 7 unknowns of every free vertex.
 *   Per free vertex k, over its entries in ascending order, starting at +0.0: the block H_k (upper triangle) gets
 *     H_ab = H_ab + w_e*h with h = the sum over the rows q = 0..6 of J_qa*J_qb in ascending q, all seven products
 *     carried out, J the dense matrix of the entry's side; the gradient gets g_k = g_k + J'(w_e*r_e).  diag_k = the
 *     diagonal of H_k.  The block with its diagonal times (1.0 + lambda) is eliminated WITHOUT pivoting exactly as the
 *     pose call's solve (f = A[r][c]/A[c][c]; A[r][j] = A[r][j] - f*A[c][j] for j > c); the solve FAILS unless every
 *     pivot is > 0, so a free vertex without an edge makes every solve fail.  Sol_k(b): b_r = b_r - f_rc*b_c for c
 *     ascending, r > c ascending; x_r = (b_r - A_r,r+1*x_r+1 - .. - A_r6*x_6)/A_rr for r = 6 .. 0.
 *   Start: x_k = 0, r_k = -g_k, z_k = Sol_k(r_k), p_k = z_k; p of a fixed vertex is +0.0 throughout.  A sum over the
 *     vertices, here rz = sum of r_k . z_k: 256 partial sums from +0.0; partial k mod 256 takes its free vertices in
 *     ascending k; then the halving tree.  thr = (cg_tol*cg_tol)*rz.
 *   Iteration n = 0 .. cg_iters - 1: stop if rz <= thr.  Per edge u_e = w_e*(J_i p_i + J_j p_j) componentwise.  Per
 *     free vertex (A p)_k = the sum over its entries in ascending order, from +0.0, of J' u_e (the entry's side), then
 *     (A p)_k,a = (A p)_k,a + (lambda*diag_k,a)*p_k,a.  pAp = the vertex sum of p_k . (A p)_k; the solve FAILS unless
 *     pAp > 0.  alpha = rz/pAp; x_k = x_k + alpha*p_k; r_k = r_k - alpha*(A p)_k; z_k = Sol_k(r_k); rz' = the vertex sum
 *     of r_k . z_k; beta = rz'/rz; p_k = z_k + beta*p_k; rz = rz'.
 *   d = x.  The solve fails as well when a word of d is not finite or |sigma_k| < 2 is false for a free vertex.  dmax =
 *     the largest |word| of d.  Trial state: S'_k = Retract(S_k, d_k) for every free vertex.
 *
 * Per graph.  The state is double(input) and stays in binary64 for the whole call, as two sets: current and trial.
 *   Refused on the device, in this order: code 3 (structure): an edge index >= nv, i == j, an inconsistent incidence
 *   index, or no fixed vertex; code 2 (values): a word of sims below nv, of meas or of weight below ne is not finite,
 *   an s <= 0, a weight < 0, or the input state is inadmissible; code 1: ne == 0 or no free vertex: nothing to do.
 *   Otherwise ONE round of the pose call's Levenberg rule word for word: lambda = 2^-10; up to `iters` iterations; a
 *   failed solve: lambda = min(8.0*lambda, 2^20), the iteration is spent; otherwise one evaluation of F at the trial
 *   state; an inadmissible trial state is rejected like a failed solve; F' < F: the trial state is taken, lambda =
 *   max(lambda*0.25, 2^-30), else lambda = min(8.0*lambda, 2^20); the round ends when dmax <= eps.  No robust kernel and
 *   no classification: ORB-SLAM has none here.
 *
 * Outputs, per graph, all device.  sims_out float [batch][v_stride][13]: float(S_k) for a free vertex, the input copied
 * for a fixed one; cost double [batch] = F at the final state; status uint32 [batch] = code | evaluations << 8
 * (evaluations = the evaluations of F made, the input state's included).  For the codes 1 to 3 the outputs are the
 * inputs copied, cost is 0 and status is the code.  Entries at and beyond a count are never written.  sims_out may be
 * exactly sims (a graph reads its similarities before it writes); no other overlap of an output with an input or
 * another output is allowed.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= v_stride <= 4096, 1 <= e_stride <= 16384; batch >= 0 with
 * no upper limit (batch == 0 is a no-op that returns PISLAM_OK after the checks of p and the shape); offsets use size_t
 * arithmetic.  Any violation, or a NULL or host pointer where a device pointer is required (weight alone may be NULL):
 * PISLAM_ERR_INVALID, before anything is launched or written.  `p` is host memory, read during the call.  Asynchronous
 * on the context stream.  The workspace (per workgroup 936 bytes per vertex of v_stride and 328 per edge of e_stride,
 * each array rounded up to 16 bytes and the slice to 256: 8.8 MiB at the limits) belongs to the context and grows on
 * demand, which synchronises; after pislam_pose_graph_reserve of the same or a larger shape the call allocates nothing
 * and never synchronises, so it can be captured into a hipGraph.  One workgroup runs a graph's whole call in one
 * launch, so a single large graph uses one compute unit; a batch above 1024 graphs is walked by the same 1024
 * workgroups in passes.
 *
 * Not here: a robust kernel, a several-workgroup form for one large graph.  That form is a call of its own,
 * pislam_pose_graph_wide_batch, below.  The bundle adjustment of the whole map that follows the correction is pislam_global_ba_batch, below.  The spanning-tree and covisibility edges of the graph come from pislam_covisibility_batch, below. */
typedef struct pislam_pose_graph_params {
  int32_t iters;     /* 1..64 Levenberg iterations (ORB-SLAM: 20) */
  int32_t cg_iters;  /* 1..1024 conjugate-gradient iterations of a solve at the most */
  double cg_tol;     /* in [0, 1): a solve stops when r'z <= cg_tol^2 times its first value */
  double eps;        /* >= 0: the round ends when no |increment word| exceeds it */
} pislam_pose_graph_params;
int pislam_pose_graph_reserve(pislam_ctx *ctx, size_t v_stride, size_t e_stride, int batch);
int pislam_pose_graph_batch(pislam_ctx *ctx, const pislam_pose_graph_params *p, const float *sims,
                            const uint32_t *v_counts, const uint8_t *fixed, const uint32_t *edges, const float *meas,
                            const float *weight, const uint32_t *e_counts, const uint32_t *inc_ptr, const uint32_t *inc,
                            size_t v_stride, size_t e_stride, int batch, float *sims_out, double *cost, uint32_t *status);

/* pislam_pose_graph_batch for large graphs: every phase of the call is one launch over all graphs of the batch and all
 * of their edges or vertices, so one large graph uses the whole device.  The contract is the comment of
 * pislam_pose_graph_batch, word for word: the residual, the Jacobians, the solve, every order of summation, the
 * Levenberg rule, the refusals with their codes and their order, the outputs and the in-place rule (sims_out may be
 * exactly sims: the state is read into the workspace before anything is written).  On the same inputs sims_out, cost
 * and status are that call's, bit for bit.  tools/probes/graph_wide_host_check.cpp runs pgr::host_graph with these
 * limits.  What differs:
 *   work       uint32 [batch][2] or NULL, device: the solves attempted and the conjugate-gradient iterations made over
 *              all of them; both 0 for the codes 1 to 3.  No overlap with an input or another output.
 *   Limits     1 <= v_stride <= 65536 (what pislam_map_points_correct_batch accepts), 1 <= e_stride <= 2^20, so an
 *              entry edge << 1 | side fits 32 bits; batch >= 0; p as in pislam_pose_graph_params.
 *   Workspace  per GRAPH of the batch, not per workgroup: a control block of 256 bytes, then 944 bytes per vertex of
 *              v_stride and 336 per edge of e_stride (pislam_pose_graph_batch's slice plus one binary64 term of the sums
 *              per vertex and per edge; each array rounded up to 16 bytes, the slice to 256: 395 MiB for one graph at
 *              the limits).  It is a buffer of its own in the context and grows on demand, which synchronises; after
 *              pislam_pose_graph_wide_reserve of the same or a larger shape and batch the call allocates nothing, never
 *              synchronises and can be captured into a hipGraph (one memset node and a single chain of kernel nodes).
 *   Launches   the host issues a fixed sequence from p alone and reads nothing back:
 *                5 + iters * (5 + 6 * cg_iters)
 *              launches (the checks, the load, the first evaluation and its rule; per Levenberg iteration the set-up
 *              and the start of the solve, six launches per conjugate-gradient iteration, the retraction, the evaluation
 *              and the rule; the outputs).  A graph that is refused, has converged, or whose solve has met its
 *              stopping rule skips the remaining launches from its control block, but the launches are still issued:
 *              iters * cg_iters is paid in launches (a few microseconds each), not only in work.  At the parameter
 *              limits that is 393 541 launches; choose cg_iters for the graph at hand.  The grid of a launch follows
 *              the strides: (graph, group of 256 items) pairs, at most 65536 workgroups, more are walked in passes.
 * Which call: this one for a graph of more than a few hundred vertices or beyond the other's limits;
 * pislam_pose_graph_batch for batches of many small graphs (INTEGRATION.md has the measured crossover).
 * Any violation of the limits, or a NULL or host pointer where a device pointer is required (weight and work alone may
 * be NULL): PISLAM_ERR_INVALID, before anything is launched or written. */
int pislam_pose_graph_wide_reserve(pislam_ctx *ctx, size_t v_stride, size_t e_stride, int batch);
int pislam_pose_graph_wide_batch(pislam_ctx *ctx, const pislam_pose_graph_params *p, const float *sims,
                                 const uint32_t *v_counts, const uint8_t *fixed, const uint32_t *edges, const float *meas,
                                 const float *weight, const uint32_t *e_counts, const uint32_t *inc_ptr,
                                 const uint32_t *inc, size_t v_stride, size_t e_stride, int batch, float *sims_out,
                                 double *cost, uint32_t *status, uint32_t *work);

/* The last step of LoopClosing::CorrectLoop: every map point moves with its reference key frame.  Point p < npt =
 * min(pt_counts[b], pt_stride) of element b with k = ref[p]: in binary64, one rounded operation at a time, with O =
 * double(sims_old[b][k]) and N = double(sims_new[b][k]) and X = double(xw[p]):
 *   c_a = s_O*((O_a0*X0 + O_a1*X1) + O_a2*X2) + t_O,a        (to the camera with the old similarity)
 *   d = c - t_N;  X'_a = ((N_0a*d0 + N_1a*d1) + N_2a*d2)/s_N  (back to the world with the new one)
 * xw_out[p] = float(X'), status[p] = 0.  If k >= nv = min(v_counts[b], v_stride) or a word of float(X') is not finite,
 * the point stays as it was (xw_out[p] = xw[p]) and status[p] = 1.  xw float [batch][pt_stride][3], ref uint16
 * [batch][pt_stride], sims_old and sims_new float [batch][v_stride][13], xw_out as xw, status uint8 [batch][pt_stride];
 * entries at and beyond npt are neither read nor written.  xw_out may be exactly xw; no other overlap of an output with
 * an input or another output is allowed.  1 <= pt_stride < 2^31, 1 <= v_stride <= 65536, batch >= 0; all pointers
 * device; a violation: PISLAM_ERR_INVALID before anything is launched.  One thread per point, walked in grid passes;
 * asynchronous on the context stream, no workspace: capturable as it is. */
int pislam_map_points_correct_batch(pislam_ctx *ctx, const float *xw, const uint16_t *ref, const uint32_t *pt_counts,
                                    const float *sims_old, const float *sims_new, const uint32_t *v_counts,
                                    size_t pt_stride, size_t v_stride, int batch, float *xw_out, uint8_t *status);

/* ---- the covisibility graph: weights, ordered neighbours, spanning tree, culling statistic ---- */

/* What ORB-SLAM's KeyFrame::UpdateConnections computes for every key frame of a MAP at once,
 * with the spanning tree that the first UpdateConnections of each key frame fixes and the statistic that
 * LocalMapping::KeyFrameCulling decides on.  One batch item is one map: a local map of a few dozen key frames, or a
 * whole map.  The reference ships nothing of the kind: the semantics are this library's own.  This comment is the
 * contract.  Everything is integer counting: every output is exact for every valid input, and the same inputs give the
 * same outputs bit for bit.  tests/test_covisibility.py restates it with dictionaries of sets; tools/probes/
 * covis_host_check.cpp compiles the kernels' own rules (pislam_covis_math.h) for the host and runs a map serially.
 *
 * Inputs, all device, read only.  Map b has nk = kf_counts[b] key frames, indexed in creation order, and n = counts[b]
 * observations; both are SIGNED words that are checked, not clamped.  Entries at and beyond n are never read.
 *   obs_pt     int32 [batch][stride]: the map point of observation i, >= 0
 *   obs_kf     uint16 [batch][stride]: its key frame, < nk
 *              The first n entries are STRICTLY ASCENDING in (obs_pt, obs_kf): sorted by point and by key frame within
 *              a point, and no pair occurs twice.
 *   obs_level  uint8 [batch][stride] or NULL: the pyramid level of the observation's keypoint; NULL: all zero
 *   cull_mask  uint8 [batch][stride] or NULL: zero takes the observation out of the culling statistic OF ITS OWN KEY
 *              FRAME only (ORB-SLAM: far stereo points are not counted); it still is an observer of its point and counts
 *              in every weight; NULL: all count
 *
 * Definitions.  The OBSERVERS of a point are the key frames of its observations.  w(i, j), i != j, is the number of
 * points that both key frame i and key frame j observe.  Key frame j QUALIFIES for i iff w(i, j) >= min_weight.  If
 * nobody qualifies for i and some w(i, j) > 0, the FALLBACK applies: the single j with the largest w(i, j) qualifies, the
 * smallest such j on a tie (UpdateConnections' "if none, keep the best").
 *
 * Outputs, per map, all device.
 *   nb_idx     uint16 [batch][kf_stride][nb_stride], nb_weight int32 of the same shape: row i holds the key frames that
 *              qualify for i, ordered by weight descending and by index ascending on equal weight
 *              (mvpOrderedConnectedKeyFrames with the tie made definite), with their weights.  The first min(nb_count,
 *              nb_stride) entries are written; the entries behind them are not touched.
 *   nb_count   int32 [batch][kf_stride]: the number that qualify; it may exceed nb_stride, which is how truncation shows
 *   parent     uint16 [batch][kf_stride]: the spanning tree.  parent[k] is the j < k with the largest w(k, j) > 0, the
 *              smallest such j on a tie, 0xFFFF if there is none: what ORB-SLAM fixes at key frame k's first
 *              UpdateConnections, when only earlier key frames exist and the fallback makes the best one front().
 *              parent[0] is always 0xFFFF and the tree has no cycle.
 *   kf_points  int32 [batch][kf_stride]: the observations of the key frame whose cull_mask is nonzero (its SUBJECTS)
 *   kf_redundant int32 [batch][kf_stride]: the subjects whose point has at least cull_min_observers OTHER observers o
 *              with level(o) <= level(subject) + cull_level_slack.  KeyFrameCulling removes k when kf_redundant >
 *              0.9 * kf_points: that comparison is the caller's.
 *   status     int32 [batch]: 0 ok; 1 nothing to do (nk == 0 or n == 0); 3 malformed: n outside [0, stride], nk outside
 *              [0, kf_stride], an obs_kf >= nk, a negative obs_pt, or a list that is not strictly ascending.
 * For the codes 1 and 3 the map's nb_count, kf_points and kf_redundant rows are zero, its parent row is 0xFFFF, and its
 * nb_idx and nb_weight are untouched.  A malformed map never indexes outside its own workspace and outputs and does not
 * disturb the other maps of the batch.  The rows k >= nk of a good map read like rows of a key frame without
 * observations (counts 0, parent 0xFFFF).  A weight can be as large as the number of observations of a key frame and
 * is carried in 32 bits throughout.  The votes of Tracking::UpdateLocalKeyFrames for a frame are the row of that frame
 * appended to the map as key frame nk, with min_weight = 1.
 *
 * Limits: the parameter ranges in the struct comments; 1 <= kf_stride <= 4096 (the vertex limit of
 * pislam_pose_graph_batch: a map that fits this call fits that one), 1 <= stride < 2^31, 1 <= nb_stride <= kf_stride;
 * batch >= 0 (batch == 0 is a no-op that returns PISLAM_OK after the checks of p and the shape); offsets use size_t
 * arithmetic.  Any violation, or a NULL or host pointer where a device pointer is required (obs_level and cull_mask
 * alone may be NULL), or an output that overlaps an input or another output: PISLAM_ERR_INVALID with a message, before
 * anything is launched or written.  `p` is host memory, read during the call.  Asynchronous on the context stream: an
 * asynchronous memset of the workspace, a pass with one thread per observation that adds into a dense uint32 matrix
 * [kf_stride][kf_stride] per map with integer atomics (the order of arrival cannot change a word), and a pass with one
 * workgroup per key frame that sorts its row.  The workspace, 4 * batch * (kf_stride^2 + 2 * kf_stride + 1) bytes (64
 * MiB per map at kf_stride = 4096), belongs to the context and grows on demand, which synchronises; a size that the
 * device refuses is PISLAM_ERR_NOMEM.  After pislam_covisibility_reserve of the same or a larger shape the call
 * allocates nothing and never synchronises, so it can be captured into a hipGraph.
 *
 * Not here: building the windows of pislam_local_ba_batch from the graph.  The choice of a map point's descriptor is
 * pislam_map_points_update_batch, below, on the same observation list. */
typedef struct pislam_covis_params {
  int32_t min_weight;          /* >= 1 (ORB-SLAM: 15) */
  int32_t cull_min_observers;  /* >= 1 (ORB-SLAM: 3) */
  int32_t cull_level_slack;    /* 0..255 (ORB-SLAM: 1) */
} pislam_covis_params;
int pislam_covisibility_reserve(pislam_ctx *ctx, size_t kf_stride, size_t stride, int batch);
int pislam_covisibility_batch(pislam_ctx *ctx, const pislam_covis_params *p, const uint16_t *obs_kf, const int32_t *obs_pt,
                              const int32_t *counts, const int32_t *kf_counts, const uint8_t *obs_level,
                              const uint8_t *cull_mask, size_t kf_stride, size_t stride, size_t nb_stride, int batch,
                              uint16_t *nb_idx, int32_t *nb_weight, int32_t *nb_count, uint16_t *parent,
                              int32_t *kf_points, int32_t *kf_redundant, int32_t *status);

/* ---- the map points' summaries: mean viewing direction, distance range, representative descriptor ---- */

/* What ORB-SLAM's MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors compute, for every point of
 * a MAP at once: the words that pislam_match_projection_batch and pislam_match_fuse_batch read
 * of a map point (normal, drange, the query descriptor) and the nobs that frontend.fuseDecisions takes.  ORB-SLAM runs
 * the two after CreateNewMapPoints, after Fuse, after local bundle adjustment and after a loop correction; this call runs
 * after pislam_triangulate_batch, pislam_match_fuse_batch, pislam_local_ba_batch and pislam_map_points_correct_batch.
 * One batch item is one map, as in pislam_covisibility_batch.  The reference ships nothing of the kind: the semantics
 * are this library's own.  This comment is the contract.  Every +, -, *, / and sqrt below is ONE binary32 operation
 * rounded to nearest even, NEVER fused into an FMA, evaluated left to right as written; the divisions and the square
 * root are correctly rounded; a NaN fails every comparison.  tests/test_map_points_update.py restates it in numpy;
 * tools/probes/mapupdate_host_check.cpp compiles the kernels' own rules (pislam_mapupdate_math.h) for the host and runs a
 * map serially.
 *
 * Inputs, all device, read only.  Map b has nk = kf_counts[b] key frames, n = counts[b] observations (SIGNED words,
 * checked, not clamped) and npt = pt_counts[b] points (checked against pt_stride).  Entries at and beyond a count are
 * never read.
 *   obs_pt, obs_kf, counts, kf_counts: pislam_covisibility_batch's observation list, as they are: the first n entries
 *              STRICTLY ASCENDING in (obs_pt, obs_kf); here obs_pt < npt as well
 *   obs_level  uint8 [batch][stride]: the pyramid level of the observation's keypoint
 *   obs_desc   uint32 [batch][stride][8] or NULL: the 256-bit descriptor of the observation's keypoint, in the matchers'
 *              word order; NULL: no descriptor is chosen, and desc must be NULL
 *   poses      float [batch][kf_stride][12]: per key frame R row-major, then t (Xc = R Xw + t): the pose call's layout
 *   xw         float [batch][pt_stride][3]: the points
 *   ref        uint16 [batch][pt_stride] or NULL: each point's reference key frame, what
 *              pislam_map_points_correct_batch takes
 *   level_scale HOST float [nlevels], read during the call and carried by value (pislam_triangulate_batch's table)
 *
 * One point p.  Its OBSERVERS are the observations with obs_pt == p, in list order (ascending key frame), n_p of them,
 * observer i in key frame k_i with pose (R, t) on level l_i.
 *   Geometry:  O_j = -((R_j*t_0 + R_(3+j)*t_1) + R_(6+j)*t_2)   (the triangulation call's camera centre),  e = Xw - O,
 *              d_i = sqrt((e_0*e_0 + e_1*e_1) + e_2*e_2),  u_i = e / d_i (three divisions);
 *              w = u_0, then w = w + u_i for i = 1 .. n_p - 1, in list order;
 *              wn = sqrt((w_0*w_0 + w_1*w_1) + w_2*w_2),  normal = w / wn.
 *              The normal is a UNIT vector, as pislam_triangulate_batch writes it (ORB-SLAM divides the sum by n_p
 *              instead; the matchers only compare its cosine).  The sum has this one order, so the words do not depend
 *              on the launch shape.
 *   Reference: the observer whose key frame equals ref[p]; the first observer if ref is NULL; also the first observer,
 *              with status 2, if ref[p] is not among the observers (what MapPoint::EraseObservation does to mpRefKF).
 *   Range:     with the reference observer r:  rr = d_r * level_scale[l_r],  drange = (rr / level_scale[nlevels - 1], rr).
 *              For a point with two observers and the first as reference, normal and drange are
 *              pislam_triangulate_batch's words exactly.
 *   Descriptor: D(i, j) is the Hamming distance of the descriptors of observers i and j, D(i, i) = 0; med(i) is the
 *              element with index floor((n_p - 1) / 2) of row i sorted ascending, the self-distance included (ORB-SLAM's
 *              vDists[0.5*(N-1)]); desc[p] is the descriptor of the observer with the smallest med, the first in list
 *              order on a tie.  An integer choice: exact.
 *
 * Outputs, device, each written for every p < min(npt, pt_stride) and for no other point:
 *   normal     float [batch][pt_stride][3] or NULL;  drange float [batch][pt_stride][2] or NULL;
 *   desc       uint32 [batch][pt_stride][8] or NULL
 *   nobs       int32 [batch][pt_stride]: n_p
 *   first      int32 [batch][pt_stride] or NULL: the list index of the point's first observation, -1 if it has none
 *   pt_status  uint8 [batch][pt_stride]: 0 ok;  1 no observers (nobs 0; normal, drange and desc untouched);  2 the
 *              reference was replaced (everything written);  3 geometry refused: a pose word of an observer or a word of
 *              xw[p] is not finite, some d_i == 0, wn == 0, or a word of normal or drange is not finite (normal and
 *              drange zeros, desc still chosen);  4 l_r >= nlevels (drange zeros, normal and desc written).  Of 3, 4 and
 *              2 the first that applies.
 *   status     int32 [batch]: 0 ok; 1 nothing to do (npt == 0 or n == 0); 3 malformed: n outside [0, stride], nk outside
 *              [0, kf_stride], npt > pt_stride, an obs_kf >= nk, an obs_pt outside [0, npt), or a list that is not
 *              strictly ascending.  For the codes 1 and 3 every point of the map gets pt_status 1, nobs 0 and first -1,
 *              and its normal, drange and desc are untouched.  A malformed map never indexes outside its own rows and
 *              does not disturb the other maps of the batch.
 *
 * Limits: level_scale 1..16 entries, finite, > 0, non-decreasing; 1 <= kf_stride <= 4096, 1 <= stride < 2^31, 1 <=
 * pt_stride < 2^31; batch >= 0 (batch == 0 is a no-op that returns PISLAM_OK after the checks of the table and the
 * shape); offsets use size_t arithmetic.  Any violation, or a NULL or host pointer where a device pointer is required
 * (obs_desc, ref, normal, drange, desc and first alone may be NULL), desc without obs_desc, or an output that overlaps
 * an input or another output: PISLAM_ERR_INVALID with a message, before anything is launched or written.  No workspace
 * and no reserve call: status[b] carries the map's flag between the kernels (an asynchronous memset, then one thread per
 * observation slot that checks it), a point's observers are found by binary search in the ascending list, one lane
 * walks a point's observers for the geometry, one wave chooses the descriptors of as many tracks as fit its 64 lanes
 * together, and a track of more than 64 observers takes a workgroup.  Asynchronous on the context stream, never
 * synchronises: the call can be captured into a hipGraph as it is.
 *
 * Not here: adding and erasing observations and replacing a fused point (frontend.fuseDecisions lists them; the map is
 * the caller's), and mnVisible / mnFound, which are counters of the tracking thread. */
int pislam_map_points_update_batch(pislam_ctx *ctx, const uint16_t *obs_kf, const int32_t *obs_pt, const int32_t *counts,
                                   const int32_t *kf_counts, const uint8_t *obs_level, const uint32_t *obs_desc,
                                   const float *poses, const float *xw, const uint32_t *pt_counts, const uint16_t *ref,
                                   const float *level_scale, int nlevels, size_t kf_stride, size_t stride,
                                   size_t pt_stride, int batch, float *normal, float *drange, uint32_t *desc,
                                   int32_t *nobs, int32_t *first, uint8_t *pt_status, int32_t *status);

/* ---- global bundle adjustment: a whole map across workgroups ---- */

/* What ORB-SLAM's Optimizer::GlobalBundleAdjustemnt does, per MAP of a batch: all free key-frame
 * poses and all map points of the map are moved together so that the robust reprojection error of every observation
 * becomes minimal.  Levenberg on the Schur complement; the reduced camera system is never formed: it is solved
 * matrix-free by block-Jacobi preconditioned conjugate gradients (PCG).  Every phase of one map is spread over many
 * workgroups, one launch per phase.  The reference ships nothing of the kind: the semantics are this library's own.
 * This comment is the contract.  It is pislam_local_ba_batch's contract with the differences stated here and no others:
 * every +, -, *, / and sqrt is ONE binary32 or binary64 operation (as marked there and here) rounded to nearest even, in
 * the order the parentheses give, NEVER fused into an FMA; a NaN fails every comparison.  tests/test_global_ba.py restates
 * it in numpy; tools/probes/gba_host_check.cpp compiles the kernels' own arithmetic header (pislam_gba_math.h) for the
 * host and runs a map serially, phase by phase in the order of the launches.
 *
 * Inputs, all device, read only.  The map is indexed exactly as pislam_covisibility_batch and
 * pislam_map_points_update_batch index it: one observation list serves the three calls.  Map b has nk = kf_counts[b] key
 * frames and n = counts[b] observations (SIGNED words, checked, not clamped) and npt = min(pt_counts[b], pt_stride) points
 * (PISLAM_COUNT_INVALID counts as 0); entries at and beyond a count are never read.
 *   obs_pt     int32 [batch][stride], obs_kf uint16 [batch][stride]: the first n entries STRICTLY ASCENDING in (obs_pt,
 *              obs_kf), 0 <= obs_pt < npt, obs_kf < nk
 *   obs_q8     int32 [batch][stride][3], level uint8 [batch][stride] or NULL, inv_sigma2 HOST float [nlevels]: read
 *              exactly as pislam_local_ba_batch reads them
 *   poses      float [batch][kf_stride][12], cams float [batch][kf_stride][5], xw float [batch][pt_stride][3]: as there
 *   fixed      uint8 [batch][kf_stride]: nonzero = the key frame is held FIXED (ORB-SLAM holds key frame 0); the others are
 *              FREE.  It replaces the local call's "first kf_free", so that key-frame indices stay the map's own.
 *   kf_ptr     uint32 [batch][kf_stride + 1], kf_obs uint32 [batch][stride]: the key-frame side of the list.  The ENTRIES of
 *              key frame k are the observation indices kf_obs[kf_ptr[k] .. kf_ptr[k+1]).  The index is CONSISTENT iff
 *              kf_ptr[0] == 0, kf_ptr[k] <= kf_ptr[k+1] <= n, kf_ptr[nk] == n, every entry of k is an index < n of an
 *              observation whose obs_kf is k, and the entries of a key frame are strictly ascending.  Then every
 *              observation is an entry of exactly one key frame.  (frontend.keyFrameObservationIndex builds it.)
 *
 * One observation, a PASS, the per-point sums V_p, g_p and (rho_p, n_p, c_p) over the point's contiguous observations in
 * ascending index, the sums S = (F, S_1, S_2) over the points (256 partials by p mod 256, then halving), the point blocks
 * at s = 1.0 + lambda with the HELD rule and Sol_p, the retraction, the Levenberg rule of a ROUND, the rounds and the
 * CLASSIFYING passes: pislam_local_ba_batch's, word for word, with "free" read off `fixed`.  The terms W (6 x 3) and the
 * 27 camera terms of a contributing observation of a free key frame are kept as binary32 words.
 *
 * Per-key-frame sums.  Every sum over a key frame's entries is a 64-PARTIAL SUM: partial q = 0..63 starts at +0.0 and
 * takes the entries at the places q, q + 64, q + 128, .. of the key frame's list in ascending order, only those that
 * qualify as stated with the sum; then the partials are combined by halving: p[q] = p[q] + p[q + h] for q < h, h = 32,
 * 16, .. 1; the sum is p[0].  An entry o TAKES PART iff it contributes (pislam_local_ba_batch's term) and its point is
 * not held.  Dot products of 6-vectors are ((((a0*b0 + a1*b1) + a2*b2) + a3*b3) + a4*b4) + a5*b5.  A sum over the
 * KEY FRAMES: 256 partial sums from +0.0, partial k mod 256 takes its free key frames in ascending k, then halving
 * (128, 64, .. 1) as for S.
 *
 * A SOLVE at lambda, binary64, s = 1.0 + lambda.
 *   Point blocks, HELD, Sol_p: the local call's.
 *   Per free key frame k (the SET-UP):
 *     H_k (21, upper triangle row by row), g_k (6): 64-partial sums of double(term) over the contributing entries.
 *     H'_k = H_k with each diagonal entry times s.
 *     For an entry o that takes part, with its point p: Y_a = Sol_p(double(W_a0), double(W_a1), double(W_a2)), a = 0..5.
 *     E_ab (a <= b) = the 64-partial sum over the entries that take part of ((Y_a0*w_b0 + Y_a1*w_b1) + Y_a2*w_b2), w =
 *     double(W);  e_a = the 64-partial sum over the same entries of ((Y_a0*g0 + Y_a1*g1) + Y_a2*g2), g = g_p.
 *     The preconditioner block S_kk = H'_k - E (entry by entry, one subtraction) is eliminated WITHOUT pivoting exactly
 *     as the pose call's solve (f = A[r][c]/A[c][c]; A[r][j] = A[r][j] - f*A[c][j] for j > c); the solve FAILS unless
 *     every pivot is > 0, which is what a free key frame without a contributing observation does.  Sol_k(b): b_r = b_r -
 *     f_rc*b_c for c ascending, r > c ascending; x_r = (b_r - A_r,r+1*x_r+1 - .. - A_r5*x_5)/A_rr for r = 5 .. 0.
 *     rhs_k,a = (-g_k,a) + e_a.   Start: x_k = 0, r_k = rhs_k, z_k = Sol_k(r_k), p_k = z_k.
 *   rz = the key-frame sum of r_k . z_k;  thr = (cg_tol*cg_tol)*rz.
 *   PCG iteration n = 0 .. cg_iters - 1: stop if rz <= thr.
 *     Per point p (one owner): t_p,j starts at +0.0; over the point's contributing observations of free key frames k in
 *     ascending index, with e = p_k:  t_j = t_j + (((((w_0j*e0 + w_1j*e1) + w_2j*e2) + w_3j*e3) + w_4j*e4) + w_5j*e5), w
 *     = double(W);  q_p = Sol_p(t_p), and q_p = 0 if the point is held.
 *     Per free key frame: (S p)_k,a = (the dot product of row a of H'_k with p_k) - the 64-partial sum over the entries
 *     that take part of ((w_a0*q0 + w_a1*q1) + w_a2*q2), q = q_p of the entry's point.
 *     pAp = the key-frame sum of p_k . (S p)_k; the solve FAILS unless pAp > 0.  alpha = rz/pAp; x_k = x_k + alpha*p_k;
 *     r_k = r_k - alpha*(S p)_k; z_k = Sol_k(r_k); rz' = the key-frame sum of r_k . z_k; beta = rz'/rz; p_k = z_k +
 *     beta*p_k; rz = rz'.   (The pose graph call's scalars in its order.)
 *   d_k = x_k.  Points: the local call's dp with e = d_k.  The solve fails as well when a word of d or of a dp is not
 *   finite.  dmax = the largest |word| of d and of all dp (a maximum: its order is free).  Trial state: as there.
 *
 * Per map.  Refused on the device, in this order: code 3 (structure): n outside [0, stride], nk outside [0, kf_stride],
 * an obs_kf >= nk, an obs_pt outside [0, npt), a list that is not strictly ascending, or an inconsistent kf_obs index;
 * code 2: a word of poses or cams below nk, or of xw below npt, is not finite; code 1: n < min_obs, or no free key
 * frame.  Otherwise the rounds run as in the local call.
 *
 * Outputs, in-place rules (poses_out may be exactly poses, xw_out exactly xw), what a refused map writes and status =
 * code | evaluations << 8: the local call's.  work uint32 [batch][2] or NULL: (the solves begun, the PCG iterations of
 * all of them).  Entries at and beyond a count are never written.
 *
 * Limits: p->ba as in its struct comments, except min_obs 1..2^24; cg_iters 1..256, cg_tol in [0, 1); 1 <= kf_stride <=
 * 4096 (the limit of pislam_pose_graph_batch and pislam_covisibility_batch), 1 <= pt_stride <= 2^22, 1 <= stride <= 2^24;
 * batch >= 0 (batch == 0 is a no-op that returns PISLAM_OK after the checks of p, the table and the shape); offsets use
 * size_t arithmetic.  Any violation, or a NULL or host pointer where a device pointer is required (level and work alone
 * may be NULL), or a forbidden overlap: PISLAM_ERR_INVALID, before anything is launched or written.  `p` and inv_sigma2
 * are host memory, read during the call.  The workspace belongs to the context: per map a control block of 256 bytes and
 * 362 bytes per observation of stride, 317 per point of pt_stride and 992 per key frame of kf_stride (each array rounded
 * up to 16 bytes, the slice to 256: 6.9 GiB for one map at the limits, which is what bounds them); it grows on demand,
 * which synchronises; a size the device refuses is PISLAM_ERR_NOMEM.  After pislam_global_ba_reserve of the same or a
 * larger shape the call allocates nothing and never synchronises, so it can be captured into a hipGraph.
 *
 * Launches.  Asynchronous on the context stream.  The host issues a FIXED sequence from the parameters alone and reads
 * nothing back: one memset of the control blocks, then 7 + the sum over the rounds r of (iters[r] * (6 + 3 * cg_iters) +
 * 2) launches (at most 99 087; ORB-SLAM's schedule, rounds 1, iters {10}, with cg_iters 50: 1569).  Per Levenberg
 * iteration: the point factors, the key-frame set-up, the PCG start; per PCG iteration the points, the key frames, the
 * scalars; then the step, the pass, the decision.  Launch order is the only synchronisation between workgroups: no
 * cooperative launch, no grid-wide wait, no polling.  A workgroup whose map is refused, finished, converged (dmax <=
 * eps ends the round; rz <= thr ends the solve) returns at once from the map's control block.  The number of workgroups
 * of a launch follows the strides (points, observations or key frames of every map), not only the batch.
 *
 * Not here: propagating the result to key frames and points outside the map (the caller's, as in ORB-SLAM),
 * marginalisation, IMU terms.  ORB-SLAM's schedule is rounds 1, iters {10} (20 at map initialisation), huber_rounds 1; the
 * closing classification gives the inlier mask that ORB-SLAM does not compute. */
typedef struct pislam_gba_params {
  pislam_ba_params ba; /* as in pislam_local_ba_batch; min_obs 1..2^24 */
  int32_t cg_iters;    /* 1..256 conjugate-gradient iterations of a solve at the most */
  double cg_tol;       /* in [0, 1): a solve stops when r'z <= cg_tol^2 times its first value */
} pislam_gba_params;
int pislam_global_ba_reserve(pislam_ctx *ctx, size_t kf_stride, size_t pt_stride, size_t stride, int batch);
int pislam_global_ba_batch(pislam_ctx *ctx, const pislam_gba_params *p, const float *poses, const float *cams,
                           const uint8_t *fixed, const int32_t *kf_counts, const float *xw, const uint32_t *pt_counts,
                           const int32_t *obs_q8, const uint16_t *obs_kf, const int32_t *obs_pt, const uint8_t *level,
                           const int32_t *counts, const uint32_t *kf_ptr, const uint32_t *kf_obs, const float *inv_sigma2,
                           int nlevels, size_t kf_stride, size_t pt_stride, size_t stride, int batch, float *poses_out,
                           float *xw_out, uint8_t *inlier, uint32_t *ninliers, double *cost, uint32_t *status,
                           uint32_t *work);

/* ---- multi-GPU: one process per GPU, pyramids sharded, ONE collective ---- */

/* The reference is a single-threaded per-frame loop without cross-frame state
 * (demo/demo.cpp:77-101, README.md:59-82), so a batch of pyramids shards across
 * GPUs with no data-path exchange: rank r of `world` runs
 * pislam_orb_frontend_batch on its own contiguous range of pyramids.  The only
 * exchange is the all-gather of the per-pyramid keypoint counts (what a consumer
 * needs to place every rank's keypoints in one global list) — ncclAllGather over
 * RCCL/xGMI, 4 bytes per pyramid.  RCCL is bound at run time (librccl.so.1;
 * override with the environment variable PISLAM_RCCL_LIB); world == 1 never
 * touches it.  PISLAM_DIST_TRACE=1 makes pislam_dist_finalize print the host time
 * spent in each call of an exchange (a diagnostic, stderr).
 *
 *   rank 0:   pislam_dist_get_unique_id(id);  -> hand `id` to every rank (file, socket, MPI, env ...)
 *   all:      pislam_ctx_create(local_device, &ctx);  pislam_dist_init(ctx, id, rank, world);
 *   per step: pislam_orb_frontend_batch(ctx, ..., counts_local);
 *             pislam_dist_allgather_counts(ctx, counts_local, n_local, counts_all);
 *   end:      pislam_dist_synchronize(ctx);  pislam_dist_finalize(ctx);
 */
#define PISLAM_DIST_ID_BYTES 128

/* Contiguous split of `global_batch` pyramids: the first (global_batch % world)
 * ranks take one more.  Pure arithmetic; no context, no GPU. */
int pislam_dist_shard(int global_batch, int rank, int world, int *first, int *count);

/* ncclGetUniqueId: call on ONE rank, distribute the bytes to all of them. */
int pislam_dist_get_unique_id(uint8_t id[PISLAM_DIST_ID_BYTES]);

/* ncclCommInitRank on the context's device (collective: every rank must call
 * it with the same id and world).  Creates the context's collective stream.
 * world == 1: no communicator, `id` may be NULL. */
int pislam_dist_init(pislam_ctx *ctx, const uint8_t id[PISLAM_DIST_ID_BYTES], int rank, int world);
int pislam_dist_rank(const pislam_ctx *ctx);
int pislam_dist_world(const pislam_ctx *ctx);
/* Ranks in the context's communicator as RCCL itself reports them (ncclCommCount) — not the `world` the caller
 * passed in: 0 without a communicator (single GPU / not initialised), negative on error. */
int pislam_dist_comm_count(pislam_ctx *ctx);

/* all_counts[r*n + i] = rank r's local_counts[i] (DEVICE pointers, n equal on
 * every rank — pad ragged shards to the largest).  Enqueued on the context's
 * COLLECTIVE stream, ordered after everything enqueued on the context stream so
 * far; asynchronous to the host and to the context stream, so the next batch
 * call overlaps it.  local_counts / all_counts must stay untouched until the
 * collective has completed (pislam_dist_fence / pislam_dist_synchronize). */
int pislam_dist_allgather_counts(pislam_ctx *ctx, const uint32_t *local_counts, size_t n,
                                 uint32_t *all_counts);

/* Makes the context stream wait (on the device, not the host) for the
 * collective issued `back` calls ago (1 = the most recent): call it before
 * work that overwrites that collective's buffers.  With two alternating output
 * sets, pislam_dist_fence(ctx, 2) before each batch call is enough.  (The
 * completion events of the last 16 collectives are kept; an older one is
 * covered by waiting for the oldest kept — the collective stream is in order.) */
int pislam_dist_fence(pislam_ctx *ctx, int back);

/* The same two calls for a process that runs SEVERAL contexts / streams (batches in flight on separate
 * pipelines) over ONE communicator: the all-gather is ordered after `producer_stream` (a hipStream_t as void*)
 * instead of the context stream, the fence makes `consumer_stream` wait.  All collectives of the process then
 * go through one communicator and one collective stream, in host issue order — identical on every rank. */
int pislam_dist_allgather_counts_on(pislam_ctx *ctx, void *producer_stream, const uint32_t *local_counts, size_t n,
                                    uint32_t *all_counts);
int pislam_dist_fence_on(pislam_ctx *ctx, int back, void *consumer_stream);

/* Blocks the host until every collective issued on this context has completed. */
int pislam_dist_synchronize(pislam_ctx *ctx);

/* MAX of one host double over all ranks (ncclAllReduce; blocking; also a
 * barrier) — the "slowest rank" reduction of a timed region. */
int pislam_dist_allreduce_max(pislam_ctx *ctx, double *value);

/* Destroys the communicator and the collective stream (pislam_ctx_destroy does
 * this too). */
int pislam_dist_finalize(pislam_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PISLAM_HIP_H_ */
