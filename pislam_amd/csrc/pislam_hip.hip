// pislam_hip.hip — C ABI (include/pislam_hip.h) over the gfx950 kernels.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// There is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pislam_hip.h"

// rotated BRIEF table (behaviour of reference Brief.h:28-53), packed per pair
__device__ const uint32_t g_brief_tab[30 * 256] = {
#include "brief_table.inc"
};
static constexpr uint32_t h_brief_tab_packed[30 * 256] = {
#include "brief_table.inc"
};
// The same table as byte offsets into the LDS patch of the ORB kernels (rows pf::orb_row_ofs apart) whose row 15 /
// column 15 is the keypoint: ofs = row_ofs(dy+15) + (dx+15); low half = first
// sample point, high half = second.  Entry order: see make_brief_ofs.
struct BriefOfsTab {
  uint32_t v[30 * 256];
};
#include "pislam_dev.h"
__device__ const pdev::VrecpeTab g_vrecpe_tab = pdev::make_vrecpe_tab();   // used by pf::k_gather_orb
__device__ const pdev::OrbMaskTab g_orb_masks = pdev::make_orb_mask_tab();  // used by pf::orb_lane
extern __device__ const BriefOfsTab g_brief_ofs;
#include "pislam_stage_kernels.h"
#include "pislam_fused_kernels.h"
static constexpr int brief_row_ofs(int r) { return pf::orb_row_ofs(r); }
static constexpr BriefOfsTab make_brief_ofs() {
  BriefOfsTab t{};
  for (int i = 0; i < 30 * 256; i++) {
    const uint32_t e = h_brief_tab_packed[i];
    const int dx0 = (int8_t)(e & 0xff), dy0 = (int8_t)((e >> 8) & 0xff);
    const int dx1 = (int8_t)((e >> 16) & 0xff), dy1 = (int8_t)(e >> 24);
    // stored as [rot][t][r] for test k = 8 r + t (pf::orb_describe: lane r of a half runs tests 8 r .. 8 r + 7)
    const int rot = i >> 8, k = i & 255;
    t.v[rot * 256 + 32 * (k & 7) + (k >> 3)] =
        (uint32_t)(brief_row_ofs(dy0 + 15) + dx0 + 15) | ((uint32_t)(brief_row_ofs(dy1 + 15) + dx1 + 15) << 16);
  }
  return t;
}
__device__ const BriefOfsTab g_brief_ofs = make_brief_ofs();

#include "pislam_prep_kernels.h"
#include "pislam_match_kernels.h"
#include "pislam_project_kernels.h"
#include "pislam_track_kernels.h"
#include "pislam_bow_kernels.h"
#include "pislam_bowdb_kernels.h"
#include "pislam_epipolar_kernels.h"
#include "pislam_select_kernels.h"
#include "pislam_geom_kernels.h"
#include "pislam_geom_host.h"
#include "pislam_recon_kernels.h"
#include "pislam_pose_kernels.h"
#include "pislam_pnp_kernels.h"
#include "pislam_sim3_kernels.h"
#include "pislam_sim3_refine_kernels.h"
#include "pislam_mappoint_kernels.h"
#include "pislam_ba_kernels.h"
#include "pislam_graph_kernels.h"
#include "pislam_gba_kernels.h"
#include "pislam_graph_wide_kernels.h"
#include "pislam_covis_kernels.h"
#include "pislam_mapupdate_kernels.h"
#include "pislam_warp_kernels.h"
#include "pislam_clahe_kernels.h"

#define PISLAM_EXPORT extern "C" __attribute__((visibility("default")))

// the front end's host half (pislam_frontend_plan.h, included by pislam_fused_kernels.h)
using fp::cdiv, fp::frame_max_batch, fp::FrontendPlan, fp::LDS_CAP, fp::LDS_OPT_IN;

namespace {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  unsigned long long reallocs = 0;   // times the buffer moved: a captured hipGraph holds the OLD address
  // returns true if (re)allocated
  int ensure(size_t bytes, bool *grew = nullptr) {
    if (grew) *grew = false;
    if (bytes <= cap) return PISLAM_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(bytes, 256);
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      return PISLAM_ERR_NOMEM;
    }
    cap = want;
    reallocs++;
    if (grew) *grew = true;
    return PISLAM_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    reallocs++;
  }
  template <class T>
  T *as() const { return (T *)p; }
};

}  // namespace

struct pislam_dist_state;   // pislam_dist.inc

struct pislam_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;    // option "own_stream": a non-blocking stream created and destroyed by the context
  pislam_dist_state *dist = nullptr;   // multi-GPU state (pislam_dist_init), nullptr for a single GPU
  std::string err;
  fp::Options opt;                   // every integer option (pislam_ctx_set_option), the device's CUs, the pipeline depth: what the planner reads
  // staging for host-pointer calls
  DevBuf s_img, s_out, s_pts, s_desc, s_misc, s_rots, s_tmp;
  // compaction scratch (shared by extract and the batch pipeline)
  DevBuf w_cnt, w_off, w_total, w_cellkp;
  // batch pipeline workspace
  DevBuf w_score, w_stage, w_stripcnt, w_work, w_prof, w_ovf, w_stagedesc;
  DevBuf w_ustage, w_ucount;         // bucket selection pass (pf::k_bucket_select): per-unit lists and counts
  // Guided matchers: pm::k_scaled_index's cell offsets, cell-sorted train entries and their descriptors.  One set per
  // matcher (windowed, scaled, stereo, projection, fuse), so a graph captured for one is never invalidated by another's reserve.
  struct CellIndex {
    DevBuf off, meta, desc;
  };
  CellIndex w_win, w_sc, w_st, w_proj, w_fuse;   // (w_proj: the projection matcher, w_fuse: the fuse matcher)
  CellIndex w_bow;                   // word-guided matcher (pb::k_bow_index): group offsets, group-sorted indices (meta), descriptors
  CellIndex w_epi;                   // epipolar matcher (pe::k_epi_index): group offsets, group-sorted entries with their geometry (meta), descriptors
  DevBuf w_ba;                       // local bundle adjustment (pbk::k_local_ba): a slice per workgroup (pbk::ws_bytes)
  DevBuf w_pg;                       // essential-graph optimisation (pgk::k_pose_graph): a slice per workgroup (pgr::ws_bytes)
  DevBuf w_pgw;                      // essential graphs across workgroups (pgw::k_pgw_*): a control block and a slice per graph
  DevBuf w_gba;                      // global bundle adjustment (gbk::k_gba_*): a control block and a slice per map (gba::ws_bytes)
  DevBuf w_cv;                       // covisibility graph (pcvk::k_covis_count, k_covis_rows): matrices, counters, flags (pcv::ws_bytes)
  DevBuf w_db;                       // key-frame database query (pd::k_db_accumulate .. k_db_merge): accumulator planes, maxima, partial lists
  // Host-built plan tables the kernels read instead of walking the plan (the bucket selection pass's unit table): one
  // device buffer per distinct CONTENT, never rewritten in place — a captured graph keeps reading the table
  // of the plan it was captured with whatever other shapes the context serves in between.  At most 16 are kept (the oldest
  // is freed, and graphs of the library's pipeline are invalidated through workspace_generation()).
  struct PlanTable {
    std::vector<uint32_t> host;      // (kept: the upload is asynchronous)
    DevBuf dev;
  };
  std::vector<PlanTable *> plan_tables;
  const uint32_t *cur_utab = nullptr;   // the table of the call being issued
  DevBuf w_sync;                     // one-launch path (pf::k_frame): per-pyramid hand-over counters, zero between launches
  // The one-launch path's bounded wait (pf::k_frame): a workgroup that gives up raises a sticky flag in w_sync AND in this
  // host-mapped word, which every call on the context reads first (a plain host load: no synchronisation, no copy).
  uint32_t *frame_flag = nullptr;    // hipHostMalloc'ed, mapped
  uint32_t *frame_flag_dev = nullptr;
  bool frame_disabled = false;       // a timeout was seen: the context takes the three-launch path from then on
  unsigned long long frame_timeouts = 0;   // (counted into workspace_generation: graphs holding a k_frame node are dropped)
  // pyramid build: all reductions in one launch (pp::k_bilinear_chain) — band counters + [done, sticky fault]; the host-mapped
  // fault word is frame_flag[1]
  DevBuf w_chain;
  size_t chain_words = 0;            // counters the last build laid out (a different layout starts from zeros)
  bool chain_disabled = false;
  uint32_t last_strips = 0;  // strips of the last fused batch call (pislam_frontend_last_stats)
  int last_pipeline = 0;
  unsigned last_path = 0;    // PISLAM_PATH_* of the last batch call
  size_t score_bytes_valid = 0;   // bytes of w_score known to be in a consistent (zero-border) state
  pislam_frontend_params last_params{};
  std::vector<pislam_level> last_levels;
  int last_batch = 0;
  size_t last_stride = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timing_valid = false;
  // Sub-batch pipelining of the fused batch path (run_fused): the strip kernels of the sub-batches run back to
  // back on the context stream, the overflow pass + gather/ORB kernel of sub-batch i on `aux_stream` under the
  // strip kernel of sub-batch i+1 (fork / join with events: one call, one context).  A call being captured into a
  // hipGraph runs its sub-batches in order on the context stream instead (run_fused).
  hipStream_t aux_stream = nullptr;    // created on first use (non-blocking)
  hipEvent_t ev_sub[fp::MAX_SUB] = {};     // strips of sub-batch i done (context stream -> aux stream)
  hipEvent_t ev_join = nullptr;        // aux stream -> context stream at the end of the call
  int ovf_nsub = 0;                    // layout of w_ovf the last call / reserve established: lists, dwords per list
  size_t ovf_stride = 0;
  unsigned long long ovf_layouts = 0;  // times that layout changed (a replayed graph would read another layout's headers)
  unsigned long long table_uploads = 0;   // plan tables evicted (a graph captured with one of them holds a dangling address)
  // Everything a captured batch call bakes into its kernel arguments besides the caller's own pointers: the
  // addresses of the workspace buffers and the overflow-list layout.  pislam_pipeline_submit replays a hipGraph
  // only while this number is what it was at capture time.
  unsigned long long workspace_generation() const {
    unsigned long long g = ovf_layouts + table_uploads + frame_timeouts;
    for (const DevBuf *b : {&w_cnt, &w_off, &w_total, &w_cellkp, &w_score, &w_stage, &w_stripcnt, &w_work, &w_prof,
                            &w_ovf, &w_stagedesc, &w_ustage, &w_ucount, &w_sync, &w_chain})
      g += b->reallocs;
    return g;
  }
};

namespace {

int fail(pislam_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  (void)hipGetLastError();
  return code;
}

#define HIPCHK(c, call)                                                   \
  do {                                                                    \
    hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) return fail((c), PISLAM_ERR_HIP, #call, e_);    \
  } while (0)

#define PCHK(call)                     \
  do {                                 \
    int r_ = (call);                   \
    if (r_ != PISLAM_OK) return r_;    \
  } while (0)

bool is_device_ptr(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Host->device staging of a read-only/in-out byte range.
struct Staged {
  const void *host = nullptr;   // original host pointer (nullptr if the caller's was device)
  void *dev = nullptr;
  size_t bytes = 0;
};

int stage_in(pislam_ctx *c, DevBuf &buf, const void *p, size_t bytes, Staged *s, bool copy = true) {
  s->bytes = bytes;
  if (bytes == 0 || is_device_ptr(p)) {
    s->host = nullptr;
    s->dev = (void *)p;
    return PISLAM_OK;
  }
  if (buf.ensure(bytes) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(staging)");
  s->host = p;
  s->dev = buf.p;
  if (copy) HIPCHK(c, hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, c->stream));
  return PISLAM_OK;
}

int stage_out(pislam_ctx *c, const Staged &s, void *host_dst, size_t bytes) {
  if (!s.host || bytes == 0) return PISLAM_OK;
  HIPCHK(c, hipMemcpyAsync(host_dst, s.dev, bytes, hipMemcpyDeviceToHost, c->stream));
  return PISLAM_OK;
}

int sync(pislam_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PISLAM_OK;
}

int launch_ok(pislam_ctx *c, const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, PISLAM_ERR_HIP, what, e);
  return PISLAM_OK;
}


// ---- the in-grid hand-overs' safety net (pf::k_frame, pp::k_bilinear_chain) --------------------------------------------
// Both kernels contain workgroups that WAIT for other workgroups of the same grid; the waits are bounded, and a workgroup
// that gives up raises a sticky flag in device memory and a word of this host-mapped block (frame_flag[0]: k_frame,
// frame_flag[1]: the build chain), which every call on the context reads first — a plain host load: no synchronisation.
int ensure_fault_flag(pislam_ctx *c) {
  if (c->frame_flag) return PISLAM_OK;
  void *h = nullptr, *d = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipGetLastError();
    if (h) (void)hipHostFree(h);
    return fail(c, PISLAM_ERR_NOMEM, "hipHostMalloc(fault flag)");
  }
  c->frame_flag = (uint32_t *)h;
  c->frame_flag_dev = (uint32_t *)d;
  ((volatile uint32_t *)c->frame_flag)[0] = 0;
  ((volatile uint32_t *)c->frame_flag)[1] = 0;
  return PISLAM_OK;
}
// Has a launch of this context given up waiting?  Called at the start of every batch call and pyramid build, by
// pislam_pipeline_submit, pislam_ctx_synchronize, pislam_pipeline_synchronize and pislam_frontend_last_stats.  If so: drain
// the stream, reset the hand-over counters, stop taking that one-launch path on this context (small batches run as three
// launches / the build as one launch per level from now on; captured graphs that hold such a node are dropped through
// workspace_generation) and report the failure ONCE.  The front-end calls that were affected have published
// counts[pyr] = PISLAM_COUNT_INVALID in the caller's own buffer; a build that was affected left levels of its pyramids
// unwritten — the error of THIS call is the notice.
int check_frame_poison(pislam_ctx *c) {
  if (!c->frame_flag) return PISLAM_OK;
  volatile uint32_t *f = (volatile uint32_t *)c->frame_flag;
  const bool frame = f[0] != 0, chain = f[1] != 0;
  if (!frame && !chain) return PISLAM_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->w_sync.p) HIPCHK(c, hipMemsetAsync(c->w_sync.p, 0, c->w_sync.cap, c->stream));
  if (c->w_chain.p) HIPCHK(c, hipMemsetAsync(c->w_chain.p, 0, c->w_chain.cap, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  f[0] = f[1] = 0;
  if (frame) c->frame_disabled = true;
  if (chain) c->chain_disabled = true;
  c->frame_timeouts++;
  if (chain && !frame)
    return fail(c, PISLAM_ERR_HIP, "the one-launch pyramid build (pp::k_bilinear_chain) gave up — a wait for a level's rows timed out, "
                                   "or a frame's workgroups did not share one XCD: the pyramids of that build are invalid; this "
                                   "context now builds one launch per level");
  return fail(c, PISLAM_ERR_HIP, "the one-launch path (pf::k_frame) timed out waiting for its strip workgroups: the affected calls "
                                 "wrote counts = PISLAM_COUNT_INVALID; this context now runs small batches as three launches");
}

// ---- launch helpers shared by the 4-call API and the staged batch path ----

int launch_detect(pislam_ctx *c, const uint8_t *d_img, uint8_t *d_out, int vstep, size_t stride,
                  int batch, int border, int width, int height, int threshold) {
  const int ny = height - 2 * border;
  if (ny <= 0) return PISLAM_OK;   // Fast.h:60: the row loop does not execute
  const int nx = width - 2 * border;
  const int xend = nx > 0 ? border + 16 * cdiv(nx, 16) : border;   // Fast.h:61,149
  dim3 grid(std::max(1, cdiv(xend - border, pk::DT_W)), cdiv(ny, pk::DT_H), batch);
  hipLaunchKernelGGL(pk::k_fast_detect, grid, dim3(256), 0, c->stream, d_img, d_out, vstep, stride,
                     border, width, height, threshold & 0xff, xend);
  return launch_ok(c, "k_fast_detect");
}

int launch_harris(pislam_ctx *c, const uint8_t *d_img, uint8_t *d_out, int vstep, size_t stride,
                  int batch, int border, int width, int height, int32_t threshold) {
  const int ny = height - 2 * border, nx = width - 2 * border;
  if (ny <= 0 || nx <= 0) return PISLAM_OK;
  dim3 grid(cdiv(nx, pk::DT_W), cdiv(ny, pk::DT_H), batch);
  hipLaunchKernelGGL(pk::k_harris_score, grid, dim3(256), 0, c->stream, d_img, d_out, vstep, stride,
                     border, width, height, threshold);
  return launch_ok(c, "k_harris_score");
}

// Ordered extraction of one level for `batch` pyramids.  d_total[b] is the
// running keypoint count of pyramid b (in: offset of this level's first
// keypoint, out: += this level's count).  Scratch: w_cnt / w_off / w_cellkp.
int launch_extract(pislam_ctx *c, const uint8_t *d_score, int vstep, size_t stride, int batch,
                   int border, int lbs, int limit, int width, int height, uint32_t *d_kp,
                   size_t kp_stride, uint32_t cap, uint32_t add_xy, uint32_t *d_total) {
  const int ny = height - 2 * border, nx = width - 2 * border;
  if (ny <= 0 || nx <= 0) return PISLAM_OK;
  if (lbs == 0) {
    const int nrows = cdiv(ny, 2);
    if (c->w_cnt.ensure(sizeof(uint32_t) * (size_t)nrows * batch) != PISLAM_OK ||
        c->w_off.ensure(sizeof(uint32_t) * (size_t)nrows * batch) != PISLAM_OK)
      return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(extract scratch)");
    dim3 grid(cdiv(nrows, 4), 1, batch);
    hipLaunchKernelGGL(pk::k_nms_rows<false>, grid, dim3(256), 0, c->stream, d_score, vstep, stride,
                       border, width, height, nrows, c->w_cnt.as<uint32_t>(), (size_t)nrows,
                       (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)0, 0u, 0u);
    PCHK(launch_ok(c, "k_nms_rows<count>"));
    hipLaunchKernelGGL(pk::k_scan_counts, dim3(batch), dim3(256), 0, c->stream,
                       c->w_cnt.as<uint32_t>(), c->w_off.as<uint32_t>(), nrows, (size_t)nrows,
                       d_total);
    PCHK(launch_ok(c, "k_scan_counts"));
    hipLaunchKernelGGL(pk::k_nms_rows<true>, grid, dim3(256), 0, c->stream, d_score, vstep, stride,
                       border, width, height, nrows, (uint32_t *)nullptr, (size_t)nrows,
                       c->w_off.as<uint32_t>(), d_kp, kp_stride, cap, add_xy);
    return launch_ok(c, "k_nms_rows<emit>");
  }
  const int bs = 1 << lbs;
  const int ncx = (nx - 1) / bs + 1;   // Fast.h:201 numBuckets
  const int ncy = (ny - 1) / bs + 1;
  const int ncells = ncx * ncy;
  if (c->w_cnt.ensure(sizeof(uint32_t) * (size_t)ncells * batch) != PISLAM_OK ||
      c->w_off.ensure(sizeof(uint32_t) * (size_t)ncells * batch) != PISLAM_OK ||
      c->w_cellkp.ensure(sizeof(uint32_t) * (size_t)ncells * batch * limit) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(extract scratch)");
  const size_t lds = sizeof(uint32_t) * (size_t)(bs / 2) * (bs / 2);
  hipLaunchKernelGGL(pk::k_nms_cells, dim3(ncx, ncy, batch), dim3(64), lds, c->stream, d_score, vstep,
                     stride, border, width, height, lbs, limit, ncx, c->w_cnt.as<uint32_t>(),
                     c->w_cellkp.as<uint32_t>(), (size_t)ncells);
  PCHK(launch_ok(c, "k_nms_cells"));
  hipLaunchKernelGGL(pk::k_scan_counts, dim3(batch), dim3(256), 0, c->stream, c->w_cnt.as<uint32_t>(),
                     c->w_off.as<uint32_t>(), ncells, (size_t)ncells, d_total);
  PCHK(launch_ok(c, "k_scan_counts"));
  hipLaunchKernelGGL(pk::k_emit_cells, dim3(cdiv(ncells * limit, 256), 1, batch), dim3(256), 0,
                     c->stream, c->w_cnt.as<uint32_t>(), c->w_off.as<uint32_t>(),
                     c->w_cellkp.as<uint32_t>(), ncells, limit, (size_t)ncells, d_kp, kp_stride, cap,
                     add_xy);
  return launch_ok(c, "k_emit_cells");
}

int check_level_args(pislam_ctx *c, int vstep, int border, int width, int height, int min_border) {
  if (!c) return PISLAM_ERR_INVALID;
  if (vstep <= 0 || width <= 0 || height <= 0 || width > vstep)
    return fail(c, PISLAM_ERR_INVALID, "bad vstep/width/height");
  if (border < min_border) return fail(c, PISLAM_ERR_INVALID, "border too small for this stage");
  return PISLAM_OK;
}

// byte hull [lo, hi) of the image the reference's orbCompute reads for these points
void orb_hull(const uint32_t *pts, size_t n, int vstep, int before, int after_rows, int after_cols, ptrdiff_t *lo,
              ptrdiff_t *hi) {
  ptrdiff_t l = PTRDIFF_MAX, h = PTRDIFF_MIN;
  for (size_t i = 0; i < n; i++) {
    const int x = (pts[i] >> 12) & 0xfff, y = pts[i] & 0xfff;
    const ptrdiff_t a = (ptrdiff_t)(y - before) * vstep + (x - before);
    const ptrdiff_t b = (ptrdiff_t)(y + after_rows) * vstep + (x + after_cols) + 1;
    l = std::min(l, a);
    h = std::max(h, b);
  }
  *lo = l;
  *hi = h;
}

// Stage points + the image hull for the point-list entry points.  On return
// *d_img_base is a device pointer such that d_img_base[y*vstep+x] is valid for
// every byte the kernels touch.
// `before`: rows/columns before a point the consumer reads; `after_rows` / `after_cols`: rows / columns after it
// (ORB: 15 before, rows y+15, columns x+16 incl. the masked column of Orb.h:200-203 — the reference never
// touches row y+16, and with border = 15 that row may lie past the caller's image; Harris 8x8: 3 / 4 / 4).
int stage_points_image(pislam_ctx *c, int vstep, const uint8_t *img, const uint32_t *points, size_t n,
                       const uint8_t **d_img_base, const uint32_t **d_pts, int before = 15,
                       int after_rows = 15, int after_cols = 16) {
  Staged sp;
  std::vector<uint32_t> host_pts;
  const bool pts_dev = is_device_ptr(points);
  const bool img_dev = is_device_ptr(img);
  PCHK(stage_in(c, c->s_pts, points, n * sizeof(uint32_t), &sp));
  *d_pts = (const uint32_t *)sp.dev;
  if (img_dev) {
    *d_img_base = img;
    return PISLAM_OK;
  }
  const uint32_t *hp = points;
  if (pts_dev) {   // need the coordinates on the host to size the hull
    host_pts.resize(n);
    HIPCHK(c, hipMemcpyAsync(host_pts.data(), points, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             c->stream));
    PCHK(sync(c));
    hp = host_pts.data();
  }
  ptrdiff_t lo, hi;
  orb_hull(hp, n, vstep, before, after_rows, after_cols, &lo, &hi);
  if (lo < 0) return fail(c, PISLAM_ERR_INVALID, "point too close to the image origin for its patch");
  const size_t bytes = (size_t)(hi - lo);
  if (c->s_img.ensure(bytes) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(image hull)");
  HIPCHK(c, hipMemcpyAsync(c->s_img.p, img + lo, bytes, hipMemcpyHostToDevice, c->stream));
  *d_img_base = c->s_img.as<uint8_t>() - lo;
  return PISLAM_OK;
}

}  // namespace

// ===========================================================================
// context
// ===========================================================================
PISLAM_EXPORT int pislam_abi_version(void) { return PISLAM_ABI_VERSION; }

PISLAM_EXPORT int pislam_ctx_create(int device, pislam_ctx **out) {
  if (!out) return PISLAM_ERR_INVALID;
  *out = nullptr;
  // creation failures have no ctx to carry a message: say why on stderr (they are fatal for the
  // caller anyway — there is no CPU fallback)
#define CREATE_CHK(call)                                                                    \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "pislam_ctx_create: %s -> %s\n", #call, hipGetErrorString(e_));       \
      (void)hipGetLastError();                                                              \
      return PISLAM_ERR_HIP;                                                                \
    }                                                                                       \
  } while (0)
  int ndev = 0;
  CREATE_CHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) {
    fprintf(stderr, "pislam_ctx_create: no HIP device\n");
    return PISLAM_ERR_HIP;
  }
  if (device < 0) CREATE_CHK(hipGetDevice(&device));
  if (device >= ndev) return PISLAM_ERR_INVALID;
  CREATE_CHK(hipSetDevice(device));
  pislam_ctx *c = new pislam_ctx();
  c->device = device;
  if (hipDeviceGetAttribute(&c->opt.num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->opt.num_cus <= 0)
    c->opt.num_cus = 256;
  for (auto &e : c->ev) {
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) {
      fprintf(stderr, "pislam_ctx_create: hipEventCreate -> %s\n", hipGetErrorString(r));
      delete c;
      return PISLAM_ERR_HIP;
    }
  }
#undef CREATE_CHK
  // pislam_match_select_batch is capturable from its first call: its kernel's LDS (a 64 KB table and a little more) is
  // allowed here, not in the call.  (Should this fail, that call's launch reports it.)
  if (hipFuncSetAttribute((const void *)ps::k_match_select, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)ps::SEL_LDS_BYTES) != hipSuccess)
    (void)hipGetLastError();
  *out = c;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_finalize(pislam_ctx *c);

PISLAM_EXPORT int pislam_ctx_destroy(pislam_ctx *c) {
  if (!c) return PISLAM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  (void)pislam_dist_finalize(c);
  (void)hipStreamSynchronize(c->stream);
  for (DevBuf *b : {&c->s_img, &c->s_out, &c->s_pts, &c->s_desc, &c->s_misc, &c->s_rots, &c->s_tmp, &c->w_cnt,
                    &c->w_off, &c->w_total, &c->w_cellkp, &c->w_score, &c->w_stage, &c->w_stripcnt, &c->w_work, &c->w_prof, &c->w_ovf,
                    &c->w_stagedesc, &c->w_ustage, &c->w_ucount, &c->w_sync, &c->w_chain})
    b->release();
  for (pislam_ctx::CellIndex *w : {&c->w_win, &c->w_sc, &c->w_st, &c->w_proj, &c->w_fuse, &c->w_bow, &c->w_epi})
    for (DevBuf *b : {&w->off, &w->meta, &w->desc}) b->release();
  c->w_db.release();
  c->w_ba.release();
  c->w_pg.release();
  c->w_gba.release();
  c->w_pgw.release();
  c->w_cv.release();
  for (auto *t : c->plan_tables) {
    t->dev.release();
    delete t;
  }
  c->plan_tables.clear();
  for (auto &e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->aux_stream) {
    (void)hipStreamSynchronize(c->aux_stream);
    (void)hipStreamDestroy(c->aux_stream);
  }
  for (auto &e : c->ev_sub)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  if (c->frame_flag) (void)hipHostFree(c->frame_flag);
  delete c;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_ctx_set_stream(pislam_ctx *c, void *s) {
  if (!c) return PISLAM_ERR_INVALID;
  c->stream = (hipStream_t)s;
  return PISLAM_OK;
}

namespace {
// mode 1: a stream with default flags — it still synchronises with the legacy null stream, so device-pointer
// inputs produced on the null stream stay ordered before the call, as they were when the context issued on
// the null stream itself; mode 2: hipStreamNonBlocking (the caller orders its producers explicitly).
int use_own_stream(pislam_ctx *c, int mode) {
  HIPCHK(c, hipSetDevice(c->device));
  if (mode) {
    if (c->own_stream) {
      HIPCHK(c, hipStreamSynchronize(c->own_stream));
      if (c->stream == c->own_stream) c->stream = nullptr;
      HIPCHK(c, hipStreamDestroy(c->own_stream));
      c->own_stream = nullptr;
    }
    HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, mode == 2 ? hipStreamNonBlocking : hipStreamDefault));
    c->stream = c->own_stream;
  } else if (c->own_stream) {
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    if (c->stream == c->own_stream) c->stream = nullptr;
    HIPCHK(c, hipStreamDestroy(c->own_stream));
    c->own_stream = nullptr;
  }
  return PISLAM_OK;
}
}  // namespace

PISLAM_EXPORT int pislam_ctx_set_option(pislam_ctx *c, const char *key, int value) {
  if (!c || !key) return PISLAM_ERR_INVALID;
  // the two options with a side effect on the context; every other one is an int of fp::Options
  if (!strcmp(key, "own_stream")) {
    if (value < 0 || value > 2) return fail(c, PISLAM_ERR_INVALID, "own_stream must be 0, 1 (default flags) or 2 (non-blocking)");
    return use_own_stream(c, value);
  }
  if (!strcmp(key, "frame_rearm")) {  // 1: take the one-launch paths again after a reported timeout (tests)
    if (value) c->frame_disabled = c->chain_disabled = false;
    return PISLAM_OK;
  }
  const char *refusal = nullptr;
  if (!fp::set_option(c->opt, key, value, &refusal)) refusal = "unknown option";
  return refusal ? fail(c, PISLAM_ERR_INVALID, refusal) : PISLAM_OK;
}

PISLAM_EXPORT int pislam_ctx_synchronize(pislam_ctx *c) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(sync(c));
  return check_frame_poison(c);
}

PISLAM_EXPORT const char *pislam_last_error(const pislam_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

PISLAM_EXPORT const int8_t *pislam_brief_table(void) {
  static int8_t tab[30 * 256 * 4];
  static bool ready = false;
  if (!ready) {
    for (int i = 0; i < 30 * 256; i++)
      for (int k = 0; k < 4; k++) tab[i * 4 + k] = (int8_t)((h_brief_tab_packed[i] >> (8 * k)) & 0xff);
    ready = true;
  }
  return tab;
}

PISLAM_EXPORT size_t pislam_centroids_size(size_t n) { return (2 * n + 7) & ~(size_t)7; }

// ===========================================================================
// the four reference entry points
// ===========================================================================
PISLAM_EXPORT int pislam_fast_detect(pislam_ctx *c, int vstep, int border, int width, int height,
                                     const uint8_t *img, uint8_t *out, int threshold) {
  PCHK(check_level_args(c, vstep, border, width, height, 3));
  if (!img || !out) return fail(c, PISLAM_ERR_INVALID, "null image");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)height * vstep;
  // The over-classified columns [width-border, xend) may run past vstep, i.e. into the next row (flat
  // addressing, as the reference's 16-byte vectors do): with a small border the ring of the last
  // classified row then reaches a few bytes beyond height*vstep — bytes the reference reads too.
  size_t img_bytes = bytes;
  if (height > 2 * border && width > 2 * border) {
    const size_t xend = (size_t)border + 16 * (size_t)cdiv(width - 2 * border, 16);
    img_bytes = std::max(bytes, (size_t)(height - border + 2) * vstep + xend + 3);
  }
  Staged si, so;
  PCHK(stage_in(c, c->s_img, img, img_bytes, &si));
  PCHK(stage_in(c, c->s_out, out, bytes, &so));
  PCHK(launch_detect(c, (const uint8_t *)si.dev, (uint8_t *)so.dev, vstep, 0, 1, border, width, height,
                     threshold));
  PCHK(stage_out(c, so, out, bytes));
  if (si.host || so.host) PCHK(sync(c));
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_fast_score_harris(pislam_ctx *c, int vstep, int border, int width, int height,
                                           const uint8_t *img, int32_t threshold, uint8_t *out) {
  PCHK(check_level_args(c, vstep, border, width, height, 4));
  if (!img || !out) return fail(c, PISLAM_ERR_INVALID, "null image");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)height * vstep;
  Staged si, so;
  PCHK(stage_in(c, c->s_img, img, bytes, &si));
  PCHK(stage_in(c, c->s_out, out, bytes, &so));
  PCHK(launch_harris(c, (const uint8_t *)si.dev, (uint8_t *)so.dev, vstep, 0, 1, border, width, height,
                     threshold));
  PCHK(stage_out(c, so, out, bytes));
  if (si.host || so.host) PCHK(sync(c));
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_fast_extract(pislam_ctx *c, int vstep, int border, int lbs, int limit, int width,
                                      int height, const uint8_t *out, uint32_t *results, size_t capacity,
                                      size_t *count) {
  PCHK(check_level_args(c, vstep, border, width, height, 1));
  if (!out || !count || (!results && capacity)) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  if (lbs < 0 || lbs > 8 || limit < 1 || limit > 64)
    return fail(c, PISLAM_ERR_INVALID, "logBucketSize must be 0..8 and bucketLimit 1..64");
  if (width > 4096 || height > 4096)
    return fail(c, PISLAM_ERR_INVALID, "encodeFast holds 12-bit coordinates (Util.h:27-29)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)height * vstep;
  Staged so, sr;
  PCHK(stage_in(c, c->s_out, out, bytes, &so));
  PCHK(stage_in(c, c->s_pts, results, capacity * sizeof(uint32_t), &sr, /*copy=*/false));
  if (c->w_total.ensure(sizeof(uint32_t)) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc");
  HIPCHK(c, hipMemsetAsync(c->w_total.p, 0, sizeof(uint32_t), c->stream));
  const uint32_t cap32 = (uint32_t)std::min<size_t>(capacity, 0xffffffffu);
  PCHK(launch_extract(c, (const uint8_t *)so.dev, vstep, 0, 1, border, lbs, limit, width, height,
                      (uint32_t *)sr.dev, 0, cap32, 0u, c->w_total.as<uint32_t>()));
  uint32_t n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, c->w_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  PCHK(sync(c));
  *count = n;
  PCHK(stage_out(c, sr, results, std::min<size_t>(n, capacity) * sizeof(uint32_t)));
  if (sr.host) PCHK(sync(c));
  return PISLAM_OK;
}

namespace {
int orb_common(pislam_ctx *c, int mode, int vstep, int words, const uint8_t *img, const uint32_t *points,
               const uint8_t *rots, size_t n, uint32_t *descriptors, int32_t *centroids) {
  if (!c) return PISLAM_ERR_INVALID;
  if (vstep <= 0) return fail(c, PISLAM_ERR_INVALID, "bad vstep");
  if (mode != 1 && (words < 1 || words > 8)) return fail(c, PISLAM_ERR_INVALID, "words must be 1..8");
  HIPCHK(c, hipSetDevice(c->device));
  if (mode == 1) {
    const size_t n8 = pislam_centroids_size(n);
    Staged sc;
    PCHK(stage_in(c, c->s_misc, centroids, n8 * sizeof(int32_t), &sc, false));
    if (n8) HIPCHK(c, hipMemsetAsync(sc.dev, 0, n8 * sizeof(int32_t), c->stream));
    if (n) {
      if (!img || !points) return fail(c, PISLAM_ERR_INVALID, "null pointer");
      const uint8_t *d_img;
      const uint32_t *d_pts;
      PCHK(stage_points_image(c, vstep, img, points, n, &d_img, &d_pts));
      hipLaunchKernelGGL(pk::k_orb<1>, dim3(cdiv((int)n, 4)), dim3(256), 0, c->stream, d_img, vstep,
                         (size_t)0, d_pts, (size_t)0, (const uint32_t *)nullptr, (uint32_t)n,
                         (uint32_t)n, 0, (uint32_t *)nullptr, (size_t)0, (int32_t *)sc.dev,
                         (const uint8_t *)nullptr);
      PCHK(launch_ok(c, "k_orb<centroids>"));
    }
    PCHK(stage_out(c, sc, centroids, n8 * sizeof(int32_t)));
    return sync(c);
  }
  if (n == 0) return PISLAM_OK;
  if (!img || !points || !descriptors) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  const uint8_t *d_img;
  const uint32_t *d_pts;
  PCHK(stage_points_image(c, vstep, img, points, n, &d_img, &d_pts));
  Staged sd, sr;
  PCHK(stage_in(c, c->s_desc, descriptors, n * words * sizeof(uint32_t), &sd, false));
  const uint8_t *d_rots = nullptr;
  if (mode == 2) {
    PCHK(stage_in(c, c->s_rots, rots, n, &sr));
    d_rots = (const uint8_t *)sr.dev;
    // rotations outside 0..29 leave the descriptor untouched (Brief.h switch): preserve caller bytes
    if (sd.host)
      HIPCHK(c, hipMemcpyAsync(sd.dev, descriptors, n * words * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream));
    hipLaunchKernelGGL(pk::k_orb<2>, dim3(cdiv((int)n, 4)), dim3(256), 0, c->stream, d_img, vstep,
                       (size_t)0, d_pts, (size_t)0, (const uint32_t *)nullptr, (uint32_t)n, (uint32_t)n,
                       words, (uint32_t *)sd.dev, (size_t)0, (int32_t *)nullptr, d_rots);
  } else {
    hipLaunchKernelGGL(pk::k_orb<0>, dim3(cdiv((int)n, 4)), dim3(256), 0, c->stream, d_img, vstep,
                       (size_t)0, d_pts, (size_t)0, (const uint32_t *)nullptr, (uint32_t)n, (uint32_t)n,
                       words, (uint32_t *)sd.dev, (size_t)0, (int32_t *)nullptr,
                       (const uint8_t *)nullptr);
  }
  PCHK(launch_ok(c, "k_orb"));
  PCHK(stage_out(c, sd, descriptors, n * words * sizeof(uint32_t)));
  return sync(c);
}
}  // namespace

PISLAM_EXPORT int pislam_orb_compute(pislam_ctx *c, int vstep, int words, const uint8_t *img,
                                     const uint32_t *points, size_t n, uint32_t *descriptors) {
  return orb_common(c, 0, vstep, words, img, points, nullptr, n, descriptors, nullptr);
}

PISLAM_EXPORT int pislam_orb_centroids(pislam_ctx *c, int vstep, const uint8_t *img, const uint32_t *points,
                                       size_t n, int32_t *centroids) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!centroids && n) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  return orb_common(c, 1, vstep, 0, img, points, nullptr, n, nullptr, centroids);
}

PISLAM_EXPORT int pislam_brief_describe(pislam_ctx *c, int vstep, int words, const uint8_t *img,
                                        const uint32_t *points, const uint8_t *rots, size_t n,
                                        uint32_t *descriptors) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!rots && n) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  return orb_common(c, 2, vstep, words, img, points, rots, n, descriptors, nullptr);
}

PISLAM_EXPORT int pislam_orb_angles(pislam_ctx *c, const int32_t *centroids, size_t n8, uint8_t *angles) {
  if (!c) return PISLAM_ERR_INVALID;
  if (n8 % 8) return fail(c, PISLAM_ERR_INVALID, "n8 must be a multiple of 8 (Orb.h:314)");
  if (n8 == 0) return PISLAM_OK;
  if (!centroids || !angles) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  Staged sc, sa;
  PCHK(stage_in(c, c->s_misc, centroids, n8 * sizeof(int32_t), &sc));
  PCHK(stage_in(c, c->s_rots, angles, n8 / 2, &sa, false));
  hipLaunchKernelGGL(pk::k_angles, dim3(cdiv((int)(n8 / 2), 256)), dim3(256), 0, c->stream,
                     (const int32_t *)sc.dev, (int)(n8 / 2), (uint8_t *)sa.dev);
  PCHK(launch_ok(c, "k_angles"));
  PCHK(stage_out(c, sa, angles, n8 / 2));
  return sync(c);
}

PISLAM_EXPORT int pislam_harris_score_points(pislam_ctx *c, int vstep, const uint8_t *img,
                                             const uint32_t *points, size_t n, int32_t threshold,
                                             uint8_t *scores) {
  if (!c) return PISLAM_ERR_INVALID;
  if (n == 0) return PISLAM_OK;
  if (!img || !points || !scores || vstep <= 0) return fail(c, PISLAM_ERR_INVALID, "bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  const uint8_t *d_img;
  const uint32_t *d_pts;
  PCHK(stage_points_image(c, vstep, img, points, n, &d_img, &d_pts, 3, 4, 4));   // Harris.h:102-110
  Staged ss;
  PCHK(stage_in(c, c->s_rots, scores, n, &ss, false));
  hipLaunchKernelGGL(pk::k_harris_points, dim3(cdiv((int)n, 256)), dim3(256), 0, c->stream, d_img, vstep,
                     d_pts, (int)n, threshold, (uint8_t *)ss.dev);
  PCHK(launch_ok(c, "k_harris_points"));
  PCHK(stage_out(c, ss, scores, n));
  return sync(c);
}



namespace {
// launch bilinear N/M for `batch` images; quad: the fast 4-block kernel (pp::quad_kernel_applies)
template <int N, int M>
int launch_bilinear(pislam_ctx *c, const uint8_t *src, uint8_t *dst, int vstep_src, int vstep_dst, size_t stride_src,
                    size_t stride_dst, int batch, int width, int height, bool quad) {
  const int nbx = cdiv(width, N), nby = cdiv(height, N);
  if (quad)
    hipLaunchKernelGGL((pp::k_bilinear4<N, M>), dim3(cdiv(cdiv(nbx, 4) * nby * M, 256), 1, batch), dim3(256), 0,
                       c->stream, src, dst, vstep_src, vstep_dst, stride_src, stride_dst, width, height);
  else
    hipLaunchKernelGGL((pp::k_bilinear<N, M>), dim3(cdiv(nbx * M, 256), cdiv(nby * M, 4), batch), dim3(256), 0, c->stream,
                       src, dst, vstep_src, vstep_dst, stride_src, stride_dst, width, height);
  return launch_ok(c, "k_bilinear");
}
}  // namespace

// ===========================================================================
// image preparation ("next" tier): gaussian5x5, bilinear7_8, bilinear13_16
// ===========================================================================
namespace {
// kind 0 = gaussian5x5, 1 = bilinear7_8, 2 = bilinear13_16
int prep_common(pislam_ctx *c, int kind, int vstep, int width, int height, const uint8_t *img, uint8_t *out) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!img || !out) return fail(c, PISLAM_ERR_INVALID, "null image");
  if (vstep <= 0 || width <= 0 || height <= 0) return fail(c, PISLAM_ERR_INVALID, "bad vstep/width/height");
  const pp::Reduction r = kind == 0 ? pp::Reduction{1, 1} : pp::reduction(kind);
  const int wpad = r.padded(width), hpad = r.padded(height);
  if (wpad > vstep) return fail(c, PISLAM_ERR_INVALID, "width (padded to the block size) exceeds vstep");
  if (kind == 0 && (width < 3 || height < 3)) return fail(c, PISLAM_ERR_INVALID, "gaussian5x5 needs at least 3x3");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t in_bytes = (size_t)hpad * vstep;
  const size_t out_rows = (size_t)r.written(height);
  const size_t out_bytes = out_rows * vstep;
  Staged si, so;
  PCHK(stage_in(c, c->s_img, img, in_bytes, &si));
  const bool inplace = img == out;
  const uint8_t *d_src = (const uint8_t *)si.dev;
  uint8_t *d_dst;
  if (inplace) {
    // results are a pure function of the ORIGINAL image (as the reference's in-place loops are):
    // run from a private copy of the source
    if (c->s_tmp.ensure(in_bytes) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(prep temp)");
    HIPCHK(c, hipMemcpyAsync(c->s_tmp.p, d_src, in_bytes, hipMemcpyDeviceToDevice, c->stream));
    d_src = c->s_tmp.as<uint8_t>();
    d_dst = (uint8_t *)si.dev;
    so = si;
  } else {
    PCHK(stage_in(c, c->s_out, out, std::max(out_bytes, (size_t)1), &so));   // keep untouched bytes
    d_dst = (uint8_t *)so.dev;
  }
  if (kind == 0) {
    dim3 grid(cdiv(width, pp::G_TW), cdiv(height, pp::G_TH), 1);
    hipLaunchKernelGGL(pp::k_gaussian5x5, grid, dim3(256), 0, c->stream, d_src, d_dst, vstep, vstep, (size_t)0,
                       (size_t)0, width, height);
    PCHK(launch_ok(c, "k_gaussian5x5"));
  } else {
    const bool quad = pp::quad_kernel_applies((unsigned)((uintptr_t)d_src % 16), (unsigned)((uintptr_t)d_dst % 16), vstep, vstep, 0, 0,
                                              r.blocks(width), r.N);
    if (kind == 1) PCHK((launch_bilinear<8, 7>(c, d_src, d_dst, vstep, vstep, 0, 0, 1, width, height, quad)));
    else PCHK((launch_bilinear<16, 13>(c, d_src, d_dst, vstep, vstep, 0, 0, 1, width, height, quad)));
  }
  if (so.host) {
    PCHK(stage_out(c, so, out, out_bytes));   // rows the kernels can have written
    PCHK(sync(c));
  } else if (si.host) {
    PCHK(sync(c));
  }
  return PISLAM_OK;
}
}  // namespace

PISLAM_EXPORT int pislam_gaussian5x5(pislam_ctx *c, int vstep, int width, int height, const uint8_t *img,
                                     uint8_t *out) {
  return prep_common(c, 0, vstep, width, height, img, out);
}
PISLAM_EXPORT int pislam_bilinear7_8(pislam_ctx *c, int vstep, int width, int height, const uint8_t *img,
                                     uint8_t *out) {
  return prep_common(c, 1, vstep, width, height, img, out);
}
PISLAM_EXPORT int pislam_bilinear13_16(pislam_ctx *c, int vstep, int width, int height, const uint8_t *img,
                                       uint8_t *out) {
  return prep_common(c, 2, vstep, width, height, img, out);
}


// ---------------------------------------------------------------------------
// on-GPU pyramid build (BASELINE config 5): frame -> gaussian5x5 -> level 0, then a chain of
// bilinear7_8 / bilinear13_16 reductions, every level written into a vertically stacked pyramid.
// ---------------------------------------------------------------------------
PISLAM_EXPORT int pislam_pyramid_layout(int width, int height, int nlevels, const int32_t *steps, int vstep_min,
                                        pislam_level *levels, int32_t *vstep, int32_t *rows) {
  return pp::layout(width, height, nlevels, steps, vstep_min, levels, vstep, rows);
}

// The steps of pislam_pyramid_build_batch, in launch order.  What each launches is decided by pp::make_build_plan.
namespace {
// Padding bytes are read by the bilinear steps (block padding) and by FAST's right-edge columns: they are
// defined as zero.  Every build rewrites the same rectangle of each level's slot and zeroes the margins
// around it that those consumers read (pp::k_zero_margins) — on EVERY call: a caller may have scribbled over
// the buffer, or the allocator may hand out a recycled address — unless the caller vouches for them
// (PISLAM_BUILD_MARGINS_CLEAN: a buffer this function filled before with the same layout and nobody wrote
// to since; the margin pass costs ~20 us per 64 720p frames).  Bytes beyond the margins are nobody's input
// and are left untouched (zero-initialise the buffer once if they must be defined).
int build_margins(pislam_ctx *c, const pp::ZeroPlan &Z, int batch, uint8_t *pyramids, size_t pyramid_stride, bool check) {
  if (check) {
    // debug: verify the caller's promise instead of trusting it (synchronises; a dirty margin is an error)
    if (c->w_total.ensure(sizeof(uint32_t)) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc");
    HIPCHK(c, hipMemsetAsync(c->w_total.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(pp::k_zero_margins<true>, dim3(2 * Z.nlevels, batch), dim3(256), 0, c->stream, Z, pyramids,
                       pyramid_stride, c->w_total.as<unsigned int>());
    PCHK(launch_ok(c, "k_zero_margins<check>"));
    uint32_t nz = 0;
    HIPCHK(c, hipMemcpyAsync(&nz, c->w_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    PCHK(sync(c));
    if (nz) return fail(c, PISLAM_ERR_INVALID, "PISLAM_BUILD_MARGINS_CLEAN was passed but the margins hold non-zero bytes");
    return PISLAM_OK;
  }
  hipLaunchKernelGGL(pp::k_zero_margins<false>, dim3(2 * Z.nlevels, batch), dim3(256), 0, c->stream, Z, pyramids,
                     pyramid_stride, (unsigned int *)nullptr);
  return launch_ok(c, "k_zero_margins");
}

// level 0 = gaussian5x5 of the frame, or the frame itself
int build_level0(pislam_ctx *c, const pislam_level &lv, const uint8_t *frames, int frame_vstep, size_t frame_stride, int batch,
                 uint8_t *pyramids, int vstep, size_t pyramid_stride, bool blur) {
  const int w0 = lv.width, h0 = lv.height;
  uint8_t *dst = pyramids + (size_t)lv.row0 * vstep;
  if (blur) {
    hipLaunchKernelGGL(pp::k_gaussian5x5, dim3(cdiv(w0, pp::G_TW), cdiv(h0, pp::G_TH), batch), dim3(256), 0, c->stream,
                       frames, dst, frame_vstep, vstep, frame_stride, pyramid_stride, w0, h0);
    return launch_ok(c, "k_gaussian5x5");
  }
  for (int b = 0; b < batch; b++)
    HIPCHK(c, hipMemcpy2DAsync(dst + b * pyramid_stride, vstep, frames + b * frame_stride, frame_vstep, w0, h0,
                               hipMemcpyDeviceToDevice, c->stream));
  return PISLAM_OK;
}

// (Fusing two chained reductions per launch — a 128-tile of level k maps onto whole blocks of 13/16 then 7/8,
//  level k+1 kept in LDS — was built and measured: 184 vs 167 us per 64 frames, 667 vs 584 us per 256.  The
//  64-frame pyramid set fits the 256 MiB Infinity Cache, so the re-read the fusion saves never reaches HBM,
//  and the LDS round trips cost more than k_bilinear4's register-only path.)
// (The small levels in ONE launch — one 1024-thread workgroup per pyramid walking levels 3 .. 7 through k_bilinear4's
//  work items, a device-scope fence + barrier between levels — was built in round 4, bit-exact, and measured: the step of
//  64 720p frames 0.375 -> 0.53 ms from level 3 on, 0.59 ms from level 2 on: 64 workgroups with a handful of dependent
//  load -> compute -> store round trips each are far slower than five launches that fill the chip, launch floors included.)
// Round 6: ALL reductions as one launch with a row-band hand-over between the levels (pp::k_bilinear_chain) — the same
// work items as the per-level launches, every workgroup starting as soon as the source rows it reads are complete.
int build_reductions(pislam_ctx *c, const pp::BuildPlan &P, int nlevels, int batch, uint8_t *pyramids, int vstep,
                     size_t pyramid_stride) {
  if (P.chain) {
    bool grew = false;
    if (c->w_chain.ensure(sizeof(uint32_t) * P.chain_words, &grew) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(build chain counters)");
    if (grew || c->chain_words != P.chain_words) {
      // (a different layout puts [done, fault] elsewhere: start from zeros — stream order puts this behind any launch in flight)
      HIPCHK(c, hipMemsetAsync(c->w_chain.p, 0, c->w_chain.cap, c->stream));
      if (!grew && c->chain_words != 0) c->ovf_layouts++;   // (a captured build holds the old layout: workspace_generation)
      c->chain_words = P.chain_words;
    }
    PCHK(ensure_fault_flag(c));
    hipLaunchKernelGGL(pp::k_bilinear_chain, dim3(P.chain_grid), dim3(256), 0, c->stream, P.C, pyramids, pyramid_stride,
                       c->w_chain.as<uint32_t>(), c->frame_flag_dev + 1, (uint32_t)c->opt.frame_test);
    return launch_ok(c, "k_bilinear_chain");
  }
  for (int l = 0; l + 1 < nlevels; l++) {
    const pp::ReductionPlan &R = P.red[l];
    const uint8_t *src = pyramids + R.src_ofs;
    uint8_t *dst = pyramids + R.dst_ofs;
    if (R.step == 1)
      PCHK((launch_bilinear<8, 7>(c, src, dst, vstep, vstep, pyramid_stride, pyramid_stride, batch, R.width, R.height, R.quad)));
    else
      PCHK((launch_bilinear<16, 13>(c, src, dst, vstep, vstep, pyramid_stride, pyramid_stride, batch, R.width, R.height, R.quad)));
  }
  return PISLAM_OK;
}
}  // namespace

PISLAM_EXPORT int pislam_pyramid_build_batch(pislam_ctx *c, int nlevels, const int32_t *steps,
                                             const pislam_level *levels, const uint8_t *frames, int frame_vstep,
                                             size_t frame_stride, int batch, uint8_t *pyramids, int vstep,
                                             int rows, size_t pyramid_stride, int flags) {
  if (!c) return PISLAM_ERR_INVALID;
  if (const char *bad = pp::check_build_call(nlevels, steps, levels, frames, pyramids, batch, flags))
    return fail(c, PISLAM_ERR_INVALID, bad);
  if (!is_device_ptr(frames) || !is_device_ptr(pyramids)) return fail(c, PISLAM_ERR_INVALID, pp::HOST_POINTERS);
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(check_frame_poison(c));
  const pp::BuildPlan P = pp::make_build_plan(nlevels, steps, levels, frame_vstep, frame_stride, batch, vstep, rows, pyramid_stride,
                                              flags, (unsigned)((uintptr_t)pyramids % 16), c->opt.build_chain && !c->chain_disabled);
  if (P.refusal) return fail(c, PISLAM_ERR_INVALID, P.refusal);
  if (P.margins)
    PCHK(build_margins(c, P.Z, batch, pyramids, pyramid_stride, (flags & PISLAM_BUILD_MARGINS_CLEAN) != 0));
  PCHK(build_level0(c, levels[0], frames, frame_vstep, frame_stride, batch, pyramids, vstep, pyramid_stride,
                    (flags & PISLAM_BUILD_BLUR) != 0));
  return build_reductions(c, P, nlevels, batch, pyramids, vstep, pyramid_stride);
}

// ===========================================================================
// batch pipeline (staged: one launch group per level, blockIdx.z = pyramid)
// ===========================================================================
namespace {
int check_params(pislam_ctx *c, const pislam_frontend_params *p, const pislam_level *lv, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  const char *refusal = fp::check_params(p, lv, batch);
  return refusal ? fail(c, PISLAM_ERR_INVALID, refusal) : PISLAM_OK;
}

// Overflow lists: one per sub-batch ([0] count, [1] count of the previous step, [2..] entries), `stride` dwords
// apart.  A new layout (or a new allocation) starts from an all-zero buffer: a stale entry must never be read
// as a list header.
int prepare_ovf(pislam_ctx *c, int nsub, size_t stride) {
  bool grew = false;
  if (c->w_ovf.ensure(sizeof(uint32_t) * stride * nsub, &grew) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(overflow list)");
  // (one list: its header is at offset 0 whatever the stride — calls of different batch sizes share the layout)
  const size_t lay = nsub == 1 ? 0 : stride;
  if (grew || c->ovf_nsub != nsub || c->ovf_stride != lay) {
    HIPCHK(c, hipMemsetAsync(c->w_ovf.p, 0, c->w_ovf.cap, c->stream));
    c->ovf_nsub = nsub;
    c->ovf_stride = lay;
    c->ovf_layouts++;
  }
  return PISLAM_OK;
}

int ensure_aux(pislam_ctx *c, int nsub) {
  if (!c->aux_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
  if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  for (int i = 0; i < nsub; i++)
    if (!c->ev_sub[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_sub[i], hipEventDisableTiming));
  return PISLAM_OK;
}


// The device copy of a host-built plan table: found by content, or created (hipMalloc + upload in stream order — never
// inside a capture: the first occurrence of a call runs eagerly, and reserve_frontend uploads the tables).
int plan_table(pislam_ctx *c, const std::vector<uint32_t> &t, const uint32_t **out) {
  for (size_t i = 0; i < c->plan_tables.size(); i++)
    if (c->plan_tables[i]->host == t) {
      std::rotate(c->plan_tables.begin() + i, c->plan_tables.begin() + i + 1, c->plan_tables.end());   // most recently used last, the others keep their order
      *out = c->plan_tables.back()->dev.as<uint32_t>();
      return PISLAM_OK;
    }
  if (c->plan_tables.size() >= 64) {                  // evict the least recently used (a table is a few KB)
    HIPCHK(c, hipStreamSynchronize(c->stream));       // (a launch in flight may still read it)
    c->plan_tables.front()->dev.release();
    delete c->plan_tables.front();
    c->plan_tables.erase(c->plan_tables.begin());
    c->table_uploads++;
  }
  pislam_ctx::PlanTable *pt = new pislam_ctx::PlanTable();
  pt->host = t;
  if (pt->dev.ensure(sizeof(uint32_t) * pt->host.size()) != PISLAM_OK) {
    delete pt;
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(plan table)");
  }
  c->plan_tables.push_back(pt);
  HIPCHK(c, hipMemcpyAsync(pt->dev.p, pt->host.data(), sizeof(uint32_t) * pt->host.size(), hipMemcpyHostToDevice, c->stream));
  *out = pt->dev.as<uint32_t>();
  return PISLAM_OK;
}

int ensure_frame_sync(pislam_ctx *c) {
  bool grew = false;
  if (c->w_sync.ensure(sizeof(uint32_t) * pf::FRAME_SYNC_WORDS, &grew) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(frame sync)");
  if (grew) HIPCHK(c, hipMemsetAsync(c->w_sync.p, 0, c->w_sync.cap, c->stream));   // (the kernel re-arms them itself)
  return ensure_fault_flag(c);
}

// The plan of a batch call (parameters checked): fp::plan_frontend from the context's options.
int plan_frontend(pislam_ctx *c, const pislam_frontend_params *p, const pislam_level *lv, int batch, FrontendPlan *P) {
  const char *refusal = fp::plan_frontend(c->opt, p, lv, batch, P);
  return refusal ? fail(c, PISLAM_ERR_INVALID, refusal) : PISLAM_OK;
}

// The workspace of plan P: the only place the front end's buffers are allocated (option "ablate" 8192's profiling aside).
int reserve_frontend(pislam_ctx *c, const pislam_frontend_params *p, const pislam_level *lv, const FrontendPlan &P, int batch) {
  const size_t pyr_bytes = (size_t)p->rows * p->vstep;
  bool grew = false;
  if (c->w_score.ensure(pyr_bytes * batch, &grew) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(score map)");
  const bool same_shape = !grew && c->last_batch >= batch && c->last_params.vstep == p->vstep &&
                          c->last_params.rows == p->rows && c->last_params.nlevels == p->nlevels &&
                          c->last_params.border == p->border && (int)c->last_levels.size() == p->nlevels &&
                          memcmp(c->last_levels.data(), lv, sizeof(pislam_level) * p->nlevels) == 0;
  if (!same_shape) {
    // Fast.h:42-44: `out` must start as zeros; afterwards the regions fastDetect rewrites are the
    // only ones that ever change, so the zeroing is needed once per shape.
    HIPCHK(c, hipMemsetAsync(c->w_score.p, 0, pyr_bytes * batch, c->stream));
    c->last_params = *p;
    c->last_levels.assign(lv, lv + p->nlevels);
    c->last_batch = batch;
  }
  size_t maxn = 1;
  for (int l = 0; l < p->nlevels; l++) {
    const int ny = lv[l].height - 2 * p->border, nx = lv[l].width - 2 * p->border;
    if (ny <= 0 || nx <= 0) continue;
    const int bs = 1 << p->log_bucket_size;
    maxn = std::max<size_t>(maxn, p->log_bucket_size == 0 ? (size_t)cdiv(ny, 2) : (size_t)((nx - 1) / bs + 1) * ((ny - 1) / bs + 1));
  }
  if (c->w_cnt.ensure(sizeof(uint32_t) * maxn * batch) != PISLAM_OK ||
      c->w_off.ensure(sizeof(uint32_t) * maxn * batch) != PISLAM_OK ||
      (p->log_bucket_size &&
       c->w_cellkp.ensure(sizeof(uint32_t) * maxn * batch * p->bucket_limit) != PISLAM_OK))
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(extract scratch)");
  if (!P.fused || P.F.strips_per_pyr == 0) return PISLAM_OK;
  // (+ 64 dwords: pf::k_bucket_select requests the first 64 slots of a strip's list whatever its count)
  if (c->w_stage.ensure(sizeof(uint32_t) * ((size_t)P.F.slots_per_pyr * batch + 64)) != PISLAM_OK ||
      c->w_stripcnt.ensure(sizeof(uint32_t) * (size_t)P.F.strips_per_pyr * batch) != PISLAM_OK ||
      c->w_stagedesc.ensure(sizeof(uint32_t) * P.sdesc_per_pyr * batch) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(fused staging)");
  if (P.alias) PCHK(prepare_ovf(c, P.nsub, P.ovf_stride));
  if (P.nsub > 1) PCHK(ensure_aux(c, P.nsub));
  if (batch <= frame_max_batch(c->opt)) PCHK(ensure_frame_sync(c));
  if (P.sel) {
    if (c->w_ustage.ensure(sizeof(uint32_t) * (size_t)P.Q.uslots_per_pyr * batch) != PISLAM_OK ||
        c->w_ucount.ensure(sizeof(uint32_t) * (size_t)P.Q.units_per_pyr * batch) != PISLAM_OK)
      return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(bucket selection staging)");
    PCHK(plan_table(c, P.utab, &c->cur_utab));
  }
  return PISLAM_OK;
}

// A kernel that asks for more dynamic LDS than LDS_OPT_IN has its limit raised first.
#define RAISE_LDS_LIMIT(c, kern, bytes)                                                                                \
  do {                                                                                                                 \
    if ((bytes) > LDS_OPT_IN)                                                                                          \
      HIPCHK(c, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));      \
  } while (0)

using StripKernT = void (*)(const pf::FusedParams, const uint8_t *, size_t, uint32_t *, uint32_t *, uint8_t *, size_t,
                            unsigned long long *, uint32_t *, uint32_t *);
using OvfKernT = void (*)(const pf::FusedParams, const uint8_t *, size_t, uint32_t *, uint32_t *, uint8_t *, size_t, const uint32_t *);

// The kernels a fused call runs.  vec: 16-byte aligned rows; hooks: score-map dump (debug / parity hook) or a profiling ablation.
StripKernT strip_kernel(bool vec, bool alias, bool hooks, bool orb_in_strip, int lbs) {
  static const StripKernT kerns[8] = {
      pf::k_fused_strips<false, false, false>, pf::k_fused_strips<false, false, true>,
      pf::k_fused_strips<false, true, false>,  pf::k_fused_strips<false, true, true>,
      pf::k_fused_strips<true, false, false>,  pf::k_fused_strips<true, false, true>,
      pf::k_fused_strips<true, true, false>,   pf::k_fused_strips<true, true, true>};
  // strips describing their own keypoints (option "orb_in_strip"): separate instantiations of the aligned ALIAS kernels
  static const StripKernT kerns_orb[2] = {pf::k_fused_strips<true, false, true, true>, pf::k_fused_strips<true, true, true, true>};
  // the default mode's kernels (aligned ALIAS layout, no buckets, gather+ORB describes): compiled without the bucket code
  static const StripKernT kerns_nb[2] = {pf::k_fused_strips<true, false, true, false, false>,
                                         pf::k_fused_strips<true, true, true, false, false>};
  return (orb_in_strip && vec && alias) ? kerns_orb[hooks ? 1 : 0]
         : (vec && alias && lbs == 0)   ? kerns_nb[hooks ? 1 : 0]
                                        : kerns[(vec ? 4 : 0) | (hooks ? 2 : 0) | (alias ? 1 : 0)];
}
OvfKernT overflow_kernel(bool vec, bool hooks) {
  static const OvfKernT okerns[4] = {pf::k_fused_overflow<false, false>, pf::k_fused_overflow<false, true>,
                                     pf::k_fused_overflow<true, false>, pf::k_fused_overflow<true, true>};
  return okerns[(vec ? 2 : 0) | (hooks ? 1 : 0)];
}
// (the profiling instantiation exists for the gather's per-phase counters: option "ablate" bits 20..23, pf::orb_describe)
auto gather_orb_kernel(int ablate) { return (ablate >> 20) & 15 ? pf::k_gather_orb<true> : pf::k_gather_orb<false>; }

// Per-keypoint ORB over n pyramids (pk::k_orb<0>, blockIdx.z = pyramid): the staged pipeline's last launch, and the fused
// pipeline's where k_gather_orb does not take the layout.
int launch_orb_batch(pislam_ctx *c, hipStream_t stream, const pislam_frontend_params *p, const uint8_t *pyramids, size_t stride,
                     int n, const uint32_t *kp, const uint32_t *counts, uint32_t *desc) {
  hipLaunchKernelGGL(pk::k_orb<0>, dim3(cdiv(p->max_keypoints, 4), 1, n), dim3(256), 0, stream, pyramids, p->vstep, stride, kp,
                     (size_t)p->max_keypoints, counts, 0u, (uint32_t)p->max_keypoints, p->words, desc,
                     (size_t)p->max_keypoints * p->words, (int32_t *)nullptr, (const uint8_t *)nullptr);
  return launch_ok(c, "k_orb<batch>");
}

// Profiling hook (option "ablate" 8192): the strip kernel's per-phase workgroup cycles, 8 counters per workgroup -> stderr.
int report_strip_profile(pislam_ctx *c, const unsigned long long *prof, size_t prof_n, hipStream_t M, double ns, unsigned workgroups) {
  std::vector<unsigned long long> hv(prof_n);
  HIPCHK(c, hipMemcpyAsync(hv.data(), prof, prof_n * sizeof(unsigned long long), hipMemcpyDeviceToHost, M));
  HIPCHK(c, hipStreamSynchronize(M));
  double h[8] = {0};
  unsigned long long why[3] = {0, 0, 0};
  for (size_t i = 0; i < prof_n; i++) {
    if ((i & 7) == 5) {
      why[0] += hv[i] & 0xfffff;
      why[1] += (hv[i] >> 20) & 0xfffff;
      why[2] += hv[i] >> 40;
    } else {
      h[i & 7] += (double)hv[i];
    }
  }
  fprintf(stderr, "[pislam prof] deferred strips by reason: corner queue %llu, score queue %llu, survivor buffer %llu\n",
          why[0], why[1], why[2]);
  fprintf(stderr, "[pislam prof] cycles/strip: stage %.0f classify %.0f harris %.0f nms %.0f emit %.0f "
                  "(strips %.0f, carried %.0f, workgroups %u, lifetime %.0f/strip)\n",
          h[0] / ns, h[1] / ns, h[2] / ns, h[3] / ns, h[4] / ns, ns, h[6], workgroups, h[7] / ns);
  return PISLAM_OK;
}

// What the launches of one fused call share: the call's arguments, the kernels chosen for it and its two streams.
struct FusedCall {
  const pislam_frontend_params *p;
  const FrontendPlan &P;
  const uint8_t *pyramids;
  size_t stride;
  int batch;
  uint32_t *kp, *desc, *counts;
  StripKernT kern;
  OvfKernT okern;
  decltype(gather_orb_kernel(0)) gkern;
  bool fork;          // sub-batches fork: an eager call with more than one
  hipStream_t M, X;   // the context stream (strips), and where the rest of a sub-batch runs: M, or the aux stream of a fork
};

// ---- small batches: strips -> (overflowed strips redone in place) -> gather + ORB as ONE launch ----
int launch_frame(pislam_ctx *c, const FusedCall &k) {
  const pislam_frontend_params *p = k.p;
  const FrontendPlan &P = k.P;
  RAISE_LDS_LIMIT(c, pf::k_frame, P.flds);
  pf::FusedParams F = P.F;
  F.batch = k.batch;
  const unsigned grid = (unsigned)(k.batch * F.runs_per_pyr + k.batch * P.fch);
  hipLaunchKernelGGL(pf::k_frame, dim3(grid), dim3(pf::NT), P.flds, c->stream, F, k.pyramids, k.stride, c->w_stage.as<uint32_t>(),
                     c->w_stripcnt.as<uint32_t>(), k.kp, (size_t)p->max_keypoints, (uint32_t)p->max_keypoints, k.counts, k.desc,
                     (size_t)p->max_keypoints * p->words, p->words, (uint32_t)P.fper, P.fch, c->w_sync.as<uint32_t>(),
                     c->w_ovf.as<uint32_t>(), c->frame_flag_dev, (uint32_t)c->opt.frame_test);
  PCHK(launch_ok(c, "k_frame"));
  c->last_path = PISLAM_PATH_FUSED | PISLAM_PATH_ONE_LAUNCH;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));   // (one launch: the stage split of last_timing is all in stage 0)
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  return PISLAM_OK;
}

// Sub-batch `sub` of the call (the whole call where nsub == 1): strips on M; overflow pass, bucket selection and gather + ORB on X.
int launch_sub_batch(pislam_ctx *c, const FusedCall &k, int sub) {
  const pislam_frontend_params *p = k.p;
  const FrontendPlan &P = k.P;
  const int S = P.F.strips_per_pyr, nsub = P.nsub, base = k.batch / nsub, rem = k.batch % nsub;
  const int first = sub * base + std::min(sub, rem), n = base + (sub < rem ? 1 : 0);
  const hipStream_t M = k.M, X = k.X;
  pf::FusedParams F = P.F;
  F.batch = n;
  const size_t dump_stride = (size_t)p->rows * p->vstep;
  const uint8_t *s_pyr = k.pyramids + (size_t)first * k.stride;
  uint32_t *s_stage = c->w_stage.as<uint32_t>() + (size_t)first * F.slots_per_pyr;
  uint32_t *s_cnt = c->w_stripcnt.as<uint32_t>() + (size_t)first * S;
  uint32_t *s_sdesc = c->w_stagedesc.as<uint32_t>() + (size_t)first * P.sdesc_per_pyr;
  uint8_t *s_dump = F.dump_score ? c->w_score.as<uint8_t>() + (size_t)first * dump_stride : nullptr;
  uint32_t *s_kp = k.kp + (size_t)first * p->max_keypoints;
  uint32_t *s_desc = k.desc + (size_t)first * p->max_keypoints * p->words;
  uint32_t *s_counts = k.counts + first;
  uint32_t *ovf = P.alias ? c->w_ovf.as<uint32_t>() + (size_t)sub * P.ovf_stride : nullptr;
  const dim3 grid((unsigned)(cdiv(n, 8) * F.runs_per_pyr * 8));
  unsigned long long *prof = nullptr;
  const size_t prof_n = (size_t)grid.x * 8;
  if (F.ablate & 8192) {                         // profiling hook: per-phase workgroup cycles -> stderr
    if (c->w_prof.ensure(prof_n * sizeof(unsigned long long)) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(prof)");
    prof = c->w_prof.as<unsigned long long>();
    HIPCHK(c, hipMemsetAsync(prof, 0, prof_n * sizeof(unsigned long long), M));
  }
  // (profiling option "repeat_strips": the strip kernel launched n times back to back inside the stage-0
  //  event bracket, so that the per-launch duration is not inflated by the command-processor latency
  //  around a single eager launch; every launch rewrites the same outputs)
  for (int rep = 0; rep < std::max(1, c->opt.repeat_strips); rep++) {
    if (rep && ovf) HIPCHK(c, hipMemsetAsync(ovf, 0, sizeof(uint32_t), M));   // the last launch's list counts
    hipLaunchKernelGGL(k.kern, grid, dim3(pf::NT), P.klds, M, F, s_pyr, k.stride, s_stage, s_cnt, s_dump, dump_stride, prof, ovf,
                       s_sdesc);
  }
  if (prof) PCHK(report_strip_profile(c, prof, prof_n, M, (double)S * n, grid.x));
  PCHK(launch_ok(c, "k_fused_strips"));
  if (nsub > 1) {
    if (k.fork) {
      // fork: the rest of this sub-batch runs on the aux stream, under the next sub-batch's strip kernel
      HIPCHK(c, hipEventRecord(c->ev_sub[sub], M));
      HIPCHK(c, hipStreamWaitEvent(X, c->ev_sub[sub], 0));
    }
    if (sub == nsub - 1) {
      HIPCHK(c, hipEventRecord(c->ev[1], M));   // stage 0 = every sub-batch's strip kernel
      HIPCHK(c, hipEventRecord(c->ev[2], M));   // (stage 1, the overflow passes, runs on the aux stream)
    }
  } else {
    HIPCHK(c, hipEventRecord(c->ev[1], M));     // stage 0 = the strip kernel alone
  }
  if (P.alias) {
    hipLaunchKernelGGL(k.okern, dim3((unsigned)std::max(8, c->opt.num_cus / 2)), dim3(pf::NT), P.lds, X, F, s_pyr, k.stride, s_stage,
                       s_cnt, s_dump, dump_stride, (const uint32_t *)ovf);
    PCHK(launch_ok(c, "k_fused_overflow"));
  }
  if (nsub == 1) HIPCHK(c, hipEventRecord(c->ev[2], M));   // stage 1 = the overflow pass (normally empty)
  // the plan, lists and counts the gather runs on: the strips' own, or the units of the bucket selection pass
  pf::FusedParams G = F;
  const uint32_t *g_stage = s_stage, *g_cnt = s_cnt;
  if (P.sel) {
    uint32_t *u_stage = c->w_ustage.as<uint32_t>() + (size_t)first * P.Q.uslots_per_pyr;
    uint32_t *u_cnt = c->w_ucount.as<uint32_t>() + (size_t)first * P.Q.units_per_pyr;
    hipLaunchKernelGGL(pf::k_bucket_select, dim3(cdiv(P.Q.units_per_pyr, pf::SEL_WAVES), n), dim3(64 * pf::SEL_WAVES), P.sel_lds, X, F, P.Q,
                       (const uint32_t *)s_stage, (const uint32_t *)s_cnt, u_stage, u_cnt, c->cur_utab);
    PCHK(launch_ok(c, "k_bucket_select"));
    G = P.U;
    G.batch = n;
    g_stage = u_stage;
    g_cnt = u_cnt;
  }
  if (P.generic_orb) {
    c->last_path |= PISLAM_PATH_GENERIC_ORB;
    hipLaunchKernelGGL(pf::k_gather, dim3(n), dim3(256), P.glds, X, G, g_stage, g_cnt, s_kp,
                       (size_t)p->max_keypoints, (uint32_t)p->max_keypoints, s_counts, ovf);
    PCHK(launch_ok(c, "k_gather"));
    return launch_orb_batch(c, X, p, s_pyr, k.stride, n, s_kp, s_counts, s_desc);
  }
  hipLaunchKernelGGL(k.gkern, dim3(P.nch, n), dim3(256), P.olds, X, G, s_pyr, k.stride, g_stage, g_cnt,
                     (const uint32_t *)s_sdesc, s_kp, (size_t)p->max_keypoints, (uint32_t)p->max_keypoints, s_counts,
                     s_desc, (size_t)p->max_keypoints * p->words, p->words, (uint32_t)P.per_max, ovf);
  return launch_ok(c, "k_gather_orb");
}

// Launches plan P (strips_per_pyr > 0, workspace reserved by reserve_frontend) with the call's pointers.
int run_fused(pislam_ctx *c, const pislam_frontend_params *p, const FrontendPlan &P, const uint8_t *pyramids, size_t stride,
              int batch, uint32_t *kp, uint32_t *desc, uint32_t *counts) {
  const int nsub = P.nsub;
  c->last_path = PISLAM_PATH_FUSED | (P.sel ? PISLAM_PATH_BUCKET_SELECT : 0u) | (P.F.lbs != 0 ? PISLAM_PATH_BUCKETS_IN_STRIPS : 0u);
  // 16-byte loads need 16-byte aligned rows
  bool vec = ((uintptr_t)pyramids % 16 == 0) && (stride % 16 == 0) && (p->vstep % 16 == 0);
  for (int l = 0; l < P.F.nlevels; l++) vec = vec && (P.F.lv[l].col0 % 16 == 0);
  if (P.alias) c->last_strips = (uint32_t)P.F.strips_per_pyr * (uint32_t)batch;
  // A call that is being captured into a hipGraph does not fork: its sub-batches then run in order on the context stream, and
  // the graph is one chain of nodes like every other captured call.  (A graph with a parallel branch from the fork crashed
  // inside hipGraphLaunch when it was replayed; chains replay fine.)  Eager calls fork as before.
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (nsub > 1 && hipStreamIsCapturing(c->stream, &capture) != hipSuccess) {
    (void)hipGetLastError();                      // (the query's own error must not be reported by a later launch check)
    capture = hipStreamCaptureStatusNone;
  }
  const bool fork = nsub > 1 && capture == hipStreamCaptureStatusNone;
  const bool hooks = P.F.dump_score || P.F.ablate;
  const StripKernT kern = strip_kernel(vec, P.alias, hooks, P.F.orb_in_strip, P.F.lbs);
  if (P.klds > LDS_CAP) return fail(c, PISLAM_ERR_INVALID, "level too wide for the strip kernel's LDS tiles");
  RAISE_LDS_LIMIT(c, kern, P.klds);
  const OvfKernT okern = overflow_kernel(vec, hooks);
  if (P.alias) RAISE_LDS_LIMIT(c, okern, P.lds);
  const auto gkern = gather_orb_kernel(P.F.ablate);
  if (!P.generic_orb) {
    if (P.olds > LDS_CAP) return fail(c, PISLAM_ERR_INVALID, "max_keypoints too large for the fused ORB kernel");
    RAISE_LDS_LIMIT(c, gkern, P.olds);
  }
  const FusedCall k{p, P, pyramids, stride, batch, kp, desc, counts, kern, okern, gkern, fork, c->stream, fork ? c->aux_stream : c->stream};
  if (c->frame_disabled) c->last_path |= PISLAM_PATH_FRAME_TIMED_OUT;
  if (P.frame && vec && !c->frame_disabled) return launch_frame(c, k);
  for (int sub = 0; sub < nsub; sub++) PCHK(launch_sub_batch(c, k, sub));
  if (fork) {                                       // join: the call is complete, in stream order, on the context stream
    HIPCHK(c, hipEventRecord(c->ev_join, k.X));
    HIPCHK(c, hipStreamWaitEvent(k.M, c->ev_join, 0));
  }
  return PISLAM_OK;
}

// The staged pipeline: a launch group per level (FAST, Harris, ordered extraction), then per-keypoint ORB over the batch.
int run_staged(pislam_ctx *c, const pislam_frontend_params *p, const pislam_level *lv, const uint8_t *pyramids, size_t stride,
               int batch, uint32_t *kp, uint32_t *desc, uint32_t *counts) {
  const size_t pyr_bytes = (size_t)p->rows * p->vstep;
  uint8_t *score = c->w_score.as<uint8_t>();
  HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(uint32_t) * batch, c->stream));
  // The score map workspace is laid out with stride pyr_bytes; the image with `stride`.  The stage
  // kernels take one stride for both, so when they differ fall back to per-pyramid launches.
  const bool same = stride == pyr_bytes;
  for (int l = 0; l < p->nlevels; l++) {
    const size_t off = (size_t)lv[l].row0 * p->vstep + lv[l].col0;
    if (same) {
      PCHK(launch_detect(c, pyramids + off, score + off, p->vstep, pyr_bytes, batch, p->border,
                         lv[l].width, lv[l].height, p->fast_threshold));
      PCHK(launch_harris(c, pyramids + off, score + off, p->vstep, pyr_bytes, batch, p->border,
                         lv[l].width, lv[l].height, p->harris_threshold));
    } else {
      for (int b = 0; b < batch; b++) {
        PCHK(launch_detect(c, pyramids + b * stride + off, score + b * pyr_bytes + off, p->vstep, 0, 1,
                           p->border, lv[l].width, lv[l].height, p->fast_threshold));
        PCHK(launch_harris(c, pyramids + b * stride + off, score + b * pyr_bytes + off, p->vstep, 0, 1,
                           p->border, lv[l].width, lv[l].height, p->harris_threshold));
      }
    }
  }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  for (int l = 0; l < p->nlevels; l++) {
    const size_t off = (size_t)lv[l].row0 * p->vstep + lv[l].col0;
    const uint32_t add_xy = ((uint32_t)lv[l].col0 << 12) | (uint32_t)lv[l].row0;   // README.md:78
    PCHK(launch_extract(c, score + off, p->vstep, pyr_bytes, batch, p->border, p->log_bucket_size,
                        p->bucket_limit, lv[l].width, lv[l].height, kp, (size_t)p->max_keypoints,
                        (uint32_t)p->max_keypoints, add_xy, counts));
  }
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  return launch_orb_batch(c, c->stream, p, pyramids, stride, batch, kp, counts, desc);
}

}  // namespace

// Host-only: plan a batch call for these parameters with the call's own planner (fp::plan_frontend: no device, no allocation,
// no launch) and check the invariants of its strip plan and bucket selection plan (fp::strip_plan_violation, fp::select_plan_violation).
// For the sanitizer runs of the host code (tests/test_sanitizers.py runs thousands of random level tables through it in a library built
// with -fsanitize=address,undefined) and for tools that want to know what a call will launch.  options: "key=value,key=value"
// (pislam_ctx_set_option keys).  summary: [0] plan entries, [1] strips per pyramid, [2] runs per pyramid, [3] staging slots per pyramid,
// [4] run length, [5] LDS bytes (plain layout), [6] LDS bytes (aliased layout), [7] units of the selection pass (0: none).
PISLAM_EXPORT int pislam_debug_build_plan(const pislam_frontend_params *p, const pislam_level *lv, int batch, int num_cus,
                                          int lanes_in_flight, const char *options, uint32_t summary[8], char *err, size_t err_cap) {
  auto say = [&](int rc, const char *prefix, const char *what) {
    if (err && err_cap) snprintf(err, err_cap, "%s%s", prefix, what);
    return rc;
  };
  auto refuse = [&](const char *what) { return say(PISLAM_ERR_INVALID, "", what); };
  auto bad = [&](const char *what) { return say(PISLAM_ERR_HIP, "plan invariant violated: ", what); };
  fp::Options o;
  o.num_cus = num_cus > 0 ? num_cus : 256;
  o.lanes_in_flight = lanes_in_flight > 0 ? lanes_in_flight : 1;
  if (!summary) return PISLAM_ERR_INVALID;
  memset(summary, 0, sizeof(uint32_t) * 8);
  for (const char *q = options; q && *q;) {
    const char *e = strchr(q, ','), *eq = strchr(q, '=');
    const size_t len = e ? (size_t)(e - q) : strlen(q);
    if (!eq || (size_t)(eq - q) >= len) return refuse("options: key=value[,key=value...]");
    const std::string key(q, eq - q);
    if (key == "own_stream") return refuse("own_stream needs a device");
    const char *refusal = nullptr;
    if (key != "frame_rearm" && !fp::set_option(o, key.c_str(), atoi(eq + 1), &refusal)) refusal = "unknown option";
    if (refusal) return refuse(refusal);
    q += len + (e ? 1 : 0);
  }
  if (const char *refusal = fp::check_params(p, lv, batch)) return refuse(refusal);
  FrontendPlan P;
  const char *plan_refusal = fp::plan_frontend(o, p, lv, batch, &P);
  if (!P.fused) return refuse("no strip plan for these parameters (the staged pipeline takes the call)");
  if (const char *what = fp::strip_plan_violation(P, p)) return bad(what);
  const uint32_t strip_summary[7] = {(uint32_t)P.F.nlevels,       (uint32_t)P.F.strips_per_pyr, (uint32_t)P.F.runs_per_pyr,
                                     (uint32_t)P.F.slots_per_pyr, (uint32_t)P.F.run_len,        (uint32_t)P.lds,
                                     (uint32_t)P.lds_alias};
  memcpy(summary, strip_summary, sizeof(strip_summary));
  if (plan_refusal) return refuse(plan_refusal);   // (a refusal of the selection plan: reported after the strip plan checks)
  if (P.sel) {
    if (const char *what = fp::select_plan_violation(P, p)) return bad(what);
    summary[7] = (uint32_t)P.Q.units_per_pyr;
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_frontend_reserve(pislam_ctx *c, const pislam_frontend_params *p,
                                          const pislam_level *lv, int batch) {
  PCHK(check_params(c, p, lv, batch));
  HIPCHK(c, hipSetDevice(c->device));
  FrontendPlan P;
  PCHK(plan_frontend(c, p, lv, batch, &P));
  return reserve_frontend(c, p, lv, P, batch);
}

PISLAM_EXPORT int pislam_orb_frontend_batch(pislam_ctx *c, const pislam_frontend_params *p,
                                            const pislam_level *lv, const uint8_t *pyramids,
                                            size_t stride, int batch, uint32_t *kp, uint32_t *desc,
                                            uint32_t *counts) {
  PCHK(check_params(c, p, lv, batch));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(check_frame_poison(c));
  if (!pyramids || !kp || !desc || !counts) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  if (stride < (size_t)p->rows * p->vstep) return fail(c, PISLAM_ERR_INVALID, "pyramid_stride too small");
  if (!is_device_ptr(pyramids) || !is_device_ptr(kp) || !is_device_ptr(desc) || !is_device_ptr(counts))
    return fail(c, PISLAM_ERR_INVALID, "the batch path takes device pointers only");
  FrontendPlan P;
  PCHK(plan_frontend(c, p, lv, batch, &P));
  if (c->opt.pipeline >= 2 && !P.fused)
    return fail(c, PISLAM_ERR_INVALID, "fused pipeline unavailable for these parameters (bucket size / LDS size)");
  PCHK(reserve_frontend(c, p, lv, P, batch));
  c->last_stride = (size_t)p->rows * p->vstep;
  c->last_pipeline = P.fused ? 2 : 1;
  c->last_path = P.fused ? PISLAM_PATH_FUSED : PISLAM_PATH_STAGED;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if (P.fused && P.F.strips_per_pyr == 0) {          // every level is smaller than 2 x border: nothing to extract
    HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(uint32_t) * batch, c->stream));
    for (int i = 1; i < 4; i++) HIPCHK(c, hipEventRecord(c->ev[i], c->stream));
    c->timing_valid = true;
    c->last_strips = 0;
    return PISLAM_OK;
  }
  PCHK(P.fused ? run_fused(c, p, P, pyramids, stride, batch, kp, desc, counts)
               : run_staged(c, p, lv, pyramids, stride, batch, kp, desc, counts));
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  c->timing_valid = true;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_frontend_get_score_map(pislam_ctx *c, int b, uint8_t *dst) {
  if (!c || !dst) return PISLAM_ERR_INVALID;
  if (b < 0 || b >= c->last_batch || !c->w_score.p || !c->last_stride)
    return fail(c, PISLAM_ERR_INVALID, "no score map for that pyramid");
  if (c->last_pipeline == 2 && !c->opt.dump_score)
    return fail(c, PISLAM_ERR_INVALID, "the fused pipeline keeps the score map in LDS (set option dump_score)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = c->last_stride;
  HIPCHK(c, hipMemcpyAsync(dst, c->w_score.as<uint8_t>() + (size_t)b * bytes, bytes, hipMemcpyDefault,
                           c->stream));
  return sync(c);
}

PISLAM_EXPORT int pislam_frontend_last_stats(pislam_ctx *c, uint32_t stats[2]) {
  if (!c || !stats) return PISLAM_ERR_INVALID;
  stats[0] = stats[1] = 0;
  if (!c->w_ovf.p || !c->last_strips) return PISLAM_OK;      // staged pipeline / separate-tile layout: nothing deferred
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(sync(c));
  PCHK(check_frame_poison(c));
  uint32_t prev[fp::MAX_SUB] = {};
  for (int i = 0; i < c->ovf_nsub; i++)          // one list per sub-batch: [1] = strips the last step deferred
    HIPCHK(c, hipMemcpyAsync(&prev[i], c->w_ovf.as<uint32_t>() + (size_t)i * c->ovf_stride + 1, sizeof(uint32_t),
                             hipMemcpyDeviceToHost, c->stream));
  PCHK(sync(c));
  for (int i = 0; i < c->ovf_nsub; i++) stats[0] += prev[i];
  stats[1] = c->last_strips;
  return PISLAM_OK;
}

PISLAM_EXPORT unsigned pislam_frontend_last_path(const pislam_ctx *c) { return c ? c->last_path : 0u; }

PISLAM_EXPORT int pislam_frontend_last_timing(pislam_ctx *c, float *total_ms, float stage_ms[3]) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!c->timing_valid) return fail(c, PISLAM_ERR_INVALID, "no batch call recorded");
  HIPCHK(c, hipEventSynchronize(c->ev[3]));
  if (total_ms) HIPCHK(c, hipEventElapsedTime(total_ms, c->ev[0], c->ev[3]));
  if (stage_ms)
    for (int i = 0; i < 3; i++) HIPCHK(c, hipEventElapsedTime(&stage_ms[i], c->ev[i], c->ev[i + 1]));
  return PISLAM_OK;
}

// ---- measurement aid: shader clock under the current load ------------------------------------------
namespace {
__global__ void k_shader_clock(unsigned long long ticks_100mhz, unsigned long long *out) {
  const unsigned long long w0 = wall_clock64(), c0 = (unsigned long long)clock64();
  unsigned long long w1 = w0;
  while (w1 - w0 < ticks_100mhz) w1 = wall_clock64();
  const unsigned long long c1 = (unsigned long long)clock64();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = w1 - w0;
  }
}
}  // namespace

PISLAM_EXPORT int pislam_debug_shader_clock(pislam_ctx *c, int micros, double *ghz) {
  if (!c || !ghz) return PISLAM_ERR_INVALID;
  if (micros < 1 || micros > 100000) return fail(c, PISLAM_ERR_INVALID, "micros must be 1..100000");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->w_total.ensure(2 * sizeof(unsigned long long)) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc");
  hipLaunchKernelGGL(k_shader_clock, dim3(1), dim3(64), 0, c->stream, (unsigned long long)micros * 100ull,
                     c->w_total.as<unsigned long long>());
  PCHK(launch_ok(c, "k_shader_clock"));
  unsigned long long r[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(r, c->w_total.p, sizeof(r), hipMemcpyDeviceToHost, c->stream));
  PCHK(sync(c));
  *ghz = r[1] ? (double)r[0] / (double)r[1] * 0.1 : 0.0;
  return PISLAM_OK;
}

// ---- descriptor matching --------------------------------------------------

namespace {

// Argument checks the matchers, the bag-of-words calls and the key-frame database share.
int check_words(pislam_ctx *c, int words) {
  if (words != 1 && words != 2 && words != 4 && words != 8) return fail(c, PISLAM_ERR_INVALID, "words must be 1, 2, 4 or 8");
  return PISLAM_OK;
}
int check_batch(pislam_ctx *c, int batch) {                                   // (a batch is the grid's y or x extent)
  if (batch < 0 || batch > 65535) return fail(c, PISLAM_ERR_INVALID, "batch must be 0..65535");
  return PISLAM_OK;
}
int check_train_stride(pislam_ctx *c, size_t t_stride, const char *what) {   // (the match keys hold a 16-bit train index)
  if (t_stride > 65535) return fail(c, PISLAM_ERR_INVALID, what);
  return PISLAM_OK;
}

// f(std::integral_constant<int, W>{}) for W = words, which check_words accepted.
template <class F>
void with_words(int words, F &&f) {
  switch (words) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// The same for sad_radius, which stereo_plan accepted (1..pm::ST_MAX_W), and the tracker's win_radius (1..pt::LK_MAX_W, also 7).
template <class F>
void with_sad_radius(int sad_radius, F &&f) {
  switch (sad_radius) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 7>{}); break;
  }
}

int launch_match(pislam_ctx *c, int words, const uint32_t *q, const uint32_t *qc, size_t q_stride, uint32_t nq,
                 const uint32_t *t, const uint32_t *tc, size_t t_stride, uint32_t nt, int batch, uint32_t max_q,
                 int32_t *idx, uint32_t *dist, uint32_t *dist2, size_t out_stride) {
  PCHK(check_words(c, words));
  const uint32_t cap_q = (uint32_t)std::min<size_t>(q_stride, 0xffffffffu), cap_t = (uint32_t)std::min<size_t>(t_stride, 65535);
  if (c->opt.match_mfma) {
    // matrix-core path (v_mfma_i32_32x32x32_i8): 4 waves x 32 queries per workgroup pass
    // query blocks per pair in flight: the batch API only knows the capacity (the counts live on the device), and a
    // workgroup that finds no queries still costs its launch (~30 ns each: 32 blocks per pair at batch 256 took
    // 0.27 ms against 0.09 ms with 8), so the grid aims at ~8 workgroups per CU and the workgroups loop
    const int per_pair = batch > 1 ? std::max(1, std::min(cdiv((int)max_q, pm::MF_Q), cdiv(8 * std::max(1, c->opt.num_cus), batch))) : 65535;
    const dim3 mgrid((unsigned)std::min(cdiv((int)max_q, pm::MF_Q), per_pair), (unsigned)batch);
    with_words(words, [&](auto w) {
      constexpr int W = decltype(w)::value;
      hipLaunchKernelGGL(pm::k_match_mfma<W>, mgrid, dim3(64 * pm::MF_WAVES), 0, c->stream, q, qc, q_stride * W, nq, t, tc,
                         t_stride * W, nt, cap_q, cap_t, idx, dist, dist2, out_stride);
    });
    return launch_ok(c, "k_match_mfma");
  }
  const dim3 grid((unsigned)std::min(cdiv((int)max_q, pm::QPW), batch > 1 ? pm::MAX_GRID_X : 65535), (unsigned)batch);
  with_words(words, [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL(pm::k_match<W>, grid, dim3(pm::QPW * pm::SPLIT), 0, c->stream, q, qc, q_stride * W, nq, t, tc,
                       t_stride * W, nt, cap_q, cap_t, idx, dist, dist2, out_stride);
  });
  return launch_ok(c, "k_match");
}

}  // namespace

PISLAM_EXPORT int pislam_match_hamming(pislam_ctx *c, int words, const uint32_t *query, size_t nq,
                                       const uint32_t *train, size_t nt, int32_t *idx, uint32_t *dist,
                                       uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(check_words(c, words));
  if (nt > 65535) return fail(c, PISLAM_ERR_INVALID, "at most 65535 train descriptors");
  if (nq > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "too many query descriptors");
  if (nq == 0) return PISLAM_OK;
  if (!query || !idx || !dist || !dist2 || (nt && !train)) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  Staged sq, st, si, sd, s2;
  PCHK(stage_in(c, c->s_desc, query, nq * words * sizeof(uint32_t), &sq));
  PCHK(stage_in(c, c->s_tmp, train, nt * words * sizeof(uint32_t), &st));
  PCHK(stage_in(c, c->s_pts, idx, nq * sizeof(int32_t), &si, false));
  PCHK(stage_in(c, c->s_misc, dist, nq * sizeof(uint32_t), &sd, false));
  PCHK(stage_in(c, c->s_out, dist2, nq * sizeof(uint32_t), &s2, false));
  PCHK(launch_match(c, words, (const uint32_t *)sq.dev, nullptr, nq, (uint32_t)nq, (const uint32_t *)st.dev, nullptr,
                    std::max<size_t>(nt, 1), (uint32_t)nt, 1, (uint32_t)nq, (int32_t *)si.dev, (uint32_t *)sd.dev,
                    (uint32_t *)s2.dev, nq));
  PCHK(stage_out(c, si, idx, nq * sizeof(int32_t)));
  PCHK(stage_out(c, sd, dist, nq * sizeof(uint32_t)));
  PCHK(stage_out(c, s2, dist2, nq * sizeof(uint32_t)));
  return sync(c);
}

PISLAM_EXPORT int pislam_match_hamming_batch(pislam_ctx *c, int words, const uint32_t *query,
                                             const uint32_t *qcounts, size_t q_stride, const uint32_t *train,
                                             const uint32_t *tcounts, size_t t_stride, int batch, int32_t *idx,
                                             uint32_t *dist, uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(check_batch(c, batch));
  PCHK(check_train_stride(c, t_stride, "at most 65535 train descriptors per pair"));
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  if (!query || !train || !qcounts || !tcounts || !idx || !dist || !dist2) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  for (const void *ptr : {(const void *)query, (const void *)train, (const void *)qcounts, (const void *)tcounts,
                          (const void *)idx, (const void *)dist, (const void *)dist2})
    if (!is_device_ptr(ptr)) return fail(c, PISLAM_ERR_INVALID, "the batch matcher takes device pointers only");
  HIPCHK(c, hipSetDevice(c->device));
  return launch_match(c, words, query, qcounts, q_stride, 0, train, tcounts, t_stride, 0, batch, (uint32_t)q_stride,
                      idx, dist, dist2, q_stride);
}

// ---- guided window matching: windowed, scale-aware ------------------------------------------

namespace {

// Checks the arguments every scaled-window call shares and lays out the per-pair cell grids (host only).  Level lt's
// grid covers its mapped extent [0, ext_x] x [0, ext_y] in level-0 pixels with square cells of side m[lt] * f, where
// m[lt] is the largest max(1, radius0[lq]) of the query levels lq that reach lt and f >= 1 is the
// smallest factor that keeps all levels' cells within pm::WIN_MAX_CELLS (the LDS histogram of k_scaled_index).  Results
// do not depend on the side: the match applies the exact window test.
// The general form (the projection matcher's): a query on level lq sees the train levels lq - level_below ..
// lq + level_above, so level lt is reached by the query levels lt - level_above .. lt + level_below.
int scaled_plan(pislam_ctx *c, int words, const pislam_level *lv, int nlevels, const int32_t *scale_q16,
                const int32_t *radius0, int level_below, int level_above, size_t t_stride, int batch, pm::ScaledPlan *P) {
  PCHK(check_words(c, words));
  if (nlevels < 1 || nlevels > pm::WIN_MAX_LEVELS) return fail(c, PISLAM_ERR_INVALID, "nlevels must be 1..16");
  if (!lv || !scale_q16 || !radius0) return fail(c, PISLAM_ERR_INVALID, "null levels / scale_q16 / radius0");
  if (level_below < 0 || level_below > nlevels - 1 || level_above < 0 || level_above > nlevels - 1)
    return fail(c, PISLAM_ERR_INVALID, level_below == level_above ? "level_span must be 0..nlevels-1"
                                                                  : "level_below / level_above must be 0..nlevels-1");
  PCHK(check_train_stride(c, t_stride, "at most 65535 train entries per pair"));
  PCHK(check_batch(c, batch));
  int32_t ext_x[pm::WIN_MAX_LEVELS], ext_y[pm::WIN_MAX_LEVELS];
  for (int l = 0; l < nlevels; l++) {
    const pislam_level &L = lv[l];
    if (L.width < 1 || L.height < 1 || L.col0 < 0 || L.row0 < 0 || L.col0 + L.width > 4096 || L.row0 + L.height > 4096)
      return fail(c, PISLAM_ERR_INVALID, "level rectangles must be non-empty and fit 12-bit coordinates");
    if (radius0[l] < 0 || radius0[l] > 65535) return fail(c, PISLAM_ERR_INVALID, "radius0 must be 0..65535");
    if (scale_q16[l] < 1 || scale_q16[l] > (1 << 20)) return fail(c, PISLAM_ERR_INVALID, "scale_q16 must be 1..2^20");
    const long long ex = ((long long)(L.width - 1) * scale_q16[l] + 32768) >> 16;
    const long long ey = ((long long)(L.height - 1) * scale_q16[l] + 32768) >> 16;
    if (ex > 65535 || ey > 65535) return fail(c, PISLAM_ERR_INVALID, "a level's mapped extent exceeds 65535");
    ext_x[l] = (int32_t)ex, ext_y[l] = (int32_t)ey;
    for (int k = 0; k < l; k++) {
      const pislam_level &K = lv[k];
      if (L.col0 < K.col0 + K.width && K.col0 < L.col0 + L.width && L.row0 < K.row0 + K.height && K.row0 < L.row0 + L.height)
        return fail(c, PISLAM_ERR_INVALID, "level rectangles overlap");
    }
  }
  long long m[pm::WIN_MAX_LEVELS];
  for (int lt = 0; lt < nlevels; lt++) {
    m[lt] = 1;
    for (int lq = std::max(0, lt - level_above); lq <= std::min(nlevels - 1, lt + level_below); lq++)
      m[lt] = std::max<long long>(m[lt], radius0[lq]);
  }
  auto side = [&](int l, long long f) { return (int)std::min<long long>(65536, m[l] * f); };
  auto cells = [&](long long f) {
    long long n = 0;
    for (int l = 0; l < nlevels; l++) n += (long long)cdiv(ext_x[l] + 1, side(l, f)) * cdiv(ext_y[l] + 1, side(l, f));
    return n;
  };
  // cells(f) ~ cells(1) / f^2: start just below that estimate; side 65536 leaves one cell per level, so this ends
  long long f = std::max(1LL, (long long)std::sqrt((double)cells(1) / pm::WIN_MAX_CELLS));
  while (cells(f) > pm::WIN_MAX_CELLS) f++;
  *P = pm::ScaledPlan{};
  int base = 0;
  for (int l = 0; l < nlevels; l++) {
    const int s = side(l, f), ncx = cdiv(ext_x[l] + 1, s);
    P->lv[l] = pm::ScaledLevel{lv[l].col0, lv[l].row0, lv[l].width, lv[l].height, scale_q16[l], ext_x[l], ext_y[l],
                               radius0[l], s, ncx, base};
    base += ncx * cdiv(ext_y[l] + 1, s);
  }
  P->nlevels = nlevels;
  P->ncells = base;
  P->span = level_below;                                 // (k_match_scaled reads it; its callers pass below == above)
  return PISLAM_OK;
}

// The symmetric form of the windowed, the scaled and the stereo call: |lq - lt| <= level_span.
int scaled_plan(pislam_ctx *c, int words, const pislam_level *lv, int nlevels, const int32_t *scale_q16,
                const int32_t *radius0, int level_span, size_t t_stride, int batch, pm::ScaledPlan *P) {
  return scaled_plan(c, words, lv, nlevels, scale_q16, radius0, level_span, level_span, t_stride, batch, P);
}

// The windowed matcher's plan: the scaled plan with unit scales (mapped = level-local coordinates), span 0 and
// radius0 = radius, so level l's cells are max(1, radius[l]) * f level pixels over its rectangle.
int window_plan(pislam_ctx *c, int words, const pislam_level *lv, int nlevels, const int32_t *radius, size_t t_stride,
                int batch, pm::ScaledPlan *P) {
  if (!lv || !radius) return fail(c, PISLAM_ERR_INVALID, "null levels / radius");
  for (int l = 0; l < std::min(nlevels, pm::WIN_MAX_LEVELS); l++)
    if (radius[l] < 0 || radius[l] > 4095) return fail(c, PISLAM_ERR_INVALID, "radius must be 0..4095");
  int32_t unit[pm::WIN_MAX_LEVELS];
  std::fill(unit, unit + pm::WIN_MAX_LEVELS, 65536);
  return scaled_plan(c, words, lv, nlevels, unit, radius, 0, t_stride, batch, P);
}

// The workspace of an index kernel (pm::lds_counting_sort): noffsets offsets per pair, and per train entry meta_bytes of
// metadata and the descriptor.
int index_workspace(pislam_ctx *c, pislam_ctx::CellIndex &w, size_t noffsets, size_t meta_bytes, int words, size_t t_stride,
                    int batch, const char *what) {
  if (w.off.ensure(sizeof(uint32_t) * noffsets * batch) != PISLAM_OK ||
      w.meta.ensure(meta_bytes * t_stride * batch) != PISLAM_OK ||
      w.desc.ensure(sizeof(uint32_t) * words * t_stride * batch) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, what);
  return PISLAM_OK;
}

// The guided matchers take device pointers only: fails with `what` at the first host pointer.
int device_ptrs(pislam_ctx *c, std::initializer_list<const void *> ptrs, const char *what) {
  for (const void *ptr : ptrs) {
    if (!ptr) return fail(c, PISLAM_ERR_INVALID, "null pointer");
    if (!is_device_ptr(ptr)) return fail(c, PISLAM_ERR_INVALID, what);
  }
  return PISLAM_OK;
}

// Query tiles per pair in flight for `qpw` queries per workgroup pass: the counts live on the device, so the grid is sized
// for the capacity and aims at ~16 workgroups per CU over the batch; a workgroup loops over further tiles of its pair.
dim3 query_grid(const pislam_ctx *c, size_t q_stride, int qpw, int batch) {
  const int tiles = cdiv((int)std::min<size_t>(q_stride, 0x7fffffff - qpw), qpw);
  const int per_pair = batch > 1 ? std::max(1, std::min(tiles, cdiv(16 * std::max(1, c->opt.num_cus), batch))) : std::min(tiles, 65535);
  return dim3((unsigned)per_pair, (unsigned)batch);
}

// pm::k_scaled_index of the train entries into workspace w (arguments checked, w reserved).
int launch_scaled_index(pislam_ctx *c, const pislam_ctx::CellIndex &w, const pm::ScaledPlan &P, int words,
                        const uint32_t *kp, const uint32_t *desc, const uint32_t *counts, size_t stride, int batch) {
  hipLaunchKernelGGL(pm::k_scaled_index, dim3((unsigned)batch), dim3(pm::WIN_INDEX_THREADS), 0, c->stream, P, words, kp,
                     desc, counts, stride, w.off.as<uint32_t>(), w.meta.as<uint2>(), w.desc.as<uint32_t>());
  return launch_ok(c, "k_scaled_index");
}

// Index + match of the windowed and the scaled call (arguments checked, workspace w reserved).
int launch_guided(pislam_ctx *c, const pislam_ctx::CellIndex &w, const pm::ScaledPlan &P, int words, const uint32_t *qkp,
                  const uint32_t *qdesc, const uint32_t *qcounts, const int32_t *qpred, size_t q_stride,
                  const uint32_t *tkp, const uint32_t *tdesc, const uint32_t *tcounts, size_t t_stride, int batch,
                  int32_t *idx, uint32_t *dist, uint32_t *dist2) {
  PCHK(launch_scaled_index(c, w, P, words, tkp, tdesc, tcounts, t_stride, batch));
  const dim3 grid = query_grid(c, q_stride, pm::WIN_QPW, batch);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(pm::WIN_THREADS), 0, c->stream, P, qkp, qdesc, qcounts, qpred, q_stride, t_stride,
                       w.off.as<uint32_t>(), w.meta.as<uint2>(), w.desc.as<uint32_t>(), idx, dist, dist2);
  };
  with_words(words, [&](auto wd) {
    constexpr int W = decltype(wd)::value;
    if (P.span == 0)
      launch(pm::k_match_scaled<W, true>);
    else
      launch(pm::k_match_scaled<W, false>);
  });
  return launch_ok(c, "k_match_scaled");
}

}  // namespace

PISLAM_EXPORT int pislam_match_window_reserve(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                              const int32_t *radius, size_t t_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(window_plan(c, words, levels, nlevels, radius, t_stride, batch, &P));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_win, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                         "hipMalloc(window matcher workspace)");
}

PISLAM_EXPORT int pislam_match_hamming_window_batch(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                                    const int32_t *radius, const uint32_t *qkp, const uint32_t *qdesc,
                                                    const uint32_t *qcounts, size_t q_stride, const uint32_t *tkp,
                                                    const uint32_t *tdesc, const uint32_t *tcounts, size_t t_stride,
                                                    int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(window_plan(c, words, levels, nlevels, radius, t_stride, batch, &P));
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {qkp, qdesc, qcounts, tkp, tdesc, tcounts, idx, dist, dist2},
                   "the window matcher takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, c->w_win, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                       "hipMalloc(window matcher workspace)"));
  return launch_guided(c, c->w_win, P, words, qkp, qdesc, qcounts, nullptr, q_stride, tkp, tdesc, tcounts, t_stride, batch,
                       idx, dist, dist2);
}

PISLAM_EXPORT int pislam_match_scaled_window_reserve(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                                     const int32_t *scale_q16, const int32_t *radius0, int level_span,
                                                     size_t t_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(scaled_plan(c, words, levels, nlevels, scale_q16, radius0, level_span, t_stride, batch, &P));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_sc, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                         "hipMalloc(scaled window matcher workspace)");
}

PISLAM_EXPORT int pislam_match_hamming_scaled_window_batch(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                                           const int32_t *scale_q16, const int32_t *radius0, int level_span,
                                                           const uint32_t *qkp, const uint32_t *qdesc, const uint32_t *qcounts,
                                                           const int32_t *qpred, size_t q_stride, const uint32_t *tkp,
                                                           const uint32_t *tdesc, const uint32_t *tcounts, size_t t_stride,
                                                           int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(scaled_plan(c, words, levels, nlevels, scale_q16, radius0, level_span, t_stride, batch, &P));
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  if (qpred && !is_device_ptr(qpred)) return fail(c, PISLAM_ERR_INVALID, "qpred must be a device pointer or null");
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {qkp, qdesc, qcounts, tkp, tdesc, tcounts, idx, dist, dist2},
                   "the scaled window matcher takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, c->w_sc, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                       "hipMalloc(scaled window matcher workspace)"));
  return launch_guided(c, c->w_sc, P, words, qkp, qdesc, qcounts, qpred, q_stride, tkp, tdesc, tcounts, t_stride, batch,
                       idx, dist, dist2);
}

// ---- map-point search by projection -------------------------------------------------------

namespace {

// Checks the tables of a projection call and lays out the train side: the scaled plan with the one-sided level window
// and, per level, the larger of the two radii (the match applies the exact radius of the query's predicted level).
int projection_plan(pislam_ctx *c, int words, const pislam_level *lv, int nlevels, const int32_t *scale_q16,
                    const int32_t *radius_far, const int32_t *radius_near, int level_below, int level_above,
                    size_t t_stride, int batch, pm::ScaledPlan *P, pjm::Tables *tab) {
  if (nlevels < 1 || nlevels > pm::WIN_MAX_LEVELS) return fail(c, PISLAM_ERR_INVALID, "nlevels must be 1..16");
  if (!radius_far) return fail(c, PISLAM_ERR_INVALID, "null radius_far");
  int32_t rmax[pm::WIN_MAX_LEVELS];
  *tab = pjm::Tables{};
  for (int l = 0; l < nlevels; l++) {
    const int32_t rf = radius_far[l], rn = radius_near ? radius_near[l] : rf;
    if (rf < 0 || rf > pjm::MAX_RADIUS || rn < 0 || rn > pjm::MAX_RADIUS)
      return fail(c, PISLAM_ERR_INVALID, "radius_far / radius_near must be 0..65535");
    tab->radius_far[l] = rf, tab->radius_near[l] = rn;
    rmax[l] = std::max(rf, rn);
  }
  tab->nlevels = nlevels;
  return scaled_plan(c, words, lv, nlevels, scale_q16, rmax, level_below, level_above, t_stride, batch, P);
}

}  // namespace

PISLAM_EXPORT int pislam_match_projection_reserve(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                                  const int32_t *scale_q16, const int32_t *radius_far,
                                                  const int32_t *radius_near, int level_below, int level_above,
                                                  size_t t_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  pjm::Tables tab;
  PCHK(projection_plan(c, words, levels, nlevels, scale_q16, radius_far, radius_near, level_below, level_above, t_stride,
                       batch, &P, &tab));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_proj, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                         "hipMalloc(projection matcher workspace)");
}

namespace {

// The projection call and the fuse call: every check of the projection call's contract, then the index and the match.
// fz null: pislam_match_projection_batch on w; otherwise pislam_match_fuse_batch (fz's table and bounds are checked by
// the caller, its two pointers here).
int projection_call(pislam_ctx *c, pislam_ctx::CellIndex &w, const char *alloc_what, const pj::FuseArgs *fz, int words,
                    const pislam_level *levels, int nlevels, const int32_t *scale_q16, const float *level_scale,
                    const int32_t *radius_far, const int32_t *radius_near, const pislam_projection_params *p,
                    const float *pose, const float *cam, const float *xw, const float *normal, const float *drange,
                    const uint8_t *qlevel, const uint32_t *qdesc, const uint32_t *qcounts, size_t q_stride,
                    const uint32_t *tkp, const uint32_t *tdesc, const uint32_t *tcounts, size_t t_stride, int batch,
                    int32_t *idx, uint32_t *dist, uint32_t *dist2, int32_t *pred, uint8_t *plevel) {
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  pm::ScaledPlan P;
  pjm::Tables tab;
  PCHK(projection_plan(c, words, levels, nlevels, scale_q16, radius_far, radius_near, p->level_below, p->level_above,
                       t_stride, batch, &P, &tab));
  if (!level_scale) return fail(c, PISLAM_ERR_INVALID, "null level_scale");
  for (int l = 0; l < nlevels; l++) {
    if (!psm::finite_f(level_scale[l]) || !(level_scale[0] > 0.0f) || (l && !(level_scale[l] >= level_scale[l - 1])))
      return fail(c, PISLAM_ERR_INVALID, "level_scale must be finite, positive and non-decreasing");
    tab.level_scale[l] = level_scale[l];
  }
  for (float v : {p->min_x, p->max_x, p->min_y, p->max_y})
    if (!(fabsf(v) <= pjm::BOUND_LIMIT)) return fail(c, PISLAM_ERR_INVALID, "the image bounds must lie within +-2^20");
  if (!(p->min_x <= p->max_x) || !(p->min_y <= p->max_y)) return fail(c, PISLAM_ERR_INVALID, "need min_x <= max_x and min_y <= max_y");
  if (p->second_same_level != 0 && p->second_same_level != 1)
    return fail(c, PISLAM_ERR_INVALID, "second_same_level must be 0 or 1");
  if ((drange != nullptr) == (qlevel != nullptr))
    return fail(c, PISLAM_ERR_INVALID, "exactly one of drange (map mode) and qlevel (level mode) must be given");
  if (normal && qlevel) return fail(c, PISLAM_ERR_INVALID, "normal needs drange (map mode)");
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  const char *what = fz ? "the fuse matcher takes device pointers only" : "the projection matcher takes device pointers only";
  for (const void *opt : {(const void *)normal, (const void *)drange, (const void *)qlevel, (const void *)pred,
                          (const void *)plevel, (const void *)(fz ? fz->qmask : nullptr)})
    if (opt && !is_device_ptr(opt)) return fail(c, PISLAM_ERR_INVALID, what);
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {pose, cam, xw, qdesc, qcounts, tkp, tdesc, tcounts, idx, dist, dist2}, what));
  if (fz) PCHK(device_ptrs(c, {fz->tobs}, what));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, w, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch, alloc_what));
  PCHK(launch_scaled_index(c, w, P, words, tkp, tdesc, tcounts, t_stride, batch));
  const pjm::Params prm{p->min_x, p->max_x, p->min_y, p->max_y, p->cos_min, p->cos_near,
                        p->level_below, p->level_above, p->second_same_level};
  pj::ProjArgs a{};
  a.pose = pose, a.cam = cam, a.xw = xw, a.normal = normal, a.drange = drange, a.qlevel = qlevel;
  a.qdesc = qdesc, a.qcount = qcounts, a.tkp = tkp, a.q_stride = q_stride, a.t_stride = t_stride;
  a.cell_off = w.off.as<uint32_t>(), a.ent_meta = w.meta.as<uint2>(), a.ent_desc = w.desc.as<uint32_t>();
  a.idx = idx, a.dist = dist, a.dist2 = dist2, a.pred = pred, a.plevel = plevel;
  const dim3 grid = query_grid(c, q_stride, pm::WIN_QPW, batch);
  with_words(words, [&](auto wd) {
    if (fz)
      hipLaunchKernelGGL(pj::k_match_fuse<decltype(wd)::value>, grid, dim3(pm::WIN_THREADS), 0, c->stream, P, tab, prm, a,
                         *fz);
    else
      hipLaunchKernelGGL(pj::k_match_projection<decltype(wd)::value>, grid, dim3(pm::WIN_THREADS), 0, c->stream, P, tab, prm,
                         a);
  });
  return launch_ok(c, fz ? "k_match_fuse" : "k_match_projection");
}

}  // namespace

PISLAM_EXPORT int pislam_match_projection_batch(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                                const int32_t *scale_q16, const float *level_scale,
                                                const int32_t *radius_far, const int32_t *radius_near,
                                                const pislam_projection_params *p, const float *pose, const float *cam,
                                                const float *xw, const float *normal, const float *drange,
                                                const uint8_t *qlevel, const uint32_t *qdesc, const uint32_t *qcounts,
                                                size_t q_stride, const uint32_t *tkp, const uint32_t *tdesc,
                                                const uint32_t *tcounts, size_t t_stride, int batch, int32_t *idx,
                                                uint32_t *dist, uint32_t *dist2, int32_t *pred, uint8_t *plevel) {
  if (!c) return PISLAM_ERR_INVALID;
  return projection_call(c, c->w_proj, "hipMalloc(projection matcher workspace)", nullptr, words, levels, nlevels,
                         scale_q16, level_scale, radius_far, radius_near, p, pose, cam, xw, normal, drange, qlevel, qdesc,
                         qcounts, q_stride, tkp, tdesc, tcounts, t_stride, batch, idx, dist, dist2, pred, plevel);
}

// ---- map-point fusion search --------------------------------------------------------------

PISLAM_EXPORT int pislam_match_fuse_reserve(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                            const int32_t *scale_q16, const int32_t *radius_far,
                                            const int32_t *radius_near, int level_below, int level_above, size_t t_stride,
                                            int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  pjm::Tables tab;
  PCHK(projection_plan(c, words, levels, nlevels, scale_q16, radius_far, radius_near, level_below, level_above, t_stride,
                       batch, &P, &tab));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_fuse, (size_t)P.ncells + 1, sizeof(uint2), words, t_stride, batch,
                         "hipMalloc(fuse matcher workspace)");
}

PISLAM_EXPORT int pislam_match_fuse_batch(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                          const int32_t *scale_q16, const float *level_scale, const int32_t *radius_far,
                                          const int32_t *radius_near, const pislam_projection_params *p,
                                          const float *inv_sigma2, const pislam_fuse_params *f, const float *pose,
                                          const float *cam, const float *xw, const float *normal, const float *drange,
                                          const uint8_t *qlevel, const uint8_t *qmask, const uint32_t *qdesc,
                                          const uint32_t *qcounts, size_t q_stride, const uint32_t *tkp,
                                          const uint32_t *tdesc, const int32_t *tobs_q8, const uint32_t *tcounts,
                                          size_t t_stride, int batch, int32_t *idx, uint32_t *dist, uint32_t *dist2,
                                          int32_t *pred, uint8_t *plevel) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!f) return fail(c, PISLAM_ERR_INVALID, "null fuse parameters");
  if (!(f->chi2_mono > 0.0f) || !(f->chi2_stereo > 0.0f))      // (a NaN fails; +inf passes)
    return fail(c, PISLAM_ERR_INVALID, "chi2_mono and chi2_stereo must be > 0");
  if (nlevels < 1 || nlevels > pm::WIN_MAX_LEVELS) return fail(c, PISLAM_ERR_INVALID, "nlevels must be 1..16");
  if (!inv_sigma2) return fail(c, PISLAM_ERR_INVALID, "null inv_sigma2");
  pj::FuseArgs fz{};
  for (int l = 0; l < nlevels; l++) {
    if (!(inv_sigma2[l] > 0.0f) || !psm::finite_f(inv_sigma2[l]))
      return fail(c, PISLAM_ERR_INVALID, "inv_sigma2 must be finite and > 0");
    fz.inv_sigma2[l] = inv_sigma2[l];
  }
  fz.tobs = tobs_q8, fz.qmask = qmask, fz.chi2_mono = f->chi2_mono, fz.chi2_stereo = f->chi2_stereo;
  return projection_call(c, c->w_fuse, "hipMalloc(fuse matcher workspace)", &fz, words, levels, nlevels, scale_q16,
                         level_scale, radius_far, radius_near, p, pose, cam, xw, normal, drange, qlevel, qdesc, qcounts,
                         q_stride, tkp, tdesc, tcounts, t_stride, batch, idx, dist, dist2, pred, plevel);
}

// ---- rectified stereo matching ------------------------------------------------------------

namespace {

// Checks the arguments every stereo call shares and lays out the right keypoints' cell grids (host only): the scaled
// window matcher's plan at span 0 with radius0 = row_radius0, so that level lr's cells are max(1, row_radius0[lr])
// level-0 pixels (coarsened to fit pm::WIN_MAX_CELLS), then the level span of the band search.
int stereo_plan(pislam_ctx *c, int words, const pislam_level *lv, int nlevels, const int32_t *scale_q16,
                const int32_t *row_radius0, const pislam_stereo_params *p, size_t r_stride, int batch, pm::ScaledPlan *P) {
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null stereo parameters");
  PCHK(scaled_plan(c, words, lv, nlevels, scale_q16, row_radius0, 0, r_stride, batch, P));
  if (p->level_span < 0 || p->level_span > nlevels - 1) return fail(c, PISLAM_ERR_INVALID, "level_span must be 0..nlevels-1");
  if (p->min_disp < 0 || p->min_disp > p->max_disp || p->max_disp > 65535)
    return fail(c, PISLAM_ERR_INVALID, "need 0 <= min_disp <= max_disp <= 65535");
  if (p->max_hamming < 0) return fail(c, PISLAM_ERR_INVALID, "max_hamming must be >= 0");
  if (p->sad_radius < 1 || p->sad_radius > pm::ST_MAX_W) return fail(c, PISLAM_ERR_INVALID, "sad_radius must be 1..7");
  if (p->search_radius < 1 || p->search_radius > pm::ST_MAX_L) return fail(c, PISLAM_ERR_INVALID, "search_radius must be 1..8");
  if (p->median_filter != 0 && p->median_filter != 1) return fail(c, PISLAM_ERR_INVALID, "median_filter must be 0 or 1");
  P->span = p->level_span;
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_match_stereo_reserve(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                              const int32_t *scale_q16, const int32_t *row_radius0,
                                              const pislam_stereo_params *p, size_t r_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(stereo_plan(c, words, levels, nlevels, scale_q16, row_radius0, p, r_stride, batch, &P));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_st, (size_t)P.ncells + 1, sizeof(uint2), words, r_stride, batch,
                         "hipMalloc(stereo matcher workspace)");
}

PISLAM_EXPORT int pislam_match_stereo_batch(pislam_ctx *c, int words, const pislam_level *levels, int nlevels,
                                            const int32_t *scale_q16, const int32_t *row_radius0,
                                            const pislam_stereo_params *p, const uint8_t *left_pyr,
                                            const uint8_t *right_pyr, int vstep, int rows, size_t pyramid_stride,
                                            const uint32_t *lkp, const uint32_t *ldesc, const uint32_t *lcounts,
                                            size_t l_stride, const uint32_t *rkp, const uint32_t *rdesc,
                                            const uint32_t *rcounts, size_t r_stride, int batch, int32_t *idx,
                                            uint32_t *dist, int32_t *disp_q8, uint32_t *sad, uint32_t *nstereo) {
  if (!c) return PISLAM_ERR_INVALID;
  pm::ScaledPlan P;
  PCHK(stereo_plan(c, words, levels, nlevels, scale_q16, row_radius0, p, r_stride, batch, &P));
  if (vstep < 1 || rows < 1) return fail(c, PISLAM_ERR_INVALID, "vstep and rows must be positive");
  for (int l = 0; l < nlevels; l++)
    if (levels[l].col0 + levels[l].width > vstep || levels[l].row0 + levels[l].height > rows)
      return fail(c, PISLAM_ERR_INVALID, "a level rectangle lies outside [0, rows) x [0, vstep)");
  if (l_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "l_stride too large");
  if (nstereo && !is_device_ptr(nstereo)) return fail(c, PISLAM_ERR_INVALID, "nstereo must be a device pointer or null");
  if (batch == 0 || (l_stride == 0 && !nstereo)) return PISLAM_OK;
  PCHK(device_ptrs(c, {left_pyr, right_pyr, lkp, ldesc, lcounts, rkp, rdesc, rcounts, idx, dist, disp_q8, sad},
                   "the stereo matcher takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, c->w_st, (size_t)P.ncells + 1, sizeof(uint2), words, r_stride, batch,
                       "hipMalloc(stereo matcher workspace)"));
  if (l_stride > 0) {
    const pislam_ctx::CellIndex &w = c->w_st;
    PCHK(launch_scaled_index(c, w, P, words, rkp, rdesc, rcounts, r_stride, batch));
    const dim3 grid = query_grid(c, l_stride, pm::WIN_QPW, batch);
    with_words(words, [&](auto wd) {
      hipLaunchKernelGGL(pm::k_match_stereo<decltype(wd)::value>, grid, dim3(pm::WIN_THREADS), 0, c->stream, P, p->min_disp,
                         p->max_disp, lkp, ldesc, lcounts, l_stride, r_stride, w.off.as<uint32_t>(), w.meta.as<uint2>(),
                         w.desc.as<uint32_t>(), idx, dist);
    });
    PCHK(launch_ok(c, "k_match_stereo"));
    const dim3 rgrid = query_grid(c, l_stride, pm::ST_QPW, batch);
    with_sad_radius(p->sad_radius, [&](auto r) {
      hipLaunchKernelGGL(pm::k_stereo_refine<decltype(r)::value>, rgrid, dim3(pm::ST_THREADS), 0, c->stream, P,
                         (uint32_t)p->max_hamming, p->search_radius, p->min_disp, p->max_disp, left_pyr, right_pyr, vstep,
                         pyramid_stride, lkp, lcounts, l_stride, rkp, r_stride, idx, dist, disp_q8, sad);
    });
    PCHK(launch_ok(c, "k_stereo_refine"));
  }
  if (p->median_filter || nstereo) {
    hipLaunchKernelGGL(pm::k_stereo_median, dim3((unsigned)batch), dim3(pm::ST_MEDIAN_THREADS), 0, c->stream,
                       p->median_filter, lcounts, l_stride, disp_q8, sad, nstereo);
    PCHK(launch_ok(c, "k_stereo_median"));
  }
  return PISLAM_OK;
}

// ---- pyramidal Lucas-Kanade tracking and match refinement ----------------------------------

namespace {

// nullptr, or what is wrong with the parameters and tables of a tracking call (host only).
const char *lk_check_tables(const pislam_lk_params *p, const pislam_level *lv, int nlevels, const int32_t *scale_q16,
                            int vstep, int rows) {
  if (!p) return "null tracking parameters";
  if (p->win_radius < 1 || p->win_radius > pt::LK_MAX_W) return "win_radius must be 1..7";
  if (p->max_iters < 1 || p->max_iters > 32) return "max_iters must be 1..32";
  if (p->eps_q8 < 0 || p->eps_q8 > 255) return "eps_q8 must be 0..255";
  if (p->max_step_q8 < 1 || p->max_step_q8 > 4096) return "max_step_q8 must be 1..4096";
  if (p->level_step < 1 || p->level_step > 15) return "level_step must be 1..15";
  if (p->max_coarse < 0 || p->max_coarse > 15) return "max_coarse must be 0..15";
  if (p->min_eig < 0 || p->min_eig > (1 << 20)) return "min_eig must be 0..2^20";
  if (p->max_err < 0 || p->max_err > 8160) return "max_err must be 0..8160";
  if (nlevels < 1 || nlevels > pt::LK_MAX_LEVELS) return "nlevels must be 1..16";
  if (!lv || !scale_q16) return "null levels / scale_q16";
  if (vstep < 1 || rows < 1) return "vstep and rows must be positive";
  for (int l = 0; l < nlevels; l++) {
    const pislam_level &L = lv[l];
    if (L.width < 1 || L.height < 1 || L.col0 < 0 || L.row0 < 0 || L.col0 + L.width > 4096 || L.row0 + L.height > 4096)
      return "level rectangles must be non-empty and fit 12-bit coordinates";
    if (L.col0 + L.width > vstep || L.row0 + L.height > rows) return "a level rectangle lies outside [0, rows) x [0, vstep)";
    if (scale_q16[l] < 1 || scale_q16[l] > (1 << 20)) return "scale_q16 must be 1..2^20";
    const long long ex = ((long long)(L.width - 1) * scale_q16[l] + 32768) >> 16;
    const long long ey = ((long long)(L.height - 1) * scale_q16[l] + 32768) >> 16;
    if (ex > 65535 || ey > 65535) return "a level's mapped extent exceeds 65535";
    for (int k = 0; k < l; k++) {
      const pislam_level &K = lv[k];
      if (L.col0 < K.col0 + K.width && K.col0 < L.col0 + L.width && L.row0 < K.row0 + K.height && K.row0 < L.row0 + L.height)
        return "level rectangles overlap";
    }
  }
  return nullptr;
}

struct LkRange {
  const void *p;
  size_t n;
};
bool lk_overlap(LkRange a, LkRange b) {
  const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
  return a.p && b.p && a.n && b.n && pa < pb + b.n && pb < pa + a.n;
}
// What is wrong with a call's byte ranges, or null: no output may overlap an input or another output (a null or empty
// range overlaps nothing).  The one alias a call allows, out[0] on in[alias_in] when both begin at the same address
// (each item is read before it is written), is passed as alias_in.
template <size_t NI, size_t NO>
const char *ranges_overlap(const LkRange (&in)[NI], const LkRange (&out)[NO], int alias_in = -1) {
  for (size_t o = 0; o < NO; o++) {
    for (size_t i = 0; i < NI; i++) {
      if (o == 0 && (int)i == alias_in && out[o].p == in[i].p) continue;
      if (lk_overlap(out[o], in[i])) return "an output overlaps an input";
    }
    for (size_t k = 0; k < o; k++)
      if (lk_overlap(out[o], out[k])) return "two outputs overlap";
  }
  return nullptr;
}

// The level table of the pose, PnP and Sim(3) calls, checked when the call has levels; `needs` opens the caller's text.
int check_level_table(pislam_ctx *c, const char *needs, const float *inv_sigma2, int nlevels) {
  if (!inv_sigma2 || nlevels < 1 || nlevels > pq::MAX_LEVELS)
    return fail(c, PISLAM_ERR_INVALID, (std::string(needs) + " inv_sigma2 with 1..16 entries").c_str());
  for (int l = 0; l < nlevels; l++)
    if (!(inv_sigma2[l] > 0.0f) || !psm::finite_f(inv_sigma2[l]))
      return fail(c, PISLAM_ERR_INVALID, "inv_sigma2 must be finite and > 0");
  return PISLAM_OK;
}
// ... and copied into the kernel's arguments: nlevels is 0 for a call without levels.
template <class ARGS>
void copy_level_table(ARGS *a, const float *inv_sigma2, int nlevels) {
  a->nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) a->inv_sigma2[l] = inv_sigma2[l];
}
// The level arrays of the two Sim(3) calls: both or neither, and with them the table.
int check_level_pair(pislam_ctx *c, const uint8_t *level1, const uint8_t *level2, const float *inv_sigma2, int nlevels) {
  if ((level1 != nullptr) != (level2 != nullptr)) return fail(c, PISLAM_ERR_INVALID, "level1 and level2 go together");
  return level1 ? check_level_table(c, "levels need", inv_sigma2, nlevels) : PISLAM_OK;
}
// What the two refinement calls check of their schedule, in their order; eps comes after the Sim(3) call's own checks.
int check_refine_schedule(pislam_ctx *c, int rounds, int iters, int huber_rounds, int min_obs) {
  if (rounds < 1 || rounds > 8) return fail(c, PISLAM_ERR_INVALID, "rounds must be 1..8");
  if (iters < 1 || iters > 32) return fail(c, PISLAM_ERR_INVALID, "iters must be 1..32");
  if (huber_rounds < 0 || huber_rounds > rounds) return fail(c, PISLAM_ERR_INVALID, "huber_rounds must be 0..rounds");
  if (min_obs < 3 || min_obs > prf::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "min_obs must be 3..16384");
  return PISLAM_OK;
}
int check_refine_eps(pislam_ctx *c, double eps) {
  return eps >= 0.0 ? PISLAM_OK : fail(c, PISLAM_ERR_INVALID, "eps must be >= 0");
}

}  // namespace

PISLAM_EXPORT int pislam_track_lk_batch(pislam_ctx *c, const pislam_lk_params *p, const pislam_level *levels, int nlevels,
                                        const int32_t *scale_q16, const uint8_t *prev_pyr, const uint8_t *next_pyr,
                                        int vstep, int rows, size_t pyramid_stride, const int32_t *pts_q8,
                                        const uint32_t *counts, const int32_t *guess_q8, size_t stride, int batch,
                                        int32_t *next_q8, uint32_t *status, uint32_t *err, uint32_t *ntracked) {
  if (!c) return PISLAM_ERR_INVALID;
  if (const char *bad = lk_check_tables(p, levels, nlevels, scale_q16, vstep, rows)) return fail(c, PISLAM_ERR_INVALID, bad);
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "stride too large");
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {prev_pyr, next_pyr, pts_q8, counts, next_q8, status, err}, "the tracker takes device pointers only"));
  if (guess_q8 && !is_device_ptr(guess_q8)) return fail(c, PISLAM_ERR_INVALID, "guess_q8 must be a device pointer or null");
  if (ntracked && !is_device_ptr(ntracked)) return fail(c, PISLAM_ERR_INVALID, "ntracked must be a device pointer or null");
  {
    const size_t B = (size_t)batch, pyr = (B - 1) * pyramid_stride + (size_t)rows * (size_t)vstep;
    const size_t words = B * stride * sizeof(uint32_t);
    const LkRange in[] = {{prev_pyr, pyr}, {next_pyr, pyr}, {pts_q8, 2 * words}, {counts, B * sizeof(uint32_t)},
                          {guess_q8, 2 * words}};
    const LkRange out[] = {{next_q8, 2 * words}, {status, words}, {err, words}, {ntracked, B * sizeof(uint32_t)}};
    // next_q8 == guess_q8 is allowed: each point reads its guess before it writes
    if (const char *bad = ranges_overlap(in, out, 4)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pt::LkArgs a{};
  for (int l = 0; l < nlevels; l++)
    a.lv[l] = pt::LkLevel{levels[l].col0, levels[l].row0, levels[l].width, levels[l].height, scale_q16[l]};
  a.nlevels = nlevels, a.max_iters = p->max_iters, a.eps_q8 = p->eps_q8, a.max_step_q8 = p->max_step_q8;
  a.level_step = p->level_step, a.max_coarse = p->max_coarse, a.min_eig = p->min_eig, a.max_err = p->max_err;
  a.vstep = vstep, a.pyramid_stride = pyramid_stride, a.stride = stride;
  for (int b0 = 0; b0 < batch; b0 += 65535) {                // (grid.y)
    const int nb = std::min(batch - b0, 65535);
    const size_t first = (size_t)b0 * stride;
    if (stride > 0) {
      a.prev = prev_pyr + (size_t)b0 * pyramid_stride, a.next = next_pyr + (size_t)b0 * pyramid_stride;
      a.pts = pts_q8 + 2 * first, a.counts = counts + b0, a.guess = guess_q8 ? guess_q8 + 2 * first : nullptr;
      a.next_q8 = next_q8 + 2 * first, a.status = status + first, a.err = err + first;
      const dim3 grid = query_grid(c, stride, pt::LK_PPW, nb);
      static_assert(pt::LK_MAX_W == pm::ST_MAX_W, "with_sad_radius covers 1..7");
      with_sad_radius(p->win_radius, [&](auto w) {
        hipLaunchKernelGGL(pt::k_track_lk<decltype(w)::value>, grid, dim3(pt::LK_THREADS), 0, c->stream, a);
      });
      PCHK(launch_ok(c, "k_track_lk"));
    }
    if (ntracked) {
      hipLaunchKernelGGL(pt::k_lk_count, dim3((unsigned)nb), dim3(pt::LK_COUNT_THREADS), 0, c->stream, counts + b0, stride,
                         status + first, ntracked + b0);
      PCHK(launch_ok(c, "k_lk_count"));
    }
  }
  return PISLAM_OK;
}

// ---- bag of words: vocabulary tree, quantisation, vector, word-guided matching ---------------

struct pislam_vocab {
  int device = 0;
  int words = 0, nnodes = 0, nwords = 0, ngroups = 0;
  DevBuf desc, meta;   // pb::k_bow_descend's node records: descriptors [nnodes][words], (first | word, count | group << 8) [nnodes]
};

PISLAM_EXPORT int pislam_vocab_create(pislam_ctx *c, int words, int nnodes, const uint32_t *node_desc,
                                      const int32_t *first_child, const int32_t *child_count, int group_depth,
                                      pislam_vocab **vocab) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!vocab) return fail(c, PISLAM_ERR_INVALID, "null vocabulary pointer");
  *vocab = nullptr;
  PCHK(check_words(c, words));
  if (nnodes < 2 || nnodes > (1 << 24)) return fail(c, PISLAM_ERR_INVALID, "nnodes must be 2..2^24");
  if (group_depth < 0 || group_depth > pb::BOW_MAX_DEPTH) return fail(c, PISLAM_ERR_INVALID, "group_depth must be 0..16");
  if (!node_desc || !first_child || !child_count) return fail(c, PISLAM_ERR_INVALID, "null node_desc / first_child / child_count");
  // children lie strictly after their parent, so one ascending pass sees a parent before its children
  std::vector<int32_t> parent((size_t)nnodes, -1);
  for (int n = 0; n < nnodes; n++) {
    const int64_t cc = child_count[n], fc = first_child[n];
    if (cc < 0 || cc > pb::BOW_MAX_CHILDREN) return fail(c, PISLAM_ERR_INVALID, "child_count must be 0..32");
    if (cc == 0) continue;
    if (fc <= n || fc < 1 || fc + cc > nnodes)
      return fail(c, PISLAM_ERR_INVALID, "a child range must lie after its parent and inside [1, nnodes)");
    for (int64_t k = fc; k < fc + cc; k++) {
      if (parent[(size_t)k] >= 0) return fail(c, PISLAM_ERR_INVALID, "child ranges overlap");
      parent[(size_t)k] = n;
    }
  }
  if (child_count[0] == 0) return fail(c, PISLAM_ERR_INVALID, "the root must not be a leaf");
  for (int n = 1; n < nnodes; n++)
    if (parent[(size_t)n] < 0) return fail(c, PISLAM_ERR_INVALID, "a node other than the root is nobody's child");
  std::vector<uint8_t> depth((size_t)nnodes, 0);
  std::vector<uint2> meta((size_t)nnodes);
  std::vector<uint32_t> grp((size_t)nnodes, 0);       // group id of the nodes at and below the group nodes
  int nwords = 0, ngroups = 0;
  for (int n = 0; n < nnodes; n++) {
    const int d = n ? depth[(size_t)parent[(size_t)n]] + 1 : 0;
    if (d > pb::BOW_MAX_DEPTH) return fail(c, PISLAM_ERR_INVALID, "the tree is deeper than 16");
    depth[(size_t)n] = (uint8_t)d;
    const bool leaf = child_count[n] == 0;
    if (d == group_depth || (leaf && d < group_depth))
      grp[(size_t)n] = (uint32_t)ngroups++;
    else if (d > group_depth)
      grp[(size_t)n] = grp[(size_t)parent[(size_t)n]];
    meta[(size_t)n] = leaf ? make_uint2((uint32_t)nwords++, grp[(size_t)n] << 8)
                           : make_uint2((uint32_t)first_child[n], (uint32_t)child_count[n]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pislam_vocab *v = new pislam_vocab();
  v->device = c->device;
  v->words = words, v->nnodes = nnodes, v->nwords = nwords, v->ngroups = ngroups;
  const size_t dbytes = sizeof(uint32_t) * (size_t)words * nnodes, mbytes = sizeof(uint2) * (size_t)nnodes;
  if (v->desc.ensure(dbytes) != PISLAM_OK || v->meta.ensure(mbytes) != PISLAM_OK) {
    v->desc.release(), v->meta.release();
    delete v;
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(vocabulary)");
  }
  hipError_t e = hipMemcpyAsync(v->desc.p, node_desc, dbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(v->meta.p, meta.data(), mbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host arrays may go away after the call)
  if (e != hipSuccess) {
    v->desc.release(), v->meta.release();
    delete v;
    return fail(c, PISLAM_ERR_HIP, "vocabulary upload", e);
  }
  *vocab = v;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_vocab_destroy(pislam_vocab *v) {
  if (!v) return PISLAM_ERR_INVALID;
  (void)hipSetDevice(v->device);
  v->desc.release(), v->meta.release();
  delete v;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_vocab_nwords(const pislam_vocab *v) { return v ? v->nwords : PISLAM_ERR_INVALID; }
PISLAM_EXPORT int pislam_vocab_ngroups(const pislam_vocab *v) { return v ? v->ngroups : PISLAM_ERR_INVALID; }

PISLAM_EXPORT int pislam_bow_transform_batch(pislam_ctx *c, const pislam_vocab *v, const uint32_t *desc,
                                             const uint32_t *counts, size_t stride, int batch, uint32_t *word,
                                             uint32_t *group, uint32_t *wdist) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!v) return fail(c, PISLAM_ERR_INVALID, "null vocabulary");
  if (v->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the vocabulary lives on another device");
  PCHK(check_batch(c, batch));
  if (stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "stride too large");
  if (group && !is_device_ptr(group)) return fail(c, PISLAM_ERR_INVALID, "group must be a device pointer or null");
  if (wdist && !is_device_ptr(wdist)) return fail(c, PISLAM_ERR_INVALID, "wdist must be a device pointer or null");
  if (batch == 0 || stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {desc, counts, word}, "the bag-of-words transform takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  const dim3 grid = query_grid(c, stride, pb::BOW_DPW, batch);
  const uint32_t *nd = v->desc.as<uint32_t>();
  const uint2 *nm = v->meta.as<uint2>();
  with_words(v->words, [&](auto w) {
    hipLaunchKernelGGL(pb::k_bow_descend<decltype(w)::value>, grid, dim3(pb::BOW_THREADS), 0, c->stream, nd, nm, desc, counts,
                       stride, word, group, wdist);
  });
  return launch_ok(c, "k_bow_descend");
}

PISLAM_EXPORT int pislam_bow_vector_batch(pislam_ctx *c, const uint32_t *word, const uint32_t *counts, size_t stride,
                                          int batch, uint32_t *bow_word, uint32_t *bow_tf, uint32_t *bow_n) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(check_batch(c, batch));
  if (stride > (size_t)pb::BOW_VEC_MAX) return fail(c, PISLAM_ERR_INVALID, "stride must be at most 16384");
  if (batch == 0) return PISLAM_OK;
  if (stride == 0) {                                    // no slot to read or write but the numbers
    PCHK(device_ptrs(c, {counts, bow_n}, "the bag-of-words vector takes device pointers only"));
  } else {
    PCHK(device_ptrs(c, {word, counts, bow_word, bow_tf, bow_n}, "the bag-of-words vector takes device pointers only"));
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(pb::k_bow_vector, dim3((unsigned)batch), dim3(pb::BOW_VEC_THREADS), 0, c->stream, word, counts, stride,
                     bow_word, bow_tf, bow_n);
  return launch_ok(c, "k_bow_vector");
}

namespace {

int bow_match_args(pislam_ctx *c, int words, int ngroups, size_t t_stride, int batch) {
  PCHK(check_words(c, words));
  if (ngroups < 1 || ngroups > pb::BOW_MAX_GROUPS) return fail(c, PISLAM_ERR_INVALID, "ngroups must be 1..16384");
  PCHK(check_train_stride(c, t_stride, "at most 65535 train entries per pair"));
  return check_batch(c, batch);
}

}  // namespace

PISLAM_EXPORT int pislam_match_bow_reserve(pislam_ctx *c, int words, int ngroups, size_t t_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(bow_match_args(c, words, ngroups, t_stride, batch));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_bow, (size_t)ngroups + 1, sizeof(uint32_t), words, t_stride, batch,
                         "hipMalloc(word-guided matcher workspace)");
}

PISLAM_EXPORT int pislam_match_hamming_bow_batch(pislam_ctx *c, int words, int ngroups, const uint32_t *qdesc,
                                                 const uint32_t *qgroup, const uint32_t *qcounts, size_t q_stride,
                                                 const uint32_t *tdesc, const uint32_t *tgroup, const uint32_t *tcounts,
                                                 size_t t_stride, int batch, int32_t *idx, uint32_t *dist,
                                                 uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(bow_match_args(c, words, ngroups, t_stride, batch));
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {qdesc, qgroup, qcounts, tdesc, tgroup, tcounts, idx, dist, dist2},
                   "the word-guided matcher takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, c->w_bow, (size_t)ngroups + 1, sizeof(uint32_t), words, t_stride, batch,
                       "hipMalloc(word-guided matcher workspace)"));
  uint32_t *off = c->w_bow.off.as<uint32_t>(), *eidx = c->w_bow.meta.as<uint32_t>(), *edesc = c->w_bow.desc.as<uint32_t>();
  hipLaunchKernelGGL(pb::k_bow_index, dim3((unsigned)batch), dim3(pm::WIN_INDEX_THREADS), 0, c->stream, (uint32_t)ngroups,
                     words, tgroup, tdesc, tcounts, t_stride, off, eidx, edesc);
  PCHK(launch_ok(c, "k_bow_index"));
  const dim3 grid = query_grid(c, q_stride, pm::WIN_QPW, batch);
  with_words(words, [&](auto w) {
    hipLaunchKernelGGL(pb::k_match_bow<decltype(w)::value>, grid, dim3(pm::WIN_THREADS), 0, c->stream, (uint32_t)ngroups, qdesc,
                       qgroup, qcounts, q_stride, t_stride, off, eidx, edesc, idx, dist, dist2);
  });
  return launch_ok(c, "k_match_bow");
}

// ---- epipolar search between two key frames -------------------------------------------------

PISLAM_EXPORT int pislam_epipolar_from_poses(const float *pose1, const float *pose2, const float *cam1, const float *cam2,
                                             float *f12, float *epipole) {
  return pem::epipolar_from_poses(pose1, pose2, cam1, cam2, f12, epipole) ? PISLAM_OK : PISLAM_ERR_INVALID;
}

namespace {

int epipolar_tables(pislam_ctx *c, const float *level_sigma2, const float *level_scale, int nlevels, pem::Tables *tab) {
  if (!level_sigma2 || !level_scale || nlevels < 1 || nlevels > pem::MAX_LEVELS)
    return fail(c, PISLAM_ERR_INVALID, "level_sigma2 and level_scale need 1..16 entries");
  *tab = pem::Tables{};
  tab->nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) {
    if (!(level_sigma2[l] > 0.0f) || !psm::finite_f(level_sigma2[l]) || !(level_scale[l] > 0.0f) ||
        !psm::finite_f(level_scale[l]))
      return fail(c, PISLAM_ERR_INVALID, "level_sigma2 and level_scale must be finite and > 0");
    if (l > 0 && level_scale[l] < level_scale[l - 1]) return fail(c, PISLAM_ERR_INVALID, "level_scale must not decrease");
    tab->level_sigma2[l] = level_sigma2[l], tab->level_scale[l] = level_scale[l];
  }
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_match_epipolar_reserve(pislam_ctx *c, int words, int ngroups, size_t t_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(bow_match_args(c, words, ngroups, t_stride, batch));
  HIPCHK(c, hipSetDevice(c->device));
  return index_workspace(c, c->w_epi, (size_t)ngroups + 1, sizeof(pe::Ent), words, t_stride, batch,
                         "hipMalloc(epipolar matcher workspace)");
}

PISLAM_EXPORT int pislam_match_hamming_epipolar_batch(
    pislam_ctx *c, int words, int ngroups, const pislam_epipolar_params *p, const float *level_sigma2,
    const float *level_scale, int nlevels, const float *f12, const float *epipole, const uint32_t *qdesc,
    const uint32_t *qgroup, const int32_t *qobs_q8, const uint8_t *qlevel, const uint8_t *qmask, const uint32_t *qcounts,
    size_t q_stride, const uint32_t *tdesc, const uint32_t *tgroup, const int32_t *tobs_q8, const uint8_t *tlevel,
    const uint8_t *tmask, const uint32_t *tcounts, size_t t_stride, int batch, int32_t *idx, uint32_t *dist,
    uint32_t *dist2) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(bow_match_args(c, words, ngroups, t_stride, batch));
  if (q_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "q_stride too large");
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  const pem::Params prm{p->chi2, p->epipole_r2};
  if (!pem::params_ok(prm)) return fail(c, PISLAM_ERR_INVALID, "chi2 must be > 0 and epipole_r2 >= 0");
  pem::Tables tab;
  PCHK(epipolar_tables(c, level_sigma2, level_scale, nlevels, &tab));
  if (batch == 0 || q_stride == 0) return PISLAM_OK;
  const char *what = "the epipolar matcher takes device pointers only";
  PCHK(device_ptrs(c, {f12, epipole, qdesc, qgroup, qobs_q8, qlevel, qcounts, tdesc, tgroup, tobs_q8, tlevel, tcounts, idx,
                       dist, dist2}, what));
  if ((qmask && !is_device_ptr(qmask)) || (tmask && !is_device_ptr(tmask))) return fail(c, PISLAM_ERR_INVALID, what);
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(index_workspace(c, c->w_epi, (size_t)ngroups + 1, sizeof(pe::Ent), words, t_stride, batch,
                       "hipMalloc(epipolar matcher workspace)"));
  pe::EpiArgs a{};
  a.ngroups = (uint32_t)ngroups;
  a.qdesc = qdesc, a.qgroup = qgroup, a.qcount = qcounts, a.qobs = qobs_q8, a.qlevel = qlevel, a.qmask = qmask;
  a.tdesc = tdesc, a.tgroup = tgroup, a.tcount = tcounts, a.tobs = tobs_q8, a.tlevel = tlevel, a.tmask = tmask;
  a.f12 = f12, a.epipole = epipole, a.q_stride = q_stride, a.t_stride = t_stride;
  a.grp_off = c->w_epi.off.as<uint32_t>(), a.ent = c->w_epi.meta.as<pe::Ent>(), a.ent_desc = c->w_epi.desc.as<uint32_t>();
  a.idx = idx, a.dist = dist, a.dist2 = dist2;
  hipLaunchKernelGGL(pe::k_epi_index, dim3((unsigned)batch), dim3(pm::WIN_INDEX_THREADS), 0, c->stream, words, nlevels, a);
  PCHK(launch_ok(c, "k_epi_index"));
  const dim3 grid = query_grid(c, q_stride, pm::WIN_QPW, batch);
  with_words(words, [&](auto w) {
    hipLaunchKernelGGL(pe::k_match_epipolar<decltype(w)::value>, grid, dim3(pm::WIN_THREADS), 0, c->stream, tab, prm, a);
  });
  return launch_ok(c, "k_match_epipolar");
}

// ---- image preparation: lens undistortion and stereo rectification as a mesh warp ----------

struct pislam_warp {
  int device = 0;
  int width = 0, height = 0, src_width = 0, src_height = 0, log_cell = 0, border = 0;
  int32_t mesh_w = 0, mesh_h = 0;
  int tiles_x = 0, ntiles = 0, staged = 0, direct = 0;
  DevBuf mesh, tiles;   // pw::k_warp's tables: mesh_x then mesh_y int32 [mesh_h][mesh_w], pw::Tile [ntiles]
};

PISLAM_EXPORT int pislam_warp_mesh_dims(int width, int height, int log_cell, int32_t *mesh_w, int32_t *mesh_h) {
  return pw::mesh_dims(width, height, log_cell, mesh_w, mesh_h) ? PISLAM_OK : PISLAM_ERR_INVALID;
}

PISLAM_EXPORT int pislam_warp_create(pislam_ctx *c, int width, int height, int src_width, int src_height, int log_cell,
                                     const int32_t *mesh_x, const int32_t *mesh_y, int border, pislam_warp **warp) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!warp) return fail(c, PISLAM_ERR_INVALID, "null warp pointer");
  *warp = nullptr;
  if (const char *bad = pw::check_create(width, height, src_width, src_height, log_cell, mesh_x, mesh_y, border))
    return fail(c, PISLAM_ERR_INVALID, bad);
  const pw::Plan plan = pw::make_plan(width, height, src_width, src_height, log_cell, mesh_x, mesh_y);
  HIPCHK(c, hipSetDevice(c->device));
  pislam_warp *w = new pislam_warp();
  w->device = c->device;
  w->width = width, w->height = height, w->src_width = src_width, w->src_height = src_height;
  w->log_cell = log_cell, w->border = border;
  pw::mesh_dims(width, height, log_cell, &w->mesh_w, &w->mesh_h);
  w->tiles_x = plan.tiles_x, w->ntiles = (int)plan.tiles.size(), w->staged = plan.staged, w->direct = plan.direct;
  const size_t nbytes = sizeof(int32_t) * (size_t)w->mesh_w * w->mesh_h, tbytes = sizeof(pw::Tile) * plan.tiles.size();
  if (w->mesh.ensure(2 * nbytes) != PISLAM_OK || w->tiles.ensure(tbytes) != PISLAM_OK) {
    w->mesh.release(), w->tiles.release();
    delete w;
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(warp)");
  }
  hipError_t e = hipMemcpyAsync(w->mesh.p, mesh_x, nbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(w->mesh.as<uint8_t>() + nbytes, mesh_y, nbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(w->tiles.p, plan.tiles.data(), tbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host arrays and the plan may go away after the call)
  if (e != hipSuccess) {
    w->mesh.release(), w->tiles.release();
    delete w;
    return fail(c, PISLAM_ERR_HIP, "warp upload", e);
  }
  *warp = w;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_warp_destroy(pislam_warp *w) {
  if (!w) return PISLAM_ERR_INVALID;
  (void)hipSetDevice(w->device);
  w->mesh.release(), w->tiles.release();
  delete w;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_warp_info(const pislam_warp *w, int32_t info[4]) {
  if (!w || !info) return PISLAM_ERR_INVALID;
  info[0] = w->ntiles, info[1] = w->staged, info[2] = w->direct, info[3] = pw::LDS_BYTES;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_warp_batch(pislam_ctx *c, const pislam_warp *w, const uint8_t *src, int src_vstep,
                                    size_t src_stride, uint8_t *dst, int dst_vstep, size_t dst_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!w) return fail(c, PISLAM_ERR_INVALID, "null warp");
  if (w->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the warp lives on another device");
  if (const char *bad = pw::check_batch(w->width, w->height, w->src_width, w->src_height, src, src_vstep, src_stride, dst,
                                        dst_vstep, dst_stride, batch))
    return fail(c, PISLAM_ERR_INVALID, bad);
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {src, dst}, "the mesh warp takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  pw::WarpArgs a{};
  a.tiles = w->tiles.as<pw::Tile>();
  a.mesh_x = w->mesh.as<int32_t>(), a.mesh_y = a.mesh_x + (size_t)w->mesh_w * w->mesh_h;
  a.mesh_w = w->mesh_w, a.log_cell = w->log_cell, a.width = w->width, a.height = w->height;
  a.src_width = w->src_width, a.src_height = w->src_height, a.border = w->border, a.tiles_x = w->tiles_x;
  a.direct = c->opt.warp_direct;
  a.src_vstep = src_vstep, a.src_stride = src_stride, a.dst_vstep = dst_vstep, a.dst_stride = dst_stride;
  for (int b0 = 0; b0 < batch; b0 += 65535) {                // (grid.y)
    const int nb = std::min(batch - b0, 65535);
    a.src = src + (size_t)b0 * src_stride, a.dst = dst + (size_t)b0 * dst_stride;
    hipLaunchKernelGGL(pw::k_warp, dim3((unsigned)w->ntiles, (unsigned)nb), dim3(pw::THREADS), 0, c->stream, a);
    PCHK(launch_ok(c, "k_warp"));
  }
  return PISLAM_OK;
}

// ---- image preparation: contrast-limited adaptive histogram equalisation -------------------

namespace {

const char *clahe_check_params(const pislam_clahe_params *p) {
  if (!p) return "null params";
  return pc::check_params(p->width, p->height, p->tiles_x, p->tiles_y, p->clip_q8);
}

// The checked arguments of one of the three calls, as kernel arguments for the whole batch.
int clahe_args(pislam_ctx *c, const pislam_clahe_params *p, const uint8_t *src, int src_vstep, size_t src_stride,
               uint8_t *dst, int dst_vstep, size_t dst_stride, uint8_t *luts, int batch, bool use_src, bool use_dst,
               pc::Args *a) {
  if (const char *bad = clahe_check_params(p)) return fail(c, PISLAM_ERR_INVALID, bad);
  if (const char *bad = pc::check_call(p->width, p->height, pislam_clahe_lut_size(p), src, src_vstep, src_stride, dst,
                                       dst_vstep, dst_stride, luts, batch, use_src, use_dst))
    return fail(c, PISLAM_ERR_INVALID, bad);
  if (batch == 0) return PISLAM_OK;
  if (use_src && !is_device_ptr(src)) return fail(c, PISLAM_ERR_INVALID, "CLAHE takes device pointers only");
  if (use_dst && !is_device_ptr(dst)) return fail(c, PISLAM_ERR_INVALID, "CLAHE takes device pointers only");
  if (!is_device_ptr(luts)) return fail(c, PISLAM_ERR_INVALID, "CLAHE takes device pointers only");
  *a = pc::geometry(p->width, p->height, p->tiles_x, p->tiles_y, p->clip_q8);
  a->src = src, a->src_vstep = src_vstep, a->src_stride = src_stride;
  a->dst = dst, a->dst_vstep = dst_vstep, a->dst_stride = dst_stride;
  a->luts = luts;
  return PISLAM_OK;
}

// One launch per 65535 frames (grid.y); `apply` chooses the kernel.
int clahe_launch(pislam_ctx *c, pc::Args a, int batch, bool apply) {
  HIPCHK(c, hipSetDevice(c->device));
  const size_t ntiles = (size_t)a.tiles_x * a.tiles_y;
  const unsigned gx = apply ? (unsigned)(a.cells_x * a.cells_y * a.chunks) : (unsigned)ntiles;
  const uint8_t *src = a.src;
  uint8_t *dst = a.dst, *luts = a.luts;
  for (int b0 = 0; b0 < batch; b0 += 65535) {
    const dim3 grid(gx, (unsigned)std::min(batch - b0, 65535)), block(pc::THREADS);
    a.src = src + (size_t)b0 * a.src_stride, a.luts = luts + (size_t)b0 * ntiles * 256;
    if (apply) a.dst = dst + (size_t)b0 * a.dst_stride;
    if (!apply && c->opt.clahe_combine) hipLaunchKernelGGL(pc::k_clahe_luts<true>, grid, block, 0, c->stream, a);
    else if (!apply) hipLaunchKernelGGL(pc::k_clahe_luts<false>, grid, block, 0, c->stream, a);
    else if (c->opt.clahe_lut_global) hipLaunchKernelGGL(pc::k_clahe_apply<false>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(pc::k_clahe_apply<true>, grid, block, 0, c->stream, a);
    PCHK(launch_ok(c, apply ? "k_clahe_apply" : "k_clahe_luts"));
  }
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT size_t pislam_clahe_lut_size(const pislam_clahe_params *p) {
  return clahe_check_params(p) ? 0 : (size_t)p->tiles_x * (size_t)p->tiles_y * 256;
}

PISLAM_EXPORT int pislam_clahe_luts_batch(pislam_ctx *c, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                                          size_t src_stride, int batch, uint8_t *luts) {
  if (!c) return PISLAM_ERR_INVALID;
  pc::Args a{};
  PCHK(clahe_args(c, p, src, src_vstep, src_stride, nullptr, 0, 0, luts, batch, true, false, &a));
  return batch ? clahe_launch(c, a, batch, false) : PISLAM_OK;
}

PISLAM_EXPORT int pislam_clahe_apply_batch(pislam_ctx *c, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                                           size_t src_stride, const uint8_t *luts, uint8_t *dst, int dst_vstep,
                                           size_t dst_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  pc::Args a{};
  PCHK(clahe_args(c, p, src, src_vstep, src_stride, dst, dst_vstep, dst_stride, const_cast<uint8_t *>(luts), batch, true,
                  true, &a));
  return batch ? clahe_launch(c, a, batch, true) : PISLAM_OK;
}

PISLAM_EXPORT int pislam_clahe_batch(pislam_ctx *c, const pislam_clahe_params *p, const uint8_t *src, int src_vstep,
                                     size_t src_stride, uint8_t *dst, int dst_vstep, size_t dst_stride, int batch,
                                     uint8_t *luts) {
  if (!c) return PISLAM_ERR_INVALID;
  pc::Args a{};
  PCHK(clahe_args(c, p, src, src_vstep, src_stride, dst, dst_vstep, dst_stride, luts, batch, true, true, &a));
  if (batch == 0) return PISLAM_OK;
  PCHK(clahe_launch(c, a, batch, false));
  return clahe_launch(c, a, batch, true);
}

// ---- after the match: batched angle bins and match selection ------------------------------

PISLAM_EXPORT int pislam_orb_angles_batch(pislam_ctx *c, const uint8_t *pyramids, int vstep, int rows,
                                          size_t pyramid_stride, const uint32_t *keypoints, const uint32_t *counts,
                                          size_t stride, int batch, uint8_t *angles) {
  if (!c) return PISLAM_ERR_INVALID;
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (vstep < 31 || rows < 31) return fail(c, PISLAM_ERR_INVALID, "vstep and rows must hold a 31 x 31 patch");
  if (stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "stride too large");
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {pyramids, keypoints, counts, angles}, "the batched angle call takes device pointers only"));
  if (stride == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  for (int b0 = 0; b0 < batch; b0 += 65535) {                // (grid.y)
    const int nb = std::min(batch - b0, 65535);
    const dim3 grid = query_grid(c, stride, 4, nb);
    hipLaunchKernelGGL(pk::k_orb_angles, grid, dim3(256), 0, c->stream, pyramids + (size_t)b0 * pyramid_stride, vstep, rows,
                       pyramid_stride, keypoints + (size_t)b0 * stride, counts + b0, stride, angles + (size_t)b0 * stride);
    PCHK(launch_ok(c, "k_orb_angles"));
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_match_select_batch(pislam_ctx *c, const pislam_select_params *p, const int32_t *idx,
                                            const uint32_t *dist, const uint32_t *dist2, const uint32_t *qcounts,
                                            size_t q_stride, const uint32_t *tcounts, size_t t_stride,
                                            const int32_t *back_idx, const uint8_t *qangle, const uint8_t *tangle,
                                            int batch, int32_t *sel_q, int32_t *sel_t, uint32_t *nsel, uint8_t *status,
                                            uint32_t *rot_hist) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->max_dist < 0 || p->max_dist > 256) return fail(c, PISLAM_ERR_INVALID, "max_dist must be 0..256");
  if (p->ratio_den != 0 && !(1 <= p->ratio_num && p->ratio_num <= p->ratio_den && p->ratio_den <= 65535))
    return fail(c, PISLAM_ERR_INVALID, "the ratio must be off (ratio_den 0) or 1 <= ratio_num <= ratio_den <= 65535");
  if (p->unique != 0 && p->unique != 1) return fail(c, PISLAM_ERR_INVALID, "unique must be 0 or 1");
  if (p->rot_keep < 0 || p->rot_keep > ps::SEL_BINS) return fail(c, PISLAM_ERR_INVALID, "rot_keep must be 0..30");
  if (p->rot_min_pct < 0 || p->rot_min_pct > 100) return fail(c, PISLAM_ERR_INVALID, "rot_min_pct must be 0..100");
  PCHK(check_train_stride(c, t_stride, "at most 65535 train entries per pair"));
  if (q_stride < 1 || q_stride > ((size_t)1 << 22)) return fail(c, PISLAM_ERR_INVALID, "q_stride must be 1..2^22");
  PCHK(check_batch(c, batch));
  if (!dist2 && p->ratio_den != 0) return fail(c, PISLAM_ERR_INVALID, "a ratio test needs dist2");
  if ((p->rot_keep > 0) != (qangle != nullptr) || (p->rot_keep > 0) != (tangle != nullptr))
    return fail(c, PISLAM_ERR_INVALID, "qangle and tangle go with rot_keep > 0, and only with it");
  const char *what = "the match selection takes device pointers only";
  PCHK(device_ptrs(c, {idx, dist, qcounts, tcounts, sel_q, sel_t, nsel}, what));
  for (const void *opt : {(const void *)dist2, (const void *)back_idx, (const void *)qangle, (const void *)tangle,
                          (const void *)status, (const void *)rot_hist})
    if (opt && !is_device_ptr(opt)) return fail(c, PISLAM_ERR_INVALID, what);
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  ps::SelArgs A;
  A.max_dist = p->max_dist, A.ratio_num = (uint32_t)p->ratio_num, A.ratio_den = (uint32_t)p->ratio_den;
  A.unique = p->unique, A.rot_keep = p->rot_keep, A.rot_min_pct = p->rot_min_pct;
  A.idx = idx, A.dist = dist, A.dist2 = p->ratio_den ? dist2 : nullptr;
  A.qcounts = qcounts, A.tcounts = tcounts, A.back_idx = back_idx, A.qangle = qangle, A.tangle = tangle;
  A.q_stride = q_stride, A.t_stride = t_stride;
  A.sel_q = sel_q, A.sel_t = sel_t, A.nsel = nsel, A.status = status, A.rot_hist = rot_hist;
  hipLaunchKernelGGL(ps::k_match_select, dim3((unsigned)batch), dim3(ps::SEL_THREADS), ps::SEL_LDS_BYTES, c->stream, A);
  return launch_ok(c, "k_match_select");
}

// ---- two-view geometry: batched RANSAC for F and H -----------------------------------------

PISLAM_EXPORT int pislam_two_view_ransac_batch(pislam_ctx *c, const pislam_two_view_params *p, const int32_t *p1_q8,
                                               const int32_t *p2_q8, const uint32_t *counts, size_t stride, int batch,
                                               int32_t *best, uint32_t *score, uint32_t *ninliers, uint8_t *inlier,
                                               float *model_n, int64_t *stats) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->model != 0 && p->model != 1) return fail(c, PISLAM_ERR_INVALID, "model must be 0 (fundamental) or 1 (homography)");
  if (p->hypotheses < 1 || p->hypotheses > pgm::MAX_HYP) return fail(c, PISLAM_ERR_INVALID, "hypotheses must be 1..1024");
  if (p->sigma_q8 < 1 || p->sigma_q8 > 4096) return fail(c, PISLAM_ERR_INVALID, "sigma_q8 must be 1..4096");
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)pgm::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {p1_q8, p2_q8, counts, best, score, ninliers, inlier, model_n, stats},
                   "the two-view call takes device pointers only"));
  {
    const size_t B = (size_t)batch, pts = B * stride * 2 * sizeof(int32_t), word = B * sizeof(uint32_t);
    const LkRange in[] = {{p1_q8, pts}, {p2_q8, pts}, {counts, word}};
    const LkRange out[] = {{best, word}, {score, word}, {ninliers, word}, {inlier, B * stride},
                           {model_n, B * 9 * sizeof(float)}, {stats, B * 8 * sizeof(int64_t)}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pg::TvArgs a{};
  a.p1 = p1_q8, a.p2 = p2_q8, a.counts = counts, a.stride = stride, a.batch = batch, a.hypotheses = p->hypotheses;
  a.seed = p->seed, a.sigma = pgm::sigma_px(p->sigma_q8);
  a.best = best, a.score = score, a.ninliers = ninliers, a.inlier = inlier, a.model_n = model_n;
  a.stats = (long long *)stats;
  const dim3 grid((unsigned)std::min(batch, prk::GRID_CAP));
  if (p->model == 0)
    hipLaunchKernelGGL(pg::k_two_view<0>, grid, dim3(prk::THREADS), 0, c->stream, a);
  else
    hipLaunchKernelGGL(pg::k_two_view<1>, grid, dim3(prk::THREADS), 0, c->stream, a);
  return launch_ok(c, "k_two_view");
}

PISLAM_EXPORT int pislam_two_view_denormalise(int model, const float *model_n, const int64_t *stats_row, double out[9]) {
  return pgh::two_view_denormalise(model, model_n, stats_row, out) ? PISLAM_OK : PISLAM_ERR_INVALID;
}

// ---- two-view reconstruction: relative pose and map points ----------------------------------

PISLAM_EXPORT int pislam_two_view_reconstruct_batch(pislam_ctx *c, const pislam_reconstruct_params *p,
                                                    const int32_t *p1_q8, const int32_t *p2_q8, const uint32_t *counts,
                                                    const uint8_t *mask, const float *cam, const float *cand,
                                                    size_t stride, int batch, int32_t *best, uint32_t *status,
                                                    uint32_t *ngood, uint32_t *npar, float *pose_out, float *xw,
                                                    uint8_t *point) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->ncand < 1 || p->ncand > prm::MAX_CAND) return fail(c, PISLAM_ERR_INVALID, "ncand must be 1..8");
  if (p->sigma_q8 < 1 || p->sigma_q8 > 4096) return fail(c, PISLAM_ERR_INVALID, "sigma_q8 must be 1..4096");
  if (!(p->cos_parallax > 0.0f && p->cos_parallax <= 1.0f)) return fail(c, PISLAM_ERR_INVALID, "cos_parallax must be in (0, 1]");
  if (!(p->cos_point > 0.0f && p->cos_point <= 1.0f)) return fail(c, PISLAM_ERR_INVALID, "cos_point must be in (0, 1]");
  if (p->min_good < 1 || p->min_good > prm::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "min_good must be 1..16384");
  if (p->min_good_pct < 0 || p->min_good_pct > 100) return fail(c, PISLAM_ERR_INVALID, "min_good_pct must be 0..100");
  if (p->similar_pct < 1 || p->similar_pct > 100) return fail(c, PISLAM_ERR_INVALID, "similar_pct must be 1..100");
  if (p->parallax_rank < 1 || p->parallax_rank > prm::MAX_STRIDE)
    return fail(c, PISLAM_ERR_INVALID, "parallax_rank must be 1..16384");
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)prm::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the reconstruction call takes device pointers only";
  PCHK(device_ptrs(c, {p1_q8, p2_q8, counts, cam, cand, best, status, ngood, npar, pose_out, xw, point}, what));
  if (mask && !is_device_ptr(mask)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, pts = B * stride * 2 * sizeof(int32_t), word = B * sizeof(uint32_t);
    const LkRange in[] = {{p1_q8, pts}, {p2_q8, pts}, {counts, word}, {cam, B * 4 * sizeof(float)},
                          {cand, B * (size_t)p->ncand * 12 * sizeof(float)}, {mask, B * stride}};
    const LkRange out[] = {{best, word}, {status, word}, {ngood, 8 * word}, {npar, 8 * word},
                           {pose_out, B * 12 * sizeof(float)}, {xw, B * stride * 3 * sizeof(float)}, {point, B * stride}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pr::RcArgs a{};
  a.p1 = p1_q8, a.p2 = p2_q8, a.counts = counts, a.mask = mask, a.cam = cam, a.cand = cand, a.stride = stride;
  a.batch = batch;
  a.p = prm::Params{p->ncand, p->sigma_q8, p->cos_parallax, p->cos_point, p->min_good, p->min_good_pct, p->similar_pct,
                    p->parallax_rank};
  a.best = best, a.status = status, a.ngood = ngood, a.npar = npar, a.pose_out = pose_out, a.xw = xw, a.point = point;
  hipLaunchKernelGGL(pr::k_reconstruct, dim3((unsigned)std::min(batch, pr::RC_GRID_CAP)), dim3(pr::RC_THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_reconstruct");
}

PISLAM_EXPORT int pislam_two_view_decompose(int model, const double m_px[9], const double cam[4], float *cand, int *ncand) {
  return pgh::two_view_decompose(model, m_px, cam, cand, ncand) ? PISLAM_OK : PISLAM_ERR_INVALID;
}

// ---- motion-only pose optimisation from 3D-2D matches ---------------------------------------

PISLAM_EXPORT int pislam_pose_refine_batch(pislam_ctx *c, const pislam_pose_params *p, const float *pose_in,
                                           const float *cam, const float *xw, const int32_t *obs_q8,
                                           const uint32_t *counts, const uint8_t *level, const float *inv_sigma2,
                                           int nlevels, size_t stride, int batch, float *pose_out, uint8_t *inlier,
                                           uint32_t *ninliers, double *cost, uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  PCHK(check_refine_schedule(c, p->rounds, p->iters, p->huber_rounds, p->min_obs));
  PCHK(check_refine_eps(c, p->eps));
  if (level) PCHK(check_level_table(c, "level needs", inv_sigma2, nlevels));
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)pq::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the pose call takes device pointers only";
  PCHK(device_ptrs(c, {pose_in, cam, xw, obs_q8, counts, pose_out, inlier, ninliers, cost, status}, what));
  if (level && !is_device_ptr(level)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), pose = B * 12 * sizeof(float);
    const LkRange in[] = {{pose_in, pose}, {cam, B * 5 * sizeof(float)}, {xw, B * stride * 3 * sizeof(float)},
                          {obs_q8, B * stride * 3 * sizeof(int32_t)}, {counts, word}, {level, B * stride}};
    const LkRange out[] = {{pose_out, pose}, {inlier, B * stride}, {ninliers, word}, {cost, B * sizeof(double)},
                           {status, word}};
    // pose_out == pose_in is allowed: a frame reads its pose before it writes it
    if (const char *bad = ranges_overlap(in, out, 0)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  po::PoArgs a{};
  a.pose_in = pose_in, a.cam = cam, a.xw = xw, a.obs = obs_q8, a.level = level, a.counts = counts, a.stride = stride;
  a.batch = batch;
  copy_level_table(&a, inv_sigma2, level ? nlevels : 0);
  a.p = pq::Params{p->rounds, p->iters, p->huber_rounds, p->min_obs, p->eps};
  a.pose_out = pose_out, a.inlier = inlier, a.ninliers = ninliers, a.status = status, a.cost = cost;
  hipLaunchKernelGGL(po::k_pose_refine, dim3((unsigned)std::min(batch, prf::GRID_CAP)), dim3(prf::THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_pose_refine");
}

// ---- absolute pose from 3D-2D matches: batched P3P RANSAC -----------------------------------

PISLAM_EXPORT int pislam_pnp_ransac_batch(pislam_ctx *c, const pislam_pnp_params *p, const float *cam, const float *xw,
                                          const int32_t *obs_q8, const uint32_t *counts, const uint8_t *level,
                                          const float *inv_sigma2, int nlevels, size_t stride, int batch, int32_t *best,
                                          uint32_t *score, uint32_t *ninliers, uint8_t *inlier, float *pose_out,
                                          uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->hypotheses < 1 || p->hypotheses > pnm::MAX_HYP) return fail(c, PISLAM_ERR_INVALID, "hypotheses must be 1..1024");
  if (p->min_inliers < pnm::SAMPLE || p->min_inliers > pnm::MAX_STRIDE)
    return fail(c, PISLAM_ERR_INVALID, "min_inliers must be 4..16384");
  if (level) PCHK(check_level_table(c, "level needs", inv_sigma2, nlevels));
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)pnm::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the absolute-pose call takes device pointers only";
  PCHK(device_ptrs(c, {cam, xw, obs_q8, counts, best, score, ninliers, inlier, pose_out, status}, what));
  if (level && !is_device_ptr(level)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t);
    const LkRange in[] = {{cam, B * 5 * sizeof(float)}, {xw, B * stride * 3 * sizeof(float)},
                          {obs_q8, B * stride * 3 * sizeof(int32_t)}, {counts, word}, {level, B * stride}};
    const LkRange out[] = {{best, word}, {score, word}, {ninliers, word}, {inlier, B * stride},
                           {pose_out, B * 12 * sizeof(float)}, {status, word}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pn::PnArgs a{};
  a.cam = cam, a.xw = xw, a.obs = obs_q8, a.level = level, a.counts = counts, a.stride = stride, a.batch = batch;
  a.hypotheses = p->hypotheses, a.min_inliers = p->min_inliers, a.seed = p->seed;
  copy_level_table(&a, inv_sigma2, level ? nlevels : 0);
  a.best = best, a.score = score, a.ninliers = ninliers, a.inlier = inlier, a.pose_out = pose_out, a.status = status;
  hipLaunchKernelGGL(pn::k_pnp_ransac, dim3((unsigned)std::min(batch, prk::GRID_CAP)), dim3(prk::THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_pnp_ransac");
}

// ---- similarity from 3D-3D matches: batched Sim(3) RANSAC -----------------------------------

PISLAM_EXPORT int pislam_sim3_ransac_batch(pislam_ctx *c, const pislam_sim3_params *p, const float *cam1,
                                           const float *cam2, const float *x1, const float *x2, const int32_t *obs1_q8,
                                           const int32_t *obs2_q8, const uint32_t *counts, const uint8_t *level1,
                                           const uint8_t *level2, const float *inv_sigma2, int nlevels, size_t stride,
                                           int batch, int32_t *best, uint32_t *score, uint32_t *ninliers,
                                           uint8_t *inlier, float *sim_out, uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->hypotheses < 1 || p->hypotheses > s3m::MAX_HYP) return fail(c, PISLAM_ERR_INVALID, "hypotheses must be 1..1024");
  if (p->min_inliers < s3m::SAMPLE || p->min_inliers > s3m::MAX_STRIDE)
    return fail(c, PISLAM_ERR_INVALID, "min_inliers must be 3..16384");
  if (p->fixed_scale != 0 && p->fixed_scale != 1) return fail(c, PISLAM_ERR_INVALID, "fixed_scale must be 0 or 1");
  PCHK(check_level_pair(c, level1, level2, inv_sigma2, nlevels));
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)s3m::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the similarity call takes device pointers only";
  PCHK(device_ptrs(c, {cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, best, score, ninliers, inlier, sim_out, status},
                   what));
  if (level1 && (!is_device_ptr(level1) || !is_device_ptr(level2))) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), cam = B * 5 * sizeof(float);
    const size_t pts = B * stride * 3 * sizeof(float), obs = B * stride * 3 * sizeof(int32_t);
    const LkRange in[] = {{cam1, cam}, {cam2, cam}, {x1, pts}, {x2, pts}, {obs1_q8, obs}, {obs2_q8, obs}, {counts, word},
                          {level1, B * stride}, {level2, B * stride}};
    const LkRange out[] = {{best, word}, {score, word}, {ninliers, word}, {inlier, B * stride},
                           {sim_out, B * s3m::OUT_WORDS * sizeof(float)}, {status, word}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  s3::S3Args a{};
  a.cam1 = cam1, a.cam2 = cam2, a.x1 = x1, a.x2 = x2, a.obs1 = obs1_q8, a.obs2 = obs2_q8, a.level1 = level1;
  a.level2 = level2, a.counts = counts, a.stride = stride, a.batch = batch, a.hypotheses = p->hypotheses;
  a.min_inliers = p->min_inliers, a.fixed_scale = p->fixed_scale, a.seed = p->seed;
  copy_level_table(&a, inv_sigma2, level1 ? nlevels : 0);
  a.best = best, a.score = score, a.ninliers = ninliers, a.inlier = inlier, a.sim_out = sim_out, a.status = status;
  hipLaunchKernelGGL(s3::k_sim3_ransac, dim3((unsigned)std::min(batch, prk::GRID_CAP)), dim3(prk::THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_sim3_ransac");
}

// ---- similarity refinement after the RANSAC: batched OptimizeSim3 ---------------------------

PISLAM_EXPORT int pislam_sim3_refine_batch(pislam_ctx *c, const pislam_sim3_refine_params *p, const float *sim_in,
                                           const float *cam1, const float *cam2, const float *x1, const float *x2,
                                           const int32_t *obs1_q8, const int32_t *obs2_q8, const uint32_t *counts,
                                           const uint8_t *level1, const uint8_t *level2, const uint8_t *mask,
                                           const float *inv_sigma2, int nlevels, size_t stride, int batch,
                                           float *sim_out, uint8_t *inlier, uint32_t *ninliers, double *cost,
                                           uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  PCHK(check_refine_schedule(c, p->rounds, p->iters, p->huber_rounds, p->min_obs));
  if (!(p->th2 > 0.0f) || !psm::finite_f(p->th2)) return fail(c, PISLAM_ERR_INVALID, "th2 must be finite and > 0");
  if (p->fixed_scale != 0 && p->fixed_scale != 1) return fail(c, PISLAM_ERR_INVALID, "fixed_scale must be 0 or 1");
  PCHK(check_refine_eps(c, p->eps));
  PCHK(check_level_pair(c, level1, level2, inv_sigma2, nlevels));
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)s3r::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the similarity refinement takes device pointers only";
  PCHK(device_ptrs(c, {sim_in, cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, sim_out, inlier, ninliers, cost, status}, what));
  if (level1 && (!is_device_ptr(level1) || !is_device_ptr(level2))) return fail(c, PISLAM_ERR_INVALID, what);
  if (mask && !is_device_ptr(mask)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), cam = B * 5 * sizeof(float);
    const size_t sim = B * s3r::STATE * sizeof(float);
    const size_t pts = B * stride * 3 * sizeof(float), obs = B * stride * 3 * sizeof(int32_t);
    const LkRange in[] = {{sim_in, sim}, {cam1, cam}, {cam2, cam}, {x1, pts}, {x2, pts}, {obs1_q8, obs}, {obs2_q8, obs},
                          {counts, word}, {level1, B * stride}, {level2, B * stride}, {mask, B * stride}};
    const LkRange out[] = {{sim_out, sim}, {inlier, B * stride}, {ninliers, word}, {cost, B * sizeof(double)},
                           {status, word}};
    // sim_out == sim_in is allowed: a pair reads its similarity before it writes it
    if (const char *bad = ranges_overlap(in, out, 0)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  sr::SrArgs a{};
  a.sim_in = sim_in, a.cam1 = cam1, a.cam2 = cam2, a.x1 = x1, a.x2 = x2, a.obs1 = obs1_q8, a.obs2 = obs2_q8;
  a.level1 = level1, a.level2 = level2, a.mask = mask, a.counts = counts, a.stride = stride, a.batch = batch;
  copy_level_table(&a, inv_sigma2, level1 ? nlevels : 0);
  a.p = s3r::Params{p->rounds, p->iters, p->huber_rounds, p->min_obs, p->th2, p->fixed_scale, p->eps};
  a.sim_out = sim_out, a.inlier = inlier, a.ninliers = ninliers, a.status = status, a.cost = cost;
  hipLaunchKernelGGL(sr::k_sim3_refine, dim3((unsigned)std::min(batch, prf::GRID_CAP)), dim3(prf::THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_sim3_refine");
}

// ---- new map points from two key frames: triangulation and stereo unprojection ------------

PISLAM_EXPORT int pislam_triangulate_batch(pislam_ctx *c, const pislam_triangulate_params *p, const float *pose1,
                                           const float *pose2, const float *cam1, const float *cam2,
                                           const int32_t *obs1_q8, const int32_t *obs2_q8, const uint8_t *level1,
                                           const uint8_t *level2, const uint32_t *counts, const float *level_scale,
                                           const float *level_sigma2, int nlevels, size_t stride, int batch, float *xw,
                                           uint8_t *status, float *normal, float *drange, uint32_t *npoints) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  const pmp::Params prm{p->cos_min_parallax, p->chi2_mono, p->chi2_stereo, p->ratio_factor};
  if (!pmp::params_ok(prm))
    return fail(c, PISLAM_ERR_INVALID, "cos_min_parallax must be finite; chi2_mono, chi2_stereo and ratio_factor finite and > 0");
  if (!level_scale || !level_sigma2 || nlevels < 1 || nlevels > pmp::MAX_LEVELS)
    return fail(c, PISLAM_ERR_INVALID, "level_scale and level_sigma2 need 1..16 entries");
  for (int l = 0; l < nlevels; l++) {
    if (!(level_scale[l] > 0.0f) || !psm::finite_f(level_scale[l]) || !(level_sigma2[l] > 0.0f) ||
        !psm::finite_f(level_sigma2[l]))
      return fail(c, PISLAM_ERR_INVALID, "level_scale and level_sigma2 must be finite and > 0");
    if (l > 0 && level_scale[l] < level_scale[l - 1]) return fail(c, PISLAM_ERR_INVALID, "level_scale must not decrease");
  }
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (stride < 1 || stride > (size_t)pmp::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the triangulation takes device pointers only";
  PCHK(device_ptrs(c, {pose1, pose2, cam1, cam2, obs1_q8, obs2_q8, level1, level2, counts, xw, status, npoints}, what));
  if ((normal && !is_device_ptr(normal)) || (drange && !is_device_ptr(drange))) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), pose = B * 12 * sizeof(float), cam = B * 5 * sizeof(float);
    const size_t obs = B * stride * 3 * sizeof(int32_t), pts = B * stride * 3 * sizeof(float);
    const LkRange in[] = {{pose1, pose}, {pose2, pose}, {cam1, cam}, {cam2, cam}, {obs1_q8, obs}, {obs2_q8, obs},
                          {level1, B * stride}, {level2, B * stride}, {counts, word}};
    const LkRange out[] = {{xw, pts}, {status, B * stride}, {normal, pts}, {drange, B * stride * 2 * sizeof(float)},
                           {npoints, word}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pmk::MpArgs a{};
  a.pose1 = pose1, a.pose2 = pose2, a.cam1 = cam1, a.cam2 = cam2, a.obs1 = obs1_q8, a.obs2 = obs2_q8;
  a.level1 = level1, a.level2 = level2, a.counts = counts, a.stride = stride, a.batch = batch;
  a.tab.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) a.tab.level_scale[l] = level_scale[l], a.tab.level_sigma2[l] = level_sigma2[l];
  a.p = prm;
  a.xw = xw, a.status = status, a.normal = normal, a.drange = drange, a.npoints = npoints;
  hipLaunchKernelGGL(pmk::k_triangulate, dim3((unsigned)std::min(batch, pmk::MP_GRID_CAP)), dim3(pmk::MP_THREADS), 0,
                     c->stream, a);
  return launch_ok(c, "k_triangulate");
}

// ---- local bundle adjustment: key-frame poses and map points together -----------------------

namespace {

int local_ba_shape(pislam_ctx *c, size_t kf_stride, size_t pt_stride, size_t stride, int batch) {
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (kf_stride < 1 || kf_stride > (size_t)pba::MAX_KF) return fail(c, PISLAM_ERR_INVALID, "kf_stride must be 1..32");
  if (pt_stride < 1 || pt_stride > (size_t)pba::MAX_PTS) return fail(c, PISLAM_ERR_INVALID, "pt_stride must be 1..4096");
  if (stride < 1 || stride > (size_t)pba::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  return PISLAM_OK;
}

int local_ba_workspace(pislam_ctx *c, size_t pt_stride, size_t stride, int batch) {
  const size_t groups = (size_t)std::min(batch, prf::GRID_CAP);
  if (c->w_ba.ensure(pbk::ws_bytes(pt_stride, stride) * groups) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(local bundle adjustment workspace)");
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_local_ba_reserve(pislam_ctx *c, size_t kf_stride, size_t pt_stride, size_t stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(local_ba_shape(c, kf_stride, pt_stride, stride, batch));
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  return local_ba_workspace(c, pt_stride, stride, batch);
}

PISLAM_EXPORT int pislam_local_ba_batch(pislam_ctx *c, const pislam_ba_params *p, const float *poses, const float *cams,
                                        const uint32_t *kf_counts, const uint32_t *kf_free, const float *xw,
                                        const uint32_t *pt_counts, const int32_t *obs_q8, const uint8_t *obs_kf,
                                        const uint16_t *obs_pt, const uint8_t *level, const uint32_t *counts,
                                        const float *inv_sigma2, int nlevels, size_t kf_stride, size_t pt_stride,
                                        size_t stride, int batch, float *poses_out, float *xw_out, uint8_t *inlier,
                                        uint32_t *ninliers, double *cost, uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->rounds < 1 || p->rounds > pba::MAX_ROUNDS) return fail(c, PISLAM_ERR_INVALID, "rounds must be 1..4");
  for (int r = 0; r < p->rounds; r++)
    if (p->iters[r] < 1 || p->iters[r] > 32) return fail(c, PISLAM_ERR_INVALID, "iters must be 1..32");
  if (p->huber_rounds < 0 || p->huber_rounds > p->rounds) return fail(c, PISLAM_ERR_INVALID, "huber_rounds must be 0..rounds");
  if (p->min_obs < 1 || p->min_obs > pba::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "min_obs must be 1..16384");
  PCHK(check_refine_eps(c, p->eps));
  if (level) PCHK(check_level_table(c, "level needs", inv_sigma2, nlevels));
  PCHK(local_ba_shape(c, kf_stride, pt_stride, stride, batch));
  if (batch == 0) return PISLAM_OK;
  const char *what = "the local bundle adjustment takes device pointers only";
  PCHK(device_ptrs(c, {poses, cams, kf_counts, kf_free, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, poses_out, xw_out,
                       inlier, ninliers, cost, status}, what));
  if (level && !is_device_ptr(level)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), pose = B * kf_stride * 12 * sizeof(float);
    const size_t pts = B * pt_stride * 3 * sizeof(float);
    const LkRange in[] = {{poses, pose}, {xw, pts}, {cams, B * kf_stride * 5 * sizeof(float)}, {kf_counts, word},
                          {kf_free, word}, {pt_counts, word}, {obs_q8, B * stride * 3 * sizeof(int32_t)},
                          {obs_kf, B * stride}, {obs_pt, B * stride * sizeof(uint16_t)}, {level, B * stride}, {counts, word}};
    const LkRange out[] = {{poses_out, pose}, {xw_out, pts}, {inlier, B * stride}, {ninliers, word},
                           {cost, B * sizeof(double)}, {status, word}};
    // poses_out == poses and xw_out == xw are allowed: a window reads its inputs before it writes them
    for (size_t o = 0; o < sizeof(out) / sizeof(out[0]); o++) {
      for (size_t i = 0; i < sizeof(in) / sizeof(in[0]); i++) {
        if (o < 2 && i == o && out[o].p == in[i].p) continue;
        if (lk_overlap(out[o], in[i])) return fail(c, PISLAM_ERR_INVALID, "an output overlaps an input");
      }
      for (size_t k = 0; k < o; k++)
        if (lk_overlap(out[o], out[k])) return fail(c, PISLAM_ERR_INVALID, "two outputs overlap");
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(local_ba_workspace(c, pt_stride, stride, batch));
  pbk::BaArgs a{};
  a.poses = poses, a.cams = cams, a.xw = xw, a.kf_counts = kf_counts, a.kf_free = kf_free, a.pt_counts = pt_counts;
  a.counts = counts, a.obs = obs_q8, a.obs_kf = obs_kf, a.obs_pt = obs_pt, a.level = level;
  a.kf_stride = kf_stride, a.pt_stride = pt_stride, a.stride = stride, a.batch = batch;
  copy_level_table(&a, inv_sigma2, level ? nlevels : 0);
  a.p = pba::Params{p->rounds, {p->iters[0], p->iters[1], p->iters[2], p->iters[3]}, p->huber_rounds, p->min_obs, p->eps};
  a.poses_out = poses_out, a.xw_out = xw_out, a.inlier = inlier, a.ninliers = ninliers, a.status = status, a.cost = cost;
  a.ws = c->w_ba.as<char>();
  hipLaunchKernelGGL(pbk::k_local_ba, dim3((unsigned)std::min(batch, prf::GRID_CAP)), dim3(prf::THREADS), 0, c->stream, a);
  return launch_ok(c, "k_local_ba");
}

// ---- essential-graph optimisation and map-point correction after a loop ---------------------

namespace {

int pose_graph_shape(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch) {
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (v_stride < 1 || v_stride > (size_t)pgr::MAX_V) return fail(c, PISLAM_ERR_INVALID, "v_stride must be 1..4096");
  if (e_stride < 1 || e_stride > (size_t)pgr::MAX_E) return fail(c, PISLAM_ERR_INVALID, "e_stride must be 1..16384");
  return PISLAM_OK;
}

int pose_graph_params_ok(pislam_ctx *c, const pislam_pose_graph_params *p) {
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->iters < 1 || p->iters > 64) return fail(c, PISLAM_ERR_INVALID, "iters must be 1..64");
  if (p->cg_iters < 1 || p->cg_iters > 1024) return fail(c, PISLAM_ERR_INVALID, "cg_iters must be 1..1024");
  if (!(p->cg_tol >= 0.0 && p->cg_tol < 1.0)) return fail(c, PISLAM_ERR_INVALID, "cg_tol must be in [0, 1)");
  return check_refine_eps(c, p->eps);
}

int pose_graph_workspace(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch) {
  const size_t groups = (size_t)std::min(batch, prf::GRID_CAP);
  if (c->w_pg.ensure(pgr::ws_bytes(v_stride, e_stride) * groups) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(pose graph workspace)");
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_pose_graph_reserve(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(pose_graph_shape(c, v_stride, e_stride, batch));
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  return pose_graph_workspace(c, v_stride, e_stride, batch);
}

PISLAM_EXPORT int pislam_pose_graph_batch(pislam_ctx *c, const pislam_pose_graph_params *p, const float *sims,
                                          const uint32_t *v_counts, const uint8_t *fixed, const uint32_t *edges,
                                          const float *meas, const float *weight, const uint32_t *e_counts,
                                          const uint32_t *inc_ptr, const uint32_t *inc, size_t v_stride, size_t e_stride,
                                          int batch, float *sims_out, double *cost, uint32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(pose_graph_params_ok(c, p));
  PCHK(pose_graph_shape(c, v_stride, e_stride, batch));
  if (batch == 0) return PISLAM_OK;
  const char *what = "the pose graph call takes device pointers only";
  PCHK(device_ptrs(c, {sims, v_counts, fixed, edges, meas, e_counts, inc_ptr, inc, sims_out, cost, status}, what));
  if (weight && !is_device_ptr(weight)) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), sim = B * v_stride * 13 * sizeof(float);
    const LkRange in[] = {{sims, sim}, {v_counts, word}, {fixed, B * v_stride}, {edges, B * e_stride * 2 * sizeof(uint32_t)},
                          {meas, B * e_stride * 13 * sizeof(float)}, {weight, B * e_stride * sizeof(float)}, {e_counts, word},
                          {inc_ptr, B * (v_stride + 1) * sizeof(uint32_t)}, {inc, B * e_stride * 2 * sizeof(uint32_t)}};
    const LkRange out[] = {{sims_out, sim}, {cost, B * sizeof(double)}, {status, word}};
    // sims_out == sims is allowed: a graph reads its similarities before it writes them
    if (const char *bad = ranges_overlap(in, out, 0)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(pose_graph_workspace(c, v_stride, e_stride, batch));
  pgk::PgArgs a{};
  a.sims = sims, a.meas = meas, a.weight = weight, a.fixed = fixed, a.v_counts = v_counts, a.e_counts = e_counts;
  a.edges = edges, a.inc_ptr = inc_ptr, a.inc = inc, a.v_stride = v_stride, a.e_stride = e_stride, a.batch = batch;
  a.p = pgr::Params{p->iters, p->cg_iters, p->cg_tol, p->eps};
  a.sims_out = sims_out, a.cost = cost, a.status = status, a.ws = c->w_pg.as<char>();
  hipLaunchKernelGGL(pgk::k_pose_graph, dim3((unsigned)std::min(batch, prf::GRID_CAP)), dim3(prf::THREADS), 0, c->stream, a);
  return launch_ok(c, "k_pose_graph");
}

PISLAM_EXPORT int pislam_map_points_correct_batch(pislam_ctx *c, const float *xw, const uint16_t *ref,
                                                  const uint32_t *pt_counts, const float *sims_old, const float *sims_new,
                                                  const uint32_t *v_counts, size_t pt_stride, size_t v_stride, int batch,
                                                  float *xw_out, uint8_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (pt_stride < 1 || pt_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "pt_stride must be 1..2^31 - 1");
  if (v_stride < 1 || v_stride > 65536) return fail(c, PISLAM_ERR_INVALID, "v_stride must be 1..65536");
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {xw, ref, pt_counts, sims_old, sims_new, v_counts, xw_out, status},
                   "the map-point correction takes device pointers only"));
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), pts = B * pt_stride * 3 * sizeof(float);
    const size_t sim = B * v_stride * 13 * sizeof(float);
    const LkRange in[] = {{xw, pts}, {ref, B * pt_stride * sizeof(uint16_t)}, {pt_counts, word}, {sims_old, sim},
                          {sims_new, sim}, {v_counts, word}};
    const LkRange out[] = {{xw_out, pts}, {status, B * pt_stride}};
    // xw_out == xw is allowed: a point is read before it is written, by the same thread
    if (const char *bad = ranges_overlap(in, out, 0)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pgk::McArgs a{};
  a.xw = xw, a.sims_old = sims_old, a.sims_new = sims_new, a.ref = ref, a.pt_counts = pt_counts, a.v_counts = v_counts;
  a.pt_stride = pt_stride, a.v_stride = v_stride, a.total = (size_t)batch * pt_stride, a.xw_out = xw_out, a.status = status;
  const size_t groups = (a.total + pgk::MC_THREADS - 1) / pgk::MC_THREADS;
  hipLaunchKernelGGL(pgk::k_map_points_correct, dim3((unsigned)std::min<size_t>(groups, pgk::MC_GRID_CAP)),
                     dim3(pgk::MC_THREADS), 0, c->stream, a);
  return launch_ok(c, "k_map_points_correct");
}

// ---- essential-graph optimisation of large graphs across workgroups -------------------------

namespace {

int pose_graph_wide_shape(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch) {
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (v_stride < 1 || v_stride > pgw::MAX_V) return fail(c, PISLAM_ERR_INVALID, "v_stride must be 1..65536");
  if (e_stride < 1 || e_stride > pgw::MAX_E) return fail(c, PISLAM_ERR_INVALID, "e_stride must be 1..2^20");
  return PISLAM_OK;
}

int pose_graph_wide_workspace(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch, size_t *per_graph) {
  *per_graph = pgw::ws_graph_bytes(v_stride, e_stride);
  if (*per_graph + pgw::CTL_BYTES > SIZE_MAX / (size_t)batch) return fail(c, PISLAM_ERR_NOMEM, "the wide pose graph workspace");
  if (c->w_pgw.ensure((*per_graph + pgw::CTL_BYTES) * (size_t)batch) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(wide pose graph workspace)");
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_pose_graph_wide_reserve(pislam_ctx *c, size_t v_stride, size_t e_stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(pose_graph_wide_shape(c, v_stride, e_stride, batch));
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  size_t per_graph;
  return pose_graph_wide_workspace(c, v_stride, e_stride, batch, &per_graph);
}

PISLAM_EXPORT int pislam_pose_graph_wide_batch(pislam_ctx *c, const pislam_pose_graph_params *p, const float *sims,
                                               const uint32_t *v_counts, const uint8_t *fixed, const uint32_t *edges,
                                               const float *meas, const float *weight, const uint32_t *e_counts,
                                               const uint32_t *inc_ptr, const uint32_t *inc, size_t v_stride,
                                               size_t e_stride, int batch, float *sims_out, double *cost, uint32_t *status,
                                               uint32_t *work) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(pose_graph_params_ok(c, p));
  PCHK(pose_graph_wide_shape(c, v_stride, e_stride, batch));
  if (batch == 0) return PISLAM_OK;
  const char *what = "the wide pose graph call takes device pointers only";
  PCHK(device_ptrs(c, {sims, v_counts, fixed, edges, meas, e_counts, inc_ptr, inc, sims_out, cost, status}, what));
  if ((weight && !is_device_ptr(weight)) || (work && !is_device_ptr(work))) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), sim = B * v_stride * 13 * sizeof(float);
    const LkRange in[] = {{sims, sim}, {v_counts, word}, {fixed, B * v_stride}, {edges, B * e_stride * 2 * sizeof(uint32_t)},
                          {meas, B * e_stride * 13 * sizeof(float)}, {weight, B * e_stride * sizeof(float)}, {e_counts, word},
                          {inc_ptr, B * (v_stride + 1) * sizeof(uint32_t)}, {inc, B * e_stride * 2 * sizeof(uint32_t)}};
    const LkRange out[] = {{sims_out, sim}, {cost, B * sizeof(double)}, {status, word}, {work, 2 * word}};
    // sims_out == sims is allowed: the state is read into the workspace before anything is written
    if (const char *bad = ranges_overlap(in, out, 0)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pgw::WideArgs a{};
  PCHK(pose_graph_wide_workspace(c, v_stride, e_stride, batch, &a.ws_graph));
  a.sims = sims, a.meas = meas, a.weight = weight, a.fixed = fixed, a.v_counts = v_counts, a.e_counts = e_counts;
  a.edges = edges, a.inc_ptr = inc_ptr, a.inc = inc, a.v_stride = v_stride, a.e_stride = e_stride, a.batch = (size_t)batch;
  a.p = pgr::Params{p->iters, p->cg_iters, p->cg_tol, p->eps};
  a.sims_out = sims_out, a.cost = cost, a.status = status, a.work = work, a.ws = c->w_pgw.as<char>();
  // the control blocks start from zero: the checks only raise flags
  HIPCHK(c, hipMemsetAsync(a.ws, 0, a.batch * pgw::CTL_BYTES, c->stream));
  const size_t V = v_stride, E = e_stride, T = pgw::THREADS;
  int rc = PISLAM_OK;
  auto run = [&](auto kernel, size_t per_graph, size_t group, const char *name, auto... more) {
    if (rc != PISLAM_OK) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)pgw::groups_of(a, per_graph, group)), dim3(pgw::THREADS), 0, c->stream, a, more...);
    rc = launch_ok(c, name);
  };
  // the fixed sequence of pgw::launch_count(): nothing is read back, a graph's control block gates every launch
  run(pgw::k_pgw_check, E + V, T, "k_pgw_check");
  run(pgw::k_pgw_load, V + E, T, "k_pgw_load");
  run(pgw::k_pgw_eval, E, T, "k_pgw_eval", (int)pgw::FIRST);
  run(pgw::k_pgw_decide, 1, 1, "k_pgw_decide", (int)pgw::FIRST);
  for (int it = 0; it < p->iters; it++) {
    run(pgw::k_pgw_setup, V, T, "k_pgw_setup");
    run(pgw::k_pgw_cg_scalar, 1, 1, "k_pgw_cg_scalar", (int)pgw::BEGIN, 0);
    for (int n = 0; n < p->cg_iters; n++) {
      run(pgw::k_pgw_edge_v, E, T, "k_pgw_edge_v");
      run(pgw::k_pgw_cg_vertex, V, T, "k_pgw_cg_vertex", (int)pgw::AP);
      run(pgw::k_pgw_cg_scalar, 1, 1, "k_pgw_cg_scalar", (int)pgw::ALPHA, n);
      run(pgw::k_pgw_cg_vertex, V, T, "k_pgw_cg_vertex", (int)pgw::UPDATE);
      run(pgw::k_pgw_cg_scalar, 1, 1, "k_pgw_cg_scalar", (int)pgw::BETA, n);
      run(pgw::k_pgw_cg_vertex, V, T, "k_pgw_cg_vertex", (int)pgw::P);
    }
    run(pgw::k_pgw_retract, V, T, "k_pgw_retract");
    run(pgw::k_pgw_eval, E, T, "k_pgw_eval", (int)pgw::TRIAL);
    run(pgw::k_pgw_decide, 1, 1, "k_pgw_decide", (int)pgw::TRIAL);
  }
  run(pgw::k_pgw_out, pgr::STATE * V, T, "k_pgw_out");
  return rc;
}

// ---- the covisibility graph of a map -------------------------------------------------------------

namespace {

int covis_shape(pislam_ctx *c, size_t kf_stride, size_t stride, int batch) {
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (kf_stride < 1 || kf_stride > (size_t)pcv::MAX_KF) return fail(c, PISLAM_ERR_INVALID, "kf_stride must be 1..4096");
  if (stride < 1 || stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..2^31 - 1");
  return PISLAM_OK;
}

int covis_workspace(pislam_ctx *c, size_t kf_stride, int batch) {
  if (c->w_cv.ensure(pcv::ws_bytes(kf_stride, (size_t)batch)) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(covisibility workspace)");
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_covisibility_reserve(pislam_ctx *c, size_t kf_stride, size_t stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(covis_shape(c, kf_stride, stride, batch));
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  return covis_workspace(c, kf_stride, batch);
}

PISLAM_EXPORT int pislam_covisibility_batch(pislam_ctx *c, const pislam_covis_params *p, const uint16_t *obs_kf,
                                            const int32_t *obs_pt, const int32_t *counts, const int32_t *kf_counts,
                                            const uint8_t *obs_level, const uint8_t *cull_mask, size_t kf_stride,
                                            size_t stride, size_t nb_stride, int batch, uint16_t *nb_idx, int32_t *nb_weight,
                                            int32_t *nb_count, uint16_t *parent, int32_t *kf_points, int32_t *kf_redundant,
                                            int32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  if (p->min_weight < 1) return fail(c, PISLAM_ERR_INVALID, "min_weight must be >= 1");
  if (p->cull_min_observers < 1) return fail(c, PISLAM_ERR_INVALID, "cull_min_observers must be >= 1");
  if (p->cull_level_slack < 0 || p->cull_level_slack > 255) return fail(c, PISLAM_ERR_INVALID, "cull_level_slack must be 0..255");
  PCHK(covis_shape(c, kf_stride, stride, batch));
  if (nb_stride < 1 || nb_stride > kf_stride) return fail(c, PISLAM_ERR_INVALID, "nb_stride must be 1..kf_stride");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the covisibility call takes device pointers only";
  PCHK(device_ptrs(c, {obs_kf, obs_pt, counts, kf_counts, nb_idx, nb_weight, nb_count, parent, kf_points, kf_redundant, status},
                   what));
  if ((obs_level && !is_device_ptr(obs_level)) || (cull_mask && !is_device_ptr(cull_mask)))
    return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(int32_t), row = B * kf_stride;
    const LkRange in[] = {{obs_kf, B * stride * sizeof(uint16_t)}, {obs_pt, B * stride * sizeof(int32_t)}, {counts, word},
                          {kf_counts, word}, {obs_level, B * stride}, {cull_mask, B * stride}};
    const LkRange out[] = {{nb_idx, row * nb_stride * sizeof(uint16_t)}, {nb_weight, row * nb_stride * sizeof(int32_t)},
                           {nb_count, row * sizeof(int32_t)}, {parent, row * sizeof(uint16_t)},
                           {kf_points, row * sizeof(int32_t)}, {kf_redundant, row * sizeof(int32_t)}, {status, word}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  PCHK(covis_workspace(c, kf_stride, batch));
  pcvk::CvArgs a{};
  a.obs_pt = obs_pt, a.counts = counts, a.kf_counts = kf_counts, a.obs_kf = obs_kf, a.obs_level = obs_level, a.cull_mask = cull_mask;
  a.kf_stride = kf_stride, a.stride = stride, a.nb_stride = nb_stride, a.batch = (size_t)batch;
  a.p = pcv::Params{p->min_weight, p->cull_min_observers, p->cull_level_slack};
  a.nb_idx = nb_idx, a.parent = parent, a.nb_weight = nb_weight, a.nb_count = nb_count, a.kf_points = kf_points;
  a.kf_redundant = kf_redundant, a.status = status;
  pcv::ws_carve(c->w_cv.p, kf_stride, a.batch, &a.ws);
  // a second call on the same context starts from a clean matrix
  HIPCHK(c, hipMemsetAsync(c->w_cv.p, 0, pcv::ws_bytes(kf_stride, a.batch), c->stream));
  const size_t slots = a.batch * stride, count_groups = (slots + pcvk::CV_THREADS - 1) / pcvk::CV_THREADS;
  hipLaunchKernelGGL(pcvk::k_covis_count, dim3((unsigned)std::min<size_t>(count_groups, pcvk::CV_GRID_CAP)),
                     dim3(pcvk::CV_THREADS), 0, c->stream, a);
  PCHK(launch_ok(c, "k_covis_count"));
  // the row kernel: 64, 128 or 256 threads and 8 bytes of LDS per key, both by kf_stride rounded up to a power of two
  size_t keys = 64;
  while (keys < kf_stride) keys <<= 1;
  hipLaunchKernelGGL(pcvk::k_covis_rows, dim3((unsigned)std::min<size_t>(a.batch * kf_stride, pcvk::CV_GRID_CAP)),
                     dim3((unsigned)std::min<size_t>(keys, pcvk::CV_THREADS)), keys * sizeof(uint64_t), c->stream, a);
  return launch_ok(c, "k_covis_rows");
}

// ---- the map points' summaries: normal, distance range, representative descriptor ----------

PISLAM_EXPORT int pislam_map_points_update_batch(pislam_ctx *c, const uint16_t *obs_kf, const int32_t *obs_pt,
                                                 const int32_t *counts, const int32_t *kf_counts, const uint8_t *obs_level,
                                                 const uint32_t *obs_desc, const float *poses, const float *xw,
                                                 const uint32_t *pt_counts, const uint16_t *ref, const float *level_scale,
                                                 int nlevels, size_t kf_stride, size_t stride, size_t pt_stride, int batch,
                                                 float *normal, float *drange, uint32_t *desc, int32_t *nobs, int32_t *first,
                                                 uint8_t *pt_status, int32_t *status) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!level_scale || nlevels < 1 || nlevels > pmu::MAX_LEVELS)
    return fail(c, PISLAM_ERR_INVALID, "level_scale needs 1..16 entries");
  for (int l = 0; l < nlevels; l++) {
    if (!(level_scale[l] > 0.0f) || !psm::finite_f(level_scale[l]))
      return fail(c, PISLAM_ERR_INVALID, "level_scale must be finite and > 0");
    if (l > 0 && level_scale[l] < level_scale[l - 1]) return fail(c, PISLAM_ERR_INVALID, "level_scale must not decrease");
  }
  PCHK(covis_shape(c, kf_stride, stride, batch));
  if (pt_stride < 1 || pt_stride > 0x7fffffffu) return fail(c, PISLAM_ERR_INVALID, "pt_stride must be 1..2^31 - 1");
  if (batch == 0) return PISLAM_OK;
  const char *what = "the map-point update takes device pointers only";
  PCHK(device_ptrs(c, {obs_kf, obs_pt, counts, kf_counts, obs_level, poses, xw, pt_counts, nobs, pt_status, status}, what));
  for (const void *opt : {(const void *)obs_desc, (const void *)ref, (const void *)normal, (const void *)drange,
                          (const void *)desc, (const void *)first})
    if (opt && !is_device_ptr(opt)) return fail(c, PISLAM_ERR_INVALID, what);
  if (desc && !obs_desc) return fail(c, PISLAM_ERR_INVALID, "desc needs obs_desc");
  {
    const size_t B = (size_t)batch, word = B * sizeof(int32_t), pts = B * pt_stride;
    const size_t words = pmu::WORDS * sizeof(uint32_t);
    const LkRange in[] = {{obs_kf, B * stride * sizeof(uint16_t)}, {obs_pt, B * stride * sizeof(int32_t)}, {counts, word},
                          {kf_counts, word}, {obs_level, B * stride}, {obs_desc, B * stride * words},
                          {poses, B * kf_stride * 12 * sizeof(float)}, {xw, pts * 3 * sizeof(float)}, {pt_counts, word},
                          {ref, pts * sizeof(uint16_t)}};
    const LkRange out[] = {{normal, pts * 3 * sizeof(float)}, {drange, pts * 2 * sizeof(float)}, {desc, pts * words},
                           {nobs, pts * sizeof(int32_t)}, {first, pts * sizeof(int32_t)}, {pt_status, pts}, {status, word}};
    if (const char *bad = ranges_overlap(in, out)) return fail(c, PISLAM_ERR_INVALID, bad);
  }
  HIPCHK(c, hipSetDevice(c->device));
  pmuk::MuArgs a{};
  a.obs_pt = obs_pt, a.counts = counts, a.kf_counts = kf_counts, a.obs_kf = obs_kf, a.ref = ref, a.obs_level = obs_level;
  a.obs_desc = obs_desc, a.pt_counts = pt_counts, a.poses = poses, a.xw = xw;
  a.kf_stride = kf_stride, a.stride = stride, a.pt_stride = pt_stride, a.batch = (size_t)batch;
  a.tab.nlevels = nlevels;
  for (int l = 0; l < pmu::MAX_LEVELS; l++) a.tab.level_scale[l] = l < nlevels ? level_scale[l] : 0.0f;
  a.normal = normal, a.drange = drange, a.desc = desc, a.nobs = nobs, a.first = first, a.status = status, a.pt_status = pt_status;
  // status[b] is the map's flag between the kernels: zero, then 3 from whoever finds the map malformed
  HIPCHK(c, hipMemsetAsync(status, 0, a.batch * sizeof(int32_t), c->stream));
  const auto grid = [](size_t groups) { return dim3((unsigned)std::min<size_t>(groups, pmuk::MU_GRID_CAP)); };
  hipLaunchKernelGGL(pmuk::k_mapupdate_check, grid((a.batch * stride + pmuk::MU_THREADS - 1) / pmuk::MU_THREADS),
                     dim3(pmuk::MU_THREADS), 0, c->stream, a);
  PCHK(launch_ok(c, "k_mapupdate_check"));
  const size_t waves = a.batch * ((pt_stride + pmuk::MU_CHUNK - 1) / pmuk::MU_CHUNK);
  hipLaunchKernelGGL(pmuk::k_mapupdate_points, grid((waves + pmuk::MU_WAVES - 1) / pmuk::MU_WAVES), dim3(pmuk::MU_THREADS), 0,
                     c->stream, a);
  PCHK(launch_ok(c, "k_mapupdate_points"));
  if (!desc) return PISLAM_OK;
  hipLaunchKernelGGL(pmuk::k_mapupdate_long, grid(a.batch * ((pt_stride + pmuk::MU_THREADS - 1) / pmuk::MU_THREADS)),
                     dim3(pmuk::MU_THREADS), 0, c->stream, a);
  return launch_ok(c, "k_mapupdate_long");
}

// ---- global bundle adjustment of whole maps across workgroups ---------------------------------

namespace {

int global_ba_shape(pislam_ctx *c, size_t kf_stride, size_t pt_stride, size_t stride, int batch) {
  if (batch < 0) return fail(c, PISLAM_ERR_INVALID, "negative batch");
  if (kf_stride < 1 || kf_stride > (size_t)gba::MAX_KF) return fail(c, PISLAM_ERR_INVALID, "kf_stride must be 1..4096");
  if (pt_stride < 1 || pt_stride > gba::MAX_PTS) return fail(c, PISLAM_ERR_INVALID, "pt_stride must be 1..2^22");
  if (stride < 1 || stride > gba::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..2^24");
  return PISLAM_OK;
}

int global_ba_workspace(pislam_ctx *c, size_t kf_stride, size_t pt_stride, size_t stride, int batch, size_t *per_map) {
  *per_map = gba::ws_bytes(kf_stride, pt_stride, stride);
  if (*per_map + gba::CTL_BYTES > SIZE_MAX / (size_t)batch) return fail(c, PISLAM_ERR_NOMEM, "the global bundle adjustment workspace");
  if (c->w_gba.ensure((*per_map + gba::CTL_BYTES) * (size_t)batch) != PISLAM_OK)
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(global bundle adjustment workspace)");
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_global_ba_reserve(pislam_ctx *c, size_t kf_stride, size_t pt_stride, size_t stride, int batch) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(global_ba_shape(c, kf_stride, pt_stride, stride, batch));
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  size_t per_map;
  return global_ba_workspace(c, kf_stride, pt_stride, stride, batch, &per_map);
}

PISLAM_EXPORT int pislam_global_ba_batch(pislam_ctx *c, const pislam_gba_params *p, const float *poses, const float *cams,
                                         const uint8_t *fixed, const int32_t *kf_counts, const float *xw,
                                         const uint32_t *pt_counts, const int32_t *obs_q8, const uint16_t *obs_kf,
                                         const int32_t *obs_pt, const uint8_t *level, const int32_t *counts,
                                         const uint32_t *kf_ptr, const uint32_t *kf_obs, const float *inv_sigma2, int nlevels,
                                         size_t kf_stride, size_t pt_stride, size_t stride, int batch, float *poses_out,
                                         float *xw_out, uint8_t *inlier, uint32_t *ninliers, double *cost, uint32_t *status,
                                         uint32_t *work) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!p) return fail(c, PISLAM_ERR_INVALID, "null parameters");
  const pislam_ba_params &q = p->ba;
  if (q.rounds < 1 || q.rounds > gba::MAX_ROUNDS) return fail(c, PISLAM_ERR_INVALID, "rounds must be 1..4");
  for (int r = 0; r < q.rounds; r++)
    if (q.iters[r] < 1 || q.iters[r] > gba::MAX_ITERS) return fail(c, PISLAM_ERR_INVALID, "iters must be 1..32");
  if (q.huber_rounds < 0 || q.huber_rounds > q.rounds) return fail(c, PISLAM_ERR_INVALID, "huber_rounds must be 0..rounds");
  if (q.min_obs < 1 || (size_t)q.min_obs > gba::MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "min_obs must be 1..2^24");
  PCHK(check_refine_eps(c, q.eps));
  if (p->cg_iters < 1 || p->cg_iters > gba::MAX_CG) return fail(c, PISLAM_ERR_INVALID, "cg_iters must be 1..256");
  if (!(p->cg_tol >= 0.0 && p->cg_tol < 1.0)) return fail(c, PISLAM_ERR_INVALID, "cg_tol must be in [0, 1)");
  if (level) PCHK(check_level_table(c, "level needs", inv_sigma2, nlevels));
  PCHK(global_ba_shape(c, kf_stride, pt_stride, stride, batch));
  if (batch == 0) return PISLAM_OK;
  const char *what = "the global bundle adjustment takes device pointers only";
  PCHK(device_ptrs(c, {poses, cams, fixed, kf_counts, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, kf_ptr, kf_obs, poses_out,
                       xw_out, inlier, ninliers, cost, status}, what));
  if ((level && !is_device_ptr(level)) || (work && !is_device_ptr(work))) return fail(c, PISLAM_ERR_INVALID, what);
  {
    const size_t B = (size_t)batch, word = B * sizeof(uint32_t), pose = B * kf_stride * 12 * sizeof(float);
    const size_t pts = B * pt_stride * 3 * sizeof(float);
    const LkRange in[] = {{poses, pose}, {xw, pts}, {cams, B * kf_stride * 5 * sizeof(float)}, {fixed, B * kf_stride},
                          {kf_counts, word}, {pt_counts, word}, {obs_q8, B * stride * 3 * sizeof(int32_t)},
                          {obs_kf, B * stride * sizeof(uint16_t)}, {obs_pt, B * stride * sizeof(int32_t)}, {level, B * stride},
                          {counts, word}, {kf_ptr, B * (kf_stride + 1) * sizeof(uint32_t)}, {kf_obs, B * stride * sizeof(uint32_t)}};
    const LkRange out[] = {{poses_out, pose}, {xw_out, pts}, {inlier, B * stride}, {ninliers, word},
                           {cost, B * sizeof(double)}, {status, word}, {work, 2 * word}};
    // poses_out == poses and xw_out == xw are allowed: the state is read into the workspace before anything is written
    for (size_t o = 0; o < sizeof(out) / sizeof(out[0]); o++) {
      for (size_t i = 0; i < sizeof(in) / sizeof(in[0]); i++) {
        if (o < 2 && i == o && out[o].p == in[i].p) continue;
        if (lk_overlap(out[o], in[i])) return fail(c, PISLAM_ERR_INVALID, "an output overlaps an input");
      }
      for (size_t k = 0; k < o; k++)
        if (lk_overlap(out[o], out[k])) return fail(c, PISLAM_ERR_INVALID, "two outputs overlap");
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  gbk::GbaArgs a{};
  PCHK(global_ba_workspace(c, kf_stride, pt_stride, stride, batch, &a.ws_map));
  a.poses = poses, a.cams = cams, a.xw = xw, a.obs = obs_q8, a.obs_pt = obs_pt, a.counts = counts, a.kf_counts = kf_counts;
  a.pt_counts = pt_counts, a.kf_ptr = kf_ptr, a.kf_obs = kf_obs, a.obs_kf = obs_kf, a.level = level, a.fixed = fixed;
  a.kf_stride = kf_stride, a.pt_stride = pt_stride, a.stride = stride, a.batch = (size_t)batch;
  copy_level_table(&a, inv_sigma2, level ? nlevels : 0);
  a.p.ba = pba::Params{q.rounds, {q.iters[0], q.iters[1], q.iters[2], q.iters[3]}, q.huber_rounds, q.min_obs, q.eps};
  a.p.cg_iters = p->cg_iters, a.p.cg_tol = p->cg_tol;
  a.poses_out = poses_out, a.xw_out = xw_out, a.inlier = inlier, a.ninliers = ninliers, a.status = status, a.work = work;
  a.cost = cost, a.ws = c->w_gba.as<char>();
  // the control blocks start from zero: the checks only raise flags
  HIPCHK(c, hipMemsetAsync(a.ws, 0, a.batch * gba::CTL_BYTES, c->stream));
  const size_t K = kf_stride, P = pt_stride, N = stride, T = gbk::THREADS, W = gbk::WAVES;
  int rc = PISLAM_OK;
  auto run = [&](auto kernel, size_t per_map, size_t group, const char *name, auto... more) {
    if (rc != PISLAM_OK) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)gbk::groups_of(a, per_map, group)), dim3(gbk::THREADS), 0, c->stream, a, more...);
    rc = launch_ok(c, name);
  };
  // the fixed sequence of gba::launch_count(): nothing is read back, a map's control block gates every launch
  run(gbk::k_gba_check_items, N + P, T, "k_gba_check_items");
  run(gbk::k_gba_check_kf, K, W, "k_gba_check_kf");
  run(gbk::k_gba_begin, 1, 1, "k_gba_begin");
  run(gbk::k_gba_load, K + P + 1 + N, T, "k_gba_load");
  run(gbk::k_gba_pass, P, T, "k_gba_pass", (int)gbk::FIRST, (int)(0 < q.huber_rounds));
  run(gbk::k_gba_decide, 1, 1, "k_gba_decide", (int)gbk::FIRST, 0);
  for (int r = 0; r < q.rounds; r++) {
    for (int it = 0; it < q.iters[r]; it++) {
      run(gbk::k_gba_factor, P, T, "k_gba_factor");
      run(gbk::k_gba_kf_setup, K, W, "k_gba_kf_setup");
      run(gbk::k_gba_cg_begin, 1, 1, "k_gba_cg_begin");
      for (int n = 0; n < p->cg_iters; n++) {
        run(gbk::k_gba_cg_point, P, T, "k_gba_cg_point");
        run(gbk::k_gba_cg_kf, K, W, "k_gba_cg_kf");
        run(gbk::k_gba_cg_scalar, 1, 1, "k_gba_cg_scalar");
      }
      run(gbk::k_gba_step, P + K, T, "k_gba_step");
      run(gbk::k_gba_pass, P, T, "k_gba_pass", (int)gbk::TRIAL, (int)(r < q.huber_rounds));
      run(gbk::k_gba_decide, 1, 1, "k_gba_decide", (int)gbk::TRIAL, r);
    }
    run(gbk::k_gba_pass, P, T, "k_gba_pass", (int)gbk::CLASSIFY, (int)(r + 1 < q.huber_rounds));
    run(gbk::k_gba_decide, 1, 1, "k_gba_decide", (int)gbk::CLASSIFY, r);
  }
  run(gbk::k_gba_out, std::max(std::max(12 * K, 3 * P), N), T, "k_gba_out");
  return rc;
}

// ---- bag of words: integer weights and the key-frame database -----------------------------

PISLAM_EXPORT int pislam_bow_weight_batch(pislam_ctx *c, const uint32_t *bow_word, const uint32_t *bow_tf,
                                          const uint32_t *bow_n, size_t stride, int batch, const uint32_t *idf,
                                          uint32_t nwords, uint32_t *bow_weight) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(check_batch(c, batch));
  if (stride > (size_t)pd::DB_MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be at most 16384");
  if (idf && !is_device_ptr(idf)) return fail(c, PISLAM_ERR_INVALID, "idf must be a device pointer or null");
  if (batch == 0 || stride == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {bow_word, bow_tf, bow_n, bow_weight}, "the bag-of-words weights take device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(pd::k_bow_weight, dim3((unsigned)batch), dim3(pd::DB_THREADS), 0, c->stream, bow_word, bow_tf, bow_n,
                     stride, idf, nwords, bow_weight);
  return launch_ok(c, "k_bow_weight");
}

struct pislam_bowdb {
  int device = 0;
  uint32_t nwords = 0;
  size_t stride = 0;
  int capacity = 0;
  int size = 0;                      // ids handed out (host state: an add is refused before anything is launched)
  std::vector<uint8_t> alive;        // host mirror of d_alive (pislam_bowdb_remove validates on it)
  // forward store [capacity][stride], entries per key frame, liveness, the number of key frames as the query reads it
  DevBuf fwd_word, fwd_weight, fwd_n, d_alive, d_size;
  // inverted file: entries per word, CSR offsets [nwords + 1], scatter cursors, chunk sums of the scan, postings (id, weight)
  DevBuf cnt, off, cursor, bsum, post;
  void release() {
    for (DevBuf *b : {&fwd_word, &fwd_weight, &fwd_n, &d_alive, &d_size, &cnt, &off, &cursor, &bsum, &post}) b->release();
  }
};

namespace {

// Launch shape and workspace layout of a query of `batch` vectors for `topk` results against a database of `capacity`.
struct DbQueryPlan {
  uint32_t cap_pad, slice, nslices, nsel;
  size_t lds, o_score, o_common, o_gmax, o_pkey, o_pcom, bytes;
};

DbQueryPlan db_query_plan(int capacity, int batch, int topk) {
  DbQueryPlan P{};
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  P.cap_pad = ((uint32_t)capacity + 1u) & ~1u;
  P.nslices = (uint32_t)cdiv(capacity, pd::DB_ACC_MAX_SLICE);
  P.slice = ((uint32_t)cdiv(capacity, (int)P.nslices) + 1u) & ~1u;
  P.nsel = (uint32_t)cdiv(capacity, pd::DB_SEL_SLICE);
  P.lds = (size_t)P.slice * 6;
  const size_t cells = (size_t)batch * P.cap_pad, part = P.nsel > 1 ? (size_t)batch * P.nsel * topk : 0;
  P.o_score = 0;
  P.o_common = up(P.o_score + 4 * cells);
  P.o_gmax = up(P.o_common + 2 * cells);
  P.o_pkey = up(P.o_gmax + 4 * (size_t)batch);
  P.o_pcom = up(P.o_pkey + 8 * part);
  P.bytes = up(P.o_pcom + 4 * part);
  return P;
}

int db_query_args(pislam_ctx *c, const pislam_bowdb *db, int batch, int topk) {
  if (!db) return fail(c, PISLAM_ERR_INVALID, "null database");
  if (db->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the database lives on another device");
  PCHK(check_batch(c, batch));
  if (topk < 1 || topk > pd::DB_MAX_TOPK) return fail(c, PISLAM_ERR_INVALID, "topk must be 1..64");
  return PISLAM_OK;
}

int db_query_workspace(pislam_ctx *c, const DbQueryPlan &P) {
  if (c->w_db.ensure(P.bytes) != PISLAM_OK) return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(database query workspace)");
  RAISE_LDS_LIMIT(c, pd::k_db_accumulate, P.lds);
  return PISLAM_OK;
}

}  // namespace

PISLAM_EXPORT int pislam_bowdb_create(pislam_ctx *c, uint32_t nwords, size_t stride, int capacity, pislam_bowdb **out) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!out) return fail(c, PISLAM_ERR_INVALID, "null database pointer");
  *out = nullptr;
  if (nwords < 1 || nwords > (1u << 24)) return fail(c, PISLAM_ERR_INVALID, "nwords must be 1..2^24");
  if (stride < 1 || stride > (size_t)pd::DB_MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be 1..16384");
  if (capacity < 1 || capacity > pd::DB_MAX_CAPACITY) return fail(c, PISLAM_ERR_INVALID, "capacity must be 1..2^20");
  const size_t entries = stride * (size_t)capacity;
  if (entries > ((size_t)1 << 31)) return fail(c, PISLAM_ERR_NOMEM, "more than 2^31 entries (capacity * stride)");
  HIPCHK(c, hipSetDevice(c->device));
  pislam_bowdb *db = new pislam_bowdb();
  db->device = c->device;
  db->nwords = nwords, db->stride = stride, db->capacity = capacity;
  db->alive.assign((size_t)capacity, 0);
  const size_t nchunks = (size_t)cdiv((int)nwords, pd::DB_SCAN_CHUNK);
  const bool ok = db->fwd_word.ensure(4 * entries) == PISLAM_OK && db->fwd_weight.ensure(4 * entries) == PISLAM_OK &&
                  db->post.ensure(8 * entries) == PISLAM_OK && db->fwd_n.ensure(4 * (size_t)capacity) == PISLAM_OK &&
                  db->d_alive.ensure((size_t)capacity) == PISLAM_OK && db->d_size.ensure(4) == PISLAM_OK &&
                  db->cnt.ensure(4 * (size_t)nwords) == PISLAM_OK && db->off.ensure(4 * ((size_t)nwords + 1)) == PISLAM_OK &&
                  db->cursor.ensure(4 * (size_t)nwords) == PISLAM_OK && db->bsum.ensure(4 * nchunks) == PISLAM_OK;
  if (!ok) {
    db->release();
    delete db;
    return fail(c, PISLAM_ERR_NOMEM, "hipMalloc(key-frame database)");
  }
  hipError_t e = hipMemsetAsync(db->cnt.p, 0, 4 * (size_t)nwords, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(db->d_alive.p, 0, (size_t)capacity, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(db->d_size.p, 0, 4, c->stream);
  if (e != hipSuccess) {
    db->release();
    delete db;
    return fail(c, PISLAM_ERR_HIP, "database initialisation", e);
  }
  *out = db;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_bowdb_destroy(pislam_bowdb *db) {
  if (!db) return PISLAM_ERR_INVALID;
  (void)hipSetDevice(db->device);
  db->release();
  delete db;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_bowdb_size(const pislam_bowdb *db) { return db ? db->size : PISLAM_ERR_INVALID; }

PISLAM_EXPORT int pislam_bowdb_add_batch(pislam_ctx *c, pislam_bowdb *db, const uint32_t *bow_word,
                                         const uint32_t *bow_weight, const uint32_t *bow_n, size_t stride, int batch,
                                         int32_t *first_id) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!db) return fail(c, PISLAM_ERR_INVALID, "null database");
  if (db->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the database lives on another device");
  if (batch < 0 || batch > db->capacity - db->size) return fail(c, PISLAM_ERR_INVALID, "the add would pass the database's capacity");
  if (stride > (size_t)pd::DB_MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be at most 16384");
  if (batch > 0) PCHK(device_ptrs(c, {bow_word, bow_weight, bow_n}, "the key-frame database takes device pointers only"));
  if (first_id) *first_id = db->size;
  if (batch == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t first = (uint32_t)db->size, dbs = (uint32_t)db->stride, nw = db->nwords;
  uint32_t *cnt = db->cnt.as<uint32_t>(), *off = db->off.as<uint32_t>(), *cursor = db->cursor.as<uint32_t>();
  uint32_t *bsum = db->bsum.as<uint32_t>();
  hipLaunchKernelGGL(pd::k_db_store, dim3((unsigned)batch), dim3(pd::DB_STORE_THREADS), 0, c->stream, first, dbs, nw,
                     bow_word, bow_weight, bow_n, stride, db->fwd_word.as<uint32_t>(), db->fwd_weight.as<uint32_t>(),
                     db->fwd_n.as<uint32_t>(), db->d_alive.as<uint8_t>(), cnt, db->d_size.as<uint32_t>());
  PCHK(launch_ok(c, "k_db_store"));
  // the ids are handed out now: the forward store holds them whatever happens to the launches below
  for (int b = 0; b < batch; b++) db->alive[(size_t)first + b] = 1;
  db->size += batch;
  const unsigned nchunks = (unsigned)cdiv((int)nw, pd::DB_SCAN_CHUNK);
  hipLaunchKernelGGL(pd::k_db_scan_chunks, dim3(nchunks), dim3(pd::DB_THREADS), 0, c->stream, cnt, nw, bsum);
  PCHK(launch_ok(c, "k_db_scan_chunks"));
  hipLaunchKernelGGL(pd::k_db_scan_sums, dim3(1), dim3(pd::DB_THREADS), 0, c->stream, nchunks, nw, bsum, off);
  PCHK(launch_ok(c, "k_db_scan_sums"));
  hipLaunchKernelGGL(pd::k_db_scan_offsets, dim3(nchunks), dim3(pd::DB_THREADS), 0, c->stream, cnt, nw, bsum, off, cursor);
  PCHK(launch_ok(c, "k_db_scan_offsets"));
  hipLaunchKernelGGL(pd::k_db_scatter, dim3((unsigned)db->size), dim3(pd::DB_STORE_THREADS), 0, c->stream, dbs, nw,
                     db->fwd_word.as<uint32_t>(), db->fwd_weight.as<uint32_t>(), db->fwd_n.as<uint32_t>(), cursor,
                     db->post.as<uint2>());
  return launch_ok(c, "k_db_scatter");
}

PISLAM_EXPORT int pislam_bowdb_remove(pislam_ctx *c, pislam_bowdb *db, const int32_t *ids, int n) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!db) return fail(c, PISLAM_ERR_INVALID, "null database");
  if (db->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the database lives on another device");
  if (n < 0 || (n > 0 && !ids)) return fail(c, PISLAM_ERR_INVALID, "null ids");
  for (int k = 0; k < n; k++) {                         // validate first: nothing changes on an error
    bool bad = ids[k] < 0 || ids[k] >= db->size || !db->alive[(size_t)ids[k]];
    for (int j = 0; j < k && !bad; j++) bad = ids[j] == ids[k];
    if (bad) return fail(c, PISLAM_ERR_INVALID, "unknown, removed or repeated key-frame id");
  }
  if (n == 0) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // (the postings of a removed key frame stay in the inverted file until pislam_bowdb_clear: the query reads the flag)
  for (int k = 0; k < n; k++) {
    HIPCHK(c, hipMemsetAsync(db->d_alive.as<uint8_t>() + ids[k], 0, 1, c->stream));
    db->alive[(size_t)ids[k]] = 0;
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_bowdb_clear(pislam_ctx *c, pislam_bowdb *db) {
  if (!c) return PISLAM_ERR_INVALID;
  if (!db) return fail(c, PISLAM_ERR_INVALID, "null database");
  if (db->device != c->device) return fail(c, PISLAM_ERR_INVALID, "the database lives on another device");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(db->d_size.p, 0, 4, c->stream));
  HIPCHK(c, hipMemsetAsync(db->cnt.p, 0, 4 * (size_t)db->nwords, c->stream));
  HIPCHK(c, hipMemsetAsync(db->d_alive.p, 0, (size_t)db->capacity, c->stream));
  std::fill(db->alive.begin(), db->alive.end(), 0);
  db->size = 0;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_bowdb_query_reserve(pislam_ctx *c, const pislam_bowdb *db, int batch, int topk) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(db_query_args(c, db, batch, topk));
  HIPCHK(c, hipSetDevice(c->device));
  return db_query_workspace(c, db_query_plan(db->capacity, batch, topk));
}

PISLAM_EXPORT int pislam_bowdb_query_batch(pislam_ctx *c, const pislam_bowdb *db, const uint32_t *q_word,
                                           const uint32_t *q_weight, const uint32_t *q_n, size_t stride, int batch,
                                           const int32_t *id_limit, int min_common_pct, int topk, int32_t *top_id,
                                           uint32_t *top_score, uint32_t *top_common, uint32_t *max_common) {
  if (!c) return PISLAM_ERR_INVALID;
  PCHK(db_query_args(c, db, batch, topk));
  if (stride > (size_t)pd::DB_MAX_STRIDE) return fail(c, PISLAM_ERR_INVALID, "stride must be at most 16384");
  if (min_common_pct < 0 || min_common_pct > 100) return fail(c, PISLAM_ERR_INVALID, "min_common_pct must be 0..100");
  if (id_limit && !is_device_ptr(id_limit)) return fail(c, PISLAM_ERR_INVALID, "id_limit must be a device pointer or null");
  if (batch == 0) return PISLAM_OK;
  PCHK(device_ptrs(c, {q_word, q_weight, q_n, top_id, top_score, top_common, max_common},
                   "the database query takes device pointers only"));
  HIPCHK(c, hipSetDevice(c->device));
  const DbQueryPlan P = db_query_plan(db->capacity, batch, topk);
  PCHK(db_query_workspace(c, P));
  uint8_t *ws = c->w_db.as<uint8_t>();
  uint32_t *acc_score = (uint32_t *)(ws + P.o_score), *acc_common = (uint32_t *)(ws + P.o_common);
  uint32_t *gmax = (uint32_t *)(ws + P.o_gmax), *pcom = (uint32_t *)(ws + P.o_pcom);
  uint64_t *pkey = (uint64_t *)(ws + P.o_pkey);
  const uint32_t *dsize = db->d_size.as<uint32_t>();
  const uint8_t *alive = db->d_alive.as<uint8_t>();
  HIPCHK(c, hipMemsetAsync(gmax, 0, 4 * (size_t)batch, c->stream));
  hipLaunchKernelGGL(pd::k_db_accumulate, dim3(P.nslices, (unsigned)batch), dim3(pd::DB_THREADS), P.lds, c->stream, db->nwords,
                     P.cap_pad, P.slice, dsize, alive, db->off.as<uint32_t>(), db->post.as<uint2>(), q_word, q_weight, q_n,
                     stride, id_limit, acc_score, acc_common, gmax);
  PCHK(launch_ok(c, "k_db_accumulate"));
  hipLaunchKernelGGL(pd::k_db_select, dim3(P.nsel, (unsigned)batch), dim3(pd::DB_THREADS), 0, c->stream, P.cap_pad, dsize,
                     alive, id_limit, (uint32_t)min_common_pct, topk, acc_score, (const uint16_t *)acc_common, gmax, pkey, pcom,
                     top_id, top_score, top_common, max_common);
  PCHK(launch_ok(c, "k_db_select"));
  if (P.nsel > 1) {
    hipLaunchKernelGGL(pd::k_db_merge, dim3((unsigned)batch), dim3(pd::DB_THREADS), 0, c->stream, P.nsel, topk, pkey, pcom,
                       gmax, top_id, top_score, top_common, max_common);
    PCHK(launch_ok(c, "k_db_merge"));
  }
  return PISLAM_OK;
}

// ---- batches in flight: a pipeline of contexts behind one object --------------------------------
// One batch call at a time leaves the GPU's issue slots idle at the seams of a step (the strip kernel's tail of
// partly filled CUs, the latency-bound gather + ORB kernel, launch gaps): 0.27 ms per 256 VGA pyramids against
// 0.23 ms with three whole batches in flight.  (Overlapping INSIDE one call was built twice and measured slower
// both times — sub-batches on a second stream, strip and ORB workgroups in one grid: DESIGN.md.)  The pipeline
// object is that choreography as library API: `depth` lanes, each a context (workspace + non-blocking stream)
// of its own; batch k runs on lane k % depth, ordered after the producer of its input (an event on the caller's
// stream) and after the lane's previous batch; the caller orders its consumers with pislam_pipeline_wait.
//
// A steady stream of batches repeats its calls exactly (same buffers, same shape): a lane replays such a call from
// a hipGraph — first occurrence eager (it may size the workspace), second captured, replayed from then on
// (3 launches + 4 event records per call become one graph launch: -2.5 % per batch at depth 3).
struct LaneCall {
  pislam_frontend_params p;
  std::vector<pislam_level> lv;
  const uint8_t *pyramids;
  size_t stride;
  int batch;
  uint32_t *kp, *desc, *counts;
  hipGraphExec_t exec = nullptr;       // nullptr: seen once, not captured yet
  bool failed = false;                 // capture / instantiation failed: stay eager
  unsigned long long ws_gen = 0;       // the lane context's workspace_generation() the graph was captured against
  bool recapture = false;              // the graph was dropped because the workspace moved: next occurrence eager, then capture
  int invalidations = 0;               // times that happened: calls that keep re-laying the lane's workspace (two repeating calls
                                       // whose overflow-list layouts differ) stop being captured after 3 — each invalidation costs a
                                       // stream drain, an eager run and a recapture, more than the graph ever returns
  unsigned long long last_use = 0;
  unsigned path = 0;                   // pislam_frontend_last_path of the captured call (a replay restores it)
  int pipeline_kind = 0;
  uint32_t strips = 0;
  bool same(const pislam_frontend_params *q, const pislam_level *l, const uint8_t *py, size_t st, int b, uint32_t *k,
            uint32_t *d, uint32_t *c) const {
    return pyramids == py && stride == st && batch == b && kp == k && desc == d && counts == c &&
           memcmp(&p, q, sizeof(p)) == 0 && (int)lv.size() == q->nlevels &&
           memcmp(lv.data(), l, sizeof(pislam_level) * lv.size()) == 0;
  }
};

struct pislam_pipeline {
  int device = 0, depth = 0;
  int use_graphs = 1;                  // option "graphs"
  std::vector<std::vector<LaneCall>> calls;   // per lane, at most 4 remembered calls
  std::vector<pislam_ctx *> lane;
  std::vector<hipEvent_t> done;        // completion of the lane's last batch
  hipEvent_t in_ready = nullptr;       // producer stream -> lane stream
  unsigned long long submitted = 0;
  unsigned long long n_replayed = 0, n_captured = 0, n_capture_failed = 0, n_invalidated = 0;
  std::string err;
};

namespace {
// An exec may still be in flight on its lane: the lane's stream is drained before one is destroyed (rare events:
// an option change, an eviction, a workspace that moved).
void destroy_exec(pislam_ctx *c, LaneCall &lc) {
  if (!lc.exec) return;
  (void)hipStreamSynchronize(c->stream);
  (void)hipGraphExecDestroy(lc.exec);
  lc.exec = nullptr;
}
void drop_lane_calls(pislam_pipeline *q) {
  for (size_t li = 0; li < q->calls.size(); li++) {
    for (auto &lc : q->calls[li]) destroy_exec(q->lane[li], lc);
    q->calls[li].clear();
  }
}
}  // namespace

PISLAM_EXPORT int pislam_pipeline_destroy(pislam_pipeline *q) {
  if (!q) return PISLAM_ERR_INVALID;
  (void)hipSetDevice(q->device);
  for (auto *c : q->lane)
    if (c) (void)hipStreamSynchronize(c->stream);
  drop_lane_calls(q);
  for (auto *c : q->lane)
    if (c) (void)pislam_ctx_destroy(c);
  for (auto e : q->done)
    if (e) (void)hipEventDestroy(e);
  if (q->in_ready) (void)hipEventDestroy(q->in_ready);
  delete q;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_create(int device, int depth, pislam_pipeline **out) {
  if (!out || depth < 1 || depth > 8) return PISLAM_ERR_INVALID;
  *out = nullptr;
  pislam_pipeline *q = new pislam_pipeline();
  q->depth = depth;
  q->calls.resize(depth);
  for (int i = 0; i < depth; i++) {
    pislam_ctx *c = nullptr;
    int rc = pislam_ctx_create(device, &c);
    if (rc == PISLAM_OK) rc = use_own_stream(c, 2);
    if (rc == PISLAM_OK) c->opt.lanes_in_flight = depth;
    hipEvent_t e = nullptr;
    if (rc == PISLAM_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = PISLAM_ERR_HIP;
    if (c) {
      q->lane.push_back(c);
      q->device = c->device;
    }
    if (e) q->done.push_back(e);
    if (rc != PISLAM_OK) {
      (void)pislam_pipeline_destroy(q);
      return rc;
    }
  }
  if (hipEventCreateWithFlags(&q->in_ready, hipEventDisableTiming) != hipSuccess) {
    (void)pislam_pipeline_destroy(q);
    return PISLAM_ERR_HIP;
  }
  *out = q;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_depth(const pislam_pipeline *q) { return q ? q->depth : 0; }
PISLAM_EXPORT pislam_ctx *pislam_pipeline_lane(pislam_pipeline *q, int lane) {
  return q && lane >= 0 && lane < q->depth ? q->lane[lane] : nullptr;
}
PISLAM_EXPORT void *pislam_pipeline_stream(pislam_pipeline *q, uint64_t ticket) {
  return q ? (void *)q->lane[ticket % q->depth]->stream : nullptr;
}
PISLAM_EXPORT const char *pislam_pipeline_last_error(const pislam_pipeline *q) { return q ? q->err.c_str() : "null pipeline"; }

PISLAM_EXPORT int pislam_pipeline_set_option(pislam_pipeline *q, const char *key, int value) {
  if (!q || !key) return PISLAM_ERR_INVALID;
  drop_lane_calls(q);                  // options change what a call launches: captured calls are dropped
  if (!strcmp(key, "graphs")) {        // 1 (default): repeated calls are replayed from hipGraphs; 0: always eager
    q->use_graphs = value != 0;
    return PISLAM_OK;
  }
  for (auto *c : q->lane) {
    const int rc = pislam_ctx_set_option(c, key, value);
    if (rc != PISLAM_OK) {
      q->err = c->err;
      return rc;
    }
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_reserve(pislam_pipeline *q, const pislam_frontend_params *p, const pislam_level *lv,
                                          int batch) {
  if (!q) return PISLAM_ERR_INVALID;
  for (auto *c : q->lane) {
    const int rc = pislam_frontend_reserve(c, p, lv, batch);
    if (rc != PISLAM_OK) {
      q->err = c->err;
      return rc;
    }
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_submit(pislam_pipeline *q, const pislam_frontend_params *p, const pislam_level *lv,
                                         const uint8_t *pyramids, size_t stride, int batch, uint32_t *kp, uint32_t *desc,
                                         uint32_t *counts, void *input_stream, int order_after_input, uint64_t *ticket) {
  if (!q) return PISLAM_ERR_INVALID;
  const int li = (int)(q->submitted % q->depth);
  pislam_ctx *c = q->lane[li];
  if (hipSetDevice(q->device) != hipSuccess) {
    q->err = "hipSetDevice";
    return PISLAM_ERR_HIP;
  }
  if (order_after_input) {
    // the lane's stream waits (on the device) for everything `input_stream` holds so far: the producer of `pyramids`
    hipError_t e = hipEventRecord(q->in_ready, (hipStream_t)input_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, q->in_ready, 0);
    if (e != hipSuccess) {
      q->err = std::string("pislam_pipeline_submit: ordering after the input stream: ") + hipGetErrorString(e);
      (void)hipGetLastError();
      return PISLAM_ERR_HIP;
    }
  }
  int rc = check_frame_poison(c);      // (a one-launch call of this lane timed out: reported once, graphs dropped below)
  if (rc != PISLAM_OK) {
    q->err = c->err;
    return rc;
  }
  LaneCall *hit = nullptr;
  if (q->use_graphs && p && lv && p->nlevels >= 1 && p->nlevels <= 16) {
    auto &v = q->calls[li];
    for (auto &lc : v)
      if (lc.same(p, lv, pyramids, stride, batch, kp, desc, counts)) hit = &lc;
    if (hit && hit->exec && hit->ws_gen != c->workspace_generation()) {
      // a larger call on this lane (or pislam_pipeline_reserve, or a direct call on pislam_pipeline_lane()) moved a
      // workspace buffer or re-laid the overflow lists since the capture: the graph holds stale addresses.  This
      // occurrence runs eagerly (it re-establishes the layout, as a first occurrence would), the next one captures.
      destroy_exec(c, *hit);
      hit->recapture = true;
      q->n_invalidated++;
      if (++hit->invalidations >= 3) hit->failed = true;   // (stays eager from now on)
    }
    if (hit && hit->recapture) {
      hit->recapture = false;
      hit->last_use = q->submitted;
    } else if (!hit) {                 // first occurrence: remember it, run it eagerly
      if (v.size() >= 4) {
        size_t old = 0;
        for (size_t i = 1; i < v.size(); i++)
          if (v[i].last_use < v[old].last_use) old = i;
        destroy_exec(c, v[old]);
        v.erase(v.begin() + old);
      }
      LaneCall lc;
      lc.p = *p;
      lc.lv.assign(lv, lv + p->nlevels);
      lc.pyramids = pyramids;
      lc.stride = stride;
      lc.batch = batch;
      lc.kp = kp;
      lc.desc = desc;
      lc.counts = counts;
      lc.last_use = q->submitted;
      v.push_back(lc);
    } else if (!hit->exec && !hit->failed) {          // second occurrence: capture
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        rc = pislam_orb_frontend_batch(c, p, lv, pyramids, stride, batch, kp, desc, counts);
        e = hipStreamEndCapture(c->stream, &g);
        if (e == hipSuccess && rc == PISLAM_OK) e = hipGraphInstantiate(&hit->exec, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
      }
      if (e != hipSuccess || rc != PISLAM_OK || !hit->exec) {
        (void)hipGetLastError();
        hit->exec = nullptr;
        hit->failed = true;            // (whatever went wrong: this call stays eager)
        rc = PISLAM_OK;
        q->n_capture_failed++;
      } else {
        hit->ws_gen = c->workspace_generation();
        hit->path = c->last_path;
        hit->pipeline_kind = c->last_pipeline;
        hit->strips = c->last_strips;
        q->n_captured++;
      }
    }
  }
  if (hit && hit->exec) {
    hit->last_use = q->submitted;
    if (hipGraphLaunch(hit->exec, c->stream) != hipSuccess) {
      q->err = "hipGraphLaunch";
      (void)hipGetLastError();
      return PISLAM_ERR_HIP;
    }
    c->timing_valid = false;           // (the timing events were recorded inside the captured call)
    c->last_path = hit->path;          // what pislam_frontend_last_path / last_stats report is the replayed call's
    c->last_pipeline = hit->pipeline_kind;
    c->last_strips = hit->strips;
    q->n_replayed++;
  } else {
    rc = pislam_orb_frontend_batch(c, p, lv, pyramids, stride, batch, kp, desc, counts);
    if (rc != PISLAM_OK) {
      q->err = c->err;
      return rc;
    }
  }
  if (hipEventRecord(q->done[li], c->stream) != hipSuccess) {
    q->err = "hipEventRecord";
    (void)hipGetLastError();
    return PISLAM_ERR_HIP;
  }
  if (ticket) *ticket = q->submitted;
  q->submitted++;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_wait(pislam_pipeline *q, uint64_t ticket, void *stream) {
  if (!q) return PISLAM_ERR_INVALID;
  if (ticket >= q->submitted) {
    q->err = "no such ticket";
    return PISLAM_ERR_INVALID;
  }
  // A lane's stream is in order: when the lane has taken a later batch since, its newer event covers this one.
  if (hipSetDevice(q->device) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, q->done[ticket % q->depth], 0) != hipSuccess) {
    q->err = "hipStreamWaitEvent";
    (void)hipGetLastError();
    return PISLAM_ERR_HIP;
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_stats(const pislam_pipeline *q, uint64_t stats[4]) {
  if (!q || !stats) return PISLAM_ERR_INVALID;
  stats[0] = q->submitted;
  stats[1] = q->n_replayed;
  stats[2] = q->n_captured;
  stats[3] = q->n_capture_failed;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_pipeline_synchronize(pislam_pipeline *q) {
  if (!q) return PISLAM_ERR_INVALID;
  for (auto *c : q->lane) {
    int rc = sync(c);
    if (rc == PISLAM_OK) rc = check_frame_poison(c);
    if (rc != PISLAM_OK) {
      q->err = c->err;
      return rc;
    }
  }
  return PISLAM_OK;
}

// ---- multi-GPU: shard + count all-gather over RCCL -------------------------------
#include "pislam_dist.inc"
