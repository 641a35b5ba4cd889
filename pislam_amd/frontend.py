"""Host-side mirror of the reference's public interface for the ORB hot path.

Same names, argument order and semantics as the header-only templates of
0xfaded/pislam (include/Fast.h, Harris.h, Orb.h, Brief.h, Util.h); the template
parameters (vstep, border, logBucketSize, bucketLimit, words) become keyword
arguments, `vstep` is taken from the array's row stride.  Every function forwards
to the C ABI of libpislam_hip.so — nothing is computed in Python and nothing
falls back to the CPU.

The batched matchers and the back-end calls behind them (match selection, two-view geometry, pose and Sim(3) estimation,
new map points, local bundle adjustment, the pose graph, bag of words) live here too; they have no counterpart in the
reference, and their contracts are the comments in include/pislam_hip.h.

Arrays may be numpy (host; staged through the device by the library) or torch
CUDA/HIP tensors (used in place).
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from . import capi
from .capi import (ClaheParams, Context, FrontendParams, Level, LkParams, SelectParams, StereoParams, TwoViewParams,
                   ptr)

_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


# ---- Util.h:27-45 ----------------------------------------------------------
def encodeFast(score, x, y):
    return ((np.uint32(score) << np.uint32(24)) | (np.uint32(x) << np.uint32(12)) | np.uint32(y)).astype(np.uint32) \
        if isinstance(score, np.ndarray) else ((int(score) << 24) | (int(x) << 12) | int(y)) & 0xFFFFFFFF


def rencodeFastScore(score, encoded):
    return ((int(score) << 24) | (int(encoded) & 0xFFFFFF)) & 0xFFFFFFFF


def decodeFastX(encoded):
    return (encoded >> 12) & 0xFFF


def decodeFastY(encoded):
    return encoded & 0xFFF


def decodeFastScore(encoded):
    return encoded >> 24


def _vstep(a) -> int:
    if a.ndim != 2:
        raise ValueError("image / score map must be 2-D [rows][vstep]")
    return int(a.shape[1])


# ---- Fast.h:54 ---------------------------------------------------------------
def fastDetect(width, height, img, out, threshold, *, border=16, ctx: Context | None = None):
    """pislam::fastDetect<vstep,border>(width, height, img, out, threshold)."""
    ctx = ctx or default_context()
    vstep = _vstep(img)
    if isinstance(img, np.ndarray) and width > 2 * border and height > 2 * border:
        # flat addressing of the over-classified columns (see pislam_hip.h): never read past the array
        need = (height - border + 2) * vstep + border + 16 * (-(-(width - 2 * border) // 16)) + 3
        if need > img.size:
            pad = np.zeros(need, np.uint8)
            pad[:img.size] = img.reshape(-1)
            img = pad
    ctx.check(ctx.lib.pislam_fast_detect(ctx.h, vstep, border, width, height, ptr(img), ptr(out),
                                         threshold), "pislam_fast_detect")


# ---- Fast.h:166 --------------------------------------------------------------
def fastScoreHarris(width, height, img, threshold, out, *, border=16, ctx: Context | None = None):
    """pislam::fastScoreHarris<vstep,border>(width, height, img, threshold, out)."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_fast_score_harris(ctx.h, _vstep(img), border, width, height, ptr(img),
                                               threshold, ptr(out)), "pislam_fast_score_harris")


# ---- Fast.h:196 --------------------------------------------------------------
def fastExtract(width, height, out, results: list | None = None, *, border=16, logBucketSize=0,
                bucketLimit=5, ctx: Context | None = None) -> np.ndarray:
    """pislam::fastExtract<vstep,border,logBucketSize,bucketLimit>(width, height, out, results).

    Appends to `results` (a Python list, like the reference's std::vector&) when given and
    returns the keypoints of this call as a uint32 array."""
    ctx = ctx or default_context()
    cap = max(16, ((width + 1) // 2) * ((height + 1) // 2))
    buf = np.zeros(cap, np.uint32)
    n = ctypes.c_size_t(0)
    ctx.check(ctx.lib.pislam_fast_extract(ctx.h, _vstep(out), border, logBucketSize, bucketLimit, width,
                                          height, ptr(out), ptr(buf), cap, ctypes.byref(n)),
              "pislam_fast_extract")
    kp = buf[:n.value].copy()
    if results is not None:
        results.extend(int(v) for v in kp)
    return kp


# ---- Harris.h:80 ---------------------------------------------------------------
def harrisScoreSobel(img, x, y, threshold, *, ctx: Context | None = None) -> int:
    """pislam::harrisScoreSobel<vstep>(img, x, y, threshold)."""
    return int(harrisScorePoints(img, np.array([(int(x) << 12) | int(y)], np.uint32), threshold, ctx=ctx)[0])


def harrisScorePoints(img, points, threshold, *, ctx: Context | None = None) -> np.ndarray:
    ctx = ctx or default_context()
    points = np.ascontiguousarray(points, np.uint32)
    scores = np.zeros(len(points), np.uint8)
    ctx.check(ctx.lib.pislam_harris_score_points(ctx.h, _vstep(img), ptr(img), ptr(points), len(points),
                                                 threshold, ptr(scores)), "pislam_harris_score_points")
    return scores


# ---- Orb.h:80 ------------------------------------------------------------------
def orbCentroids(img, points, *, ctx: Context | None = None) -> np.ndarray:
    """pislam::orbCentroids<vstep>(img, points): int32, groups [x0 x1 x2 x3 y0 y1 y2 y3]."""
    ctx = ctx or default_context()
    points = np.ascontiguousarray(points, np.uint32)
    n8 = ctx.lib.pislam_centroids_size(len(points))
    cen = np.zeros(n8, np.int32)
    ctx.check(ctx.lib.pislam_orb_centroids(ctx.h, _vstep(img), ptr(img), ptr(points), len(points),
                                           ptr(cen)), "pislam_orb_centroids")
    return cen


# ---- Orb.h:310 -----------------------------------------------------------------
def atan2(xys, *, ctx: Context | None = None) -> np.ndarray:
    """pislam::atan2(const std::vector<int32_t>&): uint8 angle bins, padding slots included."""
    ctx = ctx or default_context()
    xys = np.ascontiguousarray(xys, np.int32)
    ang = np.zeros(len(xys) // 2, np.uint8)
    ctx.check(ctx.lib.pislam_orb_angles(ctx.h, ptr(xys), len(xys), ptr(ang)), "pislam_orb_angles")
    return ang


# ---- Brief.h:637 ---------------------------------------------------------------
def briefDescribe(img, x, y, rot, *, words=8, ctx: Context | None = None) -> np.ndarray:
    """pislam::briefDescribe<vstep,words>(img, x, y, rot, descriptor)."""
    pts = np.array([(int(x) << 12) | int(y)], np.uint32)
    return briefDescribePoints(img, pts, np.array([rot], np.uint8), words=words, ctx=ctx)[0]


def briefDescribePoints(img, points, rots, *, words=8, ctx: Context | None = None) -> np.ndarray:
    ctx = ctx or default_context()
    points = np.ascontiguousarray(points, np.uint32)
    rots = np.ascontiguousarray(rots, np.uint8)
    desc = np.zeros((len(points), words), np.uint32)
    ctx.check(ctx.lib.pislam_brief_describe(ctx.h, _vstep(img), words, ptr(img), ptr(points), ptr(rots),
                                            len(points), ptr(desc)), "pislam_brief_describe")
    return desc


# ---- Orb.h:396 -----------------------------------------------------------------
def orbCompute(img, points, descriptors: list | None = None, *, words=8,
               ctx: Context | None = None) -> np.ndarray:
    """pislam::orbCompute<vstep,words>(img, points, descriptors); returns uint32 [n][words] and
    appends the flattened words to `descriptors` when given."""
    ctx = ctx or default_context()
    points = np.ascontiguousarray(points, np.uint32)
    desc = np.zeros((len(points), words), np.uint32)
    ctx.check(ctx.lib.pislam_orb_compute(ctx.h, _vstep(img), words, ptr(img), ptr(points), len(points),
                                         ptr(desc)), "pislam_orb_compute")
    if descriptors is not None:
        descriptors.extend(int(v) for v in desc.reshape(-1))
    return desc


# ---- descriptor matching (no reference counterpart) -----------------
def matchHamming(query, train, *, ctx: Context | None = None):
    """Brute-force Hamming matching of uint32 [n][words] descriptors (numpy or torch): returns
    (idx int32 [nq], dist uint32 [nq], dist2 uint32 [nq]) — nearest train index (ties: smallest
    index, -1 without train descriptors), its distance, and the best distance among the others."""
    ctx = ctx or default_context()
    query = np.ascontiguousarray(query, np.uint32)
    train = np.ascontiguousarray(train, np.uint32)
    words = query.shape[1] if query.ndim == 2 and len(query) else (train.shape[1] if train.ndim == 2 else 8)
    nq, nt = len(query), len(train)
    idx = np.zeros(nq, np.int32)
    dist = np.zeros(nq, np.uint32)
    dist2 = np.zeros(nq, np.uint32)
    ctx.check(ctx.lib.pislam_match_hamming(ctx.h, words, ptr(query) if nq else None, nq, ptr(train) if nt else None, nt,
                                           ptr(idx) if nq else None, ptr(dist) if nq else None,
                                           ptr(dist2) if nq else None), "pislam_match_hamming")
    return idx, dist, dist2


def _match_outputs(qdesc, idx, dist, dist2):
    """The (idx, dist, dist2) of a batched matcher: each the caller's tensor, or a new int32 one [batch][q_stride] on the
    device of the query descriptors [batch][q_stride][words]."""
    import torch
    new = lambda t: torch.empty(tuple(qdesc.shape[:2]), dtype=torch.int32, device=qdesc.device) if t is None else t
    return new(idx), new(dist), new(dist2)


def matchHammingBatch(qdesc, qcounts, tdesc, tcounts, idx=None, dist=None, dist2=None, *, ctx: Context | None = None):
    """Batched matcher on device-resident front-end outputs (torch tensors [batch][max_kp][words] and
    [batch] counts, as OrbFrontend writes them): pair b matches the first min(qcounts[b], q_stride) descriptors of
    qdesc[b] against the first min(tcounts[b], t_stride) of tdesc[b] (t_stride <= 65535).  Returns (idx, dist, dist2)
    int32 tensors [batch][q_stride]: idx as matchHamming; dist and dist2 hold the library's uint32 values viewed as
    int32, so "none" (0xffffffff: no train descriptor, or for dist2 fewer than two) reads as -1.  Entries at and beyond
    a pair's query count are not written.  Asynchronous on the ctx stream."""
    ctx = ctx or default_context()
    batch, qs, words = qdesc.shape
    ts = tdesc.shape[1]
    idx, dist, dist2 = _match_outputs(qdesc, idx, dist, dist2)
    ctx.check(ctx.lib.pislam_match_hamming_batch(ctx.h, words, ptr(qdesc), ptr(qcounts), qs, ptr(tdesc), ptr(tcounts), ts,
                                                 batch, ptr(idx), ptr(dist), ptr(dist2)), "pislam_match_hamming_batch")
    return idx, dist, dist2


def _window_tables(levels, radius):
    """levels [(w, h, row0[, col0])] and radius (int, or one per level) as the C arrays of the windowed matcher."""
    lv = [Level(t[0], t[1], t[2], t[3] if len(t) > 3 else 0) for t in levels]
    r = [int(radius)] * len(lv) if isinstance(radius, (int, np.integer)) else [int(v) for v in radius]
    if len(r) != len(lv):
        raise ValueError(f"radius: {len(r)} values for {len(lv)} levels")
    n = max(1, len(lv))
    return (Level * n)(*lv), len(lv), (ctypes.c_int32 * n)(*r)


def reserveMatchWindow(levels, radius, t_stride: int, batch: int, *, words=8, ctx: Context | None = None):
    """Sizes the context's windowed-matcher workspace (pislam_match_window_reserve): afterwards
    matchHammingWindowBatch of the same or a smaller shape allocates nothing and can be captured into a hipGraph."""
    ctx = ctx or default_context()
    lv, n, r = _window_tables(levels, radius)
    ctx.check(ctx.lib.pislam_match_window_reserve(ctx.h, words, lv, n, r, t_stride, batch), "pislam_match_window_reserve")


def matchHammingWindowBatch(qkp, qdesc, qcounts, tkp, tdesc, tcounts, levels, radius, idx=None, dist=None, dist2=None, *,
                            ctx: Context | None = None):
    """Spatially windowed matcher on device-resident front-end outputs (torch tensors as OrbFrontend.alloc_outputs
    makes them: keypoints [batch][max_kp], descriptors [batch][max_kp][words], counts [batch]): query i of pair b sees
    only the train keypoints on its own level within `radius` (int, or one per level) in x and in y.  `levels` is
    [(w, h, row0[, col0])].  Returns (idx, dist, dist2) int32 tensors [batch][max_kp] like matchHammingBatch
    (pislam_match_hamming_window_batch); asynchronous on the ctx stream."""
    ctx = ctx or default_context()
    batch, qs, words = qdesc.shape
    ts = tdesc.shape[1]
    if tdesc.shape[2] != words:
        raise ValueError("query and train descriptors differ in words")
    lv, n, r = _window_tables(levels, radius)
    idx, dist, dist2 = _match_outputs(qdesc, idx, dist, dist2)
    ctx.check(ctx.lib.pislam_match_hamming_window_batch(ctx.h, words, lv, n, r, ptr(qkp), ptr(qdesc), ptr(qcounts), qs,
                                                        ptr(tkp), ptr(tdesc), ptr(tcounts), ts, batch, ptr(idx), ptr(dist),
                                                        ptr(dist2)), "pislam_match_hamming_window_batch")
    return idx, dist, dist2


def level_scales_q16(levels):
    """Q16 level-0 pixels per level pixel of each level, from the level table alone: round(65536 * width_0 / width_l)
    (halves round up), the scale_q16 of matchHammingScaledWindowBatch."""
    w0 = int(levels[0][0])
    return [(2 * 65536 * w0 + int(t[0])) // (2 * int(t[0])) for t in levels]


def _scaled_tables(levels, scale_q16, radius0):
    """levels, scale_q16 and radius0 (int, or one per level; scale_q16 None = level_scales_q16) as C arrays."""
    lv, n, r = _window_tables(levels, radius0)
    if scale_q16 is None:
        scale_q16 = level_scales_q16(levels)
    s = [int(scale_q16)] * n if isinstance(scale_q16, (int, np.integer)) else [int(v) for v in scale_q16]
    if len(s) != n:
        raise ValueError(f"scale_q16: {len(s)} values for {n} levels")
    return lv, n, (ctypes.c_int32 * max(1, n))(*s), r


def reserveMatchScaledWindow(levels, scale_q16, radius0, level_span: int, t_stride: int, batch: int, *, words=8,
                             ctx: Context | None = None):
    """Sizes the context's scaled-window workspace (pislam_match_scaled_window_reserve): afterwards
    matchHammingScaledWindowBatch of the same or a smaller shape allocates nothing and can be captured into a hipGraph."""
    ctx = ctx or default_context()
    lv, n, s, r = _scaled_tables(levels, scale_q16, radius0)
    ctx.check(ctx.lib.pislam_match_scaled_window_reserve(ctx.h, words, lv, n, s, r, level_span, t_stride, batch),
              "pislam_match_scaled_window_reserve")


def matchHammingScaledWindowBatch(qkp, qdesc, qcounts, tkp, tdesc, tcounts, levels, scale_q16, radius0, level_span=1,
                                  qpred=None, idx=None, dist=None, dist2=None, *, ctx: Context | None = None):
    """Scale-aware guided window matcher (pislam_match_hamming_scaled_window_batch) on device-resident front-end
    outputs laid out as for matchHammingWindowBatch.  Positions map to level 0 through scale_q16 (Q16 level-0 pixels
    per level pixel, int or one per level; None = level_scales_q16(levels)); query i on level lq sees the train
    keypoints on levels lq - level_span .. lq + level_span within radius0[lq] (level-0 pixels, int or one per level)
    of its window centre: its own mapped position, or qpred[b][i] = (X, Y) (int32 device tensor [batch][q_stride][2])
    when given.  Returns (idx, dist, dist2) int32 tensors [batch][q_stride]; asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, qs, words = qdesc.shape
    ts = tdesc.shape[1]
    if tdesc.shape[2] != words:
        raise ValueError("query and train descriptors differ in words")
    if qpred is not None and (qpred.dtype != torch.int32 or tuple(qpred.shape) != (batch, qs, 2)):
        raise ValueError("qpred must be an int32 tensor [batch][q_stride][2]")
    lv, n, s, r = _scaled_tables(levels, scale_q16, radius0)
    idx, dist, dist2 = _match_outputs(qdesc, idx, dist, dist2)
    ctx.check(ctx.lib.pislam_match_hamming_scaled_window_batch(ctx.h, words, lv, n, s, r, int(level_span), ptr(qkp),
                                                               ptr(qdesc), ptr(qcounts), ptr(qpred), qs, ptr(tkp),
                                                               ptr(tdesc), ptr(tcounts), ts, batch, ptr(idx), ptr(dist),
                                                               ptr(dist2)), "pislam_match_hamming_scaled_window_batch")
    return idx, dist, dist2


def projectionRadii(scale_q16, th, near=2.5, far=4.0):
    """The (radius_far, radius_near) tables of matchProjectionBatch, ORB-SLAM's th * RadiusByViewingCos * scaleFactor[l]
    in level-0 pixels: per level l, floor(f * th * scale_q16[l] / 65536 + 0.5) with f = far and f = near, evaluated in
    float64 in that order of operations (halves round up) and clamped to 0..65535.  Returns two int32 numpy arrays."""
    s = np.asarray([int(v) for v in scale_q16], dtype=np.float64)

    def table(f):
        return np.clip(np.floor(np.float64(f) * np.float64(th) * s / 65536.0 + 0.5), 0, 65535).astype(np.int32)
    return table(far), table(near)


def _projection_tables(levels, scale_q16, level_scale, radius_far, radius_near, th):
    """levels, scale_q16 (None = level_scales_q16), level_scale (None = float32(scale_q16 / 65536)) and the two radius
    tables (both None = projectionRadii(scale_q16, th); radius_near alone None = NULL, i.e. radius_far) as C arrays."""
    if scale_q16 is None:
        scale_q16 = level_scales_q16(levels)
    if radius_far is None:
        if radius_near is not None:
            raise ValueError("radius_near needs radius_far")
        sq = [int(scale_q16)] * len(levels) if isinstance(scale_q16, (int, np.integer)) else scale_q16
        radius_far, radius_near = (t.tolist() for t in projectionRadii(sq, th))
    lv, n, s, rf = _scaled_tables(levels, scale_q16, radius_far)
    rn = None
    if radius_near is not None:
        rn = _window_tables(levels, radius_near)[2]
    if level_scale is None:
        level_scale = [np.float32(np.float32(v) / np.float32(65536.0)) for v in s[:n]]
    ls = [float(np.float32(v)) for v in np.asarray(level_scale, dtype=np.float32).reshape(-1)]
    if len(ls) != n:
        raise ValueError(f"level_scale: {len(ls)} values for {n} levels")
    return lv, n, s, (ctypes.c_float * max(1, n))(*ls), rf, rn


def reserveMatchProjection(levels, t_stride: int, batch: int, *, scale_q16=None, radius_far=None, radius_near=None, th=3,
                           level_below=1, level_above=0, words=8, ctx: Context | None = None):
    """Sizes the context's projection-matcher workspace (pislam_match_projection_reserve): afterwards
    matchProjectionBatch of the same or a smaller shape allocates nothing and can be captured into a hipGraph.  The
    tables default as in matchProjectionBatch."""
    ctx = ctx or default_context()
    lv, n, s, _, rf, rn = _projection_tables(levels, scale_q16, None, radius_far, radius_near, th)
    ctx.check(ctx.lib.pislam_match_projection_reserve(ctx.h, words, lv, n, s, rf, rn, int(level_below), int(level_above),
                                                      t_stride, batch), "pislam_match_projection_reserve")


def matchProjectionBatch(pose, cam, xw, qdesc, qcounts, tkp, tdesc, tcounts, levels, *, drange=None, normal=None,
                         qlevel=None, scale_q16=None, level_scale=None, radius_far=None, radius_near=None, th=3,
                         bounds=None, cos_min=0.5, cos_near=0.998, level_below=1, level_above=0, second_same_level=True,
                         idx=None, dist=None, dist2=None, pred=None, plevel=None, want_pred=True, want_plevel=True,
                         ctx: Context | None = None):
    """Map-point search by projection (pislam_match_projection_batch; the contract is the comment in
    include/pislam_hip.h), ORB-SLAM's SearchByProjection: per frame b, map points xw (float32 [batch][q_stride][3])
    with descriptors qdesc ([batch][q_stride][words]) are projected through pose (float32 [batch][12]) and cam (float32
    [batch][5]) and matched against the frame's keypoints (tkp, tdesc, tcounts as for matchHammingScaledWindowBatch) in a
    window round the projection on the predicted pyramid level.  Map mode: drange (float32 [batch][q_stride][2] = dmin,
    dmax) and optionally normal (float32 [batch][q_stride][3]); level mode: qlevel (uint8 [batch][q_stride]).  The
    defaults are ORB-SLAM's local-map search: bounds = (min_x, max_x, min_y, max_y) = (0, width_0 - 1, 0, height_0 - 1),
    cos_min 0.5, cos_near 0.998, levels pl - 1 .. pl, the ratio test's runner-up on the best's level only; scale_q16
    None = level_scales_q16(levels), level_scale None = float32(scale_q16 / 65536), radius tables both None =
    projectionRadii(scale_q16, th), radius_near alone None = radius_far.  Returns (idx, dist, dist2, pred, plevel): int32
    [batch][q_stride] three times, pred int32 [batch][q_stride][2] (None with want_pred False) and plevel uint8
    [batch][q_stride] (0xff = not visible; None with want_plevel False).  Asynchronous on the ctx stream."""
    ctx = ctx or default_context()
    batch, qs, words, ts = _projection_inputs(pose, cam, xw, qdesc, qcounts, tkp, tdesc, tcounts, normal, drange, qlevel)
    lv, n, s, ls, rf, rn = _projection_tables(levels, scale_q16, level_scale, radius_far, radius_near, th)
    p = _projection_params(levels, bounds, cos_min, cos_near, level_below, level_above, second_same_level)
    idx, dist, dist2, pred, plevel = _projection_outputs(qdesc, idx, dist, dist2, pred, plevel, want_pred, want_plevel)
    ctx.check(ctx.lib.pislam_match_projection_batch(ctx.h, words, lv, n, s, ls, rf, rn, ctypes.byref(p), ptr(pose), ptr(cam),
                                                    ptr(xw), ptr(normal), ptr(drange), ptr(qlevel), ptr(qdesc),
                                                    ptr(qcounts), qs, ptr(tkp), ptr(tdesc), ptr(tcounts), ts, batch,
                                                    ptr(idx), ptr(dist), ptr(dist2), ptr(pred), ptr(plevel)),
              "pislam_match_projection_batch")
    return idx, dist, dist2, pred, plevel


def _projection_inputs(pose, cam, xw, qdesc, qcounts, tkp, tdesc, tcounts, normal, drange, qlevel, **more):
    """Shape, type and contiguity checks shared by matchProjectionBatch and matchFuseBatch (`more`: further tensors
    that must be contiguous when given); returns (batch, q_stride, words, t_stride)."""
    import torch
    batch, qs, words = (int(v) for v in qdesc.shape)
    ts = int(tdesc.shape[1])
    if int(tdesc.shape[2]) != words:
        raise ValueError("query and train descriptors differ in words")
    if pose.dtype != torch.float32 or tuple(pose.shape) != (batch, 12):
        raise ValueError("pose must be a float32 tensor [batch][12]")
    if cam.dtype != torch.float32 or tuple(cam.shape) != (batch, 5):
        raise ValueError("cam must be a float32 tensor [batch][5]")
    for name, t, k in (("xw", xw, 3), ("normal", normal, 3), ("drange", drange, 2)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (batch, qs, k)):
            raise ValueError(f"{name} must be a float32 tensor [batch][q_stride][{k}]")
    if qlevel is not None and (qlevel.dtype != torch.uint8 or tuple(qlevel.shape) != (batch, qs)):
        raise ValueError("qlevel must be a uint8 tensor [batch][q_stride]")
    for t in (pose, cam, xw, normal, drange, qlevel, qdesc, qcounts, tkp, tdesc, tcounts) + tuple(more.values()):
        if t is not None and not t.is_contiguous():
            raise ValueError("inputs must be contiguous")
    return batch, qs, words, ts


def _projection_params(levels, bounds, cos_min, cos_near, level_below, level_above, second_same_level):
    if bounds is None:
        bounds = (0.0, float(int(levels[0][0]) - 1), 0.0, float(int(levels[0][1]) - 1))
    return capi.ProjectionParams(*(float(v) for v in bounds), float(cos_min), float(cos_near), int(level_below),
                                 int(level_above), 1 if second_same_level else 0)


def _projection_outputs(qdesc, idx, dist, dist2, pred, plevel, want_pred, want_plevel):
    import torch
    batch, qs = int(qdesc.shape[0]), int(qdesc.shape[1])
    dev = qdesc.device
    if idx is None:
        idx = torch.empty((batch, qs), dtype=torch.int32, device=dev)
    if dist is None:
        dist = torch.empty((batch, qs), dtype=torch.int32, device=dev)
    if dist2 is None:
        dist2 = torch.empty((batch, qs), dtype=torch.int32, device=dev)
    if pred is None and want_pred:
        pred = torch.empty((batch, qs, 2), dtype=torch.int32, device=dev)
    if plevel is None and want_plevel:
        plevel = torch.empty((batch, qs), dtype=torch.uint8, device=dev)
    return idx, dist, dist2, pred, plevel


def _fuse_tables(levels, scale_q16, radius_far, th):
    """Fuse's defaults: scale_q16 None = level_scales_q16(levels), radius_far None = projectionRadii(scale_q16, th,
    near=1, far=1)[0] (ORB-SLAM's th * scaleFactor[l])."""
    if scale_q16 is None:
        scale_q16 = level_scales_q16(levels)
    if radius_far is None:
        sq = [int(scale_q16)] * len(levels) if isinstance(scale_q16, (int, np.integer)) else scale_q16
        radius_far = projectionRadii(sq, th, near=1, far=1)[0].tolist()
    return scale_q16, radius_far


def reserveMatchFuse(levels, t_stride: int, batch: int, *, scale_q16=None, radius_far=None, radius_near=None, th=3,
                     level_below=1, level_above=0, words=8, ctx: Context | None = None):
    """Sizes the context's fuse-matcher workspace (pislam_match_fuse_reserve; its own, not the projection matcher's):
    afterwards matchFuseBatch of the same or a smaller shape allocates nothing and can be captured into a hipGraph.  The
    tables default as in matchFuseBatch."""
    ctx = ctx or default_context()
    scale_q16, radius_far = _fuse_tables(levels, scale_q16, radius_far, th)
    lv, n, s, _, rf, rn = _projection_tables(levels, scale_q16, None, radius_far, radius_near, th)
    ctx.check(ctx.lib.pislam_match_fuse_reserve(ctx.h, words, lv, n, s, rf, rn, int(level_below), int(level_above),
                                                t_stride, batch), "pislam_match_fuse_reserve")


def matchFuseBatch(pose, cam, xw, qdesc, qcounts, tkp, tdesc, tobs_q8, tcounts, levels, *, drange=None, normal=None,
                   qlevel=None, qmask=None, inv_sigma2=None, chi2_mono=5.99, chi2_stereo=7.8, scale_q16=None,
                   level_scale=None, radius_far=None, radius_near=None, th=3, bounds=None, cos_min=0.5, cos_near=0.998,
                   level_below=1, level_above=0, second_same_level=True, idx=None, dist=None, dist2=None, pred=None,
                   plevel=None, want_pred=True, want_plevel=True, ctx: Context | None = None):
    """Map-point fusion search (pislam_match_fuse_batch; the contract is the comment in include/pislam_hip.h),
    ORB-SLAM's ORBmatcher::Fuse: matchProjectionBatch with, per candidate keypoint, the chi-square test of the point's
    reprojection error against the keypoint's own observation tobs_q8 (int32 [batch][t_stride][3] = u, v, u_right in Q8
    level-0 pixels, INT32_MIN = monocular: poseObservationsQ8's layout) weighted by inv_sigma2 of the keypoint's level
    (None = poseLevelWeights(nlevels)); cam's bf is used.  qmask (uint8 [batch][q_stride], optional): 0 = the point is
    already in the key frame, or bad.  The defaults are Fuse's: th 3 with radius_far = projectionRadii(scale_q16, th,
    near=1, far=1)[0] and no near radius, levels pl - 1 .. pl, cos_min 0.5, chi2 5.99 / 7.8.  Pass both bounds as
    float("inf") for the Sim(3) form of Fuse (with pose = rigidFromSim3(sim)).  Every other argument and the returned
    (idx, dist, dist2, pred, plevel) are matchProjectionBatch's.  Asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, qs, words, ts = _projection_inputs(pose, cam, xw, qdesc, qcounts, tkp, tdesc, tcounts, normal, drange, qlevel,
                                              tobs_q8=tobs_q8, qmask=qmask)
    if tobs_q8 is None or tobs_q8.dtype != torch.int32 or tuple(tobs_q8.shape) != (batch, ts, 3):
        raise ValueError("tobs_q8 must be an int32 tensor [batch][t_stride][3]")
    if qmask is not None and (qmask.dtype != torch.uint8 or tuple(qmask.shape) != (batch, qs)):
        raise ValueError("qmask must be a uint8 tensor [batch][q_stride]")
    scale_q16, radius_far = _fuse_tables(levels, scale_q16, radius_far, th)
    lv, n, s, ls, rf, rn = _projection_tables(levels, scale_q16, level_scale, radius_far, radius_near, th)
    if inv_sigma2 is None:
        inv_sigma2 = poseLevelWeights(n)
    w = [float(v) for v in np.asarray(inv_sigma2, dtype=np.float32).reshape(-1)]
    if len(w) != n:
        raise ValueError(f"inv_sigma2: {len(w)} values for {n} levels")
    wt = (ctypes.c_float * max(1, n))(*w)
    p = _projection_params(levels, bounds, cos_min, cos_near, level_below, level_above, second_same_level)
    f = capi.FuseParams(float(chi2_mono), float(chi2_stereo))
    idx, dist, dist2, pred, plevel = _projection_outputs(qdesc, idx, dist, dist2, pred, plevel, want_pred, want_plevel)
    ctx.check(ctx.lib.pislam_match_fuse_batch(ctx.h, words, lv, n, s, ls, rf, rn, ctypes.byref(p), wt, ctypes.byref(f),
                                              ptr(pose), ptr(cam), ptr(xw), ptr(normal), ptr(drange), ptr(qlevel),
                                              ptr(qmask), ptr(qdesc), ptr(qcounts), qs, ptr(tkp), ptr(tdesc), ptr(tobs_q8),
                                              ptr(tcounts), ts, batch, ptr(idx), ptr(dist), ptr(dist2), ptr(pred),
                                              ptr(plevel)), "pislam_match_fuse_batch")
    return idx, dist, dist2, pred, plevel


def rigidFromSim3(sim):
    """The pose of matchFuseBatch / matchProjectionBatch for the Sim(3) form of Fuse (Fuse(pKF, Scw, ...)): sim
    [batch][13] = (R row-major, t, s) with Xc = s R Xw + t becomes [batch][12] = (R, t / s); the pixel of a point is
    the same, since the projection divides by z.  Computed in float64 and rounded once to float32.  A torch tensor
    (device or host) or a numpy array, returned as the same kind."""
    if isinstance(sim, np.ndarray):
        a = sim.astype(np.float64)
        if a.ndim != 2 or a.shape[1] != 13:
            raise ValueError("sim must be [batch][13]")
        return np.concatenate([a[:, :9], a[:, 9:12] / a[:, 12:13]], axis=1).astype(np.float32)
    import torch
    if sim.dim() != 2 or int(sim.shape[1]) != 13:
        raise ValueError("sim must be [batch][13]")
    a = sim.to(torch.float64)
    return torch.cat([a[:, :9], a[:, 9:12] / a[:, 12:13]], dim=1).to(torch.float32).contiguous()


def fuseDecisions(sel, qid, tpoint, nobs):
    """What ORBmatcher::Fuse does with each accepted match, after matchFuseBatch and selectMatchesBatch (max_dist 50,
    ratio None, rot_keep 0): sel = (sel_q, sel_t, nsel); qid (integer [batch][q_stride]) is the map's id of each query
    point, tpoint (integer [batch][t_stride]) the id of the point each keypoint holds or -1, nobs (integer [npoints])
    the number of observations of every point.  Per slot s < nsel[b], with o = tpoint[b][sel_t[b][s]] and
    me = qid[b][sel_q[b][s]]:
      o < 0               action 1: add the observation (keep me, drop -1)
      o == me             action 0: nothing to do (keep -1, drop -1)
      nobs[o] > nobs[me]  action 2: the keypoint's point replaces the query (keep o, drop me)
      otherwise           action 3: the query replaces the keypoint's point (keep me, drop o); a tie keeps the query,
                          as ORB-SLAM does.
    The slots at and beyond nsel[b] of sel_q and sel_t are unwritten memory: they are masked before gathering and come
    out as action 0, keep -1, drop -1.  Returns (action uint8, keep int64, drop int64), each [batch][q_stride], slot by
    slot as in sel.  Torch ops on the current torch stream.
    With the caller stay: applying the decisions to the map, in batch order (a point dropped in frame b may be the
    keep of a later frame: follow the chain of replacements across key frames, as ORB-SLAM's GetReplaced does), and
    descriptor / normal updates of the kept points (mapPointsUpdateBatch on the edited map; its nobs is this function's
    nobs for the next round).  With unique=0 in the selection several queries may share one
    keypoint; each gets its decision against the state passed in, not against the others' outcome."""
    import torch
    sel_q, sel_t, nsel = sel
    batch, qs = (int(v) for v in sel_q.shape)
    dev = sel_q.device
    live = torch.arange(qs, device=dev)[None, :] < nsel.to(torch.int64)[:, None]
    zero = torch.zeros_like(live, dtype=torch.int64)
    qi = torch.where(live, sel_q.to(torch.int64), zero).clamp(0, int(qid.shape[1]) - 1)
    ti = torch.where(live, sel_t.to(torch.int64), zero).clamp(0, int(tpoint.shape[1]) - 1)
    me = torch.gather(qid.to(torch.int64), 1, qi)
    o = torch.gather(tpoint.to(torch.int64), 1, ti)
    n = nobs.to(torch.int64).reshape(-1)
    last = max(int(n.shape[0]) - 1, 0)
    n_o, n_me = n[o.clamp(0, last)], n[me.clamp(0, last)]
    none = torch.full_like(me, -1)
    add, same = live & (o < 0), live & (o >= 0) & (o == me)
    theirs = live & (o >= 0) & (o != me) & (n_o > n_me)
    ours = live & (o >= 0) & (o != me) & ~(n_o > n_me)
    action = (add.to(torch.uint8) + 2 * theirs.to(torch.uint8) + 3 * ours.to(torch.uint8)).contiguous()
    keep = torch.where(add | ours, me, torch.where(theirs, o, none))
    drop = torch.where(theirs, me, torch.where(ours, o, none))
    return action, keep.contiguous(), drop.contiguous()


def _stereo_tables(levels, scale_q16, row_radius0, level_span, min_disp, max_disp, max_hamming, sad_radius,
                   search_radius, median_filter):
    """levels, scale_q16 (None = level_scales_q16), row_radius0 (int, or one per level) and the parameters as C."""
    lv, n, s, r = _scaled_tables(levels, scale_q16, row_radius0)
    p = StereoParams(int(level_span), int(min_disp), int(max_disp), int(max_hamming), int(sad_radius),
                     int(search_radius), int(median_filter))
    return lv, n, s, r, p


def reserveMatchStereo(levels, scale_q16, row_radius0, r_stride: int, batch: int, *, min_disp, max_disp, max_hamming=74,
                       level_span=1, sad_radius=5, search_radius=5, median_filter=True, words=8,
                       ctx: Context | None = None):
    """Sizes the context's stereo-matcher workspace (pislam_match_stereo_reserve): afterwards matchStereoBatch of the
    same or a smaller shape allocates nothing and can be captured into a hipGraph."""
    ctx = ctx or default_context()
    lv, n, s, r, p = _stereo_tables(levels, scale_q16, row_radius0, level_span, min_disp, max_disp, max_hamming,
                                    sad_radius, search_radius, median_filter)
    ctx.check(ctx.lib.pislam_match_stereo_reserve(ctx.h, words, lv, n, s, r, ctypes.byref(p), r_stride, batch),
              "pislam_match_stereo_reserve")


def matchStereoBatch(lkp, ldesc, lcounts, rkp, rdesc, rcounts, left_pyr, right_pyr, levels, scale_q16, row_radius0, *,
                     min_disp, max_disp, max_hamming=74, level_span=1, sad_radius=5, search_radius=5,
                     median_filter=True, idx=None, dist=None, disp_q8=None, sad=None, nstereo=None,
                     ctx: Context | None = None):
    """Rectified stereo matcher (pislam_match_stereo_batch): left keypoint i of pair b against the right keypoints of
    pair b inside the row band |Yl - Yr| <= row_radius0[lr] (level-0 pixels, int or one per level) with
    min_disp <= Xl - Xr <= max_disp, on levels within level_span; then an SAD refinement of the matches with
    dist <= max_hamming on the uint8 pyramids left_pyr / right_pyr ([batch][rows][vstep] device tensors of the same
    shape and stride), a parabola fit and, with median_filter, a per-pair median cut.  Keypoints and descriptors are
    laid out as for matchHammingWindowBatch; scale_q16 as matchHammingScaledWindowBatch (None = level_scales_q16).
    Returns (idx, dist, disp_q8, sad, nstereo): int32 tensors [batch][l_stride] (disp_q8 in level-0 pixels, Q8; -1
    and sad 0xffffffff for a rejected match) and nstereo [batch] (accepted matches); asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, ls, words = ldesc.shape
    rs = rdesc.shape[1]
    if rdesc.shape[2] != words:
        raise ValueError("left and right descriptors differ in words")
    if left_pyr.dim() != 3 or tuple(left_pyr.shape) != tuple(right_pyr.shape) or left_pyr.stride() != right_pyr.stride():
        raise ValueError("left_pyr and right_pyr must be [batch][rows][vstep] tensors of the same shape and stride")
    if left_pyr.dtype != torch.uint8 or right_pyr.dtype != torch.uint8 or left_pyr.stride(2) != 1:
        raise ValueError("pyramids must be uint8 with contiguous rows")
    rows, vstep = int(left_pyr.shape[1]), int(left_pyr.stride(1))
    if int(left_pyr.shape[2]) > vstep:
        raise ValueError("pyramid rows overlap")
    lv, n, s, r, p = _stereo_tables(levels, scale_q16, row_radius0, level_span, min_disp, max_disp, max_hamming,
                                    sad_radius, search_radius, median_filter)
    out = []
    for t in (idx, dist, disp_q8, sad):
        out.append(torch.empty((batch, ls), dtype=torch.int32, device=ldesc.device) if t is None else t)
    if nstereo is None:
        nstereo = torch.empty((batch,), dtype=torch.int32, device=ldesc.device)
    ctx.check(ctx.lib.pislam_match_stereo_batch(ctx.h, words, lv, n, s, r, ctypes.byref(p), ptr(left_pyr),
                                                ptr(right_pyr), vstep, rows, int(left_pyr.stride(0)), ptr(lkp),
                                                ptr(ldesc), ptr(lcounts), ls, ptr(rkp), ptr(rdesc), ptr(rcounts), rs,
                                                batch, *[ptr(t) for t in out], ptr(nstereo)),
              "pislam_match_stereo_batch")
    return (*out, nstereo)


# ---- pyramidal Lucas-Kanade tracking and sub-pixel match refinement ----------
def keypointsToQ8(kp):
    """Keypoint words (encodeFast: x << 12 | y in the low 24 bits; numpy array or torch tensor of any shape) as
    [..., 2] int32 (x, y) in Q8 stacked-pyramid coordinates, the pts_q8 of trackLKBatch."""
    if isinstance(kp, np.ndarray):
        k = kp.astype(np.int64)
        return np.stack([((k >> 12) & 0xFFF) << 8, (k & 0xFFF) << 8], axis=-1).astype(np.int32)
    import torch
    return torch.stack([((kp >> 12) & 0xFFF) << 8, (kp & 0xFFF) << 8], dim=-1).to(torch.int32)


def _lk_tables(levels, scale_q16):
    lv, n, s, _ = _scaled_tables(levels, scale_q16, 0)
    return lv, n, s


def trackLKBatch(prev_pyr, next_pyr, pts_q8, counts, levels, scale_q16, *, guess_q8=None, win_radius=7, max_iters=10,
                 eps_q8=8, max_step_q8=2048, level_step=3, max_coarse=2, min_eig=16, max_err=0, fb_max_q8=None,
                 next_q8=None, status=None, err=None, ntracked=None, ctx: Context | None = None):
    """Pyramidal Lucas-Kanade tracker (pislam_track_lk_batch; the contract is the comment in include/pislam_hip.h):
    point i of pair b, pts_q8[b][i] = (x, y) in Q8 stacked-pyramid coordinates of prev_pyr[b], is followed into
    next_pyr[b] (uint8 [batch][rows][vstep] device tensors of the same shape and stride) from guess_q8[b][i] (None:
    from the point itself), through up to max_coarse levels level_step apart above the point's own and then on its
    own level, with a (2 * win_radius + 1)^2 window.  scale_q16 as matchHammingScaledWindowBatch (None =
    level_scales_q16(levels)).  Returns (next_q8, status, err, ntracked): int32 tensors [batch][stride][2],
    [batch][stride] (code | iterations << 8; code 0 tracked, 1 no level or template at the border, 2 flat template,
    3 left the level, 4 over max_err), [batch][stride] (the sum of |residual| in Q5, 0xffffffff without one) and
    [batch].  Entries at and beyond counts[b] are not written.  Asynchronous on the ctx stream, no workspace.

    fb_max_q8 (None: off) adds a forward-backward check: a second call with the pyramids exchanged follows next_q8 back
    (no guess), and a fifth return value, a bool tensor [batch][stride], is true where both passes ended with code 0
    and the round trip lands within fb_max_q8 of the start on both axes (entries beyond the counts are undefined).

    The defaults min_eig = 16 and eps_q8 = 8 are guesses: nobody has measured them on real footage."""
    import torch
    ctx = ctx or default_context()
    if prev_pyr.dim() != 3 or tuple(prev_pyr.shape) != tuple(next_pyr.shape) or prev_pyr.stride() != next_pyr.stride():
        raise ValueError("prev_pyr and next_pyr must be [batch][rows][vstep] tensors of the same shape and stride")
    if prev_pyr.dtype != torch.uint8 or next_pyr.dtype != torch.uint8 or prev_pyr.stride(2) != 1:
        raise ValueError("pyramids must be uint8 with contiguous rows")
    batch, rows, vstep = int(prev_pyr.shape[0]), int(prev_pyr.shape[1]), int(prev_pyr.stride(1))
    if int(prev_pyr.shape[2]) > vstep:
        raise ValueError("pyramid rows overlap")
    if pts_q8.dtype != torch.int32 or pts_q8.dim() != 3 or int(pts_q8.shape[0]) != batch or int(pts_q8.shape[2]) != 2:
        raise ValueError("pts_q8 must be an int32 tensor [batch][stride][2]")
    stride = int(pts_q8.shape[1])
    if guess_q8 is not None and (guess_q8.dtype != torch.int32 or tuple(guess_q8.shape) != (batch, stride, 2)):
        raise ValueError("guess_q8 must be an int32 tensor [batch][stride][2]")
    lv, n, s = _lk_tables(levels, scale_q16)
    p = LkParams(int(win_radius), int(max_iters), int(eps_q8), int(max_step_q8), int(level_step), int(max_coarse),
                 int(min_eig), int(max_err))
    dev = pts_q8.device
    pstride = int(prev_pyr.stride(0)) if batch else 0

    def run(a, b, pts, guess, nq, st, er, nt):
        nq = torch.empty((batch, stride, 2), dtype=torch.int32, device=dev) if nq is None else nq
        st = torch.empty((batch, stride), dtype=torch.int32, device=dev) if st is None else st
        er = torch.empty((batch, stride), dtype=torch.int32, device=dev) if er is None else er
        nt = torch.empty((batch,), dtype=torch.int32, device=dev) if nt is None else nt
        ctx.check(ctx.lib.pislam_track_lk_batch(ctx.h, ctypes.byref(p), lv, n, s, ptr(a), ptr(b), vstep, rows, pstride,
                                                ptr(pts), ptr(counts), ptr(guess), stride, batch, ptr(nq), ptr(st),
                                                ptr(er), ptr(nt)), "pislam_track_lk_batch")
        return nq, st, er, nt

    out = run(prev_pyr, next_pyr, pts_q8, guess_q8, next_q8, status, err, ntracked)
    if fb_max_q8 is None:
        return out
    back, bst, _, _ = run(next_pyr, prev_pyr, out[0], None, None, None, None, None)
    near = ((back - pts_q8).abs() <= int(fb_max_q8)).all(dim=-1)
    return (*out, ((out[1] & 0xFF) == 0) & ((bst & 0xFF) == 0) & near)


def refineMatchesBatch(prev_pyr, next_pyr, qkp, qcounts, tkp, idx, levels, scale_q16=None, *, sel=None, win_radius=7,
                       max_iters=10, eps_q8=8, max_step_q8=2048, min_eig=16, max_err=0, ctx: Context | None = None):
    """Sub-pixel refinement of descriptor matches: query keypoint i of pair b (qkp [batch][q_stride], a keypoint of
    prev_pyr[b]) matched to train keypoint idx[b][i] (tkp [batch][t_stride], a keypoint of next_pyr[b]; idx as any
    matcher returns it, negative = unmatched) is tracked on its own level only (trackLKBatch with max_coarse = 0)
    from the train keypoint's position mapped to the query's level, u = floor((u_t * s_t + floor(s_q / 2)) / s_q) per
    axis (the header's level mapping, here in torch int64).  sel = (sel_q, sel_t, nsel) of selectMatchesBatch keeps
    only the selected matches.  Unmatched queries, and matches one of whose keypoints lies in no level, are given a
    point in no level: their status is 1.  Returns (next_q8, status, err, ntracked) as trackLKBatch, next_q8 in the
    stacked Q8 coordinates of the query's level.  The torch ops run on the current torch stream."""
    import torch
    batch, qs = (int(v) for v in qkp.shape)
    dev = qkp.device
    idx = idx.to(torch.int64)
    if sel is not None:
        sel_q, sel_t, nsel = sel
        live = torch.arange(qs, device=dev)[None, :] < nsel.to(torch.int64)[:, None]
        col = torch.where(live, sel_q.to(torch.int64), torch.full_like(idx, qs))       # dead slots go to a spare column
        keep = torch.full((batch, qs + 1), -1, dtype=torch.int64, device=dev)
        keep.scatter_(1, col, torch.where(live, sel_t.to(torch.int64), torch.full_like(idx, -1)))
        idx = torch.where(keep[:, :qs] == idx, idx, torch.full_like(idx, -1))
    matched = idx >= 0
    tk = torch.gather(tkp.to(torch.int64), 1, idx.clamp(min=0, max=int(tkp.shape[1]) - 1))
    qk = qkp.to(torch.int64)
    lvn = [(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 0) for t in levels]
    sc = level_scales_q16(levels) if scale_q16 is None else ([int(scale_q16)] * len(lvn) if isinstance(
        scale_q16, (int, np.integer)) else [int(v) for v in scale_q16])

    def local(k):
        """Level-local Q8 (u, v), scale and origin of keypoint words; scale 0 in no level."""
        x, y = (k >> 12) & 0xFFF, k & 0xFFF
        u, v, s, c0, r0 = (torch.zeros_like(k) for _ in range(5))
        for (w, h, row0, col0), sl in zip(lvn, sc):
            m = (x >= col0) & (x < col0 + w) & (y >= row0) & (y < row0 + h)
            u, v = torch.where(m, (x - col0) << 8, u), torch.where(m, (y - row0) << 8, v)
            s = torch.where(m, torch.full_like(k, sl), s)
            c0, r0 = torch.where(m, torch.full_like(k, col0), c0), torch.where(m, torch.full_like(k, row0), r0)
        return u, v, s, c0, r0

    _, _, sq, qc0, qr0 = local(qk)
    ut, vt, st, _, _ = local(tk)
    ok = matched & (sq > 0) & (st > 0)
    sq1 = sq.clamp(min=1)
    gx = torch.div(ut * st + sq1 // 2, sq1, rounding_mode="floor") + (qc0 << 8)
    gy = torch.div(vt * st + sq1 // 2, sq1, rounding_mode="floor") + (qr0 << 8)
    pts = keypointsToQ8(qk)
    pts = torch.where(ok[..., None], pts, torch.full_like(pts, -256))
    guess = torch.where(ok[..., None], torch.stack([gx, gy], dim=-1).to(torch.int32), pts).contiguous()
    return trackLKBatch(prev_pyr, next_pyr, pts.contiguous(), qcounts, levels, sc, guess_q8=guess, win_radius=win_radius,
                        max_iters=max_iters, eps_q8=eps_q8, max_step_q8=max_step_q8, level_step=1, max_coarse=0,
                        min_eig=min_eig, max_err=max_err, ctx=ctx)


# ---- bag of words: vocabulary tree, quantisation, vector, word-guided matching ----------
class Vocabulary:
    """pislam_vocab: a rooted tree of cluster centres from host arrays — node_desc uint32 [nnodes][words] (node 0 is
    the root, its descriptor is ignored), first_child and child_count int [nnodes] (children are contiguous;
    child_count 0 = leaf).  Words are the leaves in ascending node index; groups are the nodes at depth `group_depth`
    plus the leaves shallower than that (include/pislam_hip.h).  Shapes are checked here, the tree by the library."""

    def __init__(self, node_desc, first_child, child_count, group_depth: int, *, ctx: Context | None = None):
        node_desc = np.ascontiguousarray(node_desc, np.uint32)
        if node_desc.ndim != 2:
            raise ValueError("node_desc must be [nnodes][words]")
        nnodes, words = node_desc.shape
        if words not in (1, 2, 4, 8):
            raise ValueError("words must be 1, 2, 4 or 8")
        first_child = np.ascontiguousarray(first_child, np.int32)
        child_count = np.ascontiguousarray(child_count, np.int32)
        if first_child.shape != (nnodes,) or child_count.shape != (nnodes,):
            raise ValueError(f"first_child and child_count must have one entry per node ({nnodes})")
        self.h = None
        self.ctx = ctx or default_context()
        self.words, self.nnodes, self.group_depth = int(words), int(nnodes), int(group_depth)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.pislam_vocab_create(self.ctx.h, self.words, self.nnodes, ptr(node_desc),
                                                        ptr(first_child), ptr(child_count), self.group_depth,
                                                        ctypes.byref(h)), "pislam_vocab_create")
        self.h = h
        self.nwords = int(self.ctx.lib.pislam_vocab_nwords(h))
        self.ngroups = int(self.ctx.lib.pislam_vocab_ngroups(h))

    @staticmethod
    def kary_tables(k: int, depth: int):
        """(first_child, child_count) of the complete k-ary tree with leaves at `depth` in breadth-first order."""
        if not 1 <= k <= 32 or not 1 <= depth <= 16:
            raise ValueError("need 1 <= k <= 32 and 1 <= depth <= 16")
        level = [k ** d for d in range(depth + 1)]
        nnodes, inner = sum(level), sum(level[:-1])
        if nnodes > 1 << 24:
            raise ValueError("more than 2^24 nodes")
        n = np.arange(nnodes, dtype=np.int64)
        first = np.where(n < inner, n * k + 1, 0).astype(np.int32)
        count = np.where(n < inner, k, 0).astype(np.int32)
        return first, count

    @classmethod
    def from_kary(cls, node_desc, k: int, depth: int, group_depth: int = 2, *, ctx: Context | None = None):
        """A complete k-ary tree of `depth` levels below the root, nodes in breadth-first order (node n's children are
        n * k + 1 .. n * k + k): node_desc [(k^(depth+1) - 1) / (k - 1)][words]."""
        first, count = cls.kary_tables(k, depth)
        node_desc = np.asarray(node_desc)
        if node_desc.ndim != 2 or node_desc.shape[0] != len(first):
            raise ValueError(f"a {k}-ary tree of depth {depth} has {len(first)} nodes")
        return cls(node_desc, first, count, group_depth, ctx=ctx)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pislam_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bowTransformBatch(vocab: Vocabulary, desc, counts, word=None, group=None, wdist=None, *, want_group=True,
                      want_wdist=True, ctx: Context | None = None):
    """Drops every descriptor of device-resident front-end outputs (desc [batch][max_kp][words], counts [batch]) down
    the vocabulary tree (pislam_bow_transform_batch).  Returns (word, group, wdist) int32 tensors [batch][max_kp]: the
    leaf's word id, its group id and the Hamming distance to the leaf; group / wdist are None when not wanted
    (want_group / want_wdist False and no tensor given).  Asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, stride, words = desc.shape
    if words != vocab.words:
        raise ValueError(f"descriptors have {words} words, the vocabulary {vocab.words}")
    new = lambda: torch.empty((batch, stride), dtype=torch.int32, device=desc.device)
    if word is None:
        word = new()
    if group is None and want_group:
        group = new()
    if wdist is None and want_wdist:
        wdist = new()
    ctx.check(ctx.lib.pislam_bow_transform_batch(ctx.h, vocab.h, ptr(desc), ptr(counts), stride, batch, ptr(word),
                                                 ptr(group), ptr(wdist)), "pislam_bow_transform_batch")
    return word, group, wdist


def bowVectorBatch(word, counts, bow_word=None, bow_tf=None, bow_n=None, *, ctx: Context | None = None):
    """Bag-of-words vectors of word [batch][stride] (pislam_bow_vector_batch, stride <= 16384): returns (bow_word,
    bow_tf int32 [batch][stride], bow_n int32 [batch]) — pyramid b's distinct words in ascending order, how often each
    occurs, and their number; slots at and beyond bow_n[b] are not written.  Asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, stride = word.shape
    if bow_word is None:
        bow_word = torch.empty((batch, stride), dtype=torch.int32, device=word.device)
    if bow_tf is None:
        bow_tf = torch.empty((batch, stride), dtype=torch.int32, device=word.device)
    if bow_n is None:
        bow_n = torch.empty((batch,), dtype=torch.int32, device=word.device)
    ctx.check(ctx.lib.pislam_bow_vector_batch(ctx.h, ptr(word), ptr(counts), stride, batch, ptr(bow_word), ptr(bow_tf),
                                              ptr(bow_n)), "pislam_bow_vector_batch")
    return bow_word, bow_tf, bow_n


def reserveMatchBow(ngroups: int, t_stride: int, batch: int, *, words=8, ctx: Context | None = None):
    """Sizes the context's word-guided matcher workspace (pislam_match_bow_reserve): afterwards matchHammingBowBatch of
    the same or a smaller shape allocates nothing and can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_match_bow_reserve(ctx.h, words, int(ngroups), t_stride, batch), "pislam_match_bow_reserve")


def matchHammingBowBatch(qdesc, qgroup, qcounts, tdesc, tgroup, tcounts, ngroups: int, idx=None, dist=None, dist2=None,
                         *, ctx: Context | None = None):
    """Word-guided matcher (pislam_match_hamming_bow_batch) on device-resident front-end outputs and the group ids
    bowTransformBatch wrote for them ([batch][max_kp]): query i of pair b sees the train descriptors of the same
    group; ids at or above ngroups match nothing.  Returns (idx, dist, dist2) int32 tensors [batch][q_stride] like
    matchHammingBatch; asynchronous on the ctx stream."""
    ctx = ctx or default_context()
    batch, qs, words = qdesc.shape
    ts = tdesc.shape[1]
    if tdesc.shape[2] != words:
        raise ValueError("query and train descriptors differ in words")
    if tuple(qgroup.shape) != (batch, qs) or tuple(tgroup.shape) != (tdesc.shape[0], ts):
        raise ValueError("qgroup / tgroup must be [batch][stride] like the descriptors")
    idx, dist, dist2 = _match_outputs(qdesc, idx, dist, dist2)
    ctx.check(ctx.lib.pislam_match_hamming_bow_batch(ctx.h, words, int(ngroups), ptr(qdesc), ptr(qgroup), ptr(qcounts),
                                                     qs, ptr(tdesc), ptr(tgroup), ptr(tcounts), ts, batch, ptr(idx),
                                                     ptr(dist), ptr(dist2)), "pislam_match_hamming_bow_batch")
    return idx, dist, dist2


# ---- what the batched wrappers below share: tensor checks and host tables, each rule stated once ----------
@functools.cache
def _word32():
    """The dtypes that count as a 32-bit word: int32, and uint32 where this torch has it."""
    import torch
    return (torch.int32, getattr(torch, "uint32", torch.int32))


@functools.cache
def _word16():
    """The dtypes that count as a 16-bit word: int16, and uint16 where this torch has it."""
    import torch
    return (torch.int16, getattr(torch, "uint16", torch.int16))


def _tensor(t, dtype, shape, message):
    """Refuses, with the caller's message, a tensor that has not the dtype (one, or a tuple such as _word32(); None: any) or
    not the shape.  An extent given as None is free: the free extents are returned, in order."""
    if t.dtype != dtype and dtype is not None and not (type(dtype) is tuple and t.dtype in dtype):
        raise ValueError(message)
    have, free = t.shape, ()
    if have != shape:
        if len(have) != len(shape):
            raise ValueError(message)
        for h, w in zip(have, shape):
            if w is None:
                free += (h,)
            elif h != w:
                raise ValueError(message)
    return free


def _counts(message, batch, *counts):
    """Counts tensors: 32-bit words, one per batch entry."""
    words, shape = _word32(), (batch,)
    for t in counts:
        if t.dtype not in words or t.shape != shape:
            raise ValueError(message)


def _float_table(values, message, entries=None):
    """A HOST sequence of float32 as the C array the library reads: (array, length).  The library takes 1..16 entries;
    `entries` given: exactly that many (the second of two tables that go together)."""
    host = np.asarray(values, dtype=np.float32).ravel()        # (contiguous: ravel copies where it has to)
    n = host.size
    if not 1 <= n <= 16 or (entries is not None and n != entries):
        raise ValueError(message)
    return (ctypes.c_float * n).from_buffer_copy(host), n


def _level_table(levels, inv_sigma2, batch, stride, together, shaped):
    """The level arguments of the pose, Sim(3) and bundle-adjustment calls: the tensors `levels` (level, or level1 and
    level2) and the host table inv_sigma2 are given together or not at all (else ValueError(together)); each level tensor
    is uint8 [batch][stride] (else ValueError(shaped)).  Returns _float_table's (tab, ntab), (None, 0) without levels."""
    for level in levels:
        if (level is None) != (inv_sigma2 is None):
            raise ValueError(together)
    if inv_sigma2 is None:
        return None, 0
    import torch
    for level in levels:
        _tensor(level, torch.uint8, (batch, stride), shaped)
    return _float_table(inv_sigma2, "inv_sigma2 must have 1..16 entries")


def _contiguous(*tensors, message="inputs must be contiguous"):
    """Every input given (None: an optional one that is absent) is contiguous."""
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise ValueError(message)


def _on_device(a):
    """A numpy input as a tensor on the current device; anything else as it is."""
    if isinstance(a, np.ndarray):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return a


# ---- after the match: angle bins and match selection ---------------------
def orbAnglesBatch(pyramids, kp, counts, angles=None, *, ctx: Context | None = None):
    """Rotation bins of device-resident front-end keypoints (pislam_orb_angles_batch): pyramids uint8
    [batch][rows][vstep], kp [batch][stride], counts [batch].  Returns angles uint8 [batch][stride]: the bin 0..29
    orbCompute uses for each keypoint, 0xff where the patch would leave the buffer; entries at and beyond a pyramid's
    count are not written.  Asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, rows, vstep = (int(v) for v in pyramids.shape)
    stride = int(kp.shape[1])
    if int(kp.shape[0]) != batch:
        raise ValueError("pyramids and keypoints differ in batch")
    if angles is None:
        angles = torch.empty((batch, stride), dtype=torch.uint8, device=kp.device)
    ctx.check(ctx.lib.pislam_orb_angles_batch(ctx.h, ptr(pyramids), vstep, rows, int(pyramids.stride(0)) if batch else 0,
                                              ptr(kp), ptr(counts), stride, batch, ptr(angles)),
              "pislam_orb_angles_batch")
    return angles


def selectMatchesBatch(idx, dist, dist2, qcounts, tcounts, *, max_dist=50, ratio=(8, 10), unique=True, rot_keep=3,
                       rot_min_pct=10, back_idx=None, qangle=None, tangle=None, want_status=False, want_hist=False,
                       t_stride: int | None = None, sel_q=None, sel_t=None, nsel=None, status=None, rot_hist=None,
                       ctx: Context | None = None):
    """Match selection on the device (pislam_match_select_batch) over the (idx, dist, dist2) [batch][q_stride] of any
    matcher: distance threshold, ratio test (ratio = (num, den), None = off; dist2 may be None then), cross-check against
    back_idx [batch][t_stride], one-to-one claim, and ORB-SLAM's rotation histogram over qangle / tangle (orbAnglesBatch;
    rot_keep is forced to 0 when no angles are given).  Returns (sel_q, sel_t, nsel[, status][, rot_hist]): pair b's
    selected queries in ascending order and their train indices in the first nsel[b] slots of int32 [batch][q_stride]
    (the other slots are not written), status uint8 [batch][q_stride] (0 or the number of the failed test), rot_hist
    int32 [batch][30].  t_stride is taken from tangle or back_idx; without either it may be given (default 65535: the
    train counts are then not clamped).  Asynchronous on the ctx stream; no workspace."""
    import torch
    ctx = ctx or default_context()
    batch, qs = (int(v) for v in idx.shape)
    if qangle is None or tangle is None:
        if qangle is not None or tangle is not None:
            raise ValueError("qangle and tangle go together")
        rot_keep = 0
    for a in (tangle, back_idx):
        if a is not None:
            if t_stride is not None and int(a.shape[1]) != t_stride:
                raise ValueError("t_stride, tangle and back_idx disagree")
            t_stride = int(a.shape[1])
    if t_stride is None:
        t_stride = 65535
    num, den = (0, 0) if ratio is None else (int(ratio[0]), int(ratio[1]))
    p = SelectParams(int(max_dist), num, den, 1 if unique else 0, int(rot_keep), int(rot_min_pct))
    dev = idx.device
    if sel_q is None:
        sel_q = torch.empty((batch, qs), dtype=torch.int32, device=dev)
    if sel_t is None:
        sel_t = torch.empty((batch, qs), dtype=torch.int32, device=dev)
    if nsel is None:
        nsel = torch.empty((batch,), dtype=torch.int32, device=dev)
    if status is None and want_status:
        status = torch.empty((batch, qs), dtype=torch.uint8, device=dev)
    if rot_hist is None and want_hist:
        rot_hist = torch.empty((batch, 30), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.pislam_match_select_batch(ctx.h, ctypes.byref(p), ptr(idx), ptr(dist), ptr(dist2), ptr(qcounts), qs,
                                                ptr(tcounts), t_stride, ptr(back_idx), ptr(qangle), ptr(tangle), batch,
                                                ptr(sel_q), ptr(sel_t), ptr(nsel), ptr(status), ptr(rot_hist)),
              "pislam_match_select_batch")
    out = (sel_q, sel_t, nsel)
    if status is not None:
        out += (status,)
    if rot_hist is not None:
        out += (rot_hist,)
    return out


# ---- two-view geometry: batched RANSAC for F and H ----------
TWO_VIEW_MAX_STRIDE = 16384   # matches per pair (pislam_two_view_ransac_batch)
_TWO_VIEW_MODELS = {0: 0, 1: 1, "F": 0, "H": 1, "fundamental": 0, "homography": 1}


def matchedPointsQ8(qkp, tkp, sel, levels, scale_q16=None, refined=None):
    """The matched point lists of twoViewRansacBatch from selectMatchesBatch's compacted lists: sel = (sel_q, sel_t,
    nsel); slot s < nsel[b] pairs query keypoint qkp[b][sel_q[b][s]] (image 1) with train keypoint tkp[b][sel_t[b][s]]
    (image 2).  Each keypoint is mapped from its level to level 0 by the header's formula, per axis with the
    level-local Q8 coordinate u: floor((u * s_l + 32768) / 65536) in int64 (scale_q16 None = level_scales_q16(levels)).
    refined = the next_q8 of refineMatchesBatch ([batch][q_stride][2], indexed by query, in the stacked Q8 coordinates
    of the QUERY's level) replaces the train keypoint's position.  A match one of whose keypoints lies in no level is
    dropped from the list.  Returns (p1_q8, p2_q8, counts): int32 [batch][q_stride][2] twice (slots at and beyond
    counts[b] are zero) and int32 [batch].  Torch ops on the current torch stream."""
    import torch
    sel_q, sel_t, nsel = sel
    batch, qs = (int(v) for v in sel_q.shape)
    dev = sel_q.device
    lvn = [(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 0) for t in levels]
    sc = level_scales_q16(levels) if scale_q16 is None else ([int(scale_q16)] * len(lvn) if isinstance(
        scale_q16, (int, np.integer)) else [int(v) for v in scale_q16])
    live = torch.arange(qs, device=dev)[None, :] < nsel.to(torch.int64)[:, None]
    qi = torch.where(live, sel_q.to(torch.int64), torch.zeros_like(live, dtype=torch.int64)).clamp(0, int(qkp.shape[1]) - 1)
    ti = torch.where(live, sel_t.to(torch.int64), torch.zeros_like(live, dtype=torch.int64)).clamp(0, int(tkp.shape[1]) - 1)
    qk = torch.gather(qkp.to(torch.int64), 1, qi)
    tk = torch.gather(tkp.to(torch.int64), 1, ti)

    def level0(k, pos=None):
        """Level-0 Q8 (x, y) of the stacked Q8 position `pos` (None: the keypoint itself) on the level that holds the
        keypoint word k, and whether any level holds it."""
        x, y = (k >> 12) & 0xFFF, k & 0xFFF
        px, py = (x << 8, y << 8) if pos is None else (pos[..., 0], pos[..., 1])
        X, Y, found = torch.zeros_like(k), torch.zeros_like(k), torch.zeros_like(k, dtype=torch.bool)
        for (w, h, row0, col0), sl in zip(lvn, sc):
            m = (x >= col0) & (x < col0 + w) & (y >= row0) & (y < row0 + h)
            X = torch.where(m, torch.div((px - (col0 << 8)) * sl + 32768, 65536, rounding_mode="floor"), X)
            Y = torch.where(m, torch.div((py - (row0 << 8)) * sl + 32768, 65536, rounding_mode="floor"), Y)
            found |= m
        return X, Y, found

    x1, y1, ok1 = level0(qk)
    if refined is None:
        x2, y2, ok2 = level0(tk)
    else:
        pos = torch.gather(refined.to(torch.int64), 1, qi[..., None].expand(-1, -1, 2))
        x2, y2, _ = level0(qk, pos)
        ok2 = level0(tk)[2]
    keep = live & ok1 & ok2
    slot = torch.where(keep, torch.cumsum(keep.to(torch.int64), 1) - 1, torch.full_like(qi, qs))   # dropped: a spare column
    out = torch.zeros((2, batch, qs + 1, 2), dtype=torch.int64, device=dev)
    out[0].scatter_(1, slot[..., None].expand(-1, -1, 2), torch.stack([x1, y1], dim=-1))
    out[1].scatter_(1, slot[..., None].expand(-1, -1, 2), torch.stack([x2, y2], dim=-1))
    out = out[:, :, :qs].to(torch.int32)
    return out[0].contiguous(), out[1].contiguous(), keep.sum(dim=1).to(torch.int32)


def twoViewRansacBatch(p1_q8, p2_q8, counts, *, model, hypotheses=200, seed=0, sigma_q8=256, best=None, score=None,
                       ninliers=None, inlier=None, model_n=None, stats=None, ctx: Context | None = None):
    """Batched two-view RANSAC (pislam_two_view_ransac_batch; the contract is the comment in include/pislam_hip.h):
    match i of pair b is p1_q8[b][i] (image 1) and p2_q8[b][i] (image 2), (x, y) in level-0 pixels in Q8, int32 device
    tensors [batch][stride][2] with stride <= 16384; counts [batch].  model is 0 / "F" (fundamental matrix, 8 matches
    per hypothesis) or 1 / "H" (homography, 4).  All `hypotheses` (1..1024) are evaluated, scored as ORB-SLAM's
    Initializer does with a measurement sigma of sigma_q8 / 256 pixels.  Returns (best, score, ninliers, inlier,
    model_n, stats): int32 [batch] (the winning hypothesis, -1 = no model), int32 [batch] twice, uint8 [batch][stride]
    (entries at and beyond counts[b] are not written), float32 [batch][9] (the model in normalised coordinates:
    twoViewDenormalise gives pixels; F is not forced to rank 2) and int64 [batch][8].  The same inputs and seed give the
    same outputs, bit for bit.  Asynchronous on the ctx stream, no workspace: capturable as it is."""
    import torch
    ctx = ctx or default_context()
    if model not in _TWO_VIEW_MODELS:
        raise ValueError('model must be 0 / "F" or 1 / "H"')
    batch, stride = _tensor(p1_q8, torch.int32, (None, None, 2), "p1_q8 must be an int32 tensor [batch][stride][2]")
    _tensor(p2_q8, torch.int32, (batch, stride, 2), "p2_q8 must be an int32 tensor of p1_q8's shape")
    if stride > TWO_VIEW_MAX_STRIDE:
        raise ValueError(f"at most {TWO_VIEW_MAX_STRIDE} matches per pair")
    dev = p1_q8.device
    p = TwoViewParams(_TWO_VIEW_MODELS[model], int(hypotheses), int(seed) & 0xFFFFFFFF, int(sigma_q8))
    best = torch.empty((batch,), dtype=torch.int32, device=dev) if best is None else best
    score = torch.empty((batch,), dtype=torch.int32, device=dev) if score is None else score
    ninliers = torch.empty((batch,), dtype=torch.int32, device=dev) if ninliers is None else ninliers
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    model_n = torch.empty((batch, 9), dtype=torch.float32, device=dev) if model_n is None else model_n
    stats = torch.empty((batch, 8), dtype=torch.int64, device=dev) if stats is None else stats
    ctx.check(ctx.lib.pislam_two_view_ransac_batch(ctx.h, ctypes.byref(p), ptr(p1_q8), ptr(p2_q8), ptr(counts), stride,
                                                   batch, ptr(best), ptr(score), ptr(ninliers), ptr(inlier),
                                                   ptr(model_n), ptr(stats)), "pislam_two_view_ransac_batch")
    return best, score, ninliers, inlier, model_n, stats


def twoViewDenormalise(model, model_n, stats) -> np.ndarray:
    """pislam_two_view_denormalise on the host: the level-0-pixel matrices, float64 [batch][3][3] (or [3][3] for one
    row), from twoViewRansacBatch's model_n and stats (tensors or arrays; device tensors are copied to the host, which
    synchronises).  F = T2' Fn T1, H = inverse(T2) Hn T1.  A row without a model (n < 1 or D < 1) is NaN."""
    if model not in _TWO_VIEW_MODELS:
        raise ValueError('model must be 0 / "F" or 1 / "H"')
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    m = np.ascontiguousarray(host(model_n), dtype=np.float32)
    st = np.ascontiguousarray(host(stats), dtype=np.int64)
    single = m.ndim == 1
    m, st = m.reshape(-1, 9), st.reshape(-1, 8)
    if len(m) != len(st):
        raise ValueError("model_n and stats must have the same number of rows")
    out = np.full((len(m), 9), np.nan)
    lib = capi.load()
    for b in range(len(m)):
        row = (ctypes.c_double * 9)()
        rc = lib.pislam_two_view_denormalise(_TWO_VIEW_MODELS[model], m[b].ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                             st[b].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), row)
        if rc == capi.PISLAM_OK:
            out[b] = row[:]
    out = out.reshape(-1, 3, 3)
    return out[0] if single else out


def twoViewModelRatio(score_h, score_f):
    """ORB-SLAM's model choice RH = SH / (SH + SF) from the scores of the two calls (numbers, arrays or tensors;
    float64 on the host; 0 where both scores are 0).  ORB-SLAM takes the homography when RH > 0.40."""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    sh = host(score_h).astype(np.int64).astype(np.float64) if not isinstance(score_h, (int, float)) else np.float64(score_h)
    sf = host(score_f).astype(np.int64).astype(np.float64) if not isinstance(score_f, (int, float)) else np.float64(score_f)
    tot = sh + sf
    return np.where(tot > 0, sh / np.where(tot > 0, tot, 1.0), 0.0)[()]


def _camera4(K) -> np.ndarray:
    """fx, fy, cx, cy (float64) from a 3 x 3 camera matrix or from the four numbers themselves."""
    host = K.detach().cpu().numpy() if hasattr(K, "detach") else np.asarray(K)
    k = np.asarray(host, dtype=np.float64)
    if k.shape == (3, 3):
        return np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape == (4,):
        return k.copy()
    raise ValueError("K must be a 3 x 3 camera matrix or (fx, fy, cx, cy)")


def twoViewCandidates(model, m_px, K) -> np.ndarray:
    """pislam_two_view_decompose on the host: the candidate motions of the level-0-pixel matrix m_px (float64 [3][3] or
    a batch [batch][3][3]: twoViewDenormalise's output) under the camera K (3 x 3, or fx, fy, cx, cy), as float32
    [k][12] (or [batch][k][12]) rows r0 .. r8, t0 .. t2 with X2 = R X1 + t and |t| = 1: k = 4 for model 0 / "F" (the
    four motions of the essential matrix K' F K), k = 8 for model 1 / "H" (Faugeras-Lustman), in ORB-SLAM's order:
    twoViewReconstructBatch's cand.  A matrix whose decomposition is degenerate (or that is not finite) gives rows of
    NaN, which the reconstruction counts as candidates without a good match."""
    if model not in _TWO_VIEW_MODELS:
        raise ValueError('model must be 0 / "F" or 1 / "H"')
    host = m_px.detach().cpu().numpy() if hasattr(m_px, "detach") else np.asarray(m_px)
    m = np.ascontiguousarray(host, dtype=np.float64)
    if m.ndim not in (2, 3) or m.shape[-2:] != (3, 3):
        raise ValueError("m_px must be [3][3] or [batch][3][3]")
    single = m.ndim == 2
    m = m.reshape(-1, 9)
    cam = np.ascontiguousarray(_camera4(K))
    k = 4 if _TWO_VIEW_MODELS[model] == 0 else 8
    out = np.full((len(m), k, 12), np.nan, dtype=np.float32)
    lib = capi.load()
    dp = ctypes.POINTER(ctypes.c_double)
    for b in range(len(m)):
        row, got = (ctypes.c_float * 96)(), ctypes.c_int(0)
        rc = lib.pislam_two_view_decompose(_TWO_VIEW_MODELS[model], m[b].ctypes.data_as(dp), cam.ctypes.data_as(dp), row,
                                           ctypes.byref(got))
        if rc == capi.PISLAM_OK and got.value == k:
            out[b] = np.frombuffer(row, dtype=np.float32)[:12 * k].reshape(k, 12)
    return out[0] if single else out


RECONSTRUCT_MAX_STRIDE = 16384   # matches per pair (pislam_two_view_reconstruct_batch)


def twoViewReconstructBatch(p1_q8, p2_q8, counts, cam, cand, *, mask=None, sigma_q8=256, min_parallax_deg=1.0,
                            cos_point=0.99998, min_good=50, min_good_pct=90, similar_pct=70, parallax_rank=51,
                            best=None, status=None, ngood=None, npar=None, pose_out=None, xw=None, point=None,
                            ctx: Context | None = None):
    """Batched two-view reconstruction (pislam_two_view_reconstruct_batch; the contract is the comment in
    include/pislam_hip.h): per pair, every used match of p1_q8 / p2_q8 (int32 [batch][stride][2], level-0 Q8 pixels,
    stride <= 16384; counts [batch]; mask uint8 [batch][stride] or None: twoViewRansacBatch's inlier fits) is
    triangulated under every candidate motion cand (float32 [batch][ncand][12], ncand 1..8: twoViewCandidates, or one
    known relative pose) with the camera cam (float32 [batch][4]: fx, fy, cx, cy); the motion with the most good points
    wins unless too few are good (min_good, min_good_pct of the used matches), another motion has similar_pct per cent
    as many, or fewer than min(parallax_rank, the winner's count) of them have min_parallax_deg of parallax
    (cos_parallax = float32(cos(radians(min_parallax_deg)))).  Returns (best int32 [batch] (-1: refused), status int32
    [batch] = code | cbest << 8 with code 0 ok, 1 too few, 2 ambiguous, 3 low parallax, 4 no input, ngood and npar
    int32 [batch][8], pose_out float32 [batch][12] (the winner, ready for poseRefineBatch; zeros when refused), xw
    float32 [batch][stride][3] and point uint8 [batch][stride]: the winner's map points in frame 1 (entries at and
    beyond counts[b] are not written)).  The same inputs give the same outputs, bit for bit.  Asynchronous on the ctx
    stream, no workspace: capturable as it is."""
    import torch
    batch, stride = _tensor(p1_q8, torch.int32, (None, None, 2), "p1_q8 must be an int32 tensor [batch][stride][2]")
    _tensor(p2_q8, torch.int32, (batch, stride, 2), "p2_q8 must be an int32 tensor of p1_q8's shape")
    if stride > RECONSTRUCT_MAX_STRIDE:
        raise ValueError(f"at most {RECONSTRUCT_MAX_STRIDE} matches per pair")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    _tensor(cam, torch.float32, (batch, 4), "cam must be a float32 tensor [batch][4]")
    ncand, = _tensor(cand, torch.float32, (batch, None, 12), "cand must be a float32 tensor [batch][ncand][12]")
    if not 1 <= ncand <= 8:
        raise ValueError("cand must hold 1..8 candidates per pair")
    if mask is not None:
        _tensor(mask, torch.uint8, (batch, stride), "mask must be a uint8 tensor [batch][stride]")
    _contiguous(p1_q8, p2_q8, counts, cam, cand, mask)
    cos_parallax = np.float32(np.cos(np.radians(min_parallax_deg)))
    cos_point = np.float32(cos_point)
    if not 1 <= int(sigma_q8) <= 4096:
        raise ValueError("sigma_q8 must be 1..4096")
    if not 0 < cos_parallax <= 1:
        raise ValueError("min_parallax_deg must give a cosine in (0, 1]")
    if not 0 < cos_point <= 1:
        raise ValueError("cos_point must be in (0, 1]")
    if not 1 <= int(min_good) <= RECONSTRUCT_MAX_STRIDE:
        raise ValueError("min_good must be 1..16384")
    if not 0 <= int(min_good_pct) <= 100:
        raise ValueError("min_good_pct must be 0..100")
    if not 1 <= int(similar_pct) <= 100:
        raise ValueError("similar_pct must be 1..100")
    if not 1 <= int(parallax_rank) <= RECONSTRUCT_MAX_STRIDE:
        raise ValueError("parallax_rank must be 1..16384")
    ctx = ctx or default_context()
    dev = p1_q8.device
    p = capi.ReconstructParams(ncand, int(sigma_q8), float(cos_parallax), float(cos_point), int(min_good),
                               int(min_good_pct), int(similar_pct), int(parallax_rank))
    best = torch.empty((batch,), dtype=torch.int32, device=dev) if best is None else best
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    ngood = torch.empty((batch, 8), dtype=torch.int32, device=dev) if ngood is None else ngood
    npar = torch.empty((batch, 8), dtype=torch.int32, device=dev) if npar is None else npar
    pose_out = torch.empty((batch, 12), dtype=torch.float32, device=dev) if pose_out is None else pose_out
    xw = torch.empty((batch, stride, 3), dtype=torch.float32, device=dev) if xw is None else xw
    point = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if point is None else point
    ctx.check(ctx.lib.pislam_two_view_reconstruct_batch(ctx.h, ctypes.byref(p), ptr(p1_q8), ptr(p2_q8), ptr(counts),
                                                        ptr(mask), ptr(cam), ptr(cand), stride, batch, ptr(best),
                                                        ptr(status), ptr(ngood), ptr(npar), ptr(pose_out), ptr(xw),
                                                        ptr(point)), "pislam_two_view_reconstruct_batch")
    return best, status, ngood, npar, pose_out, xw, point


# ---- motion-only pose optimisation from 3D-2D matches ----------
POSE_MAX_STRIDE = 16384       # observations per frame (pislam_pose_refine_batch)
POSE_MONO = -(1 << 31)        # u_right of a monocular observation
POSE_NO_LEVEL = 255           # level of a keypoint that lies in no level: dead


def poseLevelWeights(nlevels: int, scale: float = 1.2) -> np.ndarray:
    """The inv_sigma2 table of poseRefineBatch for a pyramid of `nlevels` levels (1..16) with the scale factor
    `scale`: float32 1 / scale^(2 l), computed one float32 operation at a time: s = float32(scale), f_0 = 1,
    f_l = f_(l-1) * s, w_l = 1 / (f_l * f_l)  (ORB-SLAM's mvInvLevelSigma2)."""
    if not 1 <= int(nlevels) <= 16:
        raise ValueError("nlevels must be 1..16")
    s, f = np.float32(scale), np.float32(1.0)
    out = np.empty(int(nlevels), dtype=np.float32)
    for l in range(int(nlevels)):
        out[l] = np.float32(1.0) / (f * f)
        f = f * s
    return out


def poseObservationsQ8(kp, levels, scale_q16=None, disp_q8=None, pos_q8=None):
    """The obs_q8 and level of poseRefineBatch from keypoint words kp [batch][stride] (any integer tensor, device or
    host): each keypoint is mapped from its level to level 0 by matchedPointsQ8's formula, per axis with the
    level-local Q8 coordinate u: floor((u * s_l + 32768) / 65536) in int64 (scale_q16 None = level_scales_q16(levels)).
    pos_q8 ([batch][stride][2], e.g. refineMatchesBatch's next_q8: stacked Q8 coordinates on the keypoint's level)
    replaces the keypoint's position.  disp_q8 ([batch][stride], matchStereoBatch's, level-0 Q8): u_right = u - disp_q8
    where disp_q8 >= 0, else the monocular sentinel INT32_MIN; None: every observation is monocular.  A keypoint in no
    level gets the level 255 (dead in poseRefineBatch with a level table of at most 16 entries) and (0, 0, INT32_MIN).
    Returns (obs_q8 int32 [batch][stride][3], level uint8 [batch][stride]).  Torch ops on the current torch stream."""
    import torch
    lvn = [(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 0) for t in levels]
    sc = level_scales_q16(levels) if scale_q16 is None else ([int(scale_q16)] * len(lvn) if isinstance(
        scale_q16, (int, np.integer)) else [int(v) for v in scale_q16])
    if len(lvn) > POSE_NO_LEVEL:
        raise ValueError("at most 255 levels")
    k = kp.to(torch.int64)
    x, y = (k >> 12) & 0xFFF, k & 0xFFF
    if pos_q8 is None:
        px, py = x << 8, y << 8
    else:
        if tuple(pos_q8.shape) != tuple(kp.shape) + (2,):
            raise ValueError("pos_q8 must be [batch][stride][2]")
        p = pos_q8.to(torch.int64)
        px, py = p[..., 0], p[..., 1]
    U, V = torch.zeros_like(k), torch.zeros_like(k)
    level = torch.full_like(k, POSE_NO_LEVEL)
    for l, ((w, h, row0, col0), sl) in enumerate(zip(lvn, sc)):
        m = (x >= col0) & (x < col0 + w) & (y >= row0) & (y < row0 + h)
        U = torch.where(m, torch.div((px - (col0 << 8)) * sl + 32768, 65536, rounding_mode="floor"), U)
        V = torch.where(m, torch.div((py - (row0 << 8)) * sl + 32768, 65536, rounding_mode="floor"), V)
        level = torch.where(m, torch.full_like(k, l), level)
    found = level != POSE_NO_LEVEL
    ur = torch.full_like(k, POSE_MONO)
    if disp_q8 is not None:
        if tuple(disp_q8.shape) != tuple(kp.shape):
            raise ValueError("disp_q8 must have kp's shape")
        d = disp_q8.to(torch.int64)
        ur = torch.where(found & (d >= 0), U - d, ur)
    obs = torch.stack([U, V, ur], dim=-1).clamp(POSE_MONO, (1 << 31) - 1).to(torch.int32)
    return obs.contiguous(), level.to(torch.uint8).contiguous()


def matchedMapObservations(xw, tkp, sel, levels, scale_q16=None):
    """The (xw, obs_q8, level, counts) of poseRefineBatch from matchProjectionBatch's matches after selectMatchesBatch:
    sel = (sel_q, sel_t, nsel); slot s < nsel[b] pairs map point xw[b][sel_q[b][s]] with the observation
    poseObservationsQ8 makes of keypoint tkp[b][sel_t[b][s]] (monocular).  The slots at and beyond nsel[b] of sel_q and
    sel_t are unwritten memory: they are masked before gathering and come out as the point (0, 0, 0), the observation
    (0, 0, INT32_MIN) and the level 255.  Returns (xw float32 [batch][q_stride][3], obs_q8 int32 [batch][q_stride][3],
    level uint8 [batch][q_stride], counts int32 [batch] = nsel).  Torch ops on the current torch stream."""
    import torch
    sel_q, sel_t, nsel = sel
    batch, qs = (int(v) for v in sel_q.shape)
    dev = sel_q.device
    live = torch.arange(qs, device=dev)[None, :] < nsel.to(torch.int64)[:, None]
    zero = torch.zeros_like(live, dtype=torch.int64)
    qi = torch.where(live, sel_q.to(torch.int64), zero).clamp(0, int(xw.shape[1]) - 1)
    ti = torch.where(live, sel_t.to(torch.int64), zero).clamp(0, int(tkp.shape[1]) - 1)
    pts = torch.gather(xw, 1, qi[..., None].expand(-1, -1, 3))
    pts = torch.where(live[..., None], pts, torch.zeros_like(pts))
    obs, level = poseObservationsQ8(torch.gather(tkp.to(torch.int64), 1, ti), levels, scale_q16)
    dead = torch.tensor([0, 0, POSE_MONO], dtype=torch.int32, device=dev).expand(batch, qs, 3)
    obs = torch.where(live[..., None], obs, dead)
    level = torch.where(live, level, torch.full_like(level, POSE_NO_LEVEL))
    return pts.contiguous(), obs.contiguous(), level.contiguous(), nsel.to(torch.int32).clone()


def poseRefineBatch(pose, cam, xw, obs_q8, counts, *, level=None, inv_sigma2=None, rounds=4, iters=10, huber_rounds=3,
                    min_obs=10, eps=1e-6, pose_out=None, inlier=None, ninliers=None, cost=None, status=None,
                    ctx: Context | None = None):
    """Batched motion-only pose optimisation (pislam_pose_refine_batch; the contract is the comment in
    include/pislam_hip.h): per frame, the pose that minimises the robust reprojection error of map points xw (float32
    [batch][stride][3], stride <= 16384) against obs_q8 (int32 [batch][stride][3]: u, v, u_right in level-0 Q8 pixels,
    u_right == INT32_MIN for a monocular observation; poseObservationsQ8 makes them), starting from pose (float32
    [batch][12]: R row-major, then t; Xc = R Xw + t) with cam (float32 [batch][5]: fx, fy, cx, cy, bf); counts [batch].
    level (uint8 [batch][stride]) with inv_sigma2 (a HOST sequence of 1..16 float32, e.g. poseLevelWeights) weights
    each observation; without them every weight is 1.  ORB-SLAM's schedule: `rounds` rounds of up to `iters` Levenberg
    iterations, the first `huber_rounds` with the Huber kernel, an inlier classification after each; a round needs
    `min_obs` active observations.  Returns (pose_out float32 [batch][12], inlier uint8 [batch][stride] (entries at and
    beyond counts[b] are not written), ninliers int32 [batch], cost float64 [batch], status int32 [batch] = code |
    evaluations << 8; code 0 ok, 1 stopped for min_obs, 2 pose or cam not finite).  pose_out may be `pose` itself.
    The same inputs give the same outputs, bit for bit.  Asynchronous on the ctx stream, no workspace: capturable."""
    import torch
    ctx = ctx or default_context()
    batch, = _tensor(pose, torch.float32, (None, 12), "pose must be a float32 tensor [batch][12]")
    _tensor(cam, torch.float32, (batch, 5), "cam must be a float32 tensor [batch][5]")
    stride, = _tensor(xw, torch.float32, (batch, None, 3), "xw must be a float32 tensor [batch][stride][3]")
    _tensor(obs_q8, torch.int32, (batch, stride, 3), "obs_q8 must be an int32 tensor [batch][stride][3]")
    if stride > POSE_MAX_STRIDE:
        raise ValueError(f"at most {POSE_MAX_STRIDE} observations per frame")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    tab, ntab = _level_table((level,), inv_sigma2, batch, stride, "level and inv_sigma2 go together",
                             "level must be a uint8 tensor [batch][stride]")
    _contiguous(pose, cam, xw, obs_q8, counts, level)
    dev = pose.device
    p = capi.PoseParams(int(rounds), int(iters), int(huber_rounds), int(min_obs), float(eps))
    pose_out = torch.empty((batch, 12), dtype=torch.float32, device=dev) if pose_out is None else pose_out
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    ninliers = torch.empty((batch,), dtype=torch.int32, device=dev) if ninliers is None else ninliers
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    ctx.check(ctx.lib.pislam_pose_refine_batch(ctx.h, ctypes.byref(p), ptr(pose), ptr(cam), ptr(xw), ptr(obs_q8),
                                               ptr(counts), ptr(level), tab, ntab, stride, batch, ptr(pose_out),
                                               ptr(inlier), ptr(ninliers), ptr(cost), ptr(status)),
              "pislam_pose_refine_batch")
    return pose_out, inlier, ninliers, cost, status


# ---- absolute pose from 3D-2D matches: P3P RANSAC ----------
def pnpRansacBatch(cam, xw, obs_q8, counts, *, level=None, inv_sigma2=None, hypotheses=200, seed=0, min_inliers=10,
                   best=None, score=None, ninliers=None, inlier=None, pose_out=None, status=None,
                   ctx: Context | None = None):
    """Batched absolute-pose RANSAC (pislam_pnp_ransac_batch; the contract is the comment in include/pislam_hip.h): per
    frame, a camera pose from nothing, by P3P on `hypotheses` minimal samples of the 3D-2D matches xw (float32
    [batch][stride][3], stride <= 16384) and obs_q8 (int32 [batch][stride][3], poseRefineBatch's; the third word is
    ignored), with cam (float32 [batch][5]) and counts [batch]; level / inv_sigma2 as in poseRefineBatch.  Inputs are
    torch tensors or numpy arrays (numpy goes to the current device).  Returns (best int32 [batch] = the winning
    hypothesis or -1, score int32 [batch], ninliers int32 [batch], inlier uint8 [batch][stride] (entries at and beyond
    counts[b] are not written), pose_out float32 [batch][12] = poseRefineBatch's `pose`, status int32 [batch] = code |
    valid hypotheses << 8; code 0 ok, 1 fewer than min_inliers inliers, 2 no model, 3 bad camera).  The same inputs
    and seed give the same outputs, bit for bit.  Asynchronous on the ctx stream, no workspace: capturable."""
    import torch
    ctx = ctx or default_context()
    cam, xw, obs_q8, counts, level = map(_on_device, (cam, xw, obs_q8, counts, level))
    batch, = _tensor(cam, torch.float32, (None, 5), "cam must be a float32 tensor [batch][5]")
    stride, = _tensor(xw, torch.float32, (batch, None, 3), "xw must be a float32 tensor [batch][stride][3]")
    _tensor(obs_q8, torch.int32, (batch, stride, 3), "obs_q8 must be an int32 tensor [batch][stride][3]")
    if stride > POSE_MAX_STRIDE:
        raise ValueError(f"at most {POSE_MAX_STRIDE} observations per frame")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    tab, ntab = _level_table((level,), inv_sigma2, batch, stride, "level and inv_sigma2 go together",
                             "level must be a uint8 tensor [batch][stride]")
    _contiguous(cam, xw, obs_q8, counts, level)
    dev = cam.device
    p = capi.PnpParams(int(hypotheses), int(seed) & 0xFFFFFFFF, int(min_inliers))
    word = lambda t: torch.empty((batch,), dtype=torch.int32, device=dev) if t is None else t
    best, score, ninliers, status = word(best), word(score), word(ninliers), word(status)
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    pose_out = torch.empty((batch, 12), dtype=torch.float32, device=dev) if pose_out is None else pose_out
    ctx.check(ctx.lib.pislam_pnp_ransac_batch(ctx.h, ctypes.byref(p), ptr(cam), ptr(xw), ptr(obs_q8), ptr(counts),
                                              ptr(level), tab, ntab, stride, batch, ptr(best), ptr(score), ptr(ninliers),
                                              ptr(inlier), ptr(pose_out), ptr(status)), "pislam_pnp_ransac_batch")
    return best, score, ninliers, inlier, pose_out, status


# ---- similarity from 3D-3D matches: Sim(3) RANSAC (Horn) ----------
def cameraPoints(pose, xw):
    """Map points in camera frames: Xc = R Xw + t per frame, for pose float32 [batch][12] (R row-major, then t: the pose
    calls' layout) and world points xw float32 [batch][stride][3].  Plain torch; this is how callers who hold world
    points and key-frame poses make sim3RansacBatch's x1 and x2."""
    R, t = pose[:, :9].reshape(-1, 3, 3), pose[:, 9:12]
    return (xw @ R.transpose(1, 2) + t[:, None, :]).contiguous()


def sim3RansacBatch(cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, *, level1=None, level2=None, inv_sigma2=None,
                    hypotheses=200, seed=0, min_inliers=20, fixed_scale=False, best=None, score=None, ninliers=None,
                    inlier=None, sim_out=None, status=None, ctx: Context | None = None):
    """Batched Sim(3) RANSAC (pislam_sim3_ransac_batch; the contract is the comment in include/pislam_hip.h): per (key
    frame, loop candidate) pair, the similarity X1 = s R X2 + t by Horn's closed form on `hypotheses` minimal samples
    of the matched map points x1, x2 (float32 [batch][stride][3]: the same points in camera 1's and camera 2's frame,
    stride <= 16384), scored by reprojection against obs1_q8, obs2_q8 (int32 [batch][stride][3], poseRefineBatch's; the
    third word is ignored) with cam1, cam2 (float32 [batch][5]) and counts [batch]; level1 / level2 (both or neither)
    and inv_sigma2 as in poseRefineBatch.  fixed_scale forces s = 1 (stereo / RGB-D maps).  Inputs are torch tensors
    or numpy arrays (numpy goes to the current device).  Returns (best int32 [batch] = the winning hypothesis or -1,
    score int32 [batch], ninliers int32 [batch], inlier uint8 [batch][stride] (entries at and beyond counts[b] are not
    written), sim_out float32 [batch][13] = R row-major, t, s (the first 12 words are poseRefineBatch's `pose`),
    status int32 [batch] = code | valid hypotheses << 8; code 0 ok, 1 fewer than min_inliers inliers, 2 no model, 3 bad
    camera).  The same inputs and seed give the same outputs, bit for bit.  Asynchronous on the ctx stream, no
    workspace: capturable."""
    import torch
    ctx = ctx or default_context()
    cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2 = map(
        _on_device, (cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2))
    batch, = _tensor(cam1, torch.float32, (None, 5), "cam1 must be a float32 tensor [batch][5]")
    _tensor(cam2, torch.float32, (batch, 5), "cam2 must be a float32 tensor [batch][5]")
    stride, = _tensor(x1, torch.float32, (batch, None, 3), "x1 must be a float32 tensor [batch][stride][3]")
    _tensor(x2, torch.float32, (batch, stride, 3), "x2 must be a float32 tensor of x1's shape")
    for o in (obs1_q8, obs2_q8):
        _tensor(o, torch.int32, (batch, stride, 3), "obs1_q8 and obs2_q8 must be int32 tensors [batch][stride][3]")
    if stride > POSE_MAX_STRIDE:
        raise ValueError(f"at most {POSE_MAX_STRIDE} matches per pair")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    tab, ntab = _level_table((level1, level2), inv_sigma2, batch, stride, "level1, level2 and inv_sigma2 go together",
                             "level1 and level2 must be uint8 tensors [batch][stride]")
    _contiguous(cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2)
    dev = cam1.device
    p = capi.Sim3Params(int(hypotheses), int(seed) & 0xFFFFFFFF, int(min_inliers), int(bool(fixed_scale)))
    word = lambda t: torch.empty((batch,), dtype=torch.int32, device=dev) if t is None else t
    best, score, ninliers, status = word(best), word(score), word(ninliers), word(status)
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    sim_out = torch.empty((batch, 13), dtype=torch.float32, device=dev) if sim_out is None else sim_out
    ctx.check(ctx.lib.pislam_sim3_ransac_batch(ctx.h, ctypes.byref(p), ptr(cam1), ptr(cam2), ptr(x1), ptr(x2),
                                               ptr(obs1_q8), ptr(obs2_q8), ptr(counts), ptr(level1), ptr(level2), tab,
                                               ntab, stride, batch, ptr(best), ptr(score), ptr(ninliers), ptr(inlier),
                                               ptr(sim_out), ptr(status)), "pislam_sim3_ransac_batch")
    return best, score, ninliers, inlier, sim_out, status


def sim3RefineBatch(sim_in, cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, *, level1=None, level2=None, inv_sigma2=None,
                    mask=None, rounds=2, iters=5, huber_rounds=2, min_obs=10, th2=10.0, fixed_scale=False, eps=1e-6,
                    sim_out=None, inlier=None, ninliers=None, cost=None, status=None, ctx: Context | None = None):
    """Batched Sim(3) refinement (pislam_sim3_refine_batch; the contract is the comment in include/pislam_hip.h): per
    (key frame, loop candidate) pair, ORB-SLAM's OptimizeSim3: the similarity sim_in (float32 [batch][13]: R row-major,
    t, s; sim3RansacBatch's sim_out goes straight in) is refined over the matches by minimising the robust reprojection
    error in both images, the map points fixed.  cam1 .. counts, level1 / level2 / inv_sigma2 and fixed_scale are
    sim3RansacBatch's arguments, by its conventions.  mask (uint8 [batch][stride], optional): a 0 takes the match out
    (sim3RansacBatch's `inlier`, or the validity of a guided re-match).  ORB-SLAM's schedule: `rounds` rounds of up to
    `iters` Levenberg iterations, the first `huber_rounds` with a Huber kernel of delta^2 = th2 on each side, an inlier
    classification (both chi2 <= th2) after each; a round needs `min_obs` active matches.  Returns (sim_out float32
    [batch][13], inlier uint8 [batch][stride] (entries at and beyond counts[b] are not written), ninliers int32 [batch],
    cost float64 [batch], status int32 [batch] = code | evaluations << 8; code 0 ok, 1 stopped for min_obs, 2 bad
    similarity or camera).  sim_out may be `sim_in` itself.  The same inputs give the same outputs, bit for bit.
    Asynchronous on the ctx stream, no workspace: capturable."""
    import torch
    ctx = ctx or default_context()
    sim_in, cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2, mask = map(
        _on_device, (sim_in, cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2, mask))
    batch, = _tensor(sim_in, torch.float32, (None, 13), "sim_in must be a float32 tensor [batch][13]")
    for c in (cam1, cam2):
        _tensor(c, torch.float32, (batch, 5), "cam1 and cam2 must be float32 tensors [batch][5]")
    stride, = _tensor(x1, torch.float32, (batch, None, 3), "x1 must be a float32 tensor [batch][stride][3]")
    _tensor(x2, torch.float32, (batch, stride, 3), "x2 must be a float32 tensor of x1's shape")
    for o in (obs1_q8, obs2_q8):
        _tensor(o, torch.int32, (batch, stride, 3), "obs1_q8 and obs2_q8 must be int32 tensors [batch][stride][3]")
    if stride > POSE_MAX_STRIDE:
        raise ValueError(f"at most {POSE_MAX_STRIDE} matches per pair")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    tab, ntab = _level_table((level1, level2), inv_sigma2, batch, stride, "level1, level2 and inv_sigma2 go together",
                             "level1 and level2 must be uint8 tensors [batch][stride]")
    if mask is not None:
        _tensor(mask, torch.uint8, (batch, stride), "mask must be a uint8 tensor [batch][stride]")
    _contiguous(sim_in, cam1, cam2, x1, x2, obs1_q8, obs2_q8, counts, level1, level2, mask)
    dev = sim_in.device
    p = capi.Sim3RefineParams(int(rounds), int(iters), int(huber_rounds), int(min_obs), float(th2), int(bool(fixed_scale)),
                              float(eps))
    word = lambda t: torch.empty((batch,), dtype=torch.int32, device=dev) if t is None else t
    ninliers, status = word(ninliers), word(status)
    sim_out = torch.empty((batch, 13), dtype=torch.float32, device=dev) if sim_out is None else sim_out
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    ctx.check(ctx.lib.pislam_sim3_refine_batch(ctx.h, ctypes.byref(p), ptr(sim_in), ptr(cam1), ptr(cam2), ptr(x1), ptr(x2),
                                               ptr(obs1_q8), ptr(obs2_q8), ptr(counts), ptr(level1), ptr(level2), ptr(mask),
                                               tab, ntab, stride, batch, ptr(sim_out), ptr(inlier), ptr(ninliers),
                                               ptr(cost), ptr(status)), "pislam_sim3_refine_batch")
    return sim_out, inlier, ninliers, cost, status


# ---- new map points from two key frames ----------
def epipolarGeometry(pose1, pose2, cam1, cam2):
    """pislam_epipolar_from_poses on the host: the fundamental matrix and the epipole of key-frame pairs with known
    poses.  pose1, pose2: [12] or [batch][12] (R row-major, then t; Xc = R Xw + t), cam1, cam2: [4] or [5] (bf is
    ignored) or [batch][4 or 5]: fx, fy, cx, cy; tensors (host or device) or arrays.  Returns (f12 float32 [..][9] with
    x1' F12 x2 = 0 in level-0 pixels, epipole float32 [..][2] = camera 1's centre in image 2): matchEpipolarBatch's
    inputs, after a copy to the device.  A pair whose pose or camera is not finite, or whose fx or fy is 0, gives rows of
    NaN, which the matcher treats as a pair without candidates."""
    host = lambda a: np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
    p1, p2, c1, c2 = host(pose1), host(pose2), host(cam1), host(cam2)
    single = p1.ndim == 1
    p1, p2 = np.ascontiguousarray(p1.reshape(-1, 12)), np.ascontiguousarray(p2.reshape(-1, 12))
    c1 = np.ascontiguousarray(c1.reshape(len(p1), -1)[:, :4])
    c2 = np.ascontiguousarray(c2.reshape(len(p1), -1)[:, :4])
    if p2.shape != p1.shape or c1.shape != (len(p1), 4) or c2.shape != (len(p1), 4):
        raise ValueError("poses must be [batch][12] and cameras [batch][4 or 5]")
    f12 = np.full((len(p1), 9), np.nan, dtype=np.float32)
    epipole = np.full((len(p1), 2), np.nan, dtype=np.float32)
    lib = capi.load()
    fp = ctypes.POINTER(ctypes.c_float)
    for b in range(len(p1)):
        f, e = np.empty(9, np.float32), np.empty(2, np.float32)
        rc = lib.pislam_epipolar_from_poses(p1[b].ctypes.data_as(fp), p2[b].ctypes.data_as(fp), c1[b].ctypes.data_as(fp),
                                            c2[b].ctypes.data_as(fp), f.ctypes.data_as(fp), e.ctypes.data_as(fp))
        if rc == capi.PISLAM_OK:
            f12[b], epipole[b] = f, e
    return (f12[0], epipole[0]) if single else (f12, epipole)


def reserveMatchEpipolar(ngroups: int, t_stride: int, batch: int, *, words=8, ctx: Context | None = None):
    """Sizes the context's epipolar matcher workspace (pislam_match_epipolar_reserve): afterwards matchEpipolarBatch of
    the same or a smaller shape allocates nothing and can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_match_epipolar_reserve(ctx.h, words, int(ngroups), t_stride, batch),
              "pislam_match_epipolar_reserve")


def matchEpipolarBatch(qdesc, qgroup, qobs_q8, qlevel, qcounts, tdesc, tgroup, tobs_q8, tlevel, tcounts, ngroups: int, f12,
                       epipole, *, qmask=None, tmask=None, level_sigma2=None, level_scale=None, nlevels=8, scale=1.2,
                       chi2=3.84, epipole_r2=100.0, idx=None, dist=None, dist2=None, ctx: Context | None = None):
    """Epipolar search between two key frames (pislam_match_hamming_epipolar_batch; the contract is the comment in
    include/pislam_hip.h), ORB-SLAM's SearchForTriangulation before its selection: matchHammingBowBatch (same
    descriptors, groups and counts) restricted to the train keypoints that lie within chi2 * level_sigma2[their level] of
    the query's epipolar line and, when both keypoints are monocular, outside the disc of epipole_r2 *
    level_scale[their level] around the epipole.  qobs_q8 / tobs_q8 (int32 [batch][stride][3]) and qlevel / tlevel (uint8
    [batch][stride]) are poseObservationsQ8's outputs; qmask / tmask (uint8 [batch][stride] or None) keep the keypoints
    that have no map point yet; f12 float32 [batch][9] and epipole float32 [batch][2] are epipolarGeometry's, on the
    device.  level_sigma2 / level_scale: HOST sequences of 1..16 float32 (default: mapPointLevelTables(nlevels, scale)).
    Returns (idx, dist, dist2) int32 tensors [batch][q_stride] for selectMatchesBatch; asynchronous on the ctx stream."""
    import torch
    ctx = ctx or default_context()
    batch, qs, words = (int(v) for v in qdesc.shape)
    ts = int(tdesc.shape[1])
    if int(tdesc.shape[0]) != batch or int(tdesc.shape[2]) != words:
        raise ValueError("query and train descriptors differ in batch or words")
    for name, t, shape, dt in (("qgroup", qgroup, (batch, qs), None), ("tgroup", tgroup, (batch, ts), None),
                               ("qobs_q8", qobs_q8, (batch, qs, 3), torch.int32), ("tobs_q8", tobs_q8, (batch, ts, 3), torch.int32),
                               ("qlevel", qlevel, (batch, qs), torch.uint8), ("tlevel", tlevel, (batch, ts), torch.uint8),
                               ("qmask", qmask, (batch, qs), torch.uint8), ("tmask", tmask, (batch, ts), torch.uint8),
                               ("f12", f12, (batch, 9), torch.float32), ("epipole", epipole, (batch, 2), torch.float32)):
        if t is None and name in ("qmask", "tmask"):
            continue
        message = f"{name} must be a contiguous tensor of shape {shape}" + (f" and type {dt}" if dt else "")
        _tensor(t, dt, shape, message)
        _contiguous(t, message=message)
    if (level_sigma2 is None) != (level_scale is None):
        raise ValueError("level_sigma2 and level_scale go together")
    if level_sigma2 is None:
        level_scale, level_sigma2 = mapPointLevelTables(nlevels, scale)
    unequal = "level_sigma2 and level_scale must have the same 1..16 entries"
    tab_sg, ntab = _float_table(level_sigma2, unequal)
    tab_ls, _ = _float_table(level_scale, unequal, ntab)
    p = capi.EpipolarParams(float(np.float32(chi2)), float(np.float32(epipole_r2)))
    idx, dist, dist2 = _match_outputs(qdesc, idx, dist, dist2)
    ctx.check(ctx.lib.pislam_match_hamming_epipolar_batch(
        ctx.h, words, int(ngroups), ctypes.byref(p), tab_sg, tab_ls, ntab, ptr(f12), ptr(epipole), ptr(qdesc), ptr(qgroup),
        ptr(qobs_q8), ptr(qlevel), ptr(qmask), ptr(qcounts), qs, ptr(tdesc), ptr(tgroup), ptr(tobs_q8), ptr(tlevel),
        ptr(tmask), ptr(tcounts), ts, batch, ptr(idx), ptr(dist), ptr(dist2)), "pislam_match_hamming_epipolar_batch")
    return idx, dist, dist2


TRIANGULATE_MAX_STRIDE = 16384   # slots per pair (pislam_triangulate_batch)
TRIANGULATE_STATUS = ("ok", "no level", "low parallax", "not finite", "depth 1", "depth 2", "reprojection 1",
                      "reprojection 2", "scale", "pair")


def mapPointLevelTables(nlevels: int, scale: float = 1.2):
    """The (level_scale, level_sigma2) tables of triangulateBatch for a pyramid of `nlevels` levels (1..16) with the
    scale factor `scale`, computed one float32 operation at a time as poseLevelWeights does: s = float32(scale),
    f_0 = 1, f_l = f_(l-1) * s, level_scale_l = f_l, level_sigma2_l = f_l * f_l (ORB-SLAM's mvScaleFactors and
    mvLevelSigma2; poseLevelWeights(nlevels, scale) is 1 / level_sigma2 entry by entry)."""
    if not 1 <= int(nlevels) <= 16:
        raise ValueError("nlevels must be 1..16")
    s, f = np.float32(scale), np.float32(1.0)
    level_scale = np.empty(int(nlevels), dtype=np.float32)
    for l in range(int(nlevels)):
        level_scale[l] = f
        f = f * s
    return level_scale, level_scale * level_scale


def matchedObservationPairs(qobs, qlevel, tobs, tlevel, sel):
    """The (obs1_q8, level1, obs2_q8, level2, counts) of triangulateBatch from two key frames' observations
    (poseObservationsQ8's outputs: qobs / tobs int32 [batch][stride][3], qlevel / tlevel uint8 [batch][stride]) and the
    matches selectMatchesBatch accepted between them: sel = (sel_q, sel_t, nsel); slot s < nsel[b] pairs keypoint
    sel_q[b][s] of the query key frame (side 1) with keypoint sel_t[b][s] of the train key frame (side 2).  The slots at
    and beyond nsel[b] of sel_q and sel_t are unwritten memory: they are masked before gathering and come out as the
    observation (0, 0, INT32_MIN) and the level 255, as in matchedMapObservations.  Torch ops on the current torch
    stream."""
    import torch
    sel_q, sel_t, nsel = sel
    batch, qs = (int(v) for v in sel_q.shape)
    dev = sel_q.device
    live = torch.arange(qs, device=dev)[None, :] < nsel.to(torch.int64)[:, None]
    zero = torch.zeros_like(live, dtype=torch.int64)
    dead = torch.tensor([0, 0, POSE_MONO], dtype=torch.int32, device=dev).expand(batch, qs, 3)
    out = []
    for obs, level, sel_i in ((qobs, qlevel, sel_q), (tobs, tlevel, sel_t)):
        if obs.dtype != torch.int32 or obs.dim() != 3 or int(obs.shape[2]) != 3:
            raise ValueError("observations must be int32 tensors [batch][stride][3]")
        if level.dtype != torch.uint8 or tuple(level.shape) != tuple(obs.shape[:2]):
            raise ValueError("levels must be uint8 tensors [batch][stride]")
        i = torch.where(live, sel_i.to(torch.int64), zero).clamp(0, int(obs.shape[1]) - 1)
        o = torch.where(live[..., None], torch.gather(obs, 1, i[..., None].expand(-1, -1, 3)), dead)
        l = torch.where(live, torch.gather(level, 1, i), torch.full_like(i, POSE_NO_LEVEL, dtype=torch.uint8))
        out += [o.contiguous(), l.contiguous()]
    return out[0], out[1], out[2], out[3], nsel.to(torch.int32).clone()


def triangulateBatch(pose1, pose2, cam1, cam2, obs1_q8, obs2_q8, level1, level2, counts, *, level_scale=None,
                     level_sigma2=None, nlevels=8, scale=1.2, cos_min_parallax=0.9998, chi2_mono=5.991, chi2_stereo=7.815,
                     ratio_factor=None, want_normal=True, want_drange=True, xw=None, status=None, normal=None,
                     drange=None, npoints=None, ctx: Context | None = None):
    """Batched creation of map points from the matches of two key frames (pislam_triangulate_batch; the contract is the
    comment in include/pislam_hip.h), the geometry of ORB-SLAM's CreateNewMapPoints: per pair, slot s < counts[b] holds
    one match as two observations obs1_q8 / obs2_q8 (int32 [batch][stride][3]: u, v, u_right in level-0 Q8 pixels,
    u_right == INT32_MIN for a monocular keypoint) on the levels level1 / level2 (uint8 [batch][stride]);
    matchedObservationPairs makes all five.  pose1, pose2 (float32 [batch][12]: R row-major, then t; Xc = R Xw + t) and
    cam1, cam2 (float32 [batch][5]: fx, fy, cx, cy, bf) are the key frames.  The point is triangulated, or unprojected
    from a stereo observation when that has more parallax, and kept iff it lies in front of both cameras, reprojects
    within chi2 * level_sigma2 in both and its distances fit the two levels within ratio_factor (default: float32(1.5)
    * float32(scale)).  level_scale / level_sigma2: HOST sequences of 1..16 float32 (default: mapPointLevelTables(nlevels,
    scale)).  Returns (xw float32 [batch][stride][3] (zeros unless status is 0), status uint8 [batch][stride]
    (TRIANGULATE_STATUS names the codes), normal float32 [batch][stride][3] and drange float32 [batch][stride][2] (what
    matchProjectionBatch reads in map mode; None when not wanted), npoints int32 [batch]).  Entries at and beyond
    counts[b] are not written.  The same inputs give the same outputs, bit for bit.  Asynchronous on the ctx stream, no
    workspace: capturable as it is."""
    import torch
    ctx = ctx or default_context()
    batch, = _tensor(pose1, torch.float32, (None, 12), "pose1 must be a float32 tensor [batch][12]")
    _tensor(pose2, torch.float32, (batch, 12), "pose2 must be a float32 tensor [batch][12]")
    for cam in (cam1, cam2):
        _tensor(cam, torch.float32, (batch, 5), "cam1 and cam2 must be float32 tensors [batch][5]")
    stride, = _tensor(obs1_q8, torch.int32, (batch, None, 3), "obs1_q8 must be an int32 tensor [batch][stride][3]")
    _tensor(obs2_q8, torch.int32, (batch, stride, 3), "obs2_q8 must be an int32 tensor of obs1_q8's shape")
    if stride > TRIANGULATE_MAX_STRIDE:
        raise ValueError(f"at most {TRIANGULATE_MAX_STRIDE} slots per pair")
    for level in (level1, level2):
        _tensor(level, torch.uint8, (batch, stride), "level1 and level2 must be uint8 tensors [batch][stride]")
    _counts("counts must be a 32-bit integer tensor [batch]", batch, counts)
    _contiguous(pose1, pose2, cam1, cam2, obs1_q8, obs2_q8, level1, level2, counts)
    if (level_scale is None) != (level_sigma2 is None):
        raise ValueError("level_scale and level_sigma2 go together")
    if level_scale is None:
        level_scale, level_sigma2 = mapPointLevelTables(nlevels, scale)
    unequal = "level_scale and level_sigma2 must have the same 1..16 entries"
    tab_ls, ntab = _float_table(level_scale, unequal)
    tab_sg, _ = _float_table(level_sigma2, unequal, ntab)
    if ratio_factor is None:
        ratio_factor = np.float32(1.5) * np.float32(scale)
    p = capi.TriangulateParams(float(np.float32(cos_min_parallax)), float(np.float32(chi2_mono)),
                               float(np.float32(chi2_stereo)), float(np.float32(ratio_factor)))
    dev = pose1.device
    xw = torch.empty((batch, stride, 3), dtype=torch.float32, device=dev) if xw is None else xw
    status = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if status is None else status
    if normal is None and want_normal:
        normal = torch.empty((batch, stride, 3), dtype=torch.float32, device=dev)
    if drange is None and want_drange:
        drange = torch.empty((batch, stride, 2), dtype=torch.float32, device=dev)
    npoints = torch.empty((batch,), dtype=torch.int32, device=dev) if npoints is None else npoints
    ctx.check(ctx.lib.pislam_triangulate_batch(ctx.h, ctypes.byref(p), ptr(pose1), ptr(pose2), ptr(cam1), ptr(cam2),
                                               ptr(obs1_q8), ptr(obs2_q8), ptr(level1), ptr(level2), ptr(counts), tab_ls,
                                               tab_sg, ntab, stride, batch, ptr(xw), ptr(status), ptr(normal),
                                               ptr(drange), ptr(npoints)), "pislam_triangulate_batch")
    return xw, status, normal, drange, npoints


# ---- local bundle adjustment: key-frame poses and map points together ----------
BA_MAX_KF, BA_MAX_FREE, BA_MAX_POINTS = 32, 16, 4096


def localWindow(obs_kf, obs_pt, kp, counts, levels, scale_q16=None, disp_q8=None, pos_q8=None):
    """The observations of localBundleAdjustBatch from per-observation lists in any order: obs_kf, obs_pt and kp are
    integer tensors [batch][stride] (key frame of the window, point of the window, keypoint word), counts [batch].  The
    first counts[b] entries of a row are sorted by point and by key frame within a point (a stable sort of the key
    obs_pt * 64 + obs_kf; the call itself refuses a window in which a pair occurs twice); the entries behind them stay
    behind.  The coordinates and levels are poseObservationsQ8's (levels, scale_q16, disp_q8, pos_q8 as there), sorted
    alike.  Returns (obs_q8 int32 [batch][stride][3], obs_kf uint8 [batch][stride], obs_pt int16 [batch][stride] (the
    uint16 words of the call: a point index is below 4096), level uint8 [batch][stride], counts int32 [batch]).  Torch
    ops on the current torch stream."""
    import torch
    if obs_kf.dim() != 2 or tuple(obs_pt.shape) != tuple(obs_kf.shape) or tuple(kp.shape) != tuple(obs_kf.shape):
        raise ValueError("obs_kf, obs_pt and kp must be [batch][stride]")
    batch, stride = (int(v) for v in obs_kf.shape)
    if tuple(counts.shape) != (batch,):
        raise ValueError("counts must be [batch]")
    obs, level = poseObservationsQ8(kp, levels, scale_q16, disp_q8, pos_q8)
    k, p = obs_kf.to(torch.int64), obs_pt.to(torch.int64)
    live = torch.arange(stride, device=k.device)[None, :] < counts.to(torch.int64).clamp(0, stride)[:, None]
    key = torch.where(live, p.clamp(0, 0xFFFF) * 64 + k.clamp(0, 63), torch.full_like(k, 1 << 40))
    order = torch.argsort(key, dim=1, stable=True)
    g = lambda t: torch.gather(t, 1, order)
    obs = torch.gather(obs, 1, order[..., None].expand(-1, -1, 3))
    return (obs.contiguous(), g(k).clamp(0, 255).to(torch.uint8).contiguous(),
            g(p).clamp(0, 0x7FFF).to(torch.int16).contiguous(), g(level).contiguous(),
            counts.to(torch.int64).clamp(0, stride).to(torch.int32))


def reserveLocalBundleAdjust(kf_stride: int, pt_stride: int, stride: int, batch: int, *, ctx: Context | None = None):
    """Size the context's workspace for localBundleAdjustBatch calls of up to this shape (pislam_local_ba_reserve):
    afterwards such calls allocate nothing and never synchronise, so they can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_local_ba_reserve(ctx.h, int(kf_stride), int(pt_stride), int(stride), int(batch)),
              "pislam_local_ba_reserve")


def localBundleAdjustBatch(poses, cams, kf_counts, kf_free, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, *, level=None,
                           inv_sigma2=None, rounds=2, iters=(5, 10), huber_rounds=1, min_obs=10, eps=1e-6,
                           poses_out=None, xw_out=None, inlier=None, ninliers=None, cost=None, status=None,
                           ctx: Context | None = None):
    """Batched local bundle adjustment (pislam_local_ba_batch; the contract is the comment in include/pislam_hip.h):
    per window, the poses of the free key frames [0, kf_free[b]) and all map points are moved together to minimise the
    robust reprojection error of the observations; the key frames from kf_free[b] on are held fixed.  poses float32
    [batch][kf_stride][12] (kf_stride <= 32, at most 16 free), cams float32 [batch][kf_stride][5], xw float32
    [batch][pt_stride][3] (pt_stride <= 4096; triangulateBatch's xw as it is), obs_q8 int32 [batch][stride][3] (stride
    <= 16384) with obs_kf uint8 and obs_pt int16 or uint16 [batch][stride], sorted by point and key frame (localWindow
    makes them); kf_counts, kf_free, pt_counts, counts [batch]; level and inv_sigma2 as in poseRefineBatch.  ORB-SLAM's
    schedule: `rounds` rounds of up to iters[r] Levenberg iterations, the first `huber_rounds` robust, an inlier
    classification after each.  Returns (poses_out, xw_out, inlier uint8 [batch][stride], ninliers int32 [batch], cost
    float64 [batch], status int32 [batch] = code | evaluations << 8; code 0 ok, 1 stopped for min_obs, 2 an input is
    not finite, 3 the window is malformed).  poses_out may be `poses` and xw_out may be `xw`.  The same inputs give the
    same outputs, bit for bit.  Asynchronous on the ctx stream; capturable after reserveLocalBundleAdjust."""
    import torch
    ctx = ctx or default_context()
    batch, kfs = _tensor(poses, torch.float32, (None, None, 12), "poses must be a float32 tensor [batch][kf_stride][12]")
    _tensor(cams, torch.float32, (batch, kfs, 5), "cams must be a float32 tensor [batch][kf_stride][5]")
    pts, = _tensor(xw, torch.float32, (batch, None, 3), "xw must be a float32 tensor [batch][pt_stride][3]")
    stride, = _tensor(obs_q8, torch.int32, (batch, None, 3), "obs_q8 must be an int32 tensor [batch][stride][3]")
    _tensor(obs_kf, torch.uint8, (batch, stride), "obs_kf must be a uint8 tensor [batch][stride]")
    _tensor(obs_pt, _word16(), (batch, stride), "obs_pt must be a 16-bit integer tensor [batch][stride]")
    if kfs > BA_MAX_KF or pts > BA_MAX_POINTS or stride > POSE_MAX_STRIDE:
        raise ValueError(f"at most {BA_MAX_KF} key frames, {BA_MAX_POINTS} points and {POSE_MAX_STRIDE} observations per window")
    _counts("kf_counts, kf_free, pt_counts and counts must be 32-bit integer tensors [batch]", batch,
            kf_counts, kf_free, pt_counts, counts)
    tab, ntab = _level_table((level,), inv_sigma2, batch, stride, "level and inv_sigma2 go together",
                             "level must be a uint8 tensor [batch][stride]")
    _contiguous(poses, cams, kf_counts, kf_free, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, level)
    its = [int(v) for v in (iters if hasattr(iters, "__len__") else [iters] * int(rounds))]
    if len(its) < int(rounds) or len(its) > 4:
        raise ValueError("iters needs an entry per round, at most 4")
    p = capi.BaParams(int(rounds), (ctypes.c_int32 * 4)(*(its + [1] * (4 - len(its)))), int(huber_rounds), int(min_obs),
                      float(eps))
    dev = poses.device
    poses_out = torch.empty_like(poses) if poses_out is None else poses_out
    xw_out = torch.empty_like(xw) if xw_out is None else xw_out
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    ninliers = torch.empty((batch,), dtype=torch.int32, device=dev) if ninliers is None else ninliers
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    ctx.check(ctx.lib.pislam_local_ba_batch(ctx.h, ctypes.byref(p), ptr(poses), ptr(cams), ptr(kf_counts), ptr(kf_free),
                                            ptr(xw), ptr(pt_counts), ptr(obs_q8), ptr(obs_kf), ptr(obs_pt), ptr(level),
                                            ptr(counts), tab, ntab, kfs, pts, stride, batch, ptr(poses_out), ptr(xw_out),
                                            ptr(inlier), ptr(ninliers), ptr(cost), ptr(status)),
              "pislam_local_ba_batch")
    return poses_out, xw_out, inlier, ninliers, cost, status


# ---- after a loop is accepted: essential-graph optimisation, map points moved ----------
POSE_GRAPH_MAX_VERTICES, POSE_GRAPH_MAX_EDGES = 4096, 16384
POSE_GRAPH_WIDE_MAX_VERTICES, POSE_GRAPH_WIDE_MAX_EDGES = 65536, 1 << 20     # poseGraphWideBatch


def relativeSim3(sim_i, sim_j):
    """M = S_j o S_i^-1 for similarities [..][13] = (R row-major, t, s): the measurement of an essential-graph edge (i,
    j) taken from the two vertices (ORB-SLAM's Sji).  Computed in float64 and rounded once to float32.  Torch tensors."""
    import torch
    a, b = sim_i.to(torch.float64), sim_j.to(torch.float64)
    Ri, Rj = a[..., :9].reshape(*a.shape[:-1], 3, 3), b[..., :9].reshape(*b.shape[:-1], 3, 3)
    R = Rj @ Ri.transpose(-1, -2)
    s = b[..., 12:13] / a[..., 12:13]
    t = b[..., 9:12] - s * (R @ a[..., 9:12, None])[..., 0]
    return torch.cat([R.reshape(*a.shape[:-1], 9), t, s], dim=-1).to(torch.float32)


def essentialGraph(sims, fixed, pairs, meas=None, weight=None, *, wide=False):
    """The padded batch arrays and the incidence index of poseGraphBatch from per-graph lists.  One graph: sims float32
    [nv][13] (world to camera, the sim_out layout), fixed a boolean or integer tensor [nv] (nonzero: held), pairs an
    integer tensor [ne][2] = (i, j); a batch: lists of such tensors, one entry per graph.  meas: None, or float32
    [m][13] with m <= ne, the measurements S_j o S_i^-1 of the LAST m pairs (the loop edges, which come with their own
    measurement); the pairs before them (spanning tree, covisibility) get relativeSim3 of the similarities passed in, as
    ORB-SLAM takes them from the uncorrected poses.  weight: None or float32 [ne].  Returns (sims [batch][v_stride][13],
    v_counts int32, fixed uint8 [batch][v_stride], edges int32 [batch][e_stride][2], meas float32
    [batch][e_stride][13], weight float32 [batch][e_stride] or None, e_counts int32, inc_ptr int32
    [batch][v_stride + 1], inc int32 [batch][2 * e_stride]) with the strides of the largest graph (at least 1).  A vertex's
    entries edge << 1 | side are ascending.  The pairs are not checked: the call refuses a malformed graph with code 3.
    wide=True: the graph is for poseGraphWideBatch and is held to its limits (65536 vertices, 2^20 edges) instead.
    Torch ops on the current torch stream."""
    import torch
    one = not isinstance(sims, (list, tuple))
    if one:
        sims, fixed, pairs, meas, weight = [sims], [fixed], [pairs], [meas], [weight]
    B = len(sims)
    meas = [None] * B if meas is None else meas
    have_w = weight is not None and any(w is not None for w in weight)
    weight = [None] * B if weight is None else weight
    if not (len(fixed) == len(pairs) == len(meas) == len(weight) == B) or B == 0:
        raise ValueError("one entry per graph in every list")
    dev = sims[0].device
    V = max(max(int(s.shape[0]) for s in sims), 1)
    E = max(max(int(p.shape[0]) for p in pairs), 1)
    max_v, max_e = ((POSE_GRAPH_WIDE_MAX_VERTICES, POSE_GRAPH_WIDE_MAX_EDGES) if wide else
                    (POSE_GRAPH_MAX_VERTICES, POSE_GRAPH_MAX_EDGES))
    if V > max_v or E > max_e:
        raise ValueError(f"at most {max_v} vertices and {max_e} edges per graph")
    o_s = torch.zeros((B, V, 13), dtype=torch.float32, device=dev)
    o_f = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    o_e = torch.zeros((B, E, 2), dtype=torch.int32, device=dev)
    o_m = torch.zeros((B, E, 13), dtype=torch.float32, device=dev)
    o_w = torch.ones((B, E), dtype=torch.float32, device=dev) if have_w else None
    o_p = torch.zeros((B, V + 1), dtype=torch.int32, device=dev)
    o_i = torch.zeros((B, 2 * E), dtype=torch.int32, device=dev)
    nvs, nes = [], []
    for b in range(B):
        s, p = sims[b], pairs[b].to(torch.int64).reshape(-1, 2)
        nv, ne = int(s.shape[0]), int(p.shape[0])
        if s.dtype != torch.float32 or tuple(s.shape) != (nv, 13) or tuple(fixed[b].shape) != (nv,):
            raise ValueError("sims must be float32 [nv][13] and fixed [nv]")
        nvs.append(nv), nes.append(ne)
        o_s[b, :nv], o_f[b, :nv], o_e[b, :ne] = s, (fixed[b] != 0).to(torch.uint8), p.to(torch.int32)
        m = 0 if meas[b] is None else int(meas[b].shape[0])
        if m > ne or (m and tuple(meas[b].shape) != (m, 13)):
            raise ValueError("meas must be float32 [m][13] with m <= ne")
        if ne > m:
            i, j = p[:ne - m, 0].clamp(0, max(nv - 1, 0)), p[:ne - m, 1].clamp(0, max(nv - 1, 0))
            o_m[b, :ne - m] = relativeSim3(s[i], s[j]) if nv else 0.0
        if m:
            o_m[b, ne - m:ne] = meas[b].to(torch.float32)
        if have_w and weight[b] is not None:
            o_w[b, :ne] = weight[b].to(torch.float32)
        # the index: the entries edge << 1 | side sorted by (vertex, entry)
        ent = torch.arange(2 * ne, device=dev, dtype=torch.int64)
        vert = p.reshape(-1).clamp(0, V)                     # (a vertex out of range is refused by the call anyway)
        order = torch.argsort(vert * (2 * ne + 1) + ent, stable=True)
        o_i[b, :2 * ne] = ent[order].to(torch.int32)
        cnt = torch.bincount(vert[vert < nv], minlength=nv)[:nv] if nv else torch.zeros(0, dtype=torch.int64, device=dev)
        o_p[b, 1:nv + 1] = torch.cumsum(cnt, 0).to(torch.int32)
    cnts = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    return o_s, cnts(nvs), o_f, o_e, o_m, o_w, cnts(nes), o_p, o_i


def reservePoseGraph(v_stride: int, e_stride: int, batch: int, *, ctx: Context | None = None):
    """Size the context's workspace for poseGraphBatch calls of up to this shape (pislam_pose_graph_reserve): afterwards
    such calls allocate nothing and never synchronise, so they can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_pose_graph_reserve(ctx.h, int(v_stride), int(e_stride), int(batch)), "pislam_pose_graph_reserve")


def _pose_graph_shape(sims, edges):
    """The first tensor checks of poseGraphBatch and poseGraphWideBatch: (batch, v_stride, e_stride)."""
    import torch
    batch, V = _tensor(sims, torch.float32, (None, None, 13), "sims must be a float32 tensor [batch][v_stride][13]")
    E, = _tensor(edges, _word32(), (batch, None, 2), "edges must be a 32-bit integer tensor [batch][e_stride][2]")
    return batch, V, E


def _pose_graph_rest(batch, V, E, sims, v_counts, fixed, edges, meas, weight, e_counts, inc_ptr, inc):
    """The tensor checks that follow the limits, in their order."""
    import torch
    _tensor(fixed, torch.uint8, (batch, V), "fixed must be a uint8 tensor [batch][v_stride]")
    _tensor(meas, torch.float32, (batch, E, 13), "meas must be a float32 tensor [batch][e_stride][13]")
    if weight is not None:
        _tensor(weight, torch.float32, (batch, E), "weight must be a float32 tensor [batch][e_stride]")
    for t, shape in ((v_counts, (batch,)), (e_counts, (batch,)), (inc_ptr, (batch, V + 1)), (inc, (batch, 2 * E))):
        _tensor(t, _word32(), shape, "v_counts, e_counts [batch], inc_ptr [batch][v_stride + 1] and inc [batch][2 * e_stride] "
                                     "must be 32-bit integer tensors")
    _contiguous(sims, v_counts, fixed, edges, meas, e_counts, inc_ptr, inc, weight)


def poseGraphBatch(sims, v_counts, fixed, edges, meas, weight, e_counts, inc_ptr, inc, *, iters=20, cg_iters=256,
                   cg_tol=1e-6, eps=1e-9, sims_out=None, cost=None, status=None, ctx: Context | None = None):
    """Batched essential-graph optimisation (pislam_pose_graph_batch; the contract is the comment in include/
    pislam_hip.h), ORB-SLAM's OptimizeEssentialGraph: per graph the free vertex similarities are moved so that the sum
    of the squared relative-Sim(3) errors over the edges becomes minimal.  The arguments are essentialGraph's outputs
    in order: sims float32 [batch][v_stride][13], v_counts, fixed uint8 [batch][v_stride], edges 32-bit integers
    [batch][e_stride][2], meas float32 [batch][e_stride][13], weight float32 [batch][e_stride] or None, e_counts, inc_ptr
    [batch][v_stride + 1], inc [batch][2 * e_stride].  One Levenberg round of up to `iters` iterations, each a
    preconditioned conjugate-gradient solve of up to cg_iters iterations that stops at a relative residual of cg_tol.
    Returns (sims_out, cost float64 [batch], status int32 [batch] = code | evaluations << 8; code 0 ok, 1 nothing to do,
    2 a bad value or an inadmissible input state, 3 the graph is malformed).  sims_out may be `sims`.  The same inputs
    give the same outputs, bit for bit.  Asynchronous on the ctx stream; capturable after reservePoseGraph.  Key-frame
    poses afterwards: rigidFromSim3(sims_out[b]).  One workgroup runs a graph: for a large graph, or one beyond 4096
    vertices or 16384 edges, use poseGraphWideBatch."""
    import torch
    ctx = ctx or default_context()
    batch, V, E = _pose_graph_shape(sims, edges)
    if V > POSE_GRAPH_MAX_VERTICES or E > POSE_GRAPH_MAX_EDGES:
        raise ValueError(f"at most {POSE_GRAPH_MAX_VERTICES} vertices and {POSE_GRAPH_MAX_EDGES} edges per graph")
    _pose_graph_rest(batch, V, E, sims, v_counts, fixed, edges, meas, weight, e_counts, inc_ptr, inc)
    p = capi.PoseGraphParams(int(iters), int(cg_iters), float(cg_tol), float(eps))
    dev = sims.device
    sims_out = torch.empty_like(sims) if sims_out is None else sims_out
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    ctx.check(ctx.lib.pislam_pose_graph_batch(ctx.h, ctypes.byref(p), ptr(sims), ptr(v_counts), ptr(fixed), ptr(edges),
                                              ptr(meas), ptr(weight), ptr(e_counts), ptr(inc_ptr), ptr(inc), V, E, batch,
                                              ptr(sims_out), ptr(cost), ptr(status)), "pislam_pose_graph_batch")
    return sims_out, cost, status


def reservePoseGraphWide(v_stride: int, e_stride: int, batch: int, *, ctx: Context | None = None):
    """Size the context's workspace for poseGraphWideBatch calls of up to this shape and batch
    (pislam_pose_graph_wide_reserve): afterwards such calls allocate nothing and never synchronise, so they can be
    captured into a hipGraph.  The workspace is per graph: 944 bytes per vertex and 336 per edge of the strides."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_pose_graph_wide_reserve(ctx.h, int(v_stride), int(e_stride), int(batch)),
              "pislam_pose_graph_wide_reserve")


def poseGraphWideBatch(sims, v_counts, fixed, edges, meas, weight, e_counts, inc_ptr, inc, *, iters=20, cg_iters=256,
                       cg_tol=1e-6, eps=1e-9, sims_out=None, cost=None, status=None, work=None,
                       ctx: Context | None = None):
    """poseGraphBatch for large graphs (pislam_pose_graph_wide_batch): the same arguments, keywords, defaults and
    checks, the same outputs bit for bit, but every phase of the optimisation is one launch over all edges or vertices of
    all graphs, so one large graph uses the whole device, and the limits are 65536 vertices and 2^20 edges per graph
    (essentialGraph(..., wide=True)).  Returns (sims_out, cost, status, work); work int32 [batch][2] = the solves
    attempted and the conjugate-gradient iterations made.  The call issues 5 + iters * (5 + 6 * cg_iters) launches
    whatever the graphs need, so iters * cg_iters is paid in launches: prefer poseGraphBatch for batches of many small
    graphs.  Asynchronous on the ctx stream; capturable after reservePoseGraphWide."""
    import torch
    ctx = ctx or default_context()
    batch, V, E = _pose_graph_shape(sims, edges)
    if V > POSE_GRAPH_WIDE_MAX_VERTICES or E > POSE_GRAPH_WIDE_MAX_EDGES:
        raise ValueError(f"at most {POSE_GRAPH_WIDE_MAX_VERTICES} vertices and {POSE_GRAPH_WIDE_MAX_EDGES} edges per graph")
    _pose_graph_rest(batch, V, E, sims, v_counts, fixed, edges, meas, weight, e_counts, inc_ptr, inc)
    p = capi.PoseGraphParams(int(iters), int(cg_iters), float(cg_tol), float(eps))
    dev = sims.device
    sims_out = torch.empty_like(sims) if sims_out is None else sims_out
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    work = torch.empty((batch, 2), dtype=torch.int32, device=dev) if work is None else work
    ctx.check(ctx.lib.pislam_pose_graph_wide_batch(ctx.h, ctypes.byref(p), ptr(sims), ptr(v_counts), ptr(fixed), ptr(edges),
                                                   ptr(meas), ptr(weight), ptr(e_counts), ptr(inc_ptr), ptr(inc), V, E,
                                                   batch, ptr(sims_out), ptr(cost), ptr(status), ptr(work)),
              "pislam_pose_graph_wide_batch")
    return sims_out, cost, status, work


def correctMapPointsBatch(xw, ref, pt_counts, sims_old, sims_new, v_counts, *, xw_out=None, status=None,
                          ctx: Context | None = None):
    """Map points moved with their reference key frames after a loop correction (pislam_map_points_correct_batch, the end
    of LoopClosing::CorrectLoop): point p becomes S_new[ref[p]]^-1(S_old[ref[p]](X_p)), computed in binary64.  xw float32
    [batch][pt_stride][3], ref int16 or uint16 [batch][pt_stride] (the uint16 words of the call), pt_counts [batch],
    sims_old and sims_new float32 [batch][v_stride][13] (poseGraphBatch's input and output), v_counts [batch].  Returns
    (xw_out, status uint8 [batch][pt_stride]: 1 where ref is out of range or the result is not finite; such a point
    stays as it was).  xw_out may be `xw`.  Asynchronous on the ctx stream, no workspace: capturable as it is."""
    import torch
    ctx = ctx or default_context()
    batch, pts = _tensor(xw, torch.float32, (None, None, 3), "xw must be a float32 tensor [batch][pt_stride][3]")
    _tensor(ref, _word16(), (batch, pts), "ref must be a 16-bit integer tensor [batch][pt_stride]")
    V, = _tensor(sims_old, torch.float32, (batch, None, 13), "sims_old must be a float32 tensor [batch][v_stride][13]")
    _tensor(sims_new, torch.float32, (batch, V, 13), "sims_new must be a float32 tensor of sims_old's shape")
    _counts("pt_counts and v_counts must be 32-bit integer tensors [batch]", batch, pt_counts, v_counts)
    _contiguous(xw, ref, pt_counts, sims_old, sims_new, v_counts)
    xw_out = torch.empty_like(xw) if xw_out is None else xw_out
    status = torch.empty((batch, pts), dtype=torch.uint8, device=xw.device) if status is None else status
    ctx.check(ctx.lib.pislam_map_points_correct_batch(ctx.h, ptr(xw), ptr(ref), ptr(pt_counts), ptr(sims_old),
                                                      ptr(sims_new), ptr(v_counts), pts, V, batch,
                                                      ptr(xw_out), ptr(status)), "pislam_map_points_correct_batch")
    return xw_out, status


# ---- the covisibility graph: weights, ordered neighbours, spanning tree, culling statistic ----------
COVIS_MAX_KF = 4096         # == POSE_GRAPH_MAX_VERTICES: a map that fits covisibilityBatch fits poseGraphBatch in its
                            # vertices; its essential graph may have more than 16384 edges: poseGraphWideBatch


def mapObservations(obs_kf, obs_pt, counts, *more):
    """The observations of covisibilityBatch from per-observation lists in any order: obs_kf and obs_pt are integer
    tensors [batch][stride] (key frame of the map, point of the map), counts [batch].  The first counts[b] entries of a row
    are sorted by point and by key frame within a point (a stable sort of the key obs_pt * 65536 + obs_kf; the call
    itself refuses a map in which a pair occurs twice, a negative point or a key frame beyond the map's); the entries
    behind them stay behind.  Every further tensor [batch][stride] or [batch][stride][..] passed (obs_level, cull_mask,
    keypoint words) is sorted alike and keeps its dtype.  Returns (obs_kf int16 [batch][stride] (the uint16 words of the
    call: a key frame index is below 4096), obs_pt int32 [batch][stride], counts int32 [batch] clamped to [0, stride],
    *more).  Torch ops on the current torch stream."""
    import torch
    if obs_kf.dim() != 2 or tuple(obs_pt.shape) != tuple(obs_kf.shape):
        raise ValueError("obs_kf and obs_pt must be [batch][stride]")
    batch, stride = (int(v) for v in obs_kf.shape)
    if tuple(counts.shape) != (batch,):
        raise ValueError("counts must be [batch]")
    for t in more:
        if t.dim() < 2 or tuple(t.shape[:2]) != (batch, stride):
            raise ValueError("every further tensor must be [batch][stride] or [batch][stride][..]")
    k, p = obs_kf.to(torch.int64) & 0xFFFF, obs_pt.to(torch.int64)
    n = counts.to(torch.int64).clamp(0, stride)
    live = torch.arange(stride, device=k.device)[None, :] < n[:, None]
    key = torch.where(live, p * 65536 + k, torch.full_like(k, 1 << 62))
    order = torch.argsort(key, dim=1, stable=True)

    def g(t):
        o = order.reshape(order.shape + (1,) * (t.dim() - 2)).expand(t.shape)
        return torch.gather(t, 1, o).contiguous()
    return (((g(k) ^ 0x8000) - 0x8000).to(torch.int16), g(p).to(torch.int32), n.to(torch.int32)) + tuple(g(t) for t in more)


def reserveCovisibility(kf_stride: int, stride: int, batch: int, *, ctx: Context | None = None):
    """Size the context's workspace for covisibilityBatch calls of up to this shape (pislam_covisibility_reserve; 4 *
    batch * (kf_stride^2 + 2 * kf_stride + 1) bytes): afterwards such calls allocate nothing and never synchronise, so
    they can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_covisibility_reserve(ctx.h, int(kf_stride), int(stride), int(batch)), "pislam_covisibility_reserve")


def covisibilityBatch(obs_kf, obs_pt, counts, kf_counts, *, obs_level=None, cull_mask=None, kf_stride=None, nb_stride=None,
                      min_weight=15, cull_min_observers=3, cull_level_slack=1, nb_idx=None, nb_weight=None, nb_count=None,
                      parent=None, kf_points=None, kf_redundant=None, status=None, ctx: Context | None = None):
    """Batched covisibility graph (pislam_covisibility_batch; the contract is the comment in include/pislam_hip.h),
    ORB-SLAM's KeyFrame::UpdateConnections for every key frame of a map at once, with the spanning tree and the statistic
    of KeyFrameCulling.  Per map: obs_kf int16 or uint16 and obs_pt 32-bit integers [batch][stride], the first counts[b]
    entries strictly ascending in (obs_pt, obs_kf) (mapObservations makes them); counts and kf_counts [batch]; obs_level
    and cull_mask uint8 [batch][stride] or None (all levels zero; every observation counts in the statistic of its key
    frame).  kf_stride (<= 4096) is the key-frame extent of the outputs: given, or that of nb_count when it is passed;
    nb_stride (1..kf_stride) the neighbours kept per key frame: given, or that of nb_idx when it is passed, or kf_stride
    (nothing is truncated; the two neighbour tensors then take 6 * kf_stride^2 bytes per map).  Key frame j qualifies for
    i with at least min_weight shared points; if nobody does, the best one.  Returns (nb_idx int16 and nb_weight int32
    [batch][kf_stride][nb_stride]: the neighbours by weight descending, index ascending on a tie, written up to
    min(nb_count, nb_stride); nb_count int32 [batch][kf_stride]; parent int16 [batch][kf_stride] (the uint16 words of the
    call: -1 is 0xFFFF, no parent); kf_points and kf_redundant int32 [batch][kf_stride] (a key frame is redundant by
    ORB-SLAM's rule when kf_redundant > 0.9 * kf_points); status int32 [batch]: 0 ok, 1 nothing to do, 3 malformed).
    Numpy inputs go to the current device.  Integer counting: exact, and the same inputs give the same outputs bit for
    bit.  Asynchronous on the ctx stream; capturable after reserveCovisibility."""
    import torch
    ctx = ctx or default_context()
    obs_kf, obs_pt, counts, kf_counts, obs_level, cull_mask = (_on_device(a) for a in (obs_kf, obs_pt, counts, kf_counts,
                                                                                       obs_level, cull_mask))
    batch, stride = _tensor(obs_pt, _word32(), (None, None), "obs_pt must be a 32-bit integer tensor [batch][stride]")
    _tensor(obs_kf, _word16(), (batch, stride), "obs_kf must be a 16-bit integer tensor [batch][stride]")
    _counts("counts and kf_counts must be 32-bit integer tensors [batch]", batch, counts, kf_counts)
    for t, message in ((obs_level, "obs_level must be a uint8 tensor [batch][stride]"),
                       (cull_mask, "cull_mask must be a uint8 tensor [batch][stride]")):
        if t is not None:
            _tensor(t, torch.uint8, (batch, stride), message)
    if kf_stride is None:
        if nb_count is None or nb_count.dim() != 2:
            raise ValueError("kf_stride is needed, or the output nb_count [batch][kf_stride] to take it from")
        kf_stride = int(nb_count.shape[1])
    kf_stride = int(kf_stride)
    if not 1 <= kf_stride <= COVIS_MAX_KF:
        raise ValueError(f"kf_stride must be 1..{COVIS_MAX_KF}")
    if nb_stride is None:
        nb_stride = int(nb_idx.shape[2]) if nb_idx is not None and nb_idx.dim() == 3 else kf_stride
    nb_stride = int(nb_stride)
    if not 1 <= nb_stride <= kf_stride:
        raise ValueError("nb_stride must be 1..kf_stride")
    if int(min_weight) < 1 or int(cull_min_observers) < 1 or not 0 <= int(cull_level_slack) <= 255:
        raise ValueError("min_weight and cull_min_observers must be >= 1 and cull_level_slack 0..255")
    dev = obs_pt.device
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    nb_idx = new(torch.int16, batch, kf_stride, nb_stride) if nb_idx is None else nb_idx
    nb_weight = new(torch.int32, batch, kf_stride, nb_stride) if nb_weight is None else nb_weight
    nb_count = new(torch.int32, batch, kf_stride) if nb_count is None else nb_count
    parent = new(torch.int16, batch, kf_stride) if parent is None else parent
    kf_points = new(torch.int32, batch, kf_stride) if kf_points is None else kf_points
    kf_redundant = new(torch.int32, batch, kf_stride) if kf_redundant is None else kf_redundant
    status = new(torch.int32, batch) if status is None else status
    _tensor(nb_idx, _word16(), (batch, kf_stride, nb_stride), "nb_idx must be a 16-bit integer tensor [batch][kf_stride][nb_stride]")
    _tensor(nb_weight, _word32(), (batch, kf_stride, nb_stride),
            "nb_weight must be a 32-bit integer tensor [batch][kf_stride][nb_stride]")
    _tensor(parent, _word16(), (batch, kf_stride), "parent must be a 16-bit integer tensor [batch][kf_stride]")
    for t in (nb_count, kf_points, kf_redundant):
        _tensor(t, _word32(), (batch, kf_stride), "nb_count, kf_points and kf_redundant must be 32-bit integer tensors "
                                                  "[batch][kf_stride]")
    _counts("status must be a 32-bit integer tensor [batch]", batch, status)
    _contiguous(obs_kf, obs_pt, counts, kf_counts, obs_level, cull_mask)
    _contiguous(nb_idx, nb_weight, nb_count, parent, kf_points, kf_redundant, status, message="outputs must be contiguous")
    p = capi.CovisParams(int(min_weight), int(cull_min_observers), int(cull_level_slack))
    ctx.check(ctx.lib.pislam_covisibility_batch(ctx.h, ctypes.byref(p), ptr(obs_kf), ptr(obs_pt), ptr(counts), ptr(kf_counts),
                                                ptr(obs_level), ptr(cull_mask), kf_stride, stride, nb_stride, batch,
                                                ptr(nb_idx), ptr(nb_weight), ptr(nb_count), ptr(parent), ptr(kf_points),
                                                ptr(kf_redundant), ptr(status)), "pislam_covisibility_batch")
    return nb_idx, nb_weight, nb_count, parent, kf_points, kf_redundant, status


def essentialPairs(nb_idx, nb_weight, nb_count, parent, kf_counts, min_weight=100):
    """The `pairs` of essentialGraph from covisibilityBatch's outputs: a list with one integer tensor [ne][2] per map.
    First the spanning-tree edges (parent[k], k) in ascending k; behind them the covisibility links with nb_weight >=
    min_weight (ORB-SLAM: 100) as (i, j), i < j, in ascending order, each once, without those that are tree edges
    already.  The caller appends the loop edges behind them and passes their measurements as essentialGraph's `meas`.
    Only key frames below kf_counts[b] are looked at.  Raises ValueError if a row was truncated (nb_count > nb_stride)
    and its last written weight still reaches min_weight: a strong link may then be missing (a row is ordered by weight,
    so a truncated row whose last weight is below min_weight hides none).  Reads sizes on the host, as essentialGraph
    does (this synchronises); torch ops on the current torch stream."""
    import torch
    if nb_idx.dim() != 3 or tuple(nb_weight.shape) != tuple(nb_idx.shape):
        raise ValueError("nb_idx and nb_weight must be [batch][kf_stride][nb_stride]")
    batch, ks, nbs = (int(v) for v in nb_idx.shape)
    if tuple(nb_count.shape) != (batch, ks) or tuple(parent.shape) != (batch, ks) or tuple(kf_counts.shape) != (batch,):
        raise ValueError("nb_count and parent must be [batch][kf_stride] and kf_counts [batch]")
    out = []
    for b, nk in enumerate(int(v) for v in kf_counts.tolist()):
        nk = min(max(nk, 0), ks)
        par = parent[b, :nk].to(torch.int64) & 0xFFFF
        kid = torch.nonzero(par != 0xFFFF)[:, 0]
        tree = torch.stack([par[kid], kid], dim=1)
        cnt = nb_count[b, :nk].to(torch.int64)
        idx, w = nb_idx[b, :nk].to(torch.int64) & 0xFFFF, nb_weight[b, :nk].to(torch.int64)
        written = torch.arange(nbs, device=idx.device)[None, :] < cnt.clamp(0, nbs)[:, None]
        if bool(((cnt > nbs) & (w[:, nbs - 1] >= int(min_weight))).any()):
            raise ValueError("a neighbour row was truncated (nb_count > nb_stride) above min_weight: a strong link may be missing")
        row, col = torch.nonzero(written & (w >= int(min_weight)), as_tuple=True)
        other = idx[row, col]
        code = torch.unique(torch.minimum(row, other) * 65536 + torch.maximum(row, other))    # (sorted ascending)
        code = code[~torch.isin(code, tree[:, 0] * 65536 + tree[:, 1])]
        links = torch.stack([code // 65536, code % 65536], dim=1)
        out.append(torch.cat([tree, links]).to(torch.int32))
    return out


# ---- the map points' summaries: normal, distance range, representative descriptor ----------
MAP_POINT_STATUS = ("ok", "no observers", "reference replaced", "geometry", "no level")


def observationDescriptors(desc, obs_kf, obs_kp, counts):
    """The obs_desc of mapPointsUpdateBatch from the key frames' own descriptor tensors: desc 32-bit words
    [batch][kf_stride][kp_stride][8] (the front end's descriptors of every key frame of the map), obs_kf integer
    [batch][stride] (mapObservations' output: 16-bit words read unsigned) and obs_kp integer [batch][stride] (the index of
    the observation's keypoint in its key frame; pass it to mapObservations as a further tensor so that it is sorted
    alike), counts [batch].  Slot i < counts[b] gets desc[b][obs_kf[b][i]][obs_kp[b][i]]; the slots at and beyond
    counts[b] may hold unwritten memory: they are masked before gathering and come out as zeros.  Returns a tensor
    [batch][stride][8] of desc's dtype.  Torch ops on the current torch stream."""
    import torch
    if desc.dim() != 4 or int(desc.shape[3]) != 8 or desc.dtype not in _word32():
        raise ValueError("desc must be a 32-bit integer tensor [batch][kf_stride][kp_stride][8]")
    batch, ks, kps = (int(v) for v in desc.shape[:3])
    if obs_kf.dim() != 2 or int(obs_kf.shape[0]) != batch or tuple(obs_kp.shape) != tuple(obs_kf.shape):
        raise ValueError("obs_kf and obs_kp must be [batch][stride]")
    if tuple(counts.shape) != (batch,):
        raise ValueError("counts must be [batch]")
    stride = int(obs_kf.shape[1])
    live = torch.arange(stride, device=obs_kf.device)[None, :] < counts.to(torch.int64)[:, None]
    zero = torch.zeros_like(live, dtype=torch.int64)
    unsigned = 0xFFFF if obs_kf.dtype in _word16() else -1
    kf = torch.where(live, obs_kf.to(torch.int64) & unsigned, zero).clamp(0, ks - 1)
    kp = torch.where(live, obs_kp.to(torch.int64), zero).clamp(0, kps - 1)
    rows = desc.reshape(batch, ks * kps, 8).view(torch.int32)
    got = torch.gather(rows, 1, (kf * kps + kp)[..., None].expand(-1, -1, 8))
    return torch.where(live[..., None], got, torch.zeros_like(got)).view(desc.dtype).contiguous()


def mapPointsUpdateBatch(obs_kf, obs_pt, counts, kf_counts, obs_level, poses, xw, pt_counts, *, obs_desc=None, ref=None,
                         level_scale=None, nlevels=8, scale=1.2, want_normal=True, want_drange=True, want_first=True,
                         normal=None, drange=None, desc=None, nobs=None, first=None, pt_status=None, status=None,
                         ctx: Context | None = None):
    """Batched refresh of the map points' summaries (pislam_map_points_update_batch; the contract is the comment in
    include/pislam_hip.h), ORB-SLAM's MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors for every point of
    a map at once: what matchProjectionBatch and matchFuseBatch read of a map point (normal, drange, qdesc) and the nobs
    of fuseDecisions, after triangulateBatch, a fusion, localBundleAdjustBatch or correctMapPointsBatch changed the map.
    Per map: obs_kf int16 or uint16 and obs_pt 32-bit integers [batch][stride], the first counts[b] entries strictly
    ascending in (obs_pt, obs_kf), and obs_level uint8 [batch][stride] (mapObservations makes all three); counts and
    kf_counts [batch]; poses float32 [batch][kf_stride][12] (R row-major, then t; Xc = R Xw + t); xw float32
    [batch][pt_stride][3]; pt_counts [batch]; obs_desc 32-bit words [batch][stride][8] or None (observationDescriptors
    makes it; None: no descriptor is chosen); ref int16 or uint16 [batch][pt_stride] or None (each point's reference key
    frame, correctMapPointsBatch's; None: the first observer).  level_scale: a HOST sequence of 1..16 float32 (default:
    mapPointLevelTables(nlevels, scale)[0]).  Returns (normal float32 [batch][pt_stride][3]: the unit mean viewing
    direction; drange float32 [batch][pt_stride][2]; desc [batch][pt_stride][8] of obs_desc's dtype, None without
    obs_desc: the observer's descriptor with the least median distance to the others; nobs int32 [batch][pt_stride];
    first int32 [batch][pt_stride]: the list index of the point's first observation or -1; pt_status uint8
    [batch][pt_stride] (MAP_POINT_STATUS names the codes); status int32 [batch]: 0 ok, 1 nothing to do, 3 malformed).
    normal, drange and first are None when not wanted and not passed.  Points at and beyond pt_counts[b] are not
    written; a point without observers keeps its normal, drange and desc.  Numpy inputs go to the current device.  The
    same inputs give the same outputs, bit for bit.  Asynchronous on the ctx stream, no workspace: capturable as it
    is."""
    import torch
    ctx = ctx or default_context()
    obs_kf, obs_pt, counts, kf_counts, obs_level, poses, xw, pt_counts, obs_desc, ref = (
        _on_device(a) for a in (obs_kf, obs_pt, counts, kf_counts, obs_level, poses, xw, pt_counts, obs_desc, ref))
    batch, stride = _tensor(obs_pt, _word32(), (None, None), "obs_pt must be a 32-bit integer tensor [batch][stride]")
    _tensor(obs_kf, _word16(), (batch, stride), "obs_kf must be a 16-bit integer tensor [batch][stride]")
    _tensor(obs_level, torch.uint8, (batch, stride), "obs_level must be a uint8 tensor [batch][stride]")
    kf_stride, = _tensor(poses, torch.float32, (batch, None, 12), "poses must be a float32 tensor [batch][kf_stride][12]")
    if not 1 <= kf_stride <= COVIS_MAX_KF:
        raise ValueError(f"kf_stride must be 1..{COVIS_MAX_KF}")
    pts, = _tensor(xw, torch.float32, (batch, None, 3), "xw must be a float32 tensor [batch][pt_stride][3]")
    _counts("counts, kf_counts and pt_counts must be 32-bit integer tensors [batch]", batch, counts, kf_counts, pt_counts)
    if obs_desc is not None:
        _tensor(obs_desc, _word32(), (batch, stride, 8), "obs_desc must be a 32-bit integer tensor [batch][stride][8]")
    if ref is not None:
        _tensor(ref, _word16(), (batch, pts), "ref must be a 16-bit integer tensor [batch][pt_stride]")
    if desc is not None and obs_desc is None:
        raise ValueError("desc needs obs_desc")
    if level_scale is None:
        level_scale = mapPointLevelTables(nlevels, scale)[0]
    tab, ntab = _float_table(level_scale, "level_scale must have 1..16 entries")
    dev = obs_pt.device
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    normal = new(torch.float32, batch, pts, 3) if normal is None and want_normal else normal
    drange = new(torch.float32, batch, pts, 2) if drange is None and want_drange else drange
    first = new(torch.int32, batch, pts) if first is None and want_first else first
    desc = new(obs_desc.dtype, batch, pts, 8) if desc is None and obs_desc is not None else desc
    nobs = new(torch.int32, batch, pts) if nobs is None else nobs
    pt_status = new(torch.uint8, batch, pts) if pt_status is None else pt_status
    status = new(torch.int32, batch) if status is None else status
    if normal is not None:
        _tensor(normal, torch.float32, (batch, pts, 3), "normal must be a float32 tensor [batch][pt_stride][3]")
    if drange is not None:
        _tensor(drange, torch.float32, (batch, pts, 2), "drange must be a float32 tensor [batch][pt_stride][2]")
    if desc is not None:
        _tensor(desc, _word32(), (batch, pts, 8), "desc must be a 32-bit integer tensor [batch][pt_stride][8]")
    for t in (nobs, first):
        if t is not None:
            _tensor(t, _word32(), (batch, pts), "nobs and first must be 32-bit integer tensors [batch][pt_stride]")
    _tensor(pt_status, torch.uint8, (batch, pts), "pt_status must be a uint8 tensor [batch][pt_stride]")
    _counts("status must be a 32-bit integer tensor [batch]", batch, status)
    _contiguous(obs_kf, obs_pt, counts, kf_counts, obs_level, poses, xw, pt_counts, obs_desc, ref)
    _contiguous(normal, drange, desc, nobs, first, pt_status, status, message="outputs must be contiguous")
    ctx.check(ctx.lib.pislam_map_points_update_batch(ctx.h, ptr(obs_kf), ptr(obs_pt), ptr(counts), ptr(kf_counts),
                                                     ptr(obs_level), ptr(obs_desc), ptr(poses), ptr(xw), ptr(pt_counts),
                                                     ptr(ref), tab, ntab, kf_stride, stride, pts, batch, ptr(normal),
                                                     ptr(drange), ptr(desc), ptr(nobs), ptr(first), ptr(pt_status),
                                                     ptr(status)), "pislam_map_points_update_batch")
    return normal, drange, desc, nobs, first, pt_status, status


# ---- global bundle adjustment of whole maps ---------------------------------
GBA_MAX_KF, GBA_MAX_POINTS, GBA_MAX_STRIDE, GBA_MAX_CG = COVIS_MAX_KF, 1 << 22, 1 << 24, 256


def keyFrameObservationIndex(obs_kf, counts, kf_stride: int):
    """The key-frame side of a map's observation list, as globalBundleAdjustBatch reads it: obs_kf integer [batch][stride]
    (mapObservations' words), counts [batch], kf_stride the key-frame extent of the map's tensors.  Returns (kf_ptr int32
    [batch][kf_stride + 1], kf_obs int32 [batch][stride]): the observations of key frame k are kf_obs[kf_ptr[k] ..
    kf_ptr[k + 1]), in ascending order (a stable sort by key frame); the key frames from the map's count on have empty
    ranges, so kf_ptr[nk] is counts[b] for every nk beyond the last key frame observed.  An observation whose key frame is
    not below kf_stride is left out (the call refuses such a map by itself).  Torch ops on the current torch stream."""
    import torch
    if obs_kf.dim() != 2 or tuple(counts.shape) != (obs_kf.shape[0],):
        raise ValueError("obs_kf must be [batch][stride] and counts [batch]")
    batch, stride = (int(v) for v in obs_kf.shape)
    kf_stride = int(kf_stride)
    if not 1 <= kf_stride <= GBA_MAX_KF:
        raise ValueError(f"kf_stride must be 1..{GBA_MAX_KF}")
    k = obs_kf.to(torch.int64) & 0xFFFF
    n = counts.to(torch.int64).clamp(0, stride)
    live = (torch.arange(stride, device=k.device)[None, :] < n[:, None]) & (k < kf_stride)
    key = torch.where(live, k, torch.full_like(k, kf_stride))
    kf_obs = torch.argsort(key, dim=1, stable=True).to(torch.int32).contiguous()
    hist = torch.zeros((batch, kf_stride + 1), dtype=torch.int64, device=k.device)
    hist.scatter_add_(1, key, torch.ones_like(key))
    kf_ptr = torch.zeros((batch, kf_stride + 1), dtype=torch.int64, device=k.device)
    kf_ptr[:, 1:] = torch.cumsum(hist[:, :kf_stride], dim=1)
    return kf_ptr.to(torch.int32).contiguous(), kf_obs


def reserveGlobalBundleAdjust(kf_stride: int, pt_stride: int, stride: int, batch: int, *, ctx: Context | None = None):
    """Size the context's workspace for globalBundleAdjustBatch calls of up to this shape (pislam_global_ba_reserve; per
    map 362 bytes per observation, 317 per point and 992 per key frame): afterwards such calls allocate nothing and never
    synchronise, so they can be captured into a hipGraph."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_global_ba_reserve(ctx.h, int(kf_stride), int(pt_stride), int(stride), int(batch)),
              "pislam_global_ba_reserve")


def globalBundleAdjustBatch(poses, cams, fixed, kf_counts, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, kf_ptr, kf_obs, *,
                            level=None, inv_sigma2=None, rounds=1, iters=(10,), huber_rounds=1, min_obs=10, eps=1e-6,
                            cg_iters=50, cg_tol=1e-4, poses_out=None, xw_out=None, inlier=None, ninliers=None, cost=None,
                            status=None, work=None, ctx: Context | None = None):
    """Batched global bundle adjustment (pislam_global_ba_batch; the contract is the comment in include/pislam_hip.h):
    per map, the poses of all key frames whose `fixed` byte is zero and all map points are moved together to minimise the
    robust reprojection error of the observations.  Levenberg on the Schur complement, solved matrix-free by block-Jacobi
    preconditioned conjugate gradients (at most cg_iters iterations of a solve, stopped at cg_tol); every phase of a map
    runs across many workgroups.  poses float32 [batch][kf_stride][12] (kf_stride <= 4096), cams float32
    [batch][kf_stride][5], fixed uint8 [batch][kf_stride], xw float32 [batch][pt_stride][3], obs_q8 int32
    [batch][stride][3]; obs_kf (16-bit words), obs_pt (32-bit words), counts and kf_counts are covisibilityBatch's and
    mapPointsUpdateBatch's observation list as it is (mapObservations makes it); kf_ptr [batch][kf_stride + 1] and kf_obs
    [batch][stride] are keyFrameObservationIndex's; pt_counts [batch]; level and inv_sigma2 as in poseRefineBatch.  The
    defaults are ORB-SLAM's schedule (one round of 10 iterations, robust; 20 at map initialisation).  Returns (poses_out,
    xw_out, inlier uint8 [batch][stride], ninliers int32 [batch], cost float64 [batch], status int32 [batch] = code |
    evaluations << 8; code 0 ok, 1 stopped for min_obs or no free key frame, 2 an input is not finite, 3 the map is
    malformed, work int32 [batch][2] = (solves begun, conjugate-gradient iterations)).  poses_out may be `poses` and
    xw_out may be `xw`.  The same inputs give the same outputs, bit for bit.  Asynchronous on the ctx stream; capturable
    after reserveGlobalBundleAdjust."""
    import torch
    ctx = ctx or default_context()
    batch, kfs = _tensor(poses, torch.float32, (None, None, 12), "poses must be a float32 tensor [batch][kf_stride][12]")
    _tensor(cams, torch.float32, (batch, kfs, 5), "cams must be a float32 tensor [batch][kf_stride][5]")
    _tensor(fixed, torch.uint8, (batch, kfs), "fixed must be a uint8 tensor [batch][kf_stride]")
    pts, = _tensor(xw, torch.float32, (batch, None, 3), "xw must be a float32 tensor [batch][pt_stride][3]")
    stride, = _tensor(obs_q8, torch.int32, (batch, None, 3), "obs_q8 must be an int32 tensor [batch][stride][3]")
    _tensor(obs_kf, _word16(), (batch, stride), "obs_kf must be a 16-bit integer tensor [batch][stride]")
    _tensor(obs_pt, _word32(), (batch, stride), "obs_pt must be a 32-bit integer tensor [batch][stride]")
    _tensor(kf_ptr, _word32(), (batch, kfs + 1), "kf_ptr must be a 32-bit integer tensor [batch][kf_stride + 1]")
    _tensor(kf_obs, _word32(), (batch, stride), "kf_obs must be a 32-bit integer tensor [batch][stride]")
    if kfs > GBA_MAX_KF or pts > GBA_MAX_POINTS or stride > GBA_MAX_STRIDE:
        raise ValueError(f"at most {GBA_MAX_KF} key frames, {GBA_MAX_POINTS} points and {GBA_MAX_STRIDE} observations per map")
    _counts("kf_counts, pt_counts and counts must be 32-bit integer tensors [batch]", batch, kf_counts, pt_counts, counts)
    tab, ntab = _level_table((level,), inv_sigma2, batch, stride, "level and inv_sigma2 go together",
                             "level must be a uint8 tensor [batch][stride]")
    _contiguous(poses, cams, fixed, kf_counts, xw, pt_counts, obs_q8, obs_kf, obs_pt, counts, kf_ptr, kf_obs, level)
    its = [int(v) for v in (iters if hasattr(iters, "__len__") else [iters] * int(rounds))]
    if len(its) < int(rounds) or len(its) > 4:
        raise ValueError("iters needs an entry per round, at most 4")
    if not 1 <= int(cg_iters) <= GBA_MAX_CG or not 0.0 <= float(cg_tol) < 1.0:
        raise ValueError(f"cg_iters must be 1..{GBA_MAX_CG} and cg_tol in [0, 1)")
    p = capi.GbaParams(capi.BaParams(int(rounds), (ctypes.c_int32 * 4)(*(its + [1] * (4 - len(its)))), int(huber_rounds),
                                     int(min_obs), float(eps)), int(cg_iters), float(cg_tol))
    dev = poses.device
    poses_out = torch.empty_like(poses) if poses_out is None else poses_out
    xw_out = torch.empty_like(xw) if xw_out is None else xw_out
    inlier = torch.empty((batch, stride), dtype=torch.uint8, device=dev) if inlier is None else inlier
    ninliers = torch.empty((batch,), dtype=torch.int32, device=dev) if ninliers is None else ninliers
    cost = torch.empty((batch,), dtype=torch.float64, device=dev) if cost is None else cost
    status = torch.empty((batch,), dtype=torch.int32, device=dev) if status is None else status
    work = torch.empty((batch, 2), dtype=torch.int32, device=dev) if work is None else work
    ctx.check(ctx.lib.pislam_global_ba_batch(ctx.h, ctypes.byref(p), ptr(poses), ptr(cams), ptr(fixed), ptr(kf_counts),
                                             ptr(xw), ptr(pt_counts), ptr(obs_q8), ptr(obs_kf), ptr(obs_pt), ptr(level),
                                             ptr(counts), ptr(kf_ptr), ptr(kf_obs), tab, ntab, kfs, pts, stride, batch,
                                             ptr(poses_out), ptr(xw_out), ptr(inlier), ptr(ninliers), ptr(cost),
                                             ptr(status), ptr(work)), "pislam_global_ba_batch")
    return poses_out, xw_out, inlier, ninliers, cost, status, work


# ---- bag of words: integer weights and the key-frame database ----------
BOW_MAX_STRIDE = 16384      # entries of a bag-of-words vector (pislam_bow_vector_batch)


def _check_bow_rows(what, word, other, n):
    """[batch][stride] word / weight tensors and their [batch] counts: returns (batch, stride)."""
    if word.ndim != 2:
        raise ValueError(f"{what}: words must be [batch][stride]")
    batch, stride = (int(v) for v in word.shape)
    if stride > BOW_MAX_STRIDE:
        raise ValueError(f"{what}: stride must be at most {BOW_MAX_STRIDE}")
    if tuple(other.shape) != (batch, stride):
        raise ValueError(f"{what}: words and weights must have the same [batch][stride] shape")
    if tuple(n.shape) != (batch,):
        raise ValueError(f"{what}: one count per frame ({batch})")
    return batch, stride


def bowWeightBatch(bow_word, bow_tf, bow_n, idf=None, nwords: int | None = None, bow_weight=None, *,
                   ctx: Context | None = None):
    """Q24 integer tf-idf weights of bag-of-words vectors (pislam_bow_weight_batch): bow_weight[b][k] =
    (tf * idf << 24) / (the frame's sum of tf * idf), floored; idf is a device int32 tensor [nwords] (values above
    65535 count as 65535) or None (= 1 for every word, then `nwords` must be given).  Returns bow_weight int32
    [batch][stride]; slots at and beyond bow_n[b] are not written.  Asynchronous on the ctx stream."""
    batch, stride = _check_bow_rows("bowWeightBatch", bow_word, bow_tf, bow_n)
    if idf is not None:
        if idf.ndim != 1:
            raise ValueError("bowWeightBatch: idf must be [nwords]")
        if nwords is None:
            nwords = int(idf.shape[0])
        elif int(nwords) > int(idf.shape[0]):
            raise ValueError("bowWeightBatch: nwords exceeds the idf table")
    elif nwords is None:
        raise ValueError("bowWeightBatch: nwords is needed without an idf table")
    if not 1 <= int(nwords) <= 1 << 24:
        raise ValueError("bowWeightBatch: nwords must be 1..2^24")
    if bow_weight is not None and tuple(bow_weight.shape) != (batch, stride):
        raise ValueError("bowWeightBatch: bow_weight must be [batch][stride] like the words")
    import torch
    ctx = ctx or default_context()
    if bow_weight is None:
        bow_weight = torch.empty((batch, stride), dtype=torch.int32, device=bow_word.device)
    ctx.check(ctx.lib.pislam_bow_weight_batch(ctx.h, ptr(bow_word), ptr(bow_tf), ptr(bow_n), stride, batch, ptr(idf),
                                              int(nwords), ptr(bow_weight)), "pislam_bow_weight_batch")
    return bow_weight


class BowDatabase:
    """pislam_bowdb: up to `capacity` key frames of at most `stride` (word, weight) entries over `nwords` words, with an
    inverted file on the device.  add() takes what bowVectorBatch / bowWeightBatch wrote and returns the first new id;
    query() returns, per query vector, the `topk` key frames with the largest integer L1 score among those that share
    at least min_common_pct % of the best key frame's common words (include/pislam_hip.h).  Shapes and ranges are checked
    here, before the library is touched."""

    def __init__(self, nwords: int, stride: int, capacity: int, *, ctx: Context | None = None):
        self.h = None
        nwords, stride, capacity = int(nwords), int(stride), int(capacity)
        if not 1 <= nwords <= 1 << 24:
            raise ValueError("nwords must be 1..2^24")
        if not 1 <= stride <= BOW_MAX_STRIDE:
            raise ValueError(f"stride must be 1..{BOW_MAX_STRIDE}")
        if not 1 <= capacity <= 1 << 20:
            raise ValueError("capacity must be 1..2^20")
        if stride * capacity > 1 << 31:
            raise ValueError("capacity * stride must be at most 2^31")
        self.nwords, self.stride, self.capacity = nwords, stride, capacity
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.pislam_bowdb_create(self.ctx.h, nwords, stride, capacity, ctypes.byref(h)),
                       "pislam_bowdb_create")
        self.h = h

    @property
    def size(self) -> int:
        """Ids handed out so far (removed ones included)."""
        return int(self.ctx.lib.pislam_bowdb_size(self.h))

    def add(self, bow_word, bow_weight, bow_n) -> int:
        """Adds the frames of [batch][stride] device tensors as key frames size .. size + batch - 1; returns the first id."""
        batch, stride = _check_bow_rows("BowDatabase.add", bow_word, bow_weight, bow_n)
        first = ctypes.c_int32(-1)
        self.ctx.check(self.ctx.lib.pislam_bowdb_add_batch(self.ctx.h, self.h, ptr(bow_word), ptr(bow_weight), ptr(bow_n),
                                                           stride, batch, ctypes.byref(first)), "pislam_bowdb_add_batch")
        return int(first.value)

    def remove(self, ids):
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(ids)), np.int32)
        if ids.ndim != 1:
            raise ValueError("BowDatabase.remove: ids must be a list of key-frame ids")
        self.ctx.check(self.ctx.lib.pislam_bowdb_remove(self.ctx.h, self.h, ptr(ids), len(ids)), "pislam_bowdb_remove")

    def clear(self):
        self.ctx.check(self.ctx.lib.pislam_bowdb_clear(self.ctx.h, self.h), "pislam_bowdb_clear")

    def reserve_query(self, batch: int, topk: int):
        """Sizes the context's query workspace: afterwards query() of the same or a smaller shape allocates nothing and
        can be captured into a hipGraph."""
        if not 0 <= int(batch) <= 65535:
            raise ValueError("batch must be 0..65535")
        if not 1 <= int(topk) <= 64:
            raise ValueError("topk must be 1..64")
        self.ctx.check(self.ctx.lib.pislam_bowdb_query_reserve(self.ctx.h, self.h, int(batch), int(topk)),
                       "pislam_bowdb_query_reserve")

    def query(self, q_word, q_weight, q_n, topk: int = 16, min_common_pct: int = 80, id_limit=None, top_id=None,
              top_score=None, top_common=None, max_common=None):
        """Returns (top_id, top_score, top_common int32 [batch][topk], max_common int32 [batch]); rows with fewer than
        topk candidates end in -1 / 0 / 0.  id_limit: device int32 [batch] (key frames at or above it are not eligible)
        or None.  Asynchronous on the ctx stream."""
        batch, stride = _check_bow_rows("BowDatabase.query", q_word, q_weight, q_n)
        topk, min_common_pct = int(topk), int(min_common_pct)
        if not 1 <= topk <= 64:
            raise ValueError("topk must be 1..64")
        if not 0 <= min_common_pct <= 100:
            raise ValueError("min_common_pct must be 0..100")
        if id_limit is not None and tuple(id_limit.shape) != (batch,):
            raise ValueError(f"BowDatabase.query: one id_limit per query ({batch})")
        for t, shape in ((top_id, (batch, topk)), (top_score, (batch, topk)), (top_common, (batch, topk)),
                         (max_common, (batch,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError("BowDatabase.query: outputs must be [batch][topk] and max_common [batch]")
        import torch
        new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=q_word.device)
        top_id = new(batch, topk) if top_id is None else top_id
        top_score = new(batch, topk) if top_score is None else top_score
        top_common = new(batch, topk) if top_common is None else top_common
        max_common = new(batch) if max_common is None else max_common
        self.ctx.check(self.ctx.lib.pislam_bowdb_query_batch(self.ctx.h, self.h, ptr(q_word), ptr(q_weight), ptr(q_n), stride,
                                                             batch, ptr(id_limit), min_common_pct, topk, ptr(top_id),
                                                             ptr(top_score), ptr(top_common), ptr(max_common)),
                       "pislam_bowdb_query_batch")
        return top_id, top_score, top_common, max_common

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pislam_bowdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Gaussian.h:48, Bilinear.h:42, Bilinear.h:165 -------------------------------------
def gaussian5x5(width, height, img, out, *, ctx: Context | None = None):
    """pislam::gaussian5x5<vstep>(width, height, img, out); img may be out (in place)."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_gaussian5x5(ctx.h, _vstep(img), width, height, ptr(img), ptr(out)), "pislam_gaussian5x5")


def bilinear7_8(width, height, img, out, *, ctx: Context | None = None):
    """pislam::bilinear7_8<vstep>(width, height, img, out)."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_bilinear7_8(ctx.h, _vstep(img), width, height, ptr(img), ptr(out)), "pislam_bilinear7_8")


def bilinear13_16(width, height, img, out, *, ctx: Context | None = None):
    """pislam::bilinear13_16<vstep>(width, height, img, out)."""
    ctx = ctx or default_context()
    ctx.check(ctx.lib.pislam_bilinear13_16(ctx.h, _vstep(img), width, height, ptr(img), ptr(out)),
              "pislam_bilinear13_16")


# ---- lens undistortion / stereo rectification: the mesh warp in front of the pyramid build ---------
def warpMeshDims(width: int, height: int, log_cell: int):
    """(mesh_w, mesh_h) of a warp mesh (pislam_warp_mesh_dims): ((width - 1) >> log_cell) + 2, likewise the height."""
    mw, mh = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = capi.load().pislam_warp_mesh_dims(int(width), int(height), int(log_cell), ctypes.byref(mw), ctypes.byref(mh))
    if rc != 0:
        raise capi.PislamError(f"pislam_warp_mesh_dims failed ({rc}): need 1 <= width, height <= 4096, 0 <= log_cell <= 6")
    return mw.value, mh.value


class Warp:
    """pislam_warp: an immutable mesh of Q8 source coordinates (mesh_x, mesh_y int32 [mesh_h][mesh_w], host; node
    (j, i) = where output pixel (i << log_cell, j << log_cell) comes from, 256 = one source pixel) through which
    batches of device-resident frames uint8 [batch][src_height][src_width] are resampled bilinearly into frames
    [batch][height][width] (include/pislam_hip.h).  Source pixels outside the frame read as `border`.  Shapes are
    checked here, values by the library."""

    def __init__(self, mesh_x, mesh_y, width: int, height: int, src_width: int, src_height: int, log_cell: int,
                 border: int = 0, ctx: Context | None = None):
        self.h = None
        self.ctx = ctx or default_context()
        mesh_x = np.ascontiguousarray(mesh_x, np.int32)
        mesh_y = np.ascontiguousarray(mesh_y, np.int32)
        mw, mh = warpMeshDims(width, height, log_cell)
        if mesh_x.shape != (mh, mw) or mesh_y.shape != (mh, mw):
            raise ValueError(f"mesh_x and mesh_y must be [{mh}][{mw}] for a {width} x {height} output at log_cell {log_cell}")
        self.width, self.height, self.src_width, self.src_height = int(width), int(height), int(src_width), int(src_height)
        self.log_cell, self.border = int(log_cell), int(border)
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.pislam_warp_create(self.ctx.h, self.width, self.height, self.src_width, self.src_height,
                                                       self.log_cell, ptr(mesh_x), ptr(mesh_y), self.border,
                                                       ctypes.byref(h)), "pislam_warp_create")
        self.h = h

    @classmethod
    def from_calibration(cls, K, dist, size, *, R=None, P=None, src_size=None, log_cell: int = 3, border: int = 0,
                         ctx: Context | None = None):
        """The warp that undistorts (and, with R and P, rectifies) a camera: rectify.rectify_mesh after OpenCV's
        initUndistortRectifyMap.  size = (width, height) of the output, src_size of the camera frames (default: size).
        log_cell 3 keeps the interpolated coordinate within 0.03 px of the model for a EuRoC-like lens."""
        from . import rectify
        mx, my = rectify.rectify_mesh(K, dist, R, P, size, log_cell)
        sw, sh = src_size if src_size is not None else size
        return cls(mx, my, size[0], size[1], sw, sh, log_cell, border, ctx)

    def info(self) -> dict:
        v = (ctypes.c_int32 * 4)()
        self.ctx.check(self.ctx.lib.pislam_warp_info(self.h, ctypes.byref(v)), "pislam_warp_info")
        return {"tiles": int(v[0]), "staged": int(v[1]), "direct": int(v[2]), "lds_bytes": int(v[3])}

    def __call__(self, frames, out=None, *, ctx: Context | None = None):
        """frames: uint8 device tensor [batch][src_height][>= src_width] (a view with padded rows or frames is fine as
        long as bytes of a row are adjacent); out: likewise [batch][height][>= width], allocated when None.
        Asynchronous on the stream of `ctx` (default: the warp's context); returns out."""
        import torch
        c = ctx or self.ctx
        if frames.dtype != torch.uint8 or frames.dim() != 3 or frames.shape[1] != self.src_height \
                or frames.shape[2] < self.src_width or (frames.shape[2] > 1 and frames.stride(2) != 1):
            raise ValueError(f"frames must be uint8 [batch][{self.src_height}][>= {self.src_width}] with adjacent row bytes")
        batch = int(frames.shape[0])
        if out is None:
            out = torch.empty((batch, self.height, self.width), dtype=torch.uint8, device=frames.device)
        if out.dtype != torch.uint8 or out.dim() != 3 or out.shape[0] != batch or out.shape[1] != self.height \
                or out.shape[2] < self.width or (out.shape[2] > 1 and out.stride(2) != 1):
            raise ValueError(f"out must be uint8 [{batch}][{self.height}][>= {self.width}] with adjacent row bytes")
        c.check(c.lib.pislam_warp_batch(c.h, self.h, frames.data_ptr(), int(frames.stride(1)), int(frames.stride(0)),
                                        out.data_ptr(), int(out.stride(1)), int(out.stride(0)), batch),
                "pislam_warp_batch")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.pislam_warp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- contrast-limited adaptive histogram equalisation: between the warp and the pyramid build ------
class Clahe:
    """pislam_clahe_*: CLAHE of batches of device-resident frames uint8 [batch][height][width], after OpenCV's
    createCLAHE(clip_q8 / 256, tiles) but stated in integers (include/pislam_hip.h).  The defaults are ORB-SLAM3's
    (8 x 8 tiles, clip limit 3.0).  The tables are a caller-visible device tensor uint8
    [batch][tiles_y][tiles_x][256]; there is no workspace, so every call can be captured into a graph.  Shapes are
    checked here, values by the library."""

    def __init__(self, width: int, height: int, tiles=(8, 8), clip_q8: int = 768, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.width, self.height, self.tiles, self.clip_q8 = int(width), int(height), (int(tiles[0]), int(tiles[1])), int(clip_q8)
        self.params = ClaheParams(self.width, self.height, self.tiles[0], self.tiles[1], self.clip_q8)
        self.lut_size = int(self.ctx.lib.pislam_clahe_lut_size(ctypes.byref(self.params)))
        if self.lut_size == 0:
            raise capi.PislamError("pislam_clahe_lut_size: need 1 <= width, height <= 4096, 1 <= tiles <= min(32, size) per axis, "
                                   "a tile of at most 2^20 pixels and 0 <= clip_q8 <= 65535")
        self.last_luts = None

    def _frames(self, t, name, batch=None):
        import torch
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[1] != self.height or t.shape[2] < self.width \
                or (t.shape[2] > 1 and t.stride(2) != 1) or (batch is not None and t.shape[0] != batch):
            raise ValueError(f"{name} must be uint8 [{'batch' if batch is None else batch}][{self.height}][>= {self.width}] "
                             "with adjacent row bytes")
        return int(t.shape[0])

    def _luts(self, luts, batch, device):
        import torch
        shape = (batch, self.tiles[1], self.tiles[0], 256)
        if luts is None:
            return torch.empty(shape, dtype=torch.uint8, device=device)
        if luts.dtype != torch.uint8 or tuple(luts.shape) != shape or not luts.is_contiguous():
            raise ValueError(f"luts must be a contiguous uint8 tensor {list(shape)}")
        return luts

    def luts(self, frames, out=None, *, ctx: Context | None = None):
        """The tables of `frames` (pislam_clahe_luts_batch): uint8 [batch][tiles_y][tiles_x][256], allocated when
        `out` is None.  Asynchronous on the stream of `ctx` (default: this object's context)."""
        c = ctx or self.ctx
        batch = self._frames(frames, "frames")
        out = self._luts(out, batch, frames.device)
        c.check(c.lib.pislam_clahe_luts_batch(c.h, ctypes.byref(self.params), frames.data_ptr(), int(frames.stride(1)),
                                              int(frames.stride(0)), batch, out.data_ptr()), "pislam_clahe_luts_batch")
        return out

    def apply(self, frames, luts, out=None, *, ctx: Context | None = None):
        """Blends the given tables into `out` (pislam_clahe_apply_batch; allocated when None, may be `frames` itself)."""
        import torch
        c = ctx or self.ctx
        batch = self._frames(frames, "frames")
        luts = self._luts(luts, batch, frames.device)
        if out is None:
            out = torch.empty((batch, self.height, self.width), dtype=torch.uint8, device=frames.device)
        self._frames(out, "out", batch)
        c.check(c.lib.pislam_clahe_apply_batch(c.h, ctypes.byref(self.params), frames.data_ptr(), int(frames.stride(1)),
                                               int(frames.stride(0)), luts.data_ptr(), out.data_ptr(), int(out.stride(1)),
                                               int(out.stride(0)), batch), "pislam_clahe_apply_batch")
        return out

    def __call__(self, frames, out=None, luts=None, *, ctx: Context | None = None):
        """frames: uint8 device tensor [batch][height][>= width] (a view with padded rows or frames is fine as long as
        bytes of a row are adjacent); out: likewise, allocated when None, may be `frames` itself (in place); luts:
        the table tensor, allocated when None and kept as `last_luts` either way.  pislam_clahe_batch: tables, then
        blend, asynchronous on the stream of `ctx` (default: this object's context); returns out."""
        import torch
        c = ctx or self.ctx
        batch = self._frames(frames, "frames")
        luts = self._luts(luts, batch, frames.device)
        if out is None:
            out = torch.empty((batch, self.height, self.width), dtype=torch.uint8, device=frames.device)
        self._frames(out, "out", batch)
        c.check(c.lib.pislam_clahe_batch(c.h, ctypes.byref(self.params), frames.data_ptr(), int(frames.stride(1)),
                                         int(frames.stride(0)), out.data_ptr(), int(out.stride(1)), int(out.stride(0)), batch,
                                         luts.data_ptr()), "pislam_clahe_batch")
        self.last_luts = luts
        return out


# ---- on-GPU pyramid build (BASELINE config 5) ------------------------------------------
DEFAULT_CHAIN = (2, 1, 2, 2, 1, 2, 2)     # 13/16, 7/8, 13/16, ... : (13/16)^2 * 7/8 = 0.578 ~ 1.2^-3


class PyramidBuilder:
    """frames uint8 [batch][h][w] (device) -> stacked pyramids uint8 [batch][rows][vstep] (device):
    level 0 = gaussian5x5(frame), level k+1 = bilinear13_16 / bilinear7_8 of level k.

    Always the contiguous layout: frame_vstep = width, frame_stride = height * width, the layout's own vstep and
    pyramid_stride = rows * vstep, at the tensors' own (aligned) addresses.  pislam_pyramid_build_batch itself takes padded
    rows, gaps and unaligned bases (include/pislam_hip.h; tests/test_build_layouts.py calls it that way through ctypes)."""

    def __init__(self, width: int, height: int, steps=DEFAULT_CHAIN, *, blur=True, vstep_min=0,
                 ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.nlevels = len(steps) + 1
        self.steps = (ctypes.c_int32 * max(1, len(steps)))(*steps)
        self.levels_c = (Level * self.nlevels)()
        vs, rows = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = self.ctx.lib.pislam_pyramid_layout(width, height, self.nlevels, self.steps, vstep_min, self.levels_c,
                                                ctypes.byref(vs), ctypes.byref(rows))
        if rc != 0:
            raise capi.PislamError(f"pislam_pyramid_layout failed ({rc})")
        self.vstep, self.rows, self.blur = vs.value, rows.value, bool(blur)
        self.levels = [(l.width, l.height, l.row0, l.col0) for l in self.levels_c]

    def __call__(self, frames, pyramids, margins_clean: bool = False):
        """margins_clean: the caller vouches that `pyramids` was last filled by this builder with this layout and
        not written to since (PISLAM_BUILD_MARGINS_CLEAN) — the zero margins are then not re-established."""
        c = self.ctx
        batch = int(frames.shape[0])
        flags = (1 if self.blur else 0) | (2 if margins_clean else 0)
        c.check(c.lib.pislam_pyramid_build_batch(c.h, self.nlevels, self.steps, self.levels_c, ptr(frames),
                                                 int(frames.shape[2]), int(frames.shape[1]) * int(frames.shape[2]),
                                                 batch, ptr(pyramids), self.vstep, self.rows, self.rows * self.vstep,
                                                 flags), "pislam_pyramid_build_batch")


# ---- the measured path ---------------------------------------------------------
class OrbFrontend:
    """Batch of device-resident stacked pyramids -> keypoints + descriptors + counts.

    Runs the call sequence of reference demo/demo.cpp:77-101 for every pyramid on the
    GPU (pislam_orb_frontend_batch).  All tensors are torch device tensors."""

    def __init__(self, levels, vstep: int, rows: int, *, border=16, fast_threshold=20,
                 harris_threshold=1 << 15, log_bucket_size=0, bucket_limit=5, words=8,
                 max_keypoints=4096, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        lv = []
        for t in levels:
            w, h, r0 = t[0], t[1], t[2]
            c0 = t[3] if len(t) > 3 else 0
            lv.append(Level(w, h, r0, c0))
        self.levels = (Level * len(lv))(*lv)
        self.params = FrontendParams(vstep, rows, len(lv), border, fast_threshold, harris_threshold,
                                     log_bucket_size, bucket_limit, words, max_keypoints)

    def reserve(self, batch: int):
        c = self.ctx
        c.check(c.lib.pislam_frontend_reserve(c.h, ctypes.byref(self.params), self.levels, batch),
                "pislam_frontend_reserve")

    def alloc_outputs(self, batch: int, device):
        import torch
        p = self.params
        kp = torch.zeros((batch, p.max_keypoints), dtype=torch.int32, device=device)
        desc = torch.zeros((batch, p.max_keypoints, p.words), dtype=torch.int32, device=device)
        counts = torch.zeros((batch,), dtype=torch.int32, device=device)
        return kp, desc, counts

    def __call__(self, pyramids, kp, desc, counts):
        """pyramids: uint8 [batch][rows][vstep] device tensor; outputs int32 device tensors
        (bit patterns are the reference's uint32)."""
        c = self.ctx
        batch = int(pyramids.shape[0])
        stride = int(pyramids.stride(0)) if hasattr(pyramids, "stride") else self.params.rows * self.params.vstep
        c.check(c.lib.pislam_orb_frontend_batch(c.h, ctypes.byref(self.params), self.levels, ptr(pyramids),
                                                stride, batch, ptr(kp), ptr(desc), ptr(counts)),
                "pislam_orb_frontend_batch")

    def angles(self, pyramids, kp, counts, angles=None):
        """The rotation bin of every keypoint this front end wrote (orbAnglesBatch on this context)."""
        return orbAnglesBatch(pyramids, kp, counts, angles, ctx=self.ctx)

    def score_map(self, b: int) -> np.ndarray:
        c = self.ctx
        out = np.zeros((self.params.rows, self.params.vstep), np.uint8)
        c.check(c.lib.pislam_frontend_get_score_map(c.h, b, ptr(out)), "pislam_frontend_get_score_map")
        return out

    def last_timing(self):
        c = self.ctx
        tot = ctypes.c_float(0)
        st = (ctypes.c_float * 3)()
        c.check(c.lib.pislam_frontend_last_timing(c.h, ctypes.byref(tot), ctypes.byref(st)),
                "pislam_frontend_last_timing")
        return float(tot.value), [float(v) for v in st]

    PATH_STAGED, PATH_FUSED, PATH_ONE_LAUNCH, PATH_BUCKET_SELECT, PATH_BUCKETS_IN_STRIPS, PATH_GENERIC_ORB = 1, 2, 4, 8, 16, 32
    PATH_FRAME_TIMED_OUT = 64          # the one-launch path timed out earlier on this context: three launches from then on
    COUNT_INVALID = 0xFFFFFFFF         # PISLAM_COUNT_INVALID: counts[i] of a pyramid a timed-out one-launch call did not produce

    def last_path_of(self, ctx) -> int:
        """last_path() of another context (a pipeline lane) that ran this front-end's parameters."""
        return int(ctx.lib.pislam_frontend_last_path(ctx.h))

    def last_path(self) -> int:
        """Bit mask PATH_* of the path the last call on this context took — see pislam_frontend_last_path."""
        return int(self.ctx.lib.pislam_frontend_last_path(self.ctx.h))

    def last_stats(self):
        """(strips redone by the overflow pass, strips) of the last call — see pislam_frontend_last_stats."""
        c = self.ctx
        st = (ctypes.c_uint32 * 2)()
        c.check(c.lib.pislam_frontend_last_stats(c.h, ctypes.byref(st)), "pislam_frontend_last_stats")
        return int(st[0]), int(st[1])
