"""Map-point fusion search (pislam_match_fuse_batch), after ORB-SLAM's ORBmatcher::Fuse.

The contract is the comment in include/pislam_hip.h: the projection call's steps plus a query mask and a reprojection
test per candidate.  `ref_fuse_call` restates it in numpy binary32, one rounding per written operation: steps 1-6 are
test_match_projection.ref_project, the pixel (pu, pv, pur) is recomputed here by the stated formulas (`ref_pixel`), the
test is `ref_fuse_mask`, steps 7-8 are `ref_fuse_match`.  The CPU tests check the restatement on hand-built anchors, the
host probe (tools/probes/fuse_host_check.cpp: the library's own arithmetic header under the host compiler) against it
bit for bit, fuseDecisions / rigidFromSim3 against plain loops, and the conditions on the inputs of the GPU tests.  The
GPU tests compare the library with the restatement exactly, every output pre-filled with a sentinel."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_grid_passes as tgp
import test_match_projection as tproj
import test_match_scaled_window as tscaled
import test_match_select as tsel
from conftest import ROOT
from test_match_projection import (CASE_DEFAULTS, DEAD, F32, F64, IDENTITY, LEVELS3, NAMES, NONE, S8, S32, WIDE, Z_MIN,
                                   assert_outputs, case_hams, default_bounds, down, hexf, ref_project, rodrigues, to_dev, up)
from test_match_window import COUNT_INVALID, SENTINEL, _lv, clamp_count, pack, random_descriptors

MONO = -(1 << 31)
OBS_MAX = 1 << 22
INF = float("inf")
FUSE_DEFAULTS = dict(CASE_DEFAULTS, qmask=None, chi2_mono=5.99, chi2_stereo=7.8)
FUSE_FIELDS = ["chi2_mono", "chi2_stereo"]


# ---- the restatement -------------------------------------------------------------------------------------------------
def obs_px(q8):
    """A Q8 word as the call reads it: clamped to [-2^22, 2^22], then float(q) * (1.0f / 256.0f)."""
    return np.clip(np.asarray(q8, np.int64), -OBS_MAX, OBS_MAX).astype(F32) * F32(1.0 / 256.0)


def ref_pixel(pose, cam, xw):
    """Step 1's pixel of the n queries of one frame: (pu, pv, pur) float32 [n] each, by the stated formulas."""
    T, C = np.asarray(pose, F32), np.asarray(cam, F32)
    xw = np.asarray(xw, F32).reshape(-1, 3)
    X, Y, Z = xw[:, 0], xw[:, 1], xw[:, 2]
    with np.errstate(all="ignore"):
        x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9]
        y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10]
        z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11]
        iz = F32(1.0) / z
        pu = C[0] * (x * iz) + C[2]
        pv = C[1] * (y * iz) + C[3]
        pur = pu - C[4] * iz
    assert pu.dtype == F32 and pur.dtype == F32
    return pu, pv, pur


def ref_fuse_mask(pix, tobs, lt, inv_sigma2, chi2_mono, chi2_stereo):
    """The reprojection test of step 7: bool [nq][nt] from the pixels pix = (pu, pv, pur) [nq], the observation words
    tobs int [nt][3], the train levels lt [nt] (any value for a keypoint in no level) and the table."""
    pu, pv, pur = (np.asarray(a, F32)[:, None] for a in pix)
    tobs = np.asarray(tobs, np.int64).reshape(-1, 3)
    u, v, r = obs_px(tobs[:, 0])[None, :], obs_px(tobs[:, 1])[None, :], obs_px(tobs[:, 2])[None, :]
    mono = (tobs[:, 2] == MONO)[None, :]
    w = np.asarray(inv_sigma2, F32)[np.clip(np.asarray(lt, np.int64), 0, len(inv_sigma2) - 1)][None, :]
    with np.errstate(all="ignore"):
        ex, ey = pu - u, pv - v
        e2 = ex * ex + ey * ey
        er = pur - r
        e2s = e2 + er * er
        assert e2s.dtype == F32 and w.dtype == F32
        return np.where(mono, e2 * w <= F32(chi2_mono), e2s * w <= F32(chi2_stereo))


def ref_fuse_match(q, pix, qd, tkp, td, tobs, inv_sigma2, chi2_mono, chi2_stereo, levels, scale_q16, below, above,
                   same_level, d=None, parts=False):
    """Steps 7-8 of one frame: (idx int32, dist uint32, dist2 uint32) [nq] from ref_project's q and ref_pixel's pix.
    parts: also the window mask and the test mask (bool [nq][nt])."""
    nq, nt = len(qd), len(tkp)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE, np.uint32)
    dist2 = np.full(nq, NONE, np.uint32)
    if nq == 0 or nt == 0:
        z = np.zeros((nq, nt), bool)
        return (idx, dist, dist2, z, z) if parts else (idx, dist, dist2)
    lt, Xt, Yt = tscaled.mapped_positions(tkp, levels, scale_q16)
    if d is None:
        d = tscaled.hamming(qd, td)
    pl, r = q["pl"][:, None], q["r"][:, None]
    window = (q["live"][:, None] & (lt[None, :] >= 0) & (lt[None, :] >= pl - below) & (lt[None, :] <= pl + above)
              & (np.abs(q["xc"][:, None] - Xt[None, :]) <= r) & (np.abs(q["yc"][:, None] - Yt[None, :]) <= r))
    test = ref_fuse_mask(pix, tobs, lt, inv_sigma2, chi2_mono, chi2_stereo)
    mask = window & test
    key = np.where(mask, d * 65536 + np.arange(nt, dtype=np.int64)[None, :], tscaled.BIG)
    rows = np.arange(nq)
    am = key.argmin(1)
    best = key[rows, am]
    key[rows, am] = tscaled.BIG
    a2 = key.argmin(1)
    second = key[rows, a2]
    has, has2 = best < tscaled.BIG, second < tscaled.BIG
    if same_level:
        has2 &= lt[am] == lt[a2]
    idx[:] = np.where(has, best % 65536, -1)
    dist[:] = np.where(has, best // 65536, NONE).astype(np.uint32)
    dist2[:] = np.where(has2, second // 65536, NONE).astype(np.uint32)
    return (idx, dist, dist2, window, test) if parts else (idx, dist, dist2)


def ref_fuse_call(c, pairs=None, hams=None, parts=None):
    """The five outputs of a call on case c (host arrays [B][...]), SENTINEL where nothing is written.  parts (a list):
    gets (b, live [nq], window [nq][nt], test [nq][nt]) per frame."""
    c = dict(FUSE_DEFAULTS, **c)
    B, qs = c["qd"].shape[:2]
    ts = c["tkp"].shape[1]
    bounds = default_bounds(c["levels"]) if c["bounds"] is None else c["bounds"]
    idx = np.full((B, qs), SENTINEL, np.uint32)
    dist, dist2 = idx.copy(), idx.copy()
    pred = np.full((B, qs, 2), SENTINEL, np.uint32)
    plevel = np.full((B, qs), S8, np.uint8)
    opt = lambda k, b, n: None if c[k] is None else c[k][b, :n]
    for b in (range(B) if pairs is None else pairs):
        nq, nt = clamp_count(c["qc"][b], qs), clamp_count(c["tc"][b], ts)
        q = ref_project(c["pose"][b], c["cam"][b], c["xw"][b, :nq], c["level_scale"], c["radius_far"], c["radius_near"],
                        bounds=bounds, cos_min=c["cos_min"], cos_near=c["cos_near"], normal=opt("normal", b, nq),
                        drange=opt("drange", b, nq), qlevel=opt("qlevel", b, nq))
        if c["qmask"] is not None:                           # step 0
            dead = c["qmask"][b, :nq] == 0
            q = dict(live=q["live"] & ~dead, near=q["near"] & ~dead, xc=np.where(dead, 0, q["xc"]), yc=np.where(dead, 0, q["yc"]),
                     pl=np.where(dead, DEAD, q["pl"]), r=np.where(dead, 0, q["r"]))
        pix = ref_pixel(c["pose"][b], c["cam"][b], c["xw"][b, :nq])
        out = ref_fuse_match(q, pix, c["qd"][b, :nq], c["tkp"][b, :nt], c["td"][b, :nt], c["tobs"][b, :nt], c["inv_sigma2"],
                             c["chi2_mono"], c["chi2_stereo"], c["levels"], c["scale_q16"], c["below"], c["above"],
                             c["same_level"], d=None if hams is None else hams[b][:nq, :nt], parts=parts is not None)
        if parts is not None:
            parts.append((b, q["live"], out[3], out[4]))
        i, d, d2 = out[:3]
        idx[b, :nq], dist[b, :nq], dist2[b, :nq] = i.view(np.uint32), d, d2
        pred[b, :nq, 0], pred[b, :nq, 1] = q["xc"].astype(np.int32).view(np.uint32), q["yc"].astype(np.int32).view(np.uint32)
        plevel[b, :nq] = q["pl"]
    return idx, dist, dist2, pred, plevel


# ---- running the library ---------------------------------------------------------------------------------------------
def device_case(c):
    """The tensors of case c, uploaded once."""
    c = dict(FUSE_DEFAULTS, **c)
    t = tproj.device_case(c)
    t["tobs"] = to_dev(np.asarray(c["tobs"], np.int32))
    t["qmask"] = None if c["qmask"] is None else to_dev(c["qmask"])
    return t


def sentinel_outputs(B, qs, want_pred=True, want_plevel=True):
    import torch
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda:0")
    return dict(idx=full((B, qs), torch.int32, S32), dist=full((B, qs), torch.int32, S32), dist2=full((B, qs), torch.int32, S32),
                pred=full((B, qs, 2), torch.int32, S32) if want_pred else None,
                plevel=full((B, qs), torch.uint8, S8) if want_plevel else None)


def host_outputs(outs):
    import torch
    host = lambda o: None if o is None else (o.cpu().numpy().view(np.uint32) if o.dtype == torch.int32 else o.cpu().numpy())
    return tuple(host(outs[k]) for k in NAMES)


def fuse_keywords(c, t):
    """matchFuseBatch's keyword arguments of case c with the device tensors t."""
    return dict(drange=t["drange"], normal=t["normal"], qlevel=t["qlevel"], qmask=t["qmask"], inv_sigma2=c["inv_sigma2"],
                chi2_mono=c["chi2_mono"], chi2_stereo=c["chi2_stereo"], scale_q16=c["scale_q16"],
                level_scale=c["level_scale"], radius_far=c["radius_far"], radius_near=c["radius_near"], bounds=c["bounds"],
                cos_min=c["cos_min"], cos_near=c["cos_near"], level_below=c["below"], level_above=c["above"],
                second_same_level=bool(c["same_level"]))


def run_fuse(ctx, c, dev=None, want_pred=True, want_plevel=True):
    """Host arrays in, host arrays out: (idx, dist, dist2, pred, plevel) as uint32 / uint8 bit patterns; every output
    is pre-filled with the sentinel."""
    import torch
    from pislam_amd.frontend import matchFuseBatch
    c = dict(FUSE_DEFAULTS, **c)
    t = dev or device_case(c)
    B, qs = c["qd"].shape[:2]
    outs = sentinel_outputs(B, qs, want_pred, want_plevel)
    matchFuseBatch(t["pose"], t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tobs"], t["tc"], c["levels"],
                   want_pred=want_pred, want_plevel=want_plevel, ctx=ctx, **fuse_keywords(c, t), **outs)
    torch.cuda.synchronize()
    return host_outputs(outs)


# ---- CPU: declarations -----------------------------------------------------------------------------------------------
def test_match_fuse_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_match_fuse_batch\s*\(", code), "not declared in include/pislam_hip.h"
    assert re.search(r"\bint\s+pislam_match_fuse_reserve\s*\(", code)
    m = re.search(r"typedef struct pislam_fuse_params \{([^}]*)\} pislam_fuse_params;", code)
    assert m
    assert re.findall(r"float\s+(\w+)\s*;", m.group(1)) == FUSE_FIELDS
    assert "#define PISLAM_ABI_VERSION 2" in re.sub(r"[ \t]+", " ", text)
    # every former "Not here: ... ORBmatcher::Fuse" note now names the call
    for note in re.findall(r"Not here:.*?\*/", text, flags=re.S):
        if "ORBmatcher::Fuse" in note:
            assert "pislam_match_fuse_batch" in note, note
    assert len(re.findall(r"ORBmatcher::Fuse[^.]*?pislam_match_fuse_batch", text, flags=re.S)) >= 4
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_match_fuse_batch"][1]) == 32
    assert len(capi.SYMBOLS["pislam_match_fuse_reserve"][1]) == 11
    assert [n for n, _ in capi.FuseParams._fields_] == FUSE_FIELDS and ctypes.sizeof(capi.FuseParams) == 8
    for f in ("reserveMatchFuse", "matchFuseBatch", "rigidFromSim3", "fuseDecisions"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    assert hasattr(lib, "pislam_match_fuse_batch") and hasattr(lib, "pislam_match_fuse_reserve")
    assert os.path.exists(os.path.join(ROOT, "tools", "probes", "fuse_host_check.cpp"))
    assert "fuse_host_check" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_fuse.py"))
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "pislam_match_fuse_batch" in open(os.path.join(ROOT, doc)).read(), doc


# ---- CPU: hand-built anchors of the restatement ----------------------------------------------------------------------
CAM40 = np.array([500, 500, 320, 240, 40], F32)
P4 = np.array([[0, 0, 4]], F32)                              # pu = 320, pv = 240, iz = 0.25, pur = 310, all exact
W2 = np.array([1.0, 0.25], F32)


def mask1(tobs, lt, chi2_mono=5.99, chi2_stereo=7.8, w=W2, xw=P4, cam=CAM40):
    return ref_fuse_mask(ref_pixel(IDENTITY, cam, xw), np.asarray(tobs, np.int64).reshape(-1, 3), lt, w, chi2_mono,
                         chi2_stereo)[0].tolist()


def q8(px):
    return int(round(px * 256))


def test_ref_pixel_and_mask_anchors():
    pu, pv, pur = ref_pixel(IDENTITY, CAM40, P4)
    assert (pu[0], pv[0], pur[0]) == (320.0, 240.0, 310.0)
    # monocular, ex = 2, ey = 0: e2 = 4; e2 * w = 4 on level 0 and 1 on level 1, exactly at the bound and one ulp above it
    kp = [[q8(318), q8(240), MONO]] * 2
    assert mask1(kp, [0, 1], chi2_mono=4.0) == [True, True]
    assert mask1(kp, [0, 1], chi2_mono=float(down(4.0))) == [False, True]
    assert mask1(kp, [0, 1], chi2_mono=1.0) == [False, True]
    assert mask1(kp, [0, 1], chi2_mono=float(down(1.0))) == [False, False]
    assert mask1(kp, [0, 1], chi2_mono=float(down(1.0)), chi2_stereo=INF) == [False, False]   # the stereo bound is not used
    # stereo, ex = 1, ey = 1, er = 2: e2 = (1 + 1) + 4 = 6; 6 and 1.5
    kp = [[q8(319), q8(241), q8(308)]] * 2
    assert mask1(kp, [0, 1], chi2_stereo=6.0) == [True, True]
    assert mask1(kp, [0, 1], chi2_stereo=float(down(6.0))) == [False, True]
    assert mask1(kp, [0, 1], chi2_stereo=1.5) == [False, True]
    assert mask1(kp, [0, 1], chi2_stereo=float(down(1.5))) == [False, False]
    assert mask1(kp, [0, 1], chi2_mono=1e-3, chi2_stereo=6.0) == [True, True]                  # the mono bound is not used
    # a stereo keypoint that passes on (ex, ey) alone and fails on er; the same words as a monocular keypoint pass
    assert mask1([[q8(319), q8(241), q8(306)], [q8(319), q8(241), MONO], [q8(319), q8(241), q8(309.5)]], [0, 0, 0]) == \
        [False, True, True]
    # Q8 sub-pixel words are exact: ex = 1 / 256
    assert mask1([[q8(320) - 1, q8(240), MONO]], [0], chi2_mono=2.0 ** -16) == [True]
    assert mask1([[q8(320) - 1, q8(240), MONO]], [0], chi2_mono=float(down(2.0 ** -16))) == [False]
    # the Q8 clamp: a word beyond +-2^22 reads as +-16384 px; u_right is clamped too (and INT32_MIN is not a coordinate)
    cam = np.array([1, 1, 0, 0, 0], F32)                     # pu = X, pv = Y, pur = pu
    assert obs_px([OBS_MAX, OBS_MAX + 1, 2 ** 31 - 1, -OBS_MAX - 1, MONO + 1]).tolist() == [16384.0] * 3 + [-16384.0] * 2
    for word in (OBS_MAX, OBS_MAX + 1, 2 ** 31 - 1):
        assert mask1([[word, 0, MONO]], [0], chi2_mono=1.0, xw=np.array([[16385, 0, 1]], F32), cam=cam) == [True]    # ex = 1
        assert mask1([[word, 0, word]], [0], chi2_stereo=2.0, xw=np.array([[16385, 0, 1]], F32), cam=cam) == [True]  # er = 1 too
        assert mask1([[word, 0, word]], [0], chi2_stereo=float(down(2.0)), xw=np.array([[16385, 0, 1]], F32), cam=cam) == [False]
    assert mask1([[0, -(2 ** 30), MONO]], [0], chi2_mono=1.0, xw=np.array([[0, -16385, 1]], F32), cam=cam) == [True]
    # both bounds +inf: everything passes, garbage included (and an overflow of bf * iz is inf, not NaN)
    garbage = [[2 ** 31 - 1, MONO + 1, 12345], [MONO, MONO, MONO], [0, 0, 2 ** 31 - 1]]
    assert mask1(garbage, [0, 1, 0], INF, INF) == [True] * 3
    assert mask1(garbage, [0, 1, 0], INF, INF, cam=np.array([500, 500, 320, 240, 3e38], F32), xw=np.array([[0, 0, Z_MIN]], F32)) \
        == [True] * 3


def two_level_case(**over):
    """One frame, two levels at scale 2 (test_match_projection's hand-built frame): train 0 on level 0 at (40, 20), train
    1 on level 1 at local (20, 10) -> (40, 20), train 2 on level 1 at local (22, 10) -> (44, 20); one query that projects
    to (40, 20) exactly with pur = 30 on the predicted level 1."""
    c = dict(levels=[(200, 100, 0, 0), (100, 50, 100, 0)], scale_q16=[65536, 131072], level_scale=np.array([1, 2], F32),
             radius_far=[4, 4], inv_sigma2=W2, bounds=WIDE, pose=IDENTITY[None].copy(), cam=np.array([[1, 1, 0, 0, 10]], F32),
             xw=np.array([[[40, 20, 1]]], F32), qlevel=np.array([[1]], np.uint8), qd=np.zeros((1, 1, 1), np.uint32),
             qc=np.array([1], np.uint32), tkp=pack([40, 20, 22], [20, 110, 110])[None], td=np.array([[[1], [0], [3]]], np.uint32),
             tobs=np.array([[[q8(40), q8(20), MONO], [q8(40), q8(20), q8(30)], [q8(44), q8(20), MONO]]], np.int64),
             tc=np.array([3], np.uint32), below=1, above=0, same_level=0)
    c.update(over)
    return c


def first(c):
    o = ref_fuse_call(c)
    return int(o[0].view(np.int32)[0, 0]), int(o[1][0, 0]), int(o[2][0, 0]), o[3].view(np.int32)[0, 0].tolist(), int(o[4][0, 0])


def test_ref_fuse_call_anchors():
    assert first(two_level_case()) == (1, 0, 1, [40, 20], 1)            # train 2: ex = 4, e2 * w = 4 passes 5.99
    assert first(two_level_case(chi2_mono=3.9)) == (1, 0, 1, [40, 20], 1)          # ... and fails 3.9: runner-up train 0
    assert first(two_level_case(chi2_mono=3.9, same_level=1)) == (1, 0, NONE, [40, 20], 1)
    assert first(two_level_case(chi2_mono=4.0, below=0)) == (1, 0, 2, [40, 20], 1)  # 16 * 0.25 = 4 <= 4: train 2 is back
    assert first(two_level_case(chi2_mono=float(down(4.0)), below=0)) == (1, 0, NONE, [40, 20], 1)
    # the level of the test is the level of the keypoint's POSITION: train 0 (level 0, w = 1) with ex = 2 fails 3.9,
    # the same words on train 1's level (w = 0.25) pass
    t = two_level_case(chi2_mono=3.9)
    t["tobs"] = np.array([[[q8(42), q8(20), MONO], [q8(42), q8(20), MONO], [q8(44), q8(20), MONO]]], np.int64)
    assert first(t) == (1, 0, NONE, [40, 20], 1)
    # the right coordinate alone cuts train 1 (er = 3, 9 * 0.25 = 2.25 > 2): train 0 wins
    t = two_level_case(chi2_stereo=2.0)
    t["tobs"][0, 1, 2] = q8(27)
    assert first(t) == (0, 1, 2, [40, 20], 1)
    # qmask 0, a dead frame, a query that is dead in the projection call
    assert first(two_level_case(qmask=np.array([[0]], np.uint8))) == (-1, NONE, NONE, [0, 0], DEAD)
    assert first(two_level_case(qmask=np.array([[7]], np.uint8))) == (1, 0, 1, [40, 20], 1)
    assert first(two_level_case(cam=np.array([[1, 1, 0, 0, np.inf]], F32))) == (-1, NONE, NONE, [0, 0], DEAD)
    assert first(two_level_case(qlevel=np.array([[2]], np.uint8))) == (-1, NONE, NONE, [0, 0], DEAD)
    # both bounds +inf with garbage in tobs: the projection call's outputs
    g = two_level_case(chi2_mono=INF, chi2_stereo=INF)
    g["tobs"] = np.array([[[2 ** 31 - 1, MONO, 5], [MONO, MONO, MONO], [-7, 2 ** 30, MONO + 1]]], np.int64)
    want = tproj.ref_call(g)
    for a, b in zip(ref_fuse_call(g), want):
        assert (a == b).all()
    assert first(g) == (1, 0, 1, [40, 20], 1)
    # a count of 0 and a count above the stride
    assert (ref_fuse_call(two_level_case(qc=np.array([0], np.uint32)))[0] == SENTINEL).all()
    assert first(two_level_case(qc=np.array([9], np.uint32), tc=np.array([COUNT_INVALID], np.uint32))) == \
        (-1, NONE, NONE, [40, 20], 1)


# ---- CPU: the host probe against the restatement ---------------------------------------------------------------------
def candidate_line(cand):
    return "%d %d %d %s" % (cand["obs"][0], cand["obs"][1], cand["obs"][2], hexf([cand["w"], cand["chi2_mono"], cand["chi2_stereo"]]))


def random_candidates(queries, seed):
    """One candidate per query: near the projection (a few pixels off, in units of the level's sigma), monocular or
    stereo, now and then with words at and beyond the clamp, and bounds that are ORB-SLAM's, tight, or +inf."""
    rng = np.random.default_rng(seed)
    out = []
    for i, kw in enumerate(queries):
        pu, pv, pur = (float(a[0]) for a in ref_pixel(kw.get("pose", IDENTITY), kw.get("cam", tproj.CAM), kw["xw"]))
        w = float(F32(1.0 / 1.2 ** (2 * int(rng.integers(0, 8)))))
        sig = 1.0 / np.sqrt(w)
        ok = np.isfinite([pu, pv, pur]).all() and max(abs(pu), abs(pv), abs(pur)) < 1e6
        base = [pu, pv, pur] if ok else [0.0, 0.0, 0.0]
        obs = [int(round((base[k] + rng.normal(0, 2.0 * sig)) * 256)) for k in range(3)]
        if i % 2:
            obs[2] = MONO
        if i % 41 == 0:
            obs[int(rng.integers(0, 3))] = int(rng.choice([OBS_MAX, OBS_MAX + 1, -OBS_MAX - 1, 2 ** 31 - 1, MONO + 1]))
        chi = [(5.99, 7.8), (2.0, 3.0), (INF, INF), (5.99, INF)][int(rng.integers(0, 4))]
        out.append(dict(obs=obs, w=w, chi2_mono=chi[0], chi2_stereo=chi[1]))
    return out


def anchor_lines():
    """The mask anchors as probe cases: (keyword arguments of tproj.one, candidate)."""
    kw = dict(xw=P4[0], cam=CAM40, qlevel=0)
    A = []
    for obs, w, cm, cs in (([q8(318), q8(240), MONO], 1.0, 4.0, 7.8), ([q8(318), q8(240), MONO], 1.0, float(down(4.0)), 7.8),
                           ([q8(318), q8(240), MONO], 0.25, 1.0, 7.8), ([q8(318), q8(240), MONO], 0.25, float(down(1.0)), INF),
                           ([q8(319), q8(241), q8(308)], 1.0, 1e-3, 6.0), ([q8(319), q8(241), q8(308)], 1.0, 5.99, float(down(6.0))),
                           ([q8(319), q8(241), q8(308)], 0.25, 5.99, 1.5), ([q8(319), q8(241), q8(308)], 0.25, 5.99, float(down(1.5))),
                           ([q8(319), q8(241), q8(306)], 1.0, 5.99, 7.8), ([q8(319), q8(241), MONO], 1.0, 5.99, 7.8),
                           ([2 ** 31 - 1, MONO + 1, 12345], 1.0, INF, INF), ([MONO, MONO, MONO], 0.25, INF, INF)):
        A.append((kw, dict(obs=obs, w=w, chi2_mono=cm, chi2_stereo=cs)))
    A.append((dict(xw=[0, 0, float(Z_MIN)], cam=np.array([500, 500, 320, 240, 3e38], F32), qlevel=0),
              dict(obs=[0, 0, 5], w=1.0, chi2_mono=INF, chi2_stereo=INF)))
    A.append((dict(xw=[0, 0, -4], cam=CAM40, qlevel=0), dict(obs=[q8(320), q8(240), MONO], w=1.0, chi2_mono=INF, chi2_stereo=INF)))
    return A


@pytest.fixture(scope="module")
def run_probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fuse_probe") / "fuse_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "fuse_host_check.cpp"), "-o", exe])

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def test_probe_equals_the_restatement(run_probe):
    """About 2000 lines: test_match_projection's random queries with a bf, one random candidate each, plus the anchors."""
    queries = tproj.random_queries(1950, 11)
    cases = list(zip(queries, random_candidates(queries, 12))) + anchor_lines()
    got = run_probe([tproj.probe_line(kw) + " " + candidate_line(cand) for kw, cand in cases])
    live = passed = failed = 0
    for (kw, cand), g in zip(cases, got):
        q = tproj.one(**kw)
        pix = ref_pixel(kw.get("pose", IDENTITY), kw.get("cam", tproj.CAM), kw["xw"])
        ok = bool(q["live"]) and bool(ref_fuse_mask(pix, [cand["obs"]], [0], [cand["w"]], cand["chi2_mono"],
                                                    cand["chi2_stereo"])[0, 0])
        want = "%d %d %d %d %d %d %d" % (q["live"], q["xc"], q["yc"], q["pl"], q["near"], q["r"], ok)
        assert g == want, (kw, cand, g, want)
        live += int(q["live"])
        passed += int(ok)
        failed += int(q["live"] and not ok)
    print("probe: %d lines, %d live, %d pass, %d live and fail" % (len(cases), live, passed, failed))
    assert passed > 150 and failed > 150, (live, passed, failed)   # the verdicts are neither all yes nor all no


# ---- CPU: fuseDecisions and rigidFromSim3 ----------------------------------------------------------------------------
def loop_decisions(sq, st, nsel, qid, tpoint, nobs):
    """The docstring's rule as a plain loop."""
    B, qs = sq.shape
    action, keep, drop = np.zeros((B, qs), np.uint8), np.full((B, qs), -1, np.int64), np.full((B, qs), -1, np.int64)
    for b in range(B):
        for s in range(int(nsel[b])):
            o, me = int(tpoint[b][int(st[b][s])]), int(qid[b][int(sq[b][s])])
            if o < 0:
                action[b, s], keep[b, s] = 1, me
            elif o == me:
                pass
            elif nobs[o] > nobs[me]:
                action[b, s], keep[b, s], drop[b, s] = 2, o, me
            else:
                action[b, s], keep[b, s], drop[b, s] = 3, me, o
    return action, keep, drop


def test_fuse_decisions_on_host_tensors():
    import torch
    from pislam_amd.frontend import fuseDecisions
    rng = np.random.default_rng(8)
    B, qs, ts, npts = 3, 40, 50, 200
    qid = rng.permutation(npts)[:B * qs].reshape(B, qs)
    nobs = rng.integers(1, 5, npts)                          # few values: many ties
    nsel = np.array([qs, 17, 0], np.int32)
    sq = np.full((B, qs), 0x5A5A5A5A, np.int32)              # unwritten slots hold a value no index may take
    st = np.full((B, qs), -0x5A5A5A5B, np.int32)
    tpoint = np.full((B, ts), -1, np.int64)
    for b in range(B):
        n = int(nsel[b])
        sq[b, :n] = np.sort(rng.permutation(qs)[:n])
        st[b, :n] = rng.permutation(ts)[:n]
        for s in range(n):
            kind = s % 4
            me = qid[b, sq[b, s]]
            if kind == 1:
                tpoint[b, st[b, s]] = me                     # the keypoint holds the query itself
            elif kind >= 2:
                other = int(rng.integers(0, npts))
                tpoint[b, st[b, s]] = other if other != me else (other + 1) % npts
    want = loop_decisions(sq, st, nsel, qid, tpoint, nobs)
    ties = sum(1 for b in range(B) for s in range(int(nsel[b]))
               if want[0][b, s] == 3 and nobs[want[1][b, s]] == nobs[want[2][b, s]])
    assert all((want[0] == a).sum() >= 5 for a in (0, 1, 2, 3)) and ties >= 2, "the case misses an action or a tie"
    for dt in (torch.int32, torch.int64):
        got = fuseDecisions((torch.from_numpy(sq), torch.from_numpy(st), torch.from_numpy(nsel)),
                            torch.from_numpy(qid).to(dt), torch.from_numpy(tpoint).to(dt), torch.from_numpy(nobs).to(dt))
        assert got[0].dtype == torch.uint8 and tuple(got[0].shape) == (B, qs)
        for g, w, name in zip(got, want, ("action", "keep", "drop")):
            assert (g.numpy().astype(np.int64) == w.astype(np.int64)).all(), name
    assert (want[0][1, 17:] == 0).all() and (want[1][2] == -1).all()


def test_rigid_from_sim3():
    import torch
    from pislam_amd.frontend import rigidFromSim3
    rng = np.random.default_rng(9)
    B = 16
    sim = np.zeros((B, 13), F32)
    for b in range(B):
        sim[b, :9] = rodrigues(rng.normal(size=3), rng.uniform(0, 1)).reshape(-1)
        sim[b, 9:12] = rng.normal(0, 2, 3)
        sim[b, 12] = rng.uniform(0.3, 3.0)
    want = np.zeros((B, 12), F32)
    for b in range(B):
        for k in range(9):
            want[b, k] = sim[b, k]
        for k in range(3):
            want[b, 9 + k] = F32(float(sim[b, 9 + k]) / float(sim[b, 12]))   # float64 division, one rounding
    got = rigidFromSim3(torch.from_numpy(sim))
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 12) and got.is_contiguous()
    assert (got.numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert (rigidFromSim3(sim).view(np.uint32) == want.view(np.uint32)).all()
    # the similarity and the rigid pose project a point to the same pixel (up to rounding)
    X = rng.normal(0, 1, 3) + [0, 0, 6]
    for b in range(B):
        R, t, s = sim[b, :9].astype(F64).reshape(3, 3), sim[b, 9:12].astype(F64), float(sim[b, 12])
        a, c = s * R @ X + t, R @ X + want[b, 9:].astype(F64)
        assert np.allclose(a[:2] / a[2], c[:2] / c[2], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        rigidFromSim3(torch.zeros((2, 12)))


# ---- the pins case ---------------------------------------------------------------------------------------------------
CAM3 = np.array([100, 100, 64, 48, 40], F32)
WINDOWS = [(1, 0), (0, 1)]
LS3 = np.array([1.1, 1.3, 1.6], F32)


@functools.lru_cache(maxsize=None)
def pins_case(mode, words, B=3, qs=200, ts=300, seed=0):
    """Batch 3 on LEVELS3 (the issue's recipe).  80 % of the queries aim at a train keypoint's mapped position, an integer
    in +-3 off per axis (six in ten of them with a copy of its descriptor), the rest anywhere; radius_far [4, 5, 6];
    tobs_q8 is the mapped position plus a jitter in [-128, 127] Q8; half the keypoints are stereo with u_right =
    u - 256 * bf / z of an aiming query plus noise of sigma 128 Q8; every tenth slot is one of test_match_projection's
    dead classes in turn, or qmask 0."""
    rng = np.random.default_rng([22, seed, words, {"map": 0, "normal": 1, "level": 2}[mode]])
    levels = LEVELS3
    s = tscaled.level_scales(levels)
    nl = len(levels)
    c = dict(levels=levels, scale_q16=s, level_scale=LS3, radius_far=[4, 5, 6], inv_sigma2=(F32(1.0) / (LS3 * LS3)).astype(F32),
             pose=np.zeros((B, 12), F32), cam=np.tile(CAM3, (B, 1)), xw=np.zeros((B, qs, 3), F32),
             qd=np.zeros((B, qs, words), np.uint32), qc=np.resize(np.array([qs, qs - 31, qs - 1], np.uint32), B),
             tkp=np.zeros((B, ts), np.uint32), td=np.zeros((B, ts, words), np.uint32), tobs=np.zeros((B, ts, 3), np.int64),
             tc=np.resize(np.array([ts, ts - 17, 64], np.uint32), B), qmask=np.ones((B, qs), np.uint8))
    drange, normal, qlevel = np.zeros((B, qs, 2), F32), np.zeros((B, qs, 3), F32), np.zeros((B, qs), np.uint8)
    for b in range(B):
        R = rodrigues(rng.normal(size=3), rng.uniform(0.0, 0.1))
        t = rng.normal(0, 0.2, 3)
        c["pose"][b] = np.concatenate([R.reshape(-1), t]).astype(F32)
        Rt, tt = c["pose"][b, :9].astype(F64).reshape(3, 3), c["pose"][b, 9:].astype(F64)
        nt = int(c["tc"][b])
        c["tkp"][b], c["td"][b] = tgp.uniform_positions(rng, ts, levels), random_descriptors(rng, ts, words)
        lt, Xt, Yt = tscaled.mapped_positions(c["tkp"][b], levels, s)
        j = rng.integers(0, nt, qs)
        aimed = rng.random(qs) < 0.8
        u = np.where(aimed, Xt[j] + rng.integers(-3, 4, qs), rng.uniform(-5, 133, qs))
        v = np.where(aimed, Yt[j] + rng.integers(-3, 4, qs), rng.uniform(-5, 101, qs))
        z = rng.uniform(1, 8, qs)
        Xc = np.stack([(u - 64) / 100 * z, (v - 48) / 100 * z, z], 1)
        c["qd"][b] = np.where((aimed & (rng.random(qs) < 0.6))[:, None], c["td"][b][j], random_descriptors(rng, qs, words))
        # the observations: the mapped position plus a sub-pixel jitter; the right coordinate from an aiming query's depth
        zt = rng.uniform(1, 8, ts)
        zt[j[aimed]] = z[aimed]
        U = Xt * 256 + rng.integers(-128, 128, ts)
        V = Yt * 256 + rng.integers(-128, 128, ts)
        ur = np.floor(U - 256 * 40.0 / zt + rng.normal(0, 128, ts) + 0.5).astype(np.int64)
        c["tobs"][b] = np.stack([U, V, np.where(rng.random(ts) < 0.5, ur, MONO)], 1)
        d = np.linalg.norm(Xc, axis=1)
        # a predicted level at or next to the aimed keypoint's: dmax between d * ls[pl - 1] and d * ls[pl]
        pl = np.clip(lt[j] + rng.integers(0, 2, qs), 0, nl - 1)
        ls = c["level_scale"].astype(F64)
        dmax = d * np.where(pl == 0, 1.05, np.where(pl == nl - 1, 1.8, np.sqrt(ls[np.maximum(pl - 1, 0)] * ls[pl])))
        dmin = dmax * 0.3
        nrm = Xc / d[:, None] + rng.normal(0, 0.02, (qs, 3))  # camera frame: the viewing ray, a third of them far off it
        wide = rng.random(qs) < 0.3
        nrm[wide] += rng.normal(0, 0.6, (int(wide.sum()), 3))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        ql = pl.copy()
        kind = np.where(np.arange(qs) % 10 == 9, (np.arange(qs) // 10) % 8, -1)
        Xc[kind == 0, 2] *= -1                               # behind the camera
        Xc[kind == 1, 0] = 3.0 * Xc[kind == 1, 2]            # out of the image
        dmin[kind == 2] = d[kind == 2] * 1.01                # nearer than dmin
        dmax[kind == 3] = d[kind == 3] * 0.99                # farther than dmax (dmin follows)
        dmin[kind == 3] = dmax[kind == 3] * 0.3
        nrm[kind == 4] *= -1                                 # seen from behind
        ql[kind == 5] = nl + (np.arange(qs)[kind == 5] // 10) % 3 * 100   # no such level
        c["xw"][b] = ((Xc - tt) @ Rt).astype(F32)
        c["xw"][b, kind == 6, (np.arange(qs)[kind == 6] // 10) % 3] = np.nan
        c["qmask"][b, kind == 7] = 0                         # already in the key frame
        drange[b] = np.stack([dmin, dmax], 1).astype(F32)
        normal[b] = (nrm @ Rt).astype(F32)                   # R^T n_c
        qlevel[b] = ql
    if mode == "level":
        c["qlevel"] = qlevel
    else:
        c["drange"] = drange
        if mode == "normal":
            c["normal"] = normal
    return c


def pins_shares(c, hams=None):
    """(live, matched, lost, changed, right_cut) over the batch at ORB-SLAM's bounds: live queries; those that end with
    a match; those with window candidates that lose all of them to the test; those whose match is not the projection
    matcher's winner; candidates inside the window cut by the right coordinate alone."""
    parts = []
    want = ref_fuse_call(c, hams=hams, parts=parts)
    proj = tproj.ref_call(c, hams=hams)
    live = matched = lost = changed = right_cut = 0
    for b, lv, window, test in parts:
        nq = len(lv)
        idx = want[0][b, :nq].view(np.int32)
        pidx = proj[0][b, :nq].view(np.int32)
        live += int(lv.sum())
        matched += int((idx >= 0).sum())
        lost += int((window.any(1) & ~(window & test).any(1)).sum())
        changed += int(((idx >= 0) & (idx != pidx)).sum())
        nt = window.shape[1]
        mono = np.array(c["tobs"][b, :nt])
        mono[:, 2] = MONO
        pix = ref_pixel(c["pose"][b], c["cam"][b], c["xw"][b, :nq])
        lt = tscaled.mapped_positions(c["tkp"][b, :nt], c["levels"], c["scale_q16"])[0]
        as_mono = ref_fuse_mask(pix, mono, lt, c["inv_sigma2"], c["chi2_mono"] if "chi2_mono" in c else 5.99, INF)
        stereo = (np.asarray(c["tobs"][b, :nt, 2]) != MONO)[None, :]
        right_cut += int((window & stereo & as_mono & ~test).sum())
    return live, matched, lost, changed, right_cut


@pytest.mark.parametrize("words", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", ["map", "normal", "level"])
def test_pins_case_input_conditions(mode, words):
    """Numpy only: the pins case exercises what the GPU pins claim to pin.  Of the live queries at least 1/3 end with a
    match, at least 1/5 have window candidates and lose all of them to the test, at least 1/20 keep a match that is not
    the projection matcher's winner, and at least 50 candidates are cut by the right coordinate alone."""
    c = pins_case(mode, words)
    assert c["qc"].tolist() == [200, 169, 199] and c["tc"].tolist() == [300, 283, 64]
    live, matched, lost, changed, right_cut = pins_shares(c)
    print("pins %s/%d: %d live, %d matched, %d lost, %d changed winner, %d cut by the right coordinate alone"
          % (mode, words, live, matched, lost, changed, right_cut))
    assert live >= 300
    assert 3 * matched >= live and 5 * lost >= live and 20 * changed >= live and right_cut >= 50, \
        (live, matched, lost, changed, right_cut)
    assert (c["qmask"] == 0).sum() >= 5 and (c["tobs"][..., 2] == MONO).mean() > 0.3


# ---- the chain scene -------------------------------------------------------------------------------------------------
CHAIN_BATCH = 4
CHAIN_SELECT = dict(max_dist=50, ratio=None, unique=1, rot_keep=0)
NPTS = 400


def observations_q8(tkp, levels, scale_q16):
    """poseObservationsQ8's (U, V) of packed keypoints, in numpy."""
    lid, X, Y = tscaled.mapped_positions(tkp, levels, scale_q16)   # only for the level ids
    lv = np.array([_lv(l) for l in levels], np.int64)
    s = np.asarray(scale_q16, np.int64)
    x, y = (np.asarray(tkp, np.int64) >> 12) & 0xFFF, np.asarray(tkp, np.int64) & 0xFFF
    k = np.maximum(lid, 0)
    U = np.where(lid >= 0, ((x - lv[k, 3]) * 256 * s[k] + 32768) // 65536, 0)
    V = np.where(lid >= 0, ((y - lv[k, 2]) * 256 * s[k] + 32768) // 65536, 0)
    return U, V


@functools.lru_cache(maxsize=None)
def chain_case(sim_scale=None):
    """Four key frames of test_match_projection's scene at their true poses (400 map points and half as many distractor
    keypoints each), with bf 40: the points of frame b have the ids 400 b + i.  Of a point's own keypoint, a third
    already hold the point (qmask 0), a third hold a duplicate (id 1600 + the point's) and a third hold none; half the
    own keypoints are stereo.  sim_scale s: the poses are given as similarities (R, s t, s) whose rigidFromSim3 is the
    frame's pose, and both bounds are +inf."""
    rng = np.random.default_rng(91)
    fr = [tproj.scene(k) for k in range(CHAIN_BATCH)]
    B = len(fr)
    qs, ts = 416, max(len(f["tkp"]) for f in fr) + 7
    from pislam_amd.frontend import poseLevelWeights
    c = dict(levels=fr[0]["levels"], scale_q16=fr[0]["scale_q16"], level_scale=fr[0]["level_scale"],
             radius_far=None, inv_sigma2=poseLevelWeights(len(fr[0]["levels"])),
             pose=np.stack([f["true"] for f in fr]), cam=np.tile(np.array([500, 500, 320, 240, 40], F32), (B, 1)),
             xw=np.zeros((B, qs, 3), F32), drange=np.zeros((B, qs, 2), F32), normal=np.zeros((B, qs, 3), F32),
             qd=np.zeros((B, qs, 8), np.uint32), qc=np.zeros(B, np.uint32), tkp=np.zeros((B, ts), np.uint32),
             td=np.zeros((B, ts, 8), np.uint32), tobs=np.zeros((B, ts, 3), np.int64), tc=np.zeros(B, np.uint32),
             qmask=np.ones((B, qs), np.uint8))
    from pislam_amd.frontend import projectionRadii
    c["radius_far"] = projectionRadii(c["scale_q16"], 3, near=1, far=1)[0].tolist()
    qid = np.full((B, qs), -1, np.int64)
    tpoint = np.full((B, ts), -1, np.int64)
    nobs = rng.integers(1, 6, 2 * B * NPTS)
    cls = np.full((B, qs), -1, np.int64)
    for b, f in enumerate(fr):
        n, nt = len(f["xw"]), len(f["tkp"])
        c["xw"][b, :n], c["drange"][b, :n], c["normal"][b, :n], c["qd"][b, :n] = f["xw"], f["drange"], f["normal"], f["qd"]
        c["tkp"][b, :nt], c["td"][b, :nt] = f["tkp"], f["td"]
        c["qc"][b], c["tc"][b] = n, nt
        qid[b, :n] = NPTS * b + np.arange(n)
        U, V = observations_q8(f["tkp"], c["levels"], c["scale_q16"])
        ur = np.where(rng.random(nt) < 0.3, U - rng.integers(0, 40 * 256, nt), MONO)      # distractors
        Rt, tt = f["true"][:9].astype(F64).reshape(3, 3), f["true"][9:].astype(F64)
        zc = (f["xw"].astype(F64) @ Rt.T + tt)[:, 2]
        for i in np.flatnonzero(f["own"] >= 0):
            k = int(f["own"][i])
            ur[k] = int(np.floor(U[k] - 256 * 40.0 / zc[i] + 0.5)) if i % 2 else MONO
            cls[b, i] = (i // 2) % 3
            if cls[b, i] == 0:
                tpoint[b, k], c["qmask"][b, i] = qid[b, i], 0
            elif cls[b, i] == 1:
                tpoint[b, k] = B * NPTS + qid[b, i]
        c["tobs"][b, :nt] = np.stack([U, V, ur], 1)
    out = dict(c=c, fr=fr, qid=qid, tpoint=tpoint, nobs=nobs, cls=cls)
    if sim_scale is not None:
        s = float(sim_scale)
        out["sim"] = np.concatenate([c["pose"][:, :9], (c["pose"][:, 9:].astype(F64) * s).astype(F32),
                                     np.full((B, 1), s, F32)], 1).astype(F32)
        from pislam_amd.frontend import rigidFromSim3
        c["pose"] = rigidFromSim3(out["sim"])
        c["chi2_mono"], c["chi2_stereo"] = INF, INF
    want = ref_fuse_call(c)
    sel, dec = [], []
    sq_all = np.zeros((B, qs), np.int32)
    st_all = np.zeros((B, qs), np.int32)
    nsel = np.zeros(B, np.int32)
    for b in range(B):
        nq, nt = int(c["qc"][b]), int(c["tc"][b])
        sq, st, _, _ = tsel.ref_select(want[0][b, :nq].view(np.int32), want[1][b, :nq], want[2][b, :nq], nt, **CHAIN_SELECT)
        sel.append((sq, st))
        sq_all[b, :len(sq)], st_all[b, :len(sq)], nsel[b] = sq, st, len(sq)
    out.update(want=want, sel=sel, decisions=loop_decisions(sq_all, st_all, nsel, qid, tpoint, nobs), nsel=nsel)
    return out


@pytest.mark.parametrize("sim_scale", [None, 1.7])
def test_chain_scene_precondition(sim_scale):
    """Numpy only: in every frame at least 3/4 of the fusable points (live, not already in the key frame) get their own
    keypoint as the accepted match, and the batch holds at least 100 each of add, keep-theirs and keep-ours."""
    s = chain_case(sim_scale)
    c = s["c"]
    for b, f in enumerate(s["fr"]):
        sq, st = s["sel"][b]
        n = len(f["xw"])
        fusable = (s["want"][4][b, :n] != DEAD)
        ok = int((f["own"][sq] == st).sum())
        print("frame %d: %d fusable points, %d accepted, %d their own keypoint" % (b, fusable.sum(), len(sq), ok))
        assert fusable.sum() >= 150 and 4 * ok >= 3 * fusable.sum(), (b, fusable.sum(), len(sq), ok)
        assert not (c["qmask"][b, sq] == 0).any()
    action = s["decisions"][0]
    counts = [int((action == a).sum()) for a in (1, 2, 3)]
    print("decisions: %d add, %d keep theirs, %d keep ours" % tuple(counts))
    assert min(counts) >= 100, counts


# ---- GPU: pins -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", ["map", "normal", "level"])
def test_gpu_fuse_pins(gpu_ctx, mode, words):
    """Level windows (1, 0) and (0, 1) and the same-level rule on and off, in one mode and width."""
    base = pins_case(mode, words)
    hams = case_hams(base)
    dev = device_case(base)
    matched = same_cut = 0
    for below, above in WINDOWS:
        for same in (0, 1):
            c = dict(base, below=below, above=above, same_level=same)
            want = ref_fuse_call(c, hams=hams)
            got = run_fuse(gpu_ctx, c, dev)
            assert_outputs(got, want, (mode, words, below, above, same))
            matched += int((want[0].view(np.int32)[want[0] != SENTINEL] >= 0).sum())
            if same:
                same_cut += int((ref_fuse_call(dict(c, same_level=0), hams=hams)[2] != want[2]).sum())
    assert matched > 400 and same_cut > 0, (matched, same_cut)


# ---- GPU: where the contracts meet ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["normal", "level"])
def test_gpu_fuse_equals_match_projection_at_infinite_bounds(gpu_ctx, mode):
    """Both bounds +inf and qmask NULL: all five outputs equal matchProjectionBatch's on the same device buffers,
    whatever tobs_q8 holds (here: random words, INT32_MIN and INT32_MAX among them)."""
    rng = np.random.default_rng(41)
    base = pins_case(mode, 4)
    tobs = rng.integers(-(2 ** 31), 2 ** 31, base["tobs"].shape, dtype=np.int64)
    tobs[rng.random(tobs.shape) < 0.1] = MONO
    tobs[rng.random(tobs.shape) < 0.1] = 2 ** 31 - 1
    c = dict(base, tobs=tobs, qmask=None, chi2_mono=INF, chi2_stereo=INF)
    dev = device_case(c)
    got = run_fuse(gpu_ctx, c, dev)
    proj = tproj.run_projection(gpu_ctx, c, dev)
    assert_outputs(got, proj)
    assert_outputs(got, ref_fuse_call(c))
    assert (got[0].view(np.int32)[got[0] != SENTINEL] >= 0).sum() > 200
    finite = run_fuse(gpu_ctx, dict(c, chi2_mono=5.99, chi2_stereo=7.8), dev)   # (and the bounds do matter on these inputs)
    assert (finite[0] != got[0]).any()


# ---- GPU: counts and slots -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["normal", "level"])
def test_gpu_fuse_counts_and_slots(gpu_ctx, mode):
    """PISLAM_COUNT_INVALID and counts above the stride on both sides, a train count of 0, dead frames (a pose that is
    not finite, fx == 0), qmask all 0 for one frame, sentinel-filled outputs untouched at and beyond nq_b, NULL pred /
    plevel."""
    base = pins_case(mode, 4, B=9, seed=1)
    qs, ts = base["qd"].shape[1], base["tkp"].shape[1]
    c = dict(base, qc=np.array([COUNT_INVALID, qs + 5, 0, 37, qs, 10, qs, qs, qs], np.uint32),
             tc=np.array([ts, ts + 9, ts, COUNT_INVALID, 0, 5, ts, ts, ts], np.uint32), pose=base["pose"].copy(),
             cam=base["cam"].copy(), qmask=base["qmask"].copy())
    c["pose"][6, 4] = np.inf
    c["cam"][7, 0] = 0
    c["qmask"][8] = 0
    want = ref_fuse_call(c)
    assert (want[4][6] == DEAD).all() and (want[4][7] == DEAD).all() and (want[0][1].view(np.int32) >= 0).any()
    assert (want[4][8] == DEAD).all() and (want[0][8].view(np.int32) == -1).all() and (want[3][8] == 0).all()
    assert (want[0][0] == SENTINEL).all() and (want[0][3, 37:] == SENTINEL).all() and (want[0][3, :37].view(np.int32) == -1).all()
    assert (want[0][4].view(np.int32) == -1).all() and (want[4][4] != DEAD).any()
    got = run_fuse(gpu_ctx, c)
    assert_outputs(got, want)
    bare = run_fuse(gpu_ctx, c, want_pred=False, want_plevel=False)
    assert bare[3] is None and bare[4] is None
    assert_outputs(bare, want)


# ---- GPU: more than one grid pass ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fuse_more_queries_than_one_grid_pass(gpu_ctx):
    """k_match_fuse at batch 1024, stride 1024 on the guided matchers' case of test_grid_passes.py (the shape of
    test_gpu_projection_more_queries_than_one_grid_pass): a query in no level becomes a point behind the camera, every
    other one the point (X, Y, 1) of its mapped position on its level; the keypoints' observations are their mapped
    positions plus a jitter, a third of them stereo."""
    B, qs, ts = 1024, 1024, 300
    P = tgp.guided_pass(qs, 64, B)
    tgp.need_three_passes(qs, P, "k_match_fuse")
    g = tgp.guided_case(B, qs, ts, P)
    rng = np.random.default_rng(51)
    s = tscaled.level_scales(LEVELS3)
    lid, X, Y = tscaled.mapped_positions(g["qkp"].reshape(-1), LEVELS3, s)
    xw = np.stack([X, Y, np.where(lid >= 0, 1, -1)], 1).astype(F32).reshape(B, qs, 3)
    _, Xt, Yt = tscaled.mapped_positions(g["tkp"].reshape(-1), LEVELS3, s)
    U = Xt * 256 + rng.integers(-700, 700, B * ts)
    V = Yt * 256 + rng.integers(-700, 700, B * ts)
    ur = np.where(rng.random(B * ts) < 0.33, U - 256 * 3 + rng.integers(-400, 400, B * ts), MONO)
    c = dict(levels=LEVELS3, scale_q16=s, level_scale=[1.0, 1.2, 1.44], radius_far=tscaled.scale_radii(s, 6), bounds=WIDE,
             inv_sigma2=np.array([1.0, 0.7, 0.5], F32), pose=np.tile(IDENTITY, (B, 1)),
             cam=np.tile(np.array([1, 1, 0, 0, 3], F32), (B, 1)), xw=xw,
             qlevel=np.maximum(lid, 0).astype(np.uint8).reshape(B, qs), qd=g["qd"], qc=g["qc"], tkp=g["tkp"], td=g["td"],
             tobs=np.stack([U, V, ur], 1).reshape(B, ts, 3), tc=g["tc"], below=1, above=1, same_level=0)
    live = g["pairs"]
    got = run_fuse(gpu_ctx, c)
    want = ref_fuse_call(c, pairs=live)
    assert_outputs([o[live] for o in got], [o[live] for o in want])
    tgp.assert_empty_pairs_untouched(got, live, B)
    seg = tgp.third_pass(P, qs)
    idx = got[0].view(np.int32)
    assert (idx[0, seg] >= 0).any() and (idx[0, seg] == -1).any()
    assert idx[-1, 2 * P] != SENTINEL and (got[0][-1, 2 * P + 1:] == SENTINEL).all()
    assert (got[4][0, seg] == DEAD).any() and (got[4][0, seg] != DEAD).any()
    proj = tproj.ref_call(c, pairs=[0])
    assert (proj[0][0] != want[0][0]).any(), "the test cuts nothing in the first pair"


# ---- GPU: offsets beyond 4 GiB ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fuse_train_offsets_beyond_4_gib(gpu_ctx):
    """t_stride 65535 and 5464 frames: the last frame's tobs_q8 row (12 bytes per keypoint) begins beyond 2^32 bytes.
    Every array is allocated in one piece; all counts are 0 except the last frame's."""
    import torch
    from pislam_amd.frontend import matchFuseBatch
    B, qs, ts, words, n, nt = 5464, 160, 65535, 1, 150, 300
    assert (B - 1) * ts * 12 > 1 << 32
    need = B * ts * (12 + 4 + 4 * words) * 2 + B * qs * 64          # inputs plus the call's index of the same size
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the buffers above 4 GiB do not fit the free device memory")
    small = pins_case("level", words, B=1, qs=n, ts=nt, seed=2)
    dev = "cuda:0"
    tobs = torch.empty((B, ts, 3), dtype=torch.int32, device=dev)
    tkp = torch.empty((B, ts), dtype=torch.int32, device=dev)
    td = torch.empty((B, ts, words), dtype=torch.int32, device=dev)
    xw = torch.zeros((B, qs, 3), dtype=torch.float32, device=dev)
    qd = torch.zeros((B, qs, words), dtype=torch.int32, device=dev)
    ql = torch.zeros((B, qs), dtype=torch.uint8, device=dev)
    qm = torch.ones((B, qs), dtype=torch.uint8, device=dev)
    qc = torch.zeros((B,), dtype=torch.int32, device=dev)
    tc = torch.zeros((B,), dtype=torch.int32, device=dev)
    pose = to_dev(np.tile(small["pose"][0], (B, 1)))
    cam = to_dev(np.tile(small["cam"][0], (B, 1)))
    outs = sentinel_outputs(B, qs)
    b = B - 1
    xw[b, :n], qd[b, :n], ql[b, :n] = to_dev(small["xw"][0]), to_dev(small["qd"][0]), to_dev(small["qlevel"][0])
    qm[b, :n] = to_dev(small["qmask"][0])
    qc[b], tc[b] = n, nt
    tkp[b, :nt], td[b, :nt] = to_dev(small["tkp"][0]), to_dev(small["td"][0])
    tobs[b, :nt] = to_dev(small["tobs"][0].astype(np.int32))
    kw = dict(qlevel=ql, qmask=qm, inv_sigma2=small["inv_sigma2"], scale_q16=small["scale_q16"],
              level_scale=small["level_scale"], radius_far=small["radius_far"], ctx=gpu_ctx)
    matchFuseBatch(pose, cam, xw, qd, qc, tkp, td, tobs, tc, small["levels"], **kw, **outs)
    torch.cuda.synchronize()
    want = ref_fuse_call(dict(small, qc=np.array([n], np.uint32), tc=np.array([nt], np.uint32)))
    got = host_outputs({k: o[b - 1:] for k, o in outs.items()})
    for name, g, w in zip(NAMES, got, want):
        fill = S8 if name == "plevel" else SENTINEL
        assert (g[1, :n] == w[0, :n]).all(), name
        assert (g[1, n:] == fill).all() and (g[0] == fill).all(), (name, "written past the count")
    assert (got[0][1, :n].view(np.int32) >= 0).sum() > 20
    tobs[b, :nt, 0] += 40 * 256                                              # the row is read where it lies: moved observations
    matchFuseBatch(pose, cam, xw, qd, qc, tkp, td, tobs, tc, small["levels"], **kw, **outs)
    torch.cuda.synchronize()
    assert (outs["idx"][b, :n] == -1).all()


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fuse_refusals_write_nothing(gpu_ctx):
    import torch
    from pislam_amd import capi
    from pislam_amd.frontend import matchFuseBatch, reserveMatchFuse
    base = dict(FUSE_DEFAULTS, **pins_case("normal", 1))
    lvl = pins_case("level", 1)["qlevel"]
    t = device_case(base)
    t["qlevel_given"] = to_dev(lvl)
    B, qs = base["qd"].shape[:2]
    ts = base["tkp"].shape[1]
    outs = sentinel_outputs(B, qs)

    def call(**over):
        kw = dict(drange=t["drange"], normal=t["normal"], qlevel=None, qmask=t["qmask"], inv_sigma2=base["inv_sigma2"],
                  scale_q16=base["scale_q16"], level_scale=base["level_scale"], radius_far=base["radius_far"],
                  radius_near=None, bounds=None, level_below=1, level_above=0)
        a = dict(xw=t["xw"], td=t["td"], tkp=t["tkp"], tobs=t["tobs"])
        for k in list(over):
            if k in a:
                a[k] = over.pop(k)
        kw.update(over)
        matchFuseBatch(t["pose"], t["cam"], a["xw"], t["qd"], t["qc"], a["tkp"], a["td"], a["tobs"], t["tc"], base["levels"],
                       ctx=gpu_ctx, **kw, **outs)

    nan = float("nan")
    bad = dict(
        chi2_mono_nan=dict(chi2_mono=nan), chi2_stereo_nan=dict(chi2_stereo=nan), chi2_mono_zero=dict(chi2_mono=0.0),
        chi2_stereo_zero=dict(chi2_stereo=0.0), chi2_mono_negative=dict(chi2_mono=-1.0),
        chi2_stereo_negative=dict(chi2_stereo=-INF),
        sigma_zero=dict(inv_sigma2=[1.0, 0.0, 0.5]), sigma_inf=dict(inv_sigma2=[1.0, INF, 0.5]),
        sigma_nan=dict(inv_sigma2=[nan, 0.7, 0.5]), sigma_negative=dict(inv_sigma2=[1.0, 0.7, -0.5]),
        host_tobs=dict(tobs=t["tobs"].cpu()), host_qmask=dict(qmask=t["qmask"].cpu()),
        # the projection call's refusals
        both=dict(qlevel=t["qlevel_given"]), neither=dict(drange=None, normal=None),
        normal_with_level=dict(drange=None, qlevel=t["qlevel_given"]),
        host_pointer=dict(xw=t["xw"].cpu()), host_normal=dict(normal=t["normal"].cpu()),
        radius_far=dict(radius_far=[7, 65536, 10]), radius_far_negative=dict(radius_far=[-1, 9, 10]),
        radius_near=dict(radius_near=[7, 9, 65536]),
        bounds_nan=dict(bounds=(0.0, nan, 0.0, 95.0)), bounds_large=dict(bounds=(0.0, 2.0 ** 20 + 1, 0.0, 95.0)),
        bounds_order=dict(bounds=(10.0, 9.0, 0.0, 95.0)), bounds_order_y=dict(bounds=(0.0, 127.0, 1.0, 0.0)),
        below=dict(level_below=3), below_negative=dict(level_below=-1), above=dict(level_above=3),
        scale_zero=dict(level_scale=[0.0, 1.0, 1.2]), scale_falls=dict(level_scale=[1.0, 1.2, 1.1]),
        scale_nan=dict(level_scale=[1.0, nan, 1.2]), scale_inf=dict(level_scale=[1.0, 1.2, float("inf")]),
        t_stride=dict(tkp=torch.zeros((B, 65536), dtype=torch.int32, device="cuda:0"),
                      td=torch.zeros((B, 65536, 1), dtype=torch.int32, device="cuda:0"),
                      tobs=torch.zeros((B, 65536, 3), dtype=torch.int32, device="cuda:0")))
    call()                                                                   # the unmodified call is accepted
    call(chi2_mono=INF, chi2_stereo=INF)                                     # and so are infinite bounds
    torch.cuda.synchronize()
    assert (outs["idx"][0] != S32).all()
    for o in outs.values():
        o.fill_(S8 if o.dtype == torch.uint8 else S32)
    for name, over in bad.items():
        with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
            call(**over)
    # NULL inv_sigma2, f and tobs_q8 straight through the C ABI (the Python layer fills the first two in)
    from pislam_amd.frontend import _projection_params, _projection_tables, ptr
    lv, n, s, ls, rf, rn = _projection_tables(base["levels"], base["scale_q16"], base["level_scale"], base["radius_far"], None, 3)
    p = _projection_params(base["levels"], None, 0.5, 0.998, 1, 0, True)
    w = (ctypes.c_float * 3)(*[float(v) for v in base["inv_sigma2"]])
    f = capi.FuseParams(5.99, 7.8)

    def raw(w_, f_, tobs_):
        return gpu_ctx.lib.pislam_match_fuse_batch(
            gpu_ctx.h, 1, lv, n, s, ls, rf, rn, ctypes.byref(p), w_, f_, ptr(t["pose"]), ptr(t["cam"]), ptr(t["xw"]),
            ptr(t["normal"]), ptr(t["drange"]), None, ptr(t["qmask"]), ptr(t["qd"]), ptr(t["qc"]), qs, ptr(t["tkp"]),
            ptr(t["td"]), tobs_, ptr(t["tc"]), ts, B, ptr(outs["idx"]), ptr(outs["dist"]), ptr(outs["dist2"]),
            ptr(outs["pred"]), ptr(outs["plevel"]))
    assert raw(None, ctypes.byref(f), ptr(t["tobs"])) == -1
    assert raw(w, None, ptr(t["tobs"])) == -1
    assert raw(w, ctypes.byref(f), None) == -1
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert (o == (S8 if o.dtype == torch.uint8 else S32)).all(), ("a refused call wrote", k)
    assert raw(w, ctypes.byref(f), ptr(t["tobs"])) == 0
    torch.cuda.synchronize()
    assert (outs["idx"][0] != S32).all()
    with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
        reserveMatchFuse(base["levels"], 65536, B, words=1, ctx=gpu_ctx)


# ---- GPU: hipGraph, determinism --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fuse_is_hipgraph_capturable(gpu_ctx):
    """After the reserve the call allocates nothing and never synchronises: captured on a side stream with a context of
    its own, the replay equals the eager call; the graph keeps the host tables it was captured with, and survives a
    later, larger reserve of the projection matcher on the same context."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchFuseBatch, reserveMatchFuse, reserveMatchProjection
    c = dict(FUSE_DEFAULTS, **pins_case("normal", 8))
    want = ref_fuse_call(c)
    t = device_case(c)
    B, qs = c["qd"].shape[:2]
    ts = c["tkp"].shape[1]
    dev = torch.device("cuda:0")
    ls = np.array(c["level_scale"], F32)
    w = np.array(c["inv_sigma2"], F32)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchFuse(c["levels"], ts, B, scale_q16=c["scale_q16"], radius_far=c["radius_far"], words=8, ctx=ctx)
        outs = dict(idx=torch.zeros((B, qs), dtype=torch.int32, device=dev), dist=torch.zeros((B, qs), dtype=torch.int32, device=dev),
                    dist2=torch.zeros((B, qs), dtype=torch.int32, device=dev),
                    pred=torch.zeros((B, qs, 2), dtype=torch.int32, device=dev),
                    plevel=torch.zeros((B, qs), dtype=torch.uint8, device=dev))

        def call(**o):
            kw = fuse_keywords(c, t)
            kw.update(level_scale=ls, inv_sigma2=w)
            return matchFuseBatch(t["pose"], t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tobs"], t["tc"],
                                  c["levels"], ctx=ctx, **kw, **o)

        eager = call()                                                       # warm-up (module load) and the eager result
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(**outs)
        for o in outs.values():
            o.zero_()
        ls[:] = 5.0                                                          # the graph holds its own copy of the tables
        w[:] = 1e-6
        reserveMatchProjection(c["levels"], 4 * ts, 4 * B, scale_q16=c["scale_q16"], radius_far=c["radius_far"], words=8,
                               ctx=ctx)                                      # another call's workspace grows
        side.synchronize()
        g.replay()
        side.synchronize()
        for a, k in zip(eager, NAMES):
            assert torch.equal(a, outs[k]), k
    nq = [int(v) for v in c["qc"]]
    for k, wnt in zip(NAMES, want):
        g_ = outs[k].cpu().numpy()
        g_ = g_.view(np.uint32) if g_.dtype == np.int32 else g_
        for b, n in enumerate(nq):
            assert (g_[b, :n] == wnt[b, :n]).all(), (k, b)


@pytest.mark.gpu
def test_gpu_fuse_is_deterministic_across_calls_and_paddings(gpu_ctx):
    """Two calls give identical outputs, and so do two q_stride paddings of the same queries (another launch shape)."""
    c = pins_case("normal", 8)
    first_ = run_fuse(gpu_ctx, c)
    again = run_fuse(gpu_ctx, c)
    assert_outputs(again, first_)
    B, qs = c["qd"].shape[:2]
    pad = qs + 333
    wide = dict(c)
    for k in ("xw", "qd", "drange", "normal", "qmask"):
        a = np.zeros((B, pad) + c[k].shape[2:], c[k].dtype)
        a[:, :qs] = c[k]
        wide[k] = a
    padded = run_fuse(gpu_ctx, wide)
    for name, g, w in zip(NAMES, padded, first_):
        assert (g[:, :qs] == w).all(), name
        assert (g[:, qs:] == (S8 if name == "plevel" else SENTINEL)).all(), name


# ---- GPU: the chain fuse -> select -> decisions -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sim_scale", [None, 1.7])
def test_gpu_fuse_chain_decisions(gpu_ctx, sim_scale):
    """matchFuseBatch -> selectMatchesBatch -> fuseDecisions on the scene, batch 4, every table by default: the matches
    equal the restatement, the selected pairs equal restatement plus select, and actions, keeps and drops equal the
    plain loop's exactly.  sim_scale: the same scene through rigidFromSim3 from a similarity with s != 1, both bounds
    +inf (the loop-closing form)."""
    import torch
    from pislam_amd.frontend import fuseDecisions, matchFuseBatch, rigidFromSim3, selectMatchesBatch
    s = chain_case(sim_scale)
    c = dict(FUSE_DEFAULTS, **s["c"])
    B, qs = c["qd"].shape[:2]
    ts = c["tkp"].shape[1]
    t = device_case(c)
    pose = t["pose"]
    if sim_scale is not None:
        pose = rigidFromSim3(to_dev(s["sim"]))
        assert (pose.cpu().numpy().view(np.uint32) == c["pose"].view(np.uint32)).all()
    outs = sentinel_outputs(B, qs)
    chi = dict(chi2_mono=INF, chi2_stereo=INF) if sim_scale is not None else {}
    idx, dist, dist2, pred, plevel = matchFuseBatch(
        pose, t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tobs"], t["tc"], c["levels"], drange=t["drange"],
        normal=t["normal"], qmask=t["qmask"], ctx=gpu_ctx, **chi, **outs)    # every table and parameter by default
    gpu_ctx.synchronize()
    assert_outputs(host_outputs(outs), s["want"])
    sq, st, nsel = selectMatchesBatch(idx, dist, dist2, t["qc"], t["tc"], max_dist=50, ratio=None, rot_keep=0, t_stride=ts,
                                      ctx=gpu_ctx)
    gpu_ctx.synchronize()
    action, keep, drop = fuseDecisions((sq, st, nsel), to_dev(s["qid"]), to_dev(s["tpoint"]), to_dev(s["nobs"]))
    torch.cuda.synchronize()
    sq, st, nsel = sq.cpu().numpy(), st.cpu().numpy(), nsel.cpu().numpy()
    for b in range(B):
        eq, et = s["sel"][b]
        n = int(nsel[b])
        assert n == len(eq) and (sq[b, :n] == eq).all() and (st[b, :n] == et).all(), b
    for g, w, name in zip((action, keep, drop), s["decisions"], ("action", "keep", "drop")):
        assert (g.cpu().numpy().astype(np.int64) == w.astype(np.int64)).all(), name
    assert min(int((action == a).sum()) for a in (1, 2, 3)) >= 100
