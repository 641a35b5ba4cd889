"""Map-point search by projection (pislam_match_projection_batch).

The contract is the comment in include/pislam_hip.h.  `ref_project` restates its steps 1-6 in numpy binary32, one
rounding per written operation (numpy's float32 multiply, add, divide and sqrt are correctly rounded), and
`ref_projection_match` its steps 7-8 with an nq x nt candidate mask over the scaled matcher's mapped train positions.
The CPU tests check the restatement on hand-built anchors, the host probe (tools/probes/project_host_check.cpp: the
library's own arithmetic header under the host compiler) against it bit for bit, and the tracking scene's
precondition.  The GPU tests compare the library with the restatement exactly."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_grid_passes as tgp
import test_match_scaled_window as tscaled
import test_match_select as tsel
from conftest import DEMO_LEVELS, ROOT
from test_match_window import COUNT_INVALID, SENTINEL, _lv, clamp_count, level_ids, pack, random_descriptors

F32, F64 = np.float32, np.float64
NONE = 0xFFFFFFFF
DEAD = 0xFF
Z_MIN = F32(2.0 ** -10)
S8 = SENTINEL & 0xFF
S32 = SENTINEL - (1 << 32) if SENTINEL >= 1 << 31 else SENTINEL   # the sentinel as an int32 fill value
PARAM_FIELDS = ["min_x", "max_x", "min_y", "max_y", "cos_min", "cos_near", "level_below", "level_above",
                "second_same_level"]
LEVELS3 = tgp.LEVELS3
WIDE = (-(2.0 ** 20), 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


# ---- the restatement -------------------------------------------------------------------------------------------------
def ref_project(pose, cam, xw, level_scale, radius_far, radius_near=None, *, bounds, cos_min=0.5, cos_near=0.998,
                normal=None, drange=None, qlevel=None):
    """Steps 1-6 for the n queries of one frame: dict of live (bool), xc, yc, pl (255 dead), near (bool), r."""
    assert (drange is None) != (qlevel is None) and (normal is None or drange is not None)
    T, C = np.asarray(pose, F32), np.asarray(cam, F32)
    xw = np.asarray(xw, F32).reshape(-1, 3)
    n = len(xw)
    ls = np.asarray(level_scale, F32)
    rf = np.asarray(radius_far, np.int64)
    rn = rf if radius_near is None else np.asarray(radius_near, np.int64)
    nl = len(ls)
    out = dict(live=np.zeros(n, bool), xc=np.zeros(n, np.int64), yc=np.zeros(n, np.int64), pl=np.full(n, DEAD, np.int64),
               near=np.zeros(n, bool), r=np.zeros(n, np.int64))
    if not (np.isfinite(T).all() and np.isfinite(C).all() and C[0] != 0 and C[1] != 0):
        return out
    minx, maxx, miny, maxy = (F32(v) for v in bounds)
    X, Y, Z = xw[:, 0], xw[:, 1], xw[:, 2]
    with np.errstate(all="ignore"):
        x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9]
        y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10]
        z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11]
        live = z >= Z_MIN
        iz = F32(1.0) / z
        pu = C[0] * (x * iz) + C[2]
        pv = C[1] * (y * iz) + C[3]
        live &= (pu >= minx) & (pu <= maxx) & (pv >= miny) & (pv <= maxy)
        fx_, fy_ = np.floor(pu + F32(0.5)), np.floor(pv + F32(0.5))
        near = np.zeros(n, bool)
        if drange is not None:
            dr = np.asarray(drange, F32).reshape(-1, 2)
            dmin, dmax = dr[:, 0], dr[:, 1]
            d = np.sqrt((x * x + y * y) + z * z)
            assert d.dtype == F32
            live &= (dmin <= d) & (d <= dmax)
            if normal is not None:
                nn = np.asarray(normal, F32).reshape(-1, 3)
                n0, n1, n2 = nn[:, 0], nn[:, 1], nn[:, 2]
                nc0 = (T[0] * n0 + T[1] * n1) + T[2] * n2
                nc1 = (T[3] * n0 + T[4] * n1) + T[5] * n2
                nc2 = (T[6] * n0 + T[7] * n1) + T[8] * n2
                c = (x * nc0 + y * nc1) + z * nc2
                live &= c >= F32(cos_min) * d
                near = c > F32(cos_near) * d
            pl = np.zeros(n, np.int64)
            for l in range(nl - 1):
                pl += (d * ls[l] < dmax)
        else:
            pl = np.asarray(qlevel, np.uint8).astype(np.int64)
            live &= pl < nl
    near &= live
    k = np.minimum(pl, nl - 1)
    out["live"] = live
    out["xc"] = np.where(live, fx_, 0).astype(np.int64)
    out["yc"] = np.where(live, fy_, 0).astype(np.int64)
    out["pl"] = np.where(live, pl, DEAD)
    out["near"] = near
    out["r"] = np.where(live, np.where(near, rn[k], rf[k]), 0)
    return out


def ref_projection_match(q, qd, tkp, td, levels, scale_q16, below, above, same_level, d=None):
    """Steps 7-8 of one frame: (idx int32, dist uint32, dist2 uint32) [nq] from ref_project's q."""
    nq, nt = len(qd), len(tkp)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE, np.uint32)
    dist2 = np.full(nq, NONE, np.uint32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2
    lt, Xt, Yt = tscaled.mapped_positions(tkp, levels, scale_q16)
    if d is None:
        d = tscaled.hamming(qd, td)
    pl, r = q["pl"][:, None], q["r"][:, None]
    mask = (q["live"][:, None] & (lt[None, :] >= 0) & (lt[None, :] >= pl - below) & (lt[None, :] <= pl + above)
            & (np.abs(q["xc"][:, None] - Xt[None, :]) <= r) & (np.abs(q["yc"][:, None] - Yt[None, :]) <= r))
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
    return idx, dist, dist2


CASE_DEFAULTS = dict(normal=None, drange=None, qlevel=None, radius_near=None, bounds=None, cos_min=0.5, cos_near=0.998,
                     below=1, above=0, same_level=1)


def default_bounds(levels):
    return (0.0, float(_lv(levels[0])[0] - 1), 0.0, float(_lv(levels[0])[1] - 1))


def ref_call(c, pairs=None, hams=None):
    """The five outputs of a call on case c (host arrays [B][...]), SENTINEL where nothing is written."""
    c = dict(CASE_DEFAULTS, **c)
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
        i, d, d2 = ref_projection_match(q, c["qd"][b, :nq], c["tkp"][b, :nt], c["td"][b, :nt], c["levels"], c["scale_q16"],
                                        c["below"], c["above"], c["same_level"],
                                        d=None if hams is None else hams[b][:nq, :nt])
        idx[b, :nq], dist[b, :nq], dist2[b, :nq] = i.view(np.uint32), d, d2
        pred[b, :nq, 0], pred[b, :nq, 1] = q["xc"].astype(np.int32).view(np.uint32), q["yc"].astype(np.int32).view(np.uint32)
        plevel[b, :nq] = q["pl"]
    return idx, dist, dist2, pred, plevel


def case_hams(c):
    return [tscaled.hamming(c["qd"][b], c["td"][b]) for b in range(len(c["qd"]))]


# ---- running the library ---------------------------------------------------------------------------------------------
def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def device_case(c):
    """The tensors of case c, uploaded once."""
    c = dict(CASE_DEFAULTS, **c)
    return {k: None if c[k] is None else to_dev(c[k]) for k in ("pose", "cam", "xw", "qd", "qc", "tkp", "td", "tc", "normal",
                                                                "drange", "qlevel")}


def run_projection(ctx, c, dev=None, want_pred=True, want_plevel=True):
    """Host arrays in, host arrays out: (idx, dist, dist2, pred, plevel) as uint32 / uint8 bit patterns; every output
    is pre-filled with the sentinel."""
    import torch
    from pislam_amd.frontend import matchProjectionBatch
    c = dict(CASE_DEFAULTS, **c)
    t = dev or device_case(c)
    B, qs = c["qd"].shape[:2]
    full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda:0")
    outs = dict(idx=full((B, qs), torch.int32, S32), dist=full((B, qs), torch.int32, S32), dist2=full((B, qs), torch.int32, S32),
                pred=full((B, qs, 2), torch.int32, S32) if want_pred else None,
                plevel=full((B, qs), torch.uint8, S8) if want_plevel else None)
    matchProjectionBatch(t["pose"], t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tc"], c["levels"],
                         drange=t["drange"], normal=t["normal"], qlevel=t["qlevel"], scale_q16=c["scale_q16"],
                         level_scale=c["level_scale"], radius_far=c["radius_far"], radius_near=c["radius_near"],
                         bounds=c["bounds"], cos_min=c["cos_min"], cos_near=c["cos_near"], level_below=c["below"],
                         level_above=c["above"], second_same_level=bool(c["same_level"]), want_pred=want_pred,
                         want_plevel=want_plevel, ctx=ctx, **outs)
    torch.cuda.synchronize()
    host = lambda o: None if o is None else (o.cpu().numpy().view(np.uint32) if o.dtype == torch.int32 else o.cpu().numpy())
    return tuple(host(outs[k]) for k in ("idx", "dist", "dist2", "pred", "plevel"))


NAMES = ("idx", "dist", "dist2", "pred", "plevel")


def assert_outputs(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- CPU: declarations -----------------------------------------------------------------------------------------------
def test_match_projection_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_match_projection_batch\s*\(", code), "not declared in include/pislam_hip.h"
    assert re.search(r"\bint\s+pislam_match_projection_reserve\s*\(", code)
    m = re.search(r"typedef struct pislam_projection_params \{([^}]*)\} pislam_projection_params;", code)
    assert m
    fields = []
    for ty, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", m.group(1)):
        fields += [(n.strip(), ty) for n in names.split(",")]
    assert [n for n, _ in fields] == PARAM_FIELDS
    assert [t for _, t in fields] == ["float"] * 6 + ["int32_t"] * 3
    assert "SearchBySim3, which pislam_match_hamming_scaled_window_batch with predicted centres covers" in text
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_match_projection_batch"][1]) == 28
    assert len(capi.SYMBOLS["pislam_match_projection_reserve"][1]) == 11
    assert [n for n, _ in capi.ProjectionParams._fields_] == PARAM_FIELDS and ctypes.sizeof(capi.ProjectionParams) == 36
    for f in ("reserveMatchProjection", "matchProjectionBatch", "projectionRadii", "matchedMapObservations"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    assert hasattr(lib, "pislam_match_projection_batch") and hasattr(lib, "pislam_match_projection_reserve")
    for f in ("pislam_project_math.h", "pislam_project_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "pislam_amd", "csrc", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "probes", "project_host_check.cpp"))
    assert "project_host_check" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_match_projection.py"))


def test_projection_radii_rounding():
    from pislam_amd.frontend import projectionRadii
    far, near = projectionRadii([65536, 78643, 98304, 65536 * 3], 3)
    assert far.dtype == np.int32 and near.dtype == np.int32
    assert far.tolist() == [12, 14, 18, 36]                 # 12, 14.4, 18, 36
    assert near.tolist() == [8, 9, 11, 23]                  # 7.5 up, 8.99998, 11.25, 22.5 up
    far, near = projectionRadii([1 << 20], 3000)
    assert far.tolist() == [65535] and near.tolist() == [65535]


# ---- CPU: hand-built anchors of the restatement ----------------------------------------------------------------------
CAM = np.array([500, 500, 320, 240, 0], F32)
TAB4 = dict(level_scale=np.array([1, 1.25, 1.5, 2], F32), radius_far=[12, 15, 18, 24], radius_near=[8, 9, 11, 15])
B640 = (0.0, 639.0, 0.0, 479.0)


def one(xw, pose=IDENTITY, cam=CAM, bounds=B640, **kw):
    tab = dict(TAB4)
    for k in list(kw):
        if k in tab:
            tab[k] = kw.pop(k)
    q = ref_project(pose, cam, np.asarray(xw, F32).reshape(1, 3), tab["level_scale"], tab["radius_far"], tab["radius_near"],
                    bounds=bounds, **{k: (None if v is None else np.asarray(v)[None]) if k in ("normal", "drange", "qlevel")
                                      else v for k, v in kw.items()})
    return {k: v[0] for k, v in q.items()}


def anchor_cases():
    """(keyword arguments of `one`, expected dict) for every anchor the contract names."""
    nan = F32(np.nan)
    A = []
    add = lambda kw, **want: A.append((kw, want))
    # a point on the optical axis lands on floor(cx + 0.5)
    for cx, want in ((320.0, 320), (320.25, 320), (320.5, 321), (319.75, 320)):
        add(dict(xw=[0, 0, 5], cam=np.array([500, 500, cx, 240, 0], F32), qlevel=1), live=True, xc=want, yc=240, pl=1, r=15)
    # pu exactly at min_x / max_x is live, one ulp outside is dead (pu = fx * 0 + cx = cx)
    add(dict(xw=[0, 0, 1], bounds=(320.0, 639.0, 0.0, 479.0), qlevel=0), live=True, xc=320)
    add(dict(xw=[0, 0, 1], bounds=(float(up(320)), 639.0, 0.0, 479.0), qlevel=0), live=False)
    add(dict(xw=[0, 0, 1], bounds=(0.0, 320.0, 0.0, 479.0), qlevel=0), live=True, xc=320)
    add(dict(xw=[0, 0, 1], bounds=(0.0, float(down(320)), 0.0, 479.0), qlevel=0), live=False)
    add(dict(xw=[0, 0, 1], bounds=(0.0, 639.0, 240.0, 240.0), qlevel=0), live=True, yc=240)
    add(dict(xw=[0, 0, 1], bounds=(0.0, 639.0, float(up(240)), 479.0), qlevel=0), live=False)
    add(dict(xw=[0, 0, 1], bounds=(0.0, 639.0, 0.0, float(down(240))), qlevel=0), live=False)
    # z at 2^-10 is live, just below it is dead
    add(dict(xw=[0, 0, Z_MIN], qlevel=0), live=True, xc=320, yc=240)
    add(dict(xw=[0, 0, down(Z_MIN)], qlevel=0), live=False)
    add(dict(xw=[0, 0, -5], qlevel=0), live=False)
    # d == dmin and d == dmax are live
    add(dict(xw=[0, 0, 5], drange=[5, 5]), live=True, pl=0)
    add(dict(xw=[3, 0, 4], drange=[5, 5], bounds=WIDE), live=True, pl=0, xc=695)
    add(dict(xw=[0, 0, 5], drange=[up(5), 8]), live=False)
    add(dict(xw=[0, 0, 5], drange=[1, down(5)]), live=False)
    # d * level_scale[l] == dmax exactly gives pl = l; pl clamps at nlevels - 1
    add(dict(xw=[0, 0, 5], drange=[1, 6.25]), live=True, pl=1, r=15)
    add(dict(xw=[0, 0, 5], drange=[1, 7.5]), live=True, pl=2, r=18)
    add(dict(xw=[0, 0, 5], drange=[1, up(7.5)]), live=True, pl=3, r=24)
    add(dict(xw=[0, 0, 5], drange=[1, 1e9]), live=True, pl=3, r=24)
    # c == cos_min * d is live, c == cos_near * d is not near (c = 4 * 0.5 = 2, d = 4)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, 0.5], cos_min=0.5, cos_near=0.5), live=True, near=False, pl=1, r=15)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, 0.5], cos_min=float(up(0.5)), cos_near=0.5), live=False)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, 0.5], cos_min=0.5, cos_near=float(down(0.5))), live=True, near=True,
        pl=1, r=9)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, 1]), live=True, near=True, r=9)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, -1]), live=False)
    add(dict(xw=[0, 0, 4], drange=[1, 5], normal=[0, 0, 1], radius_near=None), live=True, near=True, r=15)
    # qlevel >= nlevels is dead
    add(dict(xw=[0, 0, 5], qlevel=3), live=True, pl=3, r=24)
    add(dict(xw=[0, 0, 5], qlevel=4), live=False)
    add(dict(xw=[0, 0, 5], qlevel=255), live=False)
    # NaN in any of xw, normal, drange is dead
    for k in range(3):
        p = [0.1, 0.1, 5.0]
        p[k] = nan
        add(dict(xw=p, drange=[1, 9]), live=False)
        add(dict(xw=p, qlevel=0), live=False)
        nn = [0.0, 0.0, 1.0]
        nn[k] = nan
        add(dict(xw=[0, 0, 5], drange=[1, 9], normal=nn), live=False)
    add(dict(xw=[0, 0, 5], drange=[nan, 9]), live=False)
    add(dict(xw=[0, 0, 5], drange=[1, nan]), live=False)
    add(dict(xw=[np.inf, 0, 5], qlevel=0), live=False)
    # a frame whose pose or camera is not finite, or whose fx or fy is 0, is dead
    bad = IDENTITY.copy()
    bad[10] = np.inf
    add(dict(xw=[0, 0, 5], qlevel=0, pose=bad), live=False)
    add(dict(xw=[0, 0, 5], qlevel=0, cam=np.array([0, 500, 320, 240, 0], F32)), live=False)
    add(dict(xw=[0, 0, 5], qlevel=0, cam=np.array([500, 500, 320, 240, np.nan], F32)), live=False)
    return A


def test_ref_project_anchors():
    for kw, want in anchor_cases():
        q = one(**kw)
        for k, v in want.items():
            assert q[k] == v, (kw, k, q)
        if not want["live"]:
            assert (q["xc"], q["yc"], q["pl"], q["near"], q["r"]) == (0, 0, DEAD, False, 0), (kw, q)


def test_ref_match_level_window_and_same_level_rule():
    """Steps 7-8 on a hand-built frame: two levels, scale 2; train 0 on level 0 at (40, 20), train 1 on level 1 at
    local (20, 10) -> (40, 20), train 2 on level 1 at local (22, 10) -> (44, 20)."""
    levels, s = [(200, 100, 0, 0), (100, 50, 100, 0)], [65536, 131072]
    tkp = pack([40, 20, 22], [20, 110, 110])
    td = np.array([[1], [0], [3]], np.uint32)
    qd = np.zeros((1, 1), np.uint32)
    q = lambda pl, r: dict(live=np.array([True]), xc=np.array([40]), yc=np.array([20]), pl=np.array([pl]), r=np.array([r]))
    m = lambda pl, r, below, above, same: tuple(int(v[0]) for v in ref_projection_match(q(pl, r), qd, tkp, td, levels, s,
                                                                                       below, above, same))
    assert m(1, 4, 1, 0, 0) == (1, 0, 1)                    # levels 0..1: best train 1, runner-up train 0 (level 0)
    assert m(1, 4, 1, 0, 1) == (1, 0, NONE)                 # ... which the same-level rule hides
    assert m(1, 4, 0, 0, 1) == (1, 0, 2)                    # level 1 only: runner-up train 2 (popcount 3 = 2 bits)
    assert m(0, 4, 0, 0, 1) == (0, 1, NONE)
    assert m(0, 4, 0, 1, 0) == (1, 0, 1)
    assert m(0, 3, 0, 1, 1) == (1, 0, NONE)                 # radius 3 drops train 2 at |dx| = 4
    assert m(1, 3, 0, 0, 0) == (1, 0, NONE)
    dead = dict(q(0, 4), live=np.array([False]))
    assert tuple(int(v[0]) for v in ref_projection_match(dead, qd, tkp, td, levels, s, 1, 1, 0)) == (-1, NONE, NONE)


# ---- CPU: the host probe against the restatement ---------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(np.asarray(a, F32)).reshape(-1).view(np.uint32))


def probe_line(kw):
    """One probe input line from the keyword arguments of `one`."""
    tab = dict(TAB4)
    tab.update({k: kw[k] for k in tab if k in kw})
    rf = list(tab["radius_far"])
    rn = rf if tab["radius_near"] is None else list(tab["radius_near"])
    nl = len(rf)
    normal, drange, qlevel = kw.get("normal"), kw.get("drange"), kw.get("qlevel")
    parts = ["%d %d %d %d" % (nl, normal is not None, drange is not None, -1 if qlevel is None else qlevel),
             hexf(kw.get("pose", IDENTITY)), hexf(kw.get("cam", CAM)), hexf(kw["xw"])]
    if normal is not None:
        parts.append(hexf(normal))
    if drange is not None:
        parts.append(hexf(drange))
    parts += [hexf(tab["level_scale"]), " ".join(str(int(v)) for v in rf), " ".join(str(int(v)) for v in rn),
              hexf(kw.get("bounds", B640)), hexf([kw.get("cos_min", 0.5), kw.get("cos_near", 0.998)])]
    return " ".join(parts)


def random_queries(n, seed):
    """Keyword arguments of `one`: both modes, with and without a normal, poses near the identity, points in front of,
    behind and beside the camera, ranges that cut and levels past the table, a non-finite pose and a zero fx."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = rng.normal(0, 0.05, 3)
        Rx = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]])
        pose = np.concatenate([Rx.reshape(-1), rng.normal(0, 0.3, 3)]).astype(F32)
        cam = np.array([rng.uniform(300, 700), rng.uniform(300, 700), rng.uniform(300, 340), rng.uniform(220, 260), 40], F32)
        z = rng.uniform(0.5, 20) * (-1 if rng.random() < 0.05 else 1)
        xw = np.array([rng.uniform(-0.8, 0.8) * z, rng.uniform(-0.6, 0.6) * z, z], F32)
        nl = int(rng.integers(1, 9))
        ls = np.cumprod(np.r_[rng.uniform(0.5, 1.5), rng.uniform(1.0, 1.4, nl - 1)]).astype(F32)
        kw = dict(xw=xw, pose=pose, cam=cam, level_scale=ls, radius_far=rng.integers(0, 60, nl).tolist(),
                  radius_near=None if i % 3 == 0 else rng.integers(0, 60, nl).tolist(),
                  cos_min=float(rng.uniform(0.3, 0.7)), cos_near=float(rng.uniform(0.9, 1.0)))
        d = float(np.linalg.norm(xw))
        if i % 2:
            dmax = d * rng.uniform(0.9, 1.2 ** nl)
            kw["drange"] = np.array([dmax * rng.uniform(0.2, 1.1), dmax], F32)
            if i % 4 == 1:
                v = xw / max(d, 1e-6) + rng.normal(0, 0.3 if i % 8 == 1 else 0.02, 3)
                kw["normal"] = (v / np.linalg.norm(v)).astype(F32)
        else:
            kw["qlevel"] = int(rng.integers(0, nl + 2))
        if i % 97 == 0:
            kw["pose"] = pose.copy()
            kw["pose"][int(rng.integers(0, 12))] = [np.nan, np.inf, -np.inf][i % 3]
        if i % 101 == 0:
            kw["cam"] = cam.copy()
            kw["cam"][int(rng.integers(0, 2))] = 0
        out.append(kw)
    return out


@pytest.fixture(scope="module")
def run_probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("project_probe") / "project_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "project_host_check.cpp"), "-o", exe])

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def test_probe_equals_the_restatement(run_probe):
    """About 2000 queries: random ones in both modes, with and without a normal, plus every anchor."""
    cases = random_queries(1950, 5) + [kw for kw, _ in anchor_cases()]
    got = run_probe([probe_line(kw) for kw in cases])
    live = 0
    for kw, g in zip(cases, got):
        q = one(**kw)
        want = "%d %d %d %d %d %d" % (q["live"], q["xc"], q["yc"], q["pl"], q["near"], q["r"])
        assert g == want, (kw, g, want)
        live += int(q["live"])
    assert 400 < live < len(cases) - 400                     # the cases are neither all live nor all dead


# ---- the tracking scene ----------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def flip_bits(rng, desc, nbits):
    out = desc.copy()
    for i in range(len(out)):
        for b in rng.choice(32 * out.shape[1], nbits, replace=False):
            out[i, b // 32] ^= np.uint32(1) << np.uint32(b % 32)
    return out


@functools.lru_cache(maxsize=None)
def scene(seed, n=400):
    """One frame of the chain test (the issue's recipe): 400 map points seen by a 640 x 480 camera with 8 levels x 1.2,
    one keypoint per live point on its predicted level at the true pose, half as many distractors again, and a starting
    pose 0.3 degrees and 0.02 units off."""
    from pislam_amd.frontend import level_scales_q16, projectionRadii
    rng = np.random.default_rng([77, seed])
    levels = DEMO_LEVELS
    s = level_scales_q16(levels)
    ls = (np.asarray(s, F32) / F32(65536.0)).astype(F32)
    far, near = projectionRadii(s, 3)
    R = rodrigues(rng.normal(size=3), rng.uniform(0.05, 0.2))
    t = rng.normal(0, 0.5, 3)
    true = np.concatenate([R.reshape(-1), t]).astype(F32)
    Rt, tt = true[:9].astype(F64).reshape(3, 3), true[9:].astype(F64)
    u, v, z = rng.uniform(20, 620, n), rng.uniform(20, 460, n), rng.uniform(2, 20, n)
    Xc = np.stack([(u - 320) / 500 * z, (v - 240) / 500 * z, z], 1)
    xw = ((Xc - tt) @ Rt).astype(F32)                        # R^T (Xc - t)
    d = np.linalg.norm(Xc, axis=1)
    lt = rng.integers(0, 8, n)
    dmax = np.maximum(d * 1.2 ** (lt - 0.5), 1.05 * d)
    drange = np.stack([0.8 * dmax / 1.2 ** 7, dmax], 1).astype(F32)
    Ow = -Rt.T @ tt
    nrm = (xw - Ow) / np.linalg.norm(xw - Ow, axis=1)[:, None] + rng.normal(0, 0.05, (n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F32)
    bounds = default_bounds(levels)
    q = ref_project(true, CAM, xw, ls, far, near, bounds=bounds, normal=nrm, drange=drange)
    live = np.flatnonzero(q["live"])
    qd = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    lv = np.array([_lv(l) for l in levels], np.int64)
    pl = q["pl"][live]
    sc = np.asarray(s, F64)[pl] / 65536.0
    ku = np.clip(np.floor(u[live] / sc + 0.5).astype(np.int64), 0, lv[pl, 0] - 1)
    kv = np.clip(np.floor(v[live] / sc + 0.5).astype(np.int64), 0, lv[pl, 1] - 1)
    kp_own = pack(lv[pl, 3] + ku, lv[pl, 2] + kv)
    nd = len(live) // 2
    tkp = np.concatenate([kp_own, tgp.uniform_positions(rng, nd, levels)])
    td = np.concatenate([flip_bits(rng, qd[live], 12), rng.integers(0, 2 ** 32, (nd, 8), dtype=np.uint64).astype(np.uint32)])
    order = rng.permutation(len(tkp))
    tkp, td = tkp[order], td[order]
    own = np.full(n, -1, np.int64)
    own[live] = np.argsort(order)[:len(live)]
    start_R = rodrigues(rng.normal(size=3), np.deg2rad(0.3)) @ Rt
    dt = rng.normal(size=3)
    start = np.concatenate([start_R.reshape(-1), tt + 0.02 * dt / np.linalg.norm(dt)]).astype(F32)
    return dict(levels=levels, scale_q16=s, level_scale=ls, radius_far=far.tolist(), radius_near=near.tolist(), true=true,
                start=start, xw=xw, drange=drange, normal=nrm, qd=qd, tkp=tkp, td=td, own=own, nlive=len(live))


SCENE_BATCH = 4
SELECT = dict(max_dist=100, ratio=(8, 10), unique=1, rot_keep=0)


@functools.lru_cache(maxsize=None)
def scene_case():
    """The four frames as one case, strides padded past the counts, and its expected outputs."""
    fr = [scene(k) for k in range(SCENE_BATCH)]
    qs, ts = 416, max(len(f["tkp"]) for f in fr) + 7
    B = len(fr)
    c = dict(levels=fr[0]["levels"], scale_q16=fr[0]["scale_q16"], level_scale=fr[0]["level_scale"],
             radius_far=fr[0]["radius_far"], radius_near=fr[0]["radius_near"],
             pose=np.stack([f["start"] for f in fr]), cam=np.tile(CAM, (B, 1)), xw=np.zeros((B, qs, 3), F32),
             drange=np.zeros((B, qs, 2), F32), normal=np.zeros((B, qs, 3), F32), qd=np.zeros((B, qs, 8), np.uint32),
             qc=np.zeros(B, np.uint32), tkp=np.zeros((B, ts), np.uint32), td=np.zeros((B, ts, 8), np.uint32),
             tc=np.zeros(B, np.uint32))
    for b, f in enumerate(fr):
        n, nt = len(f["xw"]), len(f["tkp"])
        c["xw"][b, :n], c["drange"][b, :n], c["normal"][b, :n], c["qd"][b, :n] = f["xw"], f["drange"], f["normal"], f["qd"]
        c["tkp"][b, :nt], c["td"][b, :nt] = f["tkp"], f["td"]
        c["qc"][b], c["tc"][b] = n, nt
    want = ref_call(c)
    sel = []
    for b in range(B):
        nq, nt = int(c["qc"][b]), int(c["tc"][b])
        sq, st, _, _ = tsel.ref_select(want[0][b, :nq].view(np.int32), want[1][b, :nq], want[2][b, :nq], nt, **SELECT)
        sel.append((sq, st))
    return fr, c, want, sel


def test_scene_precondition():
    """In every frame at least 3/4 of the live points get their own keypoint as the accepted match (numpy only), so the
    chain test cannot pass on a handful of lucky matches."""
    fr, c, want, sel = scene_case()
    for b, f in enumerate(fr):
        sq, st = sel[b]
        ok = int((f["own"][sq] == st).sum())
        print("frame %d: %d live points, %d accepted, %d their own keypoint" % (b, f["nlive"], len(sq), ok))
        assert f["nlive"] >= 300 and 4 * ok >= 3 * f["nlive"], (b, f["nlive"], len(sq), ok)
        assert (want[4][b, :len(f["xw"])] != DEAD).sum() >= 300


# ---- GPU: pins -------------------------------------------------------------------------------------------------------
CAM3 = np.array([100, 100, 64, 48, 0], F32)
WINDOWS = [(1, 0), (0, 2), (2, 0), (1, 1), (0, 0)]


@functools.lru_cache(maxsize=None)
def pins_case(mode, words, B=3, qs=200, ts=300, seed=0):
    """Batch 3 on LEVELS3.  Queries aim at a train keypoint's level-0 position a few pixels off (half of them with a copy
    of its descriptor) or anywhere in the image; every tenth slot is one of the dead classes in turn."""
    rng = np.random.default_rng([21, seed, words, {"map": 0, "normal": 1, "level": 2}[mode]])
    levels = LEVELS3
    s = tscaled.level_scales(levels)
    nl = len(levels)
    c = dict(levels=levels, scale_q16=s, level_scale=np.array([1.1, 1.3, 1.6], F32), radius_far=[7, 9, 10],
             pose=np.zeros((B, 12), F32), cam=np.tile(CAM3, (B, 1)), xw=np.zeros((B, qs, 3), F32),
             qd=np.zeros((B, qs, words), np.uint32), qc=np.resize(np.array([qs, qs - 31, qs - 1], np.uint32), B),
             tkp=np.zeros((B, ts), np.uint32), td=np.zeros((B, ts, words), np.uint32),
             tc=np.resize(np.array([ts, ts - 17, 64], np.uint32), B))
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
        u = np.where(aimed, Xt[j] + rng.integers(-9, 10, qs), rng.uniform(-5, 133, qs))
        v = np.where(aimed, Yt[j] + rng.integers(-9, 10, qs), rng.uniform(-5, 101, qs))
        z = rng.uniform(1, 8, qs)
        Xc = np.stack([(u - 64) / 100 * z, (v - 48) / 100 * z, z], 1)
        c["qd"][b] = np.where((aimed & (rng.random(qs) < 0.6))[:, None], c["td"][b][j], random_descriptors(rng, qs, words))
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
        kind = np.where(np.arange(qs) % 10 == 9, (np.arange(qs) // 10) % 7, -1)
        Xc[kind == 0, 2] *= -1                               # behind the camera
        Xc[kind == 1, 0] = 3.0 * Xc[kind == 1, 2]            # out of the image
        dmin[kind == 2] = d[kind == 2] * 1.01                # nearer than dmin
        dmax[kind == 3] = d[kind == 3] * 0.99                # farther than dmax (dmin follows)
        dmin[kind == 3] = dmax[kind == 3] * 0.3
        nrm[kind == 4] *= -1                                 # seen from behind
        ql[kind == 5] = nl + (np.arange(qs)[kind == 5] // 10) % 3 * 100   # no such level
        c["xw"][b] = ((Xc - tt) @ Rt).astype(F32)
        c["xw"][b, kind == 6, (np.arange(qs)[kind == 6] // 10) % 3] = np.nan
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


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", ["map", "normal", "level"])
def test_gpu_projection_pins(gpu_ctx, mode, words):
    """Every level window, the same-level rule on and off and radius_near NULL and given, in one mode and width."""
    base = pins_case(mode, words)
    hams = case_hams(base)
    dev = device_case(base)
    live = dead = matched = same_cut = near = 0
    for below, above in WINDOWS:
        for same in (0, 1):
            for rn in (None, [4, 12, 5]):
                c = dict(base, below=below, above=above, same_level=same, radius_near=rn, cos_near=0.995)
                want = ref_call(c, hams=hams)
                got = run_projection(gpu_ctx, c, dev)
                assert_outputs(got, want, (mode, words, below, above, same, rn))
                nq = [int(v) for v in c["qc"]]
                pl = np.concatenate([want[4][b, :n] for b, n in enumerate(nq)])
                live += int((pl != DEAD).sum())
                dead += int((pl == DEAD).sum())
                matched += sum(int((want[0][b, :n].view(np.int32) >= 0).sum()) for b, n in enumerate(nq))
                if same:
                    c0 = ref_call(dict(c, same_level=0), hams=hams)
                    same_cut += int((c0[2] != want[2]).sum())
    # conditions on the inputs: the cases are live, dead, matched and cut by the same-level rule
    assert live > 1000 and dead > 1000 and matched > 1000 and same_cut > 0, (live, dead, matched, same_cut)


@pytest.mark.gpu
def test_gpu_projection_radius_near_is_used(gpu_ctx):
    """With a normal, the near radius changes results against radius_near NULL (a condition on the pins, then the pin)."""
    base = pins_case("normal", 2)
    a = ref_call(dict(base, cos_near=0.995))
    b = ref_call(dict(base, cos_near=0.995, radius_near=[0, 0, 0]))
    assert (a[0] != b[0]).any()
    assert_outputs(run_projection(gpu_ctx, dict(base, cos_near=0.995, radius_near=[0, 0, 0])), b)


# ---- GPU: where the contracts meet ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("span", [0, 1])
def test_gpu_projection_equals_the_scaled_matcher(gpu_ctx, span):
    """Level mode, level_below = level_above = span, no near radius, no same-level rule, the identity pose and the camera
    (1, 1, 0, 0): the point (X, Y, 1) projects to (X, Y) exactly, and the call is the scaled matcher with that
    prediction and a query keypoint anywhere on level pl."""
    rng = np.random.default_rng(31 + span)
    B, qs, ts, words = 3, 200, 300, 2
    levels = LEVELS3
    s = tscaled.level_scales(levels)
    r = [6, 7, 9]
    tkp = np.stack([tgp.uniform_positions(rng, ts, levels) for _ in range(B)])
    td = np.stack([random_descriptors(rng, ts, words) for _ in range(B)])
    qd = np.stack([random_descriptors(rng, qs, words) for _ in range(B)])
    pl = rng.integers(0, 3, (B, qs))
    X, Y = rng.integers(-3, 131, (B, qs)), rng.integers(-3, 99, (B, qs))
    lv = np.array([_lv(t) for t in levels], np.int64)
    qkp = pack(lv[pl, 3] + rng.integers(0, 60, (B, qs)), lv[pl, 2] + rng.integers(0, 60, (B, qs)))
    qc, tc = np.array([qs, qs - 3, 77], np.uint32), np.array([ts, 100, ts], np.uint32)
    c = dict(levels=levels, scale_q16=s, level_scale=[1.0, 1.2, 1.44], radius_far=r, bounds=WIDE,
             pose=np.tile(IDENTITY, (B, 1)), cam=np.tile(np.array([1, 1, 0, 0, 0], F32), (B, 1)),
             xw=np.stack([X, Y, np.ones_like(X)], -1).astype(F32), qlevel=pl.astype(np.uint8), qd=qd, qc=qc, tkp=tkp, td=td,
             tc=tc, below=span, above=span, same_level=0)
    got = run_projection(gpu_ctx, c)
    scaled = tscaled.run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc, qpred=np.stack([X, Y], -1))
    for name, g, w in zip(NAMES, got[:3], scaled):
        assert (g == w).all(), name
    assert (got[3].view(np.int32)[0, :, 0] == X[0]).all() and (got[4][0] == pl[0]).all()
    assert (got[0].view(np.int32)[0] >= 0).sum() > 50
    assert_outputs(got, ref_call(c))


# ---- GPU: counts and slots -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["normal", "level"])
def test_gpu_projection_counts_and_slots(gpu_ctx, mode):
    """PISLAM_COUNT_INVALID and counts above the stride on both sides, a train count of 0, dead frames (a pose that is
    not finite, fx == 0), sentinel-filled outputs untouched at and beyond nq_b, NULL pred / plevel."""
    base = pins_case(mode, 4, B=8, seed=1)
    qs, ts = base["qd"].shape[1], base["tkp"].shape[1]
    c = dict(base, qc=np.array([COUNT_INVALID, qs + 5, 0, 37, qs, 10, qs, qs], np.uint32),
             tc=np.array([ts, ts + 9, ts, COUNT_INVALID, 0, 5, ts, ts], np.uint32), pose=base["pose"].copy(),
             cam=base["cam"].copy())
    c["pose"][6, 4] = np.inf
    c["cam"][7, 0] = 0
    want = ref_call(c)
    assert (want[4][6] == DEAD).all() and (want[4][7] == DEAD).all() and (want[0][1].view(np.int32) >= 0).any()
    assert (want[0][0] == SENTINEL).all() and (want[0][3, 37:] == SENTINEL).all() and (want[0][3, :37].view(np.int32) == -1).all()
    assert (want[0][4].view(np.int32) == -1).all() and (want[4][4] != DEAD).any()
    got = run_projection(gpu_ctx, c)
    assert_outputs(got, want)
    bare = run_projection(gpu_ctx, c, want_pred=False, want_plevel=False)
    assert bare[3] is None and bare[4] is None
    assert_outputs(bare, want)


# ---- GPU: more than one grid pass ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_projection_more_queries_than_one_grid_pass(gpu_ctx):
    """k_match_projection at batch 1024, stride 1024 on the guided matchers' case of test_grid_passes.py: a query in no
    level becomes a point behind the camera, every other one the point (X, Y, 1) of its mapped position on its level."""
    B, qs, ts = 1024, 1024, 300
    P = tgp.guided_pass(qs, 64, B)
    tgp.need_three_passes(qs, P, "k_match_projection")
    g = tgp.guided_case(B, qs, ts, P)
    s = tscaled.level_scales(LEVELS3)
    lid, X, Y = tscaled.mapped_positions(g["qkp"].reshape(-1), LEVELS3, s)
    xw = np.stack([X, Y, np.where(lid >= 0, 1, -1)], 1).astype(F32).reshape(B, qs, 3)
    c = dict(levels=LEVELS3, scale_q16=s, level_scale=[1.0, 1.2, 1.44], radius_far=tscaled.scale_radii(s, 6), bounds=WIDE,
             pose=np.tile(IDENTITY, (B, 1)), cam=np.tile(np.array([1, 1, 0, 0, 0], F32), (B, 1)), xw=xw,
             qlevel=np.maximum(lid, 0).astype(np.uint8).reshape(B, qs), qd=g["qd"], qc=g["qc"], tkp=g["tkp"], td=g["td"],
             tc=g["tc"], below=1, above=1, same_level=0)
    live = g["pairs"]
    got = run_projection(gpu_ctx, c)
    want = ref_call(c, pairs=live)
    assert_outputs([o[live] for o in got], [o[live] for o in want])
    tgp.assert_empty_pairs_untouched(got, live, B)
    tgp.check_guided_third_pass(got[:3], g, P, qs)
    seg = got[4][0, tgp.third_pass(P, qs)]
    assert (seg == DEAD).any() and (seg != DEAD).any()


# ---- GPU: offsets beyond 4 GiB ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_projection_offsets_beyond_4_gib(gpu_ctx):
    """q_stride 16384 and 21848 frames: the map points (12 bytes each) and the predictions of the last two frames begin
    beyond 2^32 bytes.  Every array is allocated in one piece, uninitialised; all counts are 0 except the last
    frame's, so no other frame's queries are ever read."""
    import torch
    from pislam_amd.frontend import matchProjectionBatch
    B, qs, ts, words, n = 21848, 16384, 300, 1, 150
    assert (B - 1) * qs * 12 > 1 << 32
    need = B * qs * (12 + 4 * words + 3 * 4 + 8 + 1 + 1)
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the buffers above 4 GiB do not fit the free device memory")
    small = pins_case("level", words, B=1, qs=n, ts=ts, seed=2)
    dev = "cuda:0"
    xw = torch.empty((B, qs, 3), dtype=torch.float32, device=dev)
    qd = torch.empty((B, qs, words), dtype=torch.int32, device=dev)
    ql = torch.empty((B, qs), dtype=torch.uint8, device=dev)
    qc = torch.zeros((B,), dtype=torch.int32, device=dev)
    tc = torch.zeros((B,), dtype=torch.int32, device=dev)
    tkp = torch.zeros((B, ts), dtype=torch.int32, device=dev)
    td = torch.zeros((B, ts, words), dtype=torch.int32, device=dev)
    pose = to_dev(np.tile(small["pose"][0], (B, 1)))
    cam = to_dev(np.tile(small["cam"][0], (B, 1)))
    idx, dist, dist2 = (torch.empty((B, qs), dtype=torch.int32, device=dev) for _ in range(3))
    pred = torch.empty((B, qs, 2), dtype=torch.int32, device=dev)
    plevel = torch.empty((B, qs), dtype=torch.uint8, device=dev)
    b = B - 1
    for o in (idx, dist, dist2, pred):
        o[b, :n + 16] = S32
        o[b - 1, :16] = S32
    plevel[b, :n + 16] = S8
    xw[b, :n], qd[b, :n], ql[b, :n] = to_dev(small["xw"][0]), to_dev(small["qd"][0]), to_dev(small["qlevel"][0])
    qc[b], tc[b] = n, ts
    tkp[b], td[b] = to_dev(small["tkp"][0]), to_dev(small["td"][0])
    matchProjectionBatch(pose, cam, xw, qd, qc, tkp, td, tc, small["levels"], qlevel=ql, scale_q16=small["scale_q16"],
                         level_scale=small["level_scale"], radius_far=small["radius_far"], idx=idx, dist=dist, dist2=dist2,
                         pred=pred, plevel=plevel, ctx=gpu_ctx)
    torch.cuda.synchronize()
    want = ref_call(dict(small, qc=np.array([n], np.uint32), tc=np.array([ts], np.uint32)))
    got = [idx[b, :n + 16].cpu().numpy().view(np.uint32), dist[b, :n + 16].cpu().numpy().view(np.uint32),
           dist2[b, :n + 16].cpu().numpy().view(np.uint32), pred[b, :n + 16].cpu().numpy().view(np.uint32),
           plevel[b, :n + 16].cpu().numpy()]
    for name, g, w in zip(NAMES, got, want):
        assert (g[:n] == w[0, :n]).all(), name
        assert (g[n:] == (S8 if name == "plevel" else SENTINEL)).all(), (name, "written past the count")
    assert (got[0][:n].view(np.int32) >= 0).sum() > 20
    for o in (idx, dist, dist2, pred):
        assert (o[b - 1, :16] == S32).all()


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_projection_refusals_write_nothing(gpu_ctx):
    import torch
    from pislam_amd import capi
    from pislam_amd.frontend import matchProjectionBatch, reserveMatchProjection
    base = dict(CASE_DEFAULTS, **pins_case("normal", 1))
    lvl = pins_case("level", 1)["qlevel"]
    t = device_case(base)
    t["qlevel_given"] = to_dev(lvl)
    B, qs = base["qd"].shape[:2]
    outs = dict(idx=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"),
                dist=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"),
                dist2=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"),
                pred=torch.full((B, qs, 2), S32, dtype=torch.int32, device="cuda:0"),
                plevel=torch.full((B, qs), S8, dtype=torch.uint8, device="cuda:0"))

    def call(**over):
        kw = dict(drange=t["drange"], normal=t["normal"], qlevel=None, scale_q16=base["scale_q16"],
                  level_scale=base["level_scale"], radius_far=base["radius_far"], radius_near=None, bounds=None,
                  level_below=1, level_above=0)
        a = dict(xw=t["xw"], td=t["td"], tkp=t["tkp"])
        for k in list(over):
            if k in a:
                a[k] = over.pop(k)
        kw.update(over)
        matchProjectionBatch(t["pose"], t["cam"], a["xw"], t["qd"], t["qc"], a["tkp"], a["td"], t["tc"], base["levels"],
                             ctx=gpu_ctx, **kw, **outs)

    nan = float("nan")
    bad = dict(
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
                      td=torch.zeros((B, 65536, 1), dtype=torch.int32, device="cuda:0")))
    call()                                                                   # the unmodified call is accepted
    torch.cuda.synchronize()
    assert (outs["idx"][0] != S32).all()
    for o in outs.values():
        o.fill_(S8 if o.dtype == torch.uint8 else S32)
    for name, over in bad.items():
        with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
            call(**over)
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert (o == (S8 if o.dtype == torch.uint8 else S32)).all(), ("a refused call wrote", k)
    with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
        reserveMatchProjection(base["levels"], 65536, B, words=1, ctx=gpu_ctx)


# ---- GPU: hipGraph, determinism --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_projection_is_hipgraph_capturable(gpu_ctx):
    """After the reserve the call allocates nothing and never synchronises: captured on a side stream with a context of
    its own, the replay equals the eager call; the graph keeps the host tables it was captured with."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchProjectionBatch, reserveMatchProjection
    c = dict(CASE_DEFAULTS, **pins_case("normal", 8))
    want = ref_call(dict(c, cos_near=0.995, radius_near=[4, 12, 5]))
    t = device_case(c)
    B, qs = c["qd"].shape[:2]
    ts = c["tkp"].shape[1]
    dev = torch.device("cuda:0")
    ls = np.array(c["level_scale"], F32)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchProjection(c["levels"], ts, B, scale_q16=c["scale_q16"], radius_far=c["radius_far"],
                               radius_near=[4, 12, 5], words=8, ctx=ctx)
        outs = dict(idx=torch.zeros((B, qs), dtype=torch.int32, device=dev), dist=torch.zeros((B, qs), dtype=torch.int32, device=dev),
                    dist2=torch.zeros((B, qs), dtype=torch.int32, device=dev),
                    pred=torch.zeros((B, qs, 2), dtype=torch.int32, device=dev),
                    plevel=torch.zeros((B, qs), dtype=torch.uint8, device=dev))

        def call(**o):
            return matchProjectionBatch(t["pose"], t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tc"], c["levels"],
                                        drange=t["drange"], normal=t["normal"], scale_q16=c["scale_q16"], level_scale=ls,
                                        radius_far=c["radius_far"], radius_near=[4, 12, 5], cos_near=0.995, ctx=ctx, **o)

        eager = call()                                                       # warm-up (module load) and the eager result
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(**outs)
        for o in outs.values():
            o.zero_()
        ls[:] = 5.0                                                          # the graph holds its own copy of the tables
        g.replay()
        side.synchronize()
        for a, k in zip(eager, NAMES):
            assert torch.equal(a, outs[k]), k
    nq = [int(v) for v in c["qc"]]
    for k, w in zip(NAMES, want):
        g_ = outs[k].cpu().numpy()
        g_ = g_.view(np.uint32) if g_.dtype == np.int32 else g_
        for b, n in enumerate(nq):
            assert (g_[b, :n] == w[b, :n]).all(), (k, b)


@pytest.mark.gpu
def test_gpu_projection_is_deterministic_across_calls_and_paddings(gpu_ctx):
    """Two calls give identical outputs, and so do two q_stride paddings of the same queries (another launch shape)."""
    c = pins_case("normal", 8)
    first = run_projection(gpu_ctx, c)
    again = run_projection(gpu_ctx, c)
    assert_outputs(again, first)
    B, qs = c["qd"].shape[:2]
    pad = qs + 333
    wide = dict(c)
    for k in ("xw", "qd", "drange", "normal"):
        a = np.zeros((B, pad) + c[k].shape[2:], c[k].dtype)
        a[:, :qs] = c[k]
        wide[k] = a
    padded = run_projection(gpu_ctx, wide)
    for name, g, w in zip(NAMES, padded, first):
        assert (g[:, :qs] == w).all(), name
        assert (g[:, qs:] == (S8 if name == "plevel" else SENTINEL)).all(), name


# ---- GPU: the chain project -> match -> select -> refine --------------------------------------------------------------
def pose_errors(pose, true):
    """(rotation error in degrees, translation error) of float32 [12] poses."""
    R, Rt = pose[:9].astype(F64).reshape(3, 3), true[:9].astype(F64).reshape(3, 3)
    cos = np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1)
    return float(np.degrees(np.arccos(cos))), float(np.linalg.norm(pose[9:].astype(F64) - true[9:].astype(F64)))


@pytest.mark.gpu
def test_gpu_tracking_chain_improves_the_pose(gpu_ctx):
    """matchProjectionBatch -> selectMatchesBatch -> matchedMapObservations -> poseRefineBatch on the scene, batch 4:
    the selected pairs equal restatement plus select, the gathered observations equal a host-side gather, and every
    frame's pose_out is closer to the true pose than the perturbed start, in rotation and in translation."""
    import torch
    from pislam_amd.frontend import (matchedMapObservations, matchProjectionBatch, poseLevelWeights, poseRefineBatch,
                                     selectMatchesBatch)
    fr, c, want, sel = scene_case()
    B, qs = c["qd"].shape[:2]
    ts = c["tkp"].shape[1]
    t = device_case(c)
    got = run_projection(gpu_ctx, c, t)
    assert_outputs(got, want)
    idx, dist, dist2, pred, plevel = matchProjectionBatch(
        t["pose"], t["cam"], t["xw"], t["qd"], t["qc"], t["tkp"], t["td"], t["tc"], c["levels"], drange=t["drange"],
        normal=t["normal"], th=3, ctx=gpu_ctx)                               # every table and parameter by default
    gpu_ctx.synchronize()
    assert (idx.cpu().numpy().view(np.uint32)[:, :400] == want[0][:, :400]).all()
    sq, st, nsel = selectMatchesBatch(idx, dist, dist2, t["qc"], t["tc"], max_dist=100, ratio=(8, 10), t_stride=ts, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    xs, obs, level, counts = matchedMapObservations(t["xw"], t["tkp"], (sq, st, nsel), c["levels"], c["scale_q16"])
    torch.cuda.synchronize()
    sq, st, nsel = sq.cpu().numpy(), st.cpu().numpy(), nsel.cpu().numpy()
    xs_h, obs_h, level_h = xs.cpu().numpy(), obs.cpu().numpy(), level.cpu().numpy()
    lv = np.array([_lv(l) for l in c["levels"]], np.int64)
    s = np.asarray(c["scale_q16"], np.int64)
    for b in range(B):
        eq, et = sel[b]
        n = int(nsel[b])
        assert n == len(eq) and (sq[b, :n] == eq).all() and (st[b, :n] == et).all(), b
        lid, x, y = level_ids(c["tkp"][b][et], c["levels"])
        U = ((x - lv[lid, 3]) * 256 * s[lid] + 32768) // 65536
        V = ((y - lv[lid, 2]) * 256 * s[lid] + 32768) // 65536
        assert (xs_h[b, :n].view(np.uint32) == c["xw"][b][eq].view(np.uint32)).all() and not xs_h[b, n:].any()
        assert (obs_h[b, :n, 0] == U).all() and (obs_h[b, :n, 1] == V).all() and (obs_h[b, :, 2] == -(1 << 31)).all()
        assert not obs_h[b, n:, :2].any() and (level_h[b, :n] == lid).all() and (level_h[b, n:] == 255).all()
    assert (counts.cpu().numpy() == nsel).all()
    pose_out, inlier, ninl, cost, status = poseRefineBatch(t["pose"], t["cam"], xs, obs, counts, level=level,
                                                           inv_sigma2=poseLevelWeights(len(c["levels"])), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    out, status = pose_out.cpu().numpy(), status.cpu().numpy()
    for b, f in enumerate(fr):
        r0, t0 = pose_errors(f["start"], f["true"])
        r1, t1 = pose_errors(out[b], f["true"])
        print("frame %d: %d matches, rotation %.4f -> %.4f deg, translation %.5f -> %.5f" % (b, nsel[b], r0, r1, t0, t1))
        assert status[b] & 0xFF == 0, (b, status[b])
        assert r1 < r0 and t1 < t0, (b, r0, r1, t0, t1)
