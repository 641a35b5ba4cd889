"""Epipolar search between two key frames (pislam_epipolar_from_poses, pislam_match_hamming_epipolar_batch; DESIGN.md
section 5.5).

The contract is the comment in include/pislam_hip.h.  `ref_geometry` restates the geometric half of the candidate rule in
numpy binary32, one rounding per written operation, as an nq x nt mask; `ref_epipolar_match` adds the word-guided
matcher's group rule, the masks and the levels and takes best and second on dist << 16 | j.  The CPU tests check the
restatement on hand-built anchors, the host probe (tools/probes/epipolar_host_check.cpp: the library's own arithmetic
header under the host compiler) against it bit for bit, and epipolarGeometry against numpy binary64.  The GPU tests
compare the library with the restatement exactly."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_bow as tbow
import test_grid_passes as tgp
import test_triangulate as ttri
from conftest import ROOT
from test_match_window import COUNT_INVALID, SENTINEL, clamp_count, random_descriptors
from test_match_scaled_window import hamming

F32, F64 = np.float32, np.float64
NONE = 0xFFFFFFFF
BIG = np.int64(1) << 40
MONO = -(1 << 31)
INF = float("inf")
LS8, SG8 = ttri.LS8, ttri.SG8
PARAM_FIELDS = ["chi2", "epipole_r2"]
# x1' F x2 = v2 - v1: the epipolar line of (u1, v1) is the row v2 = v1 (a = 0, b = 1, c = -v1, den = 1)
F_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F32)


# ---- the restatement -------------------------------------------------------------------------------------------------
def obs_px(q):
    return np.clip(np.asarray(q, np.int64), -(1 << 22), 1 << 22).astype(F32) * F32(1.0 / 256.0)


def ref_line(F, qobs):
    """(a, b, c, den) float32 [nq] of the queries' epipolar lines."""
    F = np.asarray(F, F32)
    qobs = np.asarray(qobs, np.int64).reshape(-1, 3)
    u1, v1 = obs_px(qobs[:, 0]), obs_px(qobs[:, 1])
    with np.errstate(all="ignore"):
        a = (u1 * F[0] + v1 * F[3]) + F[6]
        b = (u1 * F[1] + v1 * F[4]) + F[7]
        c = (u1 * F[2] + v1 * F[5]) + F[8]
        den = a * a + b * b
    assert den.dtype == F32
    return a, b, c, den


def ref_geometry(F, ep, qobs, ql, tobs, tl, sg=SG8, ls=LS8, chi2=3.84, epipole_r2=100.0):
    """dict of nq x nt masks: near (the line test), disc (inside the epipole's disc), cand (the geometric half of the rule
    with the levels: both below nlevels, near, and not (both monocular and disc)); all False when F is not finite."""
    F, ep, sg, ls = np.asarray(F, F32), np.asarray(ep, F32), np.asarray(sg, F32), np.asarray(ls, F32)
    qobs, tobs = np.asarray(qobs, np.int64).reshape(-1, 3), np.asarray(tobs, np.int64).reshape(-1, 3)
    ql, tl = np.asarray(ql, np.int64).reshape(-1), np.asarray(tl, np.int64).reshape(-1)
    nq, nt, nl = len(qobs), len(tobs), len(sg)
    out = dict(near=np.zeros((nq, nt), bool), disc=np.zeros((nq, nt), bool), cand=np.zeros((nq, nt), bool))
    if not np.isfinite(F).all():
        return out
    a, b, c, den = ref_line(F, qobs)
    u2, v2 = obs_px(tobs[:, 0]), obs_px(tobs[:, 1])
    k = np.minimum(tl, nl - 1)
    with np.errstate(all="ignore"):
        num = (a[:, None] * u2[None, :] + b[:, None] * v2[None, :]) + c[:, None]
        near = num * num < (F32(chi2) * sg[k])[None, :] * den[:, None]
        dx, dy = ep[0] - u2, ep[1] - v2
        disc = np.broadcast_to((dx * dx + dy * dy < F32(epipole_r2) * ls[k])[None, :], (nq, nt))
        assert num.dtype == F32 and dx.dtype == F32
    levels = (ql < nl)[:, None] & (tl < nl)[None, :]
    both_mono = (qobs[:, 2] == MONO)[:, None] & (tobs[:, 2] == MONO)[None, :]
    out["near"], out["disc"] = near & levels, disc & levels
    out["cand"] = levels & near & ~(both_mono & disc)
    return out


def ref_epipolar_match(qd, qg, qobs, ql, qm, td, tg, tobs, tl, tm, ngroups, F, ep, d=None, **geo):
    """(idx int32, dist uint32, dist2 uint32) [nq] of one pair, and the candidate mask."""
    nq, nt = len(qd), len(td)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE, np.uint32)
    dist2 = np.full(nq, NONE, np.uint32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2, np.zeros((nq, nt), bool)
    qg, tg = np.asarray(qg, np.int64), np.asarray(tg, np.int64)
    mask = (qg[:, None] == tg[None, :]) & (qg[:, None] < ngroups) & (tg[None, :] < ngroups)
    if qm is not None:
        mask &= (np.asarray(qm) != 0)[:, None]
    if tm is not None:
        mask &= (np.asarray(tm) != 0)[None, :]
    mask &= ref_geometry(F, ep, qobs, ql, tobs, tl, **geo)["cand"]
    if d is None:
        d = hamming(qd, td)
    key = np.where(mask, d * 65536 + np.arange(nt, dtype=np.int64)[None, :], BIG)
    rows = np.arange(nq)
    am = key.argmin(1)
    best = key[rows, am].copy()
    key[rows, am] = BIG
    second = key.min(1)
    has, has2 = best < BIG, second < BIG
    idx[:] = np.where(has, best % 65536, -1)
    dist[:] = np.where(has, best // 65536, NONE).astype(np.uint32)
    dist2[:] = np.where(has2, second // 65536, NONE).astype(np.uint32)
    return idx, dist, dist2, mask


def q8(u, v, ur=None):
    return [int(round(u * 256)), int(round(v * 256)), MONO if ur is None else int(round(ur * 256))]


def geo1(qobs, tobs, ql=0, tl=0, F=F_ROWS, ep=(np.nan, np.nan), **kw):
    g = ref_geometry(F, ep, [qobs], [ql], [tobs], [tl], **kw)
    return bool(g["cand"][0, 0]), bool(g["near"][0, 0]), bool(g["disc"][0, 0])


# ---- CPU: declarations -----------------------------------------------------------------------------------------------
def test_match_epipolar_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in ("pislam_epipolar_from_poses", "pislam_match_epipolar_reserve", "pislam_match_hamming_epipolar_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f + " is not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_epipolar_params \{([^}]*)\} pislam_epipolar_params;", code)
    assert m
    fields = []
    for ty, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", m.group(1)):
        fields += [(n.strip(), ty) for n in names.split(",")]
    assert [n for n, _ in fields] == PARAM_FIELDS and [t for _, t in fields] == ["float"] * 2
    assert "#define PISLAM_ABI_VERSION 2" in text
    assert "Not here: the baseline test that skips a key-frame pair" in text and "ORBmatcher::Fuse" in text
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_match_hamming_epipolar_batch"][1]) == 27
    assert len(capi.SYMBOLS["pislam_match_epipolar_reserve"][1]) == 5 and len(capi.SYMBOLS["pislam_epipolar_from_poses"][1]) == 6
    assert [n for n, _ in capi.EpipolarParams._fields_] == PARAM_FIELDS and ctypes.sizeof(capi.EpipolarParams) == 8
    for f in ("epipolarGeometry", "reserveMatchEpipolar", "matchEpipolarBatch", "matchedObservationPairs"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    for f in ("pislam_epipolar_from_poses", "pislam_match_epipolar_reserve", "pislam_match_hamming_epipolar_batch"):
        assert hasattr(lib, f), f
    for f in ("pislam_epipolar_math.h", "pislam_epipolar_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "pislam_amd", "csrc", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "probes", "epipolar_host_check.cpp"))
    assert "epipolar_host_check" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_new_points.py"))
    # the word-guided matcher's kernel is a sibling, not an edited copy
    bow = open(os.path.join(ROOT, "pislam_amd", "csrc", "pislam_bow_kernels.h")).read()
    assert "epipol" not in bow.lower()


# ---- CPU: hand-built anchors of the restatement ----------------------------------------------------------------------
def test_ref_line_anchors():
    a, b, c, den = ref_line(F_ROWS, [q8(30, 20)])
    assert (a[0], b[0], c[0], den[0]) == (0, 1, -20, 1)
    # a point exactly on the line is a candidate at any chi2 > 0
    assert geo1(q8(30, 20), q8(99, 20), chi2=1e-30) == (True, True, False)
    # num = 2 on level 0 (sigma2 = 1): 4 < chi2 * 1
    assert geo1(q8(30, 20), q8(99, 22), chi2=4.0) == (False, False, False)
    assert geo1(q8(30, 20), q8(99, 22), chi2=float(np.nextafter(F32(4), F32(9)))) == (True, True, False)
    assert geo1(q8(30, 20), q8(99, 18), chi2=4.0)[0] is False and geo1(q8(30, 20), q8(99, 18), chi2=4.01)[0] is True
    # num = 3 on level 2: 9 < chi2 * sigma2[2]; the two neighbouring floats of chi2 on either side of the bound
    c_hi = F32(9) / SG8[2]
    while not F32(9) < c_hi * SG8[2]:
        c_hi = np.nextafter(c_hi, F32(99))
    while F32(9) < np.nextafter(c_hi, F32(0)) * SG8[2]:
        c_hi = np.nextafter(c_hi, F32(0))
    c_lo = np.nextafter(c_hi, F32(0))
    assert c_lo * SG8[2] <= F32(9) < c_hi * SG8[2] and 4.3 < c_lo < 4.4
    assert geo1(q8(30, 20), q8(99, 23), tl=2, chi2=float(c_hi))[0] is True
    assert geo1(q8(30, 20), q8(99, 23), tl=2, chi2=float(c_lo))[0] is False
    assert geo1(q8(30, 20), q8(99, 23), tl=0, chi2=float(c_hi))[0] is False    # the TRAIN level's sigma2 counts ...
    assert geo1(q8(30, 20), q8(99, 23), ql=2, tl=0, chi2=float(c_hi))[0] is False   # ... not the query's
    # den == 0: no candidate, on the line or not, at any chi2
    zero = np.zeros(9, F32)
    for chi2 in (3.84, INF):
        assert geo1(q8(30, 20), q8(99, 20), F=zero, chi2=chi2) == (False, False, False)
    only_c = zero.copy()
    only_c[8] = 1
    assert geo1(q8(30, 20), q8(99, 20), F=only_c, chi2=INF) == (False, False, False)
    # chi2 = +inf with den > 0: every keypoint on a level
    assert geo1(q8(30, 20), q8(99, 400), chi2=INF) == (True, True, False)
    assert geo1(q8(30, 20), q8(99, 400), tl=8, chi2=INF) == (False, False, False)
    assert geo1(q8(30, 20), q8(99, 400), ql=255, chi2=INF) == (False, False, False)
    # an F that is not finite
    bad = F_ROWS.copy()
    bad[2] = np.nan
    assert geo1(q8(30, 20), q8(99, 20), F=bad, chi2=INF) == (False, False, False)


def test_ref_epipole_disc_anchors():
    """Epipole (100, 100), epipole_r2 = 100: (106, 108) is at distance 10 exactly (outside: not <), one Q8 step nearer is
    inside.  Inside excludes a pair of monocular keypoints only."""
    ep, kw = (100.0, 100.0), dict(chi2=INF, epipole_r2=100.0)
    out_, in_ = q8(106, 108), q8(106 - 1 / 256, 108)
    assert geo1(q8(5, 5), out_, ep=ep, **kw) == (True, True, False)
    assert geo1(q8(5, 5), in_, ep=ep, **kw) == (False, True, True)
    assert geo1(q8(5, 5, 3), in_, ep=ep, **kw) == (True, True, True)          # a stereo query
    assert geo1(q8(5, 5), in_[:2] + [0], ep=ep, **kw) == (True, True, True)   # a stereo train keypoint
    assert geo1(q8(5, 5, 3), in_[:2] + [77], ep=ep, **kw) == (True, True, True)
    # the disc grows with the TRAIN level's scale: level 2 (scale 1.44) takes (106, 108) in, 100 * 1.44 = 144 > 100
    assert geo1(q8(5, 5), out_, tl=2, ep=ep, **kw) == (False, True, True)
    assert geo1(q8(5, 5), q8(100, 111.75), tl=2, ep=ep, **kw) == (False, True, True)    # 138.06 < 144
    assert geo1(q8(5, 5), q8(100, 112.25), tl=2, ep=ep, **kw) == (True, True, False)    # 150.06
    # epipole_r2 = 0 excludes nothing, nor does an epipole that is not finite
    assert geo1(q8(5, 5), q8(100, 100), ep=ep, chi2=INF, epipole_r2=0.0) == (True, True, False)
    for e in ((np.nan, 100.0), (100.0, np.nan), (np.inf, 100.0), (-np.inf, np.inf)):
        assert geo1(q8(5, 5), q8(100, 100), ep=e, **kw) == (True, True, False), e


def test_ref_match_groups_masks_and_ties():
    """Four train keypoints on the query's row, one off it; groups, masks and the tie rule on a hand-built pair."""
    td = np.array([[0b111], [0b1], [0b1], [0], [0]], np.uint32)
    tobs = [q8(10, 20), q8(50, 20), q8(70, 21), q8(90, 20), q8(90, 30)]
    tg, tl = [1, 1, 1, 2, 1], [0, 0, 0, 0, 0]
    qd, qobs = np.zeros((2, 1), np.uint32), [q8(5, 20), q8(5, 20)]
    run = lambda qg, qm=None, tm=None, ql=(0, 0), **kw: [v.tolist() for v in ref_epipolar_match(
        qd, qg, qobs, list(ql), qm, td, tg, tobs, tl, tm, 3, F_ROWS, (np.nan, np.nan), **kw)[:3]]
    assert run([1, 2]) == [[1, 3], [1, 0], [1, NONE]]          # train 1 and 2 tie at distance 1: the smaller index
    assert run([1, 2], chi2=0.9) == [[1, 3], [1, 0], [3, NONE]]   # train 2 is a pixel off the row
    assert run([1, 2], chi2=101.0) == [[4, 3], [0, 0], [1, NONE]]  # train 4, ten rows off, comes in
    assert run([1, 3]) == [[1, -1], [1, NONE], [1, NONE]]      # group 3 is no group
    assert run([1, 2], qm=[0, 1]) == [[-1, 3], [NONE, 0], [NONE, NONE]]
    assert run([1, 2], tm=[1, 0, 1, 1, 1]) == [[2, 3], [1, 0], [3, NONE]]
    assert run([1, 2], ql=(8, 0)) == [[-1, 3], [NONE, 0], [NONE, NONE]]


# ---- CPU: epipolarGeometry against numpy binary64 ---------------------------------------------------------------------
def ref_epipolar_from_poses(pose1, pose2, cam1, cam2):
    """float64 (F12 [9], epipole [2]) from float32 inputs, by the textbook formulas."""
    p1, p2 = np.asarray(pose1, F32).astype(F64), np.asarray(pose2, F32).astype(F64)
    c1, c2 = np.asarray(cam1, F32).astype(F64), np.asarray(cam2, F32).astype(F64)
    R1, t1, R2, t2 = p1[:9].reshape(3, 3), p1[9:], p2[:9].reshape(3, 3), p2[9:]
    K = lambda c: np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1]])
    R12 = R1 @ R2.T
    t12 = t1 - R12 @ t2
    S = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Fm = np.linalg.inv(K(c1)).T @ S @ R12 @ np.linalg.inv(K(c2))
    C = R2 @ (-R1.T @ t1) + t2
    with np.errstate(all="ignore"):
        e = np.array([c2[0] * C[0] / C[2] + c2[2], c2[1] * C[1] / C[2] + c2[3]])
    return Fm.reshape(-1), e


def ulp32(v):
    v = np.abs(np.asarray(v, F64)).astype(F32)
    return (np.nextafter(v, F32(np.inf)) - v).astype(F64)


def test_epipolar_geometry_against_binary64():
    from pislam_amd.frontend import epipolarGeometry
    rng = np.random.default_rng(3)
    poses1, poses2, cams1, cams2 = [], [], [], []
    for i in range(200):
        p1, p2, c1, c2 = ttri.random_pair(rng, 3 if i % 4 == 0 else 0)
        poses1.append(p1), poses2.append(p2), cams1.append(c1), cams2.append(c2)
    f12, ep = epipolarGeometry(np.stack(poses1), np.stack(poses2), np.stack(cams1), np.stack(cams2))
    assert f12.dtype == F32 and f12.shape == (200, 9) and ep.shape == (200, 2)
    for b in range(200):
        Fm, e = ref_epipolar_from_poses(poses1[b], poses2[b], cams1[b], cams2[b])
        assert np.abs(f12[b].astype(F64) - Fm).max() <= ulp32(np.abs(Fm).max()), b
        assert (np.abs(ep[b].astype(F64) - e) <= ulp32(e)).all(), (b, ep[b], e)
        # x1' F12 x2 = 0 for a point both cameras see
        X = rng.uniform(-1, 1, 3) + np.array([0, 0, 6.0])
        Xw = (X - poses1[b][9:].astype(F64)) @ poses1[b][:9].astype(F64).reshape(3, 3)
        (o1, _), (o2, _) = ttri.project(poses1[b], cams1[b].astype(F64), Xw[None]), ttri.project(poses2[b], cams2[b].astype(F64), Xw[None])
        x1, x2 = np.array([o1[0, 0], o1[0, 1], 1]), np.array([o2[0, 0], o2[0, 1], 1])
        Fd = f12[b].astype(F64).reshape(3, 3)
        line = Fd.T @ x1
        assert abs(line @ x2) / np.hypot(line[0], line[1]) < 1e-2, b       # pixels
    # one pair, tensors or arrays, [5]-word cameras; refusals come back as NaN rows
    f1, e1 = epipolarGeometry(poses1[0], poses2[0], cams1[0], cams2[0])
    assert f1.shape == (9,) and (f1.view(np.uint32) == f12[0].view(np.uint32)).all() and (e1 == ep[0]).all()
    bad = poses1[1].copy()
    bad[3] = np.inf
    zero = cams2[2].copy()
    zero[1] = 0
    f, e = epipolarGeometry(np.stack([bad, poses1[2]]), np.stack([poses2[1], poses2[2]]), np.stack([cams1[1], cams1[2]]),
                            np.stack([cams2[1], zero]))
    assert np.isnan(f).all() and np.isnan(e).all()
    # the same place: t12 = 0, F = 0 up to rounding, and the epipole is 0 / 0 or far away: returned as it comes out
    same = epipolarGeometry(ttri.IDENTITY, ttri.IDENTITY, cams1[0], cams2[0])
    assert not same[0].any() and np.isnan(same[1]).all()
    from pislam_amd import capi
    fp = ctypes.POINTER(ctypes.c_float)
    buf = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(fp)
    out9, out2 = np.zeros(9, F32), np.zeros(2, F32)
    args = [buf(poses1[0]), buf(poses2[0]), buf(cams1[0][:4]), buf(cams2[0][:4]), out9.ctypes.data_as(fp), out2.ctypes.data_as(fp)]
    assert capi.load().pislam_epipolar_from_poses(*args) == 0
    for k in range(6):
        assert capi.load().pislam_epipolar_from_poses(*[None if i == k else a for i, a in enumerate(args)]) == -1


# ---- CPU: the host probe against the restatement ---------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(np.asarray(a, F32)).reshape(-1).view(np.uint32))


def probe_line(e):
    return " ".join(["%d %d %d" % (len(e["sg"]), e["ql"], e["tl"]), " ".join(str(int(v)) for v in e["qobs"]),
                     " ".join(str(int(v)) for v in e["tobs"]), hexf(e["F"]), hexf(e["ep"]), hexf(e["sg"]), hexf(e["ls"]),
                     hexf([e["chi2"], e["epipole_r2"]])])


def pair_geometry(rng, kind=0):
    """A random key-frame pair with its float32 F12 and epipole (numpy binary64, rounded)."""
    p1, p2, c1, c2 = ttri.random_pair(rng, kind)
    Fm, e = ref_epipolar_from_poses(p1, p2, c1, c2)
    return p1, p2, c1, c2, Fm.astype(F32), e.astype(F32)


def views(rng, p1, p2, c1, c2, n):
    """Q8 observations (u, v, u_right) of n random points in both key frames, and the points."""
    z = rng.uniform(1.5, 25, n)
    Xc = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    P1 = p1.astype(F64)
    X = (Xc - P1[9:]) @ P1[:9].reshape(3, 3)
    (o1, z1), (o2, z2) = ttri.project(p1, c1.astype(F64), X), ttri.project(p2, c2.astype(F64), X)
    toq = lambda o: np.clip(np.round(np.nan_to_num(o) * 256), -(1 << 30), 1 << 30).astype(np.int64)
    return toq(o1), toq(o2), X


def random_elements(n, seed):
    """Elements of the probe: a query and a train keypoint that see the same point (a few pixels apart from the line in
    turn), or unrelated ones; keypoints at the epipole; levels past the table; an F that is not finite or zero."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p1, p2, c1, c2, F, ep = pair_geometry(rng, 3 if i % 3 == 0 else 0)
        nl = int(rng.integers(1, 9)) if i % 5 == 0 else 8
        ls, sg = ttri.level_tables(nl, rng.uniform(1.1, 1.5))
        o1, o2, _ = views(rng, p1, p2, c1, c2, 2)
        qobs, tobs = o1[0], o2[0 if i % 4 else 1]
        tobs[:2] += np.round(rng.normal(0, [0.0, 1.0, 3.0, 10.0][i % 4] * 256, 2)).astype(np.int64)
        if i % 3 == 0 and np.isfinite(ep).all() and i % 2:
            tobs[:2] = np.round(ep.astype(F64) * 256 + rng.normal(0, 8 * 256, 2)).astype(np.int64)
        qobs[2] = MONO if rng.random() < 0.6 else qobs[2]
        tobs[2] = MONO if rng.random() < 0.6 else tobs[2]
        e = dict(F=F, ep=ep, qobs=qobs.tolist(), tobs=tobs.tolist(), ql=int(rng.integers(0, nl + (i % 7 == 0))),
                 tl=int(rng.integers(0, nl + (i % 11 == 0) * 3)), sg=sg, ls=ls, chi2=[3.84, 3.84, 50.0, INF][i % 4],
                 epipole_r2=[100.0, 0.0, 400.0][i % 3])
        if i % 53 == 0:
            e["F"] = F.copy()
            e["F"][int(rng.integers(0, 9))] = [np.nan, np.inf][i % 2]
        if i % 59 == 0:
            e["F"] = np.zeros(9, F32)
        if i % 61 == 0:
            e["ep"] = np.array([np.nan, ep[1]], F32)
        out.append(e)
    return out


def element_verdict(e):
    g = ref_geometry(e["F"], e["ep"], [e["qobs"]], [e["ql"]], [e["tobs"]], [e["tl"]], e["sg"], e["ls"], e["chi2"], e["epipole_r2"])
    live = np.isfinite(np.asarray(e["F"], F32)).all() and e["ql"] < len(e["sg"]) and e["tl"] < len(e["sg"])
    line = ref_line(e["F"], [e["qobs"]]) if live else [np.zeros(1, F32)] * 4
    return g, live, "%d %d %d %s" % (g["cand"][0, 0], g["near"][0, 0], g["disc"][0, 0], hexf([v[0] for v in line]))


@pytest.fixture(scope="module")
def run_probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("epipolar_probe") / "epipolar_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "epipolar_host_check.cpp"), "-o", exe])

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def test_probe_equals_the_restatement(run_probe):
    """2400 random elements; as a precondition they hold both outcomes of every test of the candidate rule."""
    cases = random_elements(2400, 17)
    got = run_probe([probe_line(e) for e in cases])
    tally = dict(live=[0, 0], near=[0, 0], disc=[0, 0], excluded=[0, 0], cand=[0, 0], den0=[0, 0], ep_finite=[0, 0])
    for e, g in zip(cases, got):
        r, live, want = element_verdict(e)
        assert g == want, (e, g, want)
        tally["live"][int(live)] += 1
        if live:
            both = e["qobs"][2] == MONO and e["tobs"][2] == MONO
            tally["near"][int(r["near"][0, 0])] += 1
            tally["disc"][int(r["disc"][0, 0])] += 1
            tally["cand"][int(r["cand"][0, 0])] += 1
            tally["ep_finite"][int(np.isfinite(e["ep"]).all())] += 1
            tally["den0"][int(ref_line(e["F"], [e["qobs"]])[3][0] == 0)] += 1
            if r["near"][0, 0] and r["disc"][0, 0]:
                tally["excluded"][int(both)] += 1
    print(tally)
    assert all(min(v) >= 10 for v in tally.values()), tally


# ---- running the library ---------------------------------------------------------------------------------------------
S32 = SENTINEL - (1 << 32) if SENTINEL >= 1 << 31 else SENTINEL
NAMES = ("idx", "dist", "dist2")
GEO = dict(sg=SG8, ls=LS8, chi2=3.84, epipole_r2=100.0)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


KEYS = ("qd", "qg", "qobs", "ql", "qc", "td", "tg", "tobs", "tl", "tc", "F", "ep", "qm", "tm")


def device_case(c):
    return {k: None if c.get(k) is None else to_dev(c[k]) for k in KEYS}


def run_epipolar(ctx, c, dev=None, masks=True, **geo):
    """Host arrays in, (idx, dist, dist2) uint32 out; every output is pre-filled with the sentinel."""
    import torch
    from pislam_amd.frontend import matchEpipolarBatch
    t = dev or device_case(c)
    g = dict(GEO, **geo)
    B, qs = c["qg"].shape
    outs = [torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    matchEpipolarBatch(t["qd"], t["qg"], t["qobs"], t["ql"], t["qc"], t["td"], t["tg"], t["tobs"], t["tl"], t["tc"],
                       c["ngroups"], t["F"], t["ep"], qmask=t["qm"] if masks else None, tmask=t["tm"] if masks else None,
                       level_sigma2=g["sg"], level_scale=g["ls"], chi2=g["chi2"], epipole_r2=g["epipole_r2"], idx=outs[0],
                       dist=outs[1], dist2=outs[2], ctx=ctx)
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in outs]


def ref_call(c, pairs=None, masks=True, hams=None, **geo):
    """(idx, dist, dist2) uint32 [B][qs] with the sentinel where nothing is written, and the candidates per pair."""
    g = dict(GEO, **geo)
    B, qs = c["qg"].shape
    ts = c["tg"].shape[1]
    outs = [np.full((B, qs), SENTINEL, np.uint32) for _ in range(3)]
    ncand = np.zeros(B, np.int64)
    for b in (range(B) if pairs is None else pairs):
        nq, nt = clamp_count(c["qc"][b], qs), clamp_count(c["tc"][b], ts)
        qm = c["qm"][b, :nq] if masks and c.get("qm") is not None else None
        tm = c["tm"][b, :nt] if masks and c.get("tm") is not None else None
        i, d, d2, m = ref_epipolar_match(c["qd"][b, :nq], c["qg"][b, :nq], c["qobs"][b, :nq], c["ql"][b, :nq], qm, c["td"][b, :nt],
                                         c["tg"][b, :nt], c["tobs"][b, :nt], c["tl"][b, :nt], tm, c["ngroups"], c["F"][b],
                                         c["ep"][b], d=None if hams is None else hams[b][:nq, :nt], sg=g["sg"], ls=g["ls"],
                                         chi2=g["chi2"], epipole_r2=g["epipole_r2"])
        outs[0][b, :nq], outs[1][b, :nq], outs[2][b, :nq] = i.view(np.uint32), d, d2
        ncand[b] = int(m.sum())
    return outs, ncand


def assert_outputs(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def pins_case(words, B=3, qs=200, ts=300, ngroups=7, seed=0):
    """B key-frame pairs: the train keypoints are views of random points in key frame 2 (a pixel of noise), the queries
    views of the same points in key frame 1 (two in three, with the train descriptor and a few flipped bits) or unrelated.
    Groups: 5 is empty on the train side, 6 holds one train entry, 0 holds a quarter of them; ids at and above ngroups on
    both sides; a twentieth of the levels is 255; a third of the keypoints is stereo; masks drop a fifth."""
    rng = np.random.default_rng([61, seed, words])
    c = dict(ngroups=ngroups, qd=np.zeros((B, qs, words), np.uint32), td=np.zeros((B, ts, words), np.uint32),
             qg=np.zeros((B, qs), np.uint32), tg=np.zeros((B, ts), np.uint32), qobs=np.zeros((B, qs, 3), np.int32),
             tobs=np.zeros((B, ts, 3), np.int32), ql=np.zeros((B, qs), np.uint8), tl=np.zeros((B, ts), np.uint8),
             qm=np.zeros((B, qs), np.uint8), tm=np.zeros((B, ts), np.uint8), qc=np.full(B, qs, np.uint32),
             tc=np.full(B, ts, np.uint32), F=np.zeros((B, 9), F32), ep=np.zeros((B, 2), F32))
    for b in range(B):
        p1, p2, c1, c2, c["F"][b], c["ep"][b] = pair_geometry(rng, 3 if b % 3 == 1 else 0)
        o1, o2, _ = views(rng, p1, p2, c1, c2, ts)
        o2[:, :2] += np.round(rng.normal(0, 256, (ts, 2))).astype(np.int64)
        tg = rng.choice(np.array([0, 0, 1, 2, 3, 4, ngroups, ngroups + 3, NONE], np.int64), ts)
        tg[7] = 6
        j = rng.integers(0, ts, qs)
        own = rng.random(qs) < 0.67
        stray, _, _ = views(rng, p1, p2, c1, c2, qs)
        c["qobs"][b] = np.where(own[:, None], o1[j], stray)
        c["tobs"][b] = o2
        c["qg"][b] = np.where(own, tg[j], rng.integers(0, ngroups + 2, qs))
        c["tg"][b] = tg
        c["td"][b] = random_descriptors(rng, ts, words)
        flip = (np.uint32(1) << rng.integers(0, 32, (qs, words)).astype(np.uint32)) * (rng.random((qs, words)) < 0.5)
        c["qd"][b] = np.where(own[:, None], c["td"][b][j] ^ flip.astype(np.uint32), random_descriptors(rng, qs, words))
        c["ql"][b] = np.where(rng.random(qs) < 0.05, 255, rng.integers(0, 8, qs))
        c["tl"][b] = np.where(rng.random(ts) < 0.05, 255, rng.integers(0, 8, ts))
        c["qobs"][b, rng.random(qs) < 0.67, 2] = MONO
        c["tobs"][b, rng.random(ts) < 0.67, 2] = MONO
        c["qm"][b] = rng.random(qs) < 0.8
        c["tm"][b] = (rng.random(ts) < 0.8) * rng.integers(1, 256, ts)
    return c


def test_pins_precondition():
    """The pins are not trivial (numpy only): group 0 is longer than three walks of a query's lanes, group 5 is empty and
    group 6 holds one entry; the line test, the disc and the masks each remove candidates the word-guided matcher has."""
    c = pins_case(2)
    for b in range(3):
        n = np.bincount(c["tg"][b][c["tg"][b] < 7].astype(np.int64), minlength=7)
        assert n[0] > 4 * 3 * 4 and n[5] == 0 and n[6] == 1, n
        assert (c["qg"][b] == 6).any() and (c["qg"][b] == 5).any() and (c["qg"][b] >= 7).any()
        assert (c["ql"][b] == 255).any() and (c["tl"][b] == 255).any()
    (idx, dist, dist2), ncand = ref_call(c)
    wide, nwide = ref_call(c, chi2=300.0, epipole_r2=2500.0)
    bow, nbow = ref_call(c, masks=False, chi2=INF, epipole_r2=0.0)
    nomask, nnomask = ref_call(c, masks=False)
    print("candidates", ncand, nwide, nnomask, nbow)
    assert (ncand > 30).all() and (nwide > 2 * ncand).all() and (nnomask > ncand).all() and (nbow > 4 * nwide).all()
    assert (idx.view(np.int32)[:, :200] >= 0).sum() > 60 and (wide[2] != NONE).sum() > 60
    # the disc matters in the forward-moving pair: the epipole lies in the image
    far, nfar = ref_call(c, chi2=300.0, epipole_r2=0.0)
    assert nfar[1] > nwide[1], (nfar, nwide)


# ---- GPU: pins -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_epipolar_pins(gpu_ctx, words):
    """Batch 3, q_stride 200, t_stride 300, 7 groups: two parameter sets, masks given and NULL."""
    c = pins_case(words)
    hams = [hamming(c["qd"][b], c["td"][b]) for b in range(3)]
    dev = device_case(c)
    for geo in (dict(), dict(chi2=300.0, epipole_r2=2500.0), dict(chi2=INF, epipole_r2=0.0)):
        for masks in (True, False):
            want, ncand = ref_call(c, masks=masks, hams=hams, **geo)
            assert (ncand > 20).all()
            assert_outputs(run_epipolar(gpu_ctx, c, dev, masks=masks, **geo), want, (words, geo, masks))


@pytest.mark.gpu
def test_gpu_epipolar_counts_and_slots(gpu_ctx):
    """Counts of 0, PISLAM_COUNT_INVALID and above the stride on both sides, a pair whose F is not finite, a pair whose F is
    zero; the sentinel stays at and beyond each query count."""
    base = pins_case(2, B=8, seed=2)
    qs, ts = 200, 300
    c = dict(base, qc=np.array([COUNT_INVALID, qs + 5, 0, 37, qs, 10, qs, qs], np.uint32),
             tc=np.array([ts, ts + 9, ts, COUNT_INVALID, 0, 5, ts, ts], np.uint32), F=base["F"].copy())
    c["F"][6, 4] = np.inf
    c["F"][7] = 0
    want, ncand = ref_call(c)
    idx = want[0].view(np.int32)
    assert (want[0][0] == SENTINEL).all() and (want[0][2] == SENTINEL).all() and (want[0][3, 37:] == SENTINEL).all()
    assert (idx[3, :37] == -1).all() and (idx[4] == -1).all() and (idx[6] == -1).all() and (idx[7] == -1).all()
    assert (idx[1] >= 0).any() and ncand[1] > 30
    assert_outputs(run_epipolar(gpu_ctx, c), want)


# ---- GPU: the two degenerate equalities --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 8])
def test_gpu_epipolar_equals_the_word_guided_matcher(gpu_ctx, words):
    """chi2 = +inf, epipole_r2 = 0, NULL masks, every level valid and den > 0 for every query: the word-guided matcher's
    outputs word for word (library against library), which in turn equal its own restatement."""
    c = dict(pins_case(words, seed=3))
    c["ql"], c["tl"] = c["ql"] % 8, c["tl"] % 8
    for b in range(3):
        assert (ref_line(c["F"][b], c["qobs"][b])[3] > 0).all()
    got = run_epipolar(gpu_ctx, c, masks=False, chi2=INF, epipole_r2=0.0)
    bow = tbow.run_bow_match(gpu_ctx, c["ngroups"], c["qd"], c["qg"], c["qc"], c["td"], c["tg"], c["tc"])
    assert_outputs(got, bow)
    tbow.check_bow_match(got, c["ngroups"], c["qd"], c["qg"], c["qc"], c["td"], c["tg"], c["tc"])
    assert (got[0].view(np.int32) >= 0).sum() > 300


@pytest.mark.gpu
def test_gpu_epipolar_masked_queries_have_no_match(gpu_ctx):
    c = dict(pins_case(2, seed=4))
    c["qm"] = c["qm"].copy()
    c["qm"][1] = 0
    got = run_epipolar(gpu_ctx, c)
    dead = c["qm"] == 0
    assert dead.sum() > 250
    assert (got[0].view(np.int32)[dead] == -1).all() and (got[1][dead] == NONE).all() and (got[2][dead] == NONE).all()
    assert_outputs(got, ref_call(c)[0])


# ---- GPU: more than one grid pass ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_epipolar_more_queries_than_one_grid_pass(gpu_ctx):
    """k_match_epipolar at batch 1024, stride 1024, 40 groups, on the word-guided matcher's case of test_grid_passes.py
    with rows as epipolar lines: slot kind 0 has a group id that is no group, 1 is a copy of a train entry below the
    count (descriptor, group and row), 2 has a random group, descriptor and row."""
    B, qs, ts, ngroups = 1024, 1024, 300, 40
    P = tgp.guided_pass(qs, 64, B)
    tgp.need_three_passes(qs, P, "k_match_epipolar")
    rng = np.random.default_rng([9, P])
    counts = tgp.pass_counts(P, qs)
    pairs = tgp.spread(B, len(counts))
    c = dict(ngroups=ngroups, qd=np.zeros((B, qs, 1), np.uint32), td=np.zeros((B, ts, 1), np.uint32),
             qg=np.zeros((B, qs), np.uint32), tg=np.zeros((B, ts), np.uint32), qobs=np.zeros((B, qs, 3), np.int32),
             tobs=np.zeros((B, ts, 3), np.int32), ql=np.zeros((B, qs), np.uint8), tl=np.zeros((B, ts), np.uint8),
             qc=np.zeros(B, np.uint32), tc=np.zeros(B, np.uint32), F=np.tile(F_ROWS, (B, 1)),
             ep=np.tile(np.array([40, 8], F32), (B, 1)))
    c["qc"][pairs] = counts
    c["tc"][pairs] = [ts, ts - 1, 257, ts + 9, COUNT_INVALID, ts, 65, ts, ts, ts]
    kind = tgp.slot_kinds(qs, P, 3)
    rows = lambda n: np.stack([rng.integers(0, 100, n) * 256, rng.integers(0, 6, n) * 2048, np.where(rng.random(n) < 0.5, MONO, 0)], 1)
    for b in pairs:
        nt = clamp_count(c["tc"][b], ts)
        c["td"][b], c["tg"][b], c["tobs"][b] = random_descriptors(rng, ts, 1), rng.integers(0, ngroups, ts), rows(ts)
        c["qd"][b], c["qg"][b], c["qobs"][b] = random_descriptors(rng, qs, 1), rng.integers(0, ngroups + 4, qs), rows(qs)
        c["qg"][b, kind == 0] = rng.choice(np.array([ngroups, ngroups + 9, 0x80000000, NONE], np.uint32), qs)[kind == 0]
        c["tl"][b], c["ql"][b] = rng.integers(0, 8, ts), rng.integers(0, 8, qs)
        if nt:
            j = rng.integers(0, nt, qs)
            k1 = kind == 1
            c["qd"][b, k1], c["qg"][b, k1], c["qobs"][b, k1] = c["td"][b, j][k1], c["tg"][b, j][k1], c["tobs"][b, j][k1]
    empty = np.setdiff1d(np.arange(B), pairs)
    c["tc"][empty[::5]] = ts
    got = run_epipolar(gpu_ctx, c)
    want, ncand = ref_call(c, pairs=pairs)
    bow, nbow = ref_call(c, pairs=pairs, chi2=INF, epipole_r2=0.0)
    assert ncand[0] > 1000 and nbow[0] > 3 * ncand[0]
    assert_outputs([g[pairs] for g in got], [w[pairs] for w in want])
    tgp.assert_empty_pairs_untouched(got, pairs, B)
    tgp.check_guided_third_pass(got, dict(pairs=pairs), P, qs)


# ---- GPU: offsets beyond 4 GiB ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_epipolar_offsets_beyond_4_gib(gpu_ctx):
    """q_stride 16384 and 21848 pairs: the query observations (12 bytes each) of the last pairs begin beyond 2^32 bytes,
    the outputs of the last third beyond 2^32 / 4 words.  Every array is allocated in one piece, uninitialised; all
    counts are 0 except the first and the last pair's, so no other pair's keypoints are ever read."""
    import torch
    from pislam_amd.frontend import matchEpipolarBatch
    B, qs, ts, words, n = 21848, 16384, 300, 1, 150
    assert (B - 1) * qs * 12 > 1 << 32
    need = B * qs * (12 + 4 * words + 4 + 1 + 3 * 4) + B * ts * (12 + 4 * words + 4 + 1) * 2
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the buffers above 4 GiB do not fit the free device memory")
    small = pins_case(words, B=2, qs=n, ts=ts, seed=5)
    dev = "cuda:0"
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    qobs, qd, qg, ql = e((B, qs, 3), torch.int32), e((B, qs, words), torch.int32), e((B, qs), torch.int32), e((B, qs), torch.uint8)
    tobs, td, tg, tl = e((B, ts, 3), torch.int32), e((B, ts, words), torch.int32), e((B, ts), torch.int32), e((B, ts), torch.uint8)
    qc, tc = torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
    F, ep = torch.zeros((B, 9), dtype=torch.float32, device=dev), torch.zeros((B, 2), dtype=torch.float32, device=dev)
    outs = [e((B, qs), torch.int32) for _ in range(3)]
    live = [0, B - 1]
    for k, b in enumerate(live):
        qobs[b, :n], qd[b, :n], qg[b, :n], ql[b, :n] = (to_dev(small[x][k]) for x in ("qobs", "qd", "qg", "ql"))
        tobs[b], td[b], tg[b], tl[b] = (to_dev(small[x][k]) for x in ("tobs", "td", "tg", "tl"))
        F[b], ep[b] = to_dev(small["F"][k]), to_dev(small["ep"][k])
        qc[b], tc[b] = n, ts
        for o in outs:
            o[b, :n + 16] = S32
    for o in outs:
        o[B - 2, :16] = S32
    matchEpipolarBatch(qd, qg, qobs, ql, qc, td, tg, tobs, tl, tc, small["ngroups"], F, ep, level_sigma2=SG8, level_scale=LS8,
                       chi2=300.0, epipole_r2=100.0, idx=outs[0], dist=outs[1], dist2=outs[2], ctx=gpu_ctx)
    torch.cuda.synchronize()
    want, ncand = ref_call(dict(small, qc=np.array([n, n], np.uint32)), masks=False, chi2=300.0)
    assert (ncand > 50).all()
    for k, b in enumerate(live):
        for name, o, w in zip(NAMES, outs, want):
            g = o[b, :n + 16].cpu().numpy().view(np.uint32)
            assert (g[:n] == w[k, :n]).all(), (name, b)
            assert (g[n:] == SENTINEL).all(), (name, "written past the count")
    for o in outs:
        assert (o[B - 2, :16] == S32).all()


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_epipolar_refusals_write_nothing(gpu_ctx):
    import torch
    from pislam_amd import capi
    from pislam_amd.frontend import matchEpipolarBatch, reserveMatchEpipolar
    c = pins_case(1)
    t = device_case(c)
    B, qs = c["qg"].shape
    outs = dict(idx=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"),
                dist=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"),
                dist2=torch.full((B, qs), S32, dtype=torch.int32, device="cuda:0"))

    def call(**over):
        a, o = dict(t), dict(outs)
        kw = dict(level_sigma2=SG8, level_scale=LS8, chi2=3.84, epipole_r2=100.0, ngroups=c["ngroups"])
        for k in list(over):
            if k in a:
                a[k] = over.pop(k)
            elif k in o:
                o[k] = over.pop(k)
        kw.update(over)
        ng = kw.pop("ngroups")
        matchEpipolarBatch(a["qd"], a["qg"], a["qobs"], a["ql"], a["qc"], a["td"], a["tg"], a["tobs"], a["tl"], a["tc"], ng,
                           a["F"], a["ep"], qmask=a["qm"], tmask=a["tm"], ctx=gpu_ctx, **kw, **o)

    nan = float("nan")
    ls, sg = LS8.tolist(), SG8.tolist()
    bad = {"host_" + k: {k: t[k].cpu()} for k in KEYS}
    bad.update({"host_" + k: {k: outs[k].cpu()} for k in outs})
    bad.update(
        sigma_zero=dict(level_sigma2=[0.0] + sg[1:]), sigma_nan=dict(level_sigma2=sg[:7] + [nan]),
        sigma_inf=dict(level_sigma2=sg[:7] + [INF]), scale_zero=dict(level_scale=[0.0] + ls[1:]),
        scale_negative=dict(level_scale=[-1.0] + ls[1:]), scale_falls=dict(level_scale=ls[:3] + [ls[1]] + ls[4:]),
        scale_nan=dict(level_scale=ls[:7] + [nan]), scale_inf=dict(level_scale=ls[:7] + [INF]),
        chi2_zero=dict(chi2=0.0), chi2_negative=dict(chi2=-3.84), chi2_nan=dict(chi2=nan), r2_negative=dict(epipole_r2=-1.0),
        r2_nan=dict(epipole_r2=nan), ngroups_zero=dict(ngroups=0), ngroups_large=dict(ngroups=16385),
        t_stride=dict(td=torch.zeros((B, 65536, 1), dtype=torch.int32, device="cuda:0"),
                      tg=torch.zeros((B, 65536), dtype=torch.int32, device="cuda:0"),
                      tobs=torch.zeros((B, 65536, 3), dtype=torch.int32, device="cuda:0"),
                      tl=torch.zeros((B, 65536), dtype=torch.uint8, device="cuda:0"),
                      tm=torch.ones((B, 65536), dtype=torch.uint8, device="cuda:0")))
    call()                                                                   # the unmodified call is accepted ...
    call(chi2=INF, epipole_r2=INF)                                           # ... and so are infinite bounds
    torch.cuda.synchronize()
    assert (outs["idx"] != S32).all()
    for o in outs.values():
        o.fill_(S32)
    for name, over in bad.items():
        with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
            call(**over)
    # NULL where a pointer is required, tables of 0 and 17 entries, words 3: through the C interface
    p = capi.EpipolarParams(3.84, 100.0)
    tab = (ctypes.c_float * 17)(*(sg + [30.0] * 9))
    lst = (ctypes.c_float * 17)(*(ls + [5.0] * 9))
    order = ("F", "ep", "qd", "qg", "qobs", "ql", "qm", "qc")
    torder = ("td", "tg", "tobs", "tl", "tm", "tc")

    def raw(drop=None, p=ctypes.byref(p), tab=tab, lst=lst, nl=8, words=1, batch=B):
        v = lambda k: None if k == drop else capi.ptr((t[k] if k in t else outs[k]))
        return gpu_ctx.lib.pislam_match_hamming_epipolar_batch(
            gpu_ctx.h, words, c["ngroups"], p, tab, lst, nl, *[v(k) for k in order], qs, *[v(k) for k in torder], 300, batch,
            v("idx"), v("dist"), v("dist2"))
    assert raw(batch=0) == 0
    for k in order + torder + NAMES:
        assert raw(drop=k) == (0 if k in ("qm", "tm") else -1), k
    torch.cuda.synchronize()
    for o in outs.values():
        o.fill_(S32)
    assert raw(p=None) == -1 and raw(tab=None) == -1 and raw(lst=None) == -1 and raw(nl=0) == -1 and raw(nl=17) == -1
    assert raw(words=3) == -1 and raw(batch=-1) == -1 and raw(batch=65536) == -1
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert (o == S32).all(), ("a refused call wrote", k)
    with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
        reserveMatchEpipolar(7, 65536, B, words=1, ctx=gpu_ctx)
    with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
        reserveMatchEpipolar(0, 300, B, words=1, ctx=gpu_ctx)


# ---- GPU: hipGraph, determinism --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_epipolar_is_hipgraph_capturable(gpu_ctx):
    """After the reserve the call allocates nothing and never synchronises: captured on a side stream with a context of
    its own, the replay equals the eager call; the graph keeps the host tables it was captured with."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchEpipolarBatch, reserveMatchEpipolar
    c = pins_case(8)
    want, _ = ref_call(c)
    t = device_case(c)
    B, qs = c["qg"].shape
    dev = torch.device("cuda:0")
    sg, ls = SG8.copy(), LS8.copy()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchEpipolar(c["ngroups"], 300, B, words=8, ctx=ctx)
        outs = [torch.zeros((B, qs), dtype=torch.int32, device=dev) for _ in range(3)]

        def call(o=(None, None, None)):
            return matchEpipolarBatch(t["qd"], t["qg"], t["qobs"], t["ql"], t["qc"], t["td"], t["tg"], t["tobs"], t["tl"],
                                      t["tc"], c["ngroups"], t["F"], t["ep"], qmask=t["qm"], tmask=t["tm"], level_sigma2=sg,
                                      level_scale=ls, idx=o[0], dist=o[1], dist2=o[2], ctx=ctx)

        eager = call()                                                       # warm-up (module load) and the eager result
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(outs)
        for o in outs:
            o.zero_()
        sg[:] = 1000.0                                                       # the graph holds its own copy of the tables
        ls[:] = 7.0
        g.replay()
        side.synchronize()
        for a, o, k in zip(eager, outs, NAMES):
            assert torch.equal(a, o), k
    for k, o, w in zip(NAMES, outs, want):
        assert (o.cpu().numpy().view(np.uint32) == w).all(), k


@pytest.mark.gpu
def test_gpu_epipolar_is_deterministic_across_calls_and_paddings(gpu_ctx):
    """Two calls give identical words, and so do two paddings of both strides (another launch shape, another index)."""
    c = pins_case(8, seed=6)
    first = run_epipolar(gpu_ctx, c)
    assert_outputs(run_epipolar(gpu_ctx, c), first)
    B, qs = c["qg"].shape
    wide = dict(c)
    for k in KEYS:
        if c.get(k) is None or k in ("qc", "tc", "F", "ep"):
            continue
        stride = c[k].shape[1] + (333 if k[0] == "q" else 77)
        a = np.zeros((B, stride) + c[k].shape[2:], c[k].dtype)
        a[:, :c[k].shape[1]] = c[k]
        wide[k] = a
    padded = run_epipolar(gpu_ctx, wide)
    for name, g, w in zip(NAMES, padded, first):
        assert (g[:, :qs] == w).all(), name
        assert (g[:, qs:] == SENTINEL).all(), name


# ---- the chain: words -> epipolar match both ways -> select -> gather -> triangulate -> projection search -------------
CHAIN_CAM = np.array([500, 500, 320, 240, 0], F32)
CHAIN_SELECT = dict(max_dist=60, ratio=(9, 10), unique=1, rot_keep=0)


@functools.lru_cache(maxsize=None)
def chain_scene(n=400):
    """Two key frames 0.8 units apart and a third frame between them see n points at 3.6 .. 9 units through a 640 x 480
    camera with the demo pyramid (8 levels x 1.2).  A point's keypoint lies on the level its depth predicts, at the
    nearest pixel of that level; its descriptor has 10 bits flipped per view.  Every fourth point has a decoy in key
    frame 2: a keypoint 40 .. 80 pixels off the point's own row with only 3 bits flipped, which a matcher without geometry prefers.  The
    vocabulary is a 5-ary k-majority tree of depth 2 over the points' descriptors, groups at depth 1."""
    import test_match_projection as tproj
    from test_match_window import _lv, pack
    from pislam_amd.frontend import level_scales_q16, projectionRadii
    from conftest import DEMO_LEVELS
    rng = np.random.default_rng(2026)
    levels = DEMO_LEVELS
    s = level_scales_q16(levels)
    lv = np.array([_lv(l) for l in levels], np.int64)
    R = lambda ax, a: tproj.rodrigues(ax, a)
    mk = lambda Rm, O: np.concatenate([Rm.reshape(-1), -Rm @ O]).astype(F32)
    poses = [mk(np.eye(3), np.zeros(3)), mk(R([0, 1, 0], -0.06), np.array([0.8, 0.05, 0.1])),
             mk(R([0.2, 1, 0], -0.03), np.array([0.4, -0.05, 0.2]))]
    z = rng.uniform(3.6, 9.0, n)                             # (levels 1 .. 6: the distance range has room on both sides)
    X = np.stack([rng.uniform(-0.55, 0.75, n) * z, rng.uniform(-0.42, 0.42, n) * z, z], 1)
    desc = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    frames = []
    for k, pose in enumerate(poses):
        o, zc = ttri.project(pose, CHAIN_CAM.astype(F64), X)
        seen = (zc > 1) & (o[:, 0] > 20) & (o[:, 0] < 620) & (o[:, 1] > 20) & (o[:, 1] < 460)
        pl = np.clip(np.round(np.log(np.maximum(zc, 1e-3) / 3) / np.log(1.2)), 0, 7).astype(np.int64)
        idx = np.flatnonzero(seen)
        u, v, l = o[idx, 0], o[idx, 1], pl[idx]
        d = tproj.flip_bits(rng, desc[idx], 10)
        if k == 1:                                           # the decoys
            dec = idx[::4]
            # (40 .. 80 pixels above or below the point's own view: the epipolar lines are close to rows here)
            side = np.where(o[dec, 1] > 240, -1.0, 1.0)
            u = np.concatenate([u, np.clip(o[dec, 0] + rng.uniform(-60, 60, len(dec)), 20, 620)])
            v = np.concatenate([v, o[dec, 1] + side * rng.uniform(40, 80, len(dec))])
            l = np.concatenate([l, pl[dec]])
            d = np.concatenate([d, tproj.flip_bits(rng, desc[dec], 3)])
            idx = np.concatenate([idx, np.full(len(dec), -1)])
        sc = np.asarray(s, F64)[l] / 65536.0
        ku = np.clip(np.floor(u / sc + 0.5).astype(np.int64), 0, lv[l, 0] - 1)
        kv = np.clip(np.floor(v / sc + 0.5).astype(np.int64), 0, lv[l, 1] - 1)
        order = rng.permutation(len(idx))
        frames.append(dict(kp=pack(lv[l, 3] + ku, lv[l, 2] + kv)[order], desc=d[order], point=idx[order]))
    node_desc, fc, cc = tbow.kmajority_tree(rng, desc, 5, 2)
    far, near = projectionRadii(s, 3)
    return dict(levels=levels, scale_q16=s, poses=poses, X=X, frames=frames, vocab=(node_desc, fc, cc), group_depth=1,
                radius_far=far.tolist(), radius_near=near.tolist())


def _pad(a, stride, fill=0):
    out = np.full((1, stride) + a.shape[1:], fill, a.dtype)
    out[0, :len(a)] = a
    return out


@functools.lru_cache(maxsize=None)
def chain_reference():
    """Every stage of the chain by the restatements alone (numpy, and poseObservationsQ8 on host tensors)."""
    import torch
    import test_match_projection as tproj
    import test_match_select as tsel
    from pislam_amd.frontend import poseObservationsQ8
    sc = chain_scene()
    f1, f2, f3 = sc["frames"]
    node_desc, fc, cc = sc["vocab"]
    tree = tbow.ref_tree(8, len(fc), fc, cc, sc["group_depth"])
    ngroups = int(tree["ngroups"])
    g1 = tbow.ref_descend(f1["desc"], node_desc, fc, cc, tree)[1]
    g2 = tbow.ref_descend(f2["desc"], node_desc, fc, cc, tree)[1]
    obs = []
    for f in (f1, f2):
        o, l = poseObservationsQ8(torch.from_numpy(f["kp"].astype(np.int64))[None], sc["levels"], sc["scale_q16"])
        obs.append((o[0].numpy(), l[0].numpy()))
    (o1, l1), (o2, l2) = obs
    cam4 = CHAIN_CAM[:4]
    F12, e12 = (a.astype(F32) for a in ref_epipolar_from_poses(sc["poses"][0], sc["poses"][1], cam4, cam4))
    F21, e21 = (a.astype(F32) for a in ref_epipolar_from_poses(sc["poses"][1], sc["poses"][0], cam4, cam4))
    fwd = ref_epipolar_match(f1["desc"], g1, o1, l1, None, f2["desc"], g2, o2, l2, None, ngroups, F12, e12)
    back = ref_epipolar_match(f2["desc"], g2, o2, l2, None, f1["desc"], g1, o1, l1, None, ngroups, F21, e21)
    plain = tbow.ref_bow_match(f1["desc"], g1, f2["desc"], g2, ngroups)
    sq, st, _, _ = tsel.ref_select(fwd[0], fwd[1], fwd[2], len(f2["kp"]), back=back[0], **CHAIN_SELECT)
    tri = ttri.ref_pair(sc["poses"][0], sc["poses"][1], CHAIN_CAM, CHAIN_CAM, o1[sq], o2[st], l1[sq], l2[st])
    # the new points, searched in the third frame with the normal and distance range the triangulation returned
    m, qs, n3 = len(sq), len(f1["kp"]) + 9, len(f3["kp"])
    ls = (np.asarray(sc["scale_q16"], F32) / F32(65536.0)).astype(F32)
    case = dict(levels=sc["levels"], scale_q16=sc["scale_q16"], level_scale=ls, radius_far=sc["radius_far"],
                radius_near=sc["radius_near"], pose=sc["poses"][2][None], cam=CHAIN_CAM[None], xw=_pad(tri["xw"], qs),
                drange=_pad(tri["drange"], qs), normal=_pad(tri["normal"], qs), qd=_pad(f1["desc"][sq], qs),
                qc=np.array([m], np.uint32), tkp=_pad(f3["kp"], n3 + 3), td=_pad(f3["desc"], n3 + 3), tc=np.array([n3], np.uint32))
    return dict(ngroups=ngroups, g1=g1, g2=g2, o1=o1, l1=l1, o2=o2, l2=l2, F12=F12, e12=e12, F21=F21, e21=e21, fwd=fwd,
                back=back, plain=plain, sq=sq, st=st, tri=tri, proj=tproj.ref_call(case))


def test_chain_scene_preconditions():
    """The scene is meaningful (restatements only).  2026-10-20: 299 points are seen by both key frames, 253 matches are
    selected and all 253 become map points; the epipolar test removes the plain word-guided matcher's best candidate for
    151 queries, 75 of them decoys; 219 of the new points are found again in the third frame; the worst distance of a
    created point to the true one is 0.518 units (points up to 9 units deep seen from 0.8 units apart, keypoints on the
    pixel grid of their level); informative only."""
    sc, r = chain_scene(), chain_reference()
    f1, f2, _ = sc["frames"]
    # the epipolar test removes candidates the plain word-guided match would have chosen as best
    best_e, best_p = r["fwd"][0], r["plain"][0]
    changed = np.flatnonzero((best_p >= 0) & (best_p != best_e))
    removed = [i for i in changed if not r["fwd"][3][i, best_p[i]]]
    decoy = [i for i in removed if f2["point"][best_p[i]] == -1]
    covisible = np.intersect1d(f1["point"], f2["point"][f2["point"] >= 0])
    made = r["tri"]["status"] == ttri.OK
    p1, p2 = f1["point"][r["sq"]], f2["point"][r["st"]]
    worst = np.linalg.norm(r["tri"]["xw"][made].astype(F64) - sc["X"][p1[made]], axis=1).max()
    print("covisible %d, selected %d, points %d, removed best candidates %d (decoys %d), worst distance %.3f" % (
        len(covisible), len(r["sq"]), made.sum(), len(removed), len(decoy), worst))
    assert len(removed) >= 1 and len(decoy) >= 1
    assert 2 * made.sum() >= len(covisible) and len(covisible) > 200
    assert (p1[made] == p2[made]).all() and (p1[made] >= 0).all()       # every created point's true index is the matched one
    # the third frame lies between the key frames and sees the points within a tenth of their distance to key frame 1,
    # well inside the distance range of a point on levels 1 .. 6: most new points are found again, each by its own keypoint
    f3 = sc["frames"][2]
    found = r["proj"][0][0, :len(r["sq"])].view(np.int32)
    hit = (found >= 0) & made & (f3["point"][np.maximum(found, 0)] == p1)
    print("%d new points, %d of them found again in the third frame" % (made.sum(), hit.sum()))
    assert 2 * hit.sum() >= made.sum()


@pytest.mark.gpu
def test_gpu_chain_new_points_are_found_in_a_third_frame(gpu_ctx):
    """bowTransformBatch -> matchEpipolarBatch both ways -> selectMatchesBatch with the cross-check ->
    matchedObservationPairs -> triangulateBatch -> matchProjectionBatch in map mode on a third frame with the returned
    normal and drange: every stage equals its restatement exactly."""
    import torch
    import test_match_projection as tproj
    from pislam_amd.frontend import (Vocabulary, bowTransformBatch, epipolarGeometry, matchedObservationPairs,
                                     matchEpipolarBatch, matchProjectionBatch, poseObservationsQ8, selectMatchesBatch,
                                     triangulateBatch)
    sc, r = chain_scene(), chain_reference()
    f1, f2, f3 = sc["frames"]
    n1, n2, n3 = len(f1["kp"]), len(f2["kp"]), len(f3["kp"])
    qs, ts = n1 + 9, n2 + 5
    node_desc, fc, cc = sc["vocab"]
    v = Vocabulary(node_desc, fc, cc, sc["group_depth"], ctx=gpu_ctx)
    assert v.ngroups == r["ngroups"]
    d1, d2 = to_dev(_pad(f1["desc"], qs)), to_dev(_pad(f2["desc"], ts))
    k1, k2 = to_dev(_pad(f1["kp"], qs)), to_dev(_pad(f2["kp"], ts))
    c1, c2 = to_dev(np.array([n1], np.uint32)), to_dev(np.array([n2], np.uint32))
    _, g1, _ = bowTransformBatch(v, d1, c1, ctx=gpu_ctx)
    _, g2, _ = bowTransformBatch(v, d2, c2, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert (g1[0, :n1].cpu().numpy() == r["g1"]).all() and (g2[0, :n2].cpu().numpy() == r["g2"]).all()
    (o1, l1), (o2, l2) = poseObservationsQ8(k1, sc["levels"], sc["scale_q16"]), poseObservationsQ8(k2, sc["levels"], sc["scale_q16"])
    assert (o1[0, :n1].cpu().numpy() == r["o1"]).all() and (l2[0, :n2].cpu().numpy() == r["l2"]).all()
    pose = [to_dev(p[None]) for p in sc["poses"]]
    cam = to_dev(CHAIN_CAM[None])
    F12, e12 = epipolarGeometry(pose[0], pose[1], cam, cam)
    F21, e21 = epipolarGeometry(pose[1], pose[0], cam, cam)
    assert np.abs(F12[0] - r["F12"]).max() <= ulp32(np.abs(r["F12"]).max())
    # (the device runs on the restatement's F and epipole words: the helper is stated to a tolerance)
    fwd = matchEpipolarBatch(d1, g1, o1, l1, c1, d2, g2, o2, l2, c2, v.ngroups, to_dev(r["F12"][None]), to_dev(r["e12"][None]), ctx=gpu_ctx)
    back = matchEpipolarBatch(d2, g2, o2, l2, c2, d1, g1, o1, l1, c1, v.ngroups, to_dev(r["F21"][None]), to_dev(r["e21"][None]), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    for got, want, n in ((fwd, r["fwd"], n1), (back, r["back"], n2)):
        for g, w in zip(got, want[:3]):
            assert (g[0, :n].cpu().numpy().view(np.uint32) == w.view(np.uint32)).all()
    sq, st, nsel = selectMatchesBatch(*fwd, c1, c2, back_idx=back[0], ctx=gpu_ctx, **CHAIN_SELECT)
    gpu_ctx.synchronize()
    m = int(nsel[0])
    assert m == len(r["sq"]) and (sq[0, :m].cpu().numpy() == r["sq"]).all() and (st[0, :m].cpu().numpy() == r["st"]).all()
    s1, sl1, s2, sl2, counts = matchedObservationPairs(o1, l1, o2, l2, (sq, st, nsel))
    torch.cuda.synchronize()
    assert (s1[0, :m].cpu().numpy() == r["o1"][r["sq"]]).all() and (s2[0, :m].cpu().numpy() == r["o2"][r["st"]]).all()
    assert (sl1[0, :m].cpu().numpy() == r["l1"][r["sq"]]).all() and (sl2[0, m:].cpu().numpy() == 255).all()
    assert (s1[0, m:, 2].cpu().numpy() == MONO).all() and not s1[0, m:, :2].any() and int(counts[0]) == m
    xw, status, normal, drange, npoints = triangulateBatch(pose[0], pose[1], cam, cam, s1, s2, sl1, sl2, counts, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    t = r["tri"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (status[0, :m].cpu().numpy() == t["status"]).all() and int(npoints[0]) == int((t["status"] == 0).sum())
    for g, w in ((xw, t["xw"]), (normal, t["normal"]), (drange, t["drange"])):
        assert (bits(g[0, :m].cpu().numpy()) == bits(w)).all()
    # the new points, searched in the third frame
    qd = torch.gather(d1, 1, sq.to(torch.int64).clamp(0, qs - 1)[..., None].expand(-1, -1, 8)).contiguous()
    k3, d3, c3 = to_dev(_pad(f3["kp"], n3 + 3)), to_dev(_pad(f3["desc"], n3 + 3)), to_dev(np.array([n3], np.uint32))
    got = matchProjectionBatch(pose[2], cam, xw, qd, counts, k3, d3, c3, sc["levels"], drange=drange, normal=normal, th=3,
                               scale_q16=sc["scale_q16"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    want = r["proj"]
    for name, g, w in zip(tproj.NAMES, got, want):
        g = g[0, :m].cpu().numpy()
        assert ((g.view(np.uint32) if g.dtype == np.int32 else g) == w[0, :m]).all(), name
