"""New map points from two key frames (pislam_triangulate_batch).

The contract is the comment in include/pislam_hip.h.  `ref_pair` restates it in numpy binary32, one rounding per written
operation (numpy's float32 multiply, add, divide and sqrt are correctly rounded), for all slots of one pair at once.  The
CPU tests check the restatement on hand-built anchors (the contract's own worked example, one slot per status code and
per mode), the host probe (tools/probes/mappoint_host_check.cpp: the library's own arithmetic header under the host
compiler) against it bit for bit, and the scene's preconditions.  The GPU tests compare the library with the restatement
exactly."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F32, F64 = np.float32, np.float64
COUNT_INVALID = 0xFFFFFFFF
MONO = -(1 << 31)
OK, NO_LEVEL, LOW_PARALLAX, NOT_FINITE, DEPTH1, DEPTH2, REPROJ1, REPROJ2, SCALE, PAIR = range(10)
NONE, TRIANGULATE, STEREO1, STEREO2 = range(4)
PARAM_FIELDS = ["cos_min_parallax", "chi2_mono", "chi2_stereo", "ratio_factor"]
PAR = dict(cos_min_parallax=0.9998, chi2_mono=5.991, chi2_stereo=7.815, ratio_factor=float(F32(1.5) * F32(1.2)))
S8 = 0xA5                                                    # what the outputs are pre-filled with
SF = np.frombuffer(bytes([S8] * 4), F32)[0]
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def level_tables(nlevels=8, scale=1.2):
    s, f = F32(scale), F32(1.0)
    ls = np.empty(nlevels, F32)
    for l in range(nlevels):
        ls[l] = f
        f = f * s
    return ls, ls * ls


LS8, SG8 = level_tables()


# ---- the restatement -------------------------------------------------------------------------------------------------
def _side(obs, C, ifx, ify, hb):
    q = np.clip(obs.astype(np.int64), -(1 << 22), 1 << 22)
    u, v, ur = (q[:, k].astype(F32) * F32(1.0 / 256.0) for k in range(3))
    x, y = (u - C[2]) * ifx, (v - C[3]) * ify
    d = u - ur
    stereo = (obs[:, 2] != MONO) & (d > 0)
    zs = C[4] / d
    zz, hh = zs * zs, hb * hb
    return dict(u=u, v=v, ur=ur, x=x, y=y, zs=zs, cs=(zz - hh) / (zz + hh), stereo=stereo)


def _to_world(R, t, X):
    e0, e1, e2 = X[0] - t[0], X[1] - t[1], X[2] - t[2]
    return [(R[j] * e0 + R[3 + j] * e1) + R[6 + j] * e2 for j in range(3)]


def _check(R, t, C, s, Xw, bound_mono, bound_stereo):
    """(depth ok, reprojection ok) of the world points through one pose."""
    X, Y, Z = Xw
    x = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
    y = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
    z = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
    iz = F32(1.0) / z
    px, py = x * iz, y * iz
    pu, pv = C[0] * px + C[2], C[1] * py + C[3]
    eu, ev = s["u"] - pu, s["v"] - pv
    e2 = eu * eu + ev * ev
    er = s["ur"] - (pu - C[4] * iz)
    e2 = np.where(s["stereo"], e2 + er * er, e2)
    assert e2.dtype == F32
    return z > 0, e2 <= np.where(s["stereo"], bound_stereo, bound_mono)


def ref_pair(pose1, pose2, cam1, cam2, obs1, obs2, l1, l2, ls=LS8, sg=SG8, **par):
    """The n slots of one pair: dict of status, mode (uint8 [n]), xw, normal (float32 [n][3]), drange (float32 [n][2]),
    and, for the anchors, scale_a / scale_b: the two inequalities of step 8 (True = holds)."""
    par = dict(PAR, **par)
    P1, P2, C1, C2 = (np.asarray(a, F32) for a in (pose1, pose2, cam1, cam2))
    obs1, obs2 = np.asarray(obs1, np.int64).reshape(-1, 3), np.asarray(obs2, np.int64).reshape(-1, 3)
    l1, l2 = np.asarray(l1, np.int64).reshape(-1), np.asarray(l2, np.int64).reshape(-1)
    ls, sg = np.asarray(ls, F32), np.asarray(sg, F32)
    n, nl = len(obs1), len(ls)
    out = dict(status=np.full(n, PAIR, np.uint8), mode=np.zeros(n, np.uint8), xw=np.zeros((n, 3), F32),
               normal=np.zeros((n, 3), F32), drange=np.zeros((n, 2), F32), scale_a=np.zeros(n, bool), scale_b=np.zeros(n, bool))
    if not (all(np.isfinite(a).all() for a in (P1, P2, C1, C2)) and C1[0] != 0 and C1[1] != 0 and C2[0] != 0 and C2[1] != 0):
        return out
    if n == 0:
        return out
    cmp_, rf = F32(par["cos_min_parallax"]), F32(par["ratio_factor"])
    R1, t1, R2, t2 = P1[:9], P1[9:], P2[:9], P2[9:]
    with np.errstate(all="ignore"):
        c = np.zeros(12, F32)
        for i in range(3):
            for j in range(3):
                c[3 * i + j] = (R2[3 * i] * R1[3 * j] + R2[3 * i + 1] * R1[3 * j + 1]) + R2[3 * i + 2] * R1[3 * j + 2]
        for i in range(3):
            c[9 + i] = t2[i] - ((c[3 * i] * t1[0] + c[3 * i + 1] * t1[1]) + c[3 * i + 2] * t1[2])
        O1 = [-((R1[j] * t1[0] + R1[3 + j] * t1[1]) + R1[6 + j] * t1[2]) for j in range(3)]
        O2 = [-((R2[j] * t2[0] + R2[3 + j] * t2[1]) + R2[6 + j] * t2[2]) for j in range(3)]
        one, half = F32(1.0), F32(0.5)
        s1 = _side(obs1, C1, one / C1[0], one / C1[1], (C1[4] / C1[0]) * half)
        s2 = _side(obs2, C2, one / C2[0], one / C2[1], (C2[4] / C2[0]) * half)
        x1, y1, x2, y2 = s1["x"], s1["y"], s2["x"], s2["y"]
        bb = (x2 * x2 + y2 * y2) + one
        a0 = (c[0] * x1 + c[1] * y1) + c[2]
        a1 = (c[3] * x1 + c[4] * y1) + c[5]
        a2 = (c[6] * x1 + c[7] * y1) + c[8]
        cs = ((a0 * x2 + a1 * y2) + a2) / np.sqrt(((a0 * a0 + a1 * a1) + a2 * a2) * bb)
        st1, st2 = s1["stereo"], s2["stereo"]
        cs1, cs2 = np.where(st1, s1["cs"], cs + one), np.where(st2, s2["cs"], cs + one)
        mn = np.where(cs2 < cs1, cs2, cs1)
        tri = (cs < mn) & (cs > 0) & (st1 | st2 | (cs < cmp_))
        m1 = ~tri & st1 & (cs1 < cs2)
        m2 = ~tri & ~m1 & st2 & (cs2 < cs1)
        mode = np.where(tri, TRIANGULATE, np.where(m1, STEREO1, np.where(m2, STEREO2, NONE)))
        # the midpoint of the closest points of the two rays
        t0_, t1_, t2_ = c[9], c[10], c[11]
        n0, n1, n2 = a1 - a2 * y2, a2 * x2 - a0, a0 * y2 - a1 * x2
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        p0, p1, p2 = y2 * t2_ - t1_, t0_ - x2 * t2_, x2 * t1_ - y2 * t0_
        q0, q1, q2 = a1 * t2_ - a2 * t1_, a2 * t0_ - a0 * t2_, a0 * t1_ - a1 * t0_
        z1 = ((p0 * n0 + p1 * n1) + p2 * n2) / nn
        z2 = ((q0 * n0 + q1 * n1) + q2 * n2) / nn
        g0, g1, g2 = z2 * x2 - t0_, z2 * y2 - t1_, z2 - t2_
        h0 = (c[0] * g0 + c[3] * g1) + c[6] * g2
        h1 = (c[1] * g0 + c[4] * g1) + c[7] * g2
        h2 = (c[2] * g0 + c[5] * g1) + c[8] * g2
        Xt = _to_world(R1, t1, [(z1 * x1 + h0) * half, (z1 * y1 + h1) * half, (z1 + h2) * half])
        Xs1 = _to_world(R1, t1, [x1 * s1["zs"], y1 * s1["zs"], s1["zs"]])
        Xs2 = _to_world(R2, t2, [x2 * s2["zs"], y2 * s2["zs"], s2["zs"]])
        Xw = [np.where(tri, Xt[j], np.where(m1, Xs1[j], Xs2[j])) for j in range(3)]
        finite = np.isfinite(Xw[0]) & np.isfinite(Xw[1]) & np.isfinite(Xw[2])
        k1, k2 = np.minimum(l1, nl - 1), np.minimum(l2, nl - 1)
        cm, cst = F32(par["chi2_mono"]), F32(par["chi2_stereo"])
        dep1, rep1 = _check(R1, t1, C1, s1, Xw, cm * sg[k1], cst * sg[k1])
        dep2, rep2 = _check(R2, t2, C2, s2, Xw, cm * sg[k2], cst * sg[k2])
        e = [Xw[j] - O1[j] for j in range(3)]
        f = [Xw[j] - O2[j] for j in range(3)]
        d1 = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        d2 = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
        r1, r2 = d1 * ls[k1], d2 * ls[k2]
        sa, sb = (d2 * rf) * ls[k2] >= r1, r2 <= r1 * rf
        scale_ok = (d1 != 0) & (d2 != 0) & sa & sb
        w = [e[j] / d1 + f[j] / d2 for j in range(3)]
        wn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        normal = np.stack([w[j] / wn for j in range(3)], 1)
        drange = np.stack([r1 / ls[nl - 1], r1], 1)
    assert all(a.dtype == F32 for a in (cs, z1, Xw[0], d1, normal, drange))
    status = np.full(n, OK, np.int64)
    for code, fails in ((SCALE, ~scale_ok), (REPROJ2, ~rep2), (REPROJ1, ~rep1), (DEPTH2, ~dep2), (DEPTH1, ~dep1),
                        (NOT_FINITE, ~finite), (LOW_PARALLAX, mode == NONE), (NO_LEVEL, (l1 >= nl) | (l2 >= nl))):
        status = np.where(fails, code, status)               # the last one written is the first test of the contract
    good = status == OK
    out["status"] = status.astype(np.uint8)
    out["mode"] = np.where(status >= LOW_PARALLAX + 1, mode, np.where(status == OK, mode, NONE)).astype(np.uint8)
    out["xw"] = np.where(good[:, None], np.stack(Xw, 1), F32(0))
    out["normal"] = np.where(good[:, None], normal, F32(0))
    out["drange"] = np.where(good[:, None], drange, F32(0))
    out["scale_a"], out["scale_b"] = sa, sb
    return out


def q8(*px):
    return [int(round(v * 256)) if v is not None else MONO for v in px]


def one(obs1, obs2, l1=0, l2=0, pose1=IDENTITY, pose2=None, cam1=None, cam2=None, ls=LS8, sg=SG8, **par):
    pose2 = pose_t(-1, 0, 0) if pose2 is None else pose2
    cam1 = CAM if cam1 is None else cam1
    cam2 = CAM if cam2 is None else cam2
    r = ref_pair(pose1, pose2, cam1, cam2, [obs1], [obs2], [l1], [l2], ls, sg, **par)
    return {k: v[0] for k, v in r.items()}


def pose_t(x, y, z, R=None):
    return np.concatenate([np.asarray(IDENTITY[:9] if R is None else R, F64).reshape(-1), [x, y, z]]).astype(F32)


CAM = np.array([100, 100, 0, 0, 10], F32)                    # baseline 0.1: hb = 0.05
UNIT = np.array([1, 1, 0, 0, 0], F32)


# ---- CPU: declarations -----------------------------------------------------------------------------------------------
def test_triangulate_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_triangulate_batch\s*\(", code), "not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_triangulate_params \{([^}]*)\} pislam_triangulate_params;", code)
    assert m
    fields = []
    for ty, names in re.findall(r"(int32_t|float)\s+([\w\s,]+);", m.group(1)):
        fields += [(n.strip(), ty) for n in names.split(",")]
    assert [n for n, _ in fields] == PARAM_FIELDS and [t for _, t in fields] == ["float"] * 4
    assert "#define PISLAM_ABI_VERSION 2" in text
    assert "Not here: the baseline test that skips a key-frame pair" in text and "local bundle" in text
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_triangulate_batch"][1]) == 21
    assert [n for n, _ in capi.TriangulateParams._fields_] == PARAM_FIELDS and ctypes.sizeof(capi.TriangulateParams) == 16
    for f in ("triangulateBatch", "matchedObservationPairs", "mapPointLevelTables"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    assert hasattr(lib, "pislam_triangulate_batch")
    for f in ("pislam_mappoint_math.h", "pislam_mappoint_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "pislam_amd", "csrc", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "probes", "mappoint_host_check.cpp"))
    assert "mappoint_host_check" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_new_points.py"))


def test_level_tables_one_operation_at_a_time():
    from pislam_amd.frontend import mapPointLevelTables, poseLevelWeights
    ls, sg = mapPointLevelTables(8, 1.2)
    assert ls.dtype == F32 and sg.dtype == F32
    assert (ls.view(np.uint32) == LS8.view(np.uint32)).all() and (sg.view(np.uint32) == SG8.view(np.uint32)).all()
    assert ls[0] == 1 and ls[1] == F32(1.2) and ls[2] == F32(1.2) * F32(1.2) and sg[2] == ls[2] * ls[2]
    assert ((F32(1.0) / sg).view(np.uint32) == poseLevelWeights(8, 1.2).view(np.uint32)).all()
    with pytest.raises(ValueError):
        mapPointLevelTables(17)


# ---- CPU: hand-built anchors of the restatement ----------------------------------------------------------------------
def test_ref_worked_example_of_the_contract():
    """Both poses the identity but t2 = (-1, 0, 0), both cameras (1, 1, 0, 0, 0), (u1, v1) = (0, 0), (u2, v2) =
    (-0.5, 0): Xw = (0, 0, 2), d1 = 2, d2 = sqrt(5)."""
    r = one(q8(0, 0, None), q8(-0.5, 0, None), cam1=UNIT, cam2=UNIT)
    assert r["status"] == OK and r["mode"] == TRIANGULATE and r["xw"].tolist() == [0, 0, 2]
    assert r["drange"][1] == 2 and r["drange"][0] == F32(2) / LS8[7]
    w = np.array([0, 0, 1], F64) + np.array([-1, 0, 2], F64) / np.sqrt(5)
    assert np.abs(r["normal"].astype(F64) - w / np.linalg.norm(w)).max() < 2e-7
    # levels: d1 * ls[l1] against d2 * ls[l2] within the ratio factor 1.8
    r = one(q8(0, 0, None), q8(-0.5, 0, None), 3, 3, cam1=UNIT, cam2=UNIT)
    assert r["status"] == OK and r["drange"][1] == F32(2) * LS8[3]


def anchor_cases():
    """(name, keyword arguments of `one`, status, mode, further expectations) for every code and mode."""
    nan = float("nan")
    far2 = pose_t(0, 0, -5)                                  # key frame 2 five units ahead of key frame 1
    near2 = pose_t(-0.01, 0, 0)                              # ... or a hundredth of a unit to its right
    st1 = q8(0, 0, -5)                                       # disparity 5 px, bf 10: zs = 2
    A = []
    add = lambda name, kw, status, mode, **more: A.append((name, kw, status, mode, more))
    add("triangulated", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None)), OK, TRIANGULATE)
    add("no level 1", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), l1=8), NO_LEVEL, NONE)
    add("no level 2", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), l2=255), NO_LEVEL, NONE)
    add("same ray, two monocular keypoints", dict(obs1=q8(0, 0, None), obs2=q8(0, 0, None), pose2=IDENTITY), LOW_PARALLAX, NONE)
    add("parallax just too low", dict(obs1=q8(0, 0, None), obs2=q8(-0.5, 0, None), pose2=near2), LOW_PARALLAX, NONE)
    add("... unless the bound is lifted", dict(obs1=q8(0, 0, None), obs2=q8(-0.5, 0, None), pose2=near2, cos_min_parallax=0.99999),
        OK, TRIANGULATE)
    add("stereo unprojection chosen over triangulation at low ray parallax",
        dict(obs1=st1, obs2=q8(-0.5, 0, None), pose2=near2), OK, STEREO1)
    add("... and from side 2", dict(obs1=q8(0.5, 0, None), obs2=st1, pose1=near2, pose2=IDENTITY), OK, STEREO2)
    add("a stereo side with d <= 0 is monocular", dict(obs1=q8(0, 0, 5), obs2=q8(-0.5, 0, None), pose2=near2), LOW_PARALLAX, NONE)
    add("... also with d == 0", dict(obs1=q8(0, 0, 0), obs2=q8(-0.5, 0, None), pose2=near2), LOW_PARALLAX, NONE)
    add("a stereo side triangulates at wide baseline", dict(obs1=st1, obs2=q8(-50, 0, None)), OK, TRIANGULATE)
    add("parallel rays", dict(obs1=q8(0, 0, None), obs2=q8(0, 0, None), pose2=IDENTITY, cos_min_parallax=2.0), NOT_FINITE, TRIANGULATE)
    add("rays that meet behind the cameras", dict(obs1=q8(0, 0, None), obs2=q8(50, 0, None)), DEPTH1, TRIANGULATE)
    add("behind key frame 2 only", dict(obs1=st1, obs2=q8(0, 0, None), pose2=far2), DEPTH2, STEREO1)
    add("six pixels apart in v on level 0", dict(obs1=q8(0, 3, None), obs2=q8(-50, -3, None)), REPROJ1, TRIANGULATE)
    add("... passes on level 3 in key frame 1 only", dict(obs1=q8(0, 3, None), obs2=q8(-50, -3, None), l1=3), REPROJ2, TRIANGULATE)
    add("... and on level 3 in both", dict(obs1=q8(0, 3, None), obs2=q8(-50, -3, None), l1=3, l2=3), OK, TRIANGULATE)
    add("the right coordinate counts on a stereo side", dict(obs1=q8(0, 0, -8), obs2=q8(-50, 0, None)), REPROJ1, TRIANGULATE)
    add("scale: key frame 1 sees it far too coarse", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), l1=7), SCALE, TRIANGULATE,
        scale_a=False, scale_b=True)
    add("scale: key frame 2 sees it far too coarse", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), l2=7), SCALE, TRIANGULATE,
        scale_a=True, scale_b=False)
    bad = IDENTITY.copy()
    bad[4] = nan
    add("a pose that is not finite", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), pose1=bad), PAIR, NONE)
    add("fx == 0", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), cam2=np.array([0, 100, 0, 0, 10], F32)), PAIR, NONE)
    add("bf infinite", dict(obs1=q8(0, 0, None), obs2=q8(-50, 0, None), cam1=np.array([100, 100, 0, 0, np.inf], F32)), PAIR, NONE)
    return A


def test_ref_anchors_cover_every_status_and_mode():
    seen, modes = set(), set()
    for name, kw, status, mode, more in anchor_cases():
        r = one(**kw)
        assert r["status"] == status and r["mode"] == mode, (name, r)
        for k, v in more.items():
            assert r[k] == v, (name, k, r)
        if status != OK:
            assert not r["xw"].any() and not r["normal"].any() and not r["drange"].any(), name
        seen.add(status)
        modes.add(mode)
    assert seen == set(range(10)) and modes == {NONE, TRIANGULATE, STEREO1, STEREO2}
    r = one(q8(0, 0, None), q8(-50, 0, None))
    assert r["xw"].tolist() == [0, 0, 2]                    # x2 = -0.5 again, now through fx = 100
    r = one(q8(0, 0, -5), q8(-0.5, 0, None), pose2=pose_t(-0.01, 0, 0))
    assert r["xw"].tolist() == [0, 0, 2]                    # unprojected: zs = bf / d = 10 / 5


# ---- CPU: the host probe against the restatement ---------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(np.asarray(a, F32)).reshape(-1).view(np.uint32))


def probe_line(kw):
    kw = dict(dict(l1=0, l2=0, pose1=IDENTITY, pose2=pose_t(-1, 0, 0), cam1=CAM, cam2=CAM, ls=LS8, sg=SG8), **kw)
    par = dict(PAR, **{k: kw[k] for k in PARAM_FIELDS if k in kw})
    return " ".join(["%d %d %d" % (len(kw["ls"]), kw["l1"], kw["l2"]), " ".join(str(int(v)) for v in kw["obs1"]),
                     " ".join(str(int(v)) for v in kw["obs2"]), hexf(kw["pose1"]), hexf(kw["pose2"]), hexf(kw["cam1"]),
                     hexf(kw["cam2"]), hexf(kw["ls"]), hexf(kw["sg"]), hexf([par[k] for k in PARAM_FIELDS])])


def rodrigues(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def project(pose, cam, X):
    """float64 pixel (u, v, u_right) and depth of world points X [n][3]."""
    p = np.asarray(pose, F64)
    Xc = X @ p[:9].reshape(3, 3).T + p[9:]
    z = Xc[:, 2]
    u = cam[0] * Xc[:, 0] / z + cam[2]
    return np.stack([u, cam[1] * Xc[:, 1] / z + cam[3], u - cam[4] / z], 1), z


def random_pair(rng, kind=0, nl=8):
    """Two key frames 0.05 .. 1 units apart that look roughly the same way; kind 1: the same place (no parallax),
    kind 2: identity rotations at the same place (parallel rays), kind 3: key frame 2 one unit ahead of key frame 1 (near
    points lie behind it)."""
    R1 = rodrigues(rng.normal(size=3), rng.uniform(0, 0.3))
    t1 = rng.normal(0, 1, 3)
    R2 = rodrigues(rng.normal(size=3), rng.uniform(0, 0.1)) @ R1
    O1 = -R1.T @ t1
    base = rng.normal(size=3)
    O2 = O1 + base / np.linalg.norm(base) * (0 if kind else rng.choice([0.05, 0.3, 1.0]))
    if kind == 3:
        O2 = O1 + R1[2]                                      # one unit ahead along key frame 1's optical axis
    if kind == 2:
        R1 = R2 = np.eye(3)
        t1 = np.round(t1 * 8) / 8
        O1 = O2 = -t1
    pose1 = np.concatenate([R1.reshape(-1), t1]).astype(F32)
    pose2 = np.concatenate([R2.reshape(-1), -R2 @ O2]).astype(F32)
    cams = [np.array([rng.uniform(300, 700), rng.uniform(300, 700), rng.uniform(300, 340), rng.uniform(220, 260),
                      rng.choice([0.0, 40.0, 80.0])], F32) for _ in range(2)]
    return pose1, pose2, cams[0], cams[1]


def random_slots(rng, pose1, pose2, cam1, cam2, n, nl=8):
    """n slots (obs1, obs2, l1, l2) of points 1 .. 30 units in front of key frame 1: consistent levels and exact
    projections for most, and in turn noise of a few pixels, a wrong level, a level past the table, stereo observations
    on either side (a tenth of them with a negative disparity), a point behind the cameras."""
    p1 = np.asarray(pose1, F64)
    R1, t1 = p1[:9].reshape(3, 3), p1[9:]
    z = rng.uniform(1, 30, n)
    kind = rng.integers(0, 12, n)
    z[kind == 6] = rng.uniform(0.2, 1.2, int((kind == 6).sum()))   # near enough to lie behind a key frame 2 further on
    Xc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    Xc[kind == 0] *= -1
    X = (Xc - t1) @ R1
    (o1, z1), (o2, z2) = project(pose1, cam1.astype(F64), X), project(pose2, cam2.astype(F64), X)
    o1[:, :2] += rng.normal(0, 1, (n, 2)) * np.where(kind == 1, 4.0, 0.2)[:, None]
    o2[:, :2] += rng.normal(0, 1, (n, 2)) * np.where(kind == 2, 4.0, 0.2)[:, None]
    with np.errstate(all="ignore"):
        l1 = np.clip(np.round(np.log(np.abs(z1) / 2) / np.log(1.2)), 0, nl - 1).astype(np.int64)
        l2 = np.clip(np.round(np.log(np.abs(z2) / 2) / np.log(1.2)), 0, nl - 1).astype(np.int64)
    l1[kind == 3] = rng.integers(0, nl, int((kind == 3).sum()))
    l2[kind == 4] = (l2[kind == 4] + 5) % nl
    l1[kind == 5] = nl + rng.integers(0, 200, int((kind == 5).sum()))
    q1 = np.clip(np.round(np.nan_to_num(o1) * 256), -(1 << 30), 1 << 30).astype(np.int64)
    q2 = np.clip(np.round(np.nan_to_num(o2) * 256), -(1 << 30), 1 << 30).astype(np.int64)
    s1, s2 = (rng.random(n) < 0.4) & (cam1[4] > 0), (rng.random(n) < 0.4) & (cam2[4] > 0)
    flip = rng.random(n) < 0.1
    q1[:, 2] = np.where(s1, np.where(flip, 2 * q1[:, 0] - q1[:, 2], q1[:, 2]), MONO)
    q2[:, 2] = np.where(s2, np.where(flip, q2[:, 0], q2[:, 2]), MONO)
    return q1, q2, l1, l2


def random_cases(n, seed):
    """Keyword arguments of `one`, a pair of its own per slot."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = 1 if i % 9 == 0 else (2 if i % 31 == 0 else (3 if i % 7 == 3 else 0))
        pose1, pose2, cam1, cam2 = random_pair(rng, kind)
        nl = int(rng.integers(1, 9)) if i % 5 == 0 else 8
        ls, sg = level_tables(nl, rng.uniform(1.1, 1.5))
        q1, q2, l1, l2 = random_slots(rng, pose1, pose2, cam1, cam2, 1, nl)
        kw = dict(obs1=q1[0].tolist(), obs2=q2[0].tolist(), l1=int(l1[0]), l2=int(l2[0]), pose1=pose1, pose2=pose2, cam1=cam1,
                  cam2=cam2, ls=ls, sg=sg, ratio_factor=float(F32(rng.uniform(1.2, 2.0))))
        if kind == 2:
            kw.update(obs2=kw["obs1"][:2] + [MONO], obs1=kw["obs1"][:2] + [MONO], cam2=cam1, cos_min_parallax=2.0)
        if i % 97 == 0:
            kw["pose%d" % (1 + i % 2)] = pose1.copy()
            kw["pose%d" % (1 + i % 2)][int(rng.integers(0, 12))] = [np.nan, np.inf, -np.inf][i % 3]
        if i % 101 == 0:
            kw["cam1"] = cam1.copy()
            kw["cam1"][int(rng.integers(0, 2))] = 0
        out.append(kw)
    return out


@pytest.fixture(scope="module")
def run_probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("mappoint_probe") / "mappoint_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "mappoint_host_check.cpp"), "-o", exe])

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def want_line(r):
    return "%d %d %s %s %s" % (r["status"], r["mode"], hexf(r["xw"]), hexf(r["normal"]), hexf(r["drange"]))


def test_probe_equals_the_restatement(run_probe):
    """2400 random slots plus every anchor; as a precondition the slots hold every status code and every mode."""
    cases = random_cases(2400, 11) + [kw for _, kw, _, _, _ in anchor_cases()]
    got = run_probe([probe_line(kw) for kw in cases])
    status, modes = np.zeros(10, np.int64), np.zeros(4, np.int64)
    for kw, g in zip(cases[:2400], got):
        r = one(**kw)
        status[r["status"]] += 1
        modes[r["mode"]] += 1
    print("status counts", status.tolist(), "mode counts", modes.tolist())
    assert (status > 0).all() and (modes > 0).all() and status[OK] > 400, (status, modes)
    for kw, g in zip(cases, got):
        assert g == want_line(one(**kw)), (kw, g, want_line(one(**kw)))


# ---- running the library ---------------------------------------------------------------------------------------------
NAMES = ("xw", "status", "normal", "drange", "npoints")


def clamp_count(c, stride):
    c = int(c)
    return 0 if c == COUNT_INVALID else min(c, stride)


@functools.lru_cache(maxsize=None)
def pins_case(B=3, stride=300, seed=0):
    """B pairs of `stride` random slots each, every status code among them."""
    rng = np.random.default_rng([41, seed])
    c = dict(pose1=np.zeros((B, 12), F32), pose2=np.zeros((B, 12), F32), cam1=np.zeros((B, 5), F32), cam2=np.zeros((B, 5), F32),
             obs1=np.zeros((B, stride, 3), np.int32), obs2=np.zeros((B, stride, 3), np.int32),
             l1=np.zeros((B, stride), np.uint8), l2=np.zeros((B, stride), np.uint8), counts=np.full(B, stride, np.uint32),
             ls=LS8, sg=SG8)
    for b in range(B):
        c["pose1"][b], c["pose2"][b], c["cam1"][b], c["cam2"][b] = random_pair(rng, 3 if b % 3 == 1 else 0)
        q1, q2, l1, l2 = random_slots(rng, c["pose1"][b], c["pose2"][b], c["cam1"][b], c["cam2"][b], stride)
        c["obs1"][b], c["obs2"][b], c["l1"][b], c["l2"][b] = q1, q2, l1, l2
    return c


def ref_call(c, pairs=None, **par):
    """The five outputs of a call on case c (host arrays [B][...]); the sentinel where nothing is written."""
    B, stride = c["obs1"].shape[:2]
    xw, normal = np.full((B, stride, 3), SF, F32), np.full((B, stride, 3), SF, F32)
    drange, status = np.full((B, stride, 2), SF, F32), np.full((B, stride), S8, np.uint8)
    npoints = np.zeros(B, np.uint32)
    for b in (range(B) if pairs is None else pairs):
        n = clamp_count(c["counts"][b], stride)
        r = ref_pair(c["pose1"][b], c["pose2"][b], c["cam1"][b], c["cam2"][b], c["obs1"][b, :n], c["obs2"][b, :n],
                     c["l1"][b, :n], c["l2"][b, :n], c["ls"], c["sg"], **par)
        xw[b, :n], normal[b, :n], drange[b, :n], status[b, :n] = r["xw"], r["normal"], r["drange"], r["status"]
        npoints[b] = int((r["status"] == OK).sum())
    return xw, status, normal, drange, npoints


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def device_case(c):
    return {k: to_dev(c[k]) for k in ("pose1", "pose2", "cam1", "cam2", "obs1", "obs2", "l1", "l2", "counts")}


def run_triangulate(ctx, c, dev=None, want_normal=True, want_drange=True, **par):
    """Host arrays in, host arrays out (xw, status, normal, drange, npoints); every output is pre-filled with the
    sentinel byte."""
    import torch
    from pislam_amd.frontend import triangulateBatch
    t = dev or device_case(c)
    B, stride = c["obs1"].shape[:2]
    full = lambda shape, dt: torch.full(shape, S8, dtype=torch.uint8, device="cuda:0").view(dt) if dt != torch.uint8 else \
        torch.full(shape, S8, dtype=torch.uint8, device="cuda:0")
    outs = dict(xw=full((B, stride, 12), torch.float32).view(B, stride, 3), status=full((B, stride), torch.uint8),
                normal=full((B, stride, 12), torch.float32).view(B, stride, 3) if want_normal else None,
                drange=full((B, stride, 8), torch.float32).view(B, stride, 2) if want_drange else None,
                npoints=full((B * 4,), torch.int32))
    got = triangulateBatch(t["pose1"], t["pose2"], t["cam1"], t["cam2"], t["obs1"], t["obs2"], t["l1"], t["l2"], t["counts"],
                           level_scale=c["ls"], level_sigma2=c["sg"], want_normal=want_normal, want_drange=want_drange,
                           ctx=ctx, **dict(PAR, **par), **outs)
    torch.cuda.synchronize()
    assert (got[2] is None) == (not want_normal) and (got[3] is None) == (not want_drange)
    return tuple(None if outs[k] is None else outs[k].cpu().numpy() for k in NAMES)


def assert_outputs(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g, w = (g.view(np.uint32), w.view(np.uint32)) if g.dtype != np.uint8 else (g, w)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- GPU: pins -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("counts", [(300, 37, 0), (COUNT_INVALID, 305, 299)])
def test_gpu_triangulate_pins(gpu_ctx, counts):
    """Batch 3, stride 300: every status code, counts of 0, 37, PISLAM_COUNT_INVALID and above the stride, the optional
    outputs present and NULL, sentinel-filled outputs untouched at and beyond each count."""
    c = dict(pins_case(), counts=np.array(counts, np.uint32))
    want = ref_call(c)
    seen = set(np.unique(np.concatenate([want[1][b, :clamp_count(n, 300)] for b, n in enumerate(counts)])).tolist())
    assert seen >= set(range(9)) - {NOT_FINITE}, seen        # (NOT_FINITE and PAIR have their own test)
    assert want[4].sum() > 100
    dev = device_case(c)
    assert_outputs(run_triangulate(gpu_ctx, c, dev), want)
    bare = run_triangulate(gpu_ctx, c, dev, want_normal=False, want_drange=False)
    assert bare[2] is None and bare[3] is None
    assert_outputs(bare, want)
    half = run_triangulate(gpu_ctx, c, dev, want_normal=False)
    assert_outputs(half, want)


@pytest.mark.gpu
def test_gpu_triangulate_other_tables_and_parameters(gpu_ctx):
    """Three levels (so that many slots have none), another ratio factor, chi2 bounds and parallax bound."""
    ls, sg = level_tables(3, 1.4)
    c = dict(pins_case(seed=1), ls=ls, sg=sg)
    par = dict(cos_min_parallax=0.99, chi2_mono=2.0, chi2_stereo=3.0, ratio_factor=1.3)
    want = ref_call(c, **par)
    assert (want[1] == NO_LEVEL).sum() > 100 and (want[1] == OK).sum() > 20
    assert (ref_call(c)[1] != want[1]).any()
    assert_outputs(run_triangulate(gpu_ctx, c, **par), want)


@pytest.mark.gpu
def test_gpu_triangulate_bad_pair_between_two_good_ones(gpu_ctx):
    c = dict(pins_case(seed=2))
    c["pose2"] = c["pose2"].copy()
    c["pose2"][1, 7] = np.nan
    want = ref_call(c)
    assert (want[1][1] == PAIR).all() and want[4][1] == 0 and want[4][0] > 0 and want[4][2] > 0
    assert_outputs(run_triangulate(gpu_ctx, c), want)
    c["pose2"][1, 7] = 0
    c["cam1"] = c["cam1"].copy()
    c["cam1"][1, 1] = 0
    want = ref_call(c)
    assert (want[1][1] == PAIR).all()
    assert_outputs(run_triangulate(gpu_ctx, c), want)


@pytest.mark.gpu
def test_gpu_triangulate_points_that_are_not_finite(gpu_ctx):
    """Pair 0: two identity poses at the same place and the same pixel on both sides, triangulated because the parallax
    bound is lifted to 2: 0 / 0.  Pair 1: translations near the largest float, so that t21 overflows."""
    c = dict(pins_case(B=2, stride=64, seed=7))
    for k in ("pose1", "pose2", "cam2", "obs1", "obs2"):
        c[k] = c[k].copy()
    c["pose1"][0] = c["pose2"][0] = pose_t(0.5, -0.25, 1)
    c["cam2"][0] = c["cam1"][0]
    c["obs1"][0, :, 2] = c["obs2"][0, :, 2] = MONO
    c["obs2"][0] = c["obs1"][0]
    c["pose1"][1, 9:] = c["pose2"][1, 9:] = 3e38
    want = ref_call(c, cos_min_parallax=2.0)
    for b in range(2):
        assert (want[1][b] == NOT_FINITE).sum() > 20, np.bincount(want[1][b], minlength=10)
    assert_outputs(run_triangulate(gpu_ctx, c, cos_min_parallax=2.0), want)


# ---- GPU: more pairs than one pass of the workgroups ---------------------------------------------------------------------
GRID_CAP = 1024                                              # pmk::MP_GRID_CAP


@pytest.mark.gpu
def test_gpu_triangulate_more_pairs_than_three_passes(gpu_ctx):
    """2053 pairs of 70 slots, nearly all empty: the live pairs 3, 1027 and 2051 are the same workgroup's first, second
    and third pair (with different slots at the same lane), pair 2052 is the last."""
    B, stride = 2 * GRID_CAP + 5, 70
    assert (B + GRID_CAP - 1) // GRID_CAP >= 3
    live = [3, 3 + GRID_CAP, 3 + 2 * GRID_CAP, B - 1]
    small = pins_case(B=4, stride=stride, seed=3)
    c = {k: np.zeros((B,) + small[k].shape[1:], small[k].dtype) for k in ("pose1", "pose2", "cam1", "cam2", "obs1", "obs2", "l1", "l2")}
    c.update(ls=LS8, sg=SG8, counts=np.zeros(B, np.uint32))
    c["counts"][1::2] = COUNT_INVALID
    for k, b in enumerate(live):
        for name in ("pose1", "pose2", "cam1", "cam2", "obs1", "obs2", "l1", "l2"):
            c[name][b] = small[name][k]
        c["counts"][b] = stride - k
    want = ref_call(c, pairs=live)
    assert (want[1][live[0]] != want[1][live[1]]).any() and (want[1][live[1]] != want[1][live[2]]).any()
    assert all(want[4][b] > 5 for b in live)
    assert_outputs(run_triangulate(gpu_ctx, c), want)


# ---- GPU: offsets beyond 4 GiB ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_triangulate_offsets_beyond_4_gib(gpu_ctx):
    """stride 16384 and 21848 pairs: the observations, points and normals (12 bytes a slot) of the last pairs begin
    beyond 2^32 bytes.  Every array is allocated in one piece, uninitialised; all counts are 0 except the first and the
    last pair's, so no other pair's slots are ever read or written."""
    import torch
    from pislam_amd.frontend import triangulateBatch
    B, stride, n = 21848, 16384, 150
    assert (B - 1) * stride * 12 > 1 << 32
    need = B * stride * (12 * 4 + 8 + 3)
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the buffers above 4 GiB do not fit the free device memory")
    small = pins_case(B=2, stride=n, seed=8)
    dev = "cuda:0"
    obs1, obs2 = (torch.empty((B, stride, 3), dtype=torch.int32, device=dev) for _ in range(2))
    l1, l2 = (torch.empty((B, stride), dtype=torch.uint8, device=dev) for _ in range(2))
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    xw, normal = (torch.empty((B, stride, 3), dtype=torch.float32, device=dev) for _ in range(2))
    drange = torch.empty((B, stride, 2), dtype=torch.float32, device=dev)
    status = torch.empty((B, stride), dtype=torch.uint8, device=dev)
    npoints = torch.full((B,), -1, dtype=torch.int32, device=dev)
    poses = {k: torch.zeros((B, 12 if k.startswith("pose") else 5), dtype=torch.float32, device=dev)
             for k in ("pose1", "pose2", "cam1", "cam2")}
    live = [0, B - 1]
    for k, b in enumerate(live):
        for name, t in poses.items():
            t[b] = to_dev(small[name][k])
        obs1[b, :n], obs2[b, :n] = to_dev(small["obs1"][k]), to_dev(small["obs2"][k])
        l1[b, :n], l2[b, :n] = to_dev(small["l1"][k]), to_dev(small["l2"][k])
        counts[b] = n
        for o in (xw, normal, drange):
            o[b, :n + 16] = float(SF)
        status[b, :n + 16] = S8
    for o in (xw, normal, drange):
        o[B - 2, :16] = float(SF)
    triangulateBatch(poses["pose1"], poses["pose2"], poses["cam1"], poses["cam2"], obs1, obs2, l1, l2, counts, level_scale=LS8,
                     level_sigma2=SG8, xw=xw, status=status, normal=normal, drange=drange, npoints=npoints, ctx=gpu_ctx,
                     **PAR)
    torch.cuda.synchronize()
    want = ref_call(dict(small, counts=np.array([n, n], np.uint32)))
    for k, b in enumerate(live):
        got = (xw[b, :n + 16].cpu().numpy(), status[b, :n + 16].cpu().numpy(), normal[b, :n + 16].cpu().numpy(),
               drange[b, :n + 16].cpu().numpy())
        for name, g, w in zip(NAMES, got, want):
            bits = (lambda a: a.view(np.uint32)) if g.dtype != np.uint8 else (lambda a: a)
            assert (bits(g[:n]) == bits(w[k, :n])).all(), (name, b)
            assert (bits(g[n:]) == bits(np.full_like(g[n:], SF if g.dtype != np.uint8 else S8))).all(), (name, "written past the count")
        assert int(npoints[b]) == int(want[4][k]) and want[4][k] > 20
    for o in (xw, normal, drange):
        assert (o[B - 2, :16].cpu().numpy().view(np.uint32) == np.full(1, SF, F32).view(np.uint32)[0]).all()
    assert int(npoints[B - 2]) == 0 and int(npoints[1]) == 0


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_triangulate_refusals_write_nothing(gpu_ctx):
    import torch
    from pislam_amd import capi
    from pislam_amd.frontend import triangulateBatch
    c = pins_case()
    t = device_case(c)
    B, stride = c["obs1"].shape[:2]
    u8 = lambda *shape: torch.full(shape, S8, dtype=torch.uint8, device="cuda:0")
    outs = dict(xw=u8(B, stride, 12).view(torch.float32).view(B, stride, 3), status=u8(B, stride),
                normal=u8(B, stride, 12).view(torch.float32).view(B, stride, 3),
                drange=u8(B, stride, 8).view(torch.float32).view(B, stride, 2), npoints=u8(B * 4).view(torch.int32))

    def call(**over):
        a = dict(t)
        o = dict(outs)
        kw = dict(PAR, level_scale=LS8, level_sigma2=SG8)
        for k in list(over):
            if k in a:
                a[k] = over.pop(k)
            elif k in o:
                o[k] = over.pop(k)
        kw.update(over)
        triangulateBatch(a["pose1"], a["pose2"], a["cam1"], a["cam2"], a["obs1"], a["obs2"], a["l1"], a["l2"], a["counts"],
                         ctx=gpu_ctx, **kw, **o)

    nan, inf = float("nan"), float("inf")
    ls = LS8.tolist()
    bad = dict(
        host_pose=dict(pose1=t["pose1"].cpu()), host_cam=dict(cam2=t["cam2"].cpu()), host_obs=dict(obs2=t["obs2"].cpu()),
        host_level=dict(l1=t["l1"].cpu()), host_counts=dict(counts=t["counts"].cpu()), host_xw=dict(xw=outs["xw"].cpu()),
        host_status=dict(status=outs["status"].cpu()), host_normal=dict(normal=outs["normal"].cpu()),
        host_drange=dict(drange=outs["drange"].cpu()), host_npoints=dict(npoints=outs["npoints"].cpu()),
        scale_zero=dict(level_scale=[0.0] + ls[1:]), scale_negative=dict(level_scale=[-1.0] + ls[1:]),
        scale_falls=dict(level_scale=ls[:3] + [ls[1]] + ls[4:]), scale_nan=dict(level_scale=ls[:7] + [nan]),
        scale_inf=dict(level_scale=ls[:7] + [inf]), sigma_zero=dict(level_sigma2=[0.0] * 8),
        sigma_nan=dict(level_sigma2=SG8.tolist()[:4] + [nan] * 4), sigma_inf=dict(level_sigma2=[inf] * 8),
        chi2_mono=dict(chi2_mono=0.0), chi2_mono_nan=dict(chi2_mono=nan), chi2_stereo=dict(chi2_stereo=-1.0),
        chi2_stereo_inf=dict(chi2_stereo=inf), ratio=dict(ratio_factor=0.0), ratio_inf=dict(ratio_factor=inf),
        parallax_nan=dict(cos_min_parallax=nan), overlap=dict(normal=outs["xw"]))
    call()                                                                   # the unmodified call is accepted
    torch.cuda.synchronize()
    assert (outs["status"] != S8).all()
    fresh = lambda: [o.view(torch.uint8).fill_(S8) for o in outs.values()]
    fresh()
    for name, over in bad.items():
        with pytest.raises(capi.PislamError, match=r"failed \(-1\)"):
            call(**over)
    # NULL where a pointer is required, tables of 0 and 17 entries, stride 0 and 16385: through the C interface
    p = capi.TriangulateParams(*[float(F32(PAR[k])) for k in PARAM_FIELDS])
    tab = (ctypes.c_float * 17)(*(LS8.tolist() + [5.0] * 9))
    sgt = (ctypes.c_float * 17)(*(SG8.tolist() + [25.0] * 9))
    args = [t["pose1"], t["pose2"], t["cam1"], t["cam2"], t["obs1"], t["obs2"], t["l1"], t["l2"], t["counts"]]
    o = [outs[k] for k in NAMES]

    def raw(args=args, o=o, p=ctypes.byref(p), tab=tab, sgt=sgt, nl=8, stride=stride, batch=B):
        return gpu_ctx.lib.pislam_triangulate_batch(gpu_ctx.h, p, *[capi.ptr(a) for a in args], tab, sgt, nl, stride, batch,
                                                    *[capi.ptr(a) for a in o])
    assert raw(batch=0) == 0                                                 # a no-op
    for k in range(9):
        assert raw(args=args[:k] + [None] + args[k + 1:]) == -1, k
    for k in (0, 1, 4):
        assert raw(o=o[:k] + [None] + o[k + 1:]) == -1, k
    assert raw(p=None) == -1 and raw(tab=None) == -1 and raw(sgt=None) == -1
    assert raw(nl=0) == -1 and raw(nl=17) == -1 and raw(stride=0) == -1 and raw(stride=16385) == -1 and raw(batch=-1) == -1
    torch.cuda.synchronize()
    for k, o_ in outs.items():
        assert (o_.view(torch.uint8) == S8).all(), ("a refused call wrote", k)


# ---- GPU: hipGraph, determinism --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_triangulate_is_hipgraph_capturable(gpu_ctx):
    """No workspace and no reserve: captured on a side stream with a context of its own, the replay equals the eager
    call; the graph keeps the host tables it was captured with."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import triangulateBatch
    c = pins_case(seed=5)
    want = ref_call(c)
    t = device_case(c)
    B, stride = c["obs1"].shape[:2]
    dev = torch.device("cuda:0")
    ls, sg = LS8.copy(), SG8.copy()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        outs = dict(xw=torch.zeros((B, stride, 3), dtype=torch.float32, device=dev),
                    status=torch.zeros((B, stride), dtype=torch.uint8, device=dev),
                    normal=torch.zeros((B, stride, 3), dtype=torch.float32, device=dev),
                    drange=torch.zeros((B, stride, 2), dtype=torch.float32, device=dev),
                    npoints=torch.zeros((B,), dtype=torch.int32, device=dev))

        def call(**o):
            return triangulateBatch(t["pose1"], t["pose2"], t["cam1"], t["cam2"], t["obs1"], t["obs2"], t["l1"], t["l2"],
                                    t["counts"], level_scale=ls, level_sigma2=sg, ctx=ctx, **PAR, **o)

        eager = call()                                                       # warm-up (module load) and the eager result
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(**outs)
        for o in outs.values():
            o.zero_()
        ls[:] = 5.0                                                          # the graph holds its own copy of the tables
        sg[:] = 0.001
        g.replay()
        side.synchronize()
        for a, k in zip(eager, NAMES):
            assert torch.equal(a.view(torch.uint8), outs[k].view(torch.uint8)), k
    assert_outputs(tuple(outs[k].cpu().numpy() for k in NAMES), want)


@pytest.mark.gpu
def test_gpu_triangulate_is_deterministic_across_calls_and_paddings(gpu_ctx):
    """Two calls give identical words, and so do two strides of the same slots."""
    c = pins_case(seed=6)
    first = run_triangulate(gpu_ctx, c)
    assert_outputs(run_triangulate(gpu_ctx, c), first)
    B, stride = c["obs1"].shape[:2]
    pad = stride + 333
    wide = dict(c)
    for k in ("obs1", "obs2", "l1", "l2"):
        a = np.zeros((B, pad) + c[k].shape[2:], c[k].dtype)
        a[:, :stride] = c[k]
        wide[k] = a
    padded = run_triangulate(gpu_ctx, wide)
    for name, g, w in zip(NAMES, padded, first):
        if name == "npoints":
            assert (g == w).all()
            continue
        assert (g[:, :stride].view(np.uint8) == w.view(np.uint8)).all(), name
        assert (g[:, stride:].view(np.uint8) == S8).all(), name
