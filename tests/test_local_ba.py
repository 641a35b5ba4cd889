"""pislam_local_ba_batch: batched local bundle adjustment (Schur-complement Levenberg).

The comment above pislam_local_ba_batch in include/pislam_hip.h is the contract.  This file restates it in numpy,
independently of the library (binary32 one operation at a time on arrays, the binary64 sums in the stated orders as
loops; the pose call's per-observation restatement of tests/test_pose_refine.py is reused with a pose and a camera per
observation).  The host probe (tools/probes/ba_host_check.cpp, the library's own arithmetic header under the host
compiler) must agree with it on every output word, a dense binary64 Levenberg without a Schur complement must reach the
same inliers and cost, and the library on the GPU must agree with the restatement (or, for large shapes, with the probe
that is pinned to it) on every output word."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import test_pose_refine as tp
from conftest import ROOT

F32, F64 = np.float32, np.float64
COUNT_INVALID = 0xFFFFFFFF
MONO = tp.MONO
SENT8 = 0xA5
BA_FIELDS = ["rounds", "iters", "huber_rounds", "min_obs", "eps"]
DEFAULT = (2, (5, 10), 1, 10, 1e-6)            # rounds, iters, huber_rounds, min_obs, eps
MAX_KF, MAX_FREE, MAX_PTS, MAX_STRIDE = 32, 16, 4096, 16384


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_obs_terms(w, Tf, Xf, robust):
    """Every observation of window w at the float32 poses Tf [nkf][12] and points Xf [npt][3]: live, chi2, th and the
    float32 terms cam [n][28], cross [n][18], pt [n][9]."""
    kf, pt = w["kf"].astype(np.int64), w["pt"].astype(np.int64)
    wt, bad = tp.frame_weights(dict(obs=w["obs"], level=w.get("level"), tab=w.get("tab")))
    T = np.ascontiguousarray(Tf[kf].T)                       # [12][n]: one pose per observation
    P = tp.ref_project(T, np.ascontiguousarray(w["cams"][kf].T), Xf[pt], w["obs"], wt)
    cam = tp.ref_terms(P, wt, robust)
    stereo, chi2, th = P["stereo"], P["chi2"], P["th"]
    Ju, Jv, Jr, eu, ev, er = P["Ju"], P["Jv"], P["Jr"], P["eu"], P["ev"], P["er"]
    with np.errstate(all="ignore"):
        wr = wt.astype(F32).copy()
        if robust:
            wr = np.where(chi2 > th, wt * np.sqrt(th / chi2), wr)
        Pu = [Ju[3] * T[j] + Ju[5] * T[6 + j] for j in range(3)]
        Pv = [Jv[4] * T[3 + j] + Jv[5] * T[6 + j] for j in range(3)]
        Pr = [Jr[3] * T[j] + Jr[5] * T[6 + j] for j in range(3)]
        cross, ptt = [], []
        for a in range(6):
            for j in range(3):
                s = Ju[a] * Pu[j] + Jv[a] * Pv[j]
                cross.append(np.where(stereo, s + Jr[a] * Pr[j], s) * wr)
        for j in range(3):
            for k in range(j, 3):
                s = Pu[j] * Pu[k] + Pv[j] * Pv[k]
                ptt.append(np.where(stereo, s + Pr[j] * Pr[k], s) * wr)
        for j in range(3):
            s = Pu[j] * eu + Pv[j] * ev
            ptt.append(np.where(stereo, s + Pr[j] * er, s) * wr)
    n = len(kf)
    cross = np.stack(cross, 1) if n else np.zeros((0, 18), F32)
    ptt = np.stack(ptt, 1) if n else np.zeros((0, 9), F32)
    assert cam.dtype == F32 and cross.dtype == F32 and ptt.dtype == F32
    return dict(live=P["live"] & ~bad, chi2=chi2, th=th, cam=cam, cross=cross, pt=ptt)


def ref_ba_pass(w, T, X, classify, robust, active):
    """One pass at the binary64 state (T [nfree][12], X [npt][3])."""
    nfree, npt, n = w["nfree"], len(w["xw"]), len(w["kf"])
    Tf = w["poses"].copy()
    Tf[:nfree] = T.astype(F32)
    E = ref_obs_terms(w, Tf, X.astype(F32), robust)
    if classify:
        with np.errstate(all="ignore"):
            active = E["live"] & (E["chi2"] <= E["th"])
    on = E["live"] & active
    V, sub = np.zeros((npt, 9)), np.zeros((npt, 3))
    for i in range(n):                                       # ascending i is ascending within every point
        if on[i]:
            p = w["pt"][i]
            V[p] = V[p] + E["pt"][i].astype(F64)
            sub[p] = sub[p] + np.array([F64(E["cam"][i][27]), 1.0, F64(E["chi2"][i])])
    return dict(S=tp.ref_tree(sub), on=on, cam=E["cam"], cross=E["cross"], V=V, active=active)


def ref_factor3(V, s):
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = V[0] * s, V[1], V[2], V[3] * s, V[4], V[5] * s
        f1, f2 = a01 / a00, a02 / a00
        b11, b12 = a11 - f1 * a01, a12 - f1 * a02
        b21, b22 = a12 - f2 * a01, a22 - f2 * a02
        f3 = b21 / b11
        c22 = b22 - f3 * b12
    return (a00, a01, a02, b11, b12, c22, f1, f2, f3), bool(a00 > 0.0) and bool(b11 > 0.0) and bool(c22 > 0.0)


def ref_sol3(F, b0, b1, b2):
    """Sol for arrays of right-hand sides (each element goes through the same operations)."""
    a00, a01, a02, b11, b12, c22, f1, f2, f3 = F
    with np.errstate(all="ignore"):
        b1 = b1 - f1 * b0
        b2 = b2 - f2 * b0
        b2 = b2 - f3 * b1
        x2 = b2 / c22
        x1 = (b1 - b12 * x2) / b11
        x0 = ((b0 - a01 * x1) - a02 * x2) / a00
    return np.stack([x0, x1, x2], -1)


def ref_ba_step(w, D, T, X, lam):
    """One solve at lam from the pass D: (ok, trial T, trial X, dmax)."""
    nfree, npt, n = w["nfree"], len(w["xw"]), len(w["kf"])
    kf, pt, on = w["kf"].astype(np.int64), w["pt"].astype(np.int64), D["on"]
    N = 6 * nfree
    s = F64(1.0) + F64(lam)
    fac, held = [], np.zeros(npt, bool)
    for p in range(npt):
        f, ok = ref_factor3(D["V"][p], s)
        fac.append(f)
        held[p] = not ok
    Wd = D["cross"].astype(F64).reshape(n, 6, 3)
    use = [bool(on[i] and kf[i] < nfree and not held[pt[i]]) for i in range(n)]
    Y = {i: ref_sol3(fac[pt[i]], Wd[i][:, 0], Wd[i][:, 1], Wd[i][:, 2]) for i in range(n) if use[i]}   # [6][3]
    klist = [[i for i in range(n) if kf[i] == k] for k in range(nfree)]
    slot = {(int(pt[i]), int(kf[i])): i for i in range(n)}
    A, rhs = np.zeros((N, N)), np.zeros(N)
    tri = [(j, k) for j in range(6) for k in range(j, 6)]
    for ki in range(nfree):
        H, g = np.zeros(21), np.zeros(6)
        for i in klist[ki]:
            if on[i]:
                H = H + D["cam"][i][:21].astype(F64)
                g = g + D["cam"][i][21:27].astype(F64)
        for kj in range(ki, nfree):
            acc = np.zeros((6, 6))
            if ki == kj:
                for o, (j, k) in enumerate(tri):
                    acc[j][k] = H[o] * s if j == k else H[o]
            for oi in klist[ki]:
                if not use[oi]:
                    continue
                oj = oi if ki == kj else slot.get((int(pt[oi]), kj))
                if oj is None or not on[oj]:
                    continue
                y, wv = Y[oi], Wd[oj]
                acc = acc - ((y[:, None, 0] * wv[None, :, 0] + y[:, None, 1] * wv[None, :, 1]) + y[:, None, 2] * wv[None, :, 2])
            for ai in range(6):
                for aj in range(6):
                    i, j = 6 * ki + ai, 6 * kj + aj
                    if j >= i:
                        A[i][j] = A[j][i] = acc[ai][aj]
        r = -g
        for oi in klist[ki]:
            if use[oi]:
                y, gp = Y[oi], D["V"][pt[oi]][6:9]
                r = r + ((y[:, 0] * gp[0] + y[:, 1] * gp[1]) + y[:, 2] * gp[2])
        rhs[6 * ki:6 * ki + 6] = r
    ok = True
    d = np.zeros(N)
    with np.errstate(all="ignore"):
        for c in range(N):
            ok = ok and bool(A[c][c] > 0.0)
            for r in range(c + 1, N):
                f = A[r][c] / A[c][c]
                A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
                rhs[r] = rhs[r] - f * rhs[c]
        if not ok:
            return False, None, None, None
        for r in range(N - 1, -1, -1):
            d[r] = rhs[r] / A[r][r]
            rhs[:r] = rhs[:r] - A[:r, r] * d[r]
        ok = bool(np.isfinite(d).all())
        dmax = F64(np.abs(d).max()) if N else F64(0.0)
        Xt = X.copy()
        first = np.searchsorted(pt, np.arange(npt + 1), side="left")
        for p in range(npt):
            if held[p]:
                continue
            b = -D["V"][p][6:9]
            for o in range(first[p], first[p + 1]):
                if on[o] and kf[o] < nfree:
                    e, wv = d[6 * kf[o]:6 * kf[o] + 6], Wd[o]
                    b = b - (((((wv[0] * e[0] + wv[1] * e[1]) + wv[2] * e[2]) + wv[3] * e[3]) + wv[4] * e[4]) + wv[5] * e[5])
            dp = ref_sol3(fac[p], b[0], b[1], b[2])
            ok = ok and bool(np.isfinite(dp).all())
            Xt[p] = X[p] + dp
            if np.isfinite(dp).all():
                dmax = max(dmax, F64(np.abs(dp).max()))
    if not ok:
        return False, None, None, None
    Tt = np.array([tp.ref_retract(T[k], d[6 * k:6 * k + 6]) for k in range(nfree)]).reshape(nfree, 12)
    return True, Tt, Xt, dmax


def window_code(w, min_obs):
    nkf, npt, n, nfree = len(w["poses"]), len(w["xw"]), len(w["kf"]), w["nfree"]
    kf, pt = w["kf"].astype(np.int64), w["pt"].astype(np.int64)
    key = pt * 256 + kf
    if nfree > MAX_FREE or nfree > nkf or (kf >= nkf).any() or (pt >= npt).any() or (np.diff(key) <= 0).any():
        return 3
    if not (np.isfinite(w["poses"]).all() and np.isfinite(w["cams"]).all() and np.isfinite(w["xw"]).all()):
        return 2
    return 1 if n < min_obs else 0


def ref_window(w, prm=DEFAULT):
    """One window of the call: dict(poses, xw, inlier, ninliers, cost, status)."""
    rounds, iters, hr, min_obs, eps = prm
    n, nfree = len(w["kf"]), w["nfree"]
    out = dict(poses=w["poses"].copy(), xw=w["xw"].copy(), inlier=np.zeros(n, np.uint8), ninliers=0, cost=0.0, status=0)
    out["status"] = window_code(w, min_obs)
    if out["status"]:
        return out
    T, X = w["poses"][:nfree].astype(F64), w["xw"].astype(F64)
    D = ref_ba_pass(w, T, X, False, 0 < hr, np.ones(n, bool))
    evals, code = 1, 0
    for r in range(rounds):
        lam = tp.LAMBDA_0
        for _ in range(iters[r]):
            ok, Tt, Xt, dmax = ref_ba_step(w, D, T, X, lam)
            if not ok:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
                continue
            Dt = ref_ba_pass(w, Tt, Xt, False, r < hr, D["active"])
            evals += 1
            if Dt["S"][0] < D["S"][0]:
                T, X, D, lam = Tt, Xt, Dt, max(lam * 0.25, tp.LAMBDA_MIN)
            else:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
            if dmax <= eps:
                break
        D = ref_ba_pass(w, T, X, True, r + 1 < hr, D["active"])
        evals += 1
        out["inlier"], out["ninliers"], out["cost"] = D["active"].astype(np.uint8), int(D["S"][1]), float(D["S"][2])
        if r + 1 < rounds and out["ninliers"] < min_obs:
            code = 1
            break
    out["poses"][:nfree] = T.astype(F32)
    out["xw"] = X.astype(F32)
    out["status"] = code | evals << 8
    return out


# ---- synthetic windows ----------------------------------------------------------------------------------------------
CAM = np.array([500.0, 500.0, 320.0, 240.0, 40.0], F32)
TAB = np.array([1.0, 0.69444448, 0.48225310, 0.33489800], F32)


def rot(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_window(seed, nkf=6, nfree=4, npt=60, seen=0.7, noise=0.5, gross=0.05, stereo=0.5, levels=True, start=1.0,
                min_seen=0, exact=0):
    """A window around a true scene: nkf cameras on an arc looking at npt points, each point seen with probability
    `seen` (at least min_seen times; exact > 0: by exactly that many cameras), noise px of noise, a share `gross` of the
    observations moved by 20 px, and a start
    off the truth by start * (0.002 rad, 0.01 of translation, 0.02 per point)."""
    rng = np.random.default_rng(seed)
    xw = np.stack([rng.uniform(-2, 2, npt), rng.uniform(-1.5, 1.5, npt), rng.uniform(4, 8, npt)], 1)
    poses, cams = np.zeros((nkf, 12)), np.zeros((nkf, 5), F32)
    for k in range(nkf):
        R = rot(np.array([0.0, 0.04 * (k - nkf / 2), 0.0]) + rng.normal(0, 0.01, 3))
        c = np.array([0.25 * (k - nkf / 2), rng.normal(0, 0.05), rng.normal(0, 0.05)])
        poses[k, :9], poses[k, 9:] = R.reshape(-1), -R @ c
        cams[k] = CAM * F32(1.0 + 0.02 * (k % 3))
        cams[k, 4] = CAM[4]
    kf, pt, obs, level = [], [], [], []
    for p in range(npt):
        vis = rng.random(nkf) < seen
        if exact:
            vis[:] = False
            vis[rng.choice(nkf, exact, replace=False)] = True
        while vis.sum() < min(min_seen, nkf):
            vis[rng.integers(nkf)] = True
        for k in range(nkf):
            if not vis[k]:
                continue
            xc = poses[k, :9].reshape(3, 3) @ xw[p] + poses[k, 9:]
            u = cams[k, 0] * xc[0] / xc[2] + cams[k, 2] + rng.normal(0, noise)
            v = cams[k, 1] * xc[1] / xc[2] + cams[k, 3] + rng.normal(0, noise)
            ur = u - cams[k, 4] / xc[2] + rng.normal(0, noise)
            if rng.random() < gross:
                a = rng.uniform(0, 2 * np.pi)
                u, v = u + 20 * np.cos(a), v + 20 * np.sin(a)
            st = rng.random() < stereo
            kf.append(k), pt.append(p), level.append(int(rng.integers(0, len(TAB))))
            obs.append([int(round(256 * u)), int(round(256 * v)), int(round(256 * ur)) if st else MONO])
    start_p = poses.copy()
    for k in range(nfree):
        R = rot(rng.normal(0, 0.002 * start / np.sqrt(3), 3)) @ poses[k, :9].reshape(3, 3)
        start_p[k, :9], start_p[k, 9:] = R.reshape(-1), poses[k, 9:] + rng.normal(0, 0.01 * start / np.sqrt(3), 3)
    w = dict(poses=start_p.astype(F32), cams=cams, nfree=nfree,
             xw=(xw + rng.normal(0, 0.02 * start / np.sqrt(3), xw.shape)).astype(F32),
             kf=np.array(kf, np.uint8), pt=np.array(pt, np.uint16), obs=np.array(obs, np.int64).reshape(-1, 3).astype(np.int32))
    if levels:
        w["level"], w["tab"] = np.array(level, np.uint8), TAB
    return w


def edit(w, **kw):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    out.update(kw)
    return out


def cases():
    """(name, window, parameters): what the issue lists; windows that share parameters make one GPU batch."""
    out = []
    base = make_window(1, nkf=4, nfree=2, npt=14, seen=0.8)
    out.append(("mixed_mono_stereo_levels", base, DEFAULT))
    w = edit(base)
    w["level"][3] = len(TAB)                                 # a level >= nlevels: dead
    w["level"][7] = 255
    out.append(("dead_level", w, DEFAULT))
    w = edit(base)
    w["xw"][2] = w["xw"][2] * F32(-1.0)                      # behind every camera
    out.append(("behind_camera", w, DEFAULT))
    w = edit(base)                                           # point 1: one observation; point 5: none
    keep = np.ones(len(w["kf"]), bool)
    keep[np.flatnonzero(w["pt"] == 1)[1:]] = False
    keep[w["pt"] == 5] = False
    for k in ("kf", "pt", "obs", "level"):
        w[k] = w[k][keep]
    out.append(("one_and_no_observation", w, DEFAULT))
    w = edit(base)                                           # every observation of point 4 is a gross outlier: held later
    for j, i in enumerate(np.flatnonzero(w["pt"] == 4)):
        w["obs"][i, :2] += 256 * 30 * (1 if j % 2 else -1)
        if w["obs"][i, 2] != MONO:
            w["obs"][i, 2] -= 256 * 25
    out.append(("point_of_outliers_held", w, DEFAULT))
    w = edit(base)                                           # free key frame 1 has no observation: every solve fails
    keep = w["kf"] != 1
    for k in ("kf", "pt", "obs", "level"):
        w[k] = w[k][keep]
    out.append(("free_key_frame_unobserved", w, DEFAULT))
    out.append(("points_only", edit(base, nfree=0), DEFAULT))
    out.append(("no_fixed_frame", edit(base, nfree=4), DEFAULT))
    out.append(("no_levels", {k: v for k, v in base.items() if k not in ("level", "tab")}, DEFAULT))
    other = make_window(2, nkf=5, nfree=3, npt=12, seen=0.8)
    out.append(("iters_differ_huber_0", other, (3, (2, 4, 3), 0, 5, 1e-6)))
    out.append(("huber_all_rounds", other, (2, (3, 2), 2, 5, 0.0)))
    out.append(("one_round", other, (1, (4,), 1, 5, 1e-3)))
    out.append(("code_1_at_start", edit(base), (2, (5, 10), 1, 4000, 1e-6)))
    w = edit(base)                                           # code 1 after round 0: nearly all observations are outliers
    w["obs"][5:, :2] += (256 * np.random.default_rng(3).choice([-70, -45, 45, 70], (len(w["obs"]) - 5, 2))).astype(np.int32)
    out.append(("code_1_after_round_0", w, DEFAULT))
    w = edit(base)
    w["xw"][3, 1] = np.inf
    out.append(("code_2_point", w, DEFAULT))
    w = edit(base)
    w["cams"][3, 4] = np.nan                                 # a fixed key frame's camera
    out.append(("code_2_camera", w, DEFAULT))
    w = edit(base)
    w["kf"][[4, 5]] = w["kf"][[5, 4]] if w["pt"][4] == w["pt"][5] else w["kf"][[4, 5]]
    w["pt"][9] = w["pt"][9] + 3                              # order violated
    out.append(("code_3_order", w, DEFAULT))
    out.append(("code_3_free", edit(base, nfree=5), DEFAULT))
    w = edit(base)
    w["pt"][-1] = 14                                         # a point beyond pt_counts
    out.append(("code_3_point", w, DEFAULT))
    return out


# ---- the host probe -------------------------------------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


def case_line(w, prm):
    rounds, iters, hr, min_obs, eps = prm
    its = list(iters) + [1] * (4 - len(iters))
    n = len(w["kf"])
    tab = w.get("tab")
    head = "%d %d %d %d %d %d %d %016x %d %d %d %d %d %d" % (
        rounds, its[0], its[1], its[2], its[3], hr, min_obs, np.array(eps, F64).view(np.uint64), int(tab is not None),
        0 if tab is None else len(tab), len(w["poses"]), w["nfree"], len(w["xw"]), n)
    parts = [head] + ([hexf(tab)] if tab is not None else [])
    for k in range(len(w["poses"])):
        parts += [hexf(w["poses"][k]), hexf(w["cams"][k])]
    parts.append(hexf(w["xw"]))
    lv = w["level"] if tab is not None else np.zeros(n, np.uint8)
    for i in range(n):
        parts.append("%d %d %d %d %d %d" % (w["kf"][i], w["pt"][i], w["obs"][i][0], w["obs"][i][1], w["obs"][i][2], lv[i]))
    return " ".join(p for p in parts if p)


@functools.lru_cache(maxsize=None)
def probe_exe():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix="ba_probe_"), "ba_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "ba_host_check.cpp"), "-o", exe])
    return exe


def probe(windows, prms):
    """The probe's outputs for the windows, as ref_window's dicts."""
    exe = probe_exe()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(case_line(w, p) for w, p in zip(windows, prms)) + "\n")
    try:
        got = subprocess.run([exe, f.name], check=True, capture_output=True, text=True).stdout.splitlines()
    finally:
        os.unlink(f.name)
    assert len(got) == len(windows)
    out = []
    for w, ln in zip(windows, got):
        t = ln.split()
        nkf, npt, n = len(w["poses"]), len(w["xw"]), len(w["kf"])
        words = np.array([int(x, 16) for x in t[3:3 + 12 * nkf + 3 * npt]], np.uint32).view(F32)
        assert len(t) == 4 + 12 * nkf + 3 * npt
        out.append(dict(status=int(t[0]), ninliers=int(t[1]), cost=float(np.array(int(t[2], 16), np.uint64).view(F64)),
                        poses=words[:12 * nkf].reshape(nkf, 12), xw=words[12 * nkf:].reshape(npt, 3),
                        inlier=np.array([c == "1" for c in t[-1]] if n else [], np.uint8)))
    return out


def assert_same(got, want, tag):
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    assert got["ninliers"] == want["ninliers"], tag
    assert np.array(got["cost"], F64).view(np.uint64) == np.array(want["cost"], F64).view(np.uint64), tag
    for k in ("poses", "xw"):
        assert np.asarray(got[k], F32).view(np.uint32).tolist() == np.asarray(want[k], F32).view(np.uint32).tolist(), (tag, k)
    assert np.asarray(got["inlier"]).tolist() == np.asarray(want["inlier"]).tolist(), tag


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def test_local_ba_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_local_ba_batch\s*\(", code) and re.search(r"\bint\s+pislam_local_ba_reserve\s*\(", code)
    m = re.search(r"typedef struct pislam_ba_params \{([^}]*)\} pislam_ba_params;", code)
    assert m, "pislam_ba_params is not declared"
    fields = re.findall(r"(int32_t|double)\s+(\w+)(\[4\])?\s*;", m.group(1))
    assert [f[1] for f in fields] == BA_FIELDS and [f[0] for f in fields] == ["int32_t"] * 4 + ["double"]
    assert fields[1][2] == "[4]"
    assert "#define PISLAM_ABI_VERSION 2" in text and "This comment is the contract" in text
    assert "HELD POINTS ARE THE NORMAL PATH" in text
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_local_ba_batch"][1]) == 25 and len(capi.SYMBOLS["pislam_local_ba_reserve"][1]) == 5
    assert [f[0] for f in capi.BaParams._fields_] == BA_FIELDS and ctypes.sizeof(capi.BaParams) == 40
    for f in ("localBundleAdjustBatch", "localWindow", "reserveLocalBundleAdjust"):
        assert callable(getattr(frontend, f))
    lib = capi.load()
    assert hasattr(lib, "pislam_local_ba_batch") and hasattr(lib, "pislam_local_ba_reserve")
    assert "ba_host_check.cpp" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()


def test_local_ba_probe_equals_the_restatement():
    cs = cases()
    got = probe([w for _, w, _ in cs], [p for _, _, p in cs])
    codes = set()
    for (name, w, prm), g in zip(cs, got):
        want = ref_window(w, prm)
        assert_same(g, want, name)
        codes.add(want["status"] & 255)
        if name.startswith("code_"):
            assert want["status"] & 255 == int(name[5]), name
        if name == "code_1_after_round_0":
            assert want["status"] >> 8 > 0
        if name == "free_key_frame_unobserved":              # no step was ever taken: the poses are the inputs
            assert want["status"] & 255 in (0, 1) and (want["poses"] == w["poses"]).all()
    assert codes == {0, 1, 2, 3}


def test_local_ba_holds_points_on_the_normal_path():
    """The window whose point 4 has only gross outliers: after round 0 the point has no active observation, is held
    (its block's first pivot is 0) and keeps the position round 0 gave it, while the rest of the window still moves."""
    name, w, prm = next(c for c in cases() if c[0] == "point_of_outliers_held")
    one = ref_window(w, (1, (5,), 1, 10, 1e-6))
    two = ref_window(w, prm)
    sel = w["pt"] == 4
    assert not one["inlier"][sel].any() and not two["inlier"][sel].any()
    assert two["xw"][4].tobytes() == one["xw"][4].tobytes()
    assert two["status"] & 255 == 0 and two["xw"].tobytes() != one["xw"].tobytes()


# ---- against a dense binary64 Levenberg without a Schur complement ------------------------------------------------------
def dense_residuals(w, T, X, active, robust, kfix=None):
    """Weighted residual rows (binary64) of the active observations at (T [nkf][12], X): (r [m], F, chi2 per observation,
    live, th, k).  kfix: the Huber factors to weight the rows with (those of the linearisation point: the robust
    weights are held fixed while the rows are differentiated, as in the contract and in ORB-SLAM's optimiser)."""
    kf, pt = w["kf"].astype(np.int64), w["pt"].astype(np.int64)
    obs = w["obs"].astype(F64) / 256.0
    stereo = w["obs"][:, 2] != MONO
    wt = w["tab"].astype(F64)[w["level"]] if w.get("tab") is not None else np.ones(len(kf))
    R, t, cam = T[kf, :9].reshape(-1, 3, 3), T[kf, 9:], w["cams"].astype(F64)[kf]
    xc = np.einsum("nij,nj->ni", R, X[pt]) + t
    live = xc[:, 2] >= 2.0 ** -10
    z = np.where(live, xc[:, 2], 1.0)
    pu, pv = cam[:, 0] * xc[:, 0] / z + cam[:, 2], cam[:, 1] * xc[:, 1] / z + cam[:, 3]
    e = np.stack([obs[:, 0] - pu, obs[:, 1] - pv, np.where(stereo, obs[:, 2] - (pu - cam[:, 4] / z), 0.0)], 1)
    chi2 = (e * e).sum(1) * wt
    th = np.where(stereo, 7.815, 5.991)
    k = np.ones(len(kf))
    rho = chi2.copy()
    if robust:
        hub = chi2 > th
        k = np.where(hub, np.sqrt(th / np.where(hub, chi2, 1.0)), 1.0)
        rho = np.where(hub, 2.0 * chi2 * k - th, chi2)
    use = live & active
    r = (e * np.sqrt(wt * (k if kfix is None else kfix))[:, None])[use].reshape(-1)
    return r, rho[use].sum(), chi2, live, th, k


def dense_lm(w, prm=DEFAULT):
    """Dense Levenberg on all 6 * nfree + 3 * npt unknowns: numerical Jacobian, np.linalg.lstsq on the damped normal
    equations, the call's damping rule, schedule and classification."""
    rounds, iters, hr, min_obs, eps = prm
    nfree, npt, n = w["nfree"], len(w["xw"]), len(w["kf"])
    T, X = w["poses"].astype(F64), w["xw"].astype(F64)
    P = 6 * nfree + 3 * npt

    def moved(T, X, d):
        Tn = T.copy()
        for k in range(nfree):
            Tn[k] = tp.ref_retract(T[k], d[6 * k:6 * k + 6])
        return Tn, X + d[6 * nfree:].reshape(npt, 3)

    active = np.ones(n, bool)
    for r in range(rounds):
        robust = r < hr
        lam = tp.LAMBDA_0
        for _ in range(iters[r]):
            r0, F, _, live, _, k0 = dense_residuals(w, T, X, active, robust)
            use = live & active
            J = np.zeros((len(r0), P))
            h = 1e-6
            for j in range(P):
                d = np.zeros(P)
                d[j] = h
                ra = dense_residuals(w, *moved(T, X, d), use, robust, k0)[0]
                rb = dense_residuals(w, *moved(T, X, -d), use, robust, k0)[0]
                J[:, j] = (ra - rb) / (2 * h)
            H, g = J.T @ J, J.T @ r0
            d = np.linalg.lstsq(H + lam * np.diag(np.diag(H)), -g, rcond=None)[0]
            Tt, Xt = moved(T, X, d)
            Ft = dense_residuals(w, Tt, Xt, active, robust)[1]
            if Ft < F:
                T, X, lam = Tt, Xt, max(lam * 0.25, tp.LAMBDA_MIN)
            else:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
            if np.abs(d).max() <= eps:
                break
        _, _, chi2, live, th, _ = dense_residuals(w, T, X, active, False)
        active = live & (chi2 <= th)
    return active, float(chi2[active].sum())


# The relative difference between the call's final cost (the probe's words) and the dense optimiser's, measured over the
# seeds 0 .. 7 of the window below with identical inlier masks: 3.2e-6, 3.74e-6, 2.43e-6, 1.63e-6, 2.26e-6, 3.69e-6, 3.47e-6,
# 2.4e-6.  The bound is 8 x the largest.  The difference is the binary32 evaluation of the residuals against the dense
# optimiser's binary64 (a cost near 100 summed from binary32 chi2 words).
DENSE_COST_RTOL = 8 * 3.74e-6
DENSE_SEEDS = list(range(8))


@functools.lru_cache(maxsize=None)
def dense_windows():
    return [make_window(100 + s, nkf=6, nfree=4, npt=60, seen=0.7, noise=0.5, gross=0.05, levels=False, min_seen=0)
            for s in DENSE_SEEDS]


@pytest.mark.parametrize("seed", DENSE_SEEDS)
def test_local_ba_against_a_dense_optimiser(seed):
    w = dense_windows()[seed]
    got = probe([w], [DEFAULT])[0]
    active, cost = dense_lm(w)
    rel = abs(got["cost"] - cost) / cost
    print("seed %d: n %d inliers %d cost %.6f dense %.6f rel %.3g" % (seed, len(w["kf"]), got["ninliers"], got["cost"], cost, rel))
    assert got["status"] & 255 == 0
    assert got["inlier"].astype(bool).tolist() == active.tolist()
    assert rel <= DENSE_COST_RTOL, (rel, DENSE_COST_RTOL)


# ---- GPU tests --------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.capi, self.ctx, self.lib = torch, capi, ctx, ctx.lib

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def sentinels(self, B, kfs, pts, stride):
        t = self.torch
        f = lambda *s: t.full(s, 0x5A5A5A5A, dtype=t.int32, device="cuda")
        return dict(poses_out=f(B, kfs, 12).view(t.float32), xw_out=f(B, pts, 3).view(t.float32),
                    inlier=t.full((B, stride), SENT8, dtype=t.uint8, device="cuda"), ninliers=f(B),
                    cost=f(B, 2).view(t.float64).reshape(B), status=f(B))

    def pack(self, windows, kfs, pts, stride, counts=None):
        """Host arrays of a batch: the slots at and beyond a window's counts hold rubbish that must not be read.
        counts: per window None or (kf_counts, pt_counts, counts) as given to the call (may exceed the strides)."""
        B = len(windows)
        rng = np.random.default_rng(7)
        h = dict(poses=rng.normal(0, 1e30, (B, kfs, 12)).astype(F32), cams=rng.normal(0, 1e30, (B, kfs, 5)).astype(F32),
                 xw=rng.normal(0, 1e30, (B, pts, 3)).astype(F32),
                 obs=rng.integers(-1 << 31, 1 << 31, (B, stride, 3)).astype(np.int32),
                 kf=rng.integers(0, 256, (B, stride)).astype(np.uint8), pt=rng.integers(0, 1 << 16, (B, stride)).astype(np.uint16),
                 level=rng.integers(0, 256, (B, stride)).astype(np.uint8), kf_counts=np.zeros(B, np.uint32),
                 kf_free=np.zeros(B, np.uint32), pt_counts=np.zeros(B, np.uint32), counts=np.zeros(B, np.uint32), tab=None)
        for b, w in enumerate(windows):
            nkf, npt, n = len(w["poses"]), len(w["xw"]), len(w["kf"])
            h["poses"][b, :nkf], h["cams"][b, :nkf], h["xw"][b, :npt] = w["poses"], w["cams"], w["xw"]
            h["obs"][b, :n], h["kf"][b, :n], h["pt"][b, :n] = w["obs"], w["kf"], w["pt"]
            if w.get("tab") is not None:
                h["level"][b, :n], h["tab"] = w["level"], w["tab"]
            c = (nkf, npt, n) if counts is None or counts[b] is None else counts[b]
            h["kf_counts"][b], h["pt_counts"][b], h["counts"][b], h["kf_free"][b] = c[0], c[1], c[2], w["nfree"]
        for k in ("kf_counts", "kf_free", "pt_counts", "counts"):
            h[k] = h[k].view(np.int32)
        h["pt"] = h["pt"].view(np.int16)
        return h

    def upload(self, h):
        return {k: (self.up(v) if k != "tab" and v is not None else v) for k, v in h.items()}

    def call(self, prm, d, shape, B, o, with_level=True):
        ptr = self.capi.ptr
        kfs, pts, stride = shape
        p = None
        if prm is not None:
            its = list(prm[1]) + [1] * (4 - len(prm[1]))
            p = self.capi.BaParams(prm[0], (ctypes.c_int32 * 4)(*its), prm[2], prm[3], prm[4])
        tab = d.get("tab") if with_level else None
        ctab = None if tab is None else (ctypes.c_float * len(tab))(*[float(v) for v in tab])
        return self.lib.pislam_local_ba_batch(
            self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["poses"]), ptr(d["cams"]), ptr(d["kf_counts"]),
            ptr(d["kf_free"]), ptr(d["xw"]), ptr(d["pt_counts"]), ptr(d["obs"]), ptr(d["kf"]), ptr(d["pt"]),
            ptr(d["level"]) if tab is not None else None, ptr(d["counts"]), ctab, 0 if tab is None else len(tab), kfs, pts,
            stride, B, ptr(o["poses_out"]), ptr(o["xw_out"]), ptr(o["inlier"]), ptr(o["ninliers"]), ptr(o["cost"]),
            ptr(o["status"]))

    def run(self, windows, prm, shape, counts=None):
        h = self.pack(windows, *shape, counts=counts)
        d = self.upload(h)
        o = self.sentinels(len(windows), *shape)
        assert self.call(prm, d, shape, len(windows), o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_windows(got, want, windows, what=""):
    """Every output word of every window, and the sentinels at and beyond the counts."""
    sent = np.array([0x5A5A5A5A], np.uint32)
    for b, (x, w) in enumerate(zip(want, windows)):
        nkf, npt, n = len(w["poses"]), len(w["xw"]), len(w["kf"])
        g = dict(status=int(got["status"][b]), ninliers=int(got["ninliers"][b]), cost=float(got["cost"][b]),
                 poses=got["poses_out"][b, :nkf], xw=got["xw_out"][b, :npt], inlier=got["inlier"][b, :n])
        assert_same(g, x, "%s window %d" % (what, b))
        assert (got["inlier"][b, n:] == SENT8).all(), (what, b)
        assert (got["poses_out"][b, nkf:].view(np.uint32) == sent).all() and (got["xw_out"][b, npt:].view(np.uint32) == sent).all()


def shape_of(windows, pad=(0, 0, 0)):
    return (max(max(len(w["poses"]) for w in windows) + pad[0], 1), max(max(len(w["xw"]) for w in windows) + pad[1], 1),
            max(max(len(w["kf"]) for w in windows) + pad[2], 1))


def smallest(seed):
    """2 key frames with 1 free, 8 points, 16 observations."""
    return make_window(seed, nkf=2, nfree=1, npt=8, seen=1.0, gross=0.0, levels=False)


SMALL_PRM = (2, (3, 4), 1, 4, 1e-6)


@pytest.mark.gpu
def test_local_ba_smallest_window(gpu_ctx):
    w = smallest(11)
    assert len(w["kf"]) == 16
    want = ref_window(w, SMALL_PRM)
    assert want["status"] & 255 == 0 and want["poses"].tobytes() != w["poses"].tobytes()
    got = Device(gpu_ctx).run([w], SMALL_PRM, (2, 8, 16))
    assert_windows(got, [want], [w], "smallest")


@pytest.mark.gpu
def test_local_ba_every_case_in_batches_with_unequal_counts(gpu_ctx):
    """The windows of the CPU test, one batch per parameter set, next to windows whose counts are 0 and
    PISLAM_COUNT_INVALID and one whose counts exceed the strides."""
    groups = {}
    for name, w, prm in cases():
        groups.setdefault(prm, []).append(w)
    empty = dict(poses=np.zeros((0, 12), F32), cams=np.zeros((0, 5), F32), nfree=0, xw=np.zeros((0, 3), F32),
                 kf=np.zeros(0, np.uint8), pt=np.zeros(0, np.uint16), obs=np.zeros((0, 3), np.int32),
                 level=np.zeros(0, np.uint8), tab=TAB)
    for prm, ws in groups.items():
        ws = [w for w in ws if w.get("tab") is not None]
        shape = shape_of(ws)
        full = next(w for w in ws if (len(w["poses"]), len(w["xw"]), len(w["kf"])) == shape)
        batch = ws + [empty, empty, full]
        counts = [None] * len(ws) + [(0, 0, 0), (COUNT_INVALID,) * 3, (shape[0] + 3, shape[1] + 9, shape[2] + 1)]
        want = [ref_window(w, prm) for w in batch]
        got = Device(gpu_ctx).run(batch, prm, shape, counts)
        assert_windows(got, want, batch, "%r" % (prm,))
    name, w, prm = next(c for c in cases() if c[0] == "no_levels")
    got = Device(gpu_ctx).run([w], prm, shape_of([w], (1, 2, 3)))
    assert_windows(got, [ref_window(w, prm)], [w], "no levels")


BOUNDARY_PRM = (2, (2, 3), 1, 10, 1e-6)


@functools.lru_cache(maxsize=None)
def boundary_windows():
    """255, 256 and 257 points; 257 and 513 observations; kf_free 15 and 16; kf_counts 32."""
    def cut(w, n):
        return edit(w, kf=w["kf"][:n], pt=w["pt"][:n], obs=w["obs"][:n], level=w["level"][:n])
    ws = [make_window(21, nkf=32, nfree=16, npt=255, seen=0.2, min_seen=2),
          make_window(22, nkf=32, nfree=15, npt=256, seen=0.2, min_seen=2),
          make_window(23, nkf=20, nfree=16, npt=257, seen=0.3, min_seen=2),
          cut(make_window(24, nkf=5, nfree=2, npt=100, seen=0.8), 257), cut(make_window(25, nkf=8, nfree=3, npt=120, seen=0.8), 513)]
    assert [len(w["kf"]) for w in ws[3:]] == [257, 513] and all(len(w["kf"]) > 513 for w in ws[:3])
    return ws


@pytest.mark.gpu
def test_local_ba_thread_and_tile_boundaries(gpu_ctx):
    ws = boundary_windows()
    want = probe(ws, [BOUNDARY_PRM] * len(ws))
    assert all(x["status"] & 255 == 0 for x in want)
    got = Device(gpu_ctx).run(ws, BOUNDARY_PRM, shape_of(ws))
    assert_windows(got, want, ws, "boundaries")


@pytest.mark.gpu
def test_local_ba_at_the_limits(gpu_ctx):
    """One window of 32 key frames with 16 free, 4096 points and 16384 observations."""
    w = make_window(31, nkf=32, nfree=16, npt=4096, exact=4, gross=0.02)
    assert len(w["kf"]) == MAX_STRIDE and int(w["pt"][-1]) == MAX_PTS - 1
    prm = (2, (2, 2), 1, 10, 1e-6)
    want = probe([w], [prm])
    assert want[0]["status"] & 255 == 0 and want[0]["status"] >> 8 >= 5
    got = Device(gpu_ctx).run([w], prm, (MAX_KF, MAX_PTS, MAX_STRIDE))
    assert_windows(got, want, [w], "limits")


@pytest.mark.gpu
def test_local_ba_second_pass_of_the_grid(gpu_ctx):
    ws = [smallest(1000 + b) for b in range(1025)]
    want = probe(ws, [SMALL_PRM] * len(ws))
    assert len({x["poses"].tobytes() for x in want}) == len(ws)
    got = Device(gpu_ctx).run(ws, SMALL_PRM, (2, 8, 16))
    assert_windows(got, want, ws, "1025 windows")


@pytest.mark.gpu
def test_local_ba_in_place_and_refusals(gpu_ctx):
    d = Device(gpu_ctx)
    t = d.torch
    ws = [make_window(41, nkf=4, nfree=2, npt=14, seen=0.8), make_window(42, nkf=3, nfree=3, npt=10, seen=0.9)]
    shape = shape_of(ws, (1, 3, 5))
    kfs, pts, stride = shape
    B = len(ws)
    h = d.pack(ws, *shape)
    dev = d.upload(h)
    o = d.sentinels(B, *shape)
    good = DEFAULT
    for prm in ((0, (5, 10), 0, 10, 1e-6), (5, (5, 10), 1, 10, 1e-6), (2, (5, 0), 1, 10, 1e-6), (2, (33, 10), 1, 10, 1e-6),
                (2, (5, 10), -1, 10, 1e-6), (2, (5, 10), 3, 10, 1e-6), (2, (5, 10), 1, 0, 1e-6), (2, (5, 10), 1, 16385, 1e-6),
                (2, (5, 10), 1, 10, -1e-9), (2, (5, 10), 1, 10, float("nan")), None):
        assert d.call(prm, dev, shape, B, o) == -1, prm
    for bad in ((0, pts, stride), (MAX_KF + 1, pts, stride), (kfs, 0, stride), (kfs, MAX_PTS + 1, stride), (kfs, pts, 0),
                (kfs, pts, MAX_STRIDE + 1)):
        assert d.call(good, dev, bad, B, o) == -1, bad
        assert d.lib.pislam_local_ba_reserve(gpu_ctx.h, bad[0], bad[1], bad[2], B) == -1, bad
    assert d.call(good, dev, shape, -1, o) == -1
    assert d.call(good, dict(dev, tab=[1.0] * 17), shape, B, o) == -1
    assert d.call(good, dict(dev, tab=[1.0, float("nan")]), shape, B, o) == -1
    host = np.zeros(B * stride * 3 + B * kfs * 12 + B * pts * 3, np.int32)
    for name in ("poses", "cams", "kf_counts", "kf_free", "xw", "pt_counts", "obs", "kf", "pt", "level", "counts",
                 "poses_out", "xw_out", "inlier", "ninliers", "cost", "status"):
        for repl in (None, host):                             # NULL, then a host pointer
            if name == "level" and repl is None:
                continue
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, shape, B, outs) == -1, name
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, dev, shape, B, dict(o, ninliers=dev["counts"])) == -1
    assert d.call(good, dev, shape, B, dict(o, inlier=dev["level"])) == -1
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["xw"])) == -1
    assert d.call(good, dev, shape, B, dict(o, xw_out=dev["poses"])) == -1
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["poses"].view(-1)[4:])) == -1
    assert d.call(good, dev, shape, B, dict(o, xw_out=dev["xw"].view(-1)[3:])) == -1
    assert d.call(good, dev, shape, B, dict(o, status=o["ninliers"])) == -1
    assert d.call(good, dev, shape, B, dict(o, xw_out=o["poses_out"])) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        a = v.cpu().numpy()
        assert (a == SENT8).all() if k == "inlier" else (a.view(np.uint8) == 0x5A).all(), k
    for k in ("poses", "cams", "xw"):
        assert dev[k].cpu().numpy().tobytes() == h[k].tobytes()
    # batch 0 is a no-op after the checks: the pointers are not looked at
    p = d.capi.BaParams(2, (ctypes.c_int32 * 4)(5, 10, 1, 1), 1, 10, 1e-6)
    assert d.lib.pislam_local_ba_batch(gpu_ctx.h, ctypes.byref(p), *([None] * 12), 0, kfs, pts, stride, 0, *([None] * 6)) == 0
    assert d.lib.pislam_local_ba_reserve(gpu_ctx.h, kfs, pts, stride, 0) == 0
    # poses_out may be poses and xw_out may be xw; nothing is written at or beyond the counts
    want = [ref_window(w, good) for w in ws]
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["poses"], xw_out=dev["xw"])) == 0
    gpu_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["poses_out"], got["xw_out"] = dev["poses"].cpu().numpy(), dev["xw"].cpu().numpy()
    for b, w in enumerate(ws):                                # beyond the counts the inputs' rubbish is untouched
        nkf, npt = len(w["poses"]), len(w["xw"])
        assert got["poses_out"][b, nkf:].tobytes() == h["poses"][b, nkf:].tobytes()
        assert got["xw_out"][b, npt:].tobytes() == h["xw"][b, npt:].tobytes()
        got["poses_out"][b, nkf:].view(np.uint32)[...] = 0x5A5A5A5A
        got["xw_out"][b, npt:].view(np.uint32)[...] = 0x5A5A5A5A
    assert_windows(got, want, ws, "in place")


@pytest.mark.gpu
def test_local_ba_determinism_and_graph_replay(gpu_ctx):
    """Two calls give the same bits; after pislam_local_ba_reserve on a fresh context the call is captured on a side
    stream without a warm-up call, and both replays write what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import localBundleAdjustBatch, reserveLocalBundleAdjust
    d = Device(gpu_ctx)
    ws = [make_window(51, nkf=5, nfree=3, npt=30, seen=0.8), make_window(52, nkf=3, nfree=1, npt=9, seen=1.0)]
    shape = shape_of(ws)
    h = d.pack(ws, *shape)
    dev = d.upload(h)
    args = (dev["poses"], dev["cams"], dev["kf_counts"], dev["kf_free"], dev["xw"], dev["pt_counts"], dev["obs"], dev["kf"],
            dev["pt"], dev["counts"])
    kw = dict(level=dev["level"], inv_sigma2=h["tab"])
    first = [x.cpu().numpy().copy() for x in localBundleAdjustBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(2, *shape))]
    again = [x.cpu().numpy().copy() for x in localBundleAdjustBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(2, *shape))]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    names = ("poses_out", "xw_out", "inlier", "ninliers", "cost", "status")
    assert_windows(dict(zip(names, first)), [ref_window(w) for w in ws], ws, "frontend")
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveLocalBundleAdjust(*shape, 2, ctx=ctx)
        o = d.sentinels(2, *shape)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            localBundleAdjustBatch(*args, ctx=ctx, **kw, **o)
        for _ in range(2):
            for k, x in o.items():
                x.view(t.uint8).fill_(SENT8 if k == "inlier" else 0x5A)
            g.replay()
            side.synchronize()
            for a, b in zip(first, o.values()):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        ctx.close()


@pytest.mark.gpu
def test_local_ba_chain_from_triangulation(gpu_ctx):
    """triangulateBatch's xw and the two poses go through localWindow into the call with no conversion in between: a
    pair of about 40 matches, the first key frame fixed (index 1), the second free (index 0)."""
    import torch as t
    from pislam_amd.frontend import localBundleAdjustBatch, localWindow, triangulateBatch
    rng = np.random.default_rng(61)
    n = 40
    levels = [(640, 480, 0, 0)]
    cam = CAM.copy()
    xw = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)
    R2, c2 = rot(np.array([0.0, -0.05, 0.0])), np.array([0.5, 0.0, 0.0])
    pose1 = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(F32)
    pose2 = np.concatenate([R2.reshape(-1), -R2 @ c2]).astype(F32)
    kps = []
    for P in (pose1, pose2):
        xc = xw @ P[:9].reshape(3, 3).astype(F64).T + P[9:]
        u = np.rint(cam[0] * xc[:, 0] / xc[:, 2] + cam[2] + rng.normal(0, 0.3, n)).astype(np.int64)
        v = np.rint(cam[1] * xc[:, 1] / xc[:, 2] + cam[3] + rng.normal(0, 0.3, n)).astype(np.int64)
        assert (u >= 0).all() and (u < 640).all() and (v >= 0).all() and (v < 480).all()
        kps.append((u << 12 | v).astype(np.int32))
    d = Device(gpu_ctx)
    from pislam_amd.frontend import poseObservationsQ8
    o1, l1 = poseObservationsQ8(d.up(kps[0][None]), levels)
    o2, l2 = poseObservationsQ8(d.up(kps[1][None]), levels)
    cnt = d.up(np.array([n], np.int32))
    p1, p2, cm = d.up(pose1[None]), d.up(pose2[None]), d.up(cam[None])
    pts, st, _, _, npoints = triangulateBatch(p1, p2, cm, cm, o1, o2, l1, l2, cnt, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert int(npoints[0]) >= 30
    # the window: key frame 0 = the second (free), key frame 1 = the first (fixed); only triangulated slots are observed
    ok = (st[0] == 0).cpu().numpy() if st.dtype != t.bool else st[0].cpu().numpy()
    made = np.flatnonzero(ok)
    okf = np.concatenate([np.ones(len(made)), np.zeros(len(made))]).astype(np.int32)      # any order: localWindow sorts
    opt = np.concatenate([made, made]).astype(np.int32)
    okp = np.concatenate([kps[0][made], kps[1][made]]).astype(np.int32)
    obs, wkf, wpt, wlv, wcnt = localWindow(d.up(okf[None]), d.up(opt[None]), d.up(okp[None]), d.up(np.array([len(okf)], np.int32)),
                                           levels)
    poses = t.stack([p2, p1], 1).contiguous()
    cams = t.stack([cm, cm], 1).contiguous()
    one = lambda v: d.up(np.array([v], np.int32))
    prm = (2, (5, 10), 1, 10, 1e-6)
    out = localBundleAdjustBatch(poses, cams, one(2), one(1), pts, one(n), obs, wkf, wpt, wcnt, level=wlv, inv_sigma2=[1.0],
                                 ctx=gpu_ctx)
    gpu_ctx.synchronize()
    w = dict(poses=poses[0].cpu().numpy(), cams=cams[0].cpu().numpy(), nfree=1, xw=pts[0].cpu().numpy(),
             kf=wkf[0].cpu().numpy(), pt=wpt[0].cpu().numpy().view(np.uint16), obs=obs[0].cpu().numpy(),
             level=wlv[0].cpu().numpy(), tab=np.ones(1, F32))
    assert (np.diff(w["pt"].astype(np.int64) * 64 + w["kf"]) > 0).all() and len(w["kf"]) == 2 * len(made)
    want = ref_window(w, prm)
    assert want["status"] & 255 == 0 and want["ninliers"] >= 2 * len(made) - 4
    got = dict(zip(("poses_out", "xw_out", "inlier", "ninliers", "cost", "status"), [x.cpu().numpy() for x in out]))
    assert_windows(dict(got, inlier=np.concatenate([got["inlier"], np.full((1, 0), SENT8, np.uint8)], 1)), [want], [w], "chain")
