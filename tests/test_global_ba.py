"""pislam_global_ba_batch: global bundle adjustment of whole maps across workgroups (Schur-complement PCG).

The comment above pislam_global_ba_batch in include/pislam_hip.h is the contract.  This file restates it in numpy,
independently of the library (the per-observation restatement and the point blocks of tests/test_local_ba.py are reused:
that part of the contract is the local call's word for word; the 64-partial key-frame sums, the preconditioner blocks,
the conjugate gradients and the refusals are restated here as loops).  The host probe (tools/probes/gba_host_check.cpp,
the library's own arithmetic header under the host compiler, run phase by phase in the order of the launches) must agree
with the restatement on every output word and on the PCG iteration count of every solve; it must reach what a dense
binary64 Levenberg without a Schur complement reaches, and what the local call's probe reaches on windows both accept; and
the library on the GPU must agree with the probe (which is pinned to the restatement) on every output word."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import test_local_ba as tl
import test_pose_refine as tp
from conftest import ROOT

F32, F64 = np.float32, np.float64
MONO = tp.MONO
SENT8 = 0xA5
COUNT_INVALID = 0xFFFFFFFF
MAX_KF, MAX_PTS, MAX_STRIDE, MAX_CG = 4096, 1 << 22, 1 << 24, 256
# rounds, iters, huber_rounds, min_obs, eps, cg_iters, cg_tol
ORB = (1, (10,), 1, 10, 1e-6, 50, 1e-4)
DEFAULT = (2, (4, 5), 1, 10, 1e-6, 30, 1e-6)


# ---- maps -------------------------------------------------------------------------------------------------------------
def kf_index(kf, nk):
    """The key-frame side of an observation list: (kf_ptr [nk + 1], kf_obs [n])."""
    kf = np.asarray(kf, np.int64)
    order = np.argsort(kf, kind="stable").astype(np.uint32)
    ptr = np.zeros(nk + 1, np.uint32)
    ptr[1:] = np.cumsum(np.bincount(kf, minlength=nk)[:nk])
    return ptr, order


def from_window(w, fixed=None):
    """A window of tests/test_local_ba.py as a map: the key frames from nfree on are fixed (or `fixed` as given)."""
    nk = len(w["poses"])
    m = dict(poses=w["poses"].copy(), cams=w["cams"].copy(), xw=w["xw"].copy(), kf=w["kf"].astype(np.uint16),
             pt=w["pt"].astype(np.int32), obs=w["obs"].copy(),
             fixed=(np.arange(nk) >= w["nfree"]).astype(np.uint8) if fixed is None else np.asarray(fixed, np.uint8))
    if w.get("tab") is not None:
        m["level"], m["tab"] = w["level"].copy(), w["tab"]
    m["kf_ptr"], m["kf_obs"] = kf_index(m["kf"], nk) if (m["kf"] < nk).all() else (np.zeros(nk + 1, np.uint32), np.arange(len(m["kf"]), dtype=np.uint32))
    return m


def edit(m, **kw):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}
    out.update(kw)
    return out


def reindex(m):
    m["kf_ptr"], m["kf_obs"] = kf_index(m["kf"], len(m["poses"]))
    return m


def keep_obs(m, keep):
    out = edit(m)
    for k in ("kf", "pt", "obs", "level"):
        if k in out:
            out[k] = out[k][keep]
    return reindex(out)


def counts_of(m):
    """(count, kf_count) as given to the call, and the strides they are checked against."""
    n, nk = len(m["kf"]), len(m["poses"])
    return m.get("count", n), m.get("kf_count", nk), m.get("stride", max(n, 1)), m.get("kf_stride", max(nk, 1))


# ---- the restatement --------------------------------------------------------------------------------------------------
def halve(part):
    part = np.array(part, F64)
    h = len(part) // 2
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def part64(entries, qualifies, term, dim):
    """A 64-partial sum over a key frame's entries: partial q takes the places q, q + 64, .. in ascending order."""
    p = np.zeros((64, dim))
    for place, o in enumerate(entries):
        if qualifies(o):
            p[place % 64] = p[place % 64] + term(o)
    return halve(p)


def kf_sum(values):
    """A sum over the free key frames: values is {k: term}."""
    p = np.zeros(256)
    for k in sorted(values):
        p[k % 256] = p[k % 256] + values[k]
    return halve(p)


def dot6(a, b):
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]


def factor6(B):
    A, ok = B.copy(), True
    for c in range(6):
        ok = ok and bool(A[c, c] > 0.0)
        for r in range(c + 1, 6):
            f = A[r, c] / A[c, c]
            A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
            A[r, c] = f
    return A, ok


def sol6(A, b):
    b, x = b.copy(), np.zeros(6)
    for c in range(6):
        for r in range(c + 1, 6):
            b[r] = b[r] - A[r, c] * b[c]
    for r in range(5, -1, -1):
        t = b[r]
        for j in range(r + 1, 6):
            t = t - A[r, j] * x[j]
        x[r] = t / A[r, r]
    return x


def ref_pass(m, T, X, classify, robust, active):
    """One pass at the binary64 state (T [nk][12] with the fixed poses as given, X [npt][3])."""
    npt, n = len(m["xw"]), len(m["kf"])
    E = tl.ref_obs_terms(m, T.astype(F32), X.astype(F32), robust)
    if classify:
        with np.errstate(all="ignore"):
            active = E["live"] & (E["chi2"] <= E["th"])
    on = E["live"] & active
    V, sub = np.zeros((npt, 9)), np.zeros((npt, 3))
    for i in range(n):
        if on[i]:
            p = m["pt"][i]
            V[p] = V[p] + E["pt"][i].astype(F64)
            sub[p] = sub[p] + np.array([F64(E["cam"][i][27]), 1.0, F64(E["chi2"][i])])
    return dict(S=tp.ref_tree(sub), on=on, cam=E["cam"], cross=E["cross"], V=V, active=active)


def cross_t(wv, e):
    return ((((wv[0] * e[0] + wv[1] * e[1]) + wv[2] * e[2]) + wv[3] * e[3]) + wv[4] * e[4]) + wv[5] * e[5]


def ref_solve(m, D, T, X, lam, cg_iters, cg_tol):
    """One solve at lam from the pass D: (ok, trial T, trial X, dmax, PCG iterations, points held)."""
    nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
    kf, pt, on = m["kf"].astype(np.int64), m["pt"].astype(np.int64), D["on"]
    free = [k for k in range(nk) if not m["fixed"][k]]
    s = F64(1.0) + F64(lam)
    with np.errstate(all="ignore"):
        fac, held = [], np.zeros(npt, bool)
        for p in range(npt):
            f, ok = tl.ref_factor3(D["V"][p], s)
            fac.append(f)
            held[p] = not ok
        nheld = int(held.sum())
        Wd = D["cross"].astype(F64).reshape(n, 6, 3)
        takes = lambda o: bool(on[o] and not held[pt[o]])
        ent = {k: [int(o) for o in m["kf_obs"][m["kf_ptr"][k]:m["kf_ptr"][k + 1]]] for k in free}
        tri = [(a, b) for a in range(6) for b in range(a, 6)]
        Hd, fk, x, r, z, pv, ok = {}, {}, {}, {}, {}, {}, True
        for k in free:
            HG = part64(ent[k], lambda o: bool(on[o]), lambda o: D["cam"][o][:27].astype(F64), 27)
            Y = {o: tl.ref_sol3(fac[pt[o]], Wd[o][:, 0], Wd[o][:, 1], Wd[o][:, 2]) for o in ent[k] if takes(o)}
            E = part64(ent[k], takes, lambda o: np.array([(Y[o][a][0] * Wd[o][b][0] + Y[o][a][1] * Wd[o][b][1]) + Y[o][a][2] * Wd[o][b][2]
                                                         for a, b in tri]), 21)
            e = part64(ent[k], takes, lambda o: (Y[o][:, 0] * D["V"][pt[o]][6] + Y[o][:, 1] * D["V"][pt[o]][7]) + Y[o][:, 2] * D["V"][pt[o]][8], 6)
            H, B = np.zeros((6, 6)), np.zeros((6, 6))
            for o_, (a, b) in enumerate(tri):
                H[a, b] = H[b, a] = HG[o_] * s if a == b else HG[o_]
                B[a, b] = B[b, a] = H[a, b] - E[o_]
            Hd[k] = H
            fk[k], good = factor6(B)
            ok = ok and good
            r[k] = -HG[21:27] + e
            z[k] = sol6(fk[k], r[k])
            pv[k], x[k] = z[k].copy(), np.zeros(6)
        ncg = 0
        if ok:
            rz = kf_sum({k: dot6(r[k], z[k]) for k in free})
            thr = (F64(cg_tol) * F64(cg_tol)) * rz
            first = np.searchsorted(pt, np.arange(npt + 1), side="left")
            for _ in range(cg_iters):
                if rz <= thr:
                    break
                ncg += 1
                q = np.zeros((npt, 3))
                for p in range(npt):
                    if held[p]:
                        continue
                    t = np.zeros(3)
                    for o in range(first[p], first[p + 1]):
                        if on[o] and not m["fixed"][kf[o]]:
                            t = t + cross_t(Wd[o], pv[kf[o]])
                    q[p] = tl.ref_sol3(fac[p], t[0], t[1], t[2])
                Sp = {}
                for k in free:
                    Eq = part64(ent[k], takes, lambda o: (Wd[o][:, 0] * q[pt[o]][0] + Wd[o][:, 1] * q[pt[o]][1]) + Wd[o][:, 2] * q[pt[o]][2], 6)
                    Sp[k] = np.array([dot6(Hd[k][a], pv[k]) for a in range(6)]) - Eq
                pAp = kf_sum({k: dot6(pv[k], Sp[k]) for k in free})
                if not pAp > 0.0:
                    ok = False
                    break
                alpha = rz / pAp
                for k in free:
                    x[k] = x[k] + alpha * pv[k]
                    r[k] = r[k] - alpha * Sp[k]
                    z[k] = sol6(fk[k], r[k])
                rz1 = kf_sum({k: dot6(r[k], z[k]) for k in free})
                beta = rz1 / rz
                for k in free:
                    pv[k] = z[k] + beta * pv[k]
                rz = rz1
        if not ok:
            return False, None, None, None, ncg, nheld
        dmax = F64(0.0)
        Tt, Xt = T.copy(), X.copy()
        first = np.searchsorted(pt, np.arange(npt + 1), side="left")
        for p in range(npt):
            if held[p]:
                continue
            b = -D["V"][p][6:9]
            for o in range(first[p], first[p + 1]):
                if on[o] and not m["fixed"][kf[o]]:
                    b = b - cross_t(Wd[o], x[kf[o]])
            dp = tl.ref_sol3(fac[p], b[0], b[1], b[2])
            ok = ok and bool(np.isfinite(dp).all())
            Xt[p] = X[p] + dp
            if np.isfinite(dp).all():
                dmax = max(dmax, F64(np.abs(dp).max()))
        for k in free:
            ok = ok and bool(np.isfinite(x[k]).all())
            if np.isfinite(x[k]).all():
                dmax = max(dmax, F64(np.abs(x[k]).max()))
            Tt[k] = np.asarray(tp.ref_retract(T[k], x[k])).reshape(12)
    if not ok:
        return False, None, None, None, ncg, nheld
    return True, Tt, Xt, dmax, ncg, nheld


def map_code(m, min_obs):
    count, kf_count, stride, kf_stride = counts_of(m)
    if not (0 <= count <= stride and 0 <= kf_count <= kf_stride):
        return 3
    nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
    kf, pt = m["kf"].astype(np.int64), m["pt"].astype(np.int64)
    if (kf >= nk).any() or (pt < 0).any() or (pt >= npt).any() or (np.diff(pt * 65536 + kf) <= 0).any():
        return 3
    ptr, ko = m["kf_ptr"].astype(np.int64), m["kf_obs"].astype(np.int64)
    for k in range(nk):
        a, b = ptr[k], ptr[k + 1]
        if not (a <= b <= n and (k != 0 or a == 0) and (k + 1 != nk or b == n)):
            return 3
        for j in range(a, b):
            if not (ko[j] < n and kf[ko[j]] == k and (j == a or ko[j - 1] < ko[j])):
                return 3
    if not (np.isfinite(m["poses"]).all() and np.isfinite(m["cams"]).all() and np.isfinite(m["xw"]).all()):
        return 2
    return 1 if n < min_obs or m["fixed"].all() else 0


def ref_map(m, prm=DEFAULT):
    """One map of the call: dict(poses, xw, inlier, ninliers, cost, status, cg: the PCG iterations of every solve)."""
    rounds, iters, hr, min_obs, eps, cg_iters, cg_tol = prm
    n = len(m["kf"])
    out = dict(poses=m["poses"].copy(), xw=m["xw"].copy(), inlier=np.zeros(n, np.uint8), ninliers=0, cost=0.0, cg=[],
               fails=0, rejects=0, held=0)
    out["status"] = map_code(m, min_obs)
    if out["status"]:
        return out
    T, X = m["poses"].astype(F64), m["xw"].astype(F64)
    D = ref_pass(m, T, X, False, 0 < hr, np.ones(n, bool))
    evals, code = 1, 0
    for r in range(rounds):
        lam = tp.LAMBDA_0
        for _ in range(iters[r]):
            ok, Tt, Xt, dmax, ncg, nheld = ref_solve(m, D, T, X, lam, cg_iters, cg_tol)
            out["cg"].append(ncg)
            out["held"] = max(out["held"], nheld)
            if not ok:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
                out["fails"] += 1
                continue
            Dt = ref_pass(m, Tt, Xt, False, r < hr, D["active"])
            evals += 1
            if Dt["S"][0] < D["S"][0]:
                T, X, D, lam = Tt, Xt, Dt, max(lam * 0.25, tp.LAMBDA_MIN)
            else:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
                out["rejects"] += 1
            if dmax <= eps:
                break
        D = ref_pass(m, T, X, True, r + 1 < hr, D["active"])
        evals += 1
        out["inlier"], out["ninliers"], out["cost"] = D["active"].astype(np.uint8), int(D["S"][1]), float(D["S"][2])
        if r + 1 < rounds and out["ninliers"] < min_obs:
            code = 1
            break
    free = m["fixed"] == 0
    out["poses"][free] = T.astype(F32)[free]
    out["xw"] = X.astype(F32)
    out["status"] = code | evals << 8
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------
def smallest(seed=11):
    """One fixed and one free key frame, three points, six stereo observations."""
    return from_window(tl.make_window(seed, nkf=2, nfree=1, npt=3, seen=1.0, gross=0.0, stereo=1.0, levels=False))


SMALL_PRM = (2, (3, 4), 1, 4, 1e-6, 8, 1e-6)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, map, parameters): what the issue lists."""
    out = [("smallest", smallest(), SMALL_PRM)]
    win = tl.make_window(1, nkf=5, nfree=3, npt=16, seen=0.8)
    base = from_window(win, fixed=[0, 0, 1, 0, 0])           # the fixed key frame in the middle: the mask, not a prefix
    out.append(("mixed_mono_stereo_levels", base, DEFAULT))
    m = edit(base)
    m["level"][3], m["level"][7] = len(tl.TAB), 255
    out.append(("dead_level", m, DEFAULT))
    m = edit(base)
    m["xw"][2] = m["xw"][2] * F32(-1.0)
    out.append(("behind_camera", m, DEFAULT))
    keep = np.ones(len(base["kf"]), bool)
    keep[np.flatnonzero(base["pt"] == 1)[1:]] = False
    keep[base["pt"] == 5] = False
    out.append(("one_and_no_observation", keep_obs(base, keep), DEFAULT))
    m = edit(base)
    for j, i in enumerate(np.flatnonzero(m["pt"] == 4)):
        m["obs"][i, :2] += 256 * 30 * (1 if j % 2 else -1)
        if m["obs"][i, 2] != MONO:
            m["obs"][i, 2] -= 256 * 25
    out.append(("point_of_outliers_held", m, DEFAULT))
    out.append(("free_key_frame_unobserved", keep_obs(base, base["kf"] != 1), DEFAULT))
    out.append(("code_1_no_free_key_frame", edit(base, fixed=np.ones(5, np.uint8)), DEFAULT))
    out.append(("two_fixed_key_frames", edit(base, fixed=np.array([1, 0, 0, 0, 1], np.uint8)), DEFAULT))
    out.append(("no_fixed_key_frame", edit(base, fixed=np.zeros(5, np.uint8)), DEFAULT))
    out.append(("no_levels", {k: v for k, v in base.items() if k not in ("level", "tab")}, DEFAULT))
    other = from_window(tl.make_window(2, nkf=6, nfree=4, npt=14, seen=0.8))
    out.append(("stops_on_tolerance", other, (1, (3,), 1, 5, 1e-6, 200, 1e-3)))
    out.append(("stops_at_cg_iters", other, (1, (3,), 1, 5, 1e-6, 2, 0.0)))
    out.append(("rejected_step", from_window(tl.make_window(6, nkf=4, nfree=3, npt=12, seen=0.9, start=200.0)), (1, (6,), 0, 5, 1e-6, 30, 1e-6)))
    out.append(("no_robust_round", other, (3, (2, 3, 2), 0, 5, 1e-6, 20, 1e-6)))
    out.append(("only_robust_rounds", other, (2, (3, 2), 2, 5, 0.0, 20, 1e-6)))
    out.append(("code_1_at_start", base, (2, (4, 5), 1, 4000, 1e-6, 30, 1e-6)))
    m = edit(base)
    m["obs"][5:, :2] += (256 * np.random.default_rng(3).choice([-70, -45, 45, 70], (len(m["obs"]) - 5, 2))).astype(np.int32)
    out.append(("code_1_after_round_0", m, DEFAULT))
    m = edit(base)
    m["xw"][3, 1] = np.inf
    out.append(("code_2_point", m, DEFAULT))
    m = edit(base)
    m["cams"][2, 4] = np.nan                                 # the fixed key frame's camera
    out.append(("code_2_camera", m, DEFAULT))
    m = edit(base)
    m["poses"][0, 9] = -np.inf
    out.append(("code_2_pose", m, DEFAULT))
    m = edit(base)
    m["pt"][9] = m["pt"][9] + 3
    out.append(("code_3_order", m, DEFAULT))
    m = edit(base)
    m["pt"][-1] = 16
    out.append(("code_3_point_beyond", m, DEFAULT))
    m = edit(base)
    m["pt"][0] = -1
    out.append(("code_3_point_negative", m, DEFAULT))
    m = edit(base)
    m["kf"][-1] = 5
    out.append(("code_3_key_frame_beyond", m, DEFAULT))
    empty = dict(poses=np.zeros((0, 12), F32), cams=np.zeros((0, 5), F32), xw=base["xw"].copy(), kf=np.zeros(0, np.uint16),
                 pt=np.zeros(0, np.int32), obs=np.zeros((0, 3), np.int32), level=np.zeros(0, np.uint8), tab=tl.TAB,
                 fixed=np.zeros(0, np.uint8), kf_ptr=np.zeros(1, np.uint32), kf_obs=np.zeros(0, np.uint32))
    out.append(("code_3_count_negative", edit(empty, count=-1, kf_count=5, stride=80, kf_stride=5), DEFAULT))
    out.append(("code_3_count_beyond", edit(empty, count=81, kf_count=5, stride=80, kf_stride=5), DEFAULT))
    out.append(("code_3_kf_count_negative", edit(empty, count=10, kf_count=-3, stride=80, kf_stride=5), DEFAULT))
    out.append(("code_3_kf_count_beyond", edit(empty, count=10, kf_count=6, stride=80, kf_stride=5), DEFAULT))
    out.append(("code_1_empty", edit(empty, count=0, kf_count=0, stride=80, kf_stride=5), DEFAULT))
    # every way the kf_obs index can be inconsistent
    n = len(base["kf"])
    m = edit(base)
    m["kf_ptr"][0] = 1
    out.append(("code_3_index_first", m, DEFAULT))
    m = edit(base)
    m["kf_ptr"][5] = n - 1
    out.append(("code_3_index_last", m, DEFAULT))
    m = edit(base)
    m["kf_ptr"][2], m["kf_ptr"][3] = base["kf_ptr"][3], base["kf_ptr"][2]
    out.append(("code_3_index_descending_ptr", m, DEFAULT))
    m = edit(base)
    m["kf_ptr"][3] = n + 7
    out.append(("code_3_index_ptr_beyond", m, DEFAULT))
    m = edit(base)
    m["kf_obs"][4] = n
    out.append(("code_3_index_entry_beyond", m, DEFAULT))
    m = edit(base)
    a, b = int(base["kf_ptr"][1]), int(base["kf_ptr"][2])
    m["kf_obs"][a], m["kf_obs"][b] = base["kf_obs"][b], base["kf_obs"][a]       # two entries in each other's key frame
    out.append(("code_3_index_wrong_key_frame", m, DEFAULT))
    m = edit(base)
    m["kf_obs"][a], m["kf_obs"][a + 1] = base["kf_obs"][a + 1], base["kf_obs"][a]
    out.append(("code_3_index_not_ascending", m, DEFAULT))
    m = edit(base)
    m["kf_obs"][a + 1] = base["kf_obs"][a]                   # an entry twice
    out.append(("code_3_index_entry_twice", m, DEFAULT))
    return out


# ---- the host probe ---------------------------------------------------------------------------------------------------
def hexf(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


def case_line(m, prm):
    rounds, iters, hr, min_obs, eps, cg_iters, cg_tol = prm
    its = list(iters) + [1] * (4 - len(iters))
    count, kf_count, stride, kf_stride = counts_of(m)
    n, nk = len(m["kf"]), len(m["poses"])
    tab = m.get("tab")
    head = "%d %d %d %d %d %d %d %016x %d %016x %d %d %d %d %d %d %d" % (
        rounds, its[0], its[1], its[2], its[3], hr, min_obs, np.array(eps, F64).view(np.uint64), cg_iters,
        np.array(cg_tol, F64).view(np.uint64), int(tab is not None), 0 if tab is None else len(tab), count, kf_count,
        len(m["xw"]), stride, kf_stride)
    parts = [head] + ([hexf(tab)] if tab is not None else [])
    for k in range(nk):
        parts += [hexf(m["poses"][k]), hexf(m["cams"][k]), "%d" % m["fixed"][k]]
    parts.append(" ".join("%d" % v for v in m["kf_ptr"]))
    parts.append(hexf(m["xw"]))
    lv = m["level"] if tab is not None else np.zeros(n, np.uint8)
    rows = np.column_stack([m["kf"].astype(np.int64), m["pt"].astype(np.int64), m["obs"].astype(np.int64), lv.astype(np.int64),
                            m["kf_obs"].astype(np.int64)]) if n else np.zeros((0, 7), np.int64)
    parts.append(" ".join(" ".join(map(str, r)) for r in rows.tolist()))
    return " ".join(p for p in parts if p)


@functools.lru_cache(maxsize=None)
def probe_exe():
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(tempfile.mkdtemp(prefix="gba_probe_"), "gba_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "gba_host_check.cpp"), "-o", exe])
    return exe


def probe(maps, prms):
    """The probe's outputs for the maps, as ref_map's dicts."""
    exe = probe_exe()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(case_line(m, p) for m, p in zip(maps, prms)) + "\n")
    try:
        got = subprocess.run([exe, f.name], check=True, capture_output=True, text=True).stdout.splitlines()
    finally:
        os.unlink(f.name)
    assert len(got) == len(maps)
    out = []
    for m, ln in zip(maps, got):
        t = ln.split()
        nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
        assert len(t) == 10 + 12 * nk + 3 * npt
        words = np.array([int(x, 16) for x in t[3:3 + 12 * nk + 3 * npt]], np.uint32).view(F32)
        out.append(dict(status=int(t[0]), ninliers=int(t[1]), cost=float(np.array(int(t[2], 16), np.uint64).view(F64)),
                        poses=words[:12 * nk].reshape(nk, 12), xw=words[12 * nk:].reshape(npt, 3),
                        inlier=np.array([c == "1" for c in t[-7]] if n else [], np.uint8), solves=int(t[-6]),
                        cg_total=int(t[-5]), fails=int(t[-4]), rejects=int(t[-3]), held=int(t[-2]),
                        cg=[] if t[-1] == "-" else [int(v) for v in t[-1].split(",")]))
    return out


def assert_same(got, want, tag):
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    assert got["ninliers"] == want["ninliers"], tag
    assert np.array(got["cost"], F64).view(np.uint64) == np.array(want["cost"], F64).view(np.uint64), tag
    for k in ("poses", "xw"):
        assert np.asarray(got[k], F32).view(np.uint32).tolist() == np.asarray(want[k], F32).view(np.uint32).tolist(), (tag, k)
    assert np.asarray(got["inlier"]).tolist() == np.asarray(want["inlier"]).tolist(), tag


# ---- CPU tests --------------------------------------------------------------------------------------------------------
def test_global_ba_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_global_ba_batch\s*\(", code) and re.search(r"\bint\s+pislam_global_ba_reserve\s*\(", code)
    m = re.search(r"typedef struct pislam_gba_params \{([^}]*)\} pislam_gba_params;", code)
    assert m and re.findall(r"(\w+)\s+(\w+)\s*;", m.group(1)) == [("pislam_ba_params", "ba"), ("int32_t", "cg_iters"), ("double", "cg_tol")]
    assert "64-PARTIAL SUM" in text and "Not here: a robust kernel, a several-workgroup form for one large graph." in text
    assert not re.search(r"Not here:[^/]*global bundle adjustment (and|afterwards)", text)
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_global_ba_batch"][1]) == 28 and len(capi.SYMBOLS["pislam_global_ba_reserve"][1]) == 5
    assert [f[0] for f in capi.GbaParams._fields_] == ["ba", "cg_iters", "cg_tol"] and ctypes.sizeof(capi.GbaParams) == 56
    assert ctypes.sizeof(capi.BaParams) == 40                # pislam_ba_params itself is unchanged
    for f in ("globalBundleAdjustBatch", "reserveGlobalBundleAdjust", "keyFrameObservationIndex"):
        assert callable(getattr(frontend, f))
    lib = capi.load()
    assert hasattr(lib, "pislam_global_ba_batch") and hasattr(lib, "pislam_global_ba_reserve")
    assert "gba_host_check.cpp" in open(os.path.join(ROOT, "tools", "probes", "README.md")).read()


def test_global_ba_probe_equals_the_restatement():
    cs = cases()
    got = probe([m for _, m, _ in cs], [p for _, _, p in cs])
    seen = {}
    for (name, m, prm), g in zip(cs, got):
        want = ref_map(m, prm)
        assert_same(g, want, name)
        assert g["cg"] == want["cg"], (name, g["cg"], want["cg"])
        assert (g["fails"], g["rejects"], g["held"]) == (want["fails"], want["rejects"], want["held"]), name
        assert g["solves"] == len(want["cg"]) and g["cg_total"] == sum(want["cg"]), name
        seen[name] = want
        if name.startswith("code_"):
            assert want["status"] & 255 == int(name[5]), name
    assert {w["status"] & 255 for w in seen.values()} == {0, 1, 2, 3}
    w = seen["smallest"]
    assert w["status"] & 255 == 0 and w["poses"].tobytes() != cs[0][1]["poses"].tobytes()
    assert seen["code_1_after_round_0"]["status"] >> 8 > 0
    w = seen["free_key_frame_unobserved"]                    # every solve fails: no step is ever taken
    m = next(c[1] for c in cs if c[0] == "free_key_frame_unobserved")
    assert w["fails"] == len(w["cg"]) > 0 and (w["poses"] == m["poses"]).all() and w["status"] & 255 in (0, 1)
    prm = next(c[2] for c in cs if c[0] == "stops_on_tolerance")
    assert all(0 < c < prm[5] for c in seen["stops_on_tolerance"]["cg"])
    assert all(c == 2 for c in seen["stops_at_cg_iters"]["cg"])
    assert seen["rejected_step"]["rejects"] > 0
    assert seen["point_of_outliers_held"]["held"] > 0 and seen["one_and_no_observation"]["held"] > 0
    for name in ("no_fixed_key_frame", "two_fixed_key_frames", "no_robust_round", "only_robust_rounds", "no_levels"):
        assert seen[name]["status"] & 255 == 0, name


def test_global_ba_holds_points_on_the_normal_path():
    """The map whose point 4 has only gross outliers: after round 0 the point has no active observation, is held and
    keeps the position round 0 gave it, while the rest of the map still moves."""
    name, m, prm = next(c for c in cases() if c[0] == "point_of_outliers_held")
    one = ref_map(m, (1, prm[1][:1]) + prm[2:])
    two = ref_map(m, prm)
    sel = m["pt"] == 4
    assert not one["inlier"][sel].any() and not two["inlier"][sel].any()
    assert two["xw"][4].tobytes() == one["xw"][4].tobytes()
    assert two["status"] & 255 == 0 and two["xw"].tobytes() != one["xw"].tobytes()


# ---- against a dense binary64 Levenberg without a Schur complement and without PCG ----------------------------------------
DENSE_PRM = (2, (10, 10), 1, 10, 1e-9, 200, 1e-8)
DENSE_SEEDS = list(range(8))


@functools.lru_cache(maxsize=None)
def dense_windows():
    """Well-posed maps of 20 to 40 key frames, two of them fixed, a few hundred stereo observations: past the local call's
    16 free key frames, and no gauge freedom is left to the damping."""
    return [tl.make_window(200 + s, nkf=20 + 20 * s // 7, nfree=18 + 20 * s // 7, npt=40, seen=0.22, noise=0.5, gross=0.05,
                           stereo=1.0, levels=False, min_seen=3) for s in DENSE_SEEDS]


def dense_lm(w, prm):
    """tests/test_local_ba.py's dense Levenberg (differenced Jacobian, robust weights held, numpy.linalg on the damped normal
    equations, the call's damping rule, schedule and classification), returning the state as well."""
    rounds, iters, hr, min_obs, eps = prm[:5]
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
            r0, F, _, live, _, k0 = tl.dense_residuals(w, T, X, active, robust)
            use = live & active
            J = np.zeros((len(r0), P))
            h = 1e-6
            for j in range(P):
                d = np.zeros(P)
                d[j] = h
                ra = tl.dense_residuals(w, *moved(T, X, d), use, robust, k0)[0]
                rb = tl.dense_residuals(w, *moved(T, X, -d), use, robust, k0)[0]
                J[:, j] = (ra - rb) / (2 * h)
            H, g = J.T @ J, J.T @ r0
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
            Tt, Xt = moved(T, X, d)
            Ft = tl.dense_residuals(w, Tt, Xt, active, robust)[1]
            if Ft < F:
                T, X, lam = Tt, Xt, max(lam * 0.25, tp.LAMBDA_MIN)
            else:
                lam = min(8.0 * lam, tp.LAMBDA_MAX)
            if np.abs(d).max() <= eps:
                break
        _, _, chi2, live, th, _ = tl.dense_residuals(w, T, X, active, False)
        active = live & (chi2 <= th)
    return active, float(chi2[active].sum()), T, X


# The relative deviation of the probe from the dense solver over the seeds 0 .. 7 of dense_windows(), with equal inlier
# masks, measured.  Final cost: 1.81e-6, 3.96e-6, 3.83e-6, 3.60e-5, 6.14e-6, 4.88e-6, 2.51e-6,
# 2.16e-6.  Output words (|probe - dense| over max(|dense|, 1), the largest over all pose and point words): 3.33e-3,
# 1.05e-6, 5.6e-6, 1.56e-4, 1.48e-6, 4.21e-5, 9.84e-7, 1.68e-5.  The bounds are 8 x the largest of each, the project's
# convention.  The cost differs by the binary32 evaluation of the residuals and by where 20 iterations of two different
# inner solvers stand; where the words differ most (seeds 0 and 3) the costs still agree to 1.81e-6 and 3.60e-5, so the
# difference lies along directions that the cost hardly fixes (not examined further).
MEASURED_DENSE_COST, MEASURED_DENSE_WORDS = 3.61e-5, 3.34e-3
DENSE_COST_RTOL, DENSE_WORDS_RTOL = 8 * MEASURED_DENSE_COST, 8 * MEASURED_DENSE_WORDS


@pytest.mark.parametrize("seed", DENSE_SEEDS)
def test_global_ba_against_a_dense_optimiser(seed):
    w = dense_windows()[seed]
    assert 20 <= len(w["poses"]) <= 40 and w["nfree"] > 16 and 150 <= len(w["kf"]) <= 500
    got = probe([from_window(w)], [DENSE_PRM])[0]
    active, cost, T, X = dense_lm(w, DENSE_PRM)
    rel = abs(got["cost"] - cost) / cost
    words = max(float(np.max(np.abs(got["poses"].astype(F64) - T) / np.maximum(np.abs(T), 1.0))),
                float(np.max(np.abs(got["xw"].astype(F64) - X) / np.maximum(np.abs(X), 1.0))))
    print("seed %d: nk %d n %d inliers %d cost %.6f dense %.6f rel %.3g words %.3g" % (
        seed, len(w["poses"]), len(w["kf"]), got["ninliers"], got["cost"], cost, rel, words))
    assert got["status"] & 255 == 0
    assert got["inlier"].astype(bool).tolist() == active.tolist()
    assert rel <= DENSE_COST_RTOL, (rel, DENSE_COST_RTOL)
    assert words <= DENSE_WORDS_RTOL, (words, DENSE_WORDS_RTOL)


# ---- against the local call on windows that both accept -------------------------------------------------------------------
LOCAL_PRM = (2, (5, 10), 1, 10, 1e-6)
# The largest relative deviation of the probe's final cost from ba_host_check's over tl.dense_windows() (seeds 0 .. 7), with
# equal inlier masks, cg_iters 200 and cg_tol 1e-10, measured: 0 (the same 64 bits) on seven of the eight and on the window
# of 16 free and 16 fixed key frames, 3.14e-6 on seed 6.  The bound is 8 x that.
MEASURED_LOCAL_COST = 3.14e-6
LOCAL_COST_RTOL = 8 * MEASURED_LOCAL_COST


def test_global_ba_against_the_local_call():
    ws = list(tl.dense_windows()) + [tl.make_window(300, nkf=32, nfree=16, npt=60, seen=0.3, min_seen=2)]
    local = tl.probe(ws, [LOCAL_PRM] * len(ws))
    glob = probe([from_window(w) for w in ws], [LOCAL_PRM + (200, 1e-10)] * len(ws))
    worst = 0.0
    for i, (a, b) in enumerate(zip(local, glob)):
        rel = abs(a["cost"] - b["cost"]) / a["cost"]
        print("window %d: local %.9f global %.9f rel %.3g" % (i, a["cost"], b["cost"], rel))
        assert a["status"] & 255 == 0 and b["status"] & 255 == 0
        assert a["inlier"].tolist() == b["inlier"].tolist(), i
        worst = max(worst, rel)
    assert worst <= LOCAL_COST_RTOL, (worst, LOCAL_COST_RTOL)


# ---- a seeded family of 64 small maps -------------------------------------------------------------------------------------
FAMILY = 64
HOSTILE = [0.0, -0.0, 1e-38, -1e-30, 1e30, -1e38, np.inf, -np.inf, np.nan, 1e-10, 3.4e38]
# The share of the family that ends with code 0, measured on the probe: 23 of 64 (code 1: 32, code 2: 2, code 3: 7; 8 maps
# hold points, 12 have failed solves, 5 rejected steps).  Half of it is the floor.
FAMILY_OK_MEASURED = 23


def family_map(i):
    rng = np.random.default_rng(9000 + i)
    nk = int(rng.choice([1, 2, 2, 3, 4, 6, 9, 17, 33]))
    nfree = int(rng.integers(0, nk + 1))
    npt = int(rng.choice([1, 2, 3, 5, 8, 13, 21, 64, 65]))
    w = tl.make_window(9100 + i, nkf=nk, nfree=nfree, npt=npt, seen=float(rng.choice([0.3, 0.6, 1.0])),
                       gross=float(rng.choice([0.0, 0.05, 0.5])), stereo=float(rng.choice([0.0, 0.5, 1.0])),
                       levels=bool(rng.integers(2)), start=float(rng.choice([0.0, 1.0, 5.0, 50.0])))
    fixed = np.zeros(nk, np.uint8)
    fixed[rng.permutation(nk)[:nk - nfree]] = 1
    m = from_window(w, fixed=fixed)
    n = len(m["kf"])
    kind = i % 8
    if kind == 1 and n:                                      # hostile numbers in the state
        for _ in range(int(rng.integers(1, 4))):
            a = m[str(rng.choice(["poses", "cams", "xw"]))]
            a.reshape(-1)[int(rng.integers(a.size))] = F32(rng.choice(HOSTILE))
    elif kind == 2 and n:                                    # hostile observations and levels
        m["obs"].reshape(-1)[rng.integers(0, 3 * n, 3)] = rng.choice([MONO, -(1 << 31), (1 << 31) - 1, 0, 1 << 22], 3).astype(np.int64).astype(np.int32)
        if "level" in m:
            m["level"][int(rng.integers(n))] = 255
    elif kind == 3 and n > 2:                                # a broken list or index
        how = int(rng.integers(5))
        if how == 0:
            m["pt"][int(rng.integers(n))] += int(rng.choice([-1, 1, 1000, -1000]))
        elif how == 1:
            m["kf"][int(rng.integers(n))] = nk
        elif how == 2:
            m["kf_obs"][int(rng.integers(n))] = int(rng.integers(0, n + 2))
        elif how == 3:
            m["kf_ptr"][int(rng.integers(nk + 1))] += 1
        else:
            m["count"], m["stride"] = int(rng.choice([-1, n + 5])), n + 4
            m = edit(m, poses=m["poses"][:0], cams=m["cams"][:0], fixed=m["fixed"][:0], kf=m["kf"][:0], pt=m["pt"][:0],
                     obs=m["obs"][:0], kf_obs=m["kf_obs"][:0], kf_ptr=np.zeros(1, np.uint32), kf_count=nk, kf_stride=nk,
                     **({"level": m["level"][:0]} if "level" in m else {}))
    elif kind == 4 and n:                                    # a free key frame loses its observations: every solve fails
        free = np.flatnonzero(m["fixed"] == 0)
        if len(free):
            m = keep_obs(m, m["kf"] != free[int(rng.integers(len(free)))])
    prm = (int(rng.integers(1, 4)),)
    prm = (prm[0], tuple(int(v) for v in rng.integers(1, 4, prm[0])), int(rng.integers(0, prm[0] + 1)),
           int(rng.choice([1, 3, 10, 60])), float(rng.choice([0.0, 1e-9, 1e-6, 1e-2])), int(rng.choice([1, 2, 5, 40])),
           float(rng.choice([0.0, 1e-8, 1e-3, 0.5])))
    return m, prm


def test_global_ba_family_of_small_maps():
    fam = [family_map(i) for i in range(FAMILY)]
    got = probe([m for m, _ in fam], [p for _, p in fam])
    codes = [g["status"] & 255 for g in got]
    ok = codes.count(0)
    print("codes", {c: codes.count(c) for c in sorted(set(codes))}, "held", sum(g["held"] > 0 for g in got), "failed",
          sum(g["fails"] > 0 for g in got), "rejected", sum(g["rejects"] > 0 for g in got))
    assert set(codes) == {0, 1, 2, 3}
    assert any(g["held"] > 0 for g in got) and any(g["fails"] > 0 for g in got) and any(g["rejects"] > 0 for g in got)
    at_max = any(c == p[5] for g, (_, p) in zip(got, fam) for c in g["cg"])
    on_tol = any(0 < c < p[5] for g, (_, p) in zip(got, fam) for c in g["cg"])
    assert at_max and on_tol
    for g, (m, _) in zip(got, fam):                          # a refused map comes back as it went in
        if g["status"] in (2, 3) or (g["status"] == 1):
            assert g["poses"].tobytes() == m["poses"].tobytes() and g["xw"].tobytes() == m["xw"].tobytes() and not g["inlier"].any()
    assert ok >= FAMILY_OK_MEASURED / 2, (ok, FAMILY_OK_MEASURED)


@pytest.mark.parametrize("i", [1, 9, 2, 4, 12, 5])
def test_global_ba_family_members_equal_the_restatement(i):
    m, prm = family_map(i)
    g = probe([m], [prm])[0]
    want = ref_map(m, prm)
    assert_same(g, want, "family %d" % i)
    assert g["cg"] == want["cg"]


# ---- GPU tests --------------------------------------------------------------------------------------------------------
NAMES = ("poses_out", "xw_out", "inlier", "ninliers", "cost", "status", "work")


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
                    cost=f(B, 2).view(t.float64).reshape(B), status=f(B), work=f(B, 2))

    def pack(self, maps, kfs, pts, stride, pt_counts=None):
        """Host arrays of a batch: the slots at and beyond a map's counts hold rubbish that must not be read."""
        B = len(maps)
        rng = np.random.default_rng(7)
        h = dict(poses=rng.normal(0, 1e30, (B, kfs, 12)).astype(F32), cams=rng.normal(0, 1e30, (B, kfs, 5)).astype(F32),
                 xw=rng.normal(0, 1e30, (B, pts, 3)).astype(F32), fixed=rng.integers(0, 2, (B, kfs)).astype(np.uint8),
                 obs=rng.integers(-1 << 31, 1 << 31, (B, stride, 3)).astype(np.int32),
                 kf=rng.integers(0, 1 << 16, (B, stride)).astype(np.uint16), pt=rng.integers(-1 << 31, 1 << 31, (B, stride)).astype(np.int32),
                 level=rng.integers(0, 256, (B, stride)).astype(np.uint8), kf_ptr=rng.integers(0, 1 << 32, (B, kfs + 1)).astype(np.uint32),
                 kf_obs=rng.integers(0, 1 << 32, (B, stride)).astype(np.uint32), kf_counts=np.zeros(B, np.int32),
                 pt_counts=np.zeros(B, np.uint32), counts=np.zeros(B, np.int32), tab=None)
        for b, m in enumerate(maps):
            nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
            h["poses"][b, :nk], h["cams"][b, :nk], h["xw"][b, :npt], h["fixed"][b, :nk] = m["poses"], m["cams"], m["xw"], m["fixed"]
            h["obs"][b, :n], h["kf"][b, :n], h["pt"][b, :n], h["kf_obs"][b, :n] = m["obs"], m["kf"], m["pt"], m["kf_obs"]
            h["kf_ptr"][b, :nk + 1] = m["kf_ptr"]
            if m.get("tab") is not None:
                h["level"][b, :n], h["tab"] = m["level"], m["tab"]
            count, kf_count, _, _ = counts_of(m)
            h["counts"][b], h["kf_counts"][b] = count, kf_count
            h["pt_counts"][b] = npt if pt_counts is None or pt_counts[b] is None else pt_counts[b]
        h["pt_counts"] = h["pt_counts"].view(np.int32)
        h["kf"], h["kf_ptr"], h["kf_obs"] = h["kf"].view(np.int16), h["kf_ptr"].view(np.int32), h["kf_obs"].view(np.int32)
        return h

    def upload(self, h):
        return {k: (self.up(v) if k != "tab" and v is not None else v) for k, v in h.items()}

    def call(self, prm, d, shape, B, o, with_level=True):
        ptr = self.capi.ptr
        kfs, pts, stride = shape
        p = None
        if prm is not None:
            its = list(prm[1]) + [1] * (4 - len(prm[1]))
            p = self.capi.GbaParams(self.capi.BaParams(prm[0], (ctypes.c_int32 * 4)(*its), prm[2], prm[3], prm[4]), prm[5], prm[6])
        tab = d.get("tab") if with_level else None
        ctab = None if tab is None else (ctypes.c_float * len(tab))(*[float(v) for v in tab])
        return self.lib.pislam_global_ba_batch(
            self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["poses"]), ptr(d["cams"]), ptr(d["fixed"]),
            ptr(d["kf_counts"]), ptr(d["xw"]), ptr(d["pt_counts"]), ptr(d["obs"]), ptr(d["kf"]), ptr(d["pt"]),
            ptr(d["level"]) if tab is not None else None, ptr(d["counts"]), ptr(d["kf_ptr"]), ptr(d["kf_obs"]), ctab,
            0 if tab is None else len(tab), kfs, pts, stride, B, ptr(o["poses_out"]), ptr(o["xw_out"]), ptr(o["inlier"]),
            ptr(o["ninliers"]), ptr(o["cost"]), ptr(o["status"]), ptr(o["work"]))

    def run(self, maps, prm, shape, pt_counts=None):
        h = self.pack(maps, *shape, pt_counts=pt_counts)
        d = self.upload(h)
        o = self.sentinels(len(maps), *shape)
        assert self.call(prm, d, shape, len(maps), o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_maps(got, want, maps, what=""):
    """Every output word of every map, the PCG iteration counts, and the sentinels at and beyond the counts."""
    sent = np.array([0x5A5A5A5A], np.uint32)
    for b, (x, m) in enumerate(zip(want, maps)):
        nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
        g = dict(status=int(got["status"][b]), ninliers=int(got["ninliers"][b]), cost=float(got["cost"][b]),
                 poses=got["poses_out"][b, :nk], xw=got["xw_out"][b, :npt], inlier=got["inlier"][b, :n])
        assert_same(g, x, "%s map %d" % (what, b))
        assert got["work"][b].tolist() == [len(x["cg"]), sum(x["cg"])], (what, b)
        assert (got["inlier"][b, n:] == SENT8).all(), (what, b)
        assert (got["poses_out"][b, nk:].view(np.uint32) == sent).all() and (got["xw_out"][b, npt:].view(np.uint32) == sent).all()


def shape_of(maps, pad=(0, 0, 0)):
    return (max(max(counts_of(m)[3] for m in maps) + pad[0], 1), max(max(len(m["xw"]) for m in maps) + pad[1], 1),
            max(max(counts_of(m)[2] for m in maps) + pad[2], 1))


def fit(m, shape):
    """A map whose counts are out of range, against the strides of the batch it runs in."""
    if "count" not in m:
        return m
    count, kf_count, stride, kf_stride = counts_of(m)
    return edit(m, count=shape[2] + 1 if count > stride else count, kf_count=shape[0] + 1 if kf_count > kf_stride else kf_count,
                stride=shape[2], kf_stride=shape[0])


@pytest.mark.gpu
def test_global_ba_smallest_map(gpu_ctx):
    m = smallest()
    assert len(m["kf"]) == 6 and m["fixed"].tolist() == [0, 1]
    want = ref_map(m, SMALL_PRM)
    assert want["status"] & 255 == 0 and want["poses"].tobytes() != m["poses"].tobytes()
    got = Device(gpu_ctx).run([m], SMALL_PRM, (2, 3, 6))
    assert_maps(got, [want], [m], "smallest")


@pytest.mark.gpu
def test_global_ba_every_case_in_batches_with_unequal_counts(gpu_ctx):
    """The maps of the CPU test, one batch per parameter set with padded strides, next to a map whose pt_counts is
    PISLAM_COUNT_INVALID."""
    groups = {}
    for name, m, prm in cases():
        groups.setdefault(prm, []).append(m)
    for prm, ms in groups.items():
        with_tab = [m for m in ms if m.get("tab") is not None]
        for batch in (with_tab, [m for m in ms if m.get("tab") is None]):
            if not batch:
                continue
            shape = shape_of(batch, (1, 2, 3))
            batch = [fit(m, shape) for m in batch]
            pc = [None] * len(batch)
            if len(batch) > 3:                               # pt_counts INVALID: no point exists
                full = max(batch, key=lambda m: len(m["kf"]))
                batch = batch + [edit(full, xw=full["xw"][:0])]
                pc = pc + [COUNT_INVALID]
            want = probe(batch, [prm] * len(batch))
            got = Device(gpu_ctx).run(batch, prm, shape, pc)
            assert_maps(got, want, batch, "%r" % (prm,))


BOUNDARY_PRM = (2, (2, 2), 1, 10, 1e-6, 6, 1e-6)


def big_map(seed, nk, npt, per_point=3, fixed=(0,), kfs=None):
    """A map of nk key frames on a line looking along z at npt points, each seen by per_point key frames near it (or by
    those of `kfs`), stereo, half a pixel of noise."""
    rng = np.random.default_rng(seed)
    xw = np.stack([rng.uniform(-2, 2, npt) , rng.uniform(-1.5, 1.5, npt), rng.uniform(4, 8, npt)], 1)
    span = 3.0
    cx = np.linspace(-span / 2, span / 2, nk) if nk > 1 else np.zeros(1)
    xw[:, 0] += np.linspace(-span / 2, span / 2, npt)
    poses = np.zeros((nk, 12))
    poses[:, 0] = poses[:, 4] = poses[:, 8] = 1.0
    poses[:, 9] = -cx
    cams = np.tile(tl.CAM, (nk, 1)).astype(F32)
    kf, pt, obs = [], [], []
    for p in range(npt):
        if kfs is not None:
            ks = sorted(kfs(p))
        else:
            c = int(round(p / max(npt - 1, 1) * (nk - 1)))
            ks = sorted({min(max(c + d, 0), nk - 1) for d in range(-(per_point // 2), per_point - per_point // 2)})
        for k in ks:
            xc = xw[p] + poses[k, 9:]
            u = tl.CAM[0] * xc[0] / xc[2] + tl.CAM[2] + rng.normal(0, 0.5)
            v = tl.CAM[1] * xc[1] / xc[2] + tl.CAM[3] + rng.normal(0, 0.5)
            ur = u - tl.CAM[4] / xc[2] + rng.normal(0, 0.5)
            kf.append(k), pt.append(p), obs.append([int(round(256 * u)), int(round(256 * v)), int(round(256 * ur))])
    start = poses.copy()
    fx = np.zeros(nk, np.uint8)
    fx[list(fixed)] = 1
    start[fx == 0, 9:] += rng.normal(0, 0.005, (int((fx == 0).sum()), 3))
    m = dict(poses=start.astype(F32), cams=cams, xw=(xw + rng.normal(0, 0.01, xw.shape)).astype(F32), fixed=fx,
             kf=np.array(kf, np.uint16), pt=np.array(pt, np.int32), obs=np.array(obs, np.int64).reshape(-1, 3).astype(np.int32))
    return reindex(m)


def cut(m, n):
    return keep_obs(m, np.arange(len(m["kf"])) < n)


@functools.lru_cache(maxsize=None)
def boundary_maps():
    """255, 256 and 257 points; 257 and 513 observations; a key frame with 63, 64, 65 and 129 entries; 17 and 33 free key
    frames; 257 and 1025 key frames."""
    ms = [big_map(21, 18, 255), big_map(22, 34, 256), big_map(23, 6, 257), cut(big_map(24, 5, 100), 257), cut(big_map(25, 8, 200), 513)]
    for e in (63, 64, 65, 129):                              # key frame 1 sees the first e points, key frames 0 and 2 all
        ms.append(big_map(30 + e, 3, 140, kfs=lambda p, e=e: [0, 2] + ([1] if p < e else [])))
    ms += [big_map(41, 257, 300), big_map(42, 1025, 1100, per_point=2)]
    return ms


@pytest.mark.gpu
def test_global_ba_thread_wave_and_partial_boundaries(gpu_ctx):
    ms = boundary_maps()
    assert [len(m["xw"]) for m in ms[:3]] == [255, 256, 257] and [len(m["kf"]) for m in ms[3:5]] == [257, 513]
    assert [int(m["kf_ptr"][2] - m["kf_ptr"][1]) for m in ms[5:9]] == [63, 64, 65, 129]
    assert [int((m["fixed"] == 0).sum()) for m in ms[:2]] == [17, 33] and [len(m["poses"]) for m in ms[9:]] == [257, 1025]
    want = probe(ms, [BOUNDARY_PRM] * len(ms))
    assert all(x["status"] & 255 == 0 and x["cg_total"] > 0 for x in want)
    d = Device(gpu_ctx)
    for group in (ms[:9], ms[9:]):
        got = d.run(group, BOUNDARY_PRM, shape_of(group))
        assert_maps(got, want[:len(group)], group, "boundaries")
        want = want[len(group):]


@pytest.mark.gpu
def test_global_ba_last_key_frame_and_large_point_index(gpu_ctx):
    """A key frame of index 4095 with kf_stride 4096 and few observations; a point index above 65535."""
    far = big_map(51, 4, 30)
    far = edit(far, kf=np.where(far["kf"] == 3, 4095, far["kf"]).astype(np.uint16))
    for k in ("poses", "cams"):
        a = np.zeros((4096,) + far[k].shape[1:], F32)
        a[:] = far[k][0]
        a[[0, 1, 2, 4095]] = far[k]
        far[k] = a
    far["fixed"] = np.ones(4096, np.uint8)
    far["fixed"][[1, 2, 4095]] = 0
    far = reindex(far)
    wide = big_map(52, 4, 30)
    wide = edit(wide, pt=(wide["pt"] + 65536 + 70).astype(np.int32))
    xw = np.zeros((65536 + 100, 3), F32)
    xw[:, 2] = 5.0
    xw[65536 + 70:] = wide["xw"]
    wide["xw"] = xw
    prm = (1, (2,), 1, 10, 1e-6, 5, 1e-6)
    d = Device(gpu_ctx)
    for m, tag in ((far, "key frame 4095"), (wide, "point above 65535")):
        want = probe([m], [prm])
        assert want[0]["status"] & 255 == 0 and want[0]["poses"].tobytes() != m["poses"].tobytes()
        got = d.run([m], prm, shape_of([m]))
        assert_maps(got, want, [m], tag)


@pytest.mark.gpu
def test_global_ba_in_place_refusals_and_replay(gpu_ctx):
    d = Device(gpu_ctx)
    t = d.torch
    ms = [c[1] for c in cases() if c[0] in ("mixed_mono_stereo_levels", "dead_level")]
    shape = shape_of(ms, (1, 3, 5))
    kfs, pts, stride = shape
    B = len(ms)
    h = d.pack(ms, *shape)
    dev = d.upload(h)
    o = d.sentinels(B, *shape)
    good = DEFAULT
    bad_prms = [(0,) + good[1:], (5,) + good[1:], (2, (4, 0)) + good[2:], (2, (33, 5)) + good[2:], good[:2] + (-1,) + good[3:],
                good[:2] + (3,) + good[3:], good[:3] + (0,) + good[4:], good[:3] + ((1 << 24) + 1,) + good[4:],
                good[:4] + (-1e-9,) + good[5:], good[:4] + (float("nan"),) + good[5:], good[:5] + (0, 1e-6), good[:5] + (257, 1e-6),
                good[:6] + (1.0,), good[:6] + (-1e-3,), good[:6] + (float("nan"),), None]
    for prm in bad_prms:
        assert d.call(prm, dev, shape, B, o) == -1, prm
    for bad in ((0, pts, stride), (MAX_KF + 1, pts, stride), (kfs, 0, stride), (kfs, MAX_PTS + 1, stride), (kfs, pts, 0),
                (kfs, pts, MAX_STRIDE + 1)):
        assert d.call(good, dev, bad, B, o) == -1, bad
        assert d.lib.pislam_global_ba_reserve(gpu_ctx.h, bad[0], bad[1], bad[2], B) == -1, bad
    assert d.call(good, dev, shape, -1, o) == -1
    assert d.call(good, dict(dev, tab=[1.0] * 17), shape, B, o) == -1
    host = np.zeros(B * stride * 3 + B * kfs * 12 + B * pts * 3, np.int32)
    for name in ("poses", "cams", "fixed", "kf_counts", "xw", "pt_counts", "obs", "kf", "pt", "level", "counts", "kf_ptr",
                 "kf_obs") + NAMES:
        for repl in (None, host):                             # NULL, then a host pointer
            if name in ("level", "work") and repl is None:
                continue
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, shape, B, outs) == -1, name
    assert d.call(good, dev, shape, B, dict(o, ninliers=dev["counts"])) == -1
    assert d.call(good, dev, shape, B, dict(o, inlier=dev["fixed"])) == -1
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["xw"])) == -1
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["poses"].view(-1)[4:])) == -1
    assert d.call(good, dev, shape, B, dict(o, status=o["ninliers"])) == -1
    assert d.call(good, dev, shape, B, dict(o, work=o["status"])) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        a = v.cpu().numpy()
        assert (a == SENT8).all() if k == "inlier" else (a.view(np.uint8) == 0x5A).all(), k
    # batch 0 is a no-op after the checks: the pointers are not looked at
    p = d.capi.GbaParams(d.capi.BaParams(2, (ctypes.c_int32 * 4)(5, 10, 1, 1), 1, 10, 1e-6), 10, 1e-6)
    assert d.lib.pislam_global_ba_batch(gpu_ctx.h, ctypes.byref(p), *([None] * 14), 0, kfs, pts, stride, 0, *([None] * 7)) == 0
    assert d.lib.pislam_global_ba_reserve(gpu_ctx.h, kfs, pts, stride, 0) == 0
    # the frontend, twice (the same bits), then captured on a side stream after a reserve on a fresh context
    from pislam_amd.capi import Context
    from pislam_amd.frontend import globalBundleAdjustBatch, reserveGlobalBundleAdjust
    want = probe(ms, [good] * B)
    args = (dev["poses"], dev["cams"], dev["fixed"], dev["kf_counts"], dev["xw"], dev["pt_counts"], dev["obs"], dev["kf"],
            dev["pt"], dev["counts"], dev["kf_ptr"], dev["kf_obs"])
    kw = dict(level=dev["level"], inv_sigma2=h["tab"], rounds=good[0], iters=good[1], huber_rounds=good[2], min_obs=good[3],
              eps=good[4], cg_iters=good[5], cg_tol=good[6])
    first = [x.cpu().numpy().copy() for x in globalBundleAdjustBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(B, *shape))]
    again = [x.cpu().numpy().copy() for x in globalBundleAdjustBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(B, *shape))]
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert_maps(dict(zip(NAMES, first)), want, ms, "frontend")
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveGlobalBundleAdjust(*shape, B, ctx=ctx)
        oc = d.sentinels(B, *shape)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            globalBundleAdjustBatch(*args, ctx=ctx, **kw, **oc)
        for _ in range(2):
            for k, x in oc.items():
                x.view(t.uint8).fill_(SENT8 if k == "inlier" else 0x5A)
            g.replay()
            side.synchronize()
            for a, b in zip(first, oc.values()):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        ctx.close()
    # poses_out may be poses and xw_out may be xw; nothing is written at or beyond the counts
    assert d.call(good, dev, shape, B, dict(o, poses_out=dev["poses"], xw_out=dev["xw"])) == 0
    gpu_ctx.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["poses_out"], got["xw_out"] = dev["poses"].cpu().numpy(), dev["xw"].cpu().numpy()
    for b, m in enumerate(ms):
        nk, npt = len(m["poses"]), len(m["xw"])
        assert got["poses_out"][b, nk:].tobytes() == h["poses"][b, nk:].tobytes()
        assert got["xw_out"][b, npt:].tobytes() == h["xw"][b, npt:].tobytes()
        got["poses_out"][b, nk:].view(np.uint32)[...] = 0x5A5A5A5A
        got["xw_out"][b, npt:].view(np.uint32)[...] = 0x5A5A5A5A
    assert_maps(got, want, ms, "in place")


@pytest.mark.gpu
def test_global_ba_chain_on_one_observation_list(gpu_ctx):
    """mapObservations -> keyFrameObservationIndex -> globalBundleAdjustBatch -> mapPointsUpdateBatch on one list, given
    in any order and padded."""
    import torch as t
    from pislam_amd.frontend import globalBundleAdjustBatch, keyFrameObservationIndex, mapObservations, mapPointsUpdateBatch
    d = Device(gpu_ctx)
    m = big_map(61, 6, 40)
    nk, npt, n = len(m["poses"]), len(m["xw"]), len(m["kf"])
    stride = n + 7
    perm = np.random.default_rng(62).permutation(n)
    pad = lambda a, fill: np.concatenate([a[perm], np.full((stride - n,) + a.shape[1:], fill, a.dtype)])[None]
    okf, opt, cnt, obs, lvl = mapObservations(d.up(pad(m["kf"].astype(np.int16), 77)), d.up(pad(m["pt"], 5)),
                                              d.up(np.array([n], np.int32)), d.up(pad(m["obs"], 9)), d.up(pad(np.zeros(n, np.uint8), 3)))
    kf_ptr, kf_obs = keyFrameObservationIndex(okf, cnt, nk)
    assert okf[0, :n].cpu().numpy().astype(np.uint16).tolist() == m["kf"].tolist() and opt[0, :n].cpu().numpy().tolist() == m["pt"].tolist()
    assert kf_ptr[0].cpu().numpy().tolist() == m["kf_ptr"].tolist() and kf_obs[0, :n].cpu().numpy().tolist() == m["kf_obs"].tolist()
    one = lambda v: d.up(np.array([v], np.int32))
    prm = (1, (3,), 1, 10, 1e-6, 8, 1e-6)
    poses, cams, fixed, xw = (d.up(m[k][None]) for k in ("poses", "cams", "fixed", "xw"))
    out = globalBundleAdjustBatch(poses, cams, fixed, one(nk), xw, one(npt), obs, okf, opt, cnt, kf_ptr, kf_obs, rounds=prm[0],
                                  iters=prm[1], huber_rounds=prm[2], min_obs=prm[3], eps=prm[4], cg_iters=prm[5], cg_tol=prm[6],
                                  ctx=gpu_ctx)
    gpu_ctx.synchronize()
    want = probe([m], [prm])[0]
    g = dict(status=int(out[5][0]), ninliers=int(out[3][0]), cost=float(out[4][0]), poses=out[0][0].cpu().numpy(),
             xw=out[1][0].cpu().numpy(), inlier=out[2][0, :n].cpu().numpy())
    assert_same(g, want, "chain")
    assert want["status"] & 255 == 0 and out[6][0].cpu().numpy().tolist() == [want["solves"], want["cg_total"]]
    upd = mapPointsUpdateBatch(okf, opt, cnt, one(nk), lvl, out[0], out[1], one(npt), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    normal, drange, _, nobs, first, pt_status, status = upd
    assert int(status[0]) == 0 and (pt_status[0].cpu().numpy() == 0).all()
    assert nobs[0].cpu().numpy().tolist() == np.bincount(m["pt"], minlength=npt).tolist()
    nrm = normal[0].cpu().numpy().astype(F64)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
