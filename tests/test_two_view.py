"""Batched two-view RANSAC: fundamental matrix and homography (pislam_two_view_ransac_batch).

The expectation is a plain-Python restatement of the contract in include/pislam_hip.h, written from that comment and
independent of the library.  Everything integral is a Python integer.  Every binary32 operation of the contract is ONE
numpy float32 operation: numpy.float32 scalars in the sampler and the solver, float32 arrays over the matches of a pair
in the scoring (an elementwise float32 array operation rounds each element exactly as the scalar operation does).
Integers become floats through exact Python integers below 2^53 (numpy.float32(int) goes through a double, which holds
them exactly, and rounds once).  The GPU must agree with it on every output word.
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F32 = np.float32
SENT32 = 0x5A5A5A5A                   # fills outputs before a call: entries the call must not write keep it
SENT8 = 0x5A
COUNT_INVALID = 0xFFFFFFFF
COORD_MAX = 1 << 20
MAX_STRIDE = 16384
FUND, HOMOG = 0, 1
SAMPLE = {FUND: 8, HOMOG: 4}
PIVOT_MIN = F32(2.0 ** -20)
TH_SCORE = F32(5.991)
TH = {FUND: F32(3.841), HOMOG: F32(5.991)}
M32 = 0xFFFFFFFF
TV_FIELDS = ["model", "hypotheses", "seed", "sigma_q8"]


# ---- the expectation ------------------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def tv_hash(seed, b, k, j):
    h = mix32((seed & M32) + 0x9E3779B9 * (b & M32))
    h = mix32(h ^ ((0x85EBCA6B * (k + 1)) & M32))
    return mix32(h ^ ((0xC2B2AE35 * (j + 1)) & M32))


def ref_sample(seed, b, k, n, m):
    """The m distinct match indices of hypothesis k, in draw order."""
    drawn = []
    for j in range(m):
        r = (tv_hash(seed, b, k, j) * (n - j)) >> 32
        for c in sorted(drawn):
            if r >= c:
                r += 1
        drawn.append(r)
    return drawn


def ref_stats(p1, p2):
    """(n, Sx1, Sy1, D1, Sx2, Sy2, D2, 0) and the clamped integer coordinates [n][4] = x1, y1, x2, y2."""
    pts = [[max(-COORD_MAX, min(COORD_MAX, int(v))) for v in (*a, *b)] for a, b in zip(p1, p2)]
    n = len(pts)
    S = [sum(p[c] for p in pts) for c in range(4)]
    D1 = sum(abs(n * p[0] - S[0]) + abs(n * p[1] - S[1]) for p in pts)
    D2 = sum(abs(n * p[2] - S[2]) + abs(n * p[3] - S[3]) for p in pts)
    assert D1 < 1 << 53 and D2 < 1 << 53
    return (n, S[0], S[1], D1, S[2], S[3], D2, 0), pts


def ref_normalise(stats, pts, sigma_q8):
    """Normalised coordinates as four float32 arrays [n], and the chi-square weights (w1, w2)."""
    n, Sx1, Sy1, D1, Sx2, Sy2, D2, _ = stats
    k1 = F32(2 * n * n) / F32(D1)
    k2 = F32(2 * n * n) / F32(D2)
    conv = lambda c, S: np.array([F32(n * p[c] - S) for p in pts], dtype=F32)
    x1, y1, x2, y2 = conv(0, Sx1) * k1, conv(1, Sy1) * k1, conv(2, Sx2) * k2, conv(3, Sy2) * k2
    sg = F32(sigma_q8) / F32(256.0)
    w = []
    for k in (k1, k2):
        s = (F32(256.0) * F32(n)) * k
        t = s * sg
        w.append(F32(1.0) / (t * t))
    return (x1, y1, x2, y2), w[0], w[1]


def ref_rows(model, X, idx):
    """The 8 x 9 system [A | b] of one hypothesis as a list of rows of float32 scalars."""
    x1, y1, x2, y2 = X
    Z, ONE = F32(0.0), F32(1.0)
    rows = []
    for i in idx:
        a, b, c, d = x1[i], y1[i], x2[i], y2[i]
        if model == FUND:
            rows.append([c * a, c * b, c, d * a, d * b, d, a, b, F32(-1.0)])
        else:
            rows.append([a, b, ONE, Z, Z, Z, -(c * a), -(c * b), c])
            rows.append([Z, Z, Z, a, b, ONE, -(d * a), -(d * b), d])
    return rows


def ref_solve(A):
    """Gaussian elimination with partial pivoting and back substitution: the 8 unknowns, or None when invalid."""
    A = [list(r) for r in A]
    for c in range(8):
        for r in range(c + 1, 8):                      # row c ends as the first row of largest magnitude
            if abs(A[r][c]) > abs(A[c][c]):
                A[c], A[r] = A[r], A[c]
        if not abs(A[c][c]) >= PIVOT_MIN:
            return None
        inv = F32(1.0) / A[c][c]
        for r in range(c + 1, 8):
            f = A[r][c] * inv
            for j in range(c + 1, 9):
                A[r][j] = A[r][j] - f * A[c][j]
    x = [None] * 8
    for r in range(7, -1, -1):
        s = A[r][8]
        for j in range(r + 1, 8):
            s = s - A[r][j] * x[j]
        x[r] = s / A[r][r]
    if not all(np.isfinite(v) for v in x):
        return None
    return x


def ref_chi(model, f, X, w1, w2):
    """(chi2 of the distance measured in image 2, chi2 of the distance measured in image 1): float32 arrays [n]."""
    x1, y1, x2, y2 = X
    f = list(f) + [F32(1.0)]
    if model == FUND:
        def direction(m, xa, ya, xb, yb, w):          # the line m * (xa, ya, 1), the distance of (xb, yb) to it
            a = (m[0] * xa + m[1] * ya) + m[2]
            b = (m[3] * xa + m[4] * ya) + m[5]
            c = (m[6] * xa + m[7] * ya) + m[8]
            num = (a * xb + b * yb) + c
            return ((num * num) / (a * a + b * b)) * w
        ft = [f[0], f[3], f[6], f[1], f[4], f[7], f[2], f[5], f[8]]
        return direction(f, x1, y1, x2, y2, w2), direction(ft, x2, y2, x1, y1, w1)

    def transfer(m, xa, ya, xb, yb, w):
        inv = F32(1.0) / ((m[6] * xa + m[7] * ya) + m[8])
        u = ((m[0] * xa + m[1] * ya) + m[2]) * inv
        v = ((m[3] * xa + m[4] * ya) + m[5]) * inv
        du, dv = xb - u, yb - v
        return (du * du + dv * dv) * w
    h = f
    g = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
         h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
         h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    return transfer(h, x1, y1, x2, y2, w2), transfer(g, x2, y2, x1, y1, w1)


def ref_score(model, f, X, w1, w2):
    """(score, inlier mask) of one model."""
    ca, cb = ref_chi(model, f, X, w1, w2)
    score, ok = 0, []
    for chi in (ca, cb):
        good = chi < TH[model]                         # false for a NaN
        pts = np.floor((TH_SCORE - chi) * F32(256.0))
        score += int(sum(int(v) for v in pts[good]))
        ok.append(good)
    return score, ok[0] & ok[1]


def ref_pair(p1, p2, b, model, hypotheses, seed, sigma_q8):
    """One pair: dict(best, score, ninliers, inlier uint8 [n], model_n float32 [9], stats [8])."""
    m = SAMPLE[model]
    stats, pts = ref_stats(p1, p2)
    n = stats[0]
    none = dict(best=-1, score=0, ninliers=0, inlier=np.zeros(n, np.uint8), model_n=np.zeros(9, F32), stats=stats)
    if n < m or stats[3] == 0 or stats[6] == 0:
        return none
    with np.errstate(all="ignore"):
        X, w1, w2 = ref_normalise(stats, pts, sigma_q8)
        best = (0, -1, None, None)
        for k in range(hypotheses):
            f = ref_solve(ref_rows(model, X, ref_sample(seed, b, k, n, m)))
            if f is None:
                continue
            score, inl = ref_score(model, f, X, w1, w2)
            if score > best[0]:
                best = (score, k, f, inl)
    if best[1] < 0:
        return none
    score, k, f, inl = best
    return dict(best=k, score=score, ninliers=int(inl.sum()), inlier=inl.astype(np.uint8),
                model_n=np.array(list(f) + [F32(1.0)], dtype=F32), stats=stats)


def ref_batch(p1, p2, counts, model, hypotheses, seed, sigma_q8, sent=True):
    """The call on int arrays [batch][stride][2] and counts [batch], outputs pre-filled with the sentinel."""
    B, stride = p1.shape[:2]
    out = dict(best=np.full(B, SENT32, np.int32), score=np.full(B, SENT32, np.uint32), ninliers=np.full(B, SENT32, np.uint32),
               inlier=np.full((B, stride), SENT8, np.uint8), model_n=np.full((B, 9), SENT32, np.uint32).view(F32),
               stats=np.full((B, 8), SENT32, np.int64))
    for b in range(B):
        n = 0 if int(counts[b]) == COUNT_INVALID else min(int(counts[b]), stride)
        r = ref_pair(p1[b, :n].tolist(), p2[b, :n].tolist(), b, model, hypotheses, seed, sigma_q8)
        out["best"][b], out["score"][b], out["ninliers"][b] = r["best"], r["score"], r["ninliers"]
        out["inlier"][b, :n], out["model_n"][b], out["stats"][b] = r["inlier"], r["model_n"], r["stats"]
    return out


def ref_denormalise(model, model_n, stats):
    """The level-0-pixel matrix in float64: F = T2^T Fn T1, H = T2^-1 Hn T1."""
    n, Sx1, Sy1, D1, Sx2, Sy2, D2, _ = (int(v) for v in stats)
    T = []
    for Sx, Sy, D in ((Sx1, Sy1, D1), (Sx2, Sy2, D2)):
        k = 2.0 * n * n / D
        T.append(np.array([[256.0 * n * k, 0, -Sx * k], [0, 256.0 * n * k, -Sy * k], [0, 0, 1.0]]))
    Mn = np.asarray(model_n, dtype=np.float64).reshape(3, 3)
    return T[1].T @ Mn @ T[0] if model == FUND else np.linalg.inv(T[1]) @ Mn @ T[0]


# ---- synthetic scenes -------------------------------------------------------------------------------------------------
def scene(seed, plane, n=300, outliers=0.2, noise=0.5):
    """n matches of a 640 x 480 camera pair, focal length 500, a small rotation plus a translation: Q8 level-0 points of
    both images [n][2] and the mask of the true inliers.  Depth 4..12 (general) or a tilted plane; Gaussian noise on
    both images; a share of the second image's points replaced by uniform random positions."""
    rng = np.random.default_rng(seed)
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    u = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    rays = np.linalg.inv(K) @ np.vstack([u.T, np.ones(n)])
    if plane:
        nrm, d = np.array([0.15, -0.1, 1.0]), 8.0
        z = d / (nrm @ rays)
    else:
        z = rng.uniform(4, 12, n)
    P = rays * z
    rx, ry, rz = 0.02, -0.03, 0.015
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    Q = K @ ((Rz @ Ry @ Rx) @ P + np.array([[0.5], [0.1], [0.05]]))
    v = (Q[:2] / Q[2]).T
    u = u + rng.normal(0, noise, u.shape)
    v = v + rng.normal(0, noise, v.shape)
    bad = rng.permutation(n)[:int(round(outliers * n))]
    v[bad] = np.stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))], 1)
    good = np.ones(n, bool)
    good[bad] = False
    return np.rint(u * 256).astype(np.int64), np.rint(v * 256).astype(np.int64), good


def collinear(n, seed):
    """n matches on a horizontal line in both images: after centring every y is exactly 0, so a whole column of every
    system is 0 and every hypothesis is invalid whatever the rounding."""
    rng = np.random.default_rng(seed)
    u = np.stack([rng.integers(0, 640 * 256, n), np.full(n, 100 * 256)], 1)
    v = np.stack([rng.integers(0, 640 * 256, n), np.full(n, 77 * 256 + 13)], 1)
    return u, v


# ---- CPU: declarations, the expectation's anchors, behaviour ------------------------------------------------------
def test_two_view_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in ("pislam_two_view_ransac_batch", "pislam_two_view_denormalise"):
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f + " is not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_two_view_params \{([^}]*)\} pislam_two_view_params;", code)
    assert m and re.findall(r"u?int32_t\s+(\w+)\s*;", m.group(1)) == TV_FIELDS
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_two_view_ransac_batch"][1]) == 13
    assert len(capi.SYMBOLS["pislam_two_view_denormalise"][1]) == 4
    assert [n for n, _ in capi.TwoViewParams._fields_] == TV_FIELDS and ctypes.sizeof(capi.TwoViewParams) == 16
    for f in ("twoViewRansacBatch", "twoViewDenormalise", "matchedPointsQ8", "twoViewModelRatio"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    assert hasattr(lib, "pislam_two_view_ransac_batch") and hasattr(lib, "pislam_two_view_denormalise")
    # the constants of the contract as the restatement holds them
    for word in ("0x7feb352d", "0x846ca68b", "0x9e3779b9", "0x85ebca6b", "0xc2b2ae35", "2^-20", "3.841f", "5.991f"):
        assert word in text, word


def test_ref_two_view_anchors():
    """The expectation itself, independent of the library."""
    # sampling: distinct, in range, every match when n == m, the same for the same counters
    for n, m in ((8, 8), (9, 8), (4, 4), (5, 4), (300, 8), (16384, 4)):
        for k in range(50):
            d = ref_sample(7, 3, k, n, m)
            assert len(set(d)) == m and min(d) >= 0 and max(d) < n and d == ref_sample(7, 3, k, n, m)
    assert sorted(ref_sample(1, 2, 3, 8, 8)) == list(range(8))
    assert ref_sample(1, 2, 3, 300, 8) != ref_sample(2, 2, 3, 300, 8) != ref_sample(2, 3, 3, 300, 8)
    firsts = np.bincount([ref_sample(5, 0, k, 10, 4)[3] for k in range(4000)], minlength=10)
    assert firsts.min() > 300 and firsts.max() < 500          # the last draw too is uniform over the 10 matches: 400 +- 5 sigma
    # a noise-free plane: the homography fits every match to a small fraction of a pixel; an exact translation likewise
    u, v, good = scene(1, True, n=60, outliers=0.0, noise=0.0)
    r = ref_pair(u.tolist(), v.tolist(), 0, HOMOG, 8, 1, 256)
    assert r["best"] >= 0 and r["ninliers"] == 60 and r["score"] > 2 * 60 * 1500
    H = ref_denormalise(HOMOG, r["model_n"], r["stats"])
    p = H @ np.vstack([u.T / 256.0, np.ones(60)])
    assert np.abs(p[:2] / p[2] - v.T / 256.0).max() < 0.05
    # no model: too few matches, identical points in either image, collinear points; the statistics are still written
    u, v, _ = scene(2, False, n=20)
    for model, m in SAMPLE.items():
        r = ref_pair(u[:m - 1].tolist(), v[:m - 1].tolist(), 0, model, 16, 0, 256)
        assert r["best"] == -1 and r["score"] == 0 and not r["model_n"].any() and r["stats"][0] == m - 1 and r["stats"][3] > 0
        same = np.tile(u[:1], (20, 1))
        for a, b in ((same, v), (u, same)):
            r = ref_pair(a.tolist(), b.tolist(), 0, model, 16, 0, 256)
            assert r["best"] == -1 and not r["inlier"].any() and (r["stats"][3] == 0) != (r["stats"][6] == 0)
        cu, cv = collinear(40, 3)
        r = ref_pair(cu.tolist(), cv.tolist(), 0, model, 64, 0, 256)
        assert r["best"] == -1 and r["stats"][3] > 0 and r["stats"][6] > 0
    # the clamp comes first
    far = [[5 << 20, -(7 << 20)], [1 << 20, 3], [-(1 << 20) - 1, 0]]
    assert ref_stats(far, far)[1] == [[1 << 20, -(1 << 20)] * 2, [1 << 20, 3] * 2, [-(1 << 20), 0] * 2]


BEHAVIOUR_SEEDS = {False: 1, True: 4}          # scene seeds 1..5 were tried for both cases with the restatement; all of
#   them meet the conditions (worst over the five: general depth 82.9 % of the true inliers at seed 2 and 1.7 % of the
#   outliers at seed 3; plane 88.3 % and 0 % with a ratio of 0.418 at seed 2)


def check_behaviour(run):
    """run(u, v, model, hypotheses, seed, sigma_q8) -> (score, inlier mask [n])."""
    u, v, good = scene(BEHAVIOUR_SEEDS[False], False)
    _, inl = run(u, v, FUND, 200, 1, 256)
    tp, fp = inl[good].mean(), inl[~good].mean()
    print("general depth, F: %.1f %% of the true inliers, %.1f %% of the outliers" % (100 * tp, 100 * fp))
    assert tp >= 0.75 and fp <= 0.10
    u, v, good = scene(BEHAVIOUR_SEEDS[True], True)
    sh, inl = run(u, v, HOMOG, 200, 1, 256)
    sf, _ = run(u, v, FUND, 200, 1, 256)
    tp, fp = inl[good].mean(), inl[~good].mean()
    from pislam_amd.frontend import twoViewModelRatio
    ratio = float(twoViewModelRatio(sh, sf))
    print("plane, H: %.1f %% of the true inliers, %.1f %% of the outliers, ratio %.3f" % (100 * tp, 100 * fp, ratio))
    assert tp >= 0.85 and fp <= 0.05 and ratio > 0.40
    assert ratio == sh / (sh + sf)


def test_behaviour_of_the_restatement():
    def run(u, v, model, hyp, seed, sigma):
        r = ref_pair(u.tolist(), v.tolist(), 0, model, hyp, seed, sigma)
        return r["score"], r["inlier"].astype(bool)
    check_behaviour(run)


def test_denormalise_against_numpy():
    """The host helper against float64 numpy on the restatement's outputs, and the pixel residuals of the true inliers
    the call marked: below the call's own threshold (chi2 < th at sigma = 1 px), with 0.1 % of room because the mask
    was decided in binary32 on normalised coordinates (relative error of a chi2 there: a few 2^-24 per operation, some
    dozen operations) and the residual here is float64 on pixels."""
    from pislam_amd import capi
    from pislam_amd.frontend import twoViewDenormalise
    lib = capi.load()
    for model, plane in ((FUND, False), (HOMOG, True)):
        u, v, good = scene(BEHAVIOUR_SEEDS[plane], plane)
        r = ref_pair(u.tolist(), v.tolist(), 0, model, 200, 1, 256)
        want = ref_denormalise(model, r["model_n"], r["stats"])
        got = twoViewDenormalise(model, r["model_n"], np.array(r["stats"], np.int64))
        assert got.shape == (3, 3) and np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
        both = twoViewDenormalise(model, np.stack([r["model_n"]] * 2), np.array([r["stats"]] * 2, np.int64))
        assert both.shape == (2, 3, 3) and (both[0] == got).all() and (both[1] == got).all()
        sel = good & r["inlier"].astype(bool)
        x1 = np.vstack([u[sel].T / 256.0, np.ones(sel.sum())])
        x2 = np.vstack([v[sel].T / 256.0, np.ones(sel.sum())])
        if model == FUND:
            l2, l1 = got @ x1, got.T @ x2
            d_a = (l2 * x2).sum(0) ** 2 / (l2[0] ** 2 + l2[1] ** 2)
            d_b = (l1 * x1).sum(0) ** 2 / (l1[0] ** 2 + l1[1] ** 2)
        else:
            f, g = got @ x1, np.linalg.inv(got) @ x2
            d_a = ((f[:2] / f[2] - x2[:2]) ** 2).sum(0)
            d_b = ((g[:2] / g[2] - x1[:2]) ** 2).sum(0)
        assert sel.sum() > 150 and max(d_a.max(), d_b.max()) < float(TH[model]) * 1.001
    # bad arguments
    m9, st, out = (ctypes.c_float * 9)(), (ctypes.c_int64 * 8)(5, 0, 0, 10, 0, 0, 10, 0), (ctypes.c_double * 9)()
    assert lib.pislam_two_view_denormalise(0, m9, st, out) == 0
    assert lib.pislam_two_view_denormalise(2, m9, st, out) == -1
    assert lib.pislam_two_view_denormalise(0, None, st, out) == -1 and lib.pislam_two_view_denormalise(0, m9, st, None) == -1
    for i, bad in ((0, 0), (3, 0), (6, 0)):
        st2 = (ctypes.c_int64 * 8)(*st)
        st2[i] = bad
        assert lib.pislam_two_view_denormalise(1, m9, st2, out) == -1
    assert np.isnan(twoViewDenormalise("H", np.zeros(9, np.float32), np.zeros(8, np.int64))).all()


# ---- matchedPointsQ8 ----------------------------------------------------------------------------------------------------
MP_LEVELS = [(40, 30, 0, 0), (33, 25, 30, 0), (28, 21, 30, 36)]          # (width, height, row0, col0): three levels
MP_SCALES = [65536, 79438, 93623]


def matched_points_case(device):
    import torch
    from pislam_amd.frontend import matchedPointsQ8
    rng = np.random.default_rng(9)
    B, QS, TS = 3, 24, 20

    def keypoints(n):
        out = []
        for i in range(n):
            if i % 7 == 5:
                x, y = 39, 58                                             # in no level
            else:
                w, h, r0, c0 = MP_LEVELS[i % 3]
                x, y = c0 + rng.integers(0, w), r0 + rng.integers(0, h)
            out.append((rng.integers(0, 256) << 24) | (int(x) << 12) | int(y))
        return np.array(out, np.int64)
    qkp = np.stack([keypoints(QS) for _ in range(B)])
    tkp = np.stack([keypoints(TS) for _ in range(B)])
    nsel = np.array([QS, 9, 0], np.int32)
    sel_q = np.stack([np.sort(rng.permutation(QS)) for _ in range(B)]).astype(np.int32)
    sel_t = rng.integers(0, TS, (B, QS)).astype(np.int32)
    refined = rng.integers(-300, 64 * 256, (B, QS, 2)).astype(np.int32)

    def level_of(k):
        x, y = (k >> 12) & 0xFFF, k & 0xFFF
        for l, (w, h, r0, c0) in enumerate(MP_LEVELS):
            if c0 <= x < c0 + w and r0 <= y < r0 + h:
                return l, x, y
        return None, x, y

    def to0(u, l):
        return (u * MP_SCALES[l] + 32768) // 65536

    for use_refined in (False, True):
        want1, want2 = np.zeros((B, QS, 2), np.int32), np.zeros((B, QS, 2), np.int32)
        wantn = np.zeros(B, np.int32)
        for b in range(B):
            for s in range(nsel[b]):
                q, t = sel_q[b, s], sel_t[b, s]
                lq, xq, yq = level_of(int(qkp[b, q]))
                lt, xt, yt = level_of(int(tkp[b, t]))
                if lq is None or lt is None:
                    continue
                w, h, r0, c0 = MP_LEVELS[lq]
                want1[b, wantn[b]] = to0((xq - c0) << 8, lq), to0((yq - r0) << 8, lq)
                if use_refined:
                    rx, ry = (int(v) for v in refined[b, q])
                    want2[b, wantn[b]] = to0(rx - (c0 << 8), lq), to0(ry - (r0 << 8), lq)
                else:
                    w, h, r0, c0 = MP_LEVELS[lt]
                    want2[b, wantn[b]] = to0((xt - c0) << 8, lt), to0((yt - r0) << 8, lt)
                wantn[b] += 1
        T = lambda a: torch.from_numpy(a).to(device)
        p1, p2, cnt = matchedPointsQ8(T(qkp.astype(np.int32)), T(tkp.astype(np.int32)), (T(sel_q), T(sel_t), T(nsel)), MP_LEVELS,
                                      MP_SCALES, refined=T(refined) if use_refined else None)
        assert p1.dtype == torch.int32 and p2.dtype == torch.int32 and cnt.dtype == torch.int32
        assert (cnt.cpu().numpy() == wantn).all() and 0 < wantn[1] < 9 and wantn[0] < QS
        assert (p1.cpu().numpy() == want1).all() and (p2.cpu().numpy() == want2).all()


def test_matched_points_q8_on_the_host():
    matched_points_case("cpu")


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class Device:
    OUTS = (("best", np.int32, ()), ("score", np.uint32, ()), ("ninliers", np.uint32, ()), ("inlier", np.uint8, None),
            ("model_n", np.uint32, (9,)), ("stats", np.int64, (8,)))

    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.ctx, self.lib, self.capi = torch, ctx, ctx.lib, capi

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def sentinels(self, B, stride):
        t = self.torch
        return dict(best=t.full((B,), SENT32, dtype=t.int32, device="cuda"), score=t.full((B,), SENT32, dtype=t.int32, device="cuda"),
                    ninliers=t.full((B,), SENT32, dtype=t.int32, device="cuda"),
                    inlier=t.full((B, stride), SENT8, dtype=t.uint8, device="cuda"),
                    model_n=t.full((B, 9), SENT32, dtype=t.int32, device="cuda"),
                    stats=t.full((B, 8), SENT32, dtype=t.int64, device="cuda"))

    def call(self, prm, p1, p2, counts, stride, batch, o):
        ptr = self.capi.ptr
        p = self.capi.TwoViewParams(*prm)
        return self.lib.pislam_two_view_ransac_batch(self.ctx.h, ctypes.byref(p), ptr(p1), ptr(p2), ptr(counts), stride, batch,
                                                     ptr(o["best"]), ptr(o["score"]), ptr(o["ninliers"]), ptr(o["inlier"]),
                                                     ptr(o["model_n"]), ptr(o["stats"]))

    def down(self, o):
        self.ctx.synchronize()
        r = {k: v.cpu().numpy() for k, v in o.items()}
        r["score"], r["ninliers"] = r["score"].view(np.uint32), r["ninliers"].view(np.uint32)
        r["model_n"] = r["model_n"].view(F32)
        return r

    def run(self, p1, p2, counts, model, hypotheses, seed, sigma_q8):
        """One call on sentinel-filled outputs, as numpy."""
        B, stride = p1.shape[:2]
        o = self.sentinels(B, stride)
        rc = self.call((model, hypotheses, seed, sigma_q8), self.up(p1.astype(np.int32)), self.up(p2.astype(np.int32)),
                       self.up(np.asarray(counts, np.uint32).view(np.int32)), stride, B, o)
        assert rc == 0, self.lib.pislam_last_error(self.ctx.h)
        return self.down(o)


def assert_same(got, want, what=""):
    """Every output word: floats are compared as their bit patterns."""
    for k in ("best", "score", "ninliers", "inlier", "stats"):
        bad = np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))
        assert len(bad) == 0, (what, k, bad[:5].tolist(), np.asarray(got[k])[tuple(bad[0])], np.asarray(want[k])[tuple(bad[0])])
    g, w = got["model_n"].view(np.uint32), want["model_n"].view(np.uint32)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (what, "model_n", bad[:5].tolist(), got["model_n"][tuple(bad[0])], want["model_n"][tuple(bad[0])])


PIN_STRIDE = 320
PIN_HYPOTHESES = (1, 63, 64, 65, 200, 512, 513, 1024)       # 512 / 513: the hypothesis loop's second trip


@functools.lru_cache(maxsize=None)
def pin_batch(model, small):
    """The pairs of the bit-exact pins: (p1, p2, counts).  Noisy scenes with outliers (a plane for H), cut to
    n = 0, m - 1, m, m + 1, 63, 64, 65 and 300; then a PISLAM_COUNT_INVALID pair, identical points in image 1 and in
    image 2, collinear points, a pair in which every match appears twice, and coordinates at and beyond +- 2^20.
    small = the subset the extreme hypothesis counts run on."""
    m = SAMPLE[model]
    ns = [m, 65, 300] if small else [0, m - 1, m, m + 1, 63, 64, 65, 300]
    pairs = []
    for i, n in enumerate(ns):
        u, v, _ = scene(20 + i, model == HOMOG)
        pairs.append((u[:n], v[:n], n))
    if not small:
        u, v, _ = scene(40, model == HOMOG)
        pairs.append((u[:50], v[:50], COUNT_INVALID))
        pairs.append((np.tile(u[:1], (30, 1)), v[:30], 30))
        pairs.append((u[:30], np.tile(v[7:8], (30, 1)), 30))
        cu, cv = collinear(40, 5)
        pairs.append((cu, cv, 40))
        pairs.append((np.repeat(u[:40], 2, 0), np.repeat(v[:40], 2, 0), 80))
        # the clamp: a scene scaled up until a third of it lies beyond +- 2^20, and exact boundary values
        big_u, big_v = (u[:60] - 320 * 256) * 9, (v[:60] - 320 * 256) * 9
        big_u[0], big_u[1], big_v[2], big_v[3] = (1 << 20, -(1 << 20)), ((1 << 20) + 1, -(1 << 20) - 1), (1 << 30, 5), (-(1 << 31), (1 << 31) - 1)
        assert (np.abs(big_u) > 1 << 20).any() and (np.abs(big_v) > 1 << 20).any()
        pairs.append((big_u, big_v, 60))
    B = len(pairs)
    rng = np.random.default_rng(77)
    p1 = rng.integers(-(1 << 31), 1 << 31, (B, PIN_STRIDE, 2)).astype(np.int64)       # garbage beyond the counts
    p2 = rng.integers(-(1 << 31), 1 << 31, (B, PIN_STRIDE, 2)).astype(np.int64)
    counts = np.zeros(B, np.int64)
    for b, (u, v, n) in enumerate(pairs):
        p1[b, :len(u)], p2[b, :len(v)], counts[b] = u, v, n
    return p1, p2, counts


@functools.lru_cache(maxsize=None)
def pin_reference(model, hypotheses, small):
    p1, p2, counts = pin_batch(model, small)
    return ref_batch(p1, p2, counts, model, hypotheses, 12345, 256)


def test_host_probe_against_the_restatement(tmp_path):
    """The library's own arithmetic header, compiled for the host with -ffp-contract=off, run serially: every output
    word of every pair of the twelve pin cases."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ransac_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "ransac_host_check.cpp"), "-o", exe])
    lines, want = [], []
    for model in (FUND, HOMOG):
        for hypotheses in PIN_HYPOTHESES:
            small = hypotheses not in (64, 200)                                       # as in test_two_view_pins
            p1, p2, counts = pin_batch(model, small)
            r = pin_reference(model, hypotheses, small)
            for b in range(len(counts)):
                n = 0 if int(counts[b]) == COUNT_INVALID else min(int(counts[b]), PIN_STRIDE)
                pts = np.concatenate([p1[b, :n], p2[b, :n]], 1).astype(np.int32)      # the call reads 32-bit words
                lines.append(" ".join(str(v) for v in [model, hypotheses, 12345, 256, b, n] + pts.ravel().tolist()))
                want.append(" ".join([str(int(r["best"][b])), str(int(r["score"][b])), str(int(r["ninliers"][b])),
                                      "".join(str(int(v)) for v in r["inlier"][b, :n]) or "-"] +
                                     ["%08x" % int(v) for v in r["model_n"][b].view(np.uint32)] +
                                     [str(int(v)) for v in r["stats"][b]]))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    got = subprocess.run([exe, str(cases)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want) == 2 * (6 * 3 + 2 * 14)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "case %d: %s" % (k, lines[k][:60])


@pytest.mark.gpu
@pytest.mark.parametrize("hypotheses", PIN_HYPOTHESES)
@pytest.mark.parametrize("model", [FUND, HOMOG])
def test_two_view_pins(gpu_ctx, model, hypotheses):
    """Every output word of the library equals the restatement's; what a call must not write keeps the sentinel."""
    small = hypotheses not in (64, 200)
    p1, p2, counts = pin_batch(model, small)
    want = pin_reference(model, hypotheses, small)
    got = Device(gpu_ctx).run(p1, p2, counts, model, hypotheses, 12345, 256)
    assert_same(got, want, (model, hypotheses))
    if not small:
        m = SAMPLE[model]
        assert list(want["best"][:3]) == [-1, -1, want["best"][2]] and (want["best"][8:12] == -1).all()
        assert (want["inlier"][7, 300:] == SENT8).all() and (want["inlier"][8] == SENT8).all() and not want["inlier"][9, :30].any()
        assert want["stats"][8, 0] == 0 and want["stats"][1, 0] == m - 1
        if hypotheses == 200:
            assert (want["best"][[3, 4, 5, 6, 7, 12]] >= 0).all() and want["ninliers"][7] > 150
            assert want["best"][13] >= 0                                  # the clamped pair still has a model


TRIP_HYPOTHESES, TRIP_NS = 65, (512, 513)


@functools.lru_cache(maxsize=None)
def second_trip_case(model):
    """Pairs of 512 and 513 matches: a workgroup scores 64 x 8 waves = 512 per trip, so the 513th is the scoring and the
    mask loop's second trip.  (p1, p2, counts, the restated outputs); the stride is just large enough."""
    u, v, good = scene(51, model == HOMOG, n=TRIP_NS[-1])
    assert good[512]                                                          # the scene's 513th match is a true one
    rng = np.random.default_rng(78)
    p1 = rng.integers(-(1 << 31), 1 << 31, (2, TRIP_NS[-1], 2)).astype(np.int64)      # garbage beyond the counts
    p2 = rng.integers(-(1 << 31), 1 << 31, (2, TRIP_NS[-1], 2)).astype(np.int64)
    for b, n in enumerate(TRIP_NS):
        p1[b, :n], p2[b, :n] = u[:n], v[:n]
    counts = np.array(TRIP_NS, np.int64)
    return p1, p2, counts, ref_batch(p1, p2, counts, model, TRIP_HYPOTHESES, 12345, 256)


@pytest.mark.parametrize("model", [FUND, HOMOG])
def test_second_trip_case_has_models(model):
    want = second_trip_case(model)[3]
    assert (want["best"] >= 0).all() and (want["ninliers"] > 200).all()
    assert want["inlier"][0, 512] == SENT8 and want["inlier"][1, 512] == 1    # the 513th is an inlier of its pair


@pytest.mark.gpu
@pytest.mark.parametrize("model", [FUND, HOMOG])
def test_two_view_second_trip_of_the_item_loops(gpu_ctx, model):
    p1, p2, counts, want = second_trip_case(model)
    assert_same(Device(gpu_ctx).run(p1, p2, counts, model, TRIP_HYPOTHESES, 12345, 256), want, (model, "second trip"))


@pytest.mark.gpu
def test_two_view_seed_and_determinism(gpu_ctx):
    d = Device(gpu_ctx)
    u, v, _ = scene(3, False)
    p1, p2 = u[None], v[None]
    a = d.run(p1, p2, [300], FUND, 200, 1, 256)
    b = d.run(p1, p2, [300], FUND, 200, 1, 256)
    c = d.run(p1, p2, [300], FUND, 200, 2, 256)
    assert_same(a, b)
    assert a["best"][0] >= 0 and c["best"][0] >= 0 and a["best"][0] != c["best"][0]
    assert a["best"][0] == ref_pair(u.tolist(), v.tolist(), 0, FUND, 200, 1, 256)["best"]


@pytest.mark.gpu
def test_two_view_behaviour_on_the_library(gpu_ctx):
    d = Device(gpu_ctx)

    def run(u, v, model, hyp, seed, sigma):
        r = d.run(u[None], v[None], [len(u)], model, hyp, seed, sigma)
        return int(r["score"][0]), r["inlier"][0].astype(bool)
    check_behaviour(run)


@pytest.mark.gpu
def test_two_view_invalid_arguments_write_nothing(gpu_ctx):
    d = Device(gpu_ctx)
    t = d.torch
    B, stride = 2, 16
    u, v, _ = scene(5, True, n=16)
    p1, p2 = d.up(np.stack([u, u]).astype(np.int32)), d.up(np.stack([v, v]).astype(np.int32))
    counts = d.up(np.array([16, 16], np.int32))
    o = d.sentinels(B, stride)
    good = (HOMOG, 8, 0, 256)
    bad_params = [(2, 8, 0, 256), (-1, 8, 0, 256), (0, 0, 0, 256), (0, 1025, 0, 256), (0, 8, 0, 0), (0, 8, 0, 4097)]
    for prm in bad_params:
        assert d.call(prm, p1, p2, counts, stride, B, o) == -1, prm
    assert d.call(good, p1, p2, counts, 0, B, o) == -1
    assert d.call(good, p1, p2, counts, MAX_STRIDE + 1, B, o) == -1
    assert d.call(good, p1, p2, counts, stride, -1, o) == -1
    ptr = d.capi.ptr
    assert d.lib.pislam_two_view_ransac_batch(gpu_ctx.h, None, ptr(p1), ptr(p2), ptr(counts), stride, B, ptr(o["best"]),
                                              ptr(o["score"]), ptr(o["ninliers"]), ptr(o["inlier"]), ptr(o["model_n"]),
                                              ptr(o["stats"])) == -1
    host = np.zeros(B * stride * 2, np.int32)
    for name in ("p1", "p2", "counts", "best", "score", "ninliers", "inlier", "model_n", "stats"):
        for repl in (None, host):                                         # NULL, then a host pointer
            ins = dict(p1=p1, p2=p2, counts=counts)
            outs = dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins["p1"], ins["p2"], ins["counts"], stride, B, outs) == -1, name
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, p1, p2, counts, stride, B, dict(o, best=counts)) == -1
    assert d.call(good, p1, p2, counts, stride, B, dict(o, inlier=p2.view(t.uint8))) == -1
    assert d.call(good, p1, p2, counts, stride, B, dict(o, score=o["best"])) == -1
    assert d.call(good, p1, p2, counts, stride, B, dict(o, ninliers=o["stats"].view(t.int32)[15:])) == -1
    r = d.down(o)
    assert (r["best"] == SENT32).all() and (r["score"] == SENT32).all() and (r["ninliers"] == SENT32).all()
    assert (r["inlier"] == SENT8).all() and (r["model_n"].view(np.uint32) == SENT32).all() and (r["stats"] == SENT32).all()
    # batch 0 is a no-op after the checks: the pointers are not looked at
    assert d.lib.pislam_two_view_ransac_batch(gpu_ctx.h, ctypes.byref(d.capi.TwoViewParams(*good)), None, None, None, stride, 0,
                                              None, None, None, None, None, None) == 0
    assert d.call(good, p1, p2, counts, stride, B, o) == 0
    assert (d.down(o)["best"] >= 0).all()


@pytest.mark.gpu
def test_two_view_graph_replay_equals_eager(gpu_ctx):
    """No workspace, no host round trip: the call is captured on a side stream (one stream, no parallel branches) of a
    fresh context without a warm-up call, and every replay writes what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import twoViewRansacBatch
    d = Device(gpu_ctx)
    u, v, _ = scene(6, True, n=100)
    p1, p2 = d.up(np.stack([u, u[::-1]]).astype(np.int32)), d.up(np.stack([v, v[::-1]]).astype(np.int32))
    counts = d.up(np.array([100, 64], np.int32))
    eager = twoViewRansacBatch(p1, p2, counts, model="H", hypotheses=65, seed=9, ctx=gpu_ctx)
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        o = d.sentinels(2, 100)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            twoViewRansacBatch(p1, p2, counts, model="H", hypotheses=65, seed=9, ctx=ctx, **o)
        for _ in range(2):
            for x in o.values():
                x.fill_(SENT8 if x.dtype == t.uint8 else SENT32)
            g.replay()
            side.synchronize()
            for a, (k, b) in zip(eager, o.items()):
                a, b = a.cpu().numpy(), b.cpu().numpy()
                if k == "inlier":
                    assert (a[0] == b[0]).all() and (a[1, :64] == b[1, :64]).all() and (b[1, 64:] == SENT8).all()
                else:
                    assert (a.view(np.uint8) == b.view(np.uint8)).all(), k
            assert (o["best"].cpu().numpy() >= 0).all()
        ctx.close()


@pytest.mark.gpu
def test_matched_points_q8_on_the_device(gpu_ctx):
    matched_points_case("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("model", [FUND, HOMOG])
def test_two_view_grid_passes(gpu_ctx, model):
    """The grid is capped at 1024 workgroups: 2051 pairs take three passes.  Pairs 0, 1023, 1024, 2047, 2048 and 2050
    hold 12 matches, the others 0..3 (no model; their statistics and zeroed masks are still pinned)."""
    B, stride = 2051, 12
    rng = np.random.default_rng(model)
    p1 = rng.integers(0, 640 * 256, (B, stride, 2))
    p2 = p1 + rng.integers(-2048, 2048, (B, stride, 2))
    counts = rng.integers(0, 4, B)
    u, v, _ = scene(8, model == HOMOG, n=12, outliers=0.0)
    for i, b in enumerate((0, 1023, 1024, 2047, 2048, 2050)):
        p1[b], p2[b], counts[b] = u + 256 * i, v - 256 * i, 12
    want = ref_batch(p1, p2, counts, model, 3, 4, 256)
    got = Device(gpu_ctx).run(p1, p2, counts, model, 3, 4, 256)
    assert_same(got, want)
    assert (want["best"][[0, 1023, 1024, 2047, 2048, 2050]] >= 0).all() and (want["best"] >= 0).sum() == 6


@pytest.mark.gpu
def test_two_view_offsets_beyond_4_gib(gpu_ctx):
    """stride 16384 and 32770 pairs: the points of pair 32769 begin beyond 2^32 bytes (each array allocated in one
    piece, uninitialised: with a count of 0 a pair's points are never read).  Pairs 1, 32768 and 32769 hold 12 matches."""
    d = Device(gpu_ctx)
    t = d.torch
    B, stride = 32770, MAX_STRIDE
    free, _ = t.cuda.mem_get_info()
    if free < 3 * (B * stride * 8) // 2 * 2:
        pytest.skip("two buffers of 4 GiB and the mask do not fit the free device memory")
    live = (1, 32768, 32769)
    assert live[-1] * stride * 8 > 1 << 32
    p1 = t.empty((B, stride, 2), dtype=t.int32, device="cuda")
    p2 = t.empty((B, stride, 2), dtype=t.int32, device="cuda")
    counts = t.zeros((B,), dtype=t.int32, device="cuda")
    o = dict(best=t.full((B,), SENT32, dtype=t.int32, device="cuda"), score=t.full((B,), SENT32, dtype=t.int32, device="cuda"),
             ninliers=t.full((B,), SENT32, dtype=t.int32, device="cuda"), inlier=t.empty((B, stride), dtype=t.uint8, device="cuda"),
             model_n=t.full((B, 9), SENT32, dtype=t.int32, device="cuda"), stats=t.full((B, 8), SENT32, dtype=t.int64, device="cuda"))
    u, v, _ = scene(8, True, n=12, outliers=0.0)
    for i, b in enumerate(live):
        p1[b, :12], p2[b, :12], counts[b] = d.up((u + 999 * i).astype(np.int32)), d.up((v - 77 * i).astype(np.int32)), 12
        o["inlier"][b, :16] = SENT8
    assert d.call((HOMOG, 5, 3, 256), p1, p2, counts, stride, B, o) == 0
    gpu_ctx.synchronize()
    best, stats = o["best"].cpu().numpy(), o["stats"].cpu().numpy()
    assert (np.delete(best, live) == -1).all() and not np.delete(stats, live, 0).any()
    for i, b in enumerate(live):
        r = ref_pair((u + 999 * i).tolist(), (v - 77 * i).tolist(), b, HOMOG, 5, 3, 256)
        assert r["best"] >= 0 and best[b] == r["best"] and int(o["score"][b]) == r["score"] and int(o["ninliers"][b]) == r["ninliers"]
        assert (o["inlier"][b, :16].cpu().numpy() == np.concatenate([r["inlier"], [SENT8] * 4])).all()
        assert (o["model_n"][b].cpu().numpy().view(np.uint32) == r["model_n"].view(np.uint32)).all()
        assert tuple(stats[b]) == r["stats"]
