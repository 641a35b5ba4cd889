"""pislam_pnp_ransac_batch: batched absolute-pose RANSAC (P3P, Lambda Twist) from 3D-2D matches.

The expectation is a numpy restatement of the contract (the comment in include/pislam_hip.h), written from that comment
and independent of the library: Python integers for everything integral, one numpy.float32 operation per binary32
operation.  The solver is stated over float32 ARRAYS, one element per hypothesis, and the scoring over arrays
[hypothesis][observation]: every element sees the contract's operations in the contract's order (a branch of the
contract is a numpy.where between both sides).  A hypothesis does not depend on how many are evaluated, so a frame's
1024 hypotheses are restated once and every hypothesis count reads its prefix.  The host probe (tools/probes/
pnp_host_check.cpp, the library's own arithmetic header under the host compiler) and the library on the GPU must agree
with it on every output word."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F32, F64 = np.float32, np.float64
M32 = 0xFFFFFFFF
COUNT_INVALID = 0xFFFFFFFF
MONO = -(1 << 31)
OBS_MAX = 1 << 22
MAX_STRIDE = 16384
MAX_HYP = 1024
Z_MIN = F32(2.0 ** -10)
TH = F32(5.991)
SENT8, SENT32 = 0xA5, 0x5A5A5A5A
PNP_FIELDS = ["hypotheses", "seed", "min_inliers"]
ONE, TWO, THREE, FOUR, HALF = F32(1.0), F32(2.0), F32(3.0), F32(4.0), F32(0.5)


# ---- the restatement: sampling ----------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def pnp_hash(seed, b, k, j):
    h = mix32((seed & M32) + 0x9E3779B9 * (b & M32))
    h = mix32(h ^ ((0x85EBCA6B * (k + 1)) & M32))
    return mix32(h ^ ((0xC2B2AE35 * (j + 1)) & M32))


def ref_sample(seed, b, k, n, m=4):
    """The m distinct observation indices of hypothesis k, in draw order."""
    drawn = []
    for j in range(m):
        r = (pnp_hash(seed, b, k, j) * (n - j)) >> 32
        for c in sorted(drawn):
            if r >= c:
                r += 1
        drawn.append(r)
    return drawn


# ---- the restatement: observations, chi2, score -------------------------------------------------------------------------
def ref_obs(fr):
    """The frame's observations as the call reads them: float32 arrays X, Y, Z, u, v, w and the level's verdict."""
    xw = np.asarray(fr["xw"], F32).reshape(-1, 3)
    obs = np.asarray(fr["obs"], np.int64).reshape(-1, 3)
    q = np.clip(obs[:, :2], -OBS_MAX, OBS_MAX).astype(F32) * F32(1.0 / 256.0)
    n = len(xw)
    w, ok = np.ones(n, F32), np.ones(n, bool)
    if fr.get("level") is not None:
        tab = np.asarray(fr["tab"], F32)
        lv = np.asarray(fr["level"], np.int64)
        ok = lv < len(tab)
        w = np.where(ok, tab[np.where(ok, lv, 0)], ONE).astype(F32)
    return dict(X=xw[:, 0].copy(), Y=xw[:, 1].copy(), Z=xw[:, 2].copy(), u=q[:, 0].copy(), v=q[:, 1].copy(), w=w, ok=ok)


def pick(O, idx):
    return {k: v[idx] for k, v in O.items()}


def ref_chi2(T, cam, O):
    """(live, chi2) of the observations O under the poses T (12 float32 arrays that broadcast against O's)."""
    fx, fy, cx, cy = cam[0], cam[1], cam[2], cam[3]
    X, Y, Z = O["X"], O["Y"], O["Z"]
    x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9]
    y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10]
    z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11]
    live = O["ok"] & (z >= Z_MIN)
    iz = ONE / z
    pu, pv = fx * (x * iz) + cx, fy * (y * iz) + cy
    eu, ev = O["u"] - pu, O["v"] - pv
    chi2 = (eu * eu + ev * ev) * O["w"]
    assert chi2.dtype == F32
    return live & np.isfinite(chi2), chi2


def ref_scores(T, cam, O):
    """(inlier [.., n] bool, what each observation adds [.., n] int64)."""
    live, chi2 = ref_chi2(T, cam, O)
    inl = live & (chi2 < TH)
    add = np.floor((TH - chi2) * F32(256.0))
    return inl, np.where(inl, add, 0).astype(np.int64)


# ---- the restatement: the solver, one element per hypothesis ----------------------------------------------------------------
def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def ref_bearing(cam, ifx, ify, u, v):
    xn, yn = (u - cam[2]) * ifx, (v - cam[3]) * ify
    r = ONE / np.sqrt((xn * xn + yn * yn) + ONE)
    return [xn * r, yn * r, r]


def ref_cubic(B, C, D):
    h = lambda t: ((t + B) * t + C) * t + D
    hp = lambda t: (THREE * t + TWO * B) * t + C
    bb, c3 = B * B, THREE * C
    v = np.sqrt(bb - c3)
    t1 = (-B - v) / THREE
    k1 = h(t1)
    ra = t1 - np.sqrt(-k1 / (THREE * t1 + B))
    t2 = (-B + v) / THREE
    k2 = h(t2)
    rb = t2 + np.sqrt(-k2 / (THREE * t2 + B))
    r0 = -B / THREE
    r0 = np.where(np.abs(hp(r0)) < F32(1e-4), r0 + ONE, r0)
    r = np.where(bb >= c3, np.where(k1 > 0, ra, rb), r0)
    for _ in range(12):
        f, fp = h(r), hp(r)
        r = np.where(fp != 0, r - f / fp, r)
    assert r.dtype == F32
    return r


def ref_solver(cam, o1, o2, o3, o4):
    """Steps 1 to 9 of the contract.  o1..o3 are the minimal problem, o4 the fourth draw, each a dict of arrays with
    one element per hypothesis.  Returns (valid bool [H], T: 12 float32 arrays [H])."""
    cam = np.asarray(cam, F32)
    with np.errstate(all="ignore"):
        ifx, ify = ONE / cam[0], ONE / cam[1]
        y1, y2, y3 = (ref_bearing(cam, ifx, ify, o["u"], o["v"]) for o in (o1, o2, o3))
        x1, x2, x3 = ([o["X"], o["Y"], o["Z"]] for o in (o1, o2, o3))
        b12, b13, b23 = F32(-2.0) * dot3(y1, y2), F32(-2.0) * dot3(y1, y3), F32(-2.0) * dot3(y2, y3)
        d12, d13, d23 = ([p[i] - q[i] for i in range(3)] for p, q in ((x1, x2), (x1, x3), (x2, x3)))
        a12, a13, a23 = dot3(d12, d12), dot3(d13, d13), dot3(d23, d23)
        c12, c23, c31 = F32(-0.5) * b12, F32(-0.5) * b23, F32(-0.5) * b13
        s12, s23, s31 = ONE - c12 * c12, ONE - c23 * c23, ONE - c31 * c31
        blob = (c12 * c23) * c31 - ONE
        p3 = a13 * (a23 * s31 - a13 * s23)
        p2 = (((TWO * blob) * a23) * a13 + (a13 * (TWO * a12 + a13)) * s23) + (a23 * (a23 - a12)) * s31
        p1 = ((a23 * (a13 - a23)) * s12 - (a12 * a12) * s23) - (TWO * a12) * (blob * a23 + a13 * s23)
        p0 = a12 * (a12 * s23 - a23 * s12)
        alive = ~(p3 == 0)
        ip = ONE / p3
        g = ref_cubic(p2 * ip, p1 * ip, p0 * ip)

        A00, A01, A02 = a23 * (ONE - g), (a23 * b12) * HALF, ((a23 * b13) * g) * F32(-0.5)
        A11, A12, A22 = (a23 - a12) + a13 * g, (b23 * (a13 * g - a12)) * HALF, g * (a13 - a23) - a12
        x01 = A01 * A01
        eb = (-A00 - A11) - A22
        ec = (((-x01 - A02 * A02) - A12 * A12) + A00 * (A11 + A22)) + A11 * A22
        disc = eb * eb - FOUR * ec
        disc = np.where(disc > 0, disc, F32(0.0))
        sq = np.sqrt(disc)
        L0 = np.where(eb < 0, -eb + sq, -eb - sq) * HALF
        L1 = ec / L0
        prec0, prec1 = A01 * A12 - A02 * A11, A01 * A02 - A00 * A12

        def eigenvector(e):
            tmp = ONE / (((e * (A00 + A11) - A00 * A11) - e * e) + x01)
            e1, e2 = -((e * A02 + prec0) * tmp), -((e * A12 + prec1) * tmp)
            rn = ONE / np.sqrt((e1 * e1 + e2 * e2) + ONE)
            return e1 * rn, e2 * rn, rn
        V00, V10, V20 = eigenvector(L0)
        V01, V11, V21 = eigenvector(L1)
        q = -L1 / L0
        v = np.where(q > 0, np.sqrt(q), F32(0.0))

        nx = cross3(d12, d13)
        m00, m01, m02, m10, m11, m12, m20, m21, m22 = d12[0], d13[0], nx[0], d12[1], d13[1], nx[1], d12[2], d13[2], nx[2]
        i00, i01, i02 = m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11
        i10, i11, i12 = m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12
        i20, i21, i22 = m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10
        idet = ONE / ((m00 * i00 + m01 * i10) + m02 * i20)
        Xi = [[i00 * idet, i01 * idet, i02 * idet], [i10 * idet, i11 * idet, i12 * idet], [i20 * idet, i21 * idet, i22 * idet]]

        H = len(p3)
        best = np.full(H, np.inf, F32)
        found = np.zeros(H, bool)
        T = [np.zeros(H, F32) for _ in range(12)]
        for s in (v, -v):
            w2 = ONE / (s * V01 - V00)
            w0, w1 = (V10 - s * V11) * w2, (V20 - s * V21) * w2
            qa = ONE / ((((a13 - a12) * w1) * w1 - (a12 * b13) * w1) - a12)
            qb = (((a13 * b12) * w1 - (a12 * b13) * w0) - ((TWO * w0) * w1) * (a12 - a13)) * qa
            qc = ((((a13 - a12) * w0) * w0 + (a13 * b12) * w0) + a13) * qa
            dq = qb * qb - FOUR * qc
            sq = np.sqrt(dq)
            for tau in ((-qb + sq) * HALF, (-qb - sq) * HALF):
                d = a23 / (tau * (b23 + tau) + ONE)
                l2 = np.sqrt(d)
                l3 = tau * l2
                l1 = w0 * l2 + w1 * l3
                ok = alive & (dq >= 0) & (tau > 0) & (d > 0) & (l1 >= 0)
                for _ in range(5):
                    r1 = ((l1 * l1 + l2 * l2) + (b12 * l1) * l2) - a12
                    r2 = ((l1 * l1 + l3 * l3) + (b13 * l1) * l3) - a13
                    r3 = ((l2 * l2 + l3 * l3) + (b23 * l2) * l3) - a23
                    v0, v1 = TWO * l1 + b12 * l2, TWO * l2 + b12 * l1
                    v3, v5 = TWO * l1 + b13 * l3, TWO * l3 + b13 * l1
                    v7, v8 = TWO * l2 + b23 * l3, TWO * l3 + b23 * l2
                    jd = ONE / (-((v0 * v5) * v7) - (v1 * v3) * v8)
                    n1 = ((v1 * v5) * r3 - (v5 * v7) * r1) - (v1 * v8) * r2
                    n2 = ((v0 * v8) * r2 - (v3 * v8) * r1) - (v0 * v5) * r3
                    n3 = ((v3 * v7) * r1 - (v0 * v7) * r2) - (v1 * v3) * r3
                    l1, l2, l3 = l1 - n1 * jd, l2 - n2 * jd, l3 - n3 * jd
                ry1 = [l1 * y1[i] for i in range(3)]
                e1 = [ry1[i] - l2 * y2[i] for i in range(3)]
                e2 = [ry1[i] - l3 * y3[i] for i in range(3)]
                e3 = cross3(e1, e2)
                P = [None] * 12
                for i in range(3):
                    for j in range(3):
                        P[3 * i + j] = (e1[i] * Xi[0][j] + e2[i] * Xi[1][j]) + e3[i] * Xi[2][j]
                    P[9 + i] = ry1[i] - ((P[3 * i] * x1[0] + P[3 * i + 1] * x1[1]) + P[3 * i + 2] * x1[2])
                for c in P:
                    assert c.dtype == F32
                    ok = ok & np.isfinite(c)
                live, chi2 = ref_chi2(P, cam, o4)
                take = ok & live & (chi2 < best)
                best = np.where(take, chi2, best)
                found = found | take
                T = [np.where(take, P[i], T[i]) for i in range(12)]
    return found, T


def cam_ok(cam):
    cam = np.asarray(cam, F32)
    return bool(np.isfinite(cam).all() and cam[0] != 0 and cam[1] != 0)


def ref_hypotheses(fr, seed, b, K=MAX_HYP):
    """Hypotheses 0 .. K-1 of frame b: None when nothing is evaluated, else dict(valid [K], T [K][12], score [K],
    inl [K][n])."""
    n = len(fr["obs"])
    if not cam_ok(fr["cam"]) or n < 4:
        return None
    O = ref_obs(fr)
    draws = np.array([ref_sample(seed, b, k, n) for k in range(K)])
    valid, T = ref_solver(fr["cam"], *(pick(O, draws[:, j]) for j in range(4)))
    with np.errstate(all="ignore"):
        inl, add = ref_scores([t[:, None] for t in T], np.asarray(fr["cam"], F32), O)
    score = np.where(valid, add.sum(1), 0)
    return dict(valid=valid, T=np.stack(T, 1), score=score, inl=inl)


def ref_result(fr, hyp, hypotheses, min_inliers):
    """One frame of the call from its restated hypotheses: dict(best, score, ninliers, inlier, pose, status)."""
    n = len(fr["obs"])
    out = dict(best=-1, score=0, ninliers=0, inlier=np.zeros(n, np.uint8), pose=np.zeros(12, F32), status=2)
    if not cam_ok(fr["cam"]):
        out["status"] = 3
        return out
    if hyp is None:
        return out
    valid, score = hyp["valid"][:hypotheses], hyp["score"][:hypotheses]
    nvalid = int(valid.sum())
    out["status"] = 2 | nvalid << 8
    if nvalid == 0 or int(score.max()) == 0:
        return out
    k = int(np.argmax(score))                                # the first of the largest: the smallest k wins a tie
    inl = hyp["inl"][k]
    out.update(best=k, score=int(score[k]), ninliers=int(inl.sum()), inlier=inl.astype(np.uint8), pose=hyp["T"][k].copy())
    out["status"] = (1 if out["ninliers"] < min_inliers else 0) | nvalid << 8
    return out


def ref_frame(fr, b, hypotheses, seed, min_inliers=10):
    return ref_result(fr, ref_hypotheses(fr, seed, b, hypotheses), hypotheses, min_inliers)


# ---- scenes -----------------------------------------------------------------------------------------------------------
CAM = np.array([500, 500, 320, 240, 40], F32)


def rodrigues(r):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    K = K / th
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def scene(seed, n=300, outliers=0.4, noise=0.75, levels=False, scale=1.0, cam=CAM):
    """The issue's scene: pixels uniform over a VGA image, depths 2..20, a rotation of up to 1 rad, pixel noise uniform
    in +-noise, a share `outliers` displaced by 30..200 px; Q8-rounded pixels.  `scale` multiplies the world (points and
    translation), `cam` is the camera (fx, fy, cx, cy, bf).  Returns the frame, the true pose (R, t) and the mask of undisplaced observations."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = (float(c) for c in cam[:4])
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
    z = rng.uniform(2, 20, n)
    xc = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
    axis = rng.normal(0, 1, 3)
    R, t = rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0, 1)), rng.uniform(-2, 2, 3)
    xw = ((xc - t) @ R) * scale                                              # xc = R xw + t
    xw = xw.astype(F32)
    xc = xw.astype(F64) @ R.T + t * scale
    uv = np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1) + rng.uniform(-noise, noise, (n, 2))
    out = rng.permutation(n)[:int(round(outliers * n))]
    ang, mag = rng.uniform(0, 2 * math.pi, len(out)), rng.uniform(30, 200, len(out))
    uv[out] += np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None]
    obs = np.concatenate([np.rint(uv * 256), np.full((n, 1), MONO)], 1).astype(np.int64)
    good = np.ones(n, bool)
    good[out] = False
    level = rng.integers(0, 4, n).astype(np.uint8) if levels else None
    tab = np.array([1.0, 0.7, 0.5, 0.35], F32) if levels else None
    return dict(cam=np.array(cam, F32), xw=xw, obs=obs, level=level, tab=tab), (R, t * scale), good


def sub(fr, n):
    return {k: (v[:n] if k in ("xw", "obs", "level") and v is not None else v) for k, v in fr.items()}


def hexf(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


def probe_line(fr, b, hypotheses, seed, min_inliers):
    n = len(fr["obs"])
    has = fr.get("level") is not None
    tab = np.asarray(fr["tab"], F32) if has else np.zeros(0, F32)
    parts = ["%d %d %d %d %d %d %d" % (hypotheses, seed, min_inliers, b, int(has), len(tab), n), hexf(fr["cam"])]
    if len(tab):
        parts.append(hexf(tab))
    xw = np.asarray(fr["xw"], F32).reshape(-1, 3).view(np.uint32)
    lv = fr["level"] if has else np.zeros(n, np.uint8)
    for i in range(n):
        o = fr["obs"][i]
        parts.append("%08x %08x %08x %d %d %d %d" % (xw[i, 0], xw[i, 1], xw[i, 2], o[0], o[1], o[2], lv[i]))
    return " ".join(parts)


def result_line(r):
    inl = "".join(str(int(v)) for v in r["inlier"]) or "-"
    return "%d %d %d %d %s %s" % (r["best"], r["score"], r["ninliers"], r["status"], hexf(r["pose"]), inl)


def parse_result(line, n):
    w = line.split()
    inl = np.zeros(0, np.uint8) if w[16] == "-" else np.array([int(c) for c in w[16]], np.uint8)
    assert len(inl) == n
    pose = np.array([int(x, 16) for x in w[4:16]], np.uint32).view(F32)
    return dict(best=int(w[0]), score=int(w[1]), ninliers=int(w[2]), status=int(w[3]), pose=pose, inlier=inl)


@pytest.fixture(scope="module")
def run_probe(tmp_path_factory):
    """run_probe(lines, ns): the host probe's output lines and their parsed form, one per case line."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pnp_probe") / "pnp_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "pnp_host_check.cpp"), "-o", exe])

    def run(lines, ns):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got, [parse_result(g, n) for g, n in zip(got, ns)]
    return run


# ---- CPU: declarations, the expectation's anchors ---------------------------------------------------------------------------
def test_pnp_ransac_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_pnp_ransac_batch\s*\(", code), "not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_pnp_params \{([^}]*)\} pislam_pnp_params;", code)
    assert m and re.findall(r"(?:int32_t|uint32_t)\s+(\w+)\s*;", m.group(1)) == PNP_FIELDS
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_pnp_ransac_batch"][1]) == 17
    assert [n for n, _ in capi.PnpParams._fields_] == PNP_FIELDS and ctypes.sizeof(capi.PnpParams) == 12
    assert callable(frontend.pnpRansacBatch)
    assert hasattr(capi.load(), "pislam_pnp_ransac_batch")
    for f in ("pislam_pnp_math.h", "pislam_pnp_kernels.h"):
        assert os.path.exists(os.path.join(ROOT, "pislam_amd", "csrc", f)), f
    assert os.path.exists(os.path.join(ROOT, "tools", "probes", "pnp_host_check.cpp"))


def exact_case():
    """Identity rotation, t = 0, four points in general position whose pixels are exact in Q8 at f = 500:
    (1, 0, 5) -> (420, 240), (-1, 1, 5) -> (220, 340), (0, -1, 4) -> (320, 115), (2, 1, 8) -> (445, 302.5)."""
    xw = np.array([[1, 0, 5], [-1, 1, 5], [0, -1, 4], [2, 1, 8]], F32)
    px = np.array([[420, 240], [220, 340], [320, 115], [445, 302.5]])
    obs = np.concatenate([px * 256, np.full((4, 1), MONO)], 1).astype(np.int64)
    assert (obs[:, :2] == px * 256).all()
    return dict(cam=CAM.copy(), xw=xw, obs=obs, level=None, tab=None)


SAMPLER_ANCHOR = ([256, 199, 217, 255], [151, 295, 227, 269])


def test_ref_pnp_anchors():
    """The expectation itself, independent of the library."""
    # the sampler: the two-view call's, with m = 4.  The first draws of (seed 7, b 3, k 0 and 1) at n = 300, worked out
    # once with integers alone, and the sampler's properties.
    assert ref_sample(7, 3, 0, 300) == SAMPLER_ANCHOR[0] and ref_sample(7, 3, 1, 300) == SAMPLER_ANCHOR[1]
    for n in (4, 5, 96, 300, 16384):
        for k in range(50):
            d = ref_sample(7, 3, k, n)
            assert len(set(d)) == 4 and min(d) >= 0 and max(d) < n
    assert sorted(ref_sample(1, 2, 3, 4)) == [0, 1, 2, 3]
    assert ref_sample(1, 2, 3, 300) != ref_sample(2, 2, 3, 300) != ref_sample(2, 3, 3, 300)
    # the exact case.  The issue's prototype measured the binary32 solver's worst reprojection at 0.022 px with f = 500,
    # that is 4.4e-5 rad; a rotation entry may be off by that much and a translation entry by that times the depth (up
    # to 8 here).  Bounds: 1024 ulps of 1.0f (1024 * 2^-23 = 1.2e-4) on R, 8 times that on t.  Every hypothesis samples
    # the same four points in another order, so every valid one must meet them.
    fr = exact_case()
    hyp = ref_hypotheses(fr, 11, 0, 24)
    assert hyp["valid"].any()
    ulp = 2.0 ** -23
    want = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F64)
    for k in np.nonzero(hyp["valid"])[0]:
        err = np.abs(hyp["T"][k].astype(F64) - want)
        assert err[:9].max() <= 1024 * ulp and err[9:].max() <= 8192 * ulp, (k, err)
        assert hyp["inl"][k].all()
    r = ref_result(fr, hyp, 24, 4)
    assert r["best"] >= 0 and r["ninliers"] == 4 and r["status"] & 255 == 0 and r["inlier"].tolist() == [1, 1, 1, 1]
    assert ref_result(fr, hyp, 24, 5)["status"] & 255 == 1
    assert r["score"] > 4 * 1500                              # four residuals of a small fraction of a pixel
    # codes: too few, a bad camera
    assert ref_frame(sub(fr, 3), 0, 8, 0)["status"] == 2
    for idx, bad in ((0, 0.0), (1, 0.0), (2, np.nan), (4, np.inf), (0, -np.inf)):
        g = dict(fr, cam=fr["cam"].copy())
        g["cam"][idx] = bad
        r = ref_frame(g, 0, 8, 0)
        assert r["status"] == 3 and r["best"] == -1 and not r["pose"].any()
    # every level out of the table: the fourth draw is dead under every pose, so no hypothesis is valid
    dead = dict(fr, level=np.full(4, 9, np.uint8), tab=np.ones(2, F32))
    assert ref_frame(dead, 0, 8, 0)["status"] == 2


# ---- the pin cases: the smallest shapes where the kernel can go wrong -------------------------------------------------
PIN_STRIDE = 96
PIN_HYPOTHESES = (1, 63, 64, 65, 200, 512, 513, 1024)   # 512 / 513: the hypothesis loop's second trip
PIN_SEED, PIN_MIN = 5, 10


@functools.lru_cache(maxsize=None)
def pin_frames():
    """(name, frame, count as passed); every frame carries levels (a call without a level table ignores them)."""
    out = []
    big = scene(21, n=PIN_STRIDE, outliers=0.3, levels=True)[0]
    for n in (0, 3, 4, 5, 70, 96):
        out.append(("n%d" % n, sub(big, n), n))
    out.append(("count above stride", big, 200))
    out.append(("invalid count", sub(big, 40), COUNT_INVALID))
    fr = scene(22, n=40, outliers=0.2, levels=True)[0]
    fr["xw"][::5] *= F32(-1)                                              # behind the camera under the true pose
    out.append(("behind", fr, 40))
    fr = scene(23, n=40, outliers=0.2, levels=True)[0]
    fr["xw"][3, 1], fr["xw"][10, 0], fr["xw"][20, 2] = np.nan, np.inf, -np.inf
    fr["obs"][30] = (1 << 30, -(1 << 30), 7)
    out.append(("non-finite points", fr, 40))
    fr = scene(24, n=20, levels=True)[0]
    fr["cam"][0] = 0.0
    out.append(("fx zero", fr, 20))
    fr = scene(25, n=20, levels=True)[0]
    fr["cam"][4] = np.inf
    out.append(("cam infinite", fr, 20))
    fr = scene(26, n=60, outliers=0.2, levels=True)[0]
    fr["level"][::3] = 4 + (np.arange(len(fr["level"][::3])) % 3) * 100    # levels out of the table: 4, 104, 204
    out.append(("bad levels", fr, 60))
    return out


def clamp_count(count, stride):
    return 0 if count == COUNT_INVALID else min(count, stride)


def pin_frame(k, with_level):
    _, fr, count = pin_frames()[k]
    f = sub(fr, clamp_count(count, PIN_STRIDE))
    return f if with_level else dict(f, level=None, tab=None)


@functools.lru_cache(maxsize=None)
def pin_hypotheses(with_level):
    return [ref_hypotheses(pin_frame(k, with_level), PIN_SEED, k) for k in range(len(pin_frames()))]


def pin_reference(hypotheses, with_level):
    return [ref_result(pin_frame(k, with_level), h, hypotheses, PIN_MIN) for k, h in enumerate(pin_hypotheses(with_level))]


def test_pin_cases_cover_the_codes():
    for with_level in (True, False):
        want = pin_reference(200, with_level)
        names = [f[0] for f in pin_frames()]
        code = {n: w["status"] & 255 for n, w in zip(names, want)}
        assert code["n0"] == 2 and code["n3"] == 2 and code["invalid count"] == 2
        assert code["fx zero"] == 3 and code["cam infinite"] == 3
        assert code["n70"] == 0 and code["n96"] == 0 and code["count above stride"] == 0 and code["behind"] == 0
        assert code["n4"] in (1, 2) and code["n5"] in (1, 2)
        assert want[names.index("n96")]["ninliers"] >= 50
        assert want[names.index("n96")]["status"] >> 8 > 100
    lv = pin_reference(200, True)[-1]
    assert not lv["inlier"][::3].any() and lv["ninliers"] >= 20


def test_host_probe_against_the_restatement(run_probe):
    """The library's own arithmetic header, compiled for the host with -ffp-contract=off, run serially: every output
    word of every pin frame, with and without the level table, at every pinned hypothesis count."""
    lines, want, ns = [], [], []
    for with_level in (True, False):
        for hypotheses in PIN_HYPOTHESES:
            for k, r in enumerate(pin_reference(hypotheses, with_level)):
                fr = pin_frame(k, with_level)
                lines.append(probe_line(fr, k, hypotheses, PIN_SEED, PIN_MIN))
                want.append(result_line(r))
                ns.append(len(fr["obs"]))
    fr = exact_case()
    lines.append(probe_line(fr, 0, 24, 11, 4))
    want.append(result_line(ref_frame(fr, 0, 24, 11, 4)))
    ns.append(4)
    got, _ = run_probe(lines, ns)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "case %d: %s" % (k, lines[k][:40])


# ---- behaviour, on the host probe's output ------------------------------------------------------------------------------
BEHAVIOUR_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def behaviour_scenes():
    return [scene(s) for s in BEHAVIOUR_SEEDS]


def collinear_frame():
    """Four world points on a line parallel to an axis: d12 x d13 is exactly zero."""
    fr = exact_case()
    fr["xw"] = np.array([[-1, 0.5, 6], [0, 0.5, 6], [1, 0.5, 6], [2, 0.5, 6]], F32)
    px = 500 * fr["xw"][:, :2].astype(F64) / 6 + np.array([320, 240])
    fr["obs"] = np.concatenate([np.rint(px * 256), np.full((4, 1), MONO)], 1).astype(np.int64)
    return fr


def test_behaviour_on_the_host_probe(run_probe):
    """The issue's scene (300 observations, 40 % displaced by 30..200 px, noise uniform in +-0.75 px, f = 500, 200
    hypotheses, three seeds): no displaced observation is an inlier, at least 90 % of the others are, the rotation is
    orthonormal to 1e-3; the same world scaled by 100 gives the same mask; four collinear points give code 2."""
    scenes = behaviour_scenes()
    scaled = [scene(s, scale=100.0) for s in BEHAVIOUR_SEEDS]
    lines = [probe_line(fr, b, 200, 7, 10) for b, (fr, _, _) in enumerate(scenes)]
    lines += [probe_line(fr, b, 200, 7, 10) for b, (fr, _, _) in enumerate(scaled)]
    lines.append(probe_line(collinear_frame(), 0, 64, 7, 4))
    _, res = run_probe(lines, [300] * 6 + [4])
    for b, ((fr, truth, good), r) in enumerate(zip(scenes, res[:3])):
        inl = r["inlier"].astype(bool)
        R = r["pose"][:9].astype(F64).reshape(3, 3)
        print("pnp behaviour, seed %d: %d of %d undisplaced are inliers, %d displaced, |R'R - I| = %.2e, valid = %d" % (
            BEHAVIOUR_SEEDS[b], (inl & good).sum(), good.sum(), (inl & ~good).sum(), np.abs(R.T @ R - np.eye(3)).max(),
            r["status"] >> 8))
    for b, ((fr, truth, good), r) in enumerate(zip(scenes, res[:3])):
        inl = r["inlier"].astype(bool)
        assert r["status"] & 255 == 0 and r["best"] >= 0 and r["ninliers"] == inl.sum()
        assert not (inl & ~good).any()
        assert (inl & good).sum() >= 0.9 * good.sum()
    for r in res[:6]:
        R = r["pose"][:9].astype(F64).reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-3
    for b, (r, rs) in enumerate(zip(res[:3], res[3:6])):
        assert (scaled[b][2] == scenes[b][2]).all()
        assert rs["status"] & 255 == 0 and (rs["inlier"] == r["inlier"]).all(), BEHAVIOUR_SEEDS[b]
    assert res[6]["status"] & 255 == 2 and res[6]["best"] == -1 and not res[6]["pose"].any()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
OUT_NAMES = ("best", "score", "ninliers", "inlier", "pose_out", "status")


class Device:
    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.capi, self.ctx, self.lib = torch, capi, ctx, ctx.lib

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def sentinels(self, B, stride):
        t = self.torch
        word = lambda: t.full((B,), SENT32, dtype=t.int32, device="cuda")
        return dict(best=word(), score=word(), ninliers=word(),
                    inlier=t.full((B, stride), SENT8, dtype=t.uint8, device="cuda"),
                    pose_out=t.full((B, 12), SENT32, dtype=t.int32, device="cuda").view(t.float32), status=word())

    def pack(self, frames, counts, stride, with_level=True):
        """Host arrays of a batch: slots at and beyond a frame's observations hold rubbish that must not be read."""
        B = len(frames)
        rng = np.random.default_rng(99)
        xw = rng.normal(0, 1e30, (B, stride, 3)).astype(F32)
        obs = rng.integers(-1 << 31, 1 << 31, (B, stride, 3)).astype(np.int32)
        level = rng.integers(0, 256, (B, stride)).astype(np.uint8)
        cam = np.zeros((B, 5), F32)
        tab = None
        for b, fr in enumerate(frames):
            n = len(fr["obs"])
            cam[b], xw[b, :n], obs[b, :n] = fr["cam"], fr["xw"], fr["obs"]
            if fr.get("level") is not None:
                level[b, :n] = fr["level"]
                tab = np.asarray(fr["tab"], F32)
        cnt = np.array(counts, np.uint32).view(np.int32)
        with_level = with_level and tab is not None           # frames without levels go without the table
        return dict(cam=cam, xw=xw, obs=obs, counts=cnt, level=level if with_level else None, tab=tab if with_level else None)

    def upload(self, h):
        return {k: (self.up(v) if k != "tab" and v is not None else v) for k, v in h.items()}

    def call(self, prm, d, stride, B, o, level="d", tab="d", nlevels=None):
        ptr = self.capi.ptr
        p = self.capi.PnpParams(*prm) if prm is not None else None
        level = d.get("level") if isinstance(level, str) else level
        tab = d.get("tab") if isinstance(tab, str) else tab
        ctab = None if tab is None else (ctypes.c_float * len(tab))(*[float(v) for v in tab])
        return self.lib.pislam_pnp_ransac_batch(self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["cam"]), ptr(d["xw"]),
                                                ptr(d["obs"]), ptr(d["counts"]), ptr(level), ctab,
                                                (0 if tab is None else len(tab)) if nlevels is None else nlevels, stride, B,
                                                ptr(o["best"]), ptr(o["score"]), ptr(o["ninliers"]), ptr(o["inlier"]),
                                                ptr(o["pose_out"]), ptr(o["status"]))

    def run(self, frames, counts, stride, prm, with_level=True):
        d = self.upload(self.pack(frames, counts, stride, with_level))
        o = self.sentinels(len(frames), stride)
        assert self.call(prm, d, stride, len(frames), o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_frames(got, want, ns, what=""):
    """Every output word of every frame, and the sentinels at and beyond n."""
    for b, (w, n) in enumerate(zip(want, ns)):
        tag = "%s frame %d" % (what, b)
        assert int(got["status"][b]) == w["status"], (tag, int(got["status"][b]), w["status"])
        assert int(got["best"][b]) == w["best"], (tag, int(got["best"][b]), w["best"])
        assert int(got["score"][b]) == w["score"] and int(got["ninliers"][b]) == w["ninliers"], tag
        assert got["pose_out"][b].view(np.uint32).tolist() == w["pose"].view(np.uint32).tolist(), tag
        assert (got["inlier"][b, :n] == w["inlier"]).all(), tag
        assert (got["inlier"][b, n:] == SENT8).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("with_level", [True, False], ids=["levels", "no_levels"])
@pytest.mark.parametrize("hypotheses", PIN_HYPOTHESES)
def test_pnp_pins(gpu_ctx, hypotheses, with_level):
    cases = pin_frames()
    frames = [pin_frame(k, True) for k in range(len(cases))]
    got = Device(gpu_ctx).run(frames, [c for _, _, c in cases], PIN_STRIDE, (hypotheses, PIN_SEED, PIN_MIN), with_level)
    want = pin_reference(hypotheses, with_level)
    assert_frames(got, want, [len(f["obs"]) for f in frames], "h%d" % hypotheses)


TRIP_HYPOTHESES, TRIP_NS = 65, (512, 513)


@functools.lru_cache(maxsize=None)
def second_trip_case():
    """Frames of 512 and 513 observations with levels: a workgroup scores 64 x 8 waves = 512 per trip, so the 513th is
    the scoring and the mask loop's second trip.  (frames, the restated results)."""
    big = scene(27, n=TRIP_NS[-1], outliers=0.3, levels=True)[0]
    frames = [sub(big, n) for n in TRIP_NS]
    return frames, [ref_frame(fr, b, TRIP_HYPOTHESES, PIN_SEED, PIN_MIN) for b, fr in enumerate(frames)]


def test_second_trip_case_has_models():
    for w in second_trip_case()[1]:
        assert w["best"] >= 0 and w["status"] & 255 == 0 and w["ninliers"] > 200
    assert second_trip_case()[1][1]["inlier"][512] == 1                       # the 513th is an inlier of its frame


@pytest.mark.gpu
def test_pnp_second_trip_of_the_item_loops(gpu_ctx):
    frames, want = second_trip_case()
    got = Device(gpu_ctx).run(frames, list(TRIP_NS), TRIP_NS[-1], (TRIP_HYPOTHESES, PIN_SEED, PIN_MIN))
    assert_frames(got, want, list(TRIP_NS), "second trip")


@pytest.mark.gpu
def test_pnp_seed_and_determinism(gpu_ctx):
    d = Device(gpu_ctx)
    fr = behaviour_scenes()[0][0]
    a = d.run([fr], [300], 300, (200, 1, 10))
    b = d.run([fr], [300], 300, (200, 1, 10))
    c = d.run([fr], [300], 300, (200, 2, 10))
    for k in OUT_NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"][0] >= 0 and c["best"][0] >= 0 and a["best"][0] != c["best"][0]
    assert_frames(a, [ref_frame(fr, 0, 200, 1)], [300], "seed 1")


@pytest.mark.gpu
def test_pnp_chain_into_pose_refine(gpu_ctx):
    """pose_out is the pose call's pose_in: on the behaviour scenes the refined mask holds no displaced observation and
    equals the mask the pose call reaches from the ground-truth pose."""
    from pislam_amd.frontend import pnpRansacBatch, poseRefineBatch
    d = Device(gpu_ctx)
    scenes = behaviour_scenes()
    h = d.pack([s[0] for s in scenes], [300] * 3, 300, False)
    dev = d.upload(h)
    best, score, ninl, inl, pose, status = pnpRansacBatch(dev["cam"], dev["xw"], dev["obs"], dev["counts"], hypotheses=200,
                                                          seed=7, ctx=gpu_ctx)
    truth = d.up(np.stack([np.concatenate([R.reshape(-1), tt]) for _, (R, tt), _ in scenes]).astype(F32))
    out = poseRefineBatch(pose, dev["cam"], dev["xw"], dev["obs"], dev["counts"], ctx=gpu_ctx)
    ref = poseRefineBatch(truth, dev["cam"], dev["xw"], dev["obs"], dev["counts"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert (status.cpu().numpy() & 255 == 0).all()
    assert (out[4].cpu().numpy() & 255 == 0).all() and (ref[4].cpu().numpy() & 255 == 0).all()
    m, mr = out[1].cpu().numpy().astype(bool), ref[1].cpu().numpy().astype(bool)
    for b, (_, _, good) in enumerate(scenes):
        assert not (m[b] & ~good).any() and m[b].sum() >= 0.9 * good.sum()
        assert (m[b] == mr[b]).all(), b


@pytest.mark.gpu
def test_pnp_invalid_arguments_write_nothing(gpu_ctx):
    d = Device(gpu_ctx)
    t = d.torch
    B, stride = 2, 64
    frames = [scene(41, n=64, levels=True)[0], scene(42, n=64, levels=True)[0]]
    h = d.pack(frames, [64, 64], stride)
    dev = d.upload(h)
    o = d.sentinels(B, stride)
    good = (8, 0, 10)
    for prm in ((0, 0, 10), (1025, 0, 10), (-1, 0, 10), (8, 0, 3), (8, 0, 16385), (8, 0, -1), None):
        assert d.call(prm, dev, stride, B, o) == -1, prm
    assert d.call(good, dev, 0, B, o) == -1
    assert d.call(good, dev, MAX_STRIDE + 1, B, o) == -1
    assert d.call(good, dev, stride, -1, o) == -1
    # the level table: missing, empty, too long, an entry that is not finite and positive
    assert d.call(good, dev, stride, B, o, tab=None) == -1
    assert d.call(good, dev, stride, B, o, nlevels=0) == -1
    assert d.call(good, dev, stride, B, o, tab=[1.0] * 17) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert d.call(good, dev, stride, B, o, tab=[1.0, bad, 1.0]) == -1, bad
    host = np.zeros(B * stride * 3, np.int32)
    for name in ("cam", "xw", "obs", "counts") + OUT_NAMES:
        for repl in (None, host):                                         # NULL, then a host pointer
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, stride, B, outs) == -1, name
    assert d.call(good, dev, stride, B, o, level=host.view(np.uint8)) == -1
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, dev, stride, B, dict(o, ninliers=dev["counts"])) == -1
    assert d.call(good, dev, stride, B, dict(o, inlier=dev["obs"].view(t.uint8))) == -1
    assert d.call(good, dev, stride, B, dict(o, inlier=dev["level"])) == -1
    assert d.call(good, dev, stride, B, dict(o, pose_out=dev["cam"])) == -1
    assert d.call(good, dev, stride, B, dict(o, status=o["best"])) == -1
    assert d.call(good, dev, stride, B, dict(o, score=o["pose_out"].view(t.int32).view(-1)[3:])) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        a = v.cpu().numpy()
        assert (a == SENT8).all() if k == "inlier" else (a.view(np.uint8) == 0x5A).all(), k
    for k in ("cam", "xw", "obs", "counts", "level"):
        assert dev[k].cpu().numpy().tobytes() == h[k].tobytes()
    # batch 0 is a no-op after the checks: the pointers are not looked at
    assert d.lib.pislam_pnp_ransac_batch(gpu_ctx.h, ctypes.byref(d.capi.PnpParams(*good)), None, None, None, None, None,
                                         None, 0, stride, 0, None, None, None, None, None, None) == 0
    # level may be NULL, and then the table is not looked at
    assert d.call(good, dev, stride, B, o, level=None, tab=None) == 0
    gpu_ctx.synchronize()
    assert (o["best"].cpu().numpy() >= 0).all()


@pytest.mark.gpu
def test_pnp_graph_replay_equals_eager(gpu_ctx):
    """No workspace, no host round trip: the call is captured on a side stream (one stream, no parallel branches) of a
    fresh context without a warm-up call, and every replay writes what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import pnpRansacBatch
    d = Device(gpu_ctx)
    frames = [scene(51, n=100, levels=True)[0], scene(52, n=64, levels=True)[0]]
    h = d.pack(frames, [100, 64], 100)
    dev = d.upload(h)
    args = (dev["cam"], dev["xw"], dev["obs"], dev["counts"])
    kw = dict(level=dev["level"], inv_sigma2=h["tab"], hypotheses=65, seed=9)
    eager = [x.cpu().numpy().copy() for x in pnpRansacBatch(*args, ctx=gpu_ctx, **kw, **d.sentinels(2, 100))]
    assert_frames(dict(zip(OUT_NAMES, eager)), [ref_frame(f, b, 65, 9) for b, f in enumerate(frames)], [100, 64], "frontend")
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        o = d.sentinels(2, 100)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            pnpRansacBatch(*args, ctx=ctx, **kw, **o)
        for _ in range(2):
            for k, x in o.items():
                x.view(t.uint8).fill_(SENT8 if k == "inlier" else 0x5A)
            g.replay()
            side.synchronize()
            for a, k in zip(eager, OUT_NAMES):
                assert a.tobytes() == o[k].cpu().numpy().tobytes(), k
        ctx.close()


@pytest.mark.gpu
def test_pnp_grid_passes(gpu_ctx):
    """The grid is capped at 1024 workgroups: 2051 frames take three passes.  Frames 0, 1023, 1024, 2047, 2048 and 2050
    hold 12 good observations, the others 0..3 (no model)."""
    B, stride, hyp, seed = 2051, 12, 3, 4
    live = (0, 1023, 1024, 2047, 2048, 2050)
    rng = np.random.default_rng(8)
    small = scene(80, n=12, outliers=0.0)[0]
    counts = rng.integers(0, 4, B)
    frames = []
    for b in range(B):
        if b in live:
            frames.append(scene(81 + live.index(b), n=12, outliers=0.0)[0])
            counts[b] = 12
        else:
            frames.append(sub(small, int(counts[b])))
    got = Device(gpu_ctx).run(frames, counts.tolist(), stride, (hyp, seed, 10), False)
    want = [ref_frame(f, b, hyp, seed) if b in live else ref_result(f, None, hyp, 10) for b, f in enumerate(frames)]
    assert_frames(got, want, [len(f["obs"]) for f in frames], "grid passes")
    assert [b for b in range(B) if want[b]["best"] >= 0] == list(live)


@pytest.mark.gpu
def test_pnp_offsets_beyond_4_gib(gpu_ctx):
    """stride 16384 and 21848 frames: the points and observations of the last two frames begin beyond 2^32 bytes (each
    array allocated in one piece, uninitialised: with a count of 0 a frame's observations are never read).  Frames 1,
    21846 and 21847 hold 12 observations."""
    d = Device(gpu_ctx)
    t = d.torch
    B, stride = 21848, MAX_STRIDE
    free, _ = t.cuda.mem_get_info()
    if free < 3 * (B * stride * 12):
        pytest.skip("two buffers above 4 GiB and the mask do not fit the free device memory")
    live = (1, B - 2, B - 1)
    assert live[1] * stride * 12 > 1 << 32
    xw = t.empty((B, stride, 3), dtype=t.float32, device="cuda")
    obs = t.empty((B, stride, 3), dtype=t.int32, device="cuda")
    counts = t.zeros((B,), dtype=t.int32, device="cuda")
    o = d.sentinels(B, 1)
    o["inlier"] = t.empty((B, stride), dtype=t.uint8, device="cuda")
    frames = [scene(91 + i, n=12, outliers=0.0)[0] for i in range(3)]
    cam = d.up(np.tile(CAM, (B, 1)))
    for fr, b in zip(frames, live):
        xw[b, :12], obs[b, :12], counts[b] = d.up(fr["xw"]), d.up(fr["obs"].astype(np.int32)), 12
        o["inlier"][b, :16] = SENT8
    dev = dict(cam=cam, xw=xw, obs=obs, counts=counts, level=None, tab=None)
    assert d.call((5, 3, 10), dev, stride, B, o) == 0
    gpu_ctx.synchronize()
    best, status = o["best"].cpu().numpy(), o["status"].cpu().numpy()
    assert (np.delete(best, live) == -1).all() and (np.delete(status, live) == 2).all()
    assert not np.delete(o["pose_out"].cpu().numpy(), live, 0).any()
    for fr, b in zip(frames, live):
        w = ref_frame(fr, b, 5, 3)
        got = {k: v[b:b + 1].cpu().numpy() for k, v in o.items()}
        got["inlier"] = got["inlier"][:, :16]
        assert w["best"] >= 0
        assert_frames(got, [w], [12], "frame %d" % b)
