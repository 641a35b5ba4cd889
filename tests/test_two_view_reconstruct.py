"""pislam_two_view_reconstruct_batch and pislam_two_view_decompose: from a verified two-view model to the relative pose
and the first map points.

The expectation is a numpy restatement of the contract (the comment in include/pislam_hip.h), independent of the
library: float32 arrays with one operation per rounding for the per-match work, Python integers for the counts and the
choice.  The host probe (tools/probes/recon_host_check.cpp, the library's own arithmetic header under the host
compiler) and the library on the GPU must agree with it on every output word.  The host helper is stated to a tolerance
and is checked against float64 numpy."""
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
COUNT_INVALID = 0xFFFFFFFF
COORD_MAX = 1 << 20
MAX_STRIDE = 16384
SENT8, SENT32 = 0xA5, 0x5A5A5A5A
RC_FIELDS = ["ncand", "sigma_q8", "cos_parallax", "cos_point", "min_good", "min_good_pct", "similar_pct", "parallax_rank"]
COS_1DEG = F32(np.cos(np.radians(1.0)))
# sigma_q8, cos_parallax, cos_point, min_good, min_good_pct, similar_pct, parallax_rank
DEFAULT = (256, COS_1DEG, F32(0.99998), 50, 90, 70, 51)
LOOSE = (512, F32(0.9999), F32(0.999999), 1, 0, 100, 1)
OUT_NAMES = ("best", "status", "ngood", "npar", "pose_out", "xw", "point")


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_eval(c, cam, q1, q2, sigma_q8, cos_parallax, cos_point):
    """One candidate on an array of matches, one float32 operation at a time.  c: float32 [..., 12] and cam: float32
    [..., 4], both broadcast against the matches q1, q2: integers [..., 2].  Returns good, parallax, point (bool) and
    X [..., 3], and the intermediate e1, e2, cs for the tests that build cases on a boundary."""
    one, half, k256 = F32(1.0), F32(0.5), F32(1.0 / 256.0)
    cos_parallax, cos_point = F32(cos_parallax), F32(cos_point)
    c = np.asarray(c, F32)
    cam = np.asarray(cam, F32)
    r = [c[..., k] for k in range(9)]
    t0, t1, t2 = c[..., 9], c[..., 10], c[..., 11]
    fx, fy, cx, cy = (cam[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        ifx, ify = one / fx, one / fy
        sg = F32(sigma_q8) * k256
        th2 = (sg * sg) * F32(4.0)
        px = lambda q: np.clip(np.asarray(q, np.int64), -COORD_MAX, COORD_MAX).astype(F32) * k256
        u1, v1, u2, v2 = px(q1[..., 0]), px(q1[..., 1]), px(q2[..., 0]), px(q2[..., 1])
        x1, y1, x2, y2 = (u1 - cx) * ifx, (v1 - cy) * ify, (u2 - cx) * ifx, (v2 - cy) * ify
        bb = (x2 * x2 + y2 * y2) + one
        a0 = (r[0] * x1 + r[1] * y1) + r[2]
        a1 = (r[3] * x1 + r[4] * y1) + r[5]
        a2 = (r[6] * x1 + r[7] * y1) + r[8]
        n0, n1, n2 = a1 - a2 * y2, a2 * x2 - a0, a0 * y2 - a1 * x2
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        p0, p1, p2 = y2 * t2 - t1, t0 - x2 * t2, x2 * t1 - y2 * t0
        s0, s1, s2 = a1 * t2 - a2 * t1, a2 * t0 - a0 * t2, a0 * t1 - a1 * t0
        z1 = ((p0 * n0 + p1 * n1) + p2 * n2) / nn
        z2 = ((s0 * n0 + s1 * n1) + s2 * n2) / nn
        g0, g1, g2 = z2 * x2 - t0, z2 * y2 - t1, z2 - t2
        h0 = (r[0] * g0 + r[3] * g1) + r[6] * g2
        h1 = (r[1] * g0 + r[4] * g1) + r[7] * g2
        h2 = (r[2] * g0 + r[5] * g1) + r[8] * g2
        X0, X1, X2 = (z1 * x1 + h0) * half, (z1 * y1 + h1) * half, (z1 + h2) * half
        Y0 = ((r[0] * X0 + r[1] * X1) + r[2] * X2) + t0
        Y1 = ((r[3] * X0 + r[4] * X1) + r[5] * X2) + t1
        Y2 = ((r[6] * X0 + r[7] * X1) + r[8] * X2) + t2
        cs = ((a0 * x2 + a1 * y2) + a2) / np.sqrt(((a0 * a0 + a1 * a1) + a2 * a2) * bb)
        i1 = one / X2
        eu, ev = u1 - (fx * (X0 * i1) + cx), v1 - (fy * (X1 * i1) + cy)
        e1 = eu * eu + ev * ev
        i2 = one / Y2
        eu, ev = u2 - (fx * (Y0 * i2) + cx), v2 - (fy * (Y1 * i2) + cy)
        e2 = eu * eu + ev * ev
        for a in (X0, X1, X2, Y0, Y1, Y2, cs, e1, e2):
            assert a.dtype == F32
        fin = np.isfinite(X0) & np.isfinite(X1) & np.isfinite(X2) & np.isfinite(Y0) & np.isfinite(Y1) & np.isfinite(Y2)
        is_point = cs < cos_point
        good = fin & ~(((X2 <= 0) | (Y2 <= 0)) & is_point) & (e1 <= th2) & (e2 <= th2)
        good = good & np.isfinite(c).all(-1)
        return dict(good=good, par=good & (cs < cos_parallax), point=good & is_point,
                    X=np.stack(np.broadcast_arrays(X0, X1, X2), -1), e1=e1, e2=e2, cs=cs, th2=th2)


def ref_choose(G, P, ncand, N, cam_ok, prm):
    _, _, _, min_good, min_good_pct, similar_pct, parallax_rank = prm
    G, P = [int(v) for v in G[:ncand]], [int(v) for v in P[:ncand]]
    gmax = max(G)
    cb = G.index(gmax)
    g2 = max([G[c] for c in range(ncand) if c != cb], default=0)
    if N == 0 or not cam_ok:
        return 4, cb
    if gmax < min_good or 100 * gmax < min_good_pct * N:
        return 1, cb
    if 100 * g2 >= similar_pct * gmax:
        return 2, cb
    if P[cb] < min(parallax_rank, gmax):
        return 3, cb
    return 0, cb


def clamp_count(count, stride):
    return 0 if count == COUNT_INVALID else min(int(count), stride)


def ref_batch(q1, q2, counts, mask, cam, cand, prm):
    """The whole call.  q1, q2: integers [B][S][2]; counts: [B] (as unsigned); mask: [B][S] or None; cam: float32
    [B][4]; cand: float32 [B][ncand][12].  Entries at and beyond n hold the sentinels."""
    q1, q2 = np.asarray(q1, np.int64), np.asarray(q2, np.int64)
    cam, cand = np.asarray(cam, F32), np.asarray(cand, F32)
    B, S = q1.shape[:2]
    ncand = cand.shape[1]
    n = np.array([clamp_count(int(c) & 0xFFFFFFFF, S) for c in counts])
    used = np.arange(S)[None, :] < n[:, None]
    if mask is not None:
        used = used & (np.asarray(mask) != 0)
    cam_ok = np.isfinite(cam).all(1) & (cam[:, 0] != 0) & (cam[:, 1] != 0)
    ev = [ref_eval(cand[:, c:c + 1, :], cam[:, None, :], q1, q2, prm[0], prm[1], prm[2]) for c in range(ncand)]
    out = dict(best=np.zeros(B, np.int32), status=np.zeros(B, np.uint32), ngood=np.zeros((B, 8), np.uint32),
               npar=np.zeros((B, 8), np.uint32), pose_out=np.zeros((B, 12), F32),
               xw=np.full((B, S, 3), SENT32, np.uint32).view(F32), point=np.full((B, S), SENT8, np.uint8), n=n)
    for b in range(B):
        ok = used[b] & bool(cam_ok[b])
        G = [int((e["good"][b] & ok).sum()) for e in ev]
        P = [int((e["par"][b] & ok).sum()) for e in ev]
        code, cb = ref_choose(G, P, ncand, int(used[b].sum()), bool(cam_ok[b]), prm)
        out["status"][b], out["best"][b] = code | cb << 8, cb if code == 0 else -1
        if code != 4:
            out["ngood"][b, :ncand], out["npar"][b, :ncand] = G, P
        out["xw"][b, :n[b]], out["point"][b, :n[b]] = 0, 0
        if code == 0:
            out["pose_out"][b] = cand[b, cb]
            pt = ev[cb]["point"][b] & ok
            out["xw"][b][pt], out["point"][b][pt] = ev[cb]["X"][b][pt], 1
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------
CAM = np.array([500, 500, 320, 240], F32)


def rodrigues(r):
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(X, cam):
    cam = np.asarray(cam, np.float64)
    u, v = cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]
    return np.rint(np.stack([u, v], 1) * 256).astype(np.int64)


def scene(seed, n, depth=(4.0, 8.0), rot_deg=6.0, baseline=0.5, far=0, cam=CAM):
    """n points seen from two cameras: X2 = R X1 + t, a rotation of rot_deg about a random axis, t = (-baseline, 0, 0)
    (camera 2 sits `baseline` along x), both under the camera `cam` (fx, fy, cx, cy).  The last `far` points lie 2000 to
    4000 units away: no parallax."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    R, t = rodrigues(axis / np.linalg.norm(axis) * np.radians(rot_deg)), np.array([-baseline, 0.0, 0.0])
    z = rng.uniform(depth[0], depth[1], n)
    z[n - far:] = rng.uniform(2000, 4000, far)
    X1 = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
    X2 = X1 @ R.T + t
    return dict(q1=project(X1, cam), q2=project(X2, cam), R=R, t=t, X1=X1)


def motion(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(F32)


def four_motions(R, t):
    """(R, t), (R2, t), (R, -t), (R2, -t) with t of unit length and R2 the twisted rotation (half a turn about t)."""
    tu = t / np.linalg.norm(t)
    R2 = (2 * np.outer(tu, tu) - np.eye(3)) @ R
    return np.stack([motion(R, tu), motion(R2, tu), motion(R, -tu), motion(R2, -tu)])


def eight_motions(sc, seed, first=0):
    """Eight candidates of a scene: the four motions of its essential matrix rolled so that the truth sits at `first`,
    a rotation 3 degrees off, no rotation, a translation along z, and one with a NaN entry."""
    rng = np.random.default_rng(1000 + seed)
    four = np.roll(four_motions(sc["R"], sc["t"]), first, 0)
    tu = sc["t"] / np.linalg.norm(sc["t"])
    off = rodrigues(rng.normal(size=3) / np.sqrt(3) * np.radians(3.0)) @ sc["R"]
    bad = motion(sc["R"], tu)
    bad[4] = np.nan
    return np.concatenate([four, [motion(off, tu), motion(np.eye(3), tu), motion(sc["R"], [0, 0, 1]), bad]])


def spoil(sc, idx):
    """Moves image 2 of the matches idx 20 pixels up: good under no candidate."""
    q2 = sc["q2"].copy()
    q2[idx, 1] -= 20 * 256
    return dict(sc, q2=q2)


# ---- the pin cases ----------------------------------------------------------------------------------------------------
PIN_STRIDE = 1003                                # not a multiple of 4
HAND_CAM = np.array([256, 256, 0, 0], F32)      # x = u / 256: the hand check's numbers are exact
HAND = motion(np.eye(3), [-1, 0, 0])


SKEW = motion(np.eye(3), [-1, 0, 0.25])           # depth differs between the frames, so e1 moves with the disparity


def boundary_match(prm):
    """Matches under SKEW around one whose e1 equals th2 exactly (and e2 <= th2), found by walking image 2's Q8
    coordinates: the row sets e1 to about (row / 512)^2, the column moves it by a few units in the last place."""
    c = 4 * prm[0]
    rows, cols = np.meshgrid(np.arange(c - 120, c + 40), np.arange(-200 * 256, -20 * 256, 64))
    q2 = np.stack([cols.ravel(), rows.ravel()], 1)
    e = ref_eval(SKEW, HAND_CAM, np.zeros_like(q2), q2, prm[0], prm[1], prm[2])
    close = q2[np.argsort(np.abs(e["e1"] - e["th2"]))[:40]]       # then every column around the 40 closest
    q2 = (close[:, None, :] + np.stack([np.arange(-64, 65), np.zeros(129, np.int64)], 1)[None]).reshape(-1, 2)
    e = ref_eval(SKEW, HAND_CAM, np.zeros_like(q2), q2, prm[0], prm[1], prm[2])
    hit = np.nonzero((e["e1"] == e["th2"]) & (e["e2"] <= e["th2"]))[0]
    assert len(hit), "no match with e1 == th2"
    k = q2[hit[0]]
    near = np.array([k + [0, d] for d in range(-8, 9)] + [k + [d, 0] for d in (-2, -1, 1, 2)])
    e = ref_eval(SKEW, HAND_CAM, np.zeros_like(near), near, prm[0], prm[1], prm[2])
    assert e["good"][8] and e["e1"][8] == e["th2"] and e["good"][0] and not e["good"][16]
    return np.zeros_like(near), near


@functools.lru_cache(maxsize=None)
def pin_batch(prm):
    """(names, q1, q2, counts, cam, cand8) at PIN_STRIDE: the shapes, then the arithmetic pins."""
    rng = np.random.default_rng(7)
    names, Q1, Q2, counts, cams, cands = [], [], [], [], [], []

    def add(name, q1, q2, cam, cand8, count=None):
        n = len(q1)
        a = rng.integers(-1 << 31, 1 << 31, (PIN_STRIDE, 2))
        b = rng.integers(-1 << 31, 1 << 31, (PIN_STRIDE, 2))
        m = min(n, PIN_STRIDE)
        a[:m], b[:m] = q1[:m], q2[:m]
        names.append(name), Q1.append(a), Q2.append(b), counts.append(n if count is None else count)
        cams.append(np.asarray(cam, F32)), cands.append(np.asarray(cand8, F32))

    for k, n in enumerate((0, 1, 50, 51, 255, 256, 257, 1000)):
        sc = scene(100 + n, n, far=n // 5)
        add("n%d" % n, sc["q1"], sc["q2"], CAM, eight_motions(sc, n, first=k % 4))
    sc = scene(31, PIN_STRIDE)
    add("count above stride", sc["q1"], sc["q2"], CAM, eight_motions(sc, 31), count=PIN_STRIDE + 7)
    add("count invalid", sc["q1"], sc["q2"], CAM, eight_motions(sc, 31), count=COUNT_INVALID)
    # the hand check, identical rays (nn = 0), a point behind camera 2 with a wide angle and with almost none
    hq1 = np.array([[0, 0], [77 * 256, 5 * 256], [0, 0], [10 * 256, 0], [3 * 256, 9 * 256]])
    hq2 = np.array([[-128 * 256, 0], [77 * 256, 5 * 256], [128 * 256, 0], [10 * 256 + 1, 0], [-61 * 256, 9 * 256]])
    hand8 = np.stack([HAND, motion(np.eye(3), [1, 0, 0]), motion(np.eye(3), [np.inf, 0, 0])] +
                     [motion(rodrigues(rng.normal(size=3) * 0.1), [0, 1, 0]) for _ in range(5)])
    add("hand", hq1, hq2, HAND_CAM, hand8)
    bq1, bq2 = boundary_match(prm)
    add("e1 at th2", bq1, bq2, HAND_CAM, np.concatenate([[SKEW], hand8[:7]]))
    sc = scene(32, 120)
    nan_first = eight_motions(sc, 32)[[7, 0, 1, 2, 3, 4, 5, 6]]
    add("nan candidate first", sc["q1"], sc["q2"], CAM, nan_first)
    for name, cam in (("fx zero", [0, 500, 320, 240]), ("fy zero", [500, 0.0, 320, 240]), ("cam inf", [500, 500, np.inf, 240]),
                      ("cam nan", [500, 500, 320, np.nan])):
        add(name, sc["q1"], sc["q2"], cam, eight_motions(sc, 32))
    far1, far2 = sc["q1"].copy(), sc["q2"].copy()
    far1[::7] = [[1 << 25, -(1 << 25)]]
    far2[::5] = [[-(1 << 31), (1 << 31) - 1]]
    far1[3], far2[3] = [COORD_MAX + 1, COORD_MAX], [COORD_MAX, COORD_MAX + 1]
    add("beyond the clamp", far1, far2, CAM, eight_motions(sc, 32))
    mask = (rng.uniform(0, 1, (len(names), PIN_STRIDE)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (len(names), PIN_STRIDE)).astype(np.uint8)
    return names, np.stack(Q1), np.stack(Q2), np.array(counts, np.uint32), np.stack(cams), np.stack(cands), mask


@functools.lru_cache(maxsize=None)
def pin_reference(prm, ncand, with_mask):
    _, q1, q2, counts, cam, cand, mask = pin_batch(prm)
    return ref_batch(q1, q2, counts, mask if with_mask else None, cam, cand[:, :ncand], prm)


PIN_CASES = [(prm, ncand, with_mask) for prm in (DEFAULT, LOOSE) for ncand in (1, 4, 8) for with_mask in (False, True)]
PIN_IDS = ["%s_c%d_%s" % ("default" if p is DEFAULT else "loose", c, "mask" if m else "nomask") for p, c, m in PIN_CASES]


# ---- the choice pins: each threshold on its boundary and one off it -----------------------------------------------------
def choice_cases():
    """(name, scene, candidates, parameters, the counts and the code the construction intends).  Near points have
    parallax and are good under the truth alone; far points have none and are good under (R, t) and (R, -t) alike."""
    out = []
    d = dict(zip(RC_FIELDS[1:], DEFAULT))

    def prm(**kw):
        return tuple(dict(d, **kw)[k] for k in RC_FIELDS[1:])

    def case(name, n, far, spoiled, p, cand=None, want=None):
        sc = spoil(scene(500 + len(out), n, far=far), np.arange(spoiled))
        out.append((name, sc, four_motions(sc["R"], sc["t"]) if cand is None else cand(sc), p, want))

    case("90 per cent: 90 of 100", 100, 0, 10, prm(), want=dict(code=0, gmax=90))
    case("90 per cent: 89 of 100", 100, 0, 11, prm(), want=dict(code=1, gmax=89))
    case("min_good: 50", 50, 0, 0, prm(min_good_pct=0), want=dict(code=0, gmax=50))
    case("min_good: 49", 50, 0, 1, prm(min_good_pct=0), want=dict(code=1, gmax=49))
    case("two identical candidates", 100, 0, 0, prm(), cand=lambda sc: four_motions(sc["R"], sc["t"])[[0, 0, 1, 2]],
         want=dict(code=2, gmax=100, g2=100, cbest=0))
    case("similar: 100 g2 = 70 gmax", 100, 70, 0, prm(parallax_rank=30), want=dict(code=2, gmax=100, g2=70))
    case("similar: one lower", 100, 69, 0, prm(parallax_rank=30), want=dict(code=0, gmax=100, g2=69))
    case("parallax rank: 51", 100, 49, 0, prm(), want=dict(code=0, gmax=100, pbest=51))
    case("parallax rank: 50", 100, 50, 0, prm(), want=dict(code=3, gmax=100, pbest=50))
    case("gmax below the rank: all", 60, 0, 0, prm(parallax_rank=100), want=dict(code=0, gmax=60, pbest=60))
    case("gmax below the rank: one short", 60, 1, 0, prm(parallax_rank=100), want=dict(code=3, gmax=60, pbest=59))
    return out


@functools.lru_cache(maxsize=None)
def choice_reference():
    res = []
    for name, sc, cand, p, want in choice_cases():
        n = len(sc["q1"])
        r = ref_batch(sc["q1"][None], sc["q2"][None], [n], None, CAM[None], cand[None], p)
        G = sorted(r["ngood"][0, :4].tolist(), reverse=True)
        got = dict(code=int(r["status"][0]) & 255, cbest=int(r["status"][0]) >> 8, gmax=G[0], g2=G[1],
                   pbest=int(r["npar"][0, int(r["status"][0]) >> 8]))
        for k, v in want.items():
            assert got[k] == v, "the construction of %r misses %s: %r" % (name, k, got)
        res.append(r)
    return res


# ---- the sequence scene -------------------------------------------------------------------------------------------------
SEQ_B, SEQ_N = 64, 600


@functools.lru_cache(maxsize=None)
def sequence_scene():
    """64 pairs, fx = fy = 500, depth 4..8, baseline 0.5 along x, 6 degrees of rotation, 600 points, rounded to Q8; the
    candidates are twoViewCandidates' of the true F = inverse(K)' [t]x R inverse(K)."""
    from pislam_amd.frontend import twoViewCandidates
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1.0]])
    Ki = np.linalg.inv(K)
    scs = [scene(900 + b, SEQ_N) for b in range(SEQ_B)]
    Fs = []
    for sc in scs:
        t = sc["t"]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Fs.append(Ki.T @ tx @ sc["R"] @ Ki)
    cand = twoViewCandidates("F", np.stack(Fs), K)
    assert cand.shape == (SEQ_B, 4, 12) and cand.dtype == F32 and np.isfinite(cand).all()
    truth = []
    for b, sc in enumerate(scs):
        want = motion(sc["R"], sc["t"] / np.linalg.norm(sc["t"]))
        hit = [c for c in range(4) if np.abs(cand[b, c] - want).max() < 1e-6]
        assert len(hit) == 1
        truth.append(hit[0])
    return dict(q1=np.stack([s["q1"] for s in scs]), q2=np.stack([s["q2"] for s in scs]), cand=cand,
                cam=np.tile(CAM, (SEQ_B, 1)), truth=np.array(truth), z=np.stack([s["X1"][:, 2] for s in scs]))


def check_sequence(best, status, xw, point, s=None):
    """status 0, the true motion, every match a point, depths within 1e-3 of the truth (t has unit length and the
    baseline is 0.5, so the map is twice the scene).  The bound is derived, not measured: a Q8 rounding error of at most
    1/512 px over f = 500 against a ray angle of at least 0.06 rad is about 7e-5 relative for one image; 1e-3 leaves
    about 15 times that.  Largest error seen: 1.25e-4, on the restatement and on the library alike (they agree bit for
    bit): both images are rounded, and the smallest ray angle of the scene is nearer 0.05 rad.  `s` is another scene of
    sequence_scene()'s layout."""
    s = sequence_scene() if s is None else s
    assert (np.asarray(status) == (s["truth"] << 8)).all() and (np.asarray(best) == s["truth"]).all()
    assert (np.asarray(point) == 1).all()
    err = np.abs(np.asarray(xw)[:, :, 2].astype(np.float64) * 0.5 - s["z"]) / s["z"]
    print("largest relative depth error: %.3g" % err.max())
    assert err.max() < 1e-3


# ---- CPU: declarations, anchors, the probe ----------------------------------------------------------------------------
def test_reconstruct_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in ("pislam_two_view_reconstruct_batch", "pislam_two_view_decompose"):
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f + " is not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_reconstruct_params \{([^}]*)\} pislam_reconstruct_params;", code)
    assert m and re.findall(r"(?:int32_t|float)\s+(\w+)\s*;", m.group(1)) == RC_FIELDS
    assert code.index("pislam_two_view_denormalise") < code.index("pislam_two_view_reconstruct_batch") < code.index("pislam_pose_refine_batch")
    from pislam_amd import capi, frontend
    assert len(capi.SYMBOLS["pislam_two_view_reconstruct_batch"][1]) == 17
    assert len(capi.SYMBOLS["pislam_two_view_decompose"][1]) == 5
    assert [n for n, _ in capi.ReconstructParams._fields_] == RC_FIELDS and ctypes.sizeof(capi.ReconstructParams) == 32
    for f in ("twoViewCandidates", "twoViewReconstructBatch"):
        assert callable(getattr(frontend, f)), f
    lib = capi.load()
    assert hasattr(lib, "pislam_two_view_reconstruct_batch") and hasattr(lib, "pislam_two_view_decompose")
    for name in ("pislam_recon_kernels.h", "pislam_recon_math.h"):
        assert os.path.exists(os.path.join(ROOT, "pislam_amd", "csrc", name)), name


def test_ref_reconstruct_anchors():
    """The expectation itself, independent of the library: the header's hand check, and a scene under its truth."""
    e = ref_eval(HAND, HAND_CAM, np.array([0, 0]), np.array([-128 * 256, 0]), *DEFAULT[:3])
    assert e["X"].tolist() == [0.0, 0.0, 2.0] and e["good"] and e["par"] and e["point"] and e["e1"] == 0 and e["e2"] == 0
    # identical rays: nn = 0, nothing finite, not good
    e = ref_eval(HAND, HAND_CAM, np.array([5, 7]), np.array([5, 7]), *DEFAULT[:3])
    assert not np.isfinite(e["X"]).any() and not e["good"]
    # behind camera 2 with a wide angle: refused; with almost none (cs >= cos_point): kept, but no point
    e = ref_eval(HAND, HAND_CAM, np.array([0, 0]), np.array([128 * 256, 0]), *DEFAULT[:3])
    assert e["X"][2] < 0 and e["cs"] < DEFAULT[2] and not e["good"]
    e = ref_eval(HAND, HAND_CAM, np.array([10 * 256, 0]), np.array([10 * 256 + 1, 0]), *DEFAULT[:3])
    assert e["X"][2] < 0 and e["cs"] >= DEFAULT[2] and e["good"] and not e["point"] and not e["par"]
    sc = scene(3, 200)
    four = four_motions(sc["R"], sc["t"])
    r = ref_batch(sc["q1"][None], sc["q2"][None], [200], None, CAM[None], four[None], DEFAULT)
    assert r["status"][0] == 0 and r["best"][0] == 0 and r["ngood"][0].tolist() == [200, 0, 0, 0, 0, 0, 0, 0]
    assert r["npar"][0, 0] == 200 and (r["point"][0, :200] == 1).all() and (r["pose_out"][0] == four[0]).all()
    assert np.abs(r["xw"][0, :200] * 0.5 - sc["X1"]).max() < 1e-2
    # every code occurs in the pin and choice cases, and the choice cases are what they were built to be
    codes = {int(s) & 255 for p, c, m in PIN_CASES for s in pin_reference(p, c, m)["status"]}
    assert len(choice_reference()) == 11
    assert codes | {int(r["status"][0]) & 255 for r in choice_reference()} == {0, 1, 2, 3, 4}


def test_sequence_on_the_restatement():
    s = sequence_scene()
    r = ref_batch(s["q1"], s["q2"], [SEQ_N] * SEQ_B, None, s["cam"], s["cand"], DEFAULT)
    check_sequence(r["best"], r["status"], r["xw"], r["point"])


def hexf(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


def probe_line(q1, q2, n, mask, cam, cand, prm):
    head = "%d %d %s %s %d %d %d %d %d %d" % (len(cand), prm[0], hexf(prm[1]), hexf(prm[2]), prm[3], prm[4], prm[5], prm[6],
                                            int(mask is not None), n)
    m = np.zeros(n, np.int64) if mask is None else mask[:n]
    rows = ["%d %d %d %d %d" % (q1[i, 0], q1[i, 1], q2[i, 0], q2[i, 1], m[i]) for i in range(n)]
    return " ".join([head, hexf(cam), hexf(cand)] + rows)


def result_line(r, b):
    n = int(r["n"][b])
    pt = "".join(str(int(v)) for v in r["point"][b, :n]) or "-"
    words = [str(int(r["best"][b])), str(int(r["status"][b]))] + [str(int(v)) for v in r["ngood"][b]] + \
            [str(int(v)) for v in r["npar"][b]] + [hexf(r["pose_out"][b]), pt]
    return " ".join(words + ([hexf(r["xw"][b, :n])] if n else []))


def test_host_probe_against_the_restatement(tmp_path):
    """The library's own arithmetic header, compiled for the host with -ffp-contract=off, run serially: every output
    word of every pin and choice case."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "recon_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "pislam_amd", "csrc"),
                           os.path.join(ROOT, "tools", "probes", "recon_host_check.cpp"), "-o", exe])
    lines, want = [], []
    for prm, ncand, with_mask in PIN_CASES:
        _, q1, q2, counts, cam, cand, mask = pin_batch(prm)
        r = pin_reference(prm, ncand, with_mask)
        for b in range(len(q1)):
            lines.append(probe_line(q1[b], q2[b], int(r["n"][b]), mask[b] if with_mask else None, cam[b], cand[b, :ncand], prm))
            want.append(result_line(r, b))
    for (name, sc, cand, p, _), r in zip(choice_cases(), choice_reference()):
        lines.append(probe_line(sc["q1"], sc["q2"], len(sc["q1"]), None, CAM, cand, p))
        want.append(result_line(r, 0))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    got = subprocess.run([exe, str(cases)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "case %d: %s" % (k, lines[k][:80])


# ---- CPU: pislam_two_view_decompose ---------------------------------------------------------------------------------------
DEC_K = np.array([[500, 0, 320], [0, 480, 240], [0, 0, 1.0]])
DEC_CAM = np.array([500, 480, 320, 240], np.float64)


def decompose(model, m):
    from pislam_amd import capi
    lib = capi.load()
    dp = ctypes.POINTER(ctypes.c_double)
    m = np.ascontiguousarray(m, np.float64)
    out, k = (ctypes.c_float * 96)(*([7.0] * 96)), ctypes.c_int(-5)
    rc = lib.pislam_two_view_decompose(model, m.ctypes.data_as(dp), DEC_CAM.ctypes.data_as(dp), out, ctypes.byref(k))
    return rc, k.value, np.frombuffer(out, F32).reshape(8, 12).copy()


def np_candidates(model, m):
    """The same decomposition with numpy's SVD in float64: rows of 12."""
    Ki = np.linalg.inv(DEC_K)
    if model == 0:
        U, _, Vt = np.linalg.svd(DEC_K.T @ m @ DEC_K)
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
        R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
        R1, R2 = R1 * np.sign(np.linalg.det(R1)), R2 * np.sign(np.linalg.det(R2))
        return np.array([np.concatenate([R.reshape(9), s * t]) for s in (1, -1) for R in (R1, R2)])
    U, d, Vt = np.linalg.svd(Ki @ m @ DEC_K)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = d
    a1, a3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
    out = []
    for neg in (False, True):
        den = (d1 - d3 if neg else d1 + d3) * d2
        sn, cs = root / den, (d1 * d3 - d2 * d2 if neg else d2 * d2 + d1 * d3) / den
        for e1, e3 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            si = e1 * e3 * sn
            Rp = np.array([[cs, 0, si], [0, -1, 0], [si, 0, -cs]]) if neg else np.array([[cs, 0, -si], [0, 1, 0], [si, 0, cs]])
            t = U @ np.array([e1 * a1, 0, e3 * a3 if neg else -e3 * a3])
            out.append(np.concatenate([(s * U @ Rp @ Vt).reshape(9), t / np.linalg.norm(t)]))
    return np.array(out)


def matching(cands, R, t, tol=1e-6):
    """The indices of the candidates that are (R, t) and (R, -t), t of unit length."""
    tu = t / np.linalg.norm(t)
    plus = [k for k, c in enumerate(cands) if np.abs(c - np.concatenate([R.reshape(9), tu])).max() < tol]
    minus = [k for k, c in enumerate(cands) if np.abs(c - np.concatenate([R.reshape(9), -tu])).max() < tol]
    return plus, minus


@pytest.mark.parametrize("seed", range(6))
def test_decompose_on_synthetic_motions(seed):
    """F and H of a known motion: the candidates are rotations (the helper checks R'R - I and det R - 1 against 1e-12
    in double before it stores floats and returns no candidate otherwise; the floats are checked here to their own
    rounding), the true rotation comes with +t exactly once and with -t exactly once (the matrix fixes t up to its
    sign), these agree with numpy's SVD to 1e-6 (float32 rounding of entries of order 1 is 6e-8: 16 times that), and a
    rank-3 perturbation of 1e-6 of the essential matrix moves the answer by less than 1e-4."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    R = rodrigues(axis / np.linalg.norm(axis) * np.radians(rng.uniform(5, 20)))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    Ki = np.linalg.inv(DEC_K)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    G = rng.normal(size=(3, 3))
    scale = rng.uniform(0.1, 10) * (-1) ** seed
    F = Ki.T @ E @ Ki * scale
    Fp = Ki.T @ (E + 1e-6 * np.linalg.norm(E) * G / np.linalg.norm(G)) @ Ki * scale
    assert np.linalg.matrix_rank(DEC_K.T @ Fp @ DEC_K, tol=1e-9) == 3
    u = R.T @ t                                   # the plane's normal: 63 degrees off R' t, so n . t = 0.45
    w = np.cross(u, np.eye(3)[np.argmin(np.abs(u))])
    nrm = 0.5 * u + w / np.linalg.norm(w)
    nrm /= np.linalg.norm(nrm)
    assert abs(nrm @ t) > 0.05
    A = R + np.outer(t, nrm) / 1.5
    sv = np.linalg.svd(A)[1]
    assert sv[0] / sv[1] >= 1.05 and sv[1] / sv[2] >= 1.05, sv
    H = DEC_K @ A @ Ki * scale
    for model, m, k in ((0, F, 4), (1, H, 8)):
        rc, got_k, cand = decompose(model, m)
        assert rc == 0 and got_k == k
        assert (cand[k:] == 0).all()
        for c in cand[:k]:
            Rc = c[:9].astype(np.float64).reshape(3, 3)
            assert np.abs(Rc.T @ Rc - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(Rc) - 1) < 1e-6
            assert abs(np.linalg.norm(c[9:].astype(np.float64)) - 1) < 1e-6
        plus, minus = matching(cand[:k], R, t)
        assert len(plus) == 1 and len(minus) == 1, (model, plus, minus)
        ref = np_candidates(model, m)
        rp, rm = matching(ref, R, t, 1e-9)
        assert len(rp) == 1 and len(rm) == 1
        assert np.abs(cand[plus[0]] - ref[rp[0]]).max() < 1e-6 and np.abs(cand[minus[0]] - ref[rm[0]]).max() < 1e-6
        if model == 0:                            # ORB-SLAM's order: (R1, t), (R2, t), (R1, -t), (R2, -t)
            assert (cand[0, :9] == cand[2, :9]).all() and (cand[1, :9] == cand[3, :9]).all()
            assert (cand[0, 9:] == -cand[2, 9:]).all() and (cand[0, 9:] == cand[1, 9:]).all()
            rc, got_k, moved = decompose(0, Fp)
            assert rc == 0 and got_k == 4
            pp, pm = matching(moved[:4], R, t, 1e-4)
            assert len(pp) == 1 and len(pm) == 1
            assert np.abs(moved[pp[0]] - cand[plus[0]]).max() < 1e-4 and np.abs(moved[pp[0]] - cand[plus[0]]).max() > 0


def test_decompose_degenerate_and_invalid():
    from pislam_amd import capi
    from pislam_amd.frontend import twoViewCandidates
    lib = capi.load()
    R = rodrigues(np.array([0.1, -0.2, 0.05]))
    Ki = np.linalg.inv(DEC_K)
    rc, k, cand = decompose(1, DEC_K @ R @ Ki)                 # a pure rotation: d1 = d2 = d3
    assert rc == 0 and k == 0 and (cand == 0).all()
    rc, k, _ = decompose(0, np.zeros((3, 3)))
    assert rc == 0 and k == 0
    bad = DEC_K @ R @ Ki
    for v in (np.nan, np.inf):
        m = bad.copy()
        m[1, 2] = v
        assert decompose(0, m)[0] == -1 and decompose(1, m)[0] == -1
    dp, m = ctypes.POINTER(ctypes.c_double), np.ascontiguousarray(bad)
    cam, out, k = DEC_CAM.copy(), (ctypes.c_float * 96)(), ctypes.c_int(0)
    mp, cp = m.ctypes.data_as(dp), cam.ctypes.data_as(dp)
    assert lib.pislam_two_view_decompose(0, mp, cp, out, ctypes.byref(k)) == 0
    assert lib.pislam_two_view_decompose(2, mp, cp, out, ctypes.byref(k)) == -1
    assert lib.pislam_two_view_decompose(-1, mp, cp, out, ctypes.byref(k)) == -1
    assert lib.pislam_two_view_decompose(0, None, cp, out, ctypes.byref(k)) == -1
    assert lib.pislam_two_view_decompose(0, mp, None, out, ctypes.byref(k)) == -1
    assert lib.pislam_two_view_decompose(0, mp, cp, None, ctypes.byref(k)) == -1
    assert lib.pislam_two_view_decompose(0, mp, cp, out, None) == -1
    for i, v in ((0, 0.0), (1, 0.0), (2, np.nan), (3, np.inf)):
        c2 = DEC_CAM.copy()
        c2[i] = v
        assert lib.pislam_two_view_decompose(0, mp, c2.ctypes.data_as(dp), out, ctypes.byref(k)) == -1
    # the Python helper: a batch, K as a matrix or as four numbers, NaN rows for a degenerate matrix
    t = np.array([0.6, 0.0, 0.8])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = Ki.T @ tx @ R @ Ki
    one = twoViewCandidates(0, F, DEC_K)
    both = twoViewCandidates("F", np.stack([F, np.zeros((3, 3))]), DEC_CAM)
    assert one.shape == (4, 12) and one.dtype == F32 and both.shape == (2, 4, 12)
    assert (both[0] == one).all() and np.isnan(both[1]).all()
    assert len(matching(one, R, t)[0]) == 1
    assert np.isnan(twoViewCandidates("H", DEC_K @ R @ Ki, DEC_K)).all() and twoViewCandidates(1, bad, DEC_K).shape == (8, 12)
    with pytest.raises(ValueError):
        twoViewCandidates(2, F, DEC_K)
    with pytest.raises(ValueError):
        twoViewCandidates(0, F, np.zeros(5))


def test_reconstruct_argument_checks_without_a_device():
    """What is refused before a device is needed: a NULL context by the library, every parameter range and every shape
    by the Python interface (host tensors never reach the library)."""
    import torch
    from pislam_amd import capi
    from pislam_amd.frontend import twoViewReconstructBatch
    lib = capi.load()
    p = capi.ReconstructParams(4, *[v.item() if hasattr(v, "item") else v for v in DEFAULT])
    assert lib.pislam_two_view_reconstruct_batch(None, ctypes.byref(p), *([None] * 6), 8, 0, *([None] * 7)) == -1
    assert lib.pislam_two_view_reconstruct_batch(None, None, *([None] * 6), 8, 1, *([None] * 7)) == -1
    B, S = 2, 8
    a = dict(p1_q8=torch.zeros((B, S, 2), dtype=torch.int32), p2_q8=torch.zeros((B, S, 2), dtype=torch.int32),
             counts=torch.zeros(B, dtype=torch.int32), cam=torch.ones((B, 4)), cand=torch.zeros((B, 4, 12)))
    for kw in (dict(sigma_q8=0), dict(sigma_q8=4097), dict(min_parallax_deg=120.0), dict(min_parallax_deg=180.0),
               dict(min_parallax_deg=float("nan")), dict(cos_point=0.0), dict(cos_point=1.0001), dict(cos_point=float("nan")),
               dict(min_good=0), dict(min_good=16385), dict(min_good_pct=-1), dict(min_good_pct=101), dict(similar_pct=0),
               dict(similar_pct=101), dict(parallax_rank=0), dict(parallax_rank=16385),
               dict(mask=torch.zeros((B, S), dtype=torch.int32)), dict(mask=torch.zeros((B, S + 1), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            twoViewReconstructBatch(**a, **kw)
    for name, bad in (("p1_q8", a["p1_q8"].to(torch.int64)), ("p2_q8", a["p2_q8"][:, :4]), ("counts", a["counts"][:1]),
                      ("cam", torch.ones((B, 5))), ("cand", torch.zeros((B, 9, 12))), ("cand", torch.zeros((B, 0, 12))),
                      ("cand", torch.zeros((B, 4, 12), dtype=torch.float64)), ("p1_q8", torch.zeros((B, MAX_STRIDE + 1, 2), dtype=torch.int32)),
                      ("cand", torch.zeros((B, 4, 24))[:, :, ::2])):
        with pytest.raises(ValueError):
            twoViewReconstructBatch(**dict(a, **{name: bad}))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.capi, self.ctx, self.lib = torch, capi, ctx, ctx.lib

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def sentinels(self, B, stride):
        t = self.torch
        w = lambda *shape: t.full(shape, SENT32, dtype=t.int32, device="cuda")
        return dict(best=w(B), status=w(B), ngood=w(B, 8), npar=w(B, 8), pose_out=w(B, 12).view(t.float32),
                    xw=w(B, stride, 3).view(t.float32), point=t.full((B, stride), SENT8, dtype=t.uint8, device="cuda"))

    def upload(self, q1, q2, counts, mask, cam, cand):
        return dict(p1=self.up(np.asarray(q1).astype(np.int32)), p2=self.up(np.asarray(q2).astype(np.int32)),
                    counts=self.up(np.asarray(counts, np.uint32).view(np.int32)),
                    mask=None if mask is None else self.up(np.asarray(mask, np.uint8)),
                    cam=self.up(np.asarray(cam, F32)), cand=self.up(np.asarray(cand, F32)))

    def params(self, ncand, prm):
        return self.capi.ReconstructParams(ncand, *[v.item() if hasattr(v, "item") else v for v in prm])

    def call(self, p, d, stride, B, o):
        ptr = self.capi.ptr
        return self.lib.pislam_two_view_reconstruct_batch(
            self.ctx.h, None if p is None else ctypes.byref(p), ptr(d["p1"]), ptr(d["p2"]), ptr(d["counts"]), ptr(d["mask"]),
            ptr(d["cam"]), ptr(d["cand"]), stride, B, ptr(o["best"]), ptr(o["status"]), ptr(o["ngood"]), ptr(o["npar"]),
            ptr(o["pose_out"]), ptr(o["xw"]), ptr(o["point"]))

    def run(self, q1, q2, counts, mask, cam, cand, prm):
        B, stride, ncand = len(q1), np.asarray(q1).shape[1], np.asarray(cand).shape[1]
        d = self.upload(q1, q2, counts, mask, cam, cand)
        o = self.sentinels(B, stride)
        assert self.call(self.params(ncand, prm), d, stride, B, o) == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_same(got, want, what=""):
    """Every output word of every pair, and the sentinels at and beyond n."""
    for k in ("best", "status", "ngood", "npar"):
        bad = np.nonzero((got[k].astype(np.int64) & 0xFFFFFFFF) != (want[k].astype(np.int64) & 0xFFFFFFFF))[0]
        assert len(bad) == 0, (what, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    for k in ("pose_out", "xw"):
        g, w = got[k].view(np.uint32), want[k].view(np.uint32)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, (what, k, bad[:5])
    assert (got["point"] == want["point"]).all(), (what, "point")


@pytest.mark.gpu
@pytest.mark.parametrize("prm,ncand,with_mask", PIN_CASES, ids=PIN_IDS)
def test_reconstruct_pins(gpu_ctx, prm, ncand, with_mask):
    """n in {0, 1, 50, 51, 255, 256, 257, 1000}, a count above the stride, PISLAM_COUNT_INVALID, and the arithmetic
    pins, at a stride that is no multiple of 4, in one batch of 19 pairs."""
    _, q1, q2, counts, cam, cand, mask = pin_batch(prm)
    got = Device(gpu_ctx).run(q1, q2, counts, mask if with_mask else None, cam, cand[:, :ncand], prm)
    assert_same(got, pin_reference(prm, ncand, with_mask), PIN_IDS[PIN_CASES.index((prm, ncand, with_mask))])


@pytest.mark.gpu
def test_reconstruct_choice_pins(gpu_ctx):
    d = Device(gpu_ctx)
    for (name, sc, cand, p, _), want in zip(choice_cases(), choice_reference()):
        n = len(sc["q1"])
        got = d.run(sc["q1"][None], sc["q2"][None], [n], None, CAM[None], cand[None], p)
        assert_same(got, want, name)


@pytest.mark.gpu
def test_reconstruct_batch_of_three(gpu_ctx):
    scs = [scene(40 + b, 300, far=20 * b) for b in range(3)]
    q1, q2 = np.stack([s["q1"] for s in scs]), np.stack([s["q2"] for s in scs])
    cand = np.stack([eight_motions(s, b, first=b)[:4] for b, s in enumerate(scs)])
    counts, cam = [300, 17, 299], np.tile(CAM, (3, 1))
    want = ref_batch(q1, q2, counts, None, cam, cand, DEFAULT)
    assert want["status"].tolist() == [0, 1 | 1 << 8, 0 | 2 << 8]
    assert_same(Device(gpu_ctx).run(q1, q2, counts, None, cam, cand, DEFAULT), want, "batch 3")


@pytest.mark.gpu
def test_reconstruct_full_stride(gpu_ctx):
    """One pair at stride 16384 with a count above it: 64 matches per lane, eight candidates."""
    sc = scene(61, MAX_STRIDE, far=3000)
    cand = eight_motions(sc, 61, first=3)[None]
    rng = np.random.default_rng(61)
    mask = (rng.uniform(0, 1, (1, MAX_STRIDE)) < 0.9).astype(np.uint8)
    want = ref_batch(sc["q1"][None], sc["q2"][None], [20000], mask, CAM[None], cand, DEFAULT)
    assert want["status"][0] == 3 << 8 and want["ngood"][0, 3] > 14000 and want["point"][0].sum() > 11000
    assert_same(Device(gpu_ctx).run(sc["q1"][None], sc["q2"][None], [20000], mask, CAM[None], cand, DEFAULT), want, "stride 16384")


@pytest.mark.gpu
def test_reconstruct_grid_passes(gpu_ctx):
    """The grid is capped at 1024 workgroups: 2049 pairs take three passes.  Every pair has its own points, its own
    count (b mod 65) and the truth at its own place among the four candidates (b mod 4)."""
    B, S = 2049, 64
    sc = scene(71, B * S)
    q1, q2 = sc["q1"].reshape(B, S, 2), sc["q2"].reshape(B, S, 2)
    four = four_motions(sc["R"], sc["t"])
    cand = np.stack([np.roll(four, b % 4, 0) for b in range(B)])
    counts = np.arange(B) % 65
    prm = (256, COS_1DEG, F32(0.99998), 5, 90, 70, 6)
    want = ref_batch(q1, q2, counts, None, np.tile(CAM, (B, 1)), cand, prm)
    ok = counts >= 5
    assert (want["best"][ok] == (np.arange(B) % 4)[ok]).all() and (want["best"][~ok] == -1).all()
    assert_same(Device(gpu_ctx).run(q1, q2, counts, None, np.tile(CAM, (B, 1)), cand, prm), want, "grid passes")


@pytest.mark.gpu
def test_reconstruct_sequence_through_python(gpu_ctx):
    """twoViewCandidates -> twoViewReconstructBatch -> poseRefineBatch on the sequence scene: the true motion, a map
    within the derived depth bound, and a pose the refinement has nothing to add to: code 0 and every point an inlier."""
    import torch as t
    from pislam_amd.frontend import poseRefineBatch, twoViewReconstructBatch
    s = sequence_scene()
    d = Device(gpu_ctx)
    up = d.upload(s["q1"], s["q2"], [SEQ_N] * SEQ_B, None, s["cam"], s["cand"])
    best, status, ngood, npar, pose, xw, point = twoViewReconstructBatch(up["p1"], up["p2"], up["counts"], up["cam"],
                                                                         up["cand"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    check_sequence(best.cpu().numpy(), status.cpu().numpy(), xw.cpu().numpy(), point.cpu().numpy())
    want = ref_batch(s["q1"], s["q2"], [SEQ_N] * SEQ_B, None, s["cam"], s["cand"], DEFAULT)
    got = dict(zip(OUT_NAMES, (x.cpu().numpy() for x in (best, status, ngood, npar, pose, xw, point))))
    assert_same(got, want, "sequence")
    obs = t.cat([up["p2"], t.full((SEQ_B, SEQ_N, 1), -(1 << 31), dtype=t.int32, device="cuda")], 2).contiguous()
    cam5 = t.cat([up["cam"], t.zeros((SEQ_B, 1), device="cuda")], 1).contiguous()
    pose2, inlier, ninliers, cost, st = poseRefineBatch(pose, cam5, xw, obs, up["counts"], ctx=gpu_ctx)
    gpu_ctx.synchronize()
    assert (st.cpu().numpy() & 255 == 0).all()
    assert (ninliers.cpu().numpy() == point.cpu().numpy().sum(1)).all() and (ninliers.cpu().numpy() == SEQ_N).all()
    print("largest pose change in the refinement: %.3g" % float((pose2 - pose).abs().max()))


@pytest.mark.gpu
def test_reconstruct_graph_replay_equals_eager(gpu_ctx):
    """No workspace, no host round trip: captured on a side stream (one stream, no parallel branches) of a fresh
    context without a warm-up call, and both replays write what the eager call wrote."""
    import torch as t
    from pislam_amd.capi import Context
    from pislam_amd.frontend import twoViewReconstructBatch
    d = Device(gpu_ctx)
    scs = [scene(80 + b, 200, far=30) for b in range(2)]
    cand = np.stack([eight_motions(s, b, first=1 + b) for b, s in enumerate(scs)])
    rng = np.random.default_rng(80)
    up = d.upload(np.stack([s["q1"] for s in scs]), np.stack([s["q2"] for s in scs]), [200, 150],
                  (rng.uniform(0, 1, (2, 200)) < 0.8).astype(np.uint8), np.tile(CAM, (2, 1)), cand)
    args = (up["p1"], up["p2"], up["counts"], up["cam"], up["cand"])
    eager = [x.cpu().numpy().copy() for x in twoViewReconstructBatch(*args, mask=up["mask"], ctx=gpu_ctx, **d.sentinels(2, 200))]
    assert eager[0].tolist() == [1, 2]
    gpu_ctx.synchronize()
    t.cuda.synchronize()
    side = t.cuda.Stream(t.device("cuda:0"))
    with t.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        o = d.sentinels(2, 200)
        side.synchronize()
        g = t.cuda.CUDAGraph()
        with t.cuda.graph(g, stream=side):
            twoViewReconstructBatch(*args, mask=up["mask"], ctx=ctx, **o)
        for _ in range(2):
            for k, x in o.items():
                x.view(t.uint8).fill_(SENT8 if k == "point" else 0x5A)
            g.replay()
            side.synchronize()
            for a, b in zip(eager, o.values()):
                assert a.tobytes() == b.cpu().numpy().tobytes()
        ctx.close()


@pytest.mark.gpu
def test_reconstruct_invalid_arguments_write_nothing(gpu_ctx):
    d = Device(gpu_ctx)
    t = d.torch
    B, stride = 2, 64
    scs = [scene(90 + b, stride) for b in range(B)]
    q1, q2 = np.stack([s["q1"] for s in scs]), np.stack([s["q2"] for s in scs])
    cand = np.stack([four_motions(s["R"], s["t"]) for s in scs])
    dev = d.upload(q1, q2, [stride] * B, np.ones((B, stride), np.uint8), np.tile(CAM, (B, 1)), cand)
    o = d.sentinels(B, stride)
    good = d.params(4, DEFAULT)
    fields = dict(zip(RC_FIELDS, [4] + [v.item() if hasattr(v, "item") else v for v in DEFAULT]))
    for name, bad in (("ncand", 0), ("ncand", 9), ("sigma_q8", 0), ("sigma_q8", 4097), ("cos_parallax", 0.0),
                      ("cos_parallax", 1.5), ("cos_parallax", float("nan")), ("cos_point", 0.0), ("cos_point", -1.0),
                      ("cos_point", 1.0000001192092896), ("cos_point", float("nan")), ("min_good", 0), ("min_good", 16385),
                      ("min_good_pct", -1), ("min_good_pct", 101), ("similar_pct", 0), ("similar_pct", 101),
                      ("parallax_rank", 0), ("parallax_rank", 16385)):
        p = d.capi.ReconstructParams(*[dict(fields, **{name: bad})[k] for k in RC_FIELDS])
        assert d.call(p, dev, stride, B, o) == -1, (name, bad)
    assert d.call(None, dev, stride, B, o) == -1
    assert d.call(good, dev, 0, B, o) == -1
    assert d.call(good, dev, MAX_STRIDE + 1, B, o) == -1
    assert d.call(good, dev, stride, -1, o) == -1
    host = np.zeros(B * stride * 3, np.int32)
    for name in ("p1", "p2", "counts", "cam", "cand", "best", "status", "ngood", "npar", "pose_out", "xw", "point"):
        for repl in (None, host):                                         # NULL, then a host pointer
            ins, outs = dict(dev), dict(o)
            (ins if name in ins else outs)[name] = repl
            assert d.call(good, ins, stride, B, outs) == -1, name
    assert d.call(good, dict(dev, mask=host.view(np.uint8)), stride, B, o) == -1
    # overlaps: an output on an input, two outputs on each other (partly, too)
    assert d.call(good, dev, stride, B, dict(o, status=dev["counts"])) == -1
    assert d.call(good, dev, stride, B, dict(o, point=dev["mask"])) == -1
    assert d.call(good, dev, stride, B, dict(o, point=dev["p2"].view(t.uint8))) == -1
    assert d.call(good, dev, stride, B, dict(o, pose_out=dev["cand"])) == -1
    assert d.call(good, dev, stride, B, dict(o, pose_out=dev["cam"])) == -1
    assert d.call(good, dev, stride, B, dict(o, xw=dev["p1"].view(t.float32))) == -1
    assert d.call(good, dev, stride, B, dict(o, best=o["status"])) == -1
    assert d.call(good, dev, stride, B, dict(o, npar=o["ngood"].view(-1)[8:])) == -1
    assert d.call(good, dev, stride, B, dict(o, point=o["xw"].view(t.uint8).view(-1)[100:])) == -1
    gpu_ctx.synchronize()
    for k, v in o.items():
        a = v.cpu().numpy()
        assert (a == SENT8).all() if k == "point" else (a.view(np.uint8) == 0x5A).all(), k
    # batch 0 is a no-op after the checks: the pointers are not looked at
    assert d.lib.pislam_two_view_reconstruct_batch(gpu_ctx.h, ctypes.byref(good), *([None] * 6), stride, 0, *([None] * 7)) == 0
    # mask NULL is allowed, and the all-ones mask changes nothing
    want = ref_batch(q1, q2, [stride] * B, None, np.tile(CAM, (B, 1)), cand, DEFAULT)
    for m in (None, dev["mask"]):
        o = d.sentinels(B, stride)
        assert d.call(good, dict(dev, mask=m), stride, B, o) == 0
        gpu_ctx.synchronize()
        assert_same({k: v.cpu().numpy() for k, v in o.items()}, want, "mask %r" % (m is None))
    assert (want["status"] == 0).all()
