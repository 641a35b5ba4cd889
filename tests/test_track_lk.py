"""Pyramidal Lucas-Kanade tracking and sub-pixel match refinement (pislam_track_lk_batch).

The expectation is a plain-Python restatement of the contract in include/pislam_hip.h, independent of the library: the
window sums are numpy int64 (every term is below 2^31 and there are at most 225 of them), everything after them —
determinant, conditioning test, step quotient — is Python integers, so nothing can overflow.  The GPU must agree with
it on every output word.
"""
import ctypes
import functools
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import ROOT

INVALID = -1
SENT = 0x5A5A5A5A                     # fills outputs before a call: entries the call must not write keep it
NO_ERR = 0xFFFFFFFF
COUNT_INVALID = 0xFFFFFFFF
COORD_MAX = 1 << 20
MAP_MAX = 1 << 22

Lk = namedtuple("Lk", "win_radius max_iters eps_q8 max_step_q8 level_step max_coarse min_eig max_err")
LK_FIELDS = list(Lk._fields)
DEFAULTS = Lk(7, 10, 8, 2048, 3, 2, 16, 0)


# ---- the expectation ------------------------------------------------------------------------------------------------
def clamp(v, lo, hi):
    return max(lo, min(hi, int(v)))


def inside(x, y, m, W, H):
    x0, y0 = x >> 8, y >> 8
    return x0 - m >= 0 and y0 - m >= 0 and x0 + m + 1 <= W - 1 and y0 + m + 1 <= H - 1


def smp_grid(img, x, y, r):
    """Smp(x + 256 dx, y + 256 dy) for |dx|, |dy| <= r: int64 [2r+1][2r+1], rows = dy.  img: the level's rectangle."""
    H, W = img.shape
    assert inside(x, y, r, W, H)                      # no byte outside the level's rectangle is ever read
    x0, ax, y0, ay = x >> 8, x & 255, y >> 8, y & 255
    B = img[y0 - r:y0 + r + 2, x0 - r:x0 + r + 2].astype(np.int64)
    assert B.shape == (2 * r + 2, 2 * r + 2)
    return ((256 - ax) * (256 - ay) * B[:-1, :-1] + ax * (256 - ay) * B[:-1, 1:] + (256 - ax) * ay * B[1:, :-1]
            + ax * ay * B[1:, 1:] + 1024) >> 11


def ref_level(prev, nxt, p, q, prm, own):
    """The level procedure on one level (prev, nxt: the level's rectangles): (code, q, it, sad or None)."""
    w = prm.win_radius
    n = (2 * w + 1) ** 2
    H, W = prev.shape
    (px, py), (qx, qy) = p, q
    if not inside(px, py, w + 1, W, H):
        return 1, q, 0, None
    T = smp_grid(prev, px, py, w + 1)
    gx = (T[1:-1, 2:] - T[1:-1, :-2] + 4) >> 3
    gy = (T[2:, 1:-1] - T[:-2, 1:-1] + 4) >> 3
    Tw = T[1:-1, 1:-1]
    assert abs(gx).max() <= 1020 and abs(gy).max() <= 1020
    A11, A12, A22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
    t = prm.min_eig * n
    det = A11 * A22 - A12 * A12
    if not (det > 0 and A11 + A22 >= 2 * t and (A11 - t) * (A22 - t) - A12 * A12 >= 0):
        return 2, q, 0, None
    if not inside(qx, qy, w, W, H):
        return 3, q, 0, None
    it = 0
    while True:
        r = smp_grid(nxt, qx, qy, w) - Tw
        sad = int(abs(r).sum())
        if it == prm.max_iters:
            code = 0
            break
        b1, b2 = int((r * gx).sum()), int((r * gy).sum())
        assert abs(b1) < 1 << 31 and abs(b2) < 1 << 31
        nx, ny = A22 * b1 - A12 * b2, A11 * b2 - A12 * b1
        sx = clamp((-64 * nx + det // 2) // det, -prm.max_step_q8, prm.max_step_q8)
        sy = clamp((-64 * ny + det // 2) // det, -prm.max_step_q8, prm.max_step_q8)
        it += 1
        if not inside(qx + sx, qy + sy, w, W, H):
            return 3, (qx, qy), it, None
        qx, qy = qx + sx, qy + sy
        if abs(sx) <= prm.eps_q8 and abs(sy) <= prm.eps_q8:
            sad = int(abs(smp_grid(nxt, qx, qy, w) - Tw).sum())
            code = 0
            break
    if own and code == 0 and prm.max_err > 0 and sad > prm.max_err * n:
        code = 4
    return code, (qx, qy), it, sad


def map_level(u, s_from, s_to):
    return clamp((u * s_from + s_to // 2) // s_to, -MAP_MAX, MAP_MAX)


def ref_point(levels, scales, prev, nxt, pt, guess, prm):
    """One point on one pair (prev, nxt: uint8 [rows][vstep]): (next x, next y, status, err)."""
    x, y = (clamp(v, -COORD_MAX, COORD_MAX) for v in pt)
    qx, qy = (x, y) if guess is None else (clamp(v, -COORD_MAX, COORD_MAX) for v in guess)
    l = None
    for k, (w, h, r0, c0) in enumerate(levels):
        if c0 <= x >> 8 < c0 + w and r0 <= y >> 8 < r0 + h:
            l = k
    if l is None:
        return qx, qy, 1, NO_ERR

    def rect(img, k):
        w, h, r0, c0 = levels[k]
        return img[r0:r0 + h, c0:c0 + w]

    c0, r0 = levels[l][3], levels[l][2]
    p = (x - 256 * c0, y - 256 * r0)
    q = (qx - 256 * c0, qy - 256 * r0)
    M = min(prm.max_coarse, (len(levels) - 1 - l) // prm.level_step)
    for m in range(M, 0, -1):
        c = l + m * prm.level_step
        pc = tuple(map_level(v, scales[l], scales[c]) for v in p)
        qc = tuple(map_level(v, scales[l], scales[c]) for v in q)
        code, qc, _, _ = ref_level(rect(prev, c), rect(nxt, c), pc, qc, prm, False)
        if code == 0:
            q = tuple(map_level(v, scales[c], scales[l]) for v in qc)
    code, q, it, sad = ref_level(rect(prev, l), rect(nxt, l), p, q, prm, True)
    return q[0] + 256 * c0, q[1] + 256 * r0, code | it << 8, sad if code in (0, 4) else NO_ERR


def norm_levels(levels):
    return [(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 0) for t in levels]


def ref_batch(levels, scales, prev, nxt, pts, counts, guess, prm):
    """prev, nxt: uint8 [B][rows][vstep]; pts (and guess, or None) int [B][S][2]; counts [B].  Returns next int32
    [B][S][2], status and err uint32 [B][S] (SENT where nothing is written) and ntracked uint32 [B]."""
    levels = norm_levels(levels)
    B, S = pts.shape[:2]
    nq = np.full((B, S, 2), SENT, np.int32)
    st = np.full((B, S), SENT, np.uint32)
    er = np.full((B, S), SENT, np.uint32)
    nt = np.zeros(B, np.uint32)
    for b in range(B):
        n = 0 if int(counts[b]) == COUNT_INVALID else min(int(counts[b]), S)
        for i in range(n):
            g = None if guess is None else guess[b, i]
            x, y, s, e = ref_point(levels, scales, prev[b], nxt[b], pts[b, i], g, prm)
            nq[b, i], st[b, i], er[b, i] = (x, y), s, e
            nt[b] += (s & 255) == 0
    return nq, st, er, nt


# ---- analytic textures ------------------------------------------------------------------------------------------------
def sinusoids(rng, n, kmin, kmax, amp):
    """n components (kx, ky, phase, amplitude) with kmin <= |k| <= kmax rad/px."""
    k = rng.uniform(kmin, kmax, n)
    th = rng.uniform(0, 2 * np.pi, n)
    return [(k[i] * math.cos(th[i]), k[i] * math.sin(th[i]), rng.uniform(0, 2 * np.pi), amp) for i in range(n)]


def render(comps, W, H, scale=1.0, shift=(0.0, 0.0)):
    """The 8-bit image whose pixel (x, y) is the texture at (x * scale - shift_x, y * scale - shift_y)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = xx * scale - shift[0], yy * scale - shift[1]
    v = np.full((H, W), 128.0)
    for kx, ky, ph, a in comps:
        v += a * np.sin(kx * X + ky * Y + ph)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def translation_case(shift, seed=5):
    rng = np.random.default_rng(seed)
    comps = sinusoids(rng, 10, 0.08, 0.35, 11.0)
    W, H = 160, 120
    prev, nxt = render(comps, W, H), render(comps, W, H, shift=shift)
    pts = np.stack([rng.integers(24 * 256, (W - 24) * 256, 60), rng.integers(24 * 256, (H - 24) * 256, 60)], 1)
    return [(W, H, 0, 0)], [65536], prev, nxt, pts


C2F_SCALES = (1.0, 1.73, 3.0)
C2F_BAND = 1.6                        # a level keeps the components below this many rad per level pixel (Nyquist: pi)


def coarse_to_fine_case(seed=11):
    """Three band-limited levels of one texture, stacked: low components every level sees, middle ones the coarsest
    level has lost, high ones only level 0 has."""
    rng = np.random.default_rng(seed)
    comps = sinusoids(rng, 4, 0.05, 0.10, 14.0) + sinusoids(rng, 4, 0.6, 0.9, 7.0) + sinusoids(rng, 6, 1.1, 1.5, 6.0)
    shift = (9.6, 7.1)
    W0, H0 = 240, 200
    levels, row = [], 0
    for s in C2F_SCALES:
        w, h = int(W0 / s), int(H0 / s)
        levels.append((w, h, row, 0))
        row += h
    prev, nxt = np.zeros((row, W0), np.uint8), np.zeros((row, W0), np.uint8)
    for (w, h, r0, _), s in zip(levels, C2F_SCALES):
        kept = [c for c in comps if math.hypot(c[0], c[1]) * s < C2F_BAND]
        assert kept and all(math.hypot(c[0], c[1]) * s < math.pi for c in kept)
        prev[r0:r0 + h, :w] = render(kept, w, h, s)
        nxt[r0:r0 + h, :w] = render(kept, w, h, s, shift)
    scales = [int(round(65536 * s)) for s in C2F_SCALES]
    pts = np.stack([rng.integers(40 * 256, (W0 - 52) * 256, 40), rng.integers(40 * 256, (H0 - 50) * 256, 40)], 1)
    return levels, scales, prev, nxt, pts, shift


# ---- CPU: declarations and the expectation's anchors ----------------------------------------------------------------
def test_track_lk_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pislam_track_lk_batch\s*\(", code), "pislam_track_lk_batch is not declared in include/pislam_hip.h"
    m = re.search(r"typedef struct pislam_lk_params \{([^}]*)\} pislam_lk_params;", code)
    assert m and re.findall(r"int32_t\s+(\w+)\s*;", m.group(1)) == LK_FIELDS
    from pislam_amd import capi, frontend
    assert "pislam_track_lk_batch" in capi.SYMBOLS and len(capi.SYMBOLS["pislam_track_lk_batch"][1]) == 19
    assert [n for n, _ in capi.LkParams._fields_] == LK_FIELDS
    assert ctypes.sizeof(capi.LkParams) == 4 * len(LK_FIELDS)
    for f in ("keypointsToQ8", "trackLKBatch", "refineMatchesBatch"):
        assert callable(getattr(frontend, f)), f
    assert hasattr(capi.load(), "pislam_track_lk_batch")


def test_ref_lk_anchors():
    """The expectation itself, independent of the library."""
    # (a) pure translation of an analytic texture (|k| <= 0.35 rad/px), one level, w = 7, 60 interior points
    worst, iters = 0.0, []
    for shift in ((0.3, -0.2), (1.7, 0.6), (-2.4, 1.9)):
        levels, scales, prev, nxt, pts = translation_case(shift)
        prm = DEFAULTS._replace(eps_q8=2, max_iters=32, max_coarse=0)
        for p in pts:
            x, y, st, err = ref_point(levels, scales, prev, nxt, p, None, prm)
            assert st & 255 == 0 and st >> 8 < 32 and err != NO_ERR, (shift, p, st)
            worst = max(worst, abs((x - p[0]) / 256 - shift[0]), abs((y - p[1]) / 256 - shift[1]))
            iters.append(st >> 8)
    print("translation: worst %.4f px, iterations %.2f mean, %d max" % (worst, np.mean(iters), max(iters)))
    assert worst <= 1 / 16                  # measured with this texture: 0.0492 px; 3.0 iterations on average, 4 at most

    # (b) coarse to fine: a 9.6 x 7.1 px shift is out of level 0's reach alone and in reach through two coarser levels
    levels, scales, prev, nxt, pts, shift = coarse_to_fine_case()
    frac = {}
    for mc in (0, 2):
        prm = DEFAULTS._replace(eps_q8=2, max_iters=32, level_step=1, max_coarse=mc)
        e = []
        for p in pts:
            x, y, st, _ = ref_point(levels, scales, prev, nxt, p, None, prm)
            e.append(max(abs((x - p[0]) / 256 - shift[0]), abs((y - p[1]) / 256 - shift[1])) if st & 255 == 0 else 1e9)
        frac[mc] = (np.mean(np.array(e) <= 0.1), max(e))
    print("coarse to fine: within 0.1 px %.0f %% at max_coarse 0, %.0f %% at 2 (worst %.4f px)"
          % (100 * frac[0][0], 100 * frac[2][0], frac[2][1]))
    assert frac[0][0] < 0.5                 # measured: 0 %
    assert frac[2][0] == 1.0                # measured: 100 %, worst 0.0414 px

    # (c) codes that can be checked by hand
    W, H = 64, 48
    lv, sc = [(W, H, 0, 0)], [65536]
    rng = np.random.default_rng(3)
    comps = sinusoids(rng, 6, 0.1, 0.35, 15.0)
    tex = render(comps, W, H)
    flat = np.full((H, W), 77, np.uint8)
    prm = DEFAULTS._replace(max_coarse=0, min_eig=0)
    mid = (32 * 256 + 40, 24 * 256 + 200)
    # a constant patch: A = 0, det = 0
    assert ref_point(lv, sc, flat, flat, mid, None, prm) == (mid[0], mid[1], 2, NO_ERR)
    # the template needs w + 1 = 8 pixels to the left and 8 + 1 to the right: column 7 fails, 8 passes; 54 passes, 55 fails
    for x0, code in ((7, 1), (8, 0), (W - 10, 0), (W - 9, 1)):
        x, y, st, err = ref_point(lv, sc, tex, tex, (x0 * 256, 24 * 256), None, prm)
        assert st & 255 == code and (code != 0 or (x, y, err) == (x0 * 256, 24 * 256, 0)), (x0, st)
    assert ref_point(lv, sc, tex, tex, (7 * 256, 24 * 256), (5, 6), prm) == (5, 6, 1, NO_ERR)      # q as it entered
    # a guess outside: the search window needs w = 7 pixels; it = 0
    assert ref_point(lv, sc, tex, tex, mid, (6 * 256 + 255, 24 * 256), prm) == (6 * 256 + 255, 24 * 256, 3, NO_ERR)
    assert ref_point(lv, sc, tex, tex, mid, (-5000, 1 << 30), prm) == (-5000, COORD_MAX, 3, NO_ERR)    # clamped first
    # a step that leaves: the patch of column 20 lies at column 5 of next, left of the first column (7) a window can
    # have; from a guess at column 9 the steps, clamped to one pixel, walk left until one would leave: that one counts
    nxt = render(comps, W, H, shift=(-15.0, 0.0))
    x, y, st, err = ref_point(lv, sc, tex, nxt, (20 * 256, 24 * 256), (9 * 256, 24 * 256), prm._replace(max_step_q8=256, eps_q8=0))
    assert st & 255 == 3 and st >> 8 >= 2 and err == NO_ERR and inside(x, y, 7, W, H) and x >> 8 == 7 and x < 9 * 256
    # a mismatched pair (next is prev with every other pixel 30 grey levels brighter, the rest as much darker: 960 in
    # Q5): with max_err of 10 grey levels the code is 4 and err still the sad; without it 0, the same position and err
    yy, xx = np.mgrid[0:H, 0:W]
    other = (tex.astype(np.int32) + 30 - 60 * ((xx + yy) & 1)).clip(0, 255).astype(np.uint8)
    a = ref_point(lv, sc, tex, other, mid, None, prm._replace(max_err=320))
    b = ref_point(lv, sc, tex, other, mid, None, prm)
    assert a[2] & 255 == 4 and b[2] & 255 == 0 and a[:2] == b[:2] and a[3] == b[3] > 320 * 225 and a[2] >> 8 == b[2] >> 8
    assert ref_point(lv, sc, tex, other, mid, None, prm._replace(max_err=8160))[2] & 255 == 0
    # no level at all
    assert ref_point([(20, 20, 0, 0)], sc, tex, tex, (30 * 256, 5 * 256), (1, 2), prm) == (1, 2, 1, NO_ERR)
    # the split quotient of the header equals the exact statement (the GPU computes it that way)
    for n, det in ((2 ** 60 - 1, 1), (-(2 ** 60) + 1, 3), (12345678901234567, 2 ** 56 - 1), (-77, 1000), (0, 5), (6400, 100),
                   (-(2 ** 59), 2 ** 40 + 1)):
        k, rem = n // det, n % det
        assert -64 * k + (det // 2 - 64 * rem) // det == (-64 * n + det // 2) // det and 64 * rem < 2 ** 62


# ---- GPU parity -------------------------------------------------------------------------------------------------------
def smooth_texture(H, W, seed):
    """Random texture with a few pixels of correlation length, full 8-bit range."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(H + 12, W + 12))
    for _ in range(2):
        a = a[:-2] + a[1:-1] + a[2:]
        a = a[:, :-2] + a[:, 1:-1] + a[:, 2:]
    a = a[2:2 + H, 2:2 + W]
    return np.clip(128 + 60 * (a - a.mean()) / a.std(), 0, 255).astype(np.uint8)


def shifted_pair(H, W, seed, dx, dy, noise=2):
    """(prev, next): next(x, y) = prev(x - dx, y - dy) plus uniform noise."""
    rng = np.random.default_rng(seed + 1000)
    big = smooth_texture(H + 8, W + 8, seed).astype(np.int32)
    prev = big[4:4 + H, 4:4 + W]
    nxt = big[4 - dy:4 - dy + H, 4 - dx:4 - dx + W] + rng.integers(-noise, noise + 1, (H, W))
    return prev.astype(np.uint8), nxt.clip(0, 255).astype(np.uint8)


def chain_scales(levels):
    w0 = levels[0][0]
    return [(2 * 65536 * w0 + t[0]) // (2 * t[0]) for t in levels]


class Device:
    def __init__(self, ctx):
        import torch
        from pislam_amd import capi
        self.torch, self.ctx, self.lib, self.capi = torch, ctx, ctx.lib, capi

    def tables(self, levels, scales):
        lv = norm_levels(levels)
        n = len(lv)
        return (self.capi.Level * n)(*[self.capi.Level(w, h, r0, c0) for w, h, r0, c0 in lv]), n, (ctypes.c_int32 * n)(*scales)

    def up(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).cuda()

    def build(self, frames_prev, frames_next, nlevels):
        """PyramidBuilder on both frame stacks: (levels, scales, prev, next device tensors, prev, next numpy)."""
        from pislam_amd.frontend import DEFAULT_CHAIN, PyramidBuilder
        B, H, W = frames_prev.shape
        pb = PyramidBuilder(W, H, DEFAULT_CHAIN[:nlevels - 1], ctx=self.ctx)
        pyr = [self.torch.zeros((B, pb.rows, pb.vstep), dtype=self.torch.uint8, device="cuda") for _ in range(2)]
        pb(self.up(frames_prev), pyr[0])
        pb(self.up(frames_next), pyr[1])
        self.ctx.synchronize()
        return pb.levels, chain_scales(pb.levels), pyr[0], pyr[1], pyr[0].cpu().numpy(), pyr[1].cpu().numpy()

    def run(self, levels, scales, prev, nxt, pts, counts, guess, prm, *, want_nt=True, alias=False, stride=None):
        """One call on sentinel-filled outputs: (rc, next, status, err, ntracked or None) as numpy."""
        torch = self.torch
        B, S = pts.shape[:2]
        lv, n, sc = self.tables(levels, scales)
        p = self.capi.LkParams(*prm)
        d_pts = self.up(pts.astype(np.int32))
        d_counts = self.up(np.asarray(counts, np.uint32).view(np.int32))
        d_guess = None if guess is None else self.up(guess.astype(np.int32))
        d_next = d_guess if alias else torch.full((B, S, 2), SENT, dtype=torch.int32, device="cuda")
        d_st = torch.full((B, S), SENT, dtype=torch.int32, device="cuda")
        d_er = torch.full((B, S), SENT, dtype=torch.int32, device="cuda")
        d_nt = torch.full((B,), SENT, dtype=torch.int32, device="cuda") if want_nt else None
        rc = self.lib.pislam_track_lk_batch(self.ctx.h, ctypes.byref(p), lv, n, sc, prev.data_ptr(), nxt.data_ptr(),
                                            int(prev.stride(1)), int(prev.shape[1]), int(prev.stride(0)) if stride is None else stride,
                                            d_pts.data_ptr(), d_counts.data_ptr(), 0 if d_guess is None else d_guess.data_ptr(), S, B,
                                            d_next.data_ptr(), d_st.data_ptr(), d_er.data_ptr(), 0 if d_nt is None else d_nt.data_ptr())
        self.ctx.synchronize()
        return (rc, d_next.cpu().numpy(), d_st.cpu().numpy().view(np.uint32), d_er.cpu().numpy().view(np.uint32),
                None if d_nt is None else d_nt.cpu().numpy().view(np.uint32))

    def check(self, levels, scales, prev, nxt, prev_np, nxt_np, pts, counts, guess, prm, tag="", **kw):
        """Runs the call and the expectation; every output word must agree.  Returns the expectation."""
        want = ref_batch(levels, scales, prev_np, nxt_np, pts, counts, guess, Lk(*prm))
        if kw.get("alias"):                                  # slots that are not written keep the guess
            keep = want[1] == SENT
            want[0][keep] = guess.astype(np.int32)[keep]
        rc, nq, st, er, nt = self.run(levels, scales, prev, nxt, pts, counts, guess, prm, **kw)
        assert rc == 0, self.lib.pislam_last_error(self.ctx.h)
        for name, got, exp in (("next_q8", nq, want[0]), ("status", st, want[1]), ("err", er, want[2])):
            bad = np.argwhere(got != exp)
            assert len(bad) == 0, "%s %s: %d differ, first %s: got %s, want %s (status %s)" % (
                tag, name, len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])], hex(int(want[1][tuple(bad[0][:2])])))
        if nt is not None:
            assert (nt == want[3]).all(), (tag, nt, want[3])
        return want


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    return Device(gpu_ctx)


# frame size, levels of the default chain, the two pairs' shifts
PYRAMIDS = {"A": (96, 80, 6, ((0, 0), (3, -2))), "B": (131, 77, 4, ((4, 1), (-1, -4))), "C": (96, 80, 5, ((2, 2), (-3, 0)))}


@functools.lru_cache(maxsize=None)
def matrix_frames(key):
    W, H, nl, shifts = PYRAMIDS[key]
    pairs = [shifted_pair(H, W, 20 + 7 * k + ord(key), dx, dy) for k, (dx, dy) in enumerate(shifts)]
    return np.stack([p for p, _ in pairs]), np.stack([n for _, n in pairs]), nl


@pytest.fixture(scope="module")
def pyramids(dev):
    return {key: dev.build(*matrix_frames(key)) for key in PYRAMIDS}


def matrix_points(levels, vstep, w, seed, B):
    """Per level: interior points, points exactly w, w + 1 and w + 2 pixels from each border (the template needs
    w + 1 on the left and top and w + 2 on the right and bottom), and points in no level."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        pts = []
        for (W, H, r0, c0) in norm_levels(levels):
            def add(x0, y0):
                fx, fy = (int(rng.choice([0, 1, 128, 255])), int(rng.choice([0, 77, 255])))
                pts.append(((c0 + x0) * 256 + fx, (r0 + y0) * 256 + fy))
            for _ in range(8):
                add(int(rng.integers(w + 2, max(w + 3, W - w - 3))), int(rng.integers(w + 2, max(w + 3, H - w - 3))))
            for d in (w, w + 1, w + 2):
                add(d, H // 2), add(W - 1 - d, H // 2), add(W // 2, d), add(W // 2, H - 1 - d)
            if c0 + W + 2 < vstep:
                pts.append(((c0 + W + 2) * 256, (r0 + H // 2) * 256))         # right of the level: in no level
        pts += [(-300, 40 * 256), (1 << 25, 1 << 25), (30 * 256, -(1 << 24))]
        out.append(pts)
    return np.array(out, np.int64)


MATRIX = [  # pyramids, Lk(w, max_iters, eps, max_step, level_step, max_coarse, min_eig, max_err), random guess
    ("A", Lk(1, 32, 0, 4096, 1, 0, 0, 0), False),
    ("B", Lk(1, 32, 255, 4096, 1, 3, 0, 400), True),
    ("C", Lk(1, 1, 0, 1, 3, 2, 0, 0), False),
    ("A", Lk(1, 32, 0, 4096, 15, 15, 1 << 20, 0), True),
    ("B", Lk(3, 32, 255, 4096, 1, 0, 0, 100), True),
    ("A", Lk(3, 32, 0, 4096, 1, 3, 0, 0), False),
    ("A", Lk(3, 1, 255, 4096, 3, 2, 0, 0), True),
    ("C", Lk(3, 32, 0, 1, 15, 15, 0, 60), False),
    ("C", Lk(7, 32, 255, 4096, 1, 0, 0, 0), False),
    ("A", Lk(7, 32, 0, 4096, 1, 3, 0, 60), True),
    ("A", Lk(7, 32, 255, 4096, 3, 2, 0, 0), False),
    ("B", Lk(7, 1, 0, 4096, 15, 15, 1 << 20, 0), True),
]
assert {m[1].win_radius for m in MATRIX} == {1, 3, 7} and {m[1].max_iters for m in MATRIX} == {1, 32}
assert {m[1].eps_q8 for m in MATRIX} == {0, 255} and {m[1].max_step_q8 for m in MATRIX} == {1, 4096}
assert {m[1].min_eig for m in MATRIX} == {0, 1 << 20} and {m[1].max_err > 0 for m in MATRIX} == {False, True}
assert {(m[1].win_radius, m[1].level_step, m[1].max_coarse) for m in MATRIX} == {
    (w, ls, mc) for w in (1, 3, 7) for ls, mc in ((1, 0), (1, 3), (3, 2), (15, 15))}
MATRIX_SEEN = {}                       # case -> status codes of the expectation (filled by the matrix test)


def matrix_case(k, levels, vstep):
    key, prm, rnd = MATRIX[k]
    pts = matrix_points(levels, vstep, prm.win_radius, 100 + k, 2)
    rng = np.random.default_rng(200 + k)
    guess = pts + rng.integers(-768, 769, pts.shape) if rnd else None
    return pts, guess, np.array([pts.shape[1]] * 2, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(MATRIX)), ids=["%s-w%d-it%d-eps%d-step%d-ls%d-mc%d-eig%d-err%d" % ((m[0],) + tuple(m[1]))
                                                      for m in MATRIX])
def test_gpu_matrix_against_ref(dev, pyramids, k):
    levels, scales, prev, nxt, prev_np, nxt_np = pyramids[MATRIX[k][0]]
    pts, guess, counts = matrix_case(k, levels, int(prev.shape[2]))
    want = dev.check(levels, scales, prev, nxt, prev_np, nxt_np, pts, counts, guess, MATRIX[k][1], tag="case %d" % k)
    MATRIX_SEEN[k] = want[1] & 255
    lv_of = set()
    for (x, y) in pts.reshape(-1, 2):
        for l, (w, h, r0, c0) in enumerate(norm_levels(levels)):
            if c0 <= x >> 8 < c0 + w and r0 <= y >> 8 < r0 + h:
                lv_of.add(l)
    assert lv_of == set(range(len(levels)))                 # every level holds some points


@pytest.mark.gpu
def test_gpu_matrix_coverage(dev, pyramids):
    """Across the matrix every status code occurs, and code 0 for at least a quarter of the points (on the
    expectation: parity is checked case by case above; a case that has not run yet is run here)."""
    for k in range(len(MATRIX)):
        if k not in MATRIX_SEEN:
            test_gpu_matrix_against_ref(dev, pyramids, k)
    codes = np.concatenate([v.reshape(-1) for v in MATRIX_SEEN.values()])
    hist = np.bincount(codes, minlength=5)
    print("matrix status codes 0..4:", hist.tolist())
    assert len(hist) == 5 and (hist > 0).all() and hist[0] * 4 >= len(codes)


def single_level(dev, prev_np, nxt_np):
    """One level that fills the buffers: (levels, scales, prev, next, prev_np, next_np), batch = the leading axis."""
    H, W = prev_np.shape[1:]
    return [(W, H, 0, 0)], [65536], dev.up(prev_np), dev.up(nxt_np), prev_np, nxt_np


def binary_images():
    """(prev, next) stacks.  0 / 255 images against their inverse: checkerboards of 2 and 3 pixel cells (|g| = 1020 on
    every pixel of the first, |r| = 8160), random bits, plain stripes (det = 0), stripes with dots, and stripes with
    faint dots of 1 to 3 grey levels (A22 tiny against a residual of 8160: the quotient k runs into the thousands).
    Last, the 2 pixel checkerboard against itself moved by one column, where r and gx agree in sign wherever r is not
    zero: the largest |b| 8-bit images allow."""
    H, W = 48, 64
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(9)
    stripes = 255 * ((xx // 2) & 1)
    prev = [255 * (((xx // 2) + (yy // 2)) & 1), 255 * (((xx // 3) + (yy // 3)) & 1), 255 * rng.integers(0, 2, (H, W)), stripes]
    dots = stripes.copy()
    dots[rng.integers(0, H, 12), rng.integers(0, W, 12)] ^= 255
    faint = stripes.copy()
    at = (rng.integers(0, H, 60), rng.integers(0, W, 60))
    faint[at] = np.abs(faint[at] - rng.integers(1, 4, 60))
    prev += [dots, faint]
    nxt = [255 - v for v in prev]
    prev.append(prev[0])
    nxt.append(np.roll(prev[0], 1, axis=1))
    return np.stack(prev).astype(np.uint8), np.stack(nxt).astype(np.uint8)


@pytest.mark.gpu
def test_gpu_worst_case_magnitudes(dev):
    """0 / 255 patterns against their inverse at w = 7: |g| = 1020 and |r| = 8160 over whole windows drive b and n to
    their bounds, the nearly singular ones drive the quotient far past the clamp."""
    prev_np, nxt_np = binary_images()
    B = len(prev_np)
    rng = np.random.default_rng(10)
    pts = np.stack([rng.integers(10, 52, (B, 24)) * 256, rng.integers(10, 36, (B, 24)) * 256], -1)
    pts[:, 12:] += rng.integers(0, 256, (B, 12, 2))                      # half of them at fractional positions
    tabs = single_level(dev, prev_np, nxt_np)
    counts = np.full(B, 24, np.uint32)
    seen = []
    for prm in (Lk(7, 32, 0, 4096, 1, 0, 0, 0), Lk(7, 32, 0, 1, 1, 0, 0, 0), Lk(7, 4, 255, 4096, 1, 0, 0, 8160)):
        seen.append(dev.check(*tabs, pts, counts, None, prm, tag=str(prm))[1] & 255)
    # the bounds are really approached: recompute b and the quotient of the first iteration on the expectation's side
    big_b, big_k = 0, 0
    for b in range(B):
        for (x, y) in pts[b]:
            T = smp_grid(prev_np[b], int(x), int(y), 8)
            gx, gy = (T[1:-1, 2:] - T[1:-1, :-2] + 4) >> 3, (T[2:, 1:-1] - T[:-2, 1:-1] + 4) >> 3
            r = smp_grid(nxt_np[b], int(x), int(y), 7) - T[1:-1, 1:-1]
            A11, A12, A22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
            b1, b2, det = int((r * gx).sum()), int((r * gy).sum()), A11 * A22 - A12 * A12
            big_b = max(big_b, abs(b1), abs(b2))
            if det > 0:
                big_k = max(big_k, abs((A22 * b1 - A12 * b2) // det), abs((A11 * b2 - A12 * b1) // det))
    print("largest |b| 2^%.1f, largest |k| %d" % (math.log2(max(big_b, 1)), big_k))
    assert big_b > 1 << 29 and big_k > 128          # measured: 2^29.8 and 1049
    assert (np.concatenate([s.reshape(-1) for s in seen]) == 2).any()   # the plain stripes: det = 0


@pytest.mark.gpu
def test_gpu_counts_and_ntracked(dev):
    """Counts of 0, beyond the stride and PISLAM_COUNT_INVALID; nothing is written at or beyond n_b; ntracked NULL or
    given."""
    prev_np, nxt_np = (np.stack(v) for v in zip(*[shifted_pair(40, 44, 30 + b, 1, -1) for b in range(4)]))
    tabs = single_level(dev, prev_np, nxt_np)
    rng = np.random.default_rng(12)
    pts = np.stack([rng.integers(9 * 256, 34 * 256, (4, 5)), rng.integers(9 * 256, 30 * 256, (4, 5))], -1)
    counts = np.array([0, 9, COUNT_INVALID, 3], np.uint32)
    prm = Lk(3, 10, 8, 2048, 1, 0, 0, 0)
    for want_nt in (True, False):
        want = dev.check(*tabs, pts, counts, None, prm, want_nt=want_nt)
    assert want[3].tolist()[0] == 0 and want[3][2] == 0 and want[3][1] > 0 and (want[1][3, 3:] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 65537])
def test_gpu_batch_sizes(dev, batch):
    """One point per pair, batch 1 and batch 65537 (past one launch's 65535 pairs).  The pairs' pyramids are 24 x 24
    windows one byte apart (pyramid_stride = 1) into a buffer of period 256, so pair b equals pair b % 256 and the
    expectation is computed 256 times."""
    torch = dev.torch
    H = W = 24
    period = smooth_texture(16, 16, 40).reshape(-1)
    other = smooth_texture(16, 16, 41).reshape(-1) // 4 + period - period // 4
    n = batch - 1 + H * W
    bufs = [np.tile(v.astype(np.uint8), n // 256 + 1)[:n] for v in (period, other)]
    nd = min(batch, 256)
    views = [np.stack([v[b:b + H * W].reshape(H, W) for b in range(nd)]) for v in bufs]
    rng = np.random.default_rng(13)
    pts_d = np.stack([rng.integers(3 * 256, 20 * 256, (nd, 1)), rng.integers(3 * 256, 20 * 256, (nd, 1))], -1)
    prm = Lk(2, 3, 8, 2048, 1, 0, 0, 0)
    want = ref_batch([(W, H, 0, 0)], [65536], views[0], views[1], pts_d, np.ones(nd, np.uint32), None, prm)
    reps = batch // nd + 1
    pts = np.tile(pts_d, (reps, 1, 1))[:batch]
    d = [dev.up(v).reshape(1, 1, -1) for v in bufs]
    lv, nl, sc = dev.tables([(W, H, 0, 0)], [65536])
    p = dev.capi.LkParams(*prm)
    d_pts, d_counts = dev.up(pts.astype(np.int32)), torch.ones((batch,), dtype=torch.int32, device="cuda")
    outs = [torch.full(s, SENT, dtype=torch.int32, device="cuda") for s in ((batch, 1, 2), (batch, 1), (batch, 1), (batch,))]
    rc = dev.lib.pislam_track_lk_batch(dev.ctx.h, ctypes.byref(p), lv, nl, sc, d[0].data_ptr(), d[1].data_ptr(), W, H, 1,
                                       d_pts.data_ptr(), d_counts.data_ptr(), 0, 1, batch, *[o.data_ptr() for o in outs])
    assert rc == 0, dev.lib.pislam_last_error(dev.ctx.h)
    dev.ctx.synchronize()
    for got, exp in zip(outs, want):
        exp = np.tile(exp, (reps,) + (1,) * (exp.ndim - 1))[:batch]
        assert (got.cpu().numpy().view(exp.dtype) == exp).all()
    assert batch == 1 or len(set(want[1].reshape(-1).tolist())) > 1


@pytest.mark.gpu
def test_gpu_next_may_alias_guess(dev, pyramids):
    levels, scales, prev, nxt, prev_np, nxt_np = pyramids["A"]
    pts, guess, counts = matrix_case(9, levels, int(prev.shape[2]))
    counts = counts - np.array([0, 7], np.uint32)                       # some slots stay unwritten: they keep the guess
    prm = Lk(7, 10, 8, 2048, 1, 3, 0, 0)
    a = dev.check(levels, scales, prev, nxt, prev_np, nxt_np, pts, counts, guess, prm)
    b = dev.check(levels, scales, prev, nxt, prev_np, nxt_np, pts, counts, guess, prm, alias=True)
    assert (a[1] == b[1]).all()


@pytest.mark.gpu
def test_gpu_strides_past_4_gib(dev):
    """Two pairs whose pyramid_stride puts pair 1 beyond 4 GiB (each pyramid stack allocated in one piece, as
    test_clahe.py does): only the pyramids' own bytes are set."""
    torch = dev.torch
    H, W = 40, 44
    stride = (1 << 32) + 4099
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * (stride + H * W) + (1 << 30):
        pytest.skip("two buffers of 4 GiB do not fit the free device memory")
    prev_np, nxt_np = (np.stack(v) for v in zip(*[shifted_pair(H, W, 50 + b, -1, 2) for b in range(2)]))
    rng = np.random.default_rng(14)
    pts = np.stack([rng.integers(9 * 256, 34 * 256, (2, 6)), rng.integers(9 * 256, 30 * 256, (2, 6))], -1)
    bufs = None
    try:
        bufs = [torch.empty((stride + H * W,), dtype=torch.uint8, device="cuda") for _ in range(2)]
        for buf, src in zip(bufs, (prev_np, nxt_np)):
            for b in range(2):
                buf[b * stride:b * stride + H * W] = dev.up(src[b].reshape(-1))
        views = [buf[:H * W].reshape(1, H, W) for buf in bufs]            # geometry of pair 0; the stride is given
        dev.check([(W, H, 0, 0)], [65536], views[0], views[1], prev_np, nxt_np, pts, np.array([6, 6], np.uint32), None,
                  Lk(3, 10, 8, 2048, 1, 0, 0, 0), stride=stride)
    finally:
        bufs = views = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_coordinate_limit(dev):
    """A level whose rectangle ends at column 4095 and row 4095, points near that corner; a second level at the origin
    serves as the coarser one."""
    torch = dev.torch
    R = 4096
    levels, scales = [(60, 50, R - 50, R - 60), (40, 34, 0, 0)], [65536, 98304]
    comps = sinusoids(np.random.default_rng(15), 8, 0.1, 0.5, 12.0)
    prev_np, nxt_np = np.zeros((1, R, R), np.uint8), np.zeros((1, R, R), np.uint8)
    for (w, h, r0, c0), s in zip(levels, (1.0, 1.5)):
        prev_np[0, r0:r0 + h, c0:c0 + w] = render(comps, w, h, s)
        nxt_np[0, r0:r0 + h, c0:c0 + w] = render(comps, w, h, s, (2.5, -1.5))
    w = 3
    xs = [R - 1 - d for d in (w + 1, w + 2, w + 3, 20)]
    pts = np.array([[(x * 256 + fx, y * 256 + fy) for x in xs for y in [R - 1 - d for d in (w + 1, w + 2, 15)]
                     for fx, fy in ((0, 0), (255, 255))]], np.int64)
    tabs = (levels, scales, dev.up(prev_np), dev.up(nxt_np), prev_np, nxt_np)
    want = dev.check(*tabs, pts, np.array([pts.shape[1]], np.uint32), None, Lk(w, 10, 8, 2048, 1, 1, 0, 0))
    codes = want[1][0] & 255
    assert (codes == 0).any() and (codes == 1).any() and int(want[0][0, :, 0].max()) >> 8 >= R - 8


@pytest.mark.gpu
def test_gpu_validation(dev):
    """Every limit of the header violated in turn, overlaps, host pointers and NULLs: PISLAM_ERR_INVALID with the
    sentinel-filled outputs untouched.  batch == 0 returns PISLAM_OK after the checks, NULL data pointers accepted."""
    torch, lib, ctx, capi = dev.torch, dev.lib, dev.ctx, dev.capi
    H, W, B, S = 40, 44, 2, 6
    levels, scales = [(W, 24, 0, 0), (20, 16, 24, 0)], [65536, 131072]
    # (large enough for the rows and steps the cases below name: a refusal is then the case's own, not an overlap)
    prev = torch.full((B * 4200 * 4200,), 7, dtype=torch.uint8, device="cuda")
    nxt = torch.full((B * 4200 * 4200,), 7, dtype=torch.uint8, device="cuda")
    pts = torch.full((B, S, 2), 12 * 256, dtype=torch.int32, device="cuda")
    counts = torch.full((B,), S, dtype=torch.int32, device="cuda")
    guess = torch.full((B, S, 2), 12 * 256, dtype=torch.int32, device="cuda")
    out = torch.full((B * S * 4 + B + 16,), SENT, dtype=torch.int32, device="cuda")
    o_next, o_st, o_er, o_nt = (out.data_ptr() + 4 * k for k in (0, 2 * B * S, 3 * B * S, 4 * B * S))
    host = np.zeros(B * H * W, np.int32)
    good = Lk(3, 10, 8, 2048, 1, 1, 0, 0)

    def call(prm=good, lv=levels, sc=scales, nl=None, a=None, b=None, vstep=W, rows=H, pstride=H * W, p=None, c=None, g=0,
             stride=S, batch=B, n=o_next, st=o_st, er=o_er, nt=o_nt, null_p=False, null_lv=False, null_sc=False):
        L, nn, s = dev.tables(lv, sc)
        return lib.pislam_track_lk_batch(ctx.h, None if null_p else ctypes.byref(capi.LkParams(*prm)), None if null_lv else L,
                                         nn if nl is None else nl, None if null_sc else s,
                                         prev.data_ptr() if a is None else a, nxt.data_ptr() if b is None else b, vstep, rows,
                                         pstride, pts.data_ptr() if p is None else p, counts.data_ptr() if c is None else c, g,
                                         stride, batch, n, st, er, nt)

    assert call() == 0 and call(g=guess.data_ptr()) == 0 and call(nt=0) == 0, lib.pislam_last_error(ctx.h)
    ctx.synchronize()
    out.fill_(SENT)
    bad = [dict(prm=good._replace(**{f: v})) for f, v in (
        ("win_radius", 0), ("win_radius", 8), ("max_iters", 0), ("max_iters", 33), ("eps_q8", -1), ("eps_q8", 256),
        ("max_step_q8", 0), ("max_step_q8", 4097), ("level_step", 0), ("level_step", 16), ("max_coarse", -1),
        ("max_coarse", 16), ("min_eig", -1), ("min_eig", (1 << 20) + 1), ("max_err", -1), ("max_err", 8161))]
    bad += [dict(null_p=True), dict(null_lv=True), dict(null_sc=True), dict(nl=0), dict(nl=17), dict(nl=-1),
            dict(lv=[(0, 24, 0, 0), levels[1]]), dict(lv=[(W, 0, 0, 0), levels[1]]), dict(lv=[(W, 24, -1, 0), levels[1]]),
            dict(lv=[(W, 24, 0, -1), levels[1]]),
            dict(lv=[(W, 25, 0, 0), levels[1]]),                                   # the rectangles overlap
            dict(lv=[levels[0], (20, 17, 24, 0)]),                                 # below the last row
            dict(lv=[(W + 1, 24, 0, 0), levels[1]]),                               # beyond vstep
            dict(lv=[(40, 24, 0, 4060), levels[1]], vstep=4200),                   # beyond 12-bit columns
            dict(lv=[(W, 24, 4080, 0), levels[1]], rows=4200),                     # beyond 12-bit rows
            dict(sc=[0, 131072]), dict(sc=[65536, (1 << 20) + 1]), dict(sc=[65536, -5]),
            # (a mapped extent above 65535 cannot be reached inside 12-bit rectangles at scales up to 2^20: 4095 * 16 = 65520)
            dict(vstep=0), dict(rows=0), dict(vstep=W - 1), dict(rows=H - 1), dict(batch=-1), dict(stride=1 << 31),
            dict(a=host.ctypes.data), dict(b=host.ctypes.data), dict(p=host.ctypes.data), dict(c=host.ctypes.data),
            dict(g=host.ctypes.data), dict(n=host.ctypes.data), dict(st=host.ctypes.data), dict(er=host.ctypes.data),
            dict(nt=host.ctypes.data), dict(a=0), dict(b=0), dict(p=0), dict(c=0), dict(n=0), dict(st=0), dict(er=0),
            dict(n=pts.data_ptr()), dict(st=pts.data_ptr() + 4 * (2 * B * S - 1)),                     # outputs on inputs
            dict(er=prev.data_ptr() + (B - 1) * H * W + H * W - 1), dict(nt=counts.data_ptr() + 4), dict(st=nxt.data_ptr()),
            dict(n=guess.data_ptr() + 8, g=guess.data_ptr()),                                          # shifted against the guess
            dict(st=o_next + 4 * (2 * B * S - 1)), dict(nt=o_er)]                                      # outputs on outputs
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert lib.pislam_last_error(ctx.h)
    assert call(batch=0) == 0 and call(batch=0, a=0, b=0, p=0, c=0, n=0, st=0, er=0, nt=0) == 0
    assert call(batch=0, prm=good._replace(win_radius=9)) == INVALID and call(batch=0, nl=0) == INVALID
    ctx.synchronize()
    assert (out.cpu().numpy() == SENT).all() and (pts.cpu().numpy() == 12 * 256).all() and bool((prev == 7).all())
    # touching ranges are no overlap, and next_q8 may be the guess itself
    assert call(n=guess.data_ptr(), g=guess.data_ptr()) == 0
    ctx.synchronize()
    # the Python wrapper checks shapes itself
    from pislam_amd.frontend import trackLKBatch
    pv, nx = prev[:B * H * W].reshape(B, H, W), nxt[:B * H * W].reshape(B, H, W)
    with pytest.raises(ValueError):
        trackLKBatch(pv, nx[:, :H - 1], pts, counts, levels, scales, ctx=ctx)
    with pytest.raises(ValueError):
        trackLKBatch(pv, nx, pts, counts, levels, scales, guess_q8=guess[:, :S - 1], ctx=ctx)
    with pytest.raises(capi.PislamError):
        trackLKBatch(pv, nx, pts, counts, levels, scales, win_radius=8, ctx=ctx)


@pytest.mark.gpu
def test_gpu_track_is_hipgraph_capturable(gpu_ctx):
    """No workspace, no host round trip: the call (with ntracked) captured on a side stream of a fresh context without
    a warm-up call, replayed twice on the same inputs and once on new ones."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import trackLKBatch
    H, W, S = 40, 44, 16
    levels, scales = [(W, H, 0, 0)], [65536]
    rng = np.random.default_rng(16)
    pts_np = np.stack([rng.integers(9 * 256, 34 * 256, (2, S)), rng.integers(9 * 256, 30 * 256, (2, S))], -1)
    counts_np = np.array([S, S - 3], np.uint32)
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        prev = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda")
        nxt = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda")
        pts = torch.from_numpy(pts_np.astype(np.int32)).cuda()
        counts = torch.from_numpy(counts_np.view(np.int32)).cuda()
        outs = [torch.full(s, SENT, dtype=torch.int32, device="cuda") for s in ((2, S, 2), (2, S), (2, S), (2,))]
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            trackLKBatch(prev, nxt, pts, counts, levels, scales, win_radius=3, max_coarse=0, min_eig=0, next_q8=outs[0],
                         status=outs[1], err=outs[2], ntracked=outs[3], ctx=ctx)
        for seed in (60, 60, 62):
            pn, nn = (np.stack(v) for v in zip(*[shifted_pair(H, W, seed + b, 1, 1) for b in range(2)]))
            prev.copy_(torch.from_numpy(pn).cuda())
            nxt.copy_(torch.from_numpy(nn).cuda())
            for o in outs:
                o.fill_(SENT)
            g.replay()
            side.synchronize()
            want = ref_batch(levels, scales, pn, nn, pts_np, counts_np, None, Lk(3, 10, 8, 2048, 3, 0, 0, 0))
            for got, exp in zip(outs, want):
                assert (got.cpu().numpy().view(exp.dtype) == exp).all(), seed
        ctx.close()


@pytest.mark.gpu
def test_gpu_match_select_refine_end_to_end(dev):
    """OrbFrontend -> matchHammingWindowBatch -> selectMatchesBatch -> refineMatchesBatch on two synthetic VGA frames,
    the second the first moved by a whole number of level-0 pixels; then one trackLKBatch with the forward-backward
    check."""
    import torch
    from pislam_amd import frontend as F
    from pislam_amd import synth
    shift = (5, -3)
    big = np.stack([synth.make_level0(3), synth.make_level0(4)])
    frames_prev = big
    frames_next = np.roll(big, (shift[1], shift[0]), axis=(1, 2))          # next(x, y) = prev(x - dx, y - dy) away from the rim
    pb = F.PyramidBuilder(640, 480, ctx=dev.ctx)
    pyr = [torch.zeros((2, pb.rows, pb.vstep), dtype=torch.uint8, device="cuda") for _ in range(2)]
    pb(dev.up(frames_prev), pyr[0])
    pb(dev.up(frames_next), pyr[1])
    levels, scales = pb.levels, F.level_scales_q16(pb.levels)
    assert scales == chain_scales(pb.levels)
    fe = F.OrbFrontend(levels, pb.vstep, pb.rows, max_keypoints=4096, ctx=dev.ctx)
    q, t = fe.alloc_outputs(2, "cuda"), fe.alloc_outputs(2, "cuda")
    fe(pyr[0], *q)
    fe(pyr[1], *t)
    idx, dist, dist2 = F.matchHammingWindowBatch(q[0], q[1], q[2], t[0], t[1], t[2], levels, 8, ctx=dev.ctx)
    sel = F.selectMatchesBatch(idx, dist, dist2, q[2], t[2], t_stride=4096, ctx=dev.ctx)
    prm = dict(win_radius=7, max_iters=10, eps_q8=8, max_step_q8=2048, min_eig=16, max_err=0)
    dev.ctx.synchronize()
    torch.cuda.synchronize()
    nq, st, er, nt = F.refineMatchesBatch(pyr[0], pyr[1], q[0], q[2], t[0], idx, levels, scales, sel=sel[:3], ctx=dev.ctx, **prm)
    dev.ctx.synchronize()
    nq, st = nq.cpu().numpy(), st.cpu().numpy().view(np.uint32)
    qk, tk = q[0].cpu().numpy().view(np.uint32).astype(np.int64), t[0].cpu().numpy().view(np.uint32).astype(np.int64)
    qn, nsel = q[2].cpu().numpy(), sel[2].cpu().numpy()
    sq, stt = sel[0].cpu().numpy(), sel[1].cpu().numpy()
    prev_np, nxt_np = pyr[0].cpu().numpy(), pyr[1].cpu().numpy()
    lv = norm_levels(levels)

    def level_of(x, y):
        return next(l for l, (w, h, r0, c0) in enumerate(lv) if c0 <= x < c0 + w and r0 <= y < r0 + h)

    assert nsel.min() > 200
    # unselected queries are left at status 1, selected ones are not
    for b in range(2):
        chosen = np.zeros(4096, bool)
        chosen[sq[b, :nsel[b]]] = True
        assert ((st[b, :qn[b]] & 255)[~chosen[:qn[b]]] == 1).all() and (st[b, :qn[b]][~chosen[:qn[b]]] >> 8 == 0).all()
    # the expectation on a subsample of 200 matches: the guess is the matched train keypoint mapped to the query's level
    rng = np.random.default_rng(17)
    picks = [(b, int(k)) for b in range(2) for k in rng.choice(nsel[b], 100, replace=False)]
    ref_prm = Lk(7, 10, 8, 2048, 1, 0, 16, 0)
    dev_l0, dev_all, tracked = [], [], 0
    for b, k in picks:
        i, j = int(sq[b, k]), int(stt[b, k])
        qx, qy, tx, ty = (qk[b, i] >> 12) & 0xFFF, qk[b, i] & 0xFFF, (tk[b, j] >> 12) & 0xFFF, tk[b, j] & 0xFFF
        lq, lt = level_of(qx, qy), level_of(tx, ty)
        g = (map_level((tx - lv[lt][3]) << 8, scales[lt], scales[lq]) + (lv[lq][3] << 8),
             map_level((ty - lv[lt][2]) << 8, scales[lt], scales[lq]) + (lv[lq][2] << 8))
        x, y, s, _ = ref_point(lv, scales, prev_np[b], nxt_np[b], (int(qx) << 8, int(qy) << 8), g, ref_prm)
        assert (int(nq[b, i, 0]), int(nq[b, i, 1]), int(st[b, i])) == (x, y, s), (b, i)
        if s & 255 == 0:
            tracked += 1
            e = max(abs((x - (qx << 8)) / 256 - shift[0] * 65536 / scales[lq]), abs((y - (qy << 8)) / 256 - shift[1] * 65536 / scales[lq]))
            dev_all.append(e)
            if lq == 0:
                dev_l0.append(e)
    tol = max(dev_all)                  # what the expectation gives on this input, plus nothing: parity is exact
    print("end to end: %d of 200 tracked; deviation from the shift: level 0 worst %.4f px, all levels worst %.4f px"
          % (tracked, max(dev_l0), tol))
    assert tracked >= 150 and len(dev_l0) >= 20
    # level 0 is the blurred frame, the blur commutes with a whole-pixel shift: as exact as anchor (a)
    assert max(dev_l0) <= 1 / 16
    for b, k in picks:
        i = int(sq[b, k])
        if st[b, i] & 255 == 0:
            lq = level_of((qk[b, i] >> 12) & 0xFFF, qk[b, i] & 0xFFF)
            for a in range(2):
                kp = ((qk[b, i] >> 12) & 0xFFF, qk[b, i] & 0xFFF)[a] << 8
                assert abs((int(nq[b, i, a]) - kp) / 256 - shift[a] * 65536 / scales[lq]) <= tol
    # forward-backward: the mask equals the one from two runs of the expectation (first 100 keypoints of each pair)
    S = 100
    pts = F.keypointsToQ8(q[0][:, :S].contiguous())
    pts[:, S - 5:] = -256                                   # five points in no level: the mask is false there
    cnt = torch.full((2,), S, dtype=torch.int32, device="cuda")
    fb = 64
    out = F.trackLKBatch(pyr[0], pyr[1], pts, cnt, levels, scales, fb_max_q8=fb, ctx=dev.ctx)
    dev.ctx.synchronize()
    assert len(out) == 5
    pts_np = F.keypointsToQ8(qk[:, :S].astype(np.uint32)).astype(np.int64)
    pts_np[:, S - 5:] = -256
    cn = np.array([S, S], np.uint32)
    fwd = ref_batch(lv, scales, prev_np, nxt_np, pts_np, cn, None, DEFAULTS)
    bwd = ref_batch(lv, scales, nxt_np, prev_np, fwd[0].astype(np.int64), cn, None, DEFAULTS)
    mask = ((fwd[1] & 255) == 0) & ((bwd[1] & 255) == 0) & (np.abs(bwd[0].astype(np.int64) - pts_np) <= fb).all(-1)
    assert (out[0].cpu().numpy() == fwd[0]).all() and (out[1].cpu().numpy().view(np.uint32) == fwd[1]).all()
    assert (out[4].cpu().numpy() == mask).all() and mask[:, :S - 5].any() and not mask[:, S - 5:].any()
