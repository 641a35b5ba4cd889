"""Scale-aware guided window matching (pislam_match_hamming_scaled_window_batch).

The semantics are the library's own (include/pislam_hip.h).  `ref_scaled_window_match` below states them independently
of the library and of its cell index: level ids by rectangle containment, the Q16 mapping to level-0 coordinates, an
nq x nt candidate mask (level span and the query level's radius around the window centre) and a masked minimum of
dist * 65536 + j for best and second.  The CPU tests check that reference itself, against the windowed matcher's
reference (test_match_window.ref_window_match) and on hand-built cases; the GPU tests compare the library with it bit
for bit."""
import ctypes

import numpy as np
import pytest

from conftest import DEMO_LEVELS
from test_match_window import (COUNT_INVALID, NONE_U32, SENTINEL, _lv, clamp_count, frontend_outputs, level_ids, pack,
                               packed_levels, random_descriptors, random_positions, ref_window_match, scaled_radii)

BIG = np.int64(1) << 40
PRED_LIMIT = 1 << 20


def map_q16(u, scale):
    """Level-0 coordinate of level-local u: (u * s + 32768) >> 16 in unsigned 32-bit arithmetic."""
    return ((np.asarray(u, np.int64) * np.asarray(scale, np.int64) + 32768) & 0xFFFFFFFF) >> 16


def mapped_positions(pos, levels, scale_q16):
    """(level id or -1, X, Y) of packed positions; X, Y are 0 for positions in no level."""
    lid, x, y = level_ids(pos, levels)
    lv = np.array([_lv(t) for t in levels], np.int64).reshape(-1, 4)
    s = np.asarray(scale_q16, np.int64)
    k = np.maximum(lid, 0)
    X = np.where(lid >= 0, map_q16(np.maximum(x - lv[k, 3], 0), s[k]), 0)
    Y = np.where(lid >= 0, map_q16(np.maximum(y - lv[k, 2], 0), s[k]), 0)
    return lid, X, Y


def hamming(qd, td):
    """nq x nt Hamming distances (bit unpacking; float32 products of 0/1 sums below 2^24 are exact)."""
    qb = np.unpackbits(np.ascontiguousarray(qd, np.uint32).view(np.uint8), axis=1).astype(np.float32)
    tb = np.unpackbits(np.ascontiguousarray(td, np.uint32).view(np.uint8), axis=1).astype(np.float32)
    return (qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2 * (qb @ tb.T)).astype(np.int64)


def ref_scaled_window_match(qkp, qd, tkp, td, levels, scale_q16, radius0, span, qpred=None, d=None):
    """(idx int32, dist uint32, dist2 uint32) [nq] of one pair.  qpred: [nq][2] int level-0 centres or None;
    d: the nq x nt Hamming matrix when the caller already has it."""
    nq, nt = len(qkp), len(tkp)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE_U32, np.uint32)
    dist2 = np.full(nq, NONE_U32, np.uint32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2
    rad = np.asarray([radius0] * len(levels) if np.isscalar(radius0) else radius0, np.int64)
    lq, Xq, Yq = mapped_positions(qkp, levels, scale_q16)
    lt, Xt, Yt = mapped_positions(tkp, levels, scale_q16)
    if qpred is not None:
        p = np.clip(np.asarray(qpred, np.int64).reshape(nq, 2), -PRED_LIMIT, PRED_LIMIT)
        Xq, Yq = p[:, 0], p[:, 1]
    if d is None:
        d = hamming(qd, td)
    r = rad[np.maximum(lq, 0)][:, None]
    mask = ((lq[:, None] >= 0) & (lt[None, :] >= 0) & (np.abs(lq[:, None] - lt[None, :]) <= span)
            & (np.abs(Xq[:, None] - Xt[None, :]) <= r) & (np.abs(Yq[:, None] - Yt[None, :]) <= r))
    key = np.where(mask, d * 65536 + np.arange(nt, dtype=np.int64)[None, :], BIG)
    rows = np.arange(nq)
    am = key.argmin(1)
    best = key[rows, am]
    key[rows, am] = BIG
    second = key.min(1)
    has, has2 = best < BIG, second < BIG
    idx[:] = np.where(has, best % 65536, -1)
    dist[:] = np.where(has, best // 65536, 0xFFFFFFFF).astype(np.uint32)
    dist2[:] = np.where(has2, second // 65536, 0xFFFFFFFF).astype(np.uint32)
    return idx, dist, dist2


def level_scales(levels):
    from pislam_amd.frontend import level_scales_q16
    return level_scales_q16(levels)


def scale_radii(scale_q16, r0=15):
    """radius0[l] = round(r0 * s_l / 65536): r0 level pixels on every level, in level-0 pixels."""
    return [int(np.floor(r0 * s / 65536 + 0.5)) for s in scale_q16]


# ---- CPU: the reference itself -----------------------------------------------------------------------------------
def test_level_scales_q16_of_the_demo_pyramid():
    s = level_scales(DEMO_LEVELS)
    assert s[0] == 65536 and all(a < b for a, b in zip(s, s[1:]))
    assert s == [(2 * 65536 * 640 + w) // (2 * w) for (w, _, _) in DEMO_LEVELS]
    assert abs(s[1] / 65536 - 1.2) < 0.01 and abs(s[7] / 65536 - 1.2 ** 7) < 0.05


@pytest.mark.parametrize("layout", ["demo", "packed"])
def test_reference_reduces_to_the_windowed_reference(layout):
    """span 0, every scale 65536, no prediction and radius0 = radius: the windowed matcher's semantics."""
    levels = DEMO_LEVELS if layout == "demo" else packed_levels()
    rng = np.random.default_rng(11 if layout == "demo" else 12)
    for words, nq, nt in [(1, 300, 400), (8, 250, 300), (2, 40, 1), (4, 1, 60)]:
        for radius in (0, 3, 15, scaled_radii(15, len(levels)), 4095):
            tkp = random_positions(rng, nt, levels, radius)
            qkp = random_positions(rng, nq, levels, radius)
            qkp[: nq // 2] = tkp[rng.integers(0, nt, nq // 2)] + np.uint32(rng.integers(0, 3) << 12)
            td = random_descriptors(rng, nt, words)
            qd = random_descriptors(rng, nq, words)
            rad = [radius] * len(levels) if np.isscalar(radius) else radius
            got = ref_scaled_window_match(qkp, qd, tkp, td, levels, [65536] * len(levels), rad, 0)
            exp = ref_window_match(qkp, qd, tkp, td, levels, radius)
            for g, e in zip(got, exp):
                assert (g == e).all(), (layout, words, radius)


def test_reference_hand_built_cases():
    levels = [(200, 100, 0, 0), (100, 50, 100, 0)]      # level 1 is half the size: scale 2.0
    s = [65536, 131072]
    z = lambda n: np.zeros((n, 1), np.uint32)
    one = np.ones((1, 1), np.uint32)
    # a twin one level up: query on level 0 at (40, 20), train on level 1 at local (20, 10) -> level-0 (40, 20)
    q, t = pack([40], [20]), pack([20], [100 + 10])
    for span, want in ((0, -1), (1, 0)):
        i, d, d2 = ref_scaled_window_match(q, z(1), t, z(1), levels, s, [2, 2], span)
        assert i[0] == want
    # the same from level 1: the query's radius (radius0[1]) decides, not the train's
    i, _, _ = ref_scaled_window_match(pack([21], [110]), z(1), pack([40], [20]), z(1), levels, s, [0, 2], 1)
    assert i[0] == 0                                    # (21, 10) on level 1 -> (42, 20): 2 px from (40, 20)
    i, _, _ = ref_scaled_window_match(pack([40], [20]), z(1), pack([21], [110]), z(1), levels, s, [1, 5], 1)
    assert i[0] == -1
    # a prediction moves the window onto one train point and off another
    t = pack([10, 150], [10, 80])
    i, _, _ = ref_scaled_window_match(pack([12], [10]), z(1), t, z(2), levels, s, [3, 3], 0)
    assert i[0] == 0
    i, _, _ = ref_scaled_window_match(pack([12], [10]), z(1), t, z(2), levels, s, [3, 3], 0, qpred=[[148, 82]])
    assert i[0] == 1
    # the prediction is clamped to [-2^20, 2^20], and a far one finds nothing
    i, _, _ = ref_scaled_window_match(pack([12], [10]), z(1), t, z(2), levels, s, [65535, 65535], 0,
                                      qpred=[[-(2 ** 31), 2 ** 31 - 1]])
    assert i[0] == -1
    # window edges in level-0 pixels: inclusive at R, excluded at R + 1 (level 1: local 10 -> 20, 13 -> 26, 14 -> 28)
    t = pack([13, 14, 10], [110, 110, 113])
    i, d, d2 = ref_scaled_window_match(pack([20], [20]), z(1), t, np.array([[1], [0], [3]], np.uint32), levels, s,
                                       [6, 6], 1)
    assert (i[0], d[0], d2[0]) == (0, 1, 2)             # (26, 20) at |dx| = 6 and (20, 26) at |dy| = 6; (28, 20) not
    for R, want in ((7, -1), (8, 0)):                   # (28, 20) alone: excluded at |dx| = R + 1, inclusive at R
        i, _, _ = ref_scaled_window_match(pack([20], [20]), z(1), t[1:2], z(1), levels, s, [R, R], 1)
        assert i[0] == want
    # Q16 rounding at a .5 boundary: scale 1.5 maps local 1 -> (98304 + 32768) >> 16 = 2 and local 3 -> 5 (4.5 up)
    lv15 = [(100, 100, 0, 0), (60, 60, 100, 0)]
    s15 = [65536, 98304]
    assert list(map_q16([1, 3, 5], 98304)) == [2, 5, 8]
    i, _, _ = ref_scaled_window_match(pack([5], [0]), z(1), pack([3], [100]), z(1), lv15, s15, [0, 0], 1)
    assert i[0] == 0                                    # 4.5 rounds up to 5
    i, _, _ = ref_scaled_window_match(pack([4], [0]), z(1), pack([3], [100]), z(1), lv15, s15, [0, 0], 1)
    assert i[0] == -1
    # a query in no level has no candidates, with or without a prediction
    for qp in (None, [[40, 20]]):
        i, d, d2 = ref_scaled_window_match(pack([300], [300]), z(1), pack([40], [20]), z(1), levels, s, [65535, 65535],
                                           1, qpred=qp)
        assert (i[0], d[0], d2[0]) == (-1, NONE_U32, NONE_U32)
    # equal distances: the smallest train index wins, dist2 is the duplicate's distance
    td = np.array([[7], [1], [3], [1]], np.uint32)
    i, d, d2 = ref_scaled_window_match(pack([10], [10]), z(1), pack([11, 12, 13, 9], [10, 10, 10, 10]), td, levels, s,
                                       [3, 3], 0)
    assert (i[0], d[0], d2[0]) == (1, 1, 1)
    # exactly one candidate: dist2 stays "none"
    i, d, d2 = ref_scaled_window_match(pack([10], [10]), one, pack([10, 190], [10, 90]), z(2), levels, s, [3, 3], 0)
    assert (i[0], d[0], d2[0]) == (0, 1, NONE_U32)


# ---- GPU ---------------------------------------------------------------------------------------------------------
PAIRS = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (1000, 1000), (1000, 1), (1, 1000), (64, 0)]


def arbitrary_scales(rng, levels):
    """Scales of all sizes inside the limits: shrinking, unit, growing, and the largest the extent allows."""
    out = []
    for t in levels:
        w, h, _, _ = _lv(t)
        top = min(1 << 20, (65536 * 65536 - 32768) // max(1, max(w, h) - 1) - 1)
        out.append(int(rng.choice([1, int(rng.integers(2, 65536)), 65536, int(rng.integers(65536, top + 1)), top])))
    return out


def run_scaled(ctx, levels, scale_q16, radius0, span, qkp, qd, qc, tkp, td, tc, qpred=None, fill=SENTINEL):
    """Host arrays in, host arrays out: (idx, dist, dist2) [batch][q_stride] as uint32 bit patterns."""
    import torch
    from pislam_amd.frontend import matchHammingScaledWindowBatch
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    B, qs = qkp.shape
    outs = [torch.full((B, qs), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device=dev) for _ in range(3)]
    qp = None if qpred is None else T(np.asarray(qpred, np.int64).astype(np.int32))
    matchHammingScaledWindowBatch(T(qkp), T(qd), T(qc), T(tkp), T(td), T(tc), levels, scale_q16, radius0, span, qp, *outs,
                                  ctx=ctx)
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in outs]


def check_against_reference(got, levels, scale_q16, radius0, span, qkp, qd, qc, tkp, td, tc, qpred=None, fill=SENTINEL,
                            dmats=None):
    gi, gd, g2 = got
    qs, ts = qkp.shape[1], tkp.shape[1]
    for b in range(qkp.shape[0]):
        nq, nt = clamp_count(qc[b], qs), clamp_count(tc[b], ts)
        d = None if dmats is None else dmats[b]
        p = None if qpred is None else np.asarray(qpred)[b, :nq]
        ei, ed, e2 = ref_scaled_window_match(qkp[b, :nq], qd[b, :nq], tkp[b, :nt], td[b, :nt], levels, scale_q16, radius0,
                                             span, qpred=p, d=d)
        bad = np.flatnonzero(gi[b, :nq].view(np.int32) != ei)[:5]
        assert (gi[b, :nq].view(np.int32) == ei).all(), (b, span, bad)
        assert (gd[b, :nq] == ed).all(), (b, span)
        assert (g2[b, :nq] == e2).all(), (b, span)
        for g in (gi, gd, g2):
            assert (g[b, nq:] == fill).all(), ("slot past the query count written", b)


def scaled_queries(rng, tkp_b, nq, levels, scale_q16, radius0, span):
    """Queries of which half sit near a train entry in level-0 pixels, on a level within span of the entry's (window
    edges: offsets R - 1 .. R + 1 in level-0 pixels), the rest anywhere."""
    q = random_positions(rng, nq, levels, 15)
    if len(tkp_b) == 0 or nq == 0:
        return q
    lv = [_lv(t) for t in levels]
    lt, Xt, Yt = mapped_positions(tkp_b, levels, scale_q16)
    src = rng.integers(0, len(tkp_b), nq)
    for k in np.flatnonzero(rng.random(nq) < 0.5):
        j = src[k]
        if lt[j] < 0:
            continue
        l = int(np.clip(lt[j] + rng.integers(-span, span + 1), 0, len(lv) - 1))
        w, h, r0, c0 = lv[l]
        R = int(radius0[l])
        o = [int(rng.choice([0, 1, -1, R, -R, R + 1, -R - 1])) for _ in range(2)]
        u = int(np.clip(np.floor((Xt[j] + o[0]) * 65536 / scale_q16[l] + rng.integers(-1, 2)), 0, w - 1))
        v = int(np.clip(np.floor((Yt[j] + o[1]) * 65536 / scale_q16[l] + rng.integers(-1, 2)), 0, h - 1))
        q[k] = pack([c0 + u], [r0 + v])[0]
    return q


def random_predictions(rng, qkp_b, tkp_b, levels, scale_q16, radius0):
    """[nq][2] centres: near a train entry's mapped position (window edges), anywhere, or far outside the clamp."""
    nq = len(qkp_b)
    p = rng.integers(-100, 70000, (nq, 2))
    lq, _, _ = mapped_positions(qkp_b, levels, scale_q16)
    if len(tkp_b):
        _, Xt, Yt = mapped_positions(tkp_b, levels, scale_q16)
        j = rng.integers(0, len(tkp_b), nq)
        R = np.asarray(radius0, np.int64)[np.maximum(lq, 0)]
        near = rng.random(nq) < 0.6
        off = rng.choice([-1, 0, 1], (nq, 2)) * (R[:, None] + rng.integers(0, 2, (nq, 2)))
        p = np.where(near[:, None], np.stack([Xt[j], Yt[j]], 1) + off, p)
    far = rng.random(nq) < 0.05
    p[far] = rng.choice([-(2 ** 31), 2 ** 31 - 1, -(2 ** 20) - 5, 2 ** 20 + 5], (int(far.sum()), 2))
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["demo", "packed"])
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_scaled_random_positions(gpu_ctx, layout, words):
    levels = DEMO_LEVELS if layout == "demo" else packed_levels()
    nl = len(levels)
    stride, B = 1000, len(PAIRS)
    rng = np.random.default_rng([words, nl])
    qc = np.array([p[0] for p in PAIRS], np.uint32)
    tc = np.array([p[1] for p in PAIRS], np.uint32)
    for span in (0, 1, 2):
        for scales in ("levels", "arbitrary"):
            s = level_scales(levels) if scales == "levels" else arbitrary_scales(rng, levels)
            r = scale_radii(s) if scales == "levels" else [int(v) for v in rng.choice([0, 1, 7, 30, 200], nl)]
            qkp = np.zeros((B, stride), np.uint32)
            tkp = np.zeros((B, stride), np.uint32)
            qd = np.zeros((B, stride, words), np.uint32)
            td = np.zeros((B, stride, words), np.uint32)
            pred = np.zeros((B, stride, 2), np.int64)
            own = np.zeros((B, stride, 2), np.int64)
            for b, (nq, nt) in enumerate(PAIRS):
                tkp[b, :nt] = random_positions(rng, nt, levels, 15)
                td[b, :nt] = random_descriptors(rng, nt, words)
                qkp[b, :nq] = scaled_queries(rng, tkp[b, :nt], nq, levels, s, r, span)
                qd[b, :nq] = random_descriptors(rng, nq, words)
                if nt and nq:                               # half of the queries carry a train entry's descriptor
                    near = rng.random(nq) < 0.5
                    qd[b, :nq] = np.where(near[:, None], td[b, rng.integers(0, nt, nq)], qd[b, :nq])
                pred[b, :nq] = random_predictions(rng, qkp[b, :nq], tkp[b, :nt], levels, s, r)
                _, X, Y = mapped_positions(qkp[b], levels, s)
                own[b] = np.stack([X, Y], 1)
            dm = [hamming(qd[b, :clamp_count(qc[b], stride)], td[b, :clamp_count(tc[b], stride)]) for b in range(B)]
            got_none = run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc)
            check_against_reference(got_none, levels, s, r, span, qkp, qd, qc, tkp, td, tc, dmats=dm)
            got = run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc, qpred=pred)
            check_against_reference(got, levels, s, r, span, qkp, qd, qc, tkp, td, tc, qpred=pred, dmats=dm)
            got_own = run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc, qpred=own)
            for a, g in zip(got_none, got_own):                 # the query's own mapped position = no prediction
                assert (a == g).all(), (span, scales)


@pytest.mark.gpu
def test_gpu_scaled_full_train_stride(gpu_ctx):
    """t_stride = 65535 (the largest index the dist << 16 | index key holds), one pair filled to the stride."""
    rng = np.random.default_rng(65535)
    levels = DEMO_LEVELS
    s = level_scales(levels)
    r = scale_radii(s)
    ts, qs, words = 65535, 70, 4
    tkp = np.zeros((2, ts), np.uint32)
    td = np.zeros((2, ts, words), np.uint32)
    tkp[0] = pack(rng.integers(0, 640, ts), rng.integers(0, 480, ts))                   # level 0: ~0.2 entries / px
    tkp[1, :100] = random_positions(rng, 100, levels, 15)
    td[0] = random_descriptors(rng, ts, words)
    td[1, :100] = random_descriptors(rng, 100, words)
    qkp = np.zeros((2, qs), np.uint32)
    qd = np.zeros((2, qs, words), np.uint32)
    qkp[0, :65] = tkp[0, ts - 65:]                                                       # find the last indices
    qd[0, :65] = td[0, ts - 65:]
    qkp[0, 65:] = pack([0, 639, 0, 178, 100], [0, 0, 479, 2076 + 133, 2000])           # corners, levels 6 and 7
    qkp[1] = random_positions(rng, qs, levels, 15)
    qd[1] = random_descriptors(rng, qs, words)
    qc = np.array([qs, qs], np.uint32)
    tc = np.array([ts, 100], np.uint32)
    for span in (0, 1, 7):
        got = run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc)
        check_against_reference(got, levels, s, r, span, qkp, qd, qc, tkp, td, tc)
        assert (got[0][0, :65].view(np.int32) >= ts - 65).all() and (got[1][0, :65] == 0).all()


@pytest.mark.gpu
def test_gpu_scaled_on_frontend_outputs(gpu_ctx):
    """Pyramid k against k + 1 of the front end's own outputs, with ragged counts, one empty train side and one query
    count above the stride (clamped).  At span 0 with unit scales and no prediction the outputs are bit-identical
    to the windowed matcher's on the same buffers."""
    import torch
    from pislam_amd.frontend import matchHammingScaledWindowBatch, matchHammingWindowBatch
    B = 8
    levels, kp, desc, counts = frontend_outputs(B + 1)
    assert counts.min() > 100
    qkp, qd, qc = kp[:B].copy(), desc[:B].copy(), counts[:B].copy()
    tkp, td, tc = kp[1:].copy(), desc[1:].copy(), counts[1:].copy()
    tc[2] = 0
    qc[3] = 3000
    s = level_scales(levels)
    r = scale_radii(s)
    for span in (0, 1, 2):
        got = run_scaled(gpu_ctx, levels, s, r, span, qkp, qd, qc, tkp, td, tc)
        check_against_reference(got, levels, s, r, span, qkp, qd, qc, tkp, td, tc)
        nq = int(min(qc[0], kp.shape[1]))
        assert (got[0][0, :nq].view(np.int32) >= 0).any()
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    args = [T(a) for a in (qkp, qd, qc, tkp, td, tc)]
    nl = len(levels)
    for radius in (scaled_radii(15, nl), 40):
        win = matchHammingWindowBatch(*args, levels, radius, ctx=gpu_ctx)
        rad = [radius] * nl if np.isscalar(radius) else radius
        sc = matchHammingScaledWindowBatch(*args, levels, [65536] * nl, rad, 0, ctx=gpu_ctx)
        torch.cuda.synchronize()
        for b in range(B):
            n = clamp_count(qc[b], kp.shape[1])
            for w, x in zip(win, sc):
                assert torch.equal(w[b, :n], x[b, :n]), (b, radius)


@pytest.mark.gpu
def test_gpu_scaled_scale_change_property(gpu_ctx):
    """Train = the query keypoints of levels >= 1 moved one level down (same level-local coordinates and
    descriptors; level-0 keypoints left out), qpred = each twin's mapped position plus an offset below the radius.
    With span >= 1 every query on a level >= 1 finds distance 0 on an identical descriptor at an index <= its twin's;
    with span 0 no query returns its twin's index."""
    B = 4
    levels, kp, desc, counts = frontend_outputs(B, seed=90)
    lv = np.array([_lv(t) for t in levels], np.int64)
    s = level_scales(levels)
    r = scale_radii(s)
    qs = kp.shape[1]
    tkp = np.zeros_like(kp)
    td = np.zeros_like(desc)
    tc = np.zeros(B, np.uint32)
    pred = np.zeros((B, qs, 2), np.int64)
    twin = np.full((B, qs), -1, np.int64)
    rng = np.random.default_rng(5)
    for b in range(B):
        n = min(int(counts[b]), qs)
        lid, x, y = level_ids(kp[b, :n], levels)
        assert (lid >= 1).sum() > 50
        up = np.flatnonzero(lid >= 1)
        l1 = lid[up] - 1
        u, v = x[up] - lv[lid[up], 3], y[up] - lv[lid[up], 2]
        tkp[b, :len(up)] = pack(lv[l1, 3] + u, lv[l1, 2] + v)
        td[b, :len(up)] = desc[b, up]
        tc[b] = len(up)
        twin[b, up] = np.arange(len(up))
        R = np.asarray(r)[lid[up]]
        off = np.stack([rng.integers(-R + 1, R), rng.integers(-R + 1, R)], 1)
        pred[b, up] = np.stack([map_q16(u, np.asarray(s)[l1]), map_q16(v, np.asarray(s)[l1])], 1) + off
    for span in (1, 2, 0):
        gi, gd, g2 = run_scaled(gpu_ctx, levels, s, r, span, kp, desc, counts, tkp, td, tc, qpred=pred)
        if span == 1:
            check_against_reference((gi, gd, g2), levels, s, r, span, kp, desc, counts, tkp, td, tc, qpred=pred)
        for b in range(B):
            n = min(int(counts[b]), qs)
            up = np.flatnonzero(twin[b, :n] >= 0)
            i = gi[b, up].view(np.int32)
            if span:
                assert (gd[b, up] == 0).all() and (i >= 0).all() and (i <= twin[b, up]).all(), (b, span)
                assert (td[b, i] == desc[b, up]).all()
            else:
                assert (i != twin[b, up]).all(), b


@pytest.mark.gpu
def test_gpu_scaled_invalid_counts_and_untouched_slots(gpu_ctx):
    """PISLAM_COUNT_INVALID on either side counts as 0; output slots at and past the query count keep their fill."""
    rng = np.random.default_rng(3)
    levels, words, n = DEMO_LEVELS, 2, 128
    s = level_scales(levels)
    qkp = np.stack([random_positions(rng, n, levels, 15) for _ in range(4)])
    tkp = np.stack([random_positions(rng, n, levels, 15) for _ in range(4)])
    tkp[:, :n // 2] = qkp[:, :n // 2]
    qd = np.stack([random_descriptors(rng, n, words) for _ in range(4)])
    td = np.stack([random_descriptors(rng, n, words) for _ in range(4)])
    qc = np.array([COUNT_INVALID, 100, 100, 50], np.uint32)
    tc = np.array([100, COUNT_INVALID, 100, 0], np.uint32)
    for fill in (SENTINEL, 0xFFFFFFFF, 0):
        got = run_scaled(gpu_ctx, levels, s, 20, 1, qkp, qd, qc, tkp, td, tc, fill=fill)
        check_against_reference(got, levels, s, 20, 1, qkp, qd, qc, tkp, td, tc, fill=fill)
        gi, gd, g2 = got
        assert (gi[0] == fill).all() and (gd[0] == fill).all() and (g2[0] == fill).all()     # no query: nothing written
        assert (gi[1, :100].view(np.int32) == -1).all() and (gd[1, :100] == NONE_U32).all()  # no train entry
        assert (gi[2, :100].view(np.int32) >= 0).any()


@pytest.mark.gpu
def test_gpu_scaled_rejects_bad_arguments(gpu_ctx):
    """Every invalid argument returns PISLAM_ERR_INVALID and leaves the outputs as they were."""
    import torch
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import matchHammingScaledWindowBatch, reserveMatchScaledWindow
    dev = torch.device("cuda:0")
    kp = torch.zeros((2, 16), dtype=torch.int32, device=dev)
    desc = torch.zeros((2, 16, 8), dtype=torch.int32, device=dev)
    cnt = torch.full((2,), 16, dtype=torch.int32, device=dev)
    pred = torch.zeros((2, 16, 2), dtype=torch.int32, device=dev)
    lv = DEMO_LEVELS
    s = level_scales(lv)
    outs = [torch.full((2, 16), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]

    def call(qd=desc, tk=kp, td=desc, levels=lv, scale=s, radius=15, span=1, qk=kp, qc=cnt, tc=cnt, qp=pred):
        matchHammingScaledWindowBatch(qk, qd, qc, tk, td, tc, levels, scale, radius, span, qp, *outs, ctx=gpu_ctx)

    call()                                                                  # the baseline call is accepted
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(SENTINEL)
    d3 = torch.zeros((2, 16, 3), dtype=torch.int32, device=dev)
    big_kp = torch.zeros((2, 65536), dtype=torch.int32, device=dev)
    big_desc = torch.zeros((2, 65536, 8), dtype=torch.int32, device=dev)
    bad = [dict(qd=d3, td=d3),                                              # words 3
           dict(tk=big_kp, td=big_desc),                                    # t_stride 65536
           dict(radius=-1), dict(radius=65536), dict(radius=[15] * 7 + [65536]),
           dict(span=-1), dict(span=8),                                     # span outside 0..nlevels-1
           dict(levels=lv[:1], scale=s[:1], span=1),
           dict(levels=[], scale=[], radius=[], span=0), dict(levels=[(10, 10, 10 * i, 0) for i in range(17)],
                                                              scale=[65536] * 17, span=0),
           dict(levels=[(640, 480, 0, 0), (100, 100, 479, 0)], scale=[65536, 65536]),     # overlapping rectangles
           dict(levels=[(100, 100, 0, 0), (100, 100, 50, 50)], scale=[65536, 65536]),
           dict(levels=[(4000, 100, 0, 100)], scale=[65536], span=0),                    # past 12-bit x
           dict(scale=0), dict(scale=-65536), dict(scale=(1 << 20) + 1), dict(scale=s[:7] + [(1 << 20) + 1]),
           dict(qk=kp.cpu(), qd=desc.cpu(), qc=cnt.cpu()),                  # host tensors
           dict(tk=kp.cpu(), td=desc.cpu(), tc=cnt.cpu()),
           dict(qp=pred.cpu())]
    for kw in bad:
        with pytest.raises(PislamError):
            call(**kw)
    torch.cuda.synchronize()
    for o in outs:                                                          # nothing was launched or written
        assert (o == SENTINEL).all()
    for kw in (dict(words=3), dict(t_stride=65536), dict(radius=65536), dict(span=8), dict(scale=0)):
        args = dict(levels=lv, scale=s, radius=15, span=1, t_stride=16, batch=2, words=8)
        args.update(kw)
        with pytest.raises(PislamError):
            reserveMatchScaledWindow(args.pop("levels"), args.pop("scale"), args.pop("radius"), args.pop("span"),
                                     args.pop("t_stride"), args.pop("batch"), ctx=gpu_ctx, **args)
    # the largest scale the limits allow on a 12-bit level is accepted (mapped extent 65520)
    call(levels=[(4096, 4096, 0, 0)], scale=1 << 20, radius=65535, span=0)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_scaled_call_is_hipgraph_capturable(gpu_ctx):
    """After pislam_match_scaled_window_reserve the call allocates nothing and never synchronises: capture one call
    (through the C entry point, with host scale and radius arrays of this test's own) on a side stream, replay it and
    compare with the eager call; then change the host arrays and the inputs, replay and compare with the reference
    for the arrays as they were at capture."""
    import torch
    from pislam_amd.capi import Context, Level
    from pislam_amd.frontend import matchHammingScaledWindowBatch, reserveMatchScaledWindow
    B, span = 4, 1
    levels, kp, desc, counts = frontend_outputs(B + 2, seed=120)
    s = level_scales(levels)
    r = scale_radii(s)
    nl, qs, words = len(levels), kp.shape[1], desc.shape[2]
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    qk, qd, qc = T(kp[:B]), T(desc[:B]), T(counts[:B])
    tk, td, tc = T(kp[1:B + 1]), T(desc[1:B + 1]), T(counts[1:B + 1])
    lv_c = (Level * nl)(*[Level(*_lv(t)) for t in levels])
    s_c = (ctypes.c_int32 * nl)(*s)
    r_c = (ctypes.c_int32 * nl)(*r)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchScaledWindow(levels, s, r, span, qs, B, words=words, ctx=ctx)
        outs = [torch.zeros((B, qs), dtype=torch.int32, device=dev) for _ in range(3)]

        def capi_call():
            ctx.check(ctx.lib.pislam_match_hamming_scaled_window_batch(
                ctx.h, words, lv_c, nl, s_c, r_c, span, qk.data_ptr(), qd.data_ptr(), qc.data_ptr(), None, qs,
                tk.data_ptr(), td.data_ptr(), tc.data_ptr(), qs, B, outs[0].data_ptr(), outs[1].data_ptr(),
                outs[2].data_ptr()), "pislam_match_hamming_scaled_window_batch")

        capi_call()                                                          # warm-up (module load)
        side.synchronize()
        eager = matchHammingScaledWindowBatch(qk, qd, qc, tk, td, tc, levels, s, r, span, ctx=ctx)
        side.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a, b)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            capi_call()
        for o in outs:
            o.zero_()
        g.replay()
        side.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a, b)
        # the graph keeps the scales and radii it was captured with; new inputs in the same buffers
        for l in range(nl):
            s_c[l], r_c[l] = 65536, 0
        for o in outs:
            o.zero_()
        qk.copy_(T(kp[1:B + 1])), qd.copy_(T(desc[1:B + 1])), qc.copy_(T(counts[1:B + 1]))
        tk.copy_(T(kp[2:])), td.copy_(T(desc[2:])), tc.copy_(T(counts[2:]))
        g.replay()
        side.synchronize()
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    check_against_reference(got, levels, s, r, span, kp[1:B + 1], desc[1:B + 1], counts[1:B + 1], kp[2:], desc[2:],
                            counts[2:], fill=0)
    assert (got[0].view(np.int32) >= 0).any()
