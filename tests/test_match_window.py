"""Spatially windowed descriptor matching (pislam_match_hamming_window_batch).

The semantics are the library's own (include/pislam_hip.h).  `ref_window_match` below states them independently of
the library and of its cell index: level ids by rectangle containment, an nq x nt window mask, the distance matrix
by bit unpacking (as numpy_match in test_match.py), and a masked minimum of dist * 65536 + j for best and second.
The CPU tests check that reference itself; the GPU tests compare the library with it bit for bit."""
import numpy as np
import pytest

from conftest import DEMO_LEVELS

BIG = np.int64(1) << 40
NONE_U32 = np.uint32(0xFFFFFFFF)
COUNT_INVALID = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A


def _lv(t):
    return (int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 0)


def level_ids(pos, levels):
    """(level id or -1, x, y) of packed positions x << 12 | y (score bits ignored)."""
    pos = np.asarray(pos, np.uint32).astype(np.int64)
    x, y = (pos >> 12) & 0xFFF, pos & 0xFFF
    lid = np.full(len(pos), -1, np.int64)
    for l, t in enumerate(levels):
        w, h, r0, c0 = _lv(t)
        lid[(x >= c0) & (x < c0 + w) & (y >= r0) & (y < r0 + h)] = l
    return lid, x, y


def ref_window_match(qkp, qd, tkp, td, levels, radius):
    """(idx int32, dist uint32, dist2 uint32) [nq] of one pair."""
    nq, nt = len(qkp), len(tkp)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, NONE_U32, np.uint32)
    dist2 = np.full(nq, NONE_U32, np.uint32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2
    rad = np.asarray([radius] * len(levels) if np.isscalar(radius) else radius, np.int64)
    lq, xq, yq = level_ids(qkp, levels)
    lt, xt, yt = level_ids(tkp, levels)
    tb = np.unpackbits(np.ascontiguousarray(td, np.uint32).view(np.uint8), axis=1).astype(np.int32)
    tpop = tb.sum(1)
    jj = np.arange(nt, dtype=np.int64)
    step = max(1, (1 << 22) // nt)                       # query rows per chunk: bounded memory for nt up to 65535
    for a in range(0, nq, step):
        s = slice(a, min(nq, a + step))
        qb = np.unpackbits(np.ascontiguousarray(qd[s], np.uint32).view(np.uint8), axis=1).astype(np.int32)
        d = (qb.sum(1)[:, None] + tpop[None, :] - 2 * (qb @ tb.T)).astype(np.int64)
        r = rad[np.maximum(lq[s], 0)][:, None]
        mask = ((lq[s][:, None] >= 0) & (lq[s][:, None] == lt[None, :])
                & (np.abs(xq[s][:, None] - xt[None, :]) <= r) & (np.abs(yq[s][:, None] - yt[None, :]) <= r))
        key = np.where(mask, d * 65536 + jj[None, :], BIG)
        rows = np.arange(key.shape[0])
        am = key.argmin(1)
        best = key[rows, am]
        key[rows, am] = BIG
        second = key.min(1)
        has, has2 = best < BIG, second < BIG
        idx[s] = np.where(has, best % 65536, -1).astype(np.int32)
        dist[s] = np.where(has, best // 65536, 0xFFFFFFFF).astype(np.uint32)
        dist2[s] = np.where(has2, second // 65536, 0xFFFFFFFF).astype(np.uint32)
    return idx, dist, dist2


def pack(x, y, score=None):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    s = np.zeros_like(x) if score is None else np.asarray(score, np.int64)
    return ((s << 24) | (x << 12) | y).astype(np.uint32)


def scaled_radii(r0, nlevels):
    return [int(round(r0 / 1.2 ** l)) for l in range(nlevels)]


# ---- CPU: the reference itself ---------------------------------------------------------------------------------
def test_reference_with_one_level_and_full_radius_is_the_brute_force_matcher(orc):
    rng = np.random.default_rng(7)
    levels = [(640, 480, 0, 0)]
    for words, nq, nt in [(1, 50, 300), (8, 200, 150), (4, 1, 1), (2, 33, 2)]:
        qkp = pack(rng.integers(0, 700, nq), rng.integers(0, 520, nq), rng.integers(0, 256, nq))   # some outside the level
        tkp = pack(rng.integers(0, 700, nt), rng.integers(0, 520, nt), rng.integers(0, 256, nt))
        qd = rng.integers(0, 2**32, (nq, words), dtype=np.uint64).astype(np.uint32)
        td = rng.integers(0, 2**32, (nt, words), dtype=np.uint64).astype(np.uint32)
        td[nt // 2] = td[0]                                      # a duplicate: ties -> smallest index
        got = ref_window_match(qkp, qd, tkp, td, levels, 4095)
        lq, _, _ = level_ids(qkp, levels)
        lt, _, _ = level_ids(tkp, levels)
        inq, tmap = lq == 0, np.flatnonzero(lt == 0)
        ei, ed, e2 = orc.match_hamming(qd[inq], td[tmap].reshape(len(tmap), words))
        ei = np.where(ei >= 0, tmap[np.maximum(ei, 0)], -1)
        assert (got[0][inq] == ei).all() and (got[1][inq] == ed).all() and (got[2][inq] == e2).all()
        assert (got[0][~inq] == -1).all() and (got[1][~inq] == NONE_U32).all() and (got[2][~inq] == NONE_U32).all()


def test_reference_hand_built_cases():
    d0 = np.zeros((1, 1), np.uint32)
    bits = lambda n: np.uint32((1 << n) - 1)
    # one level, radius 5, query at (50, 50): |dx| = 5 is a candidate, |dx| = 6 or |dy| = 6 is not
    levels = [(100, 100, 0, 0)]
    q = pack([50], [50])
    t = pack([55, 56, 50, 45, 44], [50, 50, 44, 55, 50])
    td = np.array([[bits(7)], [0], [0], [bits(3)], [0]], np.uint32)
    i, d, d2 = ref_window_match(q, d0, t, td, levels, 5)
    assert (i[0], d[0], d2[0]) == (3, 3, 7)
    # the same window on two levels side by side: (99, 10) on level 0 and (100, 10) on level 1 are 1 px apart,
    # and (20, 20) on level 0 / (120, 20) on level 1 are the same level-local position: neither is a candidate
    levels2 = [(100, 100, 0, 0), (50, 50, 0, 100)]
    i, d, d2 = ref_window_match(pack([99, 20], [10, 20]), np.zeros((2, 1), np.uint32), pack([100, 120], [10, 20]),
                                np.zeros((2, 1), np.uint32), levels2, 10)
    assert (i == -1).all() and (d == NONE_U32).all() and (d2 == NONE_U32).all()
    # a query in no level: no candidates even with the full radius
    i, d, d2 = ref_window_match(pack([300], [300]), d0, pack([50], [50]), d0, levels, 4095)
    assert (i[0], d[0], d2[0]) == (-1, NONE_U32, NONE_U32)
    # duplicate descriptors: the smallest index wins, dist2 is the duplicate's distance
    td = np.array([[bits(4)], [bits(1)], [bits(9)], [bits(1)]], np.uint32)
    i, d, d2 = ref_window_match(pack([10], [10]), d0, pack([11, 12, 13, 9], [10, 10, 10, 10]), td, levels, 3)
    assert (i[0], d[0], d2[0]) == (1, 1, 1)
    # exactly one candidate: dist2 stays "none"
    i, d, d2 = ref_window_match(pack([10], [10]), d0, pack([10, 90], [10, 90]), td[:2], levels, 3)
    assert (i[0], d[0], d2[0]) == (0, 4, NONE_U32)


# ---- GPU ---------------------------------------------------------------------------------------------------------
def random_positions(rng, n, levels, radius):
    """Packed positions that exercise the window: uniform inside levels, window edges (offsets r, r + 1 from one
    another), level borders and just outside them, outside every level, and dense clusters."""
    if n == 0:
        return np.zeros(0, np.uint32)
    lv = [_lv(t) for t in levels]
    rad = [radius] * len(lv) if np.isscalar(radius) else list(radius)
    xs, ys = np.zeros(n, np.int64), np.zeros(n, np.int64)
    kind = rng.integers(0, 6, n)
    centre = [(rng.integers(c0, c0 + w), rng.integers(r0, r0 + h)) for (w, h, r0, c0) in lv]
    for k in range(n):
        l = int(rng.integers(0, len(lv)))
        w, h, r0, c0 = lv[l]
        if kind[k] == 0 or kind[k] == 5:                     # uniform
            xs[k], ys[k] = rng.integers(c0, c0 + w), rng.integers(r0, r0 + h)
        elif kind[k] == 1 and k:                             # on / just past the window edge of an earlier position
            r = min(int(rad[l]), 4095)
            o = int(rng.choice([-r - 1, -r, r, r + 1, 0, 1]))
            xs[k] = xs[k - 1] + o
            ys[k] = ys[k - 1] + int(rng.choice([-r - 1, -r, 0, r, r + 1]))
        elif kind[k] == 2:                                   # level borders and one pixel outside
            xs[k] = int(rng.choice([c0 - 1, c0, c0 + w - 1, c0 + w, rng.integers(c0, c0 + w)]))
            ys[k] = int(rng.choice([r0 - 1, r0, r0 + h - 1, r0 + h, rng.integers(r0, r0 + h)]))
        elif kind[k] == 3:                                   # outside every level (12-bit range)
            xs[k], ys[k] = 4095 - int(rng.integers(0, 3)), 4095 - int(rng.integers(0, 3))
        else:                                                # dense cluster: hundreds in one cell
            cx, cy = centre[0]
            xs[k], ys[k] = cx + rng.integers(-2, 3), cy + rng.integers(-2, 3)
    xs, ys = np.clip(xs, 0, 4095), np.clip(ys, 0, 4095)
    return pack(xs, ys, rng.integers(0, 256, n))


def random_descriptors(rng, n, words):
    """Drawn from a small pool with a few flipped bits: many ties and duplicates."""
    pool = rng.integers(0, 2**32, (max(1, n // 4), words), dtype=np.uint64).astype(np.uint32)
    d = pool[rng.integers(0, len(pool), n)]
    flip = np.where(rng.random((n, words)) < 0.3, np.uint32(1) << rng.integers(0, 32, (n, words)).astype(np.uint32), 0)
    return (d ^ flip.astype(np.uint32)).astype(np.uint32)


def run_window(ctx, levels, radius, qkp, qd, qc, tkp, td, tc, fill=SENTINEL):
    """Host arrays in, host arrays out: (idx, dist, dist2) [batch][q_stride] as uint32 bit patterns."""
    import torch
    from pislam_amd.frontend import matchHammingWindowBatch
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    B, qs = qkp.shape
    outs = [torch.full((B, qs), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device=dev) for _ in range(3)]
    matchHammingWindowBatch(T(qkp), T(qd), T(qc), T(tkp), T(td), T(tc), levels, radius, *outs, ctx=ctx)
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in outs]


def clamp_count(c, stride):
    return 0 if int(c) == COUNT_INVALID else min(int(c), stride)


def check_against_reference(got, levels, radius, qkp, qd, qc, tkp, td, tc, fill=SENTINEL):
    gi, gd, g2 = got
    qs, ts = qkp.shape[1], tkp.shape[1]
    for b in range(qkp.shape[0]):
        nq, nt = clamp_count(qc[b], qs), clamp_count(tc[b], ts)
        ei, ed, e2 = ref_window_match(qkp[b, :nq], qd[b, :nq], tkp[b, :nt], td[b, :nt], levels, radius)
        assert (gi[b, :nq].view(np.int32) == ei).all(), (b, radius, np.flatnonzero(gi[b, :nq].view(np.int32) != ei)[:5])
        assert (gd[b, :nq] == ed).all(), (b, radius)
        assert (g2[b, :nq] == e2).all(), (b, radius)
        for g in (gi, gd, g2):
            assert (g[b, nq:] == fill).all(), ("slot past the query count written", b)


PAIRS = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (1000, 1000), (1000, 1), (1, 1000), (64, 0)]


def packed_levels():
    from pislam_amd import synth
    return synth.packed_level_table()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["demo", "packed"])
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_window_random_positions(gpu_ctx, layout, words):
    levels = DEMO_LEVELS if layout == "demo" else packed_levels()
    assert layout == "demo" or any(_lv(t)[3] != 0 for t in levels)
    stride = 1000
    B = len(PAIRS)
    for radius in (0, 1, 15, scaled_radii(15, len(levels)), 4095):
        rng = np.random.default_rng([words, len(levels), 0 if np.isscalar(radius) else 1, int(np.max(radius))])
        qkp = np.zeros((B, stride), np.uint32)
        tkp = np.zeros((B, stride), np.uint32)
        qd = np.zeros((B, stride, words), np.uint32)
        td = np.zeros((B, stride, words), np.uint32)
        qc = np.array([p[0] for p in PAIRS], np.uint32)
        tc = np.array([p[1] for p in PAIRS], np.uint32)
        for b, (nq, nt) in enumerate(PAIRS):
            tkp[b, :nt] = random_positions(rng, nt, levels, radius)
            td[b, :nt] = random_descriptors(rng, nt, words)
            # half of the queries sit near train positions, the rest anywhere
            q = random_positions(rng, nq, levels, radius)
            if nt and nq:
                near = rng.random(nq) < 0.5
                src = tkp[b, rng.integers(0, nt, nq)].astype(np.int64)
                ls, _, _ = level_ids(src, levels)                # offsets on and just past the window edge
                r = np.asarray([radius] * len(levels) if np.isscalar(radius) else radius)[np.maximum(ls, 0)]
                off = np.stack([rng.choice([-1, 0, 1], nq) * (r + rng.integers(0, 2, nq)), rng.integers(-3, 4, nq)])
                off = np.where(rng.random(nq) < 0.5, off, off[::-1])
                nx = np.clip(((src >> 12) & 0xFFF) + off[0], 0, 4095)
                ny = np.clip((src & 0xFFF) + off[1], 0, 4095)
                q = np.where(near, pack(nx, ny), q).astype(np.uint32)
                qd[b, :nq] = np.where(near[:, None], td[b, rng.integers(0, nt, nq)], random_descriptors(rng, nq, words))
            elif nq:
                qd[b, :nq] = random_descriptors(rng, nq, words)
            qkp[b, :nq] = q
        got = run_window(gpu_ctx, levels, radius, qkp, qd, qc, tkp, td, tc)
        check_against_reference(got, levels, radius, qkp, qd, qc, tkp, td, tc)


@pytest.mark.gpu
def test_gpu_window_full_train_stride(gpu_ctx):
    """t_stride = 65535 (the largest index the dist << 16 | index key holds), one pair filled to the stride."""
    rng = np.random.default_rng(65535)
    levels = DEMO_LEVELS
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
    qkp[0, 65:] = pack([0, 639, 0, 639, 320], [0, 0, 479, 479, 240])
    qkp[1] = random_positions(rng, qs, levels, 15)
    qd[1] = random_descriptors(rng, qs, words)
    qc = np.array([qs, qs], np.uint32)
    tc = np.array([ts, 100], np.uint32)
    for radius in (15, 4095):
        got = run_window(gpu_ctx, levels, radius, qkp, qd, qc, tkp, td, tc)
        check_against_reference(got, levels, radius, qkp, qd, qc, tkp, td, tc)


def frontend_outputs(B, seed=40, max_kp=2048):
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    dev = torch.device("cuda:0")
    fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=max_kp)
    kp, desc, counts = fe.alloc_outputs(B, dev)
    fe(torch.from_numpy(synth.make_batch(seed, B)).to(dev), kp, desc, counts)
    torch.cuda.synchronize()
    return levels, kp.cpu().numpy().view(np.uint32), desc.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
def test_gpu_window_on_frontend_outputs(gpu_ctx):
    """Frame k against frame k + 1 of the front end's own outputs: ragged counts, one empty train side, one query
    count above the stride (clamped)."""
    B = 8
    levels, kp, desc, counts = frontend_outputs(B + 1)
    assert counts.min() > 100
    qkp, qd, qc = kp[:B].copy(), desc[:B].copy(), counts[:B].copy()
    tkp, td, tc = kp[1:].copy(), desc[1:].copy(), counts[1:].copy()
    tc[2] = 0
    qc[3] = 3000
    for radius in (scaled_radii(15, len(levels)), 40):
        got = run_window(gpu_ctx, levels, radius, qkp, qd, qc, tkp, td, tc)
        check_against_reference(got, levels, radius, qkp, qd, qc, tkp, td, tc)
        # (synthetic pyramids are independent scenes: only some queries have a candidate in their window)
        nq = int(min(qc[0], 2048))
        assert (got[0][0, :nq].view(np.int32) >= 0).any()


@pytest.mark.gpu
def test_gpu_window_shifted_copy_property(gpu_ctx):
    """Train = the query keypoints shifted by (d, d) inside their level, same descriptors: at radius >= d every
    query finds distance 0 at its own index or at a smaller candidate index with an identical descriptor; at radius
    d - 1 no query returns its own index."""
    B, d = 4, 6
    levels, kp, desc, counts = frontend_outputs(B, seed=90)
    lid, x, y = level_ids(kp.reshape(-1), levels)
    lid, x, y = lid.reshape(kp.shape), x.reshape(kp.shape), y.reshape(kp.shape)
    w = np.array([t[0] for t in levels])[np.maximum(lid, 0)]
    h = np.array([t[1] for t in levels])[np.maximum(lid, 0)]
    r0 = np.array([t[2] for t in levels])[np.maximum(lid, 0)]
    sx = np.where(x + d < w, x + d, x - d)                     # (vertically stacked levels: col0 = 0)
    sy = np.where(y + d < r0 + h, y + d, y - d)
    tkp = pack(sx, sy).reshape(kp.shape)
    for radius, own in ((d, True), (d + 5, True), (d - 1, False)):
        gi, gd, _ = run_window(gpu_ctx, levels, radius, kp, desc, counts, tkp, desc, counts)
        for b in range(B):
            n = min(int(counts[b]), kp.shape[1])
            i = gi[b, :n].view(np.int32)
            if own:
                assert (gd[b, :n] == 0).all() and (i >= 0).all() and (i <= np.arange(n)).all()
                assert (desc[b, i] == desc[b, :n]).all()
                assert (lid[b, i] == lid[b, :n]).all()
                assert (np.abs(sx[b, i] - x[b, :n]) <= radius).all() and (np.abs(sy[b, i] - y[b, :n]) <= radius).all()
            else:
                assert (i != np.arange(n)).all()


@pytest.mark.gpu
def test_gpu_window_invalid_counts_and_untouched_slots(gpu_ctx):
    """PISLAM_COUNT_INVALID on either side counts as 0; output slots at and past the query count keep their fill."""
    rng = np.random.default_rng(3)
    levels, words, s = DEMO_LEVELS, 2, 128
    qkp = np.stack([random_positions(rng, s, levels, 15) for _ in range(4)])
    tkp = np.stack([random_positions(rng, s, levels, 15) for _ in range(4)])
    tkp[:, :s // 2] = qkp[:, :s // 2]
    qd = np.stack([random_descriptors(rng, s, words) for _ in range(4)])
    td = np.stack([random_descriptors(rng, s, words) for _ in range(4)])
    qc = np.array([COUNT_INVALID, 100, 100, 50], np.uint32)
    tc = np.array([100, COUNT_INVALID, 100, 0], np.uint32)
    for fill in (SENTINEL, 0xFFFFFFFF, 0):
        got = run_window(gpu_ctx, levels, 15, qkp, qd, qc, tkp, td, tc, fill=fill)
        check_against_reference(got, levels, 15, qkp, qd, qc, tkp, td, tc, fill=fill)
        gi, gd, g2 = got
        assert (gi[0] == fill).all() and (gd[0] == fill).all() and (g2[0] == fill).all()     # no query: nothing written
        assert (gi[1, :100].view(np.int32) == -1).all() and (gd[1, :100] == NONE_U32).all()  # no train entry
        assert (gi[2, :100].view(np.int32) >= 0).any()


def plan_cells(levels, radius):
    """(cells, f) of the windowed matcher's index by the rule the library states above its scaled_plan: level l has
    square cells of side max(1, radius[l]) * f over its rectangle, f >= 1 the smallest factor that keeps the cells of
    all levels within the 16384 bins of the index kernel's histogram."""
    rad = [radius] * len(levels) if np.isscalar(radius) else list(radius)
    f = 1
    while True:
        sides = [min(65536, max(1, int(r)) * f) for r in rad]
        n = sum(-(-_lv(t)[0] // s) * -(-_lv(t)[1] // s) for t, s in zip(levels, sides))
        if n <= 16384:
            return n, f
        f += 1


@pytest.mark.gpu
@pytest.mark.parametrize("size,radius,ncells,f", [((8, 8), 4095, 1, 1),            # a single bin
                                                  ((33, 32), 1, 1056, 1),          # chunks of 2, most threads' chunk empty
                                                  ((128, 128), 1, 16384, 1),       # the histogram's limit
                                                  ((129, 128), 1, 65 * 64, 2)])    # coarsened
def test_gpu_window_index_sort_bin_counts(gpu_ctx, size, radius, ncells, f):
    """The index kernel's counting sort at its bin-count edges, three pairs with different counts (so each pair's offset
    row is its own): no train entry under live queries, every train entry in one cell (the last), and a third of the
    train positions in no level."""
    w, h = size
    levels = [(w, h, 0, 0)]
    assert plan_cells(levels, radius) == (ncells, f)
    rng = np.random.default_rng([w, h, radius])
    words, qs, ts = 2, 200, 300
    qc = np.array([200, 150, 180], np.uint32)
    tc = np.array([0, 257, 300], np.uint32)
    tkp = np.zeros((3, ts), np.uint32)
    tkp[0] = pack(rng.integers(0, w, ts), rng.integers(0, h, ts))            # (past the count: never read)
    tkp[1] = pack(np.full(ts, w - 1), np.full(ts, h - 1))
    outside = np.arange(ts) % 3 == 0
    tkp[2] = pack(np.where(outside, rng.integers(w, w + 40, ts), rng.integers(0, w, ts)), rng.integers(0, h, ts))
    td = np.stack([random_descriptors(rng, ts, words) for _ in range(3)])
    # queries: a train position moved by -1 .. 1 (clipped into the level), or anywhere up to 2 px outside the level
    src = np.stack([tkp[b, rng.integers(0, max(1, int(tc[b])), qs)] for b in range(3)]).astype(np.int64)
    nx = np.clip(((src >> 12) & 0xFFF) + rng.integers(-1, 2, (3, qs)), 0, w - 1)
    ny = np.clip((src & 0xFFF) + rng.integers(-1, 2, (3, qs)), 0, h - 1)
    anywhere = pack(rng.integers(0, w + 2, (3, qs)), rng.integers(0, h + 2, (3, qs)))
    qkp = np.where(rng.random((3, qs)) < 0.6, pack(nx, ny), anywhere).astype(np.uint32)
    qkp[:, :5] = pack(np.full(5, w), np.arange(5))                           # in no level
    qd = np.stack([td[b, rng.integers(0, ts, qs)] for b in range(3)])
    got = run_window(gpu_ctx, levels, radius, qkp, qd, qc, tkp, td, tc)
    check_against_reference(got, levels, radius, qkp, qd, qc, tkp, td, tc)
    gi = got[0].view(np.int32)
    assert (gi[0, :200] == -1).all()
    assert (gi[1, :150] >= 0).any() and (gi[2, :180] >= 0).any() and (gi[2, :180] == -1).any()


@pytest.mark.gpu
def test_gpu_window_rejects_bad_arguments(gpu_ctx):
    import torch
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import matchHammingWindowBatch, reserveMatchWindow
    dev = torch.device("cuda:0")
    kp = torch.zeros((2, 16), dtype=torch.int32, device=dev)
    desc = torch.zeros((2, 16, 8), dtype=torch.int32, device=dev)
    cnt = torch.full((2,), 16, dtype=torch.int32, device=dev)
    lv = DEMO_LEVELS

    def call(qd=desc, tk=kp, td=desc, levels=lv, radius=15, qk=kp, qc=cnt, tc=cnt):
        matchHammingWindowBatch(qk, qd, qc, tk, td, tc, levels, radius, ctx=gpu_ctx)

    call()                                                                  # the baseline call is accepted
    torch.cuda.synchronize()
    d3 = torch.zeros((2, 16, 3), dtype=torch.int32, device=dev)
    big_kp = torch.zeros((2, 65536), dtype=torch.int32, device=dev)
    big_desc = torch.zeros((2, 65536, 8), dtype=torch.int32, device=dev)
    bad = [dict(qd=d3, td=d3),                                              # words 3
           dict(tk=big_kp, td=big_desc),                                    # t_stride 65536
           dict(radius=-1), dict(radius=4096), dict(radius=[15] * 7 + [4096]),
           dict(levels=[], radius=[]), dict(levels=[(10, 10, 10 * i, 0) for i in range(17)]),
           dict(levels=[(640, 480, 0, 0), (100, 100, 479, 0)]),            # overlapping rectangles
           dict(levels=[(100, 100, 0, 0), (100, 100, 50, 50)]),
           dict(levels=[(4000, 100, 0, 100)]),                              # past 12-bit x
           dict(qk=kp.cpu(), qd=desc.cpu(), qc=cnt.cpu()),                  # host tensors
           dict(tk=kp.cpu(), td=desc.cpu(), tc=cnt.cpu())]
    for kw in bad:
        with pytest.raises(PislamError):
            call(**kw)
    for kw in (dict(words=3), dict(t_stride=65536), dict(radius=4096)):
        args = dict(levels=lv, radius=15, t_stride=16, batch=2, words=8)
        args.update(kw)
        with pytest.raises(PislamError):
            reserveMatchWindow(args.pop("levels"), args.pop("radius"), args.pop("t_stride"), args.pop("batch"), ctx=gpu_ctx,
                               **args)


@pytest.mark.gpu
def test_gpu_window_call_is_hipgraph_capturable(gpu_ctx):
    """After pislam_match_window_reserve the call allocates nothing and never synchronises: capture one call on a
    side stream (one stream, no parallel branches), zero the outputs, replay and compare; change the inputs in
    place, replay again and compare with the reference."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchHammingWindowBatch, reserveMatchWindow
    B = 4
    levels, kp, desc, counts = frontend_outputs(B + 2, seed=120)
    radius = scaled_radii(15, len(levels))
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    qk, qd, qc = T(kp[:B]), T(desc[:B]), T(counts[:B])
    tk, td, tc = T(kp[1:B + 1]), T(desc[1:B + 1]), T(counts[1:B + 1])
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchWindow(levels, radius, kp.shape[1], B, words=desc.shape[2], ctx=ctx)
        outs = [torch.zeros((B, kp.shape[1]), dtype=torch.int32, device=dev) for _ in range(3)]
        matchHammingWindowBatch(qk, qd, qc, tk, td, tc, levels, radius, *outs, ctx=ctx)     # warm-up (module load)
        side.synchronize()
        ref = [o.clone() for o in outs]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            matchHammingWindowBatch(qk, qd, qc, tk, td, tc, levels, radius, *outs, ctx=ctx)
        for o in outs:
            o.zero_()
        g.replay()
        side.synchronize()
        for a, b in zip(ref, outs):
            assert torch.equal(a, b)
        # new inputs in the same buffers: frame k + 1 against k + 2
        for o in outs:
            o.zero_()
        qk.copy_(T(kp[1:B + 1])), qd.copy_(T(desc[1:B + 1])), qc.copy_(T(counts[1:B + 1]))
        tk.copy_(T(kp[2:])), td.copy_(T(desc[2:])), tc.copy_(T(counts[2:]))
        g.replay()
        side.synchronize()
    got = [o.cpu().numpy().view(np.uint32) for o in outs]
    check_against_reference(got, levels, radius, kp[1:B + 1], desc[1:B + 1], counts[1:B + 1], kp[2:], desc[2:], counts[2:],
                            fill=0)
