"""Every batched per-keypoint kernel's second and later grid passes, and pislam_match_hamming_batch at its own limits
(DESIGN.md section 5.5).

A batched call knows the capacity (the stride) and the batch, not the counts, which live on the device.  Its grid has
    query_grid():      min(tiles, ceil(16 * CUs / batch))   tiles per pair  (k_match_scaled, k_match_stereo,
                                                            k_stereo_refine, k_bow_descend, k_match_bow, k_track_lk)
    k_match_mfma:      min(tiles, ceil(8 * CUs / batch))
    k_match (VALU):    min(tiles, 16)
workgroups per pair, and every workgroup walks on over further tiles of its pair.  bench.py and the tools run batch 256
at strides of 2048 and more, where the later passes of that walk do most of the work; the other test modules use small
batches at strides of about 1000 and stay inside the first pass.  Part 1 has one test per kernel whose shape needs at
least three passes: a large batch at a modest stride with nearly all pairs empty (the grid depends on batch and
capacity only), live counts on both sides of one, two and all passes, and inputs planted so that neighbouring passes
differ at the same lane: a query without candidates sits where the pass before had a good match, and the reverse.  The
expectations are the other modules' references, word for word; every output is pre-filled with the sentinel and must
keep it at and beyond a pair's count and in every empty pair.  Each test works the pass size out from the rule above and
the device's CU count and asserts three passes before it launches: that is a condition on the inputs, not on the library.

Part 2 is the batched brute-force entry itself: query and train strides that differ, train counts around the 32-row
tile and clamped, t_stride 65535, batch 65535, empty calls, refusals and a hipGraph capture.

Stride products past 4 GiB of elements (q_stride * words * batch) would need tens of GB and are not covered here."""
import ctypes
import functools

import numpy as np
import pytest

import test_bow as tbow
import test_match_scaled_window as tscaled
import test_match_window as twin
import test_stereo_match as tstereo
import test_track_lk as tlk
from test_match_window import COUNT_INVALID, SENTINEL, clamp_count

NONE = 0xFFFFFFFF
OUTSIDE = (4095 << 12) | 4095                          # a position in no level of the layouts below


# ---- the launch rules ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def guided_pass(stride, qpw, batch):
    """Queries of one pair per grid pass under query_grid() for `qpw` queries per workgroup pass."""
    tiles = cdiv(stride, qpw)
    return qpw * (max(1, min(tiles, cdiv(16 * cu_count(), batch))) if batch > 1 else min(tiles, 65535))


def mfma_pass(stride, batch):
    tiles = cdiv(stride, 128)
    return 128 * (max(1, min(tiles, cdiv(8 * cu_count(), batch))) if batch > 1 else min(tiles, 65535))


def valu_pass(stride, batch):
    return 64 * min(cdiv(stride, 64), 16 if batch > 1 else 65535)


def need_three_passes(stride, P, what):
    """The condition on the inputs: with this device's CU count the shape takes at least three grid passes."""
    print(f"{what}: {cu_count()} CUs, pass size {P}, {cdiv(stride, P)} passes at stride {stride}")
    assert cdiv(stride, P) >= 3, (what, "the shape does not loop on this device", cu_count(), P, stride)


def pass_counts(P, stride):
    """Live counts: the first is the full stride (it goes to pair 0), the last 2P + 1 (to pair batch - 1)."""
    return [stride, 1, P - 1, P, P + 1, 2 * P, stride - 1, stride + 5, COUNT_INVALID, 2 * P + 1]


def spread(batch, n):
    """n pairs from 0 to batch - 1, both included."""
    pairs = np.unique(np.linspace(0, batch - 1, n).round().astype(np.int64))
    assert len(pairs) == n and pairs[0] == 0 and pairs[-1] == batch - 1
    return pairs


def slot_kinds(stride, P, kinds):
    """Kind of every slot: it changes from one slot to the next and, at the same offset, from one pass to the next."""
    i = np.arange(stride)
    return (i // P + i % P) % kinds


def third_pass(P, n):
    """The slots of the third pass below a count of n."""
    assert n > 2 * P
    return slice(2 * P, min(3 * P, n))


def rand_u32(rng, shape):
    return rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32)


def assert_empty_pairs_untouched(outs, pairs, batch):
    empty = np.ones(batch, bool)
    empty[pairs] = False
    for o in outs:
        assert (o[empty] == (SENTINEL & (0xFF if o.dtype == np.uint8 else 0xFFFFFFFF))).all(), "an empty pair was written"


@pytest.fixture(params=[1, 0], ids=["mfma", "valu"])
def match_kernel(request, gpu_ctx):
    """Both brute-force kernels: the matrix-core one (default) and the VALU popcount one."""
    gpu_ctx.set_option("match_mfma", request.param)
    yield request.param
    gpu_ctx.set_option("match_mfma", 1)


# ---- 1a. the brute-force kernels -------------------------------------------------------------------------------------
def TRAIN_COUNTS(ts):
    """Train counts of the live pairs, in the order of pass_counts: pair 0 (a full stride of queries) has ts."""
    return [ts, ts - 1, 33, ts + 9, 2, 1, 65, ts, 0, 32, COUNT_INVALID]


def brute_pair(rng, qs, ts, nt, words, P):
    """Queries [qs][words] and train [ts][words] of one pair.  Even kinds are copies of a train descriptor below the
    count (distance 0), odd kinds are random (distance far from 0).  With nt >= 40: train 30 repeats train 10 and slot
    2P + 3 asks for it (an exact tie: index 10); slot 2P + 5 is one bit from train 20, three bits from train 21."""
    t = rand_u32(rng, (ts, words))
    q = rand_u32(rng, (qs, words))
    if nt:
        copy = slot_kinds(qs, P, 2) == 0
        q[copy] = t[rng.integers(0, nt, qs)][copy]
    if nt >= 40 and qs > 2 * P + 5:
        bit = lambda v: np.array([v] + [0] * (words - 1), np.uint32)
        t[30] = t[10]
        t[21] = t[20] ^ bit(6)
        q[2 * P + 3] = t[10]
        q[2 * P + 5] = t[20] ^ bit(1)
    return q, t


def brute_expect(orc, q, qc, t, tc):
    """What a call leaves in sentinel-filled outputs: the brute-force entry takes min(count, stride) on both sides, so
    PISLAM_COUNT_INVALID means the whole stride."""
    B, qs, words = q.shape
    ts = t.shape[1]
    exp = [np.full((B, qs), SENTINEL, np.uint32) for _ in range(3)]
    for b in range(B):
        nq, nt = min(int(qc[b]), qs), min(int(tc[b]), ts)
        if nq:
            for e, r in zip(exp, orc.match_hamming(q[b, :nq], t[b, :nt].reshape(nt, words))):
                e[b, :nq] = r.view(np.uint32)
    return exp


def run_brute(ctx, q, qc, t, tc):
    import torch
    from pislam_amd.frontend import matchHammingBatch
    outs = [tbow.filled(q.shape[:2]) for _ in range(3)]
    matchHammingBatch(tbow.T(q), tbow.T(qc), tbow.T(t), tbow.T(tc), *outs, ctx=ctx)
    torch.cuda.synchronize()
    return [tbow.host(o) for o in outs]


def check_brute_passes(ctx, orc, words, B, qs, ts, P, counts, tcounts, seed):
    """One call: live pairs spread over the batch with `counts` / `tcounts`, the rest empty.  Returns got."""
    rng = np.random.default_rng([seed, words, qs])
    pairs = spread(B, len(counts)) if B >= len(counts) else np.arange(len(counts))
    q = np.zeros((B, qs, words), np.uint32)
    t = np.zeros((B, ts, words), np.uint32)
    qc, tc = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    qc[pairs], tc[pairs] = counts, tcounts
    for b in pairs:
        q[b], t[b] = brute_pair(rng, qs, ts, min(int(tc[b]), ts), words, P)
    empty = np.setdiff1d(np.arange(B), pairs)
    tc[empty[::5]] = ts                                    # some empty pairs have a train side: nothing to match it with
    got = run_brute(ctx, q, qc, t, tc)
    exp = brute_expect(orc, q, qc, t, tc)
    for name, g, e in zip(("idx", "dist", "dist2"), got, exp):
        bad = np.argwhere(g != e)
        assert len(bad) == 0, (name, words, len(bad), bad[:5].tolist(), [hex(int(g[tuple(k)])) for k in bad[:5]])
    return got, pairs


def check_brute_third_pass(got, b, n, P):
    """Pair b (nt = t_stride >= 40, count n): the third pass holds distance 0 and far matches, the tie and dist2."""
    idx, dist, dist2 = (g[b] for g in got)
    seg = third_pass(P, n)
    assert (dist[seg] == 0).any() and (dist[seg] > 0).any() and (idx[seg].view(np.int32) >= 0).all()
    assert (idx[2 * P + 3], dist[2 * P + 3], dist2[2 * P + 3]) == (10, 0, 0)
    assert (idx[2 * P + 5], dist[2 * P + 5], dist2[2 * P + 5]) == (20, 1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_match_mfma_more_queries_than_one_grid_pass(gpu_ctx, orc, words):
    """k_match_mfma at batch 1024, stride 1024: two workgroups of 128 queries per pair on 256 CUs, four passes.  A count
    of P + 1, P + 33 or 2P + 1 gives the four waves of a workgroup different trip counts."""
    B, qs, ts = 1024, 1024, 200
    P = mfma_pass(qs, B)
    need_three_passes(qs, P, "k_match_mfma")
    counts = pass_counts(P, qs)
    counts.insert(len(counts) - 1, P + 33)                 # (2P + 1 stays on the last pair)
    gpu_ctx.set_option("match_mfma", 1)
    got, pairs = check_brute_passes(gpu_ctx, orc, words, B, qs, ts, P, counts, TRAIN_COUNTS(ts), 1)
    check_brute_third_pass(got, 0, qs, P)
    assert got[0][B - 1, 2 * P] != SENTINEL and got[0][B - 1, 2 * P + 1] == SENTINEL    # 2P + 1 queries on the last pair
    assert (got[0][pairs[8], :qs] != SENTINEL).all()       # PISLAM_COUNT_INVALID: the whole stride


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_match_valu_more_queries_than_one_grid_pass(gpu_ctx, orc, words):
    """k_match (VALU) has at most 16 tiles of 64 queries per pair in flight whatever the batch: batch 3 at stride 2500 is
    three passes, the counts three to a call.  Its LDS merge buffers are reused from tile to tile."""
    B, qs, ts = 3, 2500, 200
    P = valu_pass(qs, B)
    need_three_passes(qs, P, "k_match")
    counts = pass_counts(P, qs)
    tcounts = TRAIN_COUNTS(ts)
    gpu_ctx.set_option("match_mfma", 0)
    try:
        for k in range(0, len(counts), B):
            c, t = counts[k:k + B], tcounts[k:k + B]
            c, t = c + [0] * (B - len(c)), t + [ts] * (B - len(t))
            got, _ = check_brute_passes(gpu_ctx, orc, words, B, qs, ts, P, c, t, 2 + k)
            if k == 0:
                check_brute_third_pass(got, 0, qs, P)
            if k == 6:                                     # stride - 1, stride + 5 (clamped), PISLAM_COUNT_INVALID (the stride)
                assert got[0][0, qs - 2] != SENTINEL and got[0][0, qs - 1] == SENTINEL
                assert (got[0][1] != SENTINEL).all() and (got[0][2] != SENTINEL).all()
    finally:
        gpu_ctx.set_option("match_mfma", 1)


# ---- 1b. the guided matchers: k_match_scaled (one level / span >= 1) and the windowed entry --------------------------
LEVELS3 = [(128, 96, 0, 0), (107, 80, 96, 0), (89, 67, 176, 0)]


def uniform_positions(rng, n, levels, margin=0, right_margin=0):
    """Packed positions uniform over the levels' rectangles, `margin` pixels inside them."""
    lv = np.array([twin._lv(t) for t in levels], np.int64)
    w, h, r0, c0 = lv[rng.integers(0, len(lv), n)].T
    x = c0 + margin + (rng.random(n) * (w - 2 * margin - right_margin)).astype(np.int64)
    y = r0 + margin + (rng.random(n) * (h - 2 * margin)).astype(np.int64)
    return twin.pack(x, y, rng.integers(0, 256, n))


@functools.lru_cache(maxsize=None)
def guided_case(B, qs, ts, P):
    """Query and train sides of the guided matchers, words 1.  Slot kinds: 0 lies in no level (no candidates), 1 is a
    copy of a train entry below the count (a match at distance 0), 2 is anywhere with any descriptor."""
    rng = np.random.default_rng([3, B, qs, P])
    counts = pass_counts(P, qs)
    pairs = spread(B, len(counts))
    qc, tc = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    qc[pairs] = counts
    tc[pairs] = [ts, ts - 1, 257, ts + 9, COUNT_INVALID, ts, 65, ts, ts, ts]
    qkp, tkp = np.zeros((B, qs), np.uint32), np.zeros((B, ts), np.uint32)
    qd, td = np.zeros((B, qs, 1), np.uint32), np.zeros((B, ts, 1), np.uint32)
    kind = slot_kinds(qs, P, 3)
    for b in pairs:
        nt = clamp_count(tc[b], ts)
        tkp[b], td[b] = uniform_positions(rng, ts, LEVELS3), twin.random_descriptors(rng, ts, 1)
        qkp[b], qd[b] = uniform_positions(rng, qs, LEVELS3), twin.random_descriptors(rng, qs, 1)
        qkp[b, kind == 0] = OUTSIDE
        if nt:
            j = rng.integers(0, nt, qs)
            qkp[b, kind == 1], qd[b, kind == 1] = tkp[b, j][kind == 1], td[b, j][kind == 1]
    empty = np.setdiff1d(np.arange(B), pairs)
    tc[empty[::5]] = ts                                    # train entries (all at the origin) without queries
    return dict(pairs=pairs, qkp=qkp, qd=qd, qc=qc, tkp=tkp, td=td, tc=tc)


def check_guided_third_pass(got, c, P, qs):
    """Matches and "none" results in the third pass of pair 0 (full) and of the last pair (one slot), and pair 4, whose
    train count is PISLAM_COUNT_INVALID, matches nothing."""
    idx = got[0].view(np.int32)
    seg = idx[0, third_pass(P, qs)]
    assert (seg >= 0).any() and (seg == -1).any()
    assert (got[1][0, third_pass(P, qs)] == 0).any() and (got[2][0, third_pass(P, qs)] != NONE).any()
    assert idx[-1, 2 * P] != SENTINEL and (got[0][-1, 2 * P + 1:] == SENTINEL).all()
    b = c["pairs"][4]
    assert (idx[b, :P + 1] == -1).all() and (got[0][b, P + 1:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("span", [0, 1])
def test_gpu_scaled_more_queries_than_one_grid_pass(gpu_ctx, span):
    """k_match_scaled at batch 1024, stride 1024: four workgroups of 64 queries per pair on 256 CUs, four passes; span 0
    is the ONE_LEVEL variant, span 1 the loop over the plan's levels (also with a prediction per query)."""
    B, qs, ts = 1024, 1024, 300
    P = guided_pass(qs, 64, B)
    need_three_passes(qs, P, "k_match_scaled")
    c = guided_case(B, qs, ts, P)
    s = tscaled.level_scales(LEVELS3)
    r = tscaled.scale_radii(s, 6)
    live = c["pairs"]
    args = [c[k] for k in ("qkp", "qd", "qc", "tkp", "td", "tc")]
    preds = [None]
    if span:
        _, X, Y = tscaled.mapped_positions(c["qkp"].reshape(-1), LEVELS3, s)
        own = np.stack([X, Y], 1).reshape(B, qs, 2)
        preds.append(own + np.random.default_rng(4).integers(-4, 5, own.shape))
    for pred in preds:
        got = tscaled.run_scaled(gpu_ctx, LEVELS3, s, r, span, *args, qpred=pred)
        tscaled.check_against_reference([g[live] for g in got], LEVELS3, s, r, span, *[a[live] for a in args],
                                        qpred=None if pred is None else pred[live])
        assert_empty_pairs_untouched(got, live, B)
        check_guided_third_pass(got, c, P, qs)


@pytest.mark.gpu
def test_gpu_window_more_queries_than_one_grid_pass(gpu_ctx):
    """The windowed entry (unit scales, span 0) on the same shape and inputs."""
    B, qs, ts = 1024, 1024, 300
    P = guided_pass(qs, 64, B)
    need_three_passes(qs, P, "k_match_scaled through the windowed entry")
    c = guided_case(B, qs, ts, P)
    live = c["pairs"]
    args = [c[k] for k in ("qkp", "qd", "qc", "tkp", "td", "tc")]
    radius = [6, 5, 4]
    got = twin.run_window(gpu_ctx, LEVELS3, radius, *args)
    twin.check_against_reference([g[live] for g in got], LEVELS3, radius, *[a[live] for a in args])
    assert_empty_pairs_untouched(got, live, B)
    check_guided_third_pass(got, c, P, qs)


# ---- 1c. stereo: k_match_stereo and k_stereo_refine ------------------------------------------------------------------
ST_LEVELS = [(96, 64, 0, 0), (80, 53, 64, 0)]
ST_VSTEP, ST_ROWS, ST_SHIFT = 96, 117, 6
ST_KW = dict(tstereo.KW, max_hamming=3, sad_radius=3, search_radius=3)


def run_stereo_shared(ctx, levels, s, rr, pyrs, left, right, **kw):
    """tstereo.run_stereo with one left and one right pyramid for every pair: the C entry with pyramid_stride 0."""
    import torch
    from pislam_amd.capi import Level, StereoParams
    T, dev = tbow.T, tbow.dev()
    lkp, ld, lc = left
    rkp, rd, rc = right
    B, ls, words = ld.shape
    nl = len(levels)
    lv_c = (Level * nl)(*[Level(*twin._lv(t)) for t in levels])
    s_c, r_c = (ctypes.c_int32 * nl)(*s), (ctypes.c_int32 * nl)(*rr)
    p_c = StereoParams(kw["level_span"], kw["min_disp"], kw["max_disp"], kw["max_hamming"], kw["sad_radius"],
                       kw["search_radius"], int(kw["median_filter"]))
    d_in = [T(a) for a in (lkp, ld, lc, rkp, rd, rc)]
    d_pyr = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pyrs]
    outs = [tbow.filled((B, ls)) for _ in range(4)]
    ns = tbow.filled((B,))
    rows, vstep = pyrs[0].shape
    ctx.check(ctx.lib.pislam_match_stereo_batch(
        ctx.h, words, lv_c, nl, s_c, r_c, ctypes.byref(p_c), d_pyr[0].data_ptr(), d_pyr[1].data_ptr(), vstep, rows, 0,
        d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), ls, d_in[3].data_ptr(), d_in[4].data_ptr(),
        d_in[5].data_ptr(), rkp.shape[1], B, *[o.data_ptr() for o in outs], ns.data_ptr()), "pislam_match_stereo_batch")
    torch.cuda.synchronize()
    return [tbow.host(o) for o in outs], tbow.host(ns)


@functools.lru_cache(maxsize=None)
def stereo_case(B, ls, rs, P):
    """One textured pyramid pair, the right image the left moved by ST_SHIFT pixels on every level.  Left slot kinds:
    0 lies in no level, 1 is the twin of a right keypoint below the count (its descriptor, ST_SHIFT pixels to the right:
    accepted, refined to about that disparity), 2 is anywhere with a descriptor of its own (rejected by max_hamming)."""
    rng = np.random.default_rng([5, B, ls, P])
    lp, rp = tstereo.random_image_pyramids(rng, 1, ST_LEVELS, ST_VSTEP, ST_ROWS, ST_SHIFT)
    counts = pass_counts(P, ls)
    pairs = spread(B, len(counts))
    lc, rc = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    lc[pairs] = counts
    rc[pairs] = [rs, rs - 1, 257, rs + 9, COUNT_INVALID, rs, 65, rs, rs, rs]
    lkp, rkp = np.zeros((B, ls), np.uint32), np.zeros((B, rs), np.uint32)
    ld, rd = np.zeros((B, ls, 1), np.uint32), np.zeros((B, rs, 1), np.uint32)
    kind = slot_kinds(ls, P, 3)
    for b in pairs:
        nr = clamp_count(rc[b], rs)
        rkp[b], rd[b] = uniform_positions(rng, rs, ST_LEVELS, 7, ST_SHIFT), rand_u32(rng, (rs, 1))
        lkp[b], ld[b] = uniform_positions(rng, ls, ST_LEVELS), rand_u32(rng, (ls, 1))
        lkp[b, kind == 0] = OUTSIDE
        if nr:
            j = rng.integers(0, nr, ls)
            twin_pos = (rkp[b, j] & 0xFFFFFF) + np.uint32(ST_SHIFT << 12)
            lkp[b, kind == 1], ld[b, kind == 1] = twin_pos[kind == 1], rd[b, j][kind == 1]
    return dict(pairs=pairs, pyrs=(lp[0], rp[0]), left=(lkp, ld, lc), right=(rkp, rd, rc))


@pytest.mark.gpu
def test_gpu_stereo_more_left_keypoints_than_one_grid_pass(gpu_ctx):
    """Batch 1024, l_stride 1024 on the smallest two-level pyramid, shared by all pairs: k_match_stereo has four
    workgroups of 64 left keypoints per pair on 256 CUs (four passes), k_stereo_refine four of 16 (sixteen passes)."""
    B, ls, rs = 1024, 1024, 300
    P, PR = guided_pass(ls, 64, B), guided_pass(ls, 16, B)
    need_three_passes(ls, P, "k_match_stereo")
    need_three_passes(ls, PR, "k_stereo_refine")
    c = stereo_case(B, ls, rs, P)
    live = c["pairs"]
    s = tscaled.level_scales(ST_LEVELS)
    rr = tstereo.row_radii(s)
    outs, ns = run_stereo_shared(gpu_ctx, ST_LEVELS, s, rr, c["pyrs"], c["left"], c["right"], **ST_KW)
    sub = lambda t: tuple(a[live] for a in t)
    shared = tuple(np.broadcast_to(p, (len(live),) + p.shape) for p in c["pyrs"])
    tstereo.check_stereo(([o[live] for o in outs], ns[live]), ST_LEVELS, s, rr, shared, sub(c["left"]), sub(c["right"]),
                         **ST_KW)
    assert_empty_pairs_untouched(outs, live, B)
    empty = np.setdiff1d(np.arange(B), live)
    assert (ns[empty] == 0).all()
    idx, disp = outs[0].view(np.int32), outs[2].view(np.int32)
    for p in (P, PR):                                      # the third pass of either kernel, and a late one of the refinement
        for seg in (third_pass(p, ls), slice(ls - p, ls)):
            assert (idx[0, seg] >= 0).any() and (idx[0, seg] == -1).any()
            assert (disp[0, seg] > 0).any() and (disp[0, seg] == -1).any()
            ok = disp[0, seg][disp[0, seg] > 0]
            assert (np.abs(ok - 256 * ST_SHIFT * np.array(s)[:, None] // 65536).min(0) <= 256).all()
    assert int(ns[0]) > ls // 6 and int(ns[-1]) > 2 * P // 6
    assert disp[-1, 2 * P] != SENTINEL and (outs[2][-1, 2 * P + 1:] == SENTINEL).all()


# ---- 1d. bag of words: k_bow_descend and k_match_bow -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_tree():
    """A ragged tree of a few dozen nodes, words 1: (node_desc, first_child, child_count), reference tree."""
    nd, fc, cc = tbow.random_tree(np.random.default_rng(41), 1, max_nodes=60, max_depth=3)
    tree = tbow.ref_tree(1, len(fc), fc, cc, 1)
    assert 24 <= len(fc) <= 60 and tree["nwords"] >= 12 and tree["depth"].max() >= 2
    return (nd, fc, cc), tree


@pytest.mark.gpu
def test_gpu_bow_descend_more_descriptors_than_one_grid_pass(gpu_ctx):
    """k_bow_descend at batch 1024, stride 1024: four workgroups of 16 descriptors per pyramid on 256 CUs, 16 passes.
    A descriptor's descent ends at a depth of its own, so a node or a distance kept from the pass before would show."""
    from pislam_amd.frontend import Vocabulary
    B, S = 1024, 1024
    P = guided_pass(S, 16, B)
    need_three_passes(S, P, "k_bow_descend")
    host_v, tree = small_tree()
    vocab = Vocabulary(*host_v, 1, ctx=gpu_ctx)
    rng = np.random.default_rng([6, P])
    counts_live = pass_counts(P, S)
    pairs = spread(B, len(counts_live))
    counts = np.zeros(B, np.uint32)
    counts[pairs] = counts_live
    desc = np.zeros((B, S, 1), np.uint32)
    desc[pairs] = rand_u32(rng, (len(pairs), S, 1))
    got = tbow.run_transform(gpu_ctx, vocab, desc, counts)
    tbow.check_transform([g[pairs] for g in got], desc[pairs], counts[pairs], host_v, tree)
    assert_empty_pairs_untouched(got, pairs, B)
    word, group, wdist = got
    for seg in (third_pass(P, S), slice(S - P, S)):
        assert len(set(word[0, seg].tolist())) >= 6 and len(set(group[0, seg].tolist())) >= 2
        assert len(set(wdist[0, seg].tolist())) >= 4
    assert word[-1, 2 * P] != SENTINEL and (word[-1, 2 * P + 1:] == SENTINEL).all()
    vocab.close()


@pytest.mark.gpu
def test_gpu_bow_match_more_queries_than_one_grid_pass(gpu_ctx):
    """k_match_bow at batch 1024, stride 1024, 40 groups.  Query slot kinds: 0 has a group id that is no group, 1 is a
    copy of a train entry below the count (descriptor and group), 2 has a random group and descriptor."""
    B, qs, ts, ngroups = 1024, 1024, 300, 40
    P = guided_pass(qs, 64, B)
    need_three_passes(qs, P, "k_match_bow")
    rng = np.random.default_rng([7, P])
    counts = pass_counts(P, qs)
    pairs = spread(B, len(counts))
    qc, tc = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    qc[pairs] = counts
    tc[pairs] = [ts, ts - 1, 257, ts + 9, COUNT_INVALID, ts, 65, ts, ts, ts]
    qd, td = np.zeros((B, qs, 1), np.uint32), np.zeros((B, ts, 1), np.uint32)
    qg, tg = np.zeros((B, qs), np.uint32), np.zeros((B, ts), np.uint32)
    kind = slot_kinds(qs, P, 3)
    for b in pairs:
        nt = clamp_count(tc[b], ts)
        td[b], tg[b] = twin.random_descriptors(rng, ts, 1), rng.integers(0, ngroups, ts)
        qd[b], qg[b] = twin.random_descriptors(rng, qs, 1), rng.integers(0, ngroups + 4, qs)
        qg[b, kind == 0] = rng.choice(np.array([ngroups, ngroups + 9, 0x80000000, NONE], np.uint32), qs)[kind == 0]
        if nt:
            j = rng.integers(0, nt, qs)
            qd[b, kind == 1], qg[b, kind == 1] = td[b, j][kind == 1], tg[b, j][kind == 1]
    empty = np.setdiff1d(np.arange(B), pairs)
    tc[empty[::5]] = ts
    got = tbow.run_bow_match(gpu_ctx, ngroups, qd, qg, qc, td, tg, tc)
    tbow.check_bow_match([g[pairs] for g in got], ngroups, qd[pairs], qg[pairs], qc[pairs], td[pairs], tg[pairs], tc[pairs])
    assert_empty_pairs_untouched(got, pairs, B)
    check_guided_third_pass(got, dict(pairs=pairs), P, qs)


# ---- 1e. the tracker: k_track_lk -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_track_more_points_than_one_grid_pass(gpu_ctx):
    """k_track_lk has one point per wave, four per workgroup: batch 1024 at stride 64 is four workgroups per pair on 256
    CUs and four passes.  (No other tracker test loops: test_track_lk.py has at most 2048 tiles in flight for its batches
    of 2, one point per pair in its large batches, and six points in its 4 GiB stride case.)  One 44 x 40 level shared
    by all pairs through pyramid_stride 0.  Point kinds: 0 lies in no level (status 1), 1 is well inside (tracked), 2 is
    anywhere in the level (near the border: status 1 or 3)."""
    B, S, H, W = 1024, 64, 40, 44
    P = guided_pass(S, 4, B)
    need_three_passes(S, P, "k_track_lk")
    dev = tlk.Device(gpu_ctx)
    prev_np, nxt_np = (v[None] for v in tlk.shifted_pair(H, W, 70, 1, -1))
    rng = np.random.default_rng([8, P])
    counts_live = pass_counts(P, S)
    pairs = spread(B, len(counts_live))
    counts = np.zeros(B, np.uint32)
    counts[pairs] = counts_live
    kind = slot_kinds(S, P, 3)
    pts = np.zeros((B, S, 2), np.int64)
    for b in pairs:
        inner = np.stack([rng.integers(9 * 256, 34 * 256, S), rng.integers(9 * 256, 30 * 256, S)], -1)
        anywhere = np.stack([rng.integers(0, W * 256, S), rng.integers(0, H * 256, S)], -1)
        pts[b] = np.where((kind == 1)[:, None], inner, anywhere)
        pts[b, kind == 0] = (-300, 77 * 256)
    prm = tlk.Lk(3, 5, 8, 2048, 1, 0, 0, 0)
    shared = [np.broadcast_to(v, (B, H, W)) for v in (prev_np, nxt_np)]
    want = dev.check([(W, H, 0, 0)], [65536], dev.up(prev_np), dev.up(nxt_np), *shared, pts, counts, None, prm, stride=0)
    codes = want[1] & 255                                  # (every output word equals the expectation: checked above)
    for seg in (third_pass(P, S), slice(S - P, S)):
        assert (codes[0, seg] == 0).any() and (codes[0, seg] == 1).any()
    assert want[1][-1, 2 * P] != tlk.SENT and (want[1][-1, 2 * P + 1:] == tlk.SENT).all()
    assert int(want[3][0]) >= S // 4 and int(want[3][pairs[8]]) == 0   # PISLAM_COUNT_INVALID: no point


# ---- 2. pislam_match_hamming_batch at its own limits -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_batch_matcher_different_strides(gpu_ctx, orc, match_kernel, words):
    """q_stride 300 against t_stride 70: train counts 0, 1 (dist2 0xffffffff), 2, around the 32-row tile of the
    matrix-core kernel, the stride, and beyond it (clamped); query counts likewise."""
    qs, ts = 300, 70
    tcounts = [0, 1, 2, 31, 32, 33, ts, ts + 9, COUNT_INVALID]
    qcounts = [qs, qs - 1, 129, qs + 5, 1, 64, COUNT_INVALID, qs, 0]
    B = len(tcounts)
    rng = np.random.default_rng([9, words])
    q, t = np.zeros((B, qs, words), np.uint32), np.zeros((B, ts, words), np.uint32)
    for b in range(B):
        q[b], t[b] = brute_pair(rng, qs, ts, min(tcounts[b], ts), words, 64)
    q[7, 0], q[7, 1] = t[7, ts - 1], t[7, ts - 1] ^ np.array([1] + [0] * (words - 1), np.uint32)   # the last one under the clamp
    qc, tc = np.array(qcounts, np.uint32), np.array(tcounts, np.uint32)
    got = run_brute(gpu_ctx, q, qc, t, tc)
    for g, e in zip(got, brute_expect(orc, q, qc, t, tc)):
        assert (g == e).all(), (words, np.argwhere(g != e)[:5].tolist())
    idx, dist, dist2 = got
    assert (idx[0, :qs] == NONE).all() and (dist[0, :qs] == NONE).all() and (dist2[0, :qs] == NONE).all()   # no train: -1
    assert (idx[1, :qs - 1] == 0).all() and (dist2[1, :qs - 1] == NONE).all() and dist2[2, 0] != NONE
    assert (idx[7] < ts).all() and (idx[7, 0], dist[7, 0]) == (ts - 1, 0) and (idx[7, 1], dist[7, 1]) == (ts - 1, 1)   # ts + 9 is clamped
    assert (idx[8] == SENTINEL).all()                                                       # (no query: untouched)
    assert (idx[6] != SENTINEL).all() and idx[3, qs - 1] != SENTINEL and idx[2, 129] == SENTINEL


@pytest.mark.gpu
@pytest.mark.parametrize("words", [1, 8])
def test_gpu_batch_matcher_at_the_largest_train_stride(gpu_ctx, orc, match_kernel, words):
    """t_stride = 65535 in the batched entry, batch 2: pair 1 is test_gpu_matcher_at_the_largest_16_bit_train_index's
    case (best matches and a tie above 65000, the last index included), pair 0 has 1000 train descriptors."""
    rng = np.random.default_rng(65535 + words)
    ts, qs = 65535, 300
    t = np.stack([rand_u32(rng, (ts, words)) for _ in range(2)])
    q = np.stack([rand_u32(rng, (qs, words)) for _ in range(2)])
    flip = lambda bits: np.array([bits] + [0] * (words - 1), np.uint32)
    t[1, 65533] = t[1, 65001]
    t[1, 65527] = t[1, 65002] ^ flip(4)
    q[1, 0] = t[1, 65534]
    q[1, 1] = t[1, 65534] ^ flip(1)
    q[1, 2] = t[1, 65533]
    q[1, 3] = t[1, 65002] ^ flip(3)
    q[1, 299] = t[1, 65534]
    q[0, :5] = t[1, 65530:]                                # pair 0 must not see pair 1's train descriptors
    qc, tc = np.array([qs, qs], np.uint32), np.array([1000, ts], np.uint32)
    got = run_brute(gpu_ctx, q, qc, t, tc)
    for g, e in zip(got, brute_expect(orc, q, qc, t, tc)):
        assert (g == e).all(), (words, np.argwhere(g != e)[:5].tolist())
    idx, dist, dist2 = (g[1] for g in got)
    assert (idx[0], dist[0]) == (65534, 0) and (idx[299], dist[299]) == (65534, 0)
    assert (idx[2], dist[2], dist2[2]) == (65001, 0, 0)
    if words == 8:                                         # (with 32-bit descriptors 65535 random ones come closer)
        assert (idx[1], dist[1]) == (65534, 1) and (idx[3], dist[3], dist2[3]) == (65002, 2, 3)
    assert (got[0][0] < 1000).all()


@pytest.mark.gpu
def test_gpu_batch_matcher_largest_batch(gpu_ctx, orc, match_kernel):
    """batch 65535, the largest accepted, of q_stride 2, t_stride 3, words 1: pair b carries pattern b % 257 of 257 small
    cases with cycling counts.  257 does not divide 65535, so a pair addressed at the wrong offset shows as a phase
    shift.  batch 65536 is refused."""
    import torch
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import matchHammingBatch
    B, N, qs, ts = 65535, 257, 2, 3
    rng = np.random.default_rng(257)
    q, t = rng.integers(0, 16, (N, qs, 1)).astype(np.uint32), rng.integers(0, 16, (N, ts, 1)).astype(np.uint32)
    qc = np.array([0, 1, 2, 3, COUNT_INVALID], np.uint32)[np.arange(N) % 5]
    tc = np.array([0, 1, 2, 3, 4, COUNT_INVALID], np.uint32)[np.arange(N) % 6]
    exp = brute_expect(orc, q, qc, t, tc)
    assert len({e.tobytes() for e in exp[0]}) >= 8 and (exp[2] == NONE).any() and (exp[2] < 32).any()
    which = np.arange(B) % N
    got = run_brute(gpu_ctx, q[which], qc[which], t[which], tc[which])
    for name, g, e in zip(("idx", "dist", "dist2"), got, exp):
        bad = np.flatnonzero((g != e[which]).any(axis=1))
        assert len(bad) == 0, (name, bad[:5], len(bad))
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=tbow.dev())
    outs = [tbow.filled((B + 1, qs)) for _ in range(3)]
    with pytest.raises(PislamError):
        matchHammingBatch(z(B + 1, qs, 1), z(B + 1), z(B + 1, ts, 1), z(B + 1), *outs, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert all((tbow.host(o) == SENTINEL).all() for o in outs)


@pytest.mark.gpu
def test_gpu_batch_matcher_empty_calls_and_refusals(gpu_ctx, match_kernel):
    """q_stride 0 and batch 0 return PISLAM_OK and touch nothing; t_stride 65536, a null pointer, a host pointer and
    words 3 are refused and touch nothing."""
    import torch
    from pislam_amd.capi import PislamError, ptr
    from pislam_amd.frontend import matchHammingBatch
    B, qs, ts, words = 2, 16, 8, 2
    dev = tbow.dev()
    qd = torch.zeros((B, qs, words), dtype=torch.int32, device=dev)
    td = torch.zeros((B, ts, words), dtype=torch.int32, device=dev)
    qc = torch.full((B,), qs, dtype=torch.int32, device=dev)
    tc = torch.full((B,), ts, dtype=torch.int32, device=dev)
    outs = [tbow.filled((B, qs)) for _ in range(3)]
    lib = gpu_ctx.lib

    def capi(words=words, qd=qd, qc=qc, q_stride=qs, td=td, tc=tc, t_stride=ts, batch=B, o=outs):
        return lib.pislam_match_hamming_batch(gpu_ctx.h, words, ptr(qd), ptr(qc), q_stride, ptr(td), ptr(tc), t_stride, batch,
                                              ptr(o[0]), ptr(o[1]), ptr(o[2]))

    def untouched():
        torch.cuda.synchronize()
        return all((tbow.host(o) == SENTINEL).all() for o in outs)

    assert capi(q_stride=0) == 0 and untouched()
    assert capi(batch=0) == 0 and untouched()
    assert capi(q_stride=0, qd=None, o=[None] * 3) == 0 and capi(batch=0, qd=None, td=None, qc=None, tc=None) == 0
    bad = [dict(t_stride=65536), dict(words=3), dict(batch=-1), dict(batch=65536), dict(qd=None), dict(td=None), dict(qc=None),
           dict(tc=None), dict(o=[None, outs[1], outs[2]]), dict(o=[outs[0], None, outs[2]]), dict(o=[outs[0], outs[1], None]),
           dict(qd=qd.cpu()), dict(td=td.cpu()), dict(qc=qc.cpu()), dict(tc=tc.cpu()),
           dict(o=[outs[0].cpu(), outs[1], outs[2]]), dict(o=[outs[0], outs[1], outs[2].cpu()])]
    for kw in bad:
        rc = capi(**kw)
        assert rc == -1, (list(kw), rc)
        with pytest.raises(PislamError):
            gpu_ctx.check(rc, "pislam_match_hamming_batch")
        assert untouched(), list(kw)
    big = torch.zeros((B, 65536, words), dtype=torch.int32, device=dev)
    for kw in (dict(tdesc=big), dict(qdesc=qd.cpu()), dict(tcounts=tc.cpu())):
        a = dict(qdesc=qd, qcounts=qc, tdesc=td, tcounts=tc)
        a.update(kw)
        with pytest.raises(PislamError):
            matchHammingBatch(a["qdesc"], a["qcounts"], a["tdesc"], a["tcounts"], *outs, ctx=gpu_ctx)
        assert untouched()
    assert capi() == 0                                     # the baseline call is accepted
    torch.cuda.synchronize()
    assert (tbow.host(outs[0]) == 0).all() and (tbow.host(outs[1]) == 0).all() and (tbow.host(outs[2]) == 0).all()


@pytest.mark.gpu
def test_gpu_batch_matcher_is_hipgraph_capturable(gpu_ctx, orc, match_kernel):
    """The batched matcher has no workspace and never synchronises: one call captured on a side stream (one stream, no
    parallel branches) and replayed twice; the train counts change between the replays and the results follow them."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import matchHammingBatch
    B, qs, ts, words = 4, 300, 70, 4
    rng = np.random.default_rng(10)
    q, t = np.zeros((B, qs, words), np.uint32), np.zeros((B, ts, words), np.uint32)
    for b in range(B):
        q[b], t[b] = brute_pair(rng, qs, ts, ts, words, 64)
    qc = np.array([qs, 129, 0, qs + 1], np.uint32)
    tc1, tc2 = np.array([ts, 33, 5, 1], np.uint32), np.array([1, ts + 3, 5, 0], np.uint32)
    side = torch.cuda.Stream(tbow.dev())
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        ctx.set_option("match_mfma", match_kernel)
        d_q, d_qc, d_t, d_tc = tbow.T(q), tbow.T(qc), tbow.T(t), tbow.T(tc1)
        outs = [tbow.filled((B, qs)) for _ in range(3)]
        matchHammingBatch(d_q, d_qc, d_t, d_tc, *outs, ctx=ctx)             # warm-up (module load)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            matchHammingBatch(d_q, d_qc, d_t, d_tc, *outs, ctx=ctx)
        for tc in (tc1, tc2):
            for o in outs:
                o.fill_(SENTINEL)
            d_tc.copy_(tbow.T(tc))
            g.replay()
            side.synchronize()
            for got, e in zip(outs, brute_expect(orc, q, qc, t, tc)):
                assert (tbow.host(got) == e).all(), tc.tolist()
        assert (tbow.host(outs[0])[3, :qs] == NONE).all()                    # the second replay saw the train count 0
        ctx.close()
