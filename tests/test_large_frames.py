"""Frames at the 12-bit coordinate limit of the packed keypoint (score << 24 | x << 12 | y, Util.h:27-29).

The library takes any layout whose levels end at or below column 4096 and row 4096.  These tests run the front end, the
pyramid builder and the matchers at that limit and compare them bit for bit with the oracle:

  layout 1      1920x1080, packed_level_table with vstep 4096: 3355 rows, levels 4-7 beside level 3, level 5 at column
                2048 (keypoints with x >= 2048 set bit 23, next to the score byte); 19 plan entries, up to four x-tiles
                per level.
  layout 2      4096x768 stacked, vstep 4096: 3535 rows.  Its first three levels need 9 + 8 + 6 = 23 plan entries and
                run fused; all eight need 41, more than the strip plan holds (24), and run staged.
  the corner    a small level whose rectangle ends exactly at column 4096 and row 4096.
  4 GiB batch   320 pyramids of layout 1 (13 742 080 bytes each): pyramids 156 and 312 straddle 2^31 and 2^32 bytes.

The CPU test at the top records, through the host-only planner, why each GPU case reaches the path it asserts."""
import ctypes

import numpy as np
import pytest

from test_match_scaled_window import check_against_reference, level_scales, run_scaled, scale_radii
from test_prep import build_defined_mask
from test_stereo_match import KW, check_stereo, host_pyramid, row_radii, run_stereo

VSTEP = 4096
MAX_PLAN_ENTRIES = 24                 # pf::MAX_LEVELS: more entries and the call takes the staged pipeline
SEL_NB = 1024                         # pf::SEL_NB: buckets per cell row the selection pass holds
STAGED, FUSED, ONE_LAUNCH, BUCKET_SELECT = 1, 2, 4, 8      # PISLAM_PATH_*


def layout1():
    from pislam_amd import synth
    return [tuple(t) for t in synth.packed_level_table(1920, 1080, vstep=VSTEP)]


def layout2():
    from pislam_amd import synth
    return [(w, h, r0, 0) for (w, h, r0) in synth.level_table(4096, 768)]


def rows_of(levels):
    return max(t[2] + t[1] for t in levels)


def x_tiles(w, border=16):
    """Plan entries of one level (plan_entries): more than 704 classified columns are cut into tiles of about
    448 owned columns, T a multiple of 32."""
    nx = w - 2 * border
    if 16 * -(-nx // 16) <= 704:
        return 1
    nt = max(2, (nx + 224) // 448)
    T = (-(-nx // nt) + 31) & ~31
    return -(-nx // T)


def corner_layout(dx=0, dy=0):
    """A VGA level at the origin and a 160x128 level ending at column 4096 + dx and row 4096 + dy, in a buffer with room
    to spare (vstep 4112, 4104 rows): only the 12-bit rule can refuse dx or dy = 1."""
    return [(640, 480, 0, 0), (160, 128, 3968 + dy, 3936 + dx)], 4112, 4104


def debug_plan(levels, vstep, rows, batch=1, lbs=0, limit=5, opts=b""):
    from pislam_amd import capi
    lib = capi.load(rebuild_if_stale=False)
    n = len(levels)
    L = (capi.Level * n)(*[capi.Level(t[0], t[1], t[2], t[3] if len(t) > 3 else 0) for t in levels])
    P = capi.FrontendParams(vstep, rows, n, 16, 20, 1 << 15, lbs, limit, 8, 16384)
    out = (ctypes.c_uint32 * 8)()
    err = ctypes.create_string_buffer(256)
    rc = lib.pislam_debug_build_plan(ctypes.byref(P), L, batch, 256, 1, opts, ctypes.byref(out), err, 256)
    return rc, list(out), err.value.decode()


# ---- CPU: the plans behind the GPU cases -------------------------------------------------------------------------
def test_plans_of_the_large_frame_cases():
    l1 = layout1()
    assert rows_of(l1) == 3355 and max(t[3] + t[0] for t in l1) == 4024
    assert [t[2] for t in l1[3:]] == [2730] * 5 and l1[5][3] == 2048          # levels 4-7 beside level 3
    assert [x_tiles(t[0]) for t in l1] == [4, 4, 3, 2, 2, 2, 1, 1]
    for batch in (1, 2, 5, 320):
        for lbs, limit in ((0, 5), (4, 3), (1, 2)):
            rc, s, msg = debug_plan(l1, VSTEP, 3355, batch, lbs, limit)
            assert rc == 0 and s[0] == 19, (batch, lbs, s, msg)
            # buckets: the selection pass holds every level (1888 columns / 2 = 944 <= 1024 buckets at lbs 1)
            assert (s[7] > 0) == (lbs != 0), (batch, lbs, s)
    for opts in (b"sub_batches=3", b"sub_batches=0"):
        rc, s, msg = debug_plan(l1, VSTEP, 3355, 320, opts=opts)
        assert rc == 0 and s[0] == 19, (opts, msg)

    l2 = layout2()
    assert rows_of(l2) == 3535 and l2[0][0] == 4096
    tiles = [x_tiles(t[0]) for t in l2]
    assert tiles[:3] == [9, 8, 6] and sum(tiles[:3]) == 23 <= MAX_PLAN_ENTRIES < sum(tiles) == 41
    for batch in (1, 2):
        rc, s, msg = debug_plan(l2[:3], VSTEP, 3535, batch)
        assert rc == 0 and s[0] == 23 and s[7] == 0, (s, msg)
        rc, s, msg = debug_plan(l2, VSTEP, 3535, batch)
        assert rc == -1 and "staged" in msg, msg                                 # 41 entries: no strip plan
        # lbs 1: 2032 two-pixel buckets on level 0 turn the selection pass off; in-strip buckets need 4..32 px cells
        assert (4096 - 32 - 1) // 2 + 1 > SEL_NB
        rc, s, msg = debug_plan(l2[:3], VSTEP, 3535, batch, 1, 2)
        assert rc == -1 and "staged" in msg, msg
        rc, s, msg = debug_plan(l2[:3], VSTEP, 3535, batch, 4, 3)
        assert rc == 0 and s[0] == 23 and s[7] > 0, (s, msg)

    lv, vstep, rows = corner_layout()
    assert max(t[3] + t[0] for t in lv) == 4096 and max(t[2] + t[1] for t in lv) == 4096
    assert debug_plan(lv, vstep, rows)[0] == 0
    for dx, dy in ((1, 0), (0, 1)):
        lv, vstep, rows = corner_layout(dx, dy)
        assert max(t[3] + t[0] for t in lv) <= vstep and max(t[2] + t[1] for t in lv) <= rows
        rc, _, msg = debug_plan(lv, vstep, rows)
        assert rc == -1 and "12 bits" in msg, (dx, dy, msg)


# ---- GPU ---------------------------------------------------------------------------------------------------------
def oracle_levels(orc, pyr, levels, lbs=0, limit=5):
    """(keypoints, descriptors) of one pyramid: the oracle run level by level on a view that starts at the level's
    first pixel (the reference's flat addressing), keypoints offset by (col0, row0), then one orbCompute."""
    vstep = pyr.shape[1]
    exp = []
    for (w, h, r0, c0) in levels:
        view = np.ascontiguousarray(pyr[r0:r0 + h].reshape(-1)[c0:])
        view = np.concatenate([view, np.zeros((-len(view)) % vstep, np.uint8)]).reshape(-1, vstep)
        lkp, _, _ = orc.pyramid(view, [(w, h, 0)], log_bucket=lbs, bucket_limit=limit)
        exp.append(lkp + np.uint32((c0 << 12) | r0))
    exp = np.concatenate(exp)
    return exp, orc.orb_compute(pyr, exp)


def run_frontend(ctx, levels, vstep, rows, d_pyr, cap, lbs=0, limit=5):
    import torch
    from pislam_amd.frontend import OrbFrontend
    fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=cap, log_bucket_size=lbs, bucket_limit=limit, ctx=ctx)
    kp, desc, counts = fe.alloc_outputs(int(d_pyr.shape[0]), d_pyr.device)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc)) + (fe.last_path(),)


def assert_matches(c, k, d, b, exp, what):
    okp, odesc = exp
    n = len(okp)
    assert int(c[b]) == n, (what, b, int(c[b]), n)
    bad = np.flatnonzero(k[b, :n] != okp)[:5]
    assert (k[b, :n] == okp).all(), (what, b, bad, k[b, bad], okp[bad])
    assert (d[b, :n] == odesc).all(), (what, b)


@pytest.mark.gpu
def test_1080p_pyramid_with_keypoints_past_column_2048(gpu_ctx, orc):
    """Layout 1 through OrbFrontend: batch 1 and 2 (one launch and three launches), batch 5 staged and fused, without
    buckets, with the README's <4,3> and with 2-pixel buckets <1,2>: counts, keypoints and descriptors equal the oracle,
    and keypoints with x >= 2048 occur."""
    import torch
    from pislam_amd import synth
    levels, rows = layout1(), 3355
    pyr = synth.make_batch(500, 5, w0=1920, h0=1080, vstep=VSTEP, levels=levels)
    d_pyr = torch.from_numpy(pyr).to("cuda:0")
    runs = [(1, "frame", 1), (1, "frame", 0), (2, "frame", 1), (2, "frame", 0), (5, "pipeline", 1), (5, "pipeline", 2)]
    defaults = {"frame": 1, "pipeline": 0}
    for lbs, limit in ((0, 5), (4, 3), (1, 2)):
        exp = [oracle_levels(orc, pyr[b], levels, lbs, limit) for b in range(5)]
        if lbs == 0:
            for okp, _ in exp:
                assert ((okp >> 12) & 0xFFF).max() >= 2048 and (okp & 0xFFF).max() < 3355
        for batch, key, val in runs:
            gpu_ctx.set_option(key, val)
            try:
                c, k, d, path = run_frontend(gpu_ctx, levels, VSTEP, rows, d_pyr[:batch], 16384, lbs, limit)
            finally:
                gpu_ctx.set_option(key, defaults[key])
            if key == "pipeline" and val == 1:
                want = STAGED
            else:
                one = lbs == 0 and key == "frame" and val == 1
                want = FUSED | (BUCKET_SELECT if lbs else 0) | (ONE_LAUNCH if one else 0)
            assert path == want, (lbs, batch, key, val, path)
            for b in range(batch):
                assert_matches(c, k, d, b, exp[b], (lbs, batch, key, val))
            assert (((k[0, :int(c[0])] >> 12) & 0xFFF) >= 2048).any()


@pytest.mark.gpu
def test_4096_wide_level0(gpu_ctx, orc):
    """Layout 2: its first three levels run fused with nine x-tiles at level 0 (one launch and three launches); all
    eight levels, and three levels with 2-pixel buckets, run staged; three levels with 16-pixel buckets run fused with
    the selection pass.  Every case equals the oracle."""
    import torch
    from pislam_amd import synth
    levels, rows = layout2(), 3535
    pyr = synth.make_batch(520, 2, w0=4096, h0=768, vstep=VSTEP, levels=levels)
    d_pyr = torch.from_numpy(pyr).to("cuda:0")
    cases = [(3, 0, 5, 1, FUSED | ONE_LAUNCH), (3, 0, 5, 0, FUSED), (8, 0, 5, 1, STAGED), (3, 1, 2, 1, STAGED),
             (3, 4, 3, 1, FUSED | BUCKET_SELECT)]
    for nl, lbs, limit, frame, want in cases:
        lv = levels[:nl]
        gpu_ctx.set_option("frame", frame)
        try:
            c, k, d, path = run_frontend(gpu_ctx, lv, VSTEP, rows, d_pyr, 32768, lbs, limit)
        finally:
            gpu_ctx.set_option("frame", 1)
        assert path == want, (nl, lbs, frame, path)
        for b in range(2):
            exp = oracle_levels(orc, pyr[b], lv, lbs, limit)
            assert len(exp[0]) > 1000
            assert_matches(c, k, d, b, exp, (nl, lbs, frame))
        assert ((k[0, :int(c[0])] >> 12) & 0xFFF).max() >= 4000


def corner_pyramids(B, dx=0, dy=0):
    from pislam_amd import synth
    lv, vstep, rows = corner_layout(dx, dy)
    rng = np.random.default_rng(7)
    pyr = np.zeros((B, rows, vstep), np.uint8)
    for b in range(B):
        pyr[b, :480, :640] = synth.make_level0(720 + b, 640, 480)
        w, h, r0, c0 = lv[1]
        pyr[b, r0:r0 + h, c0:c0 + w] = np.kron(rng.integers(0, 256, (h // 4, w // 4)), np.ones((4, 4), np.int64))
    return lv, vstep, rows, pyr


@pytest.mark.gpu
def test_level_ending_at_column_and_row_4096(gpu_ctx, orc):
    """A level whose rectangle ends exactly at column 4096 and row 4096 is accepted on both pipelines and equals the
    oracle, with keypoints within 32 px of column and row 4095; one column or one row further is refused with the
    outputs untouched."""
    import torch
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import OrbFrontend
    dev = torch.device("cuda:0")
    lv, vstep, rows, pyr = corner_pyramids(2)
    d_pyr = torch.from_numpy(pyr).to(dev)
    exp = [oracle_levels(orc, pyr[b], lv) for b in range(2)]
    for pl, want in ((0, FUSED | ONE_LAUNCH), (1, STAGED)):
        gpu_ctx.set_option("pipeline", pl)
        try:
            c, k, d, path = run_frontend(gpu_ctx, lv, vstep, rows, d_pyr, 8192)
        finally:
            gpu_ctx.set_option("pipeline", 0)
        assert path == want, (pl, path)
        for b in range(2):
            assert_matches(c, k, d, b, exp[b], pl)
            x, y = (k[b, :int(c[b])] >> 12) & 0xFFF, k[b, :int(c[b])] & 0xFFF
            assert ((x >= 4064) & (y >= 4064)).any(), b
    for dx, dy in ((1, 0), (0, 1)):
        lv1, _, _, _ = corner_pyramids(0, dx, dy)
        fe = OrbFrontend(lv1, vstep=vstep, rows=rows, max_keypoints=8192, ctx=gpu_ctx)
        kp, desc, counts = fe.alloc_outputs(2, dev)
        for t in (kp, desc, counts):
            t.fill_(0x5A5A5A5A)
        with pytest.raises(PislamError, match="12 bits"):
            fe(d_pyr, kp, desc, counts)
        torch.cuda.synchronize()
        for t in (kp, desc, counts):
            assert (t == 0x5A5A5A5A).all(), (dx, dy)


@pytest.mark.gpu
def test_batch_past_4_gib(orc):
    """320 pyramids of layout 1 (4.4 GB) built on the device from four host pyramids, pyramid b rolled along its rows by
    b columns: the pyramids on both sides of 2^31 and 2^32 bytes equal the oracle, with one launch group and with 3 and
    with automatic (bytes per sub-batch) sub-batches; every run writes the same outputs."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend
    levels, rows = layout1(), 3355
    B, pyr_bytes = 320, 3355 * VSTEP
    assert pyr_bytes == 13742080
    assert 156 * pyr_bytes < 1 << 31 < 157 * pyr_bytes and 312 * pyr_bytes < 1 << 32 < 313 * pyr_bytes
    probes = (0, 155, 156, 157, 311, 312, 313, 319)
    base = synth.make_batch(540, 4, w0=1920, h0=1080, vstep=VSTEP, levels=levels)
    exp = {b: oracle_levels(orc, np.ascontiguousarray(np.roll(base[b % 4], b, axis=1)), levels) for b in probes}
    dev = torch.device("cuda:0")
    ctx = Context()                       # (its 4.4 GB score-map workspace goes with it)
    try:
        d_base = torch.from_numpy(base).to(dev)
        d_pyr = torch.empty((B, rows, VSTEP), dtype=torch.uint8, device=dev)
        for b in range(B):
            d_pyr[b] = torch.roll(d_base[b % 4], shifts=b, dims=1)
        del d_base
        fe = OrbFrontend(levels, vstep=VSTEP, rows=rows, max_keypoints=16384, ctx=ctx)
        kp, desc, counts = fe.alloc_outputs(B, dev)
        first = None
        for nsub in (1, 3, 0):
            ctx.set_option("sub_batches", nsub)
            for t in (kp, desc, counts):
                t.fill_(-1)
            fe(d_pyr, kp, desc, counts)
            torch.cuda.synchronize()
            assert fe.last_path() == FUSED, (nsub, fe.last_path())
            sel = torch.tensor(probes, device=dev)
            c, k, d = (t[sel].cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
            for i, b in enumerate(probes):
                assert_matches(c, k, d, i, exp[b], (nsub, b))
            if first is None:
                first = (counts.clone(), kp.clone(), desc.clone())
            else:
                assert all(torch.equal(a, g) for a, g in zip(first, (counts, kp, desc))), nsub
    finally:
        first = kp = desc = counts = d_pyr = None
        ctx.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("w0,h0,steps", [(1920, 1080, (2, 2, 1, 2)), (4096, 720, (2, 1, 2, 2, 1, 2, 2))])
@pytest.mark.parametrize("chain", [0, 1])
def test_pyramid_build_at_large_widths(gpu_ctx, orc, w0, h0, steps, chain):
    """The builder at 1920 and 4096 columns, one launch per level and one launch for the whole chain: the bytes equal
    the oracle's gaussian5x5 + bilinear sequence on a zeroed buffer, bytes outside what the build defines stay untouched,
    and the front end on the built pyramids equals the oracle."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import PyramidBuilder
    pb = PyramidBuilder(w0, h0, steps, ctx=gpu_ctx)
    assert pb.vstep == w0 and pb.rows <= 4096
    rng = np.random.default_rng(11)
    B = 2
    frames = np.stack([rng.integers(0, 256, (h0, w0), dtype=np.uint8), synth.make_level0(60, w0, h0)])
    d_fr = torch.from_numpy(frames).cuda()
    d_pyr = torch.full((B, pb.rows, pb.vstep), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_ctx.set_option("build_chain", chain)
    try:
        pb(d_fr, d_pyr)
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_option("build_chain", 0)
    got = d_pyr.cpu().numpy()
    mask = build_defined_mask(pb, steps)
    assert (got[:, ~mask] == 0xAB).all()
    got = np.where(mask[None], got, 0)
    for b in range(B):
        exp = np.zeros((pb.rows, pb.vstep), np.uint8)
        w, h, r0, _ = pb.levels[0]
        exp[r0:r0 + h, :w] = frames[b]
        orc.gaussian5x5(exp[r0:], w, h)
        for k, st in enumerate(steps):
            w, h, r0, _ = pb.levels[k]
            tmp = exp[r0:].copy()
            (orc.bilinear7_8 if st == 1 else orc.bilinear13_16)(tmp, w, h)
            w1, h1, r1, _ = pb.levels[k + 1]
            N, M = (8, 7) if st == 1 else (16, 13)
            oh, ow = -(-h // N) * M, -(-w // N) * M
            exp[r1:r1 + oh, :ow] = tmp[:oh, :ow]
            assert (w1, h1) == (w * M // N, h * M // N)
        assert (got[b] == exp).all(), (w0, h0, b, np.argwhere(got[b] != exp)[:4])
    d_clean = torch.from_numpy(got).cuda()
    c, k, d, _ = run_frontend(gpu_ctx, pb.levels, pb.vstep, pb.rows, d_clean, 32768)
    assert_matches(c, k, d, 1, oracle_levels(orc, got[1], pb.levels), (w0, chain))


@pytest.fixture(scope="module")
def wide_matcher_inputs():
    """Layout 1 front-end outputs of frame A, of A moved by (2, 5) px (the next frame) and of A moved 24 px left (the
    right image of a stereo pair): 200 shapes per frame keep each side below ~3000 keypoints."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels, rows = layout1(), 3355
    l0 = synth.make_level0(710, 1920, 1080, 200)
    pyr = np.stack([host_pyramid(f, levels, VSTEP, rows)
                    for f in (l0, np.roll(l0, (2, 5), axis=(0, 1)), np.roll(l0, -24, axis=1))])
    fe = OrbFrontend(levels, vstep=VSTEP, rows=rows, max_keypoints=4096)
    kp, desc, counts = fe.alloc_outputs(3, torch.device("cuda:0"))
    fe(torch.from_numpy(pyr).to("cuda:0"), kp, desc, counts)
    torch.cuda.synchronize()
    kp, desc, counts = (t.cpu().numpy().view(np.uint32) for t in (kp, desc, counts))
    assert counts.max() <= 4096 and counts.min() > 2000
    return levels, pyr, kp, desc, counts


@pytest.mark.gpu
def test_scaled_window_matcher_on_wide_positions(gpu_ctx, wide_matcher_inputs):
    """The next frame against frame A at span 0 and 1 equals ref_scaled_window_match, with good matches at x >= 2048."""
    levels, _, kp, desc, counts = wide_matcher_inputs
    s = level_scales(levels)
    r = scale_radii(s)
    q = (kp[1:2], desc[1:2], counts[1:2])
    t = (kp[0:1], desc[0:1], counts[0:1])
    for span in (0, 1):
        got = run_scaled(gpu_ctx, levels, s, r, span, *q, *t)
        check_against_reference(got, levels, s, r, span, *q, *t)
        n = int(counts[1])
        x = (kp[1, :n] >> 12) & 0xFFF
        good = (got[0][0, :n].view(np.int32) >= 0) & (got[1][0, :n] < 32)
        assert (good & (x >= 2048)).sum() > 50, span


@pytest.mark.gpu
def test_stereo_matcher_on_wide_positions(gpu_ctx, wide_matcher_inputs):
    """Frame A against its 24 px shifted copy with ORB-SLAM2's disparity band (0..448) equals ref_stereo_match, with
    accepted matches at x >= 2048."""
    levels, pyr, kp, desc, counts = wide_matcher_inputs
    s = level_scales(levels)
    rr = row_radii(s)
    left = (kp[0:1], desc[0:1], counts[0:1])
    right = (kp[2:3], desc[2:3], counts[2:3])
    pyrs = (pyr[0:1], pyr[2:3])
    kw = {**KW, "min_disp": 0, "max_disp": 448}
    got = run_stereo(gpu_ctx, levels, s, rr, pyrs, left, right, **kw)
    check_stereo(got, levels, s, rr, pyrs, left, right, min_disp=0, max_disp=448)
    n = int(counts[0])
    x = (kp[0, :n] >> 12) & 0xFFF
    accepted = got[0][3][0, :n] != 0xFFFFFFFF
    assert int(got[1][0]) > 500 and (accepted & (x >= 2048)).sum() > 100
