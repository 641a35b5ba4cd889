"""GPU parity suite (pytest -m gpu): HIP path through the C ABI vs the oracle, bit-exact."""
import numpy as np
import pytest

from conftest import SURVEY_PINS, sha16

pytestmark = pytest.mark.gpu


def _levels_stagewise(fe, orc, img, levels, ctx, border=16, thr=20, hthr=1 << 15):
    det_g = np.zeros_like(img)
    det_o = np.zeros_like(img)
    for w, h, r0 in levels:
        fe.fastDetect(w, h, img[r0:r0 + h], det_g[r0:r0 + h], thr, border=border, ctx=ctx)
        orc.fast_detect(img[r0:r0 + h], det_o[r0:r0 + h], w, h, thr, border=border)
    assert (det_g == det_o).all(), f"FAST maps differ at {np.argwhere(det_g != det_o)[:5]}"
    sc_g, sc_o = det_g.copy(), det_o.copy()
    if border < 4:          # Fast.h:46-49: Harris needs border >= 4; the ABI rejects it instead of UB
        from pislam_amd.capi import PislamError
        with pytest.raises(PislamError):
            fe.fastScoreHarris(levels[0][0], levels[0][1], img, hthr, sc_g, border=border, ctx=ctx)
        return det_g, sc_g
    for w, h, r0 in levels:
        fe.fastScoreHarris(w, h, img[r0:r0 + h], hthr, sc_g[r0:r0 + h], border=border, ctx=ctx)
        orc.fast_score_harris(img[r0:r0 + h], sc_o[r0:r0 + h], w, h, hthr, border=border)
    assert (sc_g == sc_o).all(), f"score maps differ at {np.argwhere(sc_g != sc_o)[:5]}"
    return det_g, sc_g


def test_four_call_api_on_reference_demo_pyramid(gpu_ctx, orc, demo):
    """README.md:67-82 call sequence through the drop-in API; every stage equals the reference's
    recorded outputs (SURVEY §8c pins) on the reference's own input."""
    from pislam_amd import frontend as fe
    img, levels = demo["img"], demo["levels"]
    det, score = _levels_stagewise(fe, orc, img, levels, gpu_ctx)
    assert sha16(det) == SURVEY_PINS["det"] and sha16(score) == SURVEY_PINS["score"]
    kp = np.concatenate([fe.fastExtract(w, h, score[r0:r0 + h], ctx=gpu_ctx) + np.uint32(r0) for w, h, r0 in levels])
    assert sha16(kp.astype(np.uint32)) == SURVEY_PINS["kp"] and (kp == demo["kp"]).all()
    kpb = np.concatenate([fe.fastExtract(w, h, score[r0:r0 + h], logBucketSize=4, bucketLimit=3, ctx=gpu_ctx)
                          + np.uint32(r0) for w, h, r0 in levels])
    assert sha16(kpb.astype(np.uint32)) == SURVEY_PINS["kp_bucket43"]
    cen = fe.orbCentroids(img, kp, ctx=gpu_ctx)
    assert sha16(cen) == SURVEY_PINS["centroids"]
    ang = fe.atan2(cen, ctx=gpu_ctx)
    assert sha16(ang) == SURVEY_PINS["angles"]
    desc = fe.orbCompute(img, kp, ctx=gpu_ctx)
    assert sha16(desc) == SURVEY_PINS["desc"] and (desc == demo["desc"]).all()


@pytest.fixture(params=[1, 2], ids=["staged", "fused"])
def pipeline(request, gpu_ctx):
    """Run the batch tests on both pipelines; the fused one also dumps its LDS score tiles."""
    gpu_ctx.set_option("pipeline", request.param)
    gpu_ctx.set_option("dump_score", 1)
    yield request.param
    gpu_ctx.set_option("pipeline", 0)
    gpu_ctx.set_option("dump_score", 0)
    gpu_ctx.set_option("strip_rows", 0)


@pytest.fixture(params=[8, 0], ids=["one-launch", "three-launches"])
def frame(request, gpu_ctx):
    """Small batches run as ONE launch (pf::k_frame; option "frame": 1 = the default, batches of 1 or 2 pyramids; 8 = up to 8)
    or as strips -> overflow pass -> gather+ORB."""
    gpu_ctx.set_option("frame", request.param)
    yield request.param
    gpu_ctx.set_option("frame", 1)


@pytest.mark.parametrize("batch", [1, 2, 4, 8, 9])
def test_one_launch_path_on_reference_demo_pyramid(gpu_ctx, demo, orc, batch):
    """The reference's own use is a frame at a time (demo.cpp:77-101): small batches take the one-launch path
    (strip workgroups, then the gather + ORB workgroups of the same grid waiting for their pyramid) — the demo pyramid
    against the SURVEY pins at every slot, a flipped pyramid in between against the oracle, the path reported by
    pislam_frontend_last_path, repeated calls (the launch re-arms its own hand-over counters) and a hipGraph replay."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    img = demo["img"]
    dev = torch.device("cuda:0")
    flip = img[::-1].copy()
    host = np.stack([flip if (b % 3) == 1 else img for b in range(batch)])
    okp, odesc, _ = orc.pyramid(flip, demo["levels"])
    gpu_ctx.set_option("frame", 8)                    # (the default takes batches of 1 and 2)
    fe = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=4096, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(batch, dev)
    d_pyr = torch.from_numpy(host).to(dev)

    def check():
        c = counts.cpu().numpy().view(np.uint32)
        k = kp.cpu().numpy().view(np.uint32)
        d = desc.cpu().numpy().view(np.uint32)
        for b in range(batch):
            if (b % 3) == 1:
                assert c[b] == len(okp) and (k[b, :len(okp)] == okp).all() and (d[b, :len(okp)] == odesc).all(), b
            else:
                assert c[b] == 1754 and sha16(k[b, :1754]) == SURVEY_PINS["kp"] and sha16(d[b, :1754]) == SURVEY_PINS["desc"], b

    for rep in range(3):
        for t in (kp, desc, counts):
            t.zero_()
        fe(d_pyr, kp, desc, counts)
        torch.cuda.synchronize()
        one = bool(fe.last_path() & fe.PATH_ONE_LAUNCH)
        assert one == (batch <= 8), (batch, fe.last_path())
        assert fe.last_stats()[0] == 0                     # the demo photo stays on the fast path
        check()
    gpu_ctx.set_option("frame", 1)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    assert bool(fe.last_path() & fe.PATH_ONE_LAUNCH) == (batch <= 2)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        from pislam_amd.capi import Context
        ctx = Context(device=0, stream=side.cuda_stream)
        fe2 = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=4096, ctx=ctx)
        fe2.reserve(batch)
        fe2(d_pyr, kp, desc, counts)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fe2(d_pyr, kp, desc, counts)
        for rep in range(3):
            for t in (kp, desc, counts):
                t.zero_()
            g.replay()
            side.synchronize()
            check()


def test_one_launch_timeout_is_reported_and_the_context_recovers(demo):
    """The one-launch path's bounded wait (pf::k_frame): a strip workgroup that never publishes its hand-over (test hook
    "frame_test": the first strip workgroup skips its release, the poll limit is 2^12) makes the gather + ORB workgroups of
    that pyramid give up.  Nothing stale may be returned silently: counts[0] is PISLAM_COUNT_INVALID, the NEXT call on the
    context fails once with PISLAM_ERR_HIP naming the time-out, and from then on the context takes three launches
    (PISLAM_PATH_FRAME_TIMED_OUT) with the reference's results — also on a pipeline lane, whose captured one-launch graph
    is dropped."""
    import torch
    from pislam_amd.capi import Context, Pipeline, PislamError
    from pislam_amd.frontend import OrbFrontend
    dev = torch.device("cuda:0")
    img = demo["img"]
    d_pyr = torch.from_numpy(np.stack([img, img[::-1].copy()])).to(dev)
    ctx = Context(device=0)
    fe = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=4096, ctx=ctx)
    kp, desc, counts = fe.alloc_outputs(2, dev)

    def good(k, d, c, b=0):
        c_ = c.cpu().numpy().view(np.uint32)
        return c_[b] == 1754 and sha16(k.cpu().numpy().view(np.uint32)[b, :1754]) == SURVEY_PINS["kp"] and \
            sha16(d.cpu().numpy().view(np.uint32)[b, :1754]) == SURVEY_PINS["desc"]

    fe(d_pyr, kp, desc, counts)                         # a healthy one-launch call first
    ctx.synchronize()
    assert fe.last_path() & fe.PATH_ONE_LAUNCH and good(kp, desc, counts)
    ctx.set_option("frame_test", 1 | (12 << 8))
    counts.fill_(7)
    fe(d_pyr, kp, desc, counts)                         # pyramid 0's hand-over never completes
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    assert c[0] == fe.COUNT_INVALID, c                  # (pyramid 1 of the same launch is complete and correct)
    ctx.set_option("frame_test", 0)
    with pytest.raises(PislamError, match="timed out"):
        fe(d_pyr, kp, desc, counts)                     # reported once, state reset
    for rep in range(2):
        for t in (kp, desc, counts):
            t.zero_()
        fe(d_pyr, kp, desc, counts)
        ctx.synchronize()
        assert not (fe.last_path() & fe.PATH_ONE_LAUNCH) and (fe.last_path() & fe.PATH_FRAME_TIMED_OUT)
        assert good(kp, desc, counts)
    ctx.set_option("frame_rearm", 1)                    # the path can be taken again (its counters were reset)
    for t in (kp, desc, counts):
        t.zero_()
    fe(d_pyr, kp, desc, counts)
    ctx.synchronize()
    assert fe.last_path() & fe.PATH_ONE_LAUNCH and good(kp, desc, counts)
    # ... and reported by pislam_ctx_synchronize when no further call follows
    ctx.set_option("frame_test", 1 | (12 << 8))
    fe(d_pyr, kp, desc, counts)
    with pytest.raises(PislamError, match="timed out"):
        ctx.synchronize()
    ctx.set_option("frame_test", 0)
    # a pipeline lane: eager, captured, replayed — then the time-out: the next submit fails once, the graph is dropped,
    # later submits run as three launches
    pipe = Pipeline(device=0, depth=1)
    one = d_pyr[:1]
    k1, d1, c1 = fe.alloc_outputs(1, dev)
    for rep in range(4):
        pipe.submit(fe.params, fe.levels, one, k1, d1, c1)
    pipe.synchronize()
    assert pipe.stats()["replayed_from_graphs"] >= 1 and good(k1, d1, c1)
    assert fe.last_path_of(pipe.lane(0)) & fe.PATH_ONE_LAUNCH
    pipe.set_option("frame_test", 1 | (12 << 8))        # (drops the captured calls: the next two run eagerly, then capture)
    pipe.submit(fe.params, fe.levels, one, k1, d1, c1)
    torch.cuda.synchronize()
    assert c1.cpu().numpy().view(np.uint32)[0] == fe.COUNT_INVALID
    pipe.set_option("frame_test", 0)
    with pytest.raises(PislamError, match="timed out"):
        pipe.submit(fe.params, fe.levels, one, k1, d1, c1)
    for rep in range(4):
        c1.zero_()
        pipe.submit(fe.params, fe.levels, one, k1, d1, c1)
        pipe.synchronize()
        assert good(k1, d1, c1)
        p_ = fe.last_path_of(pipe.lane(0))
        assert not (p_ & fe.PATH_ONE_LAUNCH) and (p_ & fe.PATH_FRAME_TIMED_OUT), p_
    pipe.close()


def test_batch_path_on_reference_demo_pyramid(gpu_ctx, demo, pipeline, frame):
    import torch
    from pislam_amd.frontend import OrbFrontend
    img = demo["img"]
    dev = torch.device("cuda:0")
    pyr = torch.from_numpy(np.stack([img, img[::-1].copy(), img])).to(dev)   # same pyramid at batch slots 0 and 2
    fe = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=4096, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(3, dev)
    fe(pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    k = kp.cpu().numpy().view(np.uint32)
    d = desc.cpu().numpy().view(np.uint32)
    assert c[0] == 1754 == c[2]
    assert sha16(k[0, :1754]) == SURVEY_PINS["kp"] and sha16(d[0, :1754]) == SURVEY_PINS["desc"]
    assert (k[2] == k[0]).all() and (d[2] == d[0]).all()           # independent of batch position
    if pipeline == 2:
        # the reference's own demo photo must stay on the fast path: no strip redone by the overflow pass
        redone, strips = fe.last_stats()
        assert strips > 0 and redone == 0, (redone, strips)
    try:
        sm = fe.score_map(0)
    except Exception:
        sm = None
    if sm is not None:
        assert sha16(sm) == SURVEY_PINS["score"]
    # bucketed mode (README's recommended <4,3>), same pipeline
    feb = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=4096, log_bucket_size=4,
                      bucket_limit=3, ctx=gpu_ctx)
    feb(pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    assert c[0] == 1315 and sha16(kp.cpu().numpy().view(np.uint32)[0, :1315]) == SURVEY_PINS["kp_bucket43"]


@pytest.mark.parametrize("tile_cols,alias,orb_in_strip", [(64, 1, 0), (128, 1, 1), (200, 0, 0), (320, 1, 0)])
def test_x_tiles_as_work_items_reproduce_reference_order(gpu_ctx, demo, tile_cols, alias, orb_in_strip):
    """Levels cut into x-tiles that separate workgroups process like levels of their own (option tile_cols; the
    default cuts levels wider than 704 classified columns — BASELINE config 4): the tiles' per-strip lists must
    merge back into the reference's block-raster order (Fast.h:228-320) / bucket flush order (Fast.h:211-226),
    boundary blocks must see their neighbours' scores, and the right-edge 0xff columns (Fast.h:172) stay with
    the last tile.  Checked on the reference's demo photo (SURVEY pins) and a dense variant (overflow pass)."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    from oracle import orc
    img = demo["img"]
    dev = torch.device("cuda:0")
    noisy = (img.astype(np.int32) + np.random.default_rng(7).integers(-40, 41, img.shape)).clip(0, 255).astype(np.uint8)
    pyr = torch.from_numpy(np.stack([img, noisy])).to(dev)
    for k, v in dict(tile_cols=tile_cols, alias=alias, orb_in_strip=orb_in_strip).items():
        gpu_ctx.set_option(k, v)
    try:
        for lbs, lim, n, pin in ((0, 5, 1754, "kp"), (4, 3, 1315, "kp_bucket43"), (5, 2, None, None), (2, 1, None, None)):
            fe = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=16384, log_bucket_size=lbs,
                             bucket_limit=lim, ctx=gpu_ctx)
            kp, desc, counts = fe.alloc_outputs(2, dev)
            fe(pyr, kp, desc, counts)
            torch.cuda.synchronize()
            c = counts.cpu().numpy().view(np.uint32)
            k = kp.cpu().numpy().view(np.uint32)
            d = desc.cpu().numpy().view(np.uint32)
            if n is not None:
                assert c[0] == n and sha16(k[0, :n]) == SURVEY_PINS[pin]
                if lbs == 0:
                    assert sha16(d[0, :n]) == SURVEY_PINS["desc"]
            for b, im in enumerate((img, noisy)):
                okp, odesc, _ = orc.pyramid(im, demo["levels"], log_bucket=lbs, bucket_limit=lim)
                m = min(len(okp), 16384)
                assert c[b] == len(okp), (b, lbs, c[b], len(okp))
                assert (k[b, :m] == okp[:m]).all() and (d[b, :m] == odesc[:m]).all(), (b, lbs)
    finally:
        for k, v in dict(tile_cols=0, alias=1, orb_in_strip=0).items():
            gpu_ctx.set_option(k, v)


@pytest.mark.parametrize("orb_in_strip,rows_max", [(0, 0), (1, 0), (0, 56), (1, 44), (0, 64)])
def test_product_kernels_on_reference_demo_pyramid(gpu_ctx, demo, orb_in_strip, rows_max, frame):
    """The product instantiations (no debug hooks) with either ORB placement — one gather+ORB pass (default) or
    every strip describing its own keypoints (strip_body phase E, descriptors staged per strip) — and with the
    strip-height cap of small launches (28) and of large ones (56: up to 56-row strips on the narrow levels) —
    on the reference's demo photo and a dense variant that sends strips through the overflow pass."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    img = demo["img"]
    dev = torch.device("cuda:0")
    noisy = (img.astype(np.int32) + np.random.default_rng(1).integers(-40, 41, img.shape)).clip(0, 255).astype(np.uint8)
    pyr = torch.from_numpy(np.stack([img, noisy, img])).to(dev)
    gpu_ctx.set_option("orb_in_strip", orb_in_strip)
    gpu_ctx.set_option("strip_rows_max", rows_max)
    try:
        for lbs, lim, n, pin in ((0, 5, 1754, "kp"), (4, 3, 1315, "kp_bucket43")):
            fe = OrbFrontend(demo["levels"], vstep=640, rows=2210, max_keypoints=16384, log_bucket_size=lbs,
                             bucket_limit=lim, ctx=gpu_ctx)
            kp, desc, counts = fe.alloc_outputs(3, dev)
            fe(pyr, kp, desc, counts)
            torch.cuda.synchronize()
            c = counts.cpu().numpy().view(np.uint32)
            k = kp.cpu().numpy().view(np.uint32)
            d = desc.cpu().numpy().view(np.uint32)
            assert c[0] == n == c[2] and sha16(k[0, :n]) == SURVEY_PINS[pin]
            if lbs == 0:
                assert sha16(d[0, :n]) == SURVEY_PINS["desc"]
            assert (k[2] == k[0]).all() and (d[2] == d[0]).all()
            from oracle import orc
            okp, odesc, _ = orc.pyramid(noisy, demo["levels"], log_bucket=lbs, bucket_limit=lim)
            m = min(len(okp), 16384)
            assert c[1] == len(okp) and (k[1, :m] == okp[:m]).all() and (d[1, :m] == odesc[:m]).all()
            redone, strips = fe.last_stats()
            assert strips > 0 and (redone > 0 or lbs != 0 or True)
    finally:
        gpu_ctx.set_option("orb_in_strip", 0)
        gpu_ctx.set_option("strip_rows_max", 0)


@pytest.mark.parametrize("w,h,border,thr", [
    (64, 48, 16, 20),      # (w-2B) % 16 == 0
    (77, 61, 16, 20),      # odd (w-2B): over-classified right edge emits score-255 keypoints
    (90, 70, 16, 10),      # even, not multiple of 16
    (33, 33, 16, 20),      # a single classified column/row
    (32, 40, 16, 20),      # width == 2*border: nothing to do
    (50, 44, 3, 30),       # small border (detect only contract), xend past width
    (130, 47, 4, 0),       # threshold 0
    (100, 60, 16, 276),    # threshold truncated to uint8 (276 & 0xff = 20), Fast.h:58
])
def test_stage_parity_on_adversarial_levels(gpu_ctx, orc, w, h, border, thr):
    """Noise/blocks images with NON-zero padding right of the level (reads past `width`)."""
    from pislam_amd import frontend as fe
    rng = np.random.default_rng(w * 1000 + h)
    vstep = 160
    img = rng.integers(0, 256, (h, vstep), dtype=np.uint8)
    img[:, : w // 2] = (img[:, : w // 2] // 64) * 64
    det, score = _levels_stagewise(fe, orc, img, [(w, h, 0)], gpu_ctx, border=border, thr=thr)
    if border >= 16:
        for lb, lim in [(0, 5), (4, 3), (3, 1), (5, 7), (1, 2)]:
            g = fe.fastExtract(w, h, score, border=border, logBucketSize=lb, bucketLimit=lim, ctx=gpu_ctx)
            o = orc.fast_extract(score, w, h, border=border, log_bucket=lb, bucket_limit=lim)
            assert len(g) == len(o) and (g == o).all(), (lb, lim)
        kp = orc.fast_extract(score, w, h, border=border)
        if len(kp):
            for words in (8, 5, 1):
                assert (fe.orbCompute(img, kp, words=words, ctx=gpu_ctx) == orc.orb_compute(img, kp, words=words)).all()
            assert (fe.orbCentroids(img, kp, ctx=gpu_ctx) == orc.orb_centroids(img, kp)).all()


def test_score_map_with_stale_values_and_dense_scores(gpu_ctx, orc):
    """fastScoreHarris scores ANY non-zero byte (Fast.h:173-176); NMS on a dense random score map."""
    from pislam_amd import frontend as fe
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (80, 128), dtype=np.uint8)
    out = (rng.integers(0, 4, (80, 128)) == 0).astype(np.uint8) * rng.integers(1, 256, (80, 128)).astype(np.uint8)
    g, o = out.copy(), out.copy()
    fe.fastScoreHarris(120, 80, img, 1000, g, ctx=gpu_ctx)
    orc.fast_score_harris(img, o, 120, 80, 1000)
    assert (g == o).all()
    dense = rng.integers(0, 256, (80, 128), dtype=np.uint8)
    dense[rng.integers(0, 2, (80, 128)) == 0] = 200                      # many ties
    for lb, lim in [(0, 5), (4, 5), (2, 2), (6, 64)]:
        a = fe.fastExtract(121, 79, dense, logBucketSize=lb, bucketLimit=lim, ctx=gpu_ctx)
        b = orc.fast_extract(dense, 121, 79, log_bucket=lb, bucket_limit=lim)
        assert len(a) == len(b) and (a == b).all(), (lb, lim)
    # capacity clipping: count is the reference's count, storage is clipped
    import ctypes
    from pislam_amd.capi import ptr
    buf = np.zeros(7, np.uint32)
    n = ctypes.c_size_t(0)
    gpu_ctx.check(gpu_ctx.lib.pislam_fast_extract(gpu_ctx.h, 128, 16, 0, 5, 121, 79, ptr(dense), ptr(buf), 7,
                                                  ctypes.byref(n)), "extract")
    full = orc.fast_extract(dense, 121, 79)
    assert n.value == len(full) and (buf == full[:7]).all()


def test_harris_and_angle_primitives(gpu_ctx, orc, demo):
    from pislam_amd import frontend as fe
    img = demo["img"]
    rng = np.random.default_rng(5)
    pts = ((rng.integers(16, 600, 500).astype(np.uint32) << 12) | rng.integers(16, 2190, 500).astype(np.uint32))
    g = fe.harrisScorePoints(img, pts, 1 << 15, ctx=gpu_ctx)
    o = np.array([orc.lib().orc_harris_score_sobel(640, img.ctypes.data, int(p >> 12) & 0xFFF, int(p) & 0xFFF, 1 << 15)
                  for p in pts], np.uint8)
    assert (g == o).all()
    noise = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    noise[::2] = 255 - noise[::2] // 8
    pts = ((rng.integers(8, 56, 300).astype(np.uint32) << 12) | rng.integers(8, 56, 300).astype(np.uint32))
    for thr in (-(1 << 31), -5, 0, 1 << 15, (1 << 31) - 1):
        g = fe.harrisScorePoints(noise, pts, thr, ctx=gpu_ctx)
        o = np.array([orc.lib().orc_harris_score_sobel(64, noise.ctypes.data, int(p >> 12) & 0xFFF, int(p) & 0xFFF, thr)
                      for p in pts], np.uint8)
        assert (g == o).all(), thr
    # angle bins: exhaustive-ish sweep incl. zeros, axes, diagonals, extremes (Orb.h:310-387)
    xs = np.concatenate([rng.integers(-1365780, 1365781, 40000), [0, 0, 1, -1, 5, -5, 1365780, -1365780, 7, 7]])
    ys = np.concatenate([rng.integers(-1365780, 1365781, 40000), [0, 5, 0, 0, 5, 5, -1365780, 1365780, -7, 7]])
    n = (len(xs) + 3) // 4 * 4
    xs = np.pad(xs, (0, n - len(xs))).astype(np.int32)
    ys = np.pad(ys, (0, n - len(ys))).astype(np.int32)
    grouped = np.stack([xs.reshape(-1, 4), ys.reshape(-1, 4)], axis=1).reshape(-1)
    assert (fe.atan2(grouped, ctx=gpu_ctx) == orc.atan2_bins(grouped)).all()
    # the whole int32 domain of the public helper (pislam::atan2 takes any vector<int32_t>): extremes, powers of two
    # and their neighbours (float rounding boundaries of the int -> float conversion), random full-range pairs
    edge = np.array([0, 1, -1, 2, 3, 255, 256, 257, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 25) + 1,
                     (1 << 30) - 1, 1 << 30, (1 << 31) - 1, -(1 << 31), -(1 << 31) + 1, 0x7fffff80, 0x7fffffbf, 0x7fffffc0], np.int64)
    edge = np.concatenate([edge, -edge[edge > -(1 << 31)]]).astype(np.int32)
    ex, ey = np.meshgrid(edge, edge)
    wx = np.concatenate([ex.reshape(-1), rng.integers(-(1 << 31), 1 << 31, 60000)]).astype(np.int32)
    wy = np.concatenate([ey.reshape(-1), rng.integers(-(1 << 31), 1 << 31, 60000)]).astype(np.int32)
    n = (len(wx) + 3) // 4 * 4
    wx = np.pad(wx, (0, n - len(wx))); wy = np.pad(wy, (0, n - len(wy)))
    grouped = np.stack([wx.reshape(-1, 4), wy.reshape(-1, 4)], axis=1).reshape(-1).astype(np.int32)
    assert (fe.atan2(grouped, ctx=gpu_ctx) == orc.atan2_bins(grouped)).all()
    small = np.arange(-40, 41, dtype=np.int32)
    gx, gy = np.meshgrid(small, small)
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    n = (len(gx) + 3) // 4 * 4
    gx = np.pad(gx, (0, n - len(gx))); gy = np.pad(gy, (0, n - len(gy)))
    grouped = np.stack([gx.reshape(-1, 4), gy.reshape(-1, 4)], axis=1).reshape(-1).astype(np.int32)
    assert (fe.atan2(grouped, ctx=gpu_ctx) == orc.atan2_bins(grouped)).all()


def test_brief_describe_all_rotations(gpu_ctx, orc, demo):
    from pislam_amd import frontend as fe
    img = demo["img"]
    kp = demo["kp"][::13]
    rots = (np.arange(len(kp)) % 32).astype(np.uint8)          # includes out-of-range 30, 31
    g = fe.briefDescribePoints(img, kp, rots, ctx=gpu_ctx)
    for i, p in enumerate(kp):
        exp = orc.brief_describe(img, (int(p) >> 12) & 0xFFF, int(p) & 0xFFF, int(rots[i])) if rots[i] < 30 else 0
        assert (g[i] == exp).all(), (i, rots[i])


@pytest.mark.parametrize("strip_rows,sub_batches,run_len",
                         [(0, 1, 0), (16, 1, 1), (16, 1, 3), (32, 1, 2), (2, 1, 0), (64, 1, 64), (0, 2, 0), (0, 3, 1),
                          (16, 2, 5), (32, 3, 0), (0, 16, 0), (10, 1, 64), (12, 1, 7), (8, 1, 4)])
def test_fused_strip_heights(gpu_ctx, orc, strip_rows, sub_batches, run_len, frame):
    """The fused pipeline's result must not depend on how levels are cut into strips and runs of strips (halo
    rows carried over in LDS between the strips of a run), nor on the batch being cut into sub-batches."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    pyr = synth.make_batch(300, 3)
    dev = torch.device("cuda:0")
    gpu_ctx.set_option("pipeline", 2)
    gpu_ctx.set_option("dump_score", 1)
    gpu_ctx.set_option("strip_rows", strip_rows)
    gpu_ctx.set_option("sub_batches", sub_batches)
    gpu_ctx.set_option("run_len", run_len)
    try:
        ref = [orc.pyramid(pyr[b], levels, return_score=True) for b in range(3)]
        # alias: score tile laid over the dead image rows (default) / separate tiles; dump: HOOKS kernels
        # (score map compared too) / the product instantiation; ablate 512: every strip is forced onto
        # the overflow list and redone by k_fused_overflow with the scan fallbacks
        for alias, dump, ablate in [(1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 1, 512), (0, 1, 512)]:
            gpu_ctx.set_option("alias", alias)
            gpu_ctx.set_option("dump_score", dump)
            gpu_ctx.set_option("ablate", ablate)
            fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=4096, ctx=gpu_ctx)
            kp, desc, counts = fe.alloc_outputs(3, dev)
            for rep in range(2):          # twice: the overflow list must be emptied between steps
                fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
            torch.cuda.synchronize()
            c = counts.cpu().numpy().view(np.uint32)
            k = kp.cpu().numpy().view(np.uint32)
            d = desc.cpu().numpy().view(np.uint32)
            for b in range(3):
                okp, odesc, _, osc = ref[b]
                assert c[b] == len(okp), (alias, dump, ablate)
                assert (k[b, :c[b]] == okp).all() and (d[b, :c[b]] == odesc).all(), (alias, dump, ablate)
                if dump:
                    assert (fe.score_map(b) == osc).all(), (alias, dump, ablate)
    finally:
        gpu_ctx.set_option("pipeline", 0)
        gpu_ctx.set_option("dump_score", 0)
        gpu_ctx.set_option("strip_rows", 0)
        gpu_ctx.set_option("sub_batches", 1)
        gpu_ctx.set_option("run_len", 0)
        gpu_ctx.set_option("alias", 1)
        gpu_ctx.set_option("ablate", 0)


def test_fused_odd_shapes_and_unaligned_layouts(gpu_ctx, orc, frame):
    """Packed side-by-side layout (col0 != 0, not 16-aligned -> scalar staging path), ragged level
    sizes, odd (w-2B), levels too small to hold a keypoint, batch not a multiple of 8."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    rng = np.random.default_rng(77)
    vstep, rows = 400, 260
    levels = [(200, 150, 0, 0), (131, 97, 0, 205), (77, 61, 150, 7), (40, 33, 150, 100), (33, 40, 150, 150),
              (32, 32, 150, 200), (150, 49, 211, 16)]
    B = 11
    pyr = rng.integers(0, 256, (B, rows, vstep), dtype=np.uint8)
    pyr[:, :, ::3] = (pyr[:, :, ::3] // 96) * 96
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    res = {}
    for lb, lim in [(0, 5), (4, 3), (2, 1), (3, 2), (5, 40)]:
        for pl in (1, 2):   # (the persistent variant needs 16-byte aligned level columns: not this layout)
            gpu_ctx.set_option("pipeline", pl)
            try:
                fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=8192, log_bucket_size=lb,
                                 bucket_limit=lim, ctx=gpu_ctx)
                kp, desc, counts = fe.alloc_outputs(B, dev)
                fe(d_pyr, kp, desc, counts)
                torch.cuda.synchronize()
                res[pl] = tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
            finally:
                gpu_ctx.set_option("pipeline", 0)
        for a, b in zip(res[1], res[2]):
            assert (a == b).all(), (lb, lim)
        if lb:      # buckets vs the oracle on one pyramid (dense noise -> exercises the per-cell fallback)
            c, k, d = res[2]
            exp = []
            for (w, h, r0, c0) in levels:
                view = np.ascontiguousarray(pyr[3, r0:r0 + h].reshape(-1)[c0:])
                view = np.concatenate([view, np.zeros((-len(view)) % vstep, np.uint8)]).reshape(-1, vstep)
                lkp, _, _ = orc.pyramid(view, [(w, h, 0)], log_bucket=lb, bucket_limit=lim)
                exp.append(lkp + np.uint32((c0 << 12) | r0))
            exp = np.concatenate(exp)
            assert c[3] == len(exp) and (k[3, :len(exp)] == exp).all(), (lb, lim)
    gpu_ctx.set_option("pipeline", 1)
    fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=8192, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(B, dev)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    res[1] = tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    gpu_ctx.set_option("pipeline", 2)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    res[2] = tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    gpu_ctx.set_option("pipeline", 0)
    # and against the oracle, level by level (col0 != 0 -> offset views)
    c, k, d = res[2]
    for b in (0, 5, 10):
        exp = []
        for (w, h, r0, c0) in levels:
            view = np.ascontiguousarray(pyr[b, r0:r0 + h].reshape(-1)[c0:])
            pad = (-len(view)) % vstep
            view = np.concatenate([view, np.zeros(pad, np.uint8)]).reshape(-1, vstep)
            lkp, _, _ = orc.pyramid(view, [(w, h, 0)])
            exp.append(lkp + np.uint32((c0 << 12) | r0))
        exp = np.concatenate(exp)
        assert c[b] == len(exp) and (k[b, :len(exp)] == exp).all()
        assert (d[b, :len(exp)] == orc.orb_compute(pyr[b], exp)).all()


def test_batch_parity_on_synthetic_pyramids(gpu_ctx, orc, pipeline, frame):
    """bench workload (VGA 8-level x1.2, thr 20, Harris 1<<15): batch path vs oracle, bit-exact,
    incl. score maps, with and without buckets, and with a clipped keypoint capacity."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    B = 6
    pyr = synth.make_batch(100, B)
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    for lb, lim, cap in [(0, 5, 4096), (4, 3, 4096), (0, 5, 300)]:
        fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=cap, log_bucket_size=lb, bucket_limit=lim,
                         ctx=gpu_ctx)
        kp, desc, counts = fe.alloc_outputs(B, dev)
        fe(d_pyr, kp, desc, counts)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(np.uint32)
        k = kp.cpu().numpy().view(np.uint32)
        d = desc.cpu().numpy().view(np.uint32)
        for b in range(B):
            okp, odesc, _, osc = orc.pyramid(pyr[b], levels, log_bucket=lb, bucket_limit=lim, return_score=True)
            assert c[b] == len(okp), (b, c[b], len(okp))
            n = min(len(okp), cap)
            assert (k[b, :n] == okp[:n]).all(), b
            assert (d[b, :n] == odesc[:n]).all(), b
            try:
                sm = fe.score_map(b)
            except Exception:
                sm = None
            if sm is not None:
                assert (sm == osc).all(), b


def test_full_batch_properties(gpu_ctx, orc, pipeline):
    """BASELINE config 2 size (batch 256): size-independent properties — results do not depend on
    the batch slot, repeated runs are bit-identical (ordered compaction, no atomics-order), a sample
    of slots equals the oracle, every keypoint lies inside its level, list order is the reference's."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    base = synth.make_batch(0, 8)
    batch = 256
    idx = np.arange(batch) % 8
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(base).to(dev)[torch.from_numpy(idx).to(dev)].contiguous()
    fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=4096, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(batch, dev)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c1, k1, d1 = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c2, k2, d2 = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    assert (c1 == c2).all() and (k1 == k2).all() and (d1 == d2).all()
    for b in range(8, batch):
        n = c1[b]
        assert n == c1[b % 8] and (k1[b, :n] == k1[b % 8, :n]).all() and (d1[b, :n] == d1[b % 8, :n]).all()
    for b in (0, 3, 7):
        okp, odesc, _ = orc.pyramid(base[b], levels)
        assert c1[b] == len(okp) and (k1[b, :len(okp)] == okp).all() and (d1[b, :len(okp)] == odesc).all()
    # geometry + ordering invariants for every slot
    for b in range(0, batch, 17):
        n = c1[b]
        x = (k1[b, :n] >> 12) & 0xFFF
        y = k1[b, :n] & 0xFFF
        lvl = np.zeros(n, int)
        for li, (w, h, r0) in enumerate(levels):
            m = (y >= r0) & (y < r0 + h)
            lvl[m] = li
            assert ((x[m] >= 16) & (x[m] <= w - 16) & (y[m] - r0 >= 16) & (y[m] - r0 <= h - 16)).all()
        assert (np.diff(lvl) >= 0).all()
        key = lvl * (1 << 24) + ((y - np.array([levels[l][2] for l in lvl])) // 2) * 4096 + x // 2
        assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("nshapes", [148, None], ids=["on-spec-148-shapes", "dense-320-shapes"])
def test_full_batch_properties_1280x960(gpu_ctx, orc, nshapes):
    """BASELINE configs[3] at its bench size (batch 256; x-tiled wide levels, packed shelves) on BOTH generators bench.py
    runs: 148 shapes per frame = the on-spec workload (`--workload 1280x960`: "~2000 kp/frame", checked here: 1900 <= mean
    <= 2100) and the area-scaled 320 shapes (`1280x960-dense`, ~4400 keypoints: what rounds 2-4 measured).  Repeated runs
    bit-identical, results independent of the batch slot, a sample of slots equal to the oracle (orc_pyramid4)."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    dev = torch.device("cuda:0")
    levels = synth.packed_level_table(1280, 960)
    rows = synth.pyramid_rows(levels)
    base = synth.make_batch(0, 8, w0=1280, h0=960, vstep=1280, levels=levels, nshapes=nshapes)
    batch = 256
    idx = torch.arange(batch, device=dev) % 8
    d_pyr = torch.from_numpy(base).to(dev)[idx].contiguous()
    fe = OrbFrontend(levels, vstep=1280, rows=rows, max_keypoints=8192, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(batch, dev)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c1, k1, d1 = (t.cpu().numpy().view(np.uint32).copy() for t in (counts, kp, desc))
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c2, k2, d2 = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    assert (c1 == c2).all() and (k1 == k2).all() and (d1 == d2).all()
    if nshapes == 148:
        assert 1900 <= float(c1[:8].mean()) <= 2100, c1[:8]          # BASELINE.json configs[3]: "~2000 kp/frame"
    else:
        assert float(c1[:8].mean()) > 3500, c1[:8]
    for b in range(8, batch):
        n = min(int(c1[b]), 8192)
        assert c1[b] == c1[b % 8] and (k1[b, :n] == k1[b % 8, :n]).all() and (d1[b, :n] == d1[b % 8, :n]).all()
    for b in (0, 5):
        okp, odesc, _ = orc.pyramid4(base[b], levels)
        m = min(len(okp), 8192)
        assert c1[b] == len(okp) and (k1[b, :m] == okp[:m]).all() and (d1[b, :m] == odesc[:m]).all()
    redone, strips = fe.last_stats()
    assert strips > 0 and redone == 0


def test_full_batch_properties_720p_build(gpu_ctx, orc):
    """BASELINE configs[4] at its bench size (batch 64, pyramid built on the device): the steady-state refill reproduces the
    first build, results independent of the batch slot, a sample of slots equal to the oracle (orc_pyramid4)."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend, PyramidBuilder
    dev = torch.device("cuda:0")
    # ---- configs[4]: 64 720p frames -> pyramids built on the device -> ORB ----
    pb = PyramidBuilder(1280, 720, ctx=gpu_ctx)
    frames = np.stack([synth.make_level0(100 + i, 1280, 720) for i in range(4)])
    B = 64
    d_fr = torch.from_numpy(frames).to(dev)[torch.arange(B, device=dev) % 4].contiguous()
    d_pyr = torch.zeros((B, pb.rows, pb.vstep), dtype=torch.uint8, device=dev)
    pb(d_fr, d_pyr)
    snap = d_pyr.clone()
    pb(d_fr, d_pyr, margins_clean=True)                     # the bench's steady-state refill
    torch.cuda.synchronize()
    assert torch.equal(snap, d_pyr)
    fe = OrbFrontend(pb.levels, vstep=pb.vstep, rows=pb.rows, max_keypoints=8192, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(B, dev)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c, k, d = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    host = d_pyr[:4].cpu().numpy()
    for b in range(4, B):
        n = int(c[b])
        assert c[b] == c[b % 4] and (k[b, :n] == k[b % 4, :n]).all() and (d[b, :n] == d[b % 4, :n]).all()
    for b in range(2):
        okp, odesc, _ = orc.pyramid4(host[b], pb.levels)
        assert c[b] == len(okp) and (k[b, :len(okp)] == okp).all() and (d[b, :len(okp)] == odesc).all()


def test_packed_1280x960_layout(gpu_ctx, orc):
    """BASELINE configs[3]: 1280x960, vstep 1280, levels 4|5 and 6|7 side by side (12-bit y limit of
    encodeFast, Util.h:27-29): both pipelines equal the oracle run level by level."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = synth.packed_level_table(1280, 960)
    rows = synth.pyramid_rows(levels)
    assert rows == 3768 and max(t[3] + t[0] for t in levels) <= 1280
    pyr = synth.make_batch(900, 2, w0=1280, h0=960, vstep=1280, levels=levels)
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    res = {}
    for pl in (1, 2):
        gpu_ctx.set_option("pipeline", pl)
        try:
            fe = OrbFrontend(levels, vstep=1280, rows=rows, max_keypoints=16384, ctx=gpu_ctx)
            kp, desc, counts = fe.alloc_outputs(2, dev)
            fe(d_pyr, kp, desc, counts)
            torch.cuda.synchronize()
            res[pl] = tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
        finally:
            gpu_ctx.set_option("pipeline", 0)
    for a, b in zip(res[1], res[2]):
        assert (a == b).all()
    c, k, d = res[2]
    for b in range(2):
        exp = []
        for (w, h, r0, c0) in levels:
            view = np.ascontiguousarray(pyr[b, r0:r0 + h].reshape(-1)[c0:])
            view = np.concatenate([view, np.zeros((-len(view)) % 1280, np.uint8)]).reshape(-1, 1280)
            lkp, _, _ = orc.pyramid(view, [(w, h, 0)])
            exp.append(lkp + np.uint32((c0 << 12) | r0))
        exp = np.concatenate(exp)
        assert c[b] == len(exp) and (k[b, :len(exp)] == exp).all()
        assert (d[b, :len(exp)] == orc.orb_compute(pyr[b], exp)).all()
        assert ((k[b, :len(exp)] & 0xFFF) < 4096).all()


def test_fused_unaligned_vstep(gpu_ctx, orc):
    """vstep % 16 != 0: scalar LDS staging + generic gather / per-keypoint ORB kernels on the fused path."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    rng = np.random.default_rng(5)
    vstep, rows = 203, 150
    levels = [(150, 90, 0, 0), (101, 60, 90, 3)]
    pyr = rng.integers(0, 256, (5, rows, vstep), dtype=np.uint8)
    pyr[:, :, ::2] = (pyr[:, :, ::2] // 128) * 128
    dev = torch.device("cuda:0")
    gpu_ctx.set_option("pipeline", 2)
    try:
        fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=4096, ctx=gpu_ctx)
        kp, desc, counts = fe.alloc_outputs(5, dev)
        fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_option("pipeline", 0)
    c, k, d = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    for b in range(5):
        exp = []
        for (w, h, r0, c0) in levels:
            view = np.ascontiguousarray(pyr[b, r0:r0 + h].reshape(-1)[c0:])
            view = np.concatenate([view, np.zeros((-len(view)) % vstep, np.uint8)]).reshape(-1, vstep)
            lkp, _, _ = orc.pyramid(view, [(w, h, 0)])
            exp.append(lkp + np.uint32((c0 << 12) | r0))
        exp = np.concatenate(exp)
        assert c[b] == len(exp) and (k[b, :len(exp)] == exp).all()
        assert (d[b, :len(exp)] == orc.orb_compute(pyr[b], exp)).all()


@pytest.mark.parametrize("buckets", [0, 1])
def test_cpp_dropin_readme_loop_runs_on_gpu(tmp_path, demo, buckets):
    """The reference README.md:59-82 loop as a C++ program against include/pislam/*.h + libpislam_hip.so
    (no Python, no torch in the process): outputs equal the reference's recorded results."""
    import os
    import subprocess
    import torch
    from conftest import ROOT
    from pislam_amd import build
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = build.build()
    exe = tmp_path / "readme_loop"
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "readme_loop.cpp"), "-o", str(exe),
                        "-L", os.path.dirname(lib), "-lpislam_hip", "-Wl,-rpath," + os.path.dirname(lib), "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = tmp_path / "pyr.raw"
    demo["img"].tofile(raw)
    outp = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(raw), str(outp), str(buckets)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    b = np.fromfile(outp, np.uint32)
    n, m = int(b[0]), int(b[1])
    kp, desc = b[2:2 + n], b[2 + n:2 + n + m]
    if buckets:
        assert n == 1315 and sha16(kp) == SURVEY_PINS["kp_bucket43"]
    else:
        assert n == 1754 and sha16(kp) == SURVEY_PINS["kp"] and sha16(desc) == SURVEY_PINS["desc"]
        rest = b[2 + n + m:]
        nc = int(rest[0])
        cen = rest[1:1 + nc].view(np.int32)
        assert sha16(cen) == SURVEY_PINS["centroids"]
        tail = rest[1 + nc:].tobytes()
        na = int(np.frombuffer(tail[:4], np.uint32)[0])
        assert sha16(np.frombuffer(tail[4:4 + na], np.uint8)) == SURVEY_PINS["angles"]


def test_batch_call_is_hipgraph_capturable(gpu_ctx, orc):
    """After pislam_frontend_reserve the batch call allocates nothing and never synchronises, so it can be
    captured into a hipGraph (torch.cuda.CUDAGraph) and replayed; replays give identical results."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    pyr = synth.make_batch(40, 4)
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=4096, ctx=ctx)
        fe.reserve(4)
        kp, desc, counts = fe.alloc_outputs(4, dev)
        fe(d_pyr, kp, desc, counts)                     # warm-up outside the capture (module load, option checks)
        side.synchronize()
        ref = tuple(t.clone() for t in (kp, desc, counts))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fe(d_pyr, kp, desc, counts)
        for t in (kp, desc, counts):
            t.zero_()
        g.replay()
        side.synchronize()
        for a, b in zip(ref, (kp, desc, counts)):
            assert torch.equal(a, b)
        d_pyr.copy_(torch.from_numpy(synth.make_batch(60, 4)).to(dev))   # new input, same graph
        g.replay()
        side.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    okp, odesc, _ = orc.pyramid(synth.make_pyramid(61), levels)
    assert c[1] == len(okp) and (kp.cpu().numpy().view(np.uint32)[1, :len(okp)] == okp).all()


def test_first_bucket_mode_call_after_reserve_is_capturable(gpu_ctx, orc):
    """pislam_frontend_reserve sizes the bucket selection pass's staging too (round-4 advisor finding: w_ustage / w_ucount were
    allocated by the first bucket-mode call itself — a synchronising hipMalloc inside a capture): reserve, then capture the
    VERY FIRST <4,3> call on the context (only a call without buckets ran before: module load), replay, compare with the oracle."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend
    levels = synth.level_table()
    pyr = synth.make_batch(44, 3)
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        fe0 = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=4096, ctx=ctx)
        kp, desc, counts = fe0.alloc_outputs(3, dev)
        fe0(d_pyr, kp, desc, counts)                    # no buckets: loads the module, touches none of the selection buffers
        fe = OrbFrontend(levels, vstep=640, rows=2210, max_keypoints=4096, ctx=ctx, log_bucket_size=4, bucket_limit=3)
        fe.reserve(3)
        side.synchronize()
        for t in (kp, desc, counts):
            t.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fe(d_pyr, kp, desc, counts)                 # the first bucket-mode call of this context
        g.replay()
        side.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    kk, dd = kp.cpu().numpy().view(np.uint32), desc.cpu().numpy().view(np.uint32)
    for b in range(3):
        okp, odesc, _ = orc.pyramid(pyr[b], levels, log_bucket=4, bucket_limit=3)
        assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (dd[b, :len(okp)] == odesc).all(), b


def test_first_call_of_every_fused_path_after_reserve_is_capturable(gpu_ctx, orc):
    """pislam_frontend_reserve and the batch call size the workspace from one plan, so after a reserve the first call of ANY
    configuration allocates nothing.  For every path whose workspace differs (three launches, one launch, buckets in the
    strips, orb_in_strip, alias 0, two sub-batches, generic ORB): a fresh context runs one call of another shape (module
    load), sets the options, reserves, captures its first call of that configuration, replays it and matches the oracle."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend as FE
    levels, small = synth.level_table(), synth.level_table(320, 240, 4)
    rows = synth.pyramid_rows(levels)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    d_small = torch.from_numpy(synth.make_batch(0, 3, w0=320, h0=240, nlevels=4, levels=small)).to(dev)
    cases = [  # name, batch, options, (log_bucket_size, bucket_limit), vstep, path
        ("three launches", 4, {}, (0, 5), 640, FE.PATH_FUSED),
        ("one launch", 1, {}, (0, 5), 640, FE.PATH_FUSED | FE.PATH_ONE_LAUNCH),
        ("buckets in strips", 3, {"bucket_select": 0}, (4, 3), 640, FE.PATH_FUSED | FE.PATH_BUCKETS_IN_STRIPS),
        ("orb_in_strip", 3, {"orb_in_strip": 1}, (0, 5), 640, FE.PATH_FUSED),
        ("alias 0", 3, {"alias": 0}, (0, 5), 640, FE.PATH_FUSED),
        ("sub_batches 2", 4, {"sub_batches": 2}, (0, 5), 640, FE.PATH_FUSED),
        ("generic ORB", 3, {}, (0, 5), 648, FE.PATH_FUSED | FE.PATH_GENERIC_ORB),
    ]
    for i, (name, batch, options, (lbs, limit), vstep, path) in enumerate(cases):
        pyr = synth.make_batch(70 + 8 * i, batch, vstep=vstep, levels=levels)
        d_pyr = torch.from_numpy(pyr).to(dev)
        with torch.cuda.stream(side):
            ctx = Context(device=0, stream=side.cuda_stream)
            fe0 = FE(small, vstep=320, rows=synth.pyramid_rows(small), max_keypoints=2048, ctx=ctx)
            fe0(d_small, *fe0.alloc_outputs(3, dev))
            for k, v in options.items():
                ctx.set_option(k, v)
            fe = FE(levels, vstep=vstep, rows=rows, max_keypoints=4096, ctx=ctx, log_bucket_size=lbs, bucket_limit=limit)
            fe.reserve(batch)
            kp, desc, counts = fe.alloc_outputs(batch, dev)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fe(d_pyr, kp, desc, counts)             # the first call of this configuration on the context
            g.replay()
            side.synchronize()
        assert fe.last_path() == path, (name, fe.last_path())
        c = counts.cpu().numpy().view(np.uint32)
        kk, dd = kp.cpu().numpy().view(np.uint32), desc.cpu().numpy().view(np.uint32)
        for b in range(batch):
            okp, odesc, _ = orc.pyramid(pyr[b], levels, log_bucket=lbs, bucket_limit=limit)
            assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (dd[b, :len(okp)] == odesc).all(), (name, b)
        del g
        ctx.close()


def test_dense_input_takes_the_overflow_pass_and_stays_exact(gpu_ctx, orc, frame):
    """Level 0: isolated bright dots on the lattice spanned by (4, 0) and (2, 1) — no lattice point lies on another's
    FAST ring, so every dot is a corner: one pixel in four, more than the fast path's on-chip corner queue (at most 4096
    entries) holds for a 32-row strip — and levels of uniform noise: the strips whose queue overflows are redone by the
    overflow pass (plain layout, scan fallbacks).  Results must not change and pislam_frontend_last_stats must report
    it; a second call must start from an empty overflow list."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = [(640, 120, 0), (133, 100, 120), (111, 83, 220)]
    rows = 303
    rng = np.random.default_rng(7)
    pyr = np.zeros((2, rows, 640), np.uint8)
    yy, xx = np.mgrid[0:120, 0:640]
    dots = np.full((120, 640), 20, np.uint8)
    lattice = (xx - 2 * yy) % 4 == 0
    dots[lattice] = rng.integers(120, 256, int(lattice.sum()), dtype=np.uint8)
    pyr[0, :120, :640] = dots
    for (w, h, r0) in levels[1:]:
        pyr[0, r0:r0 + h, :w] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    pyr[1] = synth.make_batch(5, 1, w0=640, h0=120, vstep=640, levels=levels)[0]   # a sparse one in the same batch
    dev = torch.device("cuda:0")
    gpu_ctx.set_option("pipeline", 2)
    gpu_ctx.set_option("strip_rows", 32)
    try:
        fe = OrbFrontend(levels, vstep=640, rows=rows, max_keypoints=8192, ctx=gpu_ctx)
        kp, desc, counts = fe.alloc_outputs(2, dev)
        for rep in range(2):
            fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
            torch.cuda.synchronize()
            redone, strips = fe.last_stats()
            assert strips > 0 and 0 < redone < strips, (redone, strips)
            c = counts.cpu().numpy().view(np.uint32)
            k = kp.cpu().numpy().view(np.uint32)
            d = desc.cpu().numpy().view(np.uint32)
            for b in range(2):
                okp, odesc, _ = orc.pyramid(pyr[b], levels)
                n = min(int(c[b]), 8192)
                assert c[b] == len(okp)
                assert (k[b, :n] == okp[:n]).all() and (d[b, :n] == odesc[:n]).all()
    finally:
        gpu_ctx.set_option("pipeline", 0)
        gpu_ctx.set_option("strip_rows", 0)


def test_count_exchange_on_rccl_single_rank_group():
    """pislam_amd.dist.CountExchange on the real RCCL backend (a 1-rank group is all a 1-GPU box offers):
    asynchronous all-gathers on RCCL's stream, two alternating buffers, waits ordered for buffer reuse."""
    import os
    import torch
    import torch.distributed as dist
    from pislam_amd import dist as pdist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1, device_id=dev)
    try:
        x = pdist.CountExchange(1, always_collective=True)
        bufs = [torch.zeros(256, dtype=torch.int32, device=dev) for _ in range(2)]
        for i in range(7):
            x.before_step()
            b = bufs[i & 1]
            b.fill_(i + 1)                    # "step i" writes its counts ...
            x.start(b)                        # ... and hands them to the exchange
        out = x.finish()
        torch.cuda.synchronize()
        assert out.shape == (256,) and (out.cpu().numpy() == 7).all()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("rccl", [0, 1])
def test_count_exchange_through_the_c_abi(rccl):
    """pislam_dist_* (include/pislam_hip.h): communicator from a unique id, all-gather on the context's
    collective stream ordered after the context stream, fences for buffer reuse, MAX all-reduce.  rccl=1
    keeps the real RCCL path (a 1-rank communicator is all a 1-GPU box offers); rank>1 needs more GPUs."""
    import os
    import torch
    from pislam_amd import capi, dist as pdist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    ctx = capi.Context(device=0, stream=s.cuda_stream)
    try:
        ctx.set_option("dist_rccl_single", rccl)
        with pytest.raises(capi.PislamError):
            ctx.dist_fence(1)                               # not initialised yet
        ctx.dist_init(capi.dist_unique_id() if rccl else None, 0, 1)
        assert ctx.lib.pislam_dist_world(ctx.h) == 1 and ctx.lib.pislam_dist_rank(ctx.h) == 0
        x = pdist.CountExchange(1, ctx=ctx, always_collective=True)
        assert "C ABI" in x.path
        bufs = [torch.zeros(256, dtype=torch.int32, device=dev) for _ in range(2)]
        with torch.cuda.stream(s):
            for i in range(9):
                x.before_step()
                bufs[i & 1].fill_(i + 1)                    # "step i" writes its counts on the context stream ...
                x.start(bufs[i & 1])                        # ... the all-gather follows it on the collective stream
            out = x.finish()
        torch.cuda.synchronize()
        assert out.shape == (256,) and (out.cpu().numpy() == 9).all()
        assert ctx.dist_allreduce_max(3.25) == 3.25
        with pytest.raises(capi.PislamError):
            ctx.dist_allgather_counts(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))   # host tensors
        ctx.dist_finalize()
        ctx.dist_finalize()                                 # idempotent
    finally:
        ctx.close()


def test_bench_step_with_the_c_abi_exchange_on_one_rank():
    """bench.py's N>1 step structure on this 1-GPU box: hipGraph replays on the launch stream(s), the count
    all-gather of every step through pislam_dist_* on the collective stream (a 1-rank RCCL communicator per
    pipeline context), fences for buffer reuse — with one pipeline and two output sets, and with 2 / 3
    pipelines (batches in flight on separate HIP streams) — and the same keypoint totals as the plain run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = []
    for extra in (["--streams", "1"], ["--streams", "1", "--force-exchange"], ["--streams", "2", "--force-exchange"],
                  ["--streams", "3", "--force-exchange"], []):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "7", "--warmup", "2", "--batch", "16",
                              "--no-cpu-baseline", "--spin-s", "0.1"] + extra, capture_output=True, text=True, timeout=300,
                             cwd=root, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        res.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    assert "none" in res[0]["config"]["count_allgather"] and "none" in res[4]["config"]["count_allgather"]
    for r, s in zip(res[1:4], (1, 2, 3)):
        assert "C ABI" in r["config"]["count_allgather"] and r["config"]["streams"] == s
        # every lane owns its own batch of pyramids (seeds): lane 0's batch is the same in every run
        lanes = r["config"]["keypoints_per_step_by_lane"]
        assert len(lanes) == s and lanes[0] == res[0]["config"]["keypoints_per_step_by_lane"][0] > 1600
        assert len(set(lanes)) == s and r["config"]["input_buffers_per_lane"] == "distinct"
        assert r["config"]["launch"] == res[0]["config"]["launch"] == "hipGraph replay"
    assert res[4]["config"]["keypoints_per_step_by_lane"][0] == res[0]["config"]["keypoints_per_step_by_lane"][0]
    assert len(res[4]["config"]["keypoints_per_step_by_lane"]) == 3


def test_bench_dump_outputs_are_the_same_in_every_run(tmp_path):
    """`bench.py --dump-outputs DIR`: the outputs of the last timed step as float64 .npy files, identical in a plain run and a
    --full run with the same arguments (the input is seeded); their counts are the keypoints the line reports for that
    step's lane, the --full run's own parity check passed on the same output set, the plain line carries none of the
    --full figures, and --steps is the number of timed steps the line reports."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines, dumps = [], []
    for run, mode in enumerate(([], ["--full"])):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "1", "--batch", "16",
                              "--no-cpu-baseline", "--spin-s", "0.1", "--dump-outputs", str(d)] + mode,
                             capture_output=True, text=True, timeout=300, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    plain, full = lines
    assert full["parity_in_run"]["ok"] and full["roofline"]["launch_ms"] > 0 and full["one_batch_ms"] > 0
    assert not {"parity_in_run", "roofline", "one_batch_ms", "cpu_baseline"} & set(plain)
    for r, a in zip(lines, dumps):
        assert r["steps"] == 5 and r["ms_per_step"] > 0
        assert set(a) == {"counts", "pyramids", "keypoints", "descriptors"} and all(v.dtype == np.float64 for v in a.values())
        assert r["dump_outputs"]["pyramids"] == "16 of 16" and len(a["counts"]) == 16
        lane_kp = r["config"]["keypoints_per_step_by_lane"][r["dump_outputs"]["lane"]]
        assert len(a["keypoints"]) == len(a["descriptors"]) == int(np.minimum(a["counts"], 4096).sum()) == lane_kp > 0
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])


def test_bench_self_launch_two_ranks_sharing_this_gpu():
    """Plain `python bench.py --gpus 2 --dist-backend gloo` (no torchrun environment): bench.py starts its two
    ranks itself and rank 0 reports n_gpus 2."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                          "--batch", "8", "--dist-backend", "gloo", "--no-cpu-baseline", "--spin-s", "0.1"],
                         capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["global_batch"] == 16


@pytest.mark.parametrize("w,h,seed", [(128, 96, 1007), (192, 80, 1007), (64, 128, 1008)])
def test_keypoints_at_the_last_pixel_of_the_buffer(gpu_ctx, orc, w, h, seed, frame):
    """ONE level that IS the buffer (w = vstep, h = rows), uniform noise: keypoints on the last classifiable row (h - 17) and
    column (w - 17), one of them on both — the patch rows of the gather's 48-byte windows then end one row above the end of
    the allocation, and the 12-byte pieces of a window (pf::orb_fetch) that reach past it are moved back as a whole: no
    piece that holds a patch byte may be among them.  The LAST pyramid of the batch ends the tensor."""
    import torch
    from pislam_amd.frontend import OrbFrontend
    levels = [(w, h, 0)]
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    okp, odesc, _ = orc.pyramid(img, levels)
    x, y = (okp >> 12) & 0xfff, okp & 0xfff
    assert ((x == w - 17) & (y == h - 17)).any() and (y == h - 17).sum() > 3 and (x == w - 17).sum() > 3
    dev = torch.device("cuda:0")
    for batch in (1, 3):
        pyr = np.repeat(img[None], batch, axis=0)
        fe = OrbFrontend(levels, vstep=w, rows=h, max_keypoints=2048, ctx=gpu_ctx)
        kp, desc, counts = fe.alloc_outputs(batch, dev)
        fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(np.uint32)
        k = kp.cpu().numpy().view(np.uint32)
        d = desc.cpu().numpy().view(np.uint32)
        for b in range(batch):
            assert c[b] == len(okp)
            assert (k[b, :c[b]] == okp).all() and (d[b, :c[b]] == odesc).all(), (batch, b)


@pytest.mark.parametrize("border", [16, 17, 19, 20, 32])
def test_fused_borders(gpu_ctx, orc, border, frame):
    """Any border >= 16 (odd ones too: block origins and x-tile edges then fall off dword boundaries), with
    and without buckets, on both LDS layouts."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    levels = [(320, 240, 0), (267, 200, 240), (222, 167, 440), (185, 139, 607)]
    rows = 746
    pyr = synth.make_batch(11, 2, w0=320, h0=240, vstep=320, levels=levels)
    dev = torch.device("cuda:0")
    try:
        for lbs, lim in ((0, 5), (3, 2)):
            ref = [orc.pyramid(pyr[b], levels, border=border, log_bucket=lbs, bucket_limit=lim) for b in range(2)]
            for alias in (1, 0):
                gpu_ctx.set_option("alias", alias)
                fe = OrbFrontend(levels, vstep=320, rows=rows, max_keypoints=4096, border=border, log_bucket_size=lbs,
                                 bucket_limit=lim, ctx=gpu_ctx)
                kp, desc, counts = fe.alloc_outputs(2, dev)
                fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
                torch.cuda.synchronize()
                c = counts.cpu().numpy().view(np.uint32)
                k = kp.cpu().numpy().view(np.uint32)
                d = desc.cpu().numpy().view(np.uint32)
                for b in range(2):
                    okp, odesc, _ = ref[b]
                    assert c[b] == len(okp), (border, lbs, alias)
                    assert (k[b, :c[b]] == okp).all() and (d[b, :c[b]] == odesc).all(), (border, lbs, alias)
    finally:
        gpu_ctx.set_option("alias", 1)


def test_bench_two_ranks_on_one_gpu_does_not_deadlock():
    """bench.py under torchrun with 2 ranks (gloo test mode: both ranks share this box's one GPU): every
    collective must be reached by both ranks the same number of times — time-based loops may hold none —
    and rank 0 prints the one JSON line."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29541", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "6",
           "--warmup", "2", "--batch", "16", "--dist-backend", "gloo", "--no-cpu-baseline", "--spin-s", "0.2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["value"] > 0 and d["config"]["global_batch"] == 32


@pytest.mark.gpu
def test_bench_eight_ranks_self_launched_on_one_gpu():
    """The path the driver takes without torchrun for BASELINE configs[2]: `python bench.py --gpus N` starts its own
    supervised workers (gloo test mode: the ranks share this box's one GPU, the count exchange goes through
    torch.distributed); one JSON line with n_gpus, the global batch, per-rank step times and an empty fallback list.
    Run with 4 ranks, not 8: eight workers beside this test process would hold one shared GPU in nine processes at once.
    With 4, at most 5 do (every rank's worker; the supervisors, whose final torch.distributed.barrier probes the device,
    only after their workers have exited)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "6", "--warmup", "2", "--batch", "8",
           "--dist-backend", "gloo", "--no-cpu-baseline", "--spin-s", "0.2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    c = d["config"]
    assert d["n_gpus"] == 4 and d["steps"] == 6 and d["value"] > 0 and c["global_batch"] == 32
    assert c["dist_fallbacks"] == [] and c["ms_per_step_ranks"]["max"] >= c["ms_per_step_ranks"]["min"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("nsub", [2, 3, 5])
def test_sub_batch_pipelining_inside_the_call_is_exact(gpu_ctx, orc, nsub):
    """Option "sub_batches": the batch call cuts its batch into sub-batches whose overflow pass + gather/ORB
    kernels run on the context's second stream under the next sub-batch's strip kernel (fork / join inside the
    call).  Ragged splits (7 pyramids over 2 / 3 / 5), a dense pyramid that takes the overflow pass in one
    sub-batch only, buckets, a hipGraph capture of the forked call: all identical to the one-launch-group result
    and to the oracle; pislam_frontend_last_stats sums the sub-batches' overflow lists."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import Context
    from pislam_amd.frontend import OrbFrontend
    levels = [(160, 120, 0), (133, 100, 120), (111, 83, 220)]
    rows = 303
    B = 7
    pyr = synth.make_batch(21, B, w0=160, h0=120, vstep=160, levels=levels)
    rng = np.random.default_rng(3)
    for (w, h, r0) in levels:                                   # pyramid 4: uniform noise -> overflow pass
        pyr[4, r0:r0 + h, :w] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dev = torch.device("cuda:0")
    d_pyr = torch.from_numpy(pyr).to(dev)
    try:
        for lbs, lim in ((0, 5), (3, 2)):
            ref = [orc.pyramid(pyr[b], levels, log_bucket=lbs, bucket_limit=lim) for b in range(B)]
            outs = {}
            for n in (1, nsub):
                gpu_ctx.set_option("sub_batches", n)
                fe = OrbFrontend(levels, vstep=160, rows=rows, max_keypoints=8192, log_bucket_size=lbs, bucket_limit=lim,
                                 ctx=gpu_ctx)
                kp, desc, counts = fe.alloc_outputs(B, dev)
                for rep in range(2):                              # the second call starts from emptied overflow lists
                    fe(d_pyr, kp, desc, counts)
                    torch.cuda.synchronize()
                outs[n] = (tuple(t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc)), fe.last_stats())
            (c, k, d), st = outs[nsub]
            assert st == outs[1][1] and st[0] > 0
            for b in range(B):
                okp, odesc, _ = ref[b]
                n = min(len(okp), 8192)
                assert c[b] == len(okp), (nsub, lbs, b)
                assert (k[b, :n] == okp[:n]).all() and (d[b, :n] == odesc[:n]).all(), (nsub, lbs, b)
            assert (outs[1][0][0] == c).all()
    finally:
        gpu_ctx.set_option("sub_batches", 1)
    # the forked call inside a hipGraph capture
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        ctx.set_option("sub_batches", nsub)
        fe = OrbFrontend(levels, vstep=160, rows=rows, max_keypoints=8192, ctx=ctx)
        fe.reserve(B)
        kp, desc, counts = fe.alloc_outputs(B, dev)
        fe(d_pyr, kp, desc, counts)
        side.synchronize()
        want = tuple(t.clone() for t in (kp, desc, counts))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fe(d_pyr, kp, desc, counts)
        for t in (kp, desc, counts):
            t.zero_()
        for _ in range(3):
            g.replay()
        side.synchronize()
        for a, b in zip(want, (kp, desc, counts)):
            assert torch.equal(a, b)
        ctx.close()



@pytest.mark.parametrize("depth", [1, 3])
def test_pipeline_api_keeps_batches_in_flight_and_exact(orc, depth):
    """pislam_pipeline_*: batch k on lane k % depth, ordered after the producer of its input (a copy enqueued on the
    caller's stream right before the submit) and waited for per ticket; every batch equals the oracle."""
    import torch
    from pislam_amd import capi, synth
    from pislam_amd.frontend import OrbFrontend
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    levels = synth.level_table(320, 240, 4)
    rows = synth.pyramid_rows(levels)
    dev = torch.device("cuda:0")
    NB, B = 7, 3
    host = [synth.make_batch(900 + 10 * k, B, w0=320, h0=240, nlevels=4, levels=levels, nshapes=30) for k in range(NB)]
    fe = OrbFrontend(levels, vstep=320, rows=rows, max_keypoints=2048)          # (parameter / level structs only)
    pipe = capi.Pipeline(device=0, depth=depth)
    assert pipe.lib.pislam_pipeline_depth(pipe.h) == depth
    pipe.reserve(fe.params, fe.levels, B)
    prod = torch.cuda.Stream(dev)
    cons = torch.cuda.Stream(dev)
    d_in = [torch.empty((B, rows, 320), dtype=torch.uint8, device=dev) for _ in range(NB)]
    outs = [fe.alloc_outputs(B, dev) for _ in range(NB)]
    pinned = [torch.from_numpy(h).pin_memory() for h in host]
    tickets = []
    with torch.cuda.stream(prod):
        for k in range(NB):
            d_in[k].copy_(pinned[k], non_blocking=True)                        # the producer of batch k's input
            tickets.append(pipe.submit(fe.params, fe.levels, d_in[k], *outs[k], input_stream=prod.cuda_stream))
    assert tickets == list(range(NB))
    assert len({pipe.stream_of(t) for t in tickets}) == min(depth, NB)
    res = []
    with torch.cuda.stream(cons):
        for k in reversed(range(NB)):                                          # consumers wait per ticket, any order
            pipe.wait(tickets[k], cons.cuda_stream)
            res.append((k, [t.to("cpu", non_blocking=True) for t in outs[k]]))
    cons.synchronize()
    with pytest.raises(capi.PislamError):
        pipe.wait(NB, cons.cuda_stream)
    for k, (kp, desc, counts) in res:
        c, kk, d = (t.numpy().view(np.uint32) for t in (counts, kp, desc))
        for b in range(B):
            okp, odesc, _ = orc.pyramid(host[k][b], levels)
            assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (d[b, :len(okp)] == odesc).all(), (k, b)
    pipe.synchronize()
    pipe.close()


@pytest.mark.gpu
def test_pipeline_replays_repeated_calls_from_graphs_and_says_so(orc):
    """A call that repeats exactly on a lane: eager the first time, captured the second time and launched from the graph from then on
    (pislam_pipeline_stats counts each); replays equal the oracle; option "graphs"=0 keeps every call eager; a lane's
    context (pislam_pipeline_lane) takes other calls of the C ABI on the lane's stream."""
    import torch
    from pislam_amd import capi, synth
    from pislam_amd.frontend import OrbFrontend
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    levels = synth.level_table(320, 240, 4)
    rows = synth.pyramid_rows(levels)
    dev = torch.device("cuda:0")
    B, D, R = 2, 2, 5
    host = synth.make_batch(4200, B, w0=320, h0=240, nlevels=4, levels=levels, nshapes=30)
    d_in = torch.from_numpy(host).to(dev)
    fe = OrbFrontend(levels, vstep=320, rows=rows, max_keypoints=2048)
    want = [orc.pyramid(host[b], levels) for b in range(B)]
    for graphs in (1, 0):
        pipe = capi.Pipeline(device=0, depth=D)
        pipe.set_option("graphs", graphs)
        pipe.reserve(fe.params, fe.levels, B)
        outs = [fe.alloc_outputs(B, dev) for _ in range(D)]
        for r in range(R):
            for l in range(D):
                for t in outs[l]:
                    t.zero_()                                  # (on torch's stream; the submit below is ordered after it)
                pipe.submit(fe.params, fe.levels, d_in, *outs[l], input_stream=torch.cuda.current_stream().cuda_stream)
            pipe.synchronize()
            for l in range(D):
                c = outs[l][2].cpu().numpy().view(np.uint32)
                kk = outs[l][0].cpu().numpy().view(np.uint32)
                dd = outs[l][1].cpu().numpy().view(np.uint32)
                for b in range(B):
                    okp, odesc, _ = want[b]
                    assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (dd[b, :len(okp)] == odesc).all(), (graphs, r, l, b)
        st = pipe.stats()
        assert st["submitted"] == D * R
        if graphs:
            assert st["captured"] == D and st["capture_failed"] == 0 and st["replayed_from_graphs"] == D * (R - 1), st
        else:
            assert st["captured"] == 0 and st["replayed_from_graphs"] == 0, st
        lane = pipe.lane(1)                                    # borrowed context: plain batch call on the lane's stream
        k2, d2, c2 = fe.alloc_outputs(B, dev)
        OrbFrontend(levels, vstep=320, rows=rows, max_keypoints=2048, ctx=lane)(d_in, k2, d2, c2)
        pipe.synchronize()
        assert torch.equal(c2, outs[0][2]) and torch.equal(k2, outs[0][0])
        pipe.close()



def test_bucket_mode_graphs_of_two_shapes_on_one_lane_keep_their_own_unit_tables(orc):
    """The bucket selection pass reads a host-built unit table (one record per unit).  Two calls of different shapes that repeat
    alternately on ONE lane are both replayed from their graphs: each graph must keep reading the table of ITS plan — the
    tables are device buffers per distinct content, never rewritten in place (a single rewritten table made the first
    shape's replay read the second shape's records)."""
    import torch
    from pislam_amd import capi, synth
    from pislam_amd.frontend import OrbFrontend
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    shapes = []
    for (w0, h0, nl, B, seed) in ((640, 480, 8, 3, 4300), (320, 240, 4, 2, 4400)):
        levels = synth.level_table(w0, h0, nl)
        rows = synth.pyramid_rows(levels)
        host = synth.make_batch(seed, B, w0=w0, h0=h0, nlevels=nl, levels=levels, nshapes=40)
        fe = OrbFrontend(levels, vstep=w0, rows=rows, max_keypoints=2048, log_bucket_size=4, bucket_limit=3)
        want = [orc.pyramid(host[b], levels, log_bucket=4, bucket_limit=3) for b in range(B)]
        shapes.append((fe, torch.from_numpy(host).to(dev), fe.alloc_outputs(B, dev), want, B))
    pipe = capi.Pipeline(device=0, depth=1)
    pipe.set_option("frame", 0)                             # (small batches: keep them on the path with the selection pass)
    for fe, d_in, out, want, B in shapes:
        pipe.reserve(fe.params, fe.levels, B)
    order = [0, 0, 1, 1, 0, 1, 0, 1, 1, 0]                    # eager, captured, eager, captured, then replays in both orders
    for k, i in enumerate(order):
        fe, d_in, out, want, B = shapes[i]
        for t in out:
            t.zero_()
        pipe.submit(fe.params, fe.levels, d_in, *out, input_stream=torch.cuda.current_stream().cuda_stream)
        pipe.synchronize()
        assert OrbFrontend.PATH_BUCKET_SELECT & fe.last_path_of(pipe.lane(0))
        c = out[2].cpu().numpy().view(np.uint32)
        kk, dd = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(np.uint32)
        for b in range(B):
            okp, odesc, _ = want[b]
            assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (dd[b, :len(okp)] == odesc).all(), (k, i, b)
    st = pipe.stats()
    assert st["captured"] == 2 and st["capture_failed"] == 0 and st["replayed_from_graphs"] == len(order) - 2, st   # (a shape's first call is eager; its second is captured AND launched from the graph)
    pipe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sub_batches", [1, 2])
def test_pipeline_graph_survives_a_workspace_that_moved(orc, sub_batches):
    """A captured call bakes the lane's workspace addresses (and, with sub-batches, the overflow-list layout) into its
    graph.  A LARGER call on the same lane reallocates them: the small call's graph must not be replayed against the
    freed buffers (round-3 advisor finding) — the library notices the moved workspace, runs the call eagerly once and
    captures it again.  Every result equals the oracle."""
    import torch
    from pislam_amd import capi, synth
    from pislam_amd.frontend import OrbFrontend
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    levels = synth.level_table(320, 240, 4)
    rows = synth.pyramid_rows(levels)
    dev = torch.device("cuda:0")
    small, big = 2, 24
    host = synth.make_batch(7700, big, w0=320, h0=240, nlevels=4, levels=levels, nshapes=30)
    d_big = torch.from_numpy(host).to(dev)
    d_small = d_big[:small]
    fe = OrbFrontend(levels, vstep=320, rows=rows, max_keypoints=2048)
    want = [orc.pyramid(host[b], levels) for b in range(big)]
    pipe = capi.Pipeline(device=0, depth=1)
    pipe.set_option("sub_batches", sub_batches)
    o_small, o_big = fe.alloc_outputs(small, dev), fe.alloc_outputs(big, dev)

    def run(d_in, outs, n):
        for t in outs:
            t.zero_()
        pipe.submit(fe.params, fe.levels, d_in, *outs, input_stream=torch.cuda.current_stream().cuda_stream)
        pipe.synchronize()
        c, kk, dd = (t.cpu().numpy().view(np.uint32) for t in (outs[2], outs[0], outs[1]))
        for b in range(n):
            okp, odesc, _ = want[b]
            assert c[b] == len(okp) and (kk[b, :len(okp)] == okp).all() and (dd[b, :len(okp)] == odesc).all(), b

    for _ in range(3):                       # eager, captured (+ launched), replayed
        run(d_small, o_small, small)
    st = pipe.stats()
    assert st["captured"] == 1 and st["replayed_from_graphs"] == 2, st
    run(d_big, o_big, big)                   # first occurrence of a larger call: eager, the workspace moves
    run(d_small, o_small, small)             # the old graph is stale: eager, NOT a replay
    st = pipe.stats()
    assert st["captured"] == 1 and st["replayed_from_graphs"] == 2, st
    run(d_small, o_small, small)             # captured again, against the new workspace
    run(d_small, o_small, small)
    run(d_big, o_big, big)                   # the big call's second occurrence: captured (workspace large enough: no move)
    run(d_small, o_small, small)
    run(d_big, o_big, big)
    st = pipe.stats()
    if sub_batches == 1:
        assert st["captured"] == 3 and st["capture_failed"] == 0 and st["replayed_from_graphs"] == 7, st
    pipe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lbs,limit", [(4, 3), (2, 1), (5, 2), (3, 6), (1, 1), (6, 4)])
def test_bucket_selection_pass_and_in_strip_selection_agree_with_the_oracle(gpu_ctx, orc, lbs, limit):
    """fastExtract's buckets on the batch path, both ways: the default — strips exactly as without buckets, then
    pf::k_bucket_select (one wave per level and cell row: per-bucket top-`limit`, flush order) — and option
    bucket_select = 0 (the selection inside the strips, strips cut on bucket rows; cells of 4..32 px only).  Inputs: sparse
    synthetic pyramids, a level of uniform noise (hundreds of survivors per cell row: the selection pass's dense path) and a
    1280-wide packed level table (x-tiles: a unit collects from several tiles' lists)."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 + lbs)
    cases = []
    levels = synth.level_table(320, 240, 4)
    pyr = synth.make_batch(8100, 3, w0=320, h0=240, nlevels=4, levels=levels, nshapes=30)
    lv0 = levels[1]
    pyr[1, lv0[2]:lv0[2] + lv0[1], :lv0[0]] = rng.integers(0, 256, (lv0[1], lv0[0]), dtype=np.uint8)     # a dense level
    cases.append((levels, 320, synth.pyramid_rows(levels), pyr, 16384))
    wide = synth.packed_level_table(1280, 960)
    rows_w = synth.pyramid_rows(wide)
    cases.append((wide, 1280, rows_w, synth.make_batch(8200, 1, w0=1280, h0=960, vstep=1280, levels=wide), 16384))
    for levels, vstep, rows, pyr, cap in cases:
        want = [orc.pyramid4(pyr[b], levels, log_bucket=lbs, bucket_limit=limit, cap=1 << 17) for b in range(len(pyr))]
        for select in (1, 0):
            if not select and not 2 <= lbs <= 5:
                continue                                  # (in-strip selection: bucket sizes 4..32 only — others take the staged pipeline)
            gpu_ctx.set_option("bucket_select", select)
            gpu_ctx.set_option("pipeline", 2)
            try:
                fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=cap, log_bucket_size=lbs, bucket_limit=limit,
                                 ctx=gpu_ctx)
                kp, desc, counts = fe.alloc_outputs(len(pyr), dev)
                for _ in range(2):
                    fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
                torch.cuda.synchronize()
                assert fe.last_stats()[1] > 0             # (strips of the fused pipeline ran: not the staged fallback)
            finally:
                gpu_ctx.set_option("bucket_select", 1)
                gpu_ctx.set_option("pipeline", 0)
            c, k, d = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
            for b in range(len(pyr)):
                okp, odesc, _ = want[b]
                n = min(len(okp), cap)
                assert c[b] == len(okp), (select, b, int(c[b]), len(okp))
                assert (k[b, :n] == okp[:n]).all() and (d[b, :n] == odesc[:n]).all(), (select, b)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["vga", "1280x960"])
def test_full_batch_properties_with_readme_buckets(gpu_ctx, orc, workload):
    """The README's recommended mode fastExtract<.., 4, 3> at the bench's batch size (256): repeated runs bit-identical,
    results independent of the batch slot, a sample of slots equal to the oracle, at most 3 keypoints per 16 x 16 cell,
    cells in flush order (cell row, bucket, ascending word) inside every level — through the selection pass."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    dev = torch.device("cuda:0")
    if workload == "vga":
        levels4 = [(w, h, r0, 0) for (w, h, r0) in synth.level_table()]
        vstep, rows, cap = 640, 2210, 4096
        base = synth.make_batch(40, 8)
    else:
        levels4 = [tuple(t) for t in synth.packed_level_table(1280, 960)]
        vstep, rows, cap = 1280, synth.pyramid_rows(levels4), 8192
        base = synth.make_batch(40, 8, w0=1280, h0=960, vstep=1280, levels=levels4)
    batch = 256
    d_pyr = torch.from_numpy(base).to(dev)[torch.arange(batch, device=dev) % 8].contiguous()
    fe = OrbFrontend(levels4 if workload != "vga" else [t[:3] for t in levels4], vstep=vstep, rows=rows, max_keypoints=cap,
                     log_bucket_size=4, bucket_limit=3, ctx=gpu_ctx)
    kp, desc, counts = fe.alloc_outputs(batch, dev)
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c1, k1, d1 = (t.cpu().numpy().view(np.uint32).copy() for t in (counts, kp, desc))
    fe(d_pyr, kp, desc, counts)
    torch.cuda.synchronize()
    c2, k2, d2 = (t.cpu().numpy().view(np.uint32) for t in (counts, kp, desc))
    assert (c1 == c2).all() and (k1 == k2).all() and (d1 == d2).all()
    assert fe.last_stats()[1] > 0
    for b in range(8, batch):
        n = min(int(c1[b]), cap)
        assert c1[b] == c1[b % 8] and (k1[b, :n] == k1[b % 8, :n]).all() and (d1[b, :n] == d1[b % 8, :n]).all()
    for b in (1, 6):
        okp, odesc, _ = orc.pyramid4(base[b], levels4, log_bucket=4, bucket_limit=3)
        m = min(len(okp), cap)
        assert c1[b] == len(okp) and (k1[b, :m] == okp[:m]).all() and (d1[b, :m] == odesc[:m]).all()
    for b in range(0, batch, 37):
        n = min(int(c1[b]), cap)
        x, y = (k1[b, :n] >> 12) & 0xFFF, k1[b, :n] & 0xFFF
        pos = 0
        for (w, h, r0, c0) in levels4:
            m = (y >= r0) & (y < r0 + h) & (x >= c0) & (x < c0 + w)
            idx = np.flatnonzero(m)
            assert len(idx) == 0 or (idx[0] == pos and (np.diff(idx) == 1).all())       # levels are contiguous, in order
            pos += len(idx)
            cell = ((y[m] - r0 - 16) >> 4).astype(np.int64) * 4096 + ((x[m] - c0 - 16) >> 4)
            assert (np.diff(cell) >= 0).all()
            words = k1[b, :n][m].astype(np.int64) - ((c0 << 12) | r0)
            same = np.diff(cell) == 0
            assert (np.diff(words)[same] > 0).all()                                       # ascending inside a cell
            assert len(cell) == 0 or np.bincount(np.unique(cell, return_inverse=True)[1]).max() <= 3
        assert pos == n
