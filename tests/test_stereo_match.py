"""Rectified stereo matching (pislam_match_stereo_batch).

The semantics are the library's own (include/pislam_hip.h), after ORB-SLAM2's Frame::ComputeStereoMatches.
`ref_stereo_match` below states them independently of the library and of its cell index: an nl x nr brute-force
candidate mask (level span, the right level's row radius, the signed disparity band) with a masked minimum of
dist * 65536 + j, the SADs by direct patch slicing of the level images, the parabola fit in integers, and the median
rule taken literally from a sorted list.  The CPU tests check that reference itself; the GPU tests compare the library
with it bit for bit on all five outputs."""
import ctypes

import numpy as np
import pytest

from test_match_scaled_window import hamming, level_scales, mapped_positions
from test_match_window import (COUNT_INVALID, NONE_U32, SENTINEL, _lv, clamp_count, pack, packed_levels,
                               random_descriptors, random_positions)

BIG = np.int64(1) << 40


# ---- the reference -----------------------------------------------------------------------------------------------
def subpixel_q8(d1, d2, d3):
    """delta_q8 of the parabola through (-1, d1), (0, d2), (1, d3): floor((512 num + den) / (2 den)), 0 if den == 0."""
    num, den = int(d1) - int(d3), 2 * (int(d1) + int(d3) - 2 * int(d2))
    return 0 if den == 0 else (512 * num + den) // (2 * den)


def right_centre(Xr, s):
    """ur0 = floor((Xr * 65536 + floor(s / 2)) / s): the level-ll column of a level-0 X."""
    return (int(Xr) * 65536 + int(s) // 2) // int(s)


def level_image(pyr, t):
    w, h, r0, c0 = _lv(t)
    return np.asarray(pyr)[r0:r0 + h, c0:c0 + w].astype(np.int64)


def sad_curve(limg, rimg, ul, vl, ur0, w, L):
    """[sad(inc) for inc in -L..L], or None when any pixel the refinement reads lies outside the level."""
    h, wd = limg.shape
    if ul - w < 0 or ul + w > wd - 1 or vl - w < 0 or vl + w > h - 1 or ur0 - L - w < 0 or ur0 + L + w > wd - 1:
        return None
    lp = limg[vl - w:vl + w + 1, ul - w:ul + w + 1] - limg[vl, ul]
    out = []
    for inc in range(-L, L + 1):
        c = ur0 + inc
        rp = rimg[vl - w:vl + w + 1, c - w:c + w + 1] - rimg[vl, c]
        out.append(int(np.abs(lp - rp).sum()))
    return out


def refine_one(limg, rimg, ul, vl, ur0, s, w, L, min_disp, max_disp):
    """(disp_q8, sad) of one accepted candidate, or None when steps 3-5 reject it."""
    sads = sad_curve(limg, rimg, ul, vl, ur0, w, L)
    if sads is None:
        return None
    t = int(np.argmin(sads))                             # first minimum: ties go to the smallest inc
    if t == 0 or t == 2 * L:
        return None
    ib = t - L
    delta = subpixel_q8(sads[t - 1], sads[t], sads[t + 1])
    dl = 256 * (ul - ur0 - ib) - delta
    disp = (dl * int(s) + 32768) // 65536                # Python //: floor
    if not (256 * min_disp <= disp <= 256 * max_disp):
        return None
    return max(disp, 1), sads[t]


def median_keep(sads):
    """Which of the accepted SADs survive the median rule: m = sorted(sads)[n // 2], rejected when 10 sad > 21 m."""
    if len(sads) == 0:
        return np.zeros(0, bool)
    m = int(np.sort(np.asarray(sads, np.int64))[len(sads) // 2])
    return np.asarray([10 * int(v) <= 21 * m for v in sads], bool)


def ref_stereo_match(lkp, ld, rkp, rd, lpyr, rpyr, levels, scale_q16, row_radius0, *, span, min_disp, max_disp,
                     max_hamming, w, L, median_filter, d=None):
    """(idx int32, dist uint32, disp_q8 int32, sad uint32 [nl], nstereo) of one pair; lpyr / rpyr: [rows][vstep]."""
    nl, nr = len(lkp), len(rkp)
    idx = np.full(nl, -1, np.int32)
    dist = np.full(nl, NONE_U32, np.uint32)
    disp = np.full(nl, -1, np.int32)
    sad = np.full(nl, NONE_U32, np.uint32)
    if nl == 0 or nr == 0:
        return idx, dist, disp, sad, 0
    rr = np.asarray(row_radius0, np.int64)
    s = np.asarray(scale_q16, np.int64)
    ll, Xl, Yl = mapped_positions(lkp, levels, scale_q16)
    lr, Xr, Yr = mapped_positions(rkp, levels, scale_q16)
    if d is None:
        d = hamming(ld, rd)
    dx = Xl[:, None] - Xr[None, :]
    mask = ((ll[:, None] >= 0) & (lr[None, :] >= 0) & (np.abs(ll[:, None] - lr[None, :]) <= span)
            & (np.abs(Yl[:, None] - Yr[None, :]) <= rr[np.maximum(lr, 0)][None, :])
            & (dx >= min_disp) & (dx <= max_disp))
    key = np.where(mask, d * 65536 + np.arange(nr, dtype=np.int64)[None, :], BIG).min(1)
    has = key < BIG
    idx[:] = np.where(has, key % 65536, -1)
    dist[:] = np.where(has, key // 65536, 0xFFFFFFFF).astype(np.uint32)
    lv = [_lv(t) for t in levels]
    imgs = {}
    for i in np.flatnonzero(has & (key // 65536 <= max_hamming)):
        l, j = int(ll[i]), int(idx[i])
        if l not in imgs:
            imgs[l] = (level_image(lpyr, levels[l]), level_image(rpyr, levels[l]))
        x, y = int((lkp[i] >> 12) & 0xFFF), int(lkp[i] & 0xFFF)
        ul, vl = x - lv[l][3], y - lv[l][2]
        got = refine_one(*imgs[l], ul, vl, right_centre(Xr[j], s[l]), s[l], w, L, min_disp, max_disp)
        if got is not None:
            disp[i], sad[i] = got
    if median_filter:
        acc = np.flatnonzero(sad != NONE_U32)
        drop = acc[~median_keep(sad[acc])]
        disp[drop], sad[drop] = -1, NONE_U32
    return idx, dist, disp, sad, int((sad != NONE_U32).sum())


# ---- CPU: the reference itself -----------------------------------------------------------------------------------
def test_subpixel_fit_and_rounding():
    assert subpixel_q8(30, 10, 50) == -43                # (-10240 + 120) / 240 = -42.2 -> floor -43, not -42
    assert subpixel_q8(50, 10, 30) == 43                 # (10240 + 120) / 240 = 43.2
    assert subpixel_q8(10, 10, 10) == 0                  # den == 0
    assert subpixel_q8(20, 10, 20) == 0                  # symmetric
    assert subpixel_q8(11, 10, 10) == 128 and subpixel_q8(10, 10, 11) == -128     # the extremes: |delta| <= 128
    rng = np.random.default_rng(1)
    for _ in range(2000):
        d2 = int(rng.integers(0, 1000))
        d1, d3 = d2 + int(rng.integers(1, 1000)), d2 + int(rng.integers(0, 1000))
        q = subpixel_q8(d1, d2, d3)
        assert abs(q) <= 128
        assert abs(q - 256 * (d1 - d3) / (2 * (d1 + d3 - 2 * d2))) <= 0.5 + 1e-9


def test_right_centre_is_the_keypoint_column_on_its_own_level():
    from test_match_scaled_window import map_q16
    rng = np.random.default_rng(2)
    for s in [65536, 65537, 78643, 94372, 98304, 131072, 163840, 262144, 1 << 20] + list(rng.integers(65536, 1 << 20, 40)):
        umax = min(4095, (65535 * 65536 - 32768) // int(s))
        for u in list(range(0, min(umax, 64))) + list(rng.integers(0, umax + 1, 200)):
            assert right_centre(map_q16(int(u), int(s)), s) == u, (s, u)


def textured(rng, h, w):
    """A random texture with no flat runs: a box-smoothed noise image."""
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.int64)
    return ((n[:-2, 1:-1] + n[2:, 1:-1] + n[1:-1, :-2] + n[1:-1, 2:] + 4 * n[1:-1, 1:-1]) // 8).astype(np.uint8)


def one_level_pair(d, h=40, w=100, seed=3):
    rng = np.random.default_rng(seed)
    left = textured(rng, h, w + d)
    return left[:, :w].copy(), left[:, d:d + w].copy()   # right(x) = left(x + d): a scene point at x in the left is
                                                          # at x - d in the right


def stereo_one(lx, ly, rx, ry, limg, rimg, **kw):
    levels = [(limg.shape[1], limg.shape[0], 0, 0)]
    args = dict(span=0, min_disp=0, max_disp=64, max_hamming=10, w=3, L=4, median_filter=False)
    args.update(kw)
    z = np.zeros((len(lx), 1), np.uint32)
    return ref_stereo_match(pack(lx, ly), z, pack(rx, ry), np.zeros((len(rx), 1), np.uint32), limg, rimg, levels,
                            [65536], [2], **args)


def test_known_integer_shift():
    d = 9
    limg, rimg = one_level_pair(d)
    for e in (-3, -1, 0, 2, 3):                          # the right keypoint e px off the true match: the SAD finds it
        i, dist, disp, sad, n = stereo_one([50], [20], [50 - d + e], [20], limg, rimg, L=4)
        assert (i[0], dist[0], n, sad[0]) == (0, 0, 1, 0), e
        assert abs(int(disp[0]) - 256 * d) <= 128, e     # sad(ib) = 0: the fit moves it by at most half a pixel
    sads = sad_curve(limg.astype(np.int64), rimg.astype(np.int64), 50, 20, 50 - d, 3, 4)
    assert sads[4] == 0 and min(sads[:4] + sads[5:]) > 0


def test_edge_of_level_rejection():
    d, w, L = 9, 3, 4
    limg, rimg = one_level_pair(d)
    W = limg.shape[1]
    ok = lambda lx, ly, rx: stereo_one([lx], [ly], [rx], [ly], limg, rimg, w=w, L=L)[3][0] != NONE_U32
    assert ok(w + L + d, 20, w + L)                      # every read inside: accepted
    assert not ok(w + L + d - 1, 20, w + L - 1)          # ur0 - L - w = -1
    assert not ok(w - 1, 20, 0) and not ok(50, w - 1, 50 - d) and not ok(50, 40 - w, 50 - d)   # left patch / rows
    assert not ok(W - w, 20, W - w - d)                  # ul + w = W
    limg, rimg = one_level_pair(3)                       # d = 3: the true offset stays inside +-L at the right edge
    assert ok(W - 1 - w, 20, W - 1 - w - L)              # ur0 + L + w = W - 1
    assert not ok(W - 1 - w, 20, W - w - L)              # ur0 + L + w = W: one column past


def test_best_offset_at_the_search_edge_is_rejected():
    d, L = 9, 4
    limg, rimg = one_level_pair(d)
    for e, accepted in ((L - 1, True), (L, False), (-L + 1, True), (-L, False)):
        _, _, disp, sad, n = stereo_one([50], [20], [50 - d + e], [20], limg, rimg, L=L)
        assert (sad[0] != NONE_U32) == accepted and n == int(accepted), e
        if accepted:
            assert abs(int(disp[0]) - 256 * d) <= 128


def test_sad_ties_pick_the_smallest_offset():
    rng = np.random.default_rng(4)
    col = rng.integers(0, 256, 3)
    img = np.tile(col[np.arange(100) % 3], (40, 1)).astype(np.int64)   # period 3: sad(inc) = sad(inc + 3)
    sads = sad_curve(img, img, 50, 20, 50, 2, 5)
    assert sads[5] == 0 and sads[2] == 0 and sads[8] == 0 and int(np.argmin(sads)) == 2
    got = refine_one(img, img, 50, 20, 50, 65536, 2, 5, 0, 64)
    assert got is not None and abs(got[0] - 256 * 3) <= 128 and got[1] == 0    # ib = -3 (not 0 or +3)
    flat = np.full((40, 100), 77, np.int64)              # every sad 0: ib = -L, rejected
    assert refine_one(flat, flat, 50, 20, 50, 65536, 2, 5, 0, 64) is None


def test_median_rule():
    assert list(median_keep([0, 0, 0, 5])) == [True, True, True, False]                 # m = 0 keeps only zeros
    assert list(median_keep([0, 1])) == [True, True]                                      # n = 2: m = sorted[1] = 1
    assert list(median_keep([1, 0])) == [True, True]
    assert list(median_keep([10, 20, 21, 45, 44])) == [True, True, True, False, True]     # odd n: m = 21: 450 > 441
    assert list(median_keep([10, 20, 30, 63, 64])) == [True, True, True, True, False]     # m = 30: 630 <= 630
    assert list(median_keep([7, 1, 100, 2])) == [True, True, False, True]                 # even n: m = sorted[2] = 7
    assert list(median_keep([5])) == [True]
    assert len(median_keep([])) == 0


def test_reference_band_and_median_on_a_shifted_scene():
    """Many keypoints of a shifted one-level pair: the band finds the twin, a decoy outside the band is ignored, and
    the median filter removes the matches whose patches were corrupted."""
    d = 12
    limg, rimg = one_level_pair(d, h=60, w=160, seed=5)
    xs = np.arange(30, 140, 7)
    ys = np.full(len(xs), 30)
    ld = np.arange(len(xs), dtype=np.uint32)[:, None] * np.uint32(0x01010101)
    rx = np.concatenate([xs - d, xs - d - 70])             # twins, and decoys 70 px further (outside max_disp 64)
    rdesc = np.concatenate([ld, ld])
    lv = [(160, 60, 0, 0)]
    rb = rimg.copy()
    rb[25:36, xs[3] - d - 8:xs[3] - d + 9] = 255 - rb[25:36, xs[3] - d - 8:xs[3] - d + 9]   # one patch corrupted
    kw = dict(span=0, min_disp=0, max_disp=64, max_hamming=0, w=5, L=5)
    for mf in (False, True):
        i, dist, disp, sad, n = ref_stereo_match(pack(xs, ys), ld, pack(rx, np.concatenate([ys, ys])), rdesc, limg, rb, lv, [65536], [2],
                                                 median_filter=mf, **kw)
        assert (i == np.arange(len(xs))).all() and (dist == 0).all()
        good = np.flatnonzero(sad != NONE_U32)
        assert n == len(good) and len(good) >= len(xs) - 4
        clean = good[sad[good] == 0]
        assert len(clean) >= len(xs) - 3 and (np.abs(disp[clean].astype(np.int64) - 256 * d) <= 128).all()
        if mf:                                           # m = 0: only the zero-SAD matches stay
            assert 3 not in good and (sad[good] == 0).all()
        else:
            assert 3 in good and sad[3] > 0


# ---- GPU ---------------------------------------------------------------------------------------------------------
def host_pyramid(l0, levels, vstep, rows):
    from pislam_amd import synth
    out = np.zeros((rows, vstep), np.uint8)
    h0, w0 = l0.shape
    for t in levels:
        w, h, r0, c0 = _lv(t)
        out[r0:r0 + h, c0:c0 + w] = l0 if (w, h) == (w0, h0) else synth._resize_bilinear(l0, w, h)
    return out


def stereo_inputs(B, d, layout, seed=0, max_kp=None, log_bucket_size=0):
    """B synthetic stereo pairs: left = synth frame, right = the same frame shifted left by d (right(x) = left(x + d),
    the last d columns wrapped round), host-built pyramids of `layout`, both through OrbFrontend as one batch of 2B.
    Returns levels, (lpyr, rpyr) uint8 [B][rows][vstep], and (kp, desc, counts) of the left and of the right."""
    import torch
    from pislam_amd import synth
    from pislam_amd.frontend import OrbFrontend
    w0, h0 = (640, 480) if layout == "vga" else (1280, 960)
    levels = synth.level_table(w0, h0) if layout == "vga" else packed_levels()
    vstep, rows = w0, synth.pyramid_rows(levels)
    max_kp = max_kp or (2048 if layout == "vga" else 4096)
    pyr = np.zeros((2 * B, rows, vstep), np.uint8)
    for b in range(B):
        l0 = synth.make_level0(seed + b, w0, h0, None if layout == "vga" else 148)
        pyr[b] = host_pyramid(l0, levels, vstep, rows)
        pyr[B + b] = host_pyramid(np.roll(l0, -d, axis=1), levels, vstep, rows)
    dev = torch.device("cuda:0")
    fe = OrbFrontend(levels, vstep=vstep, rows=rows, max_keypoints=max_kp, log_bucket_size=log_bucket_size)
    kp, desc, counts = fe.alloc_outputs(2 * B, dev)
    fe(torch.from_numpy(pyr).to(dev), kp, desc, counts)
    torch.cuda.synchronize()
    kp, desc, counts = (kp.cpu().numpy().view(np.uint32), desc.cpu().numpy().view(np.uint32),
                        counts.cpu().numpy().view(np.uint32))
    return levels, (pyr[:B], pyr[B:]), (kp[:B], desc[:B], counts[:B]), (kp[B:], desc[B:], counts[B:])


def row_radii(scale_q16):
    return [int(np.floor(2 * s / 65536 + 0.5)) for s in scale_q16]


def run_stereo(ctx, levels, s, rr, pyrs, left, right, fill=SENTINEL, **kw):
    """Host arrays in, host arrays out: (idx, dist, disp_q8, sad) [B][l_stride] as uint32 bit patterns, nstereo [B]."""
    import torch
    from pislam_amd.frontend import matchStereoBatch
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    lkp, ld, lc = left
    rkp, rd, rc = right
    B, ls = lkp.shape
    f = fill - (1 << 32) if fill >= 1 << 31 else fill
    outs = [torch.full((B, ls), f, dtype=torch.int32, device=dev) for _ in range(4)]
    ns = torch.full((B,), f, dtype=torch.int32, device=dev)
    P = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pyrs]
    matchStereoBatch(T(lkp), T(ld), T(lc), T(rkp), T(rd), T(rc), P[0], P[1], levels, s, rr, *[], idx=outs[0],
                     dist=outs[1], disp_q8=outs[2], sad=outs[3], nstereo=ns, ctx=ctx, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32) for o in outs], ns.cpu().numpy().view(np.uint32)


KW = dict(min_disp=0, max_disp=64, max_hamming=74, level_span=1, sad_radius=5, search_radius=5, median_filter=True)


def check_stereo(got, levels, s, rr, pyrs, left, right, fill=SENTINEL, dmats=None, **kw):
    (gi, gd, gp, gs), gn = got
    p = dict(KW)
    p.update(kw)
    lkp, ld, lc = left
    rkp, rd, rc = right
    ls, rs = lkp.shape[1], rkp.shape[1]
    for b in range(lkp.shape[0]):
        nl, nr = clamp_count(lc[b], ls), clamp_count(rc[b], rs)
        ei, ed, ep, es, en = ref_stereo_match(
            lkp[b, :nl], ld[b, :nl], rkp[b, :nr], rd[b, :nr], pyrs[0][b], pyrs[1][b], levels, s, rr,
            span=p["level_span"], min_disp=p["min_disp"], max_disp=p["max_disp"], max_hamming=p["max_hamming"],
            w=p["sad_radius"], L=p["search_radius"], median_filter=p["median_filter"],
            d=None if dmats is None else dmats[b])
        bad = np.flatnonzero(gi[b, :nl].view(np.int32) != ei)[:5]
        assert (gi[b, :nl].view(np.int32) == ei).all(), (b, bad)
        assert (gd[b, :nl] == ed).all(), b
        bad = np.flatnonzero(gp[b, :nl].view(np.int32) != ep)[:5]
        assert (gp[b, :nl].view(np.int32) == ep).all(), (b, bad, gp[b, bad].view(np.int32), ep[bad])
        assert (gs[b, :nl] == es).all(), b
        assert int(gn[b]) == en, (b, int(gn[b]), en)
        for g in (gi, gd, gp, gs):
            assert (g[b, nl:] == fill).all(), ("slot past the left count written", b)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["vga", "packed"])
def test_gpu_stereo_on_frontend_outputs(gpu_ctx, layout):
    B = 4
    levels, pyrs, left, right = stereo_inputs(B, 16, layout, seed=10 if layout == "vga" else 20)
    right[2][2] = 0                                       # one pair without right keypoints
    left[2][3] = 5000                                     # a left count above the stride (clamped)
    s = level_scales(levels)
    rr = row_radii(s)
    for span in (0, 1, 2):
        for mf in (True, False):
            got = run_stereo(gpu_ctx, levels, s, rr, pyrs, left, right, level_span=span, median_filter=mf,
                             **{k: v for k, v in KW.items() if k not in ("level_span", "median_filter")})
            check_stereo(got, levels, s, rr, pyrs, left, right, level_span=span, median_filter=mf)
            assert int(got[1][0]) > 50
    for mx in (16, 448):                                  # a narrow band and ORB-SLAM2's default one
        got = run_stereo(gpu_ctx, levels, s, rr, pyrs, left, right, **{**KW, "max_disp": mx, "min_disp": 1})
        check_stereo(got, levels, s, rr, pyrs, left, right, max_disp=mx, min_disp=1)


def random_image_pyramids(rng, B, levels, vstep, rows, d):
    """Textured random stacked pyramids; the right one is the left shifted by d on every level, plus noise."""
    lp = np.zeros((B, rows, vstep), np.uint8)
    rp = np.zeros((B, rows, vstep), np.uint8)
    for b in range(B):
        for t in levels:
            w, h, r0, c0 = _lv(t)
            img = textured(rng, h, w + d)
            lp[b, r0:r0 + h, c0:c0 + w] = img[:, :w]
            noise = rng.integers(-2, 3, (h, w))
            rp[b, r0:r0 + h, c0:c0 + w] = np.clip(img[:, d:d + w].astype(np.int64) + noise, 0, 255)
    return lp, rp


def stereo_positions(rng, lkp_b, n, levels, s, rr, d):
    """Right positions: half of them the left ones moved by about d level-0 pixels (band edges: row offsets rr and
    rr + 1, disparity offsets), on a level within 2 of the left's, the rest anywhere."""
    r = random_positions(rng, n, levels, 5)
    if len(lkp_b) == 0 or n == 0:
        return r
    lv = [_lv(t) for t in levels]
    ll, Xl, Yl = mapped_positions(lkp_b, levels, s)
    src = rng.integers(0, len(lkp_b), n)
    for k in np.flatnonzero(rng.random(n) < 0.5):
        j = src[k]
        if ll[j] < 0:
            continue
        l = int(np.clip(ll[j] + rng.integers(-2, 3), 0, len(lv) - 1))
        w, h, r0, c0 = lv[l]
        R = int(rr[l])
        X = Xl[j] - d + int(rng.choice([0, 1, -1, 3, -3, d + 1, 64 - d, 65 - d]))
        Y = Yl[j] + int(rng.choice([0, 1, -1, R, -R, R + 1, -R - 1]))
        u = int(np.clip(np.floor(X * 65536 / s[l] + rng.integers(-1, 2)), 0, w - 1))
        v = int(np.clip(np.floor(Y * 65536 / s[l] + rng.integers(-1, 2)), 0, h - 1))
        r[k] = pack([c0 + u], [r0 + v])[0]
    return r


PAIRS = [(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (1000, 1000), (1000, 1), (1, 1000), (64, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["demo", "packed"])
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_gpu_stereo_random_positions(gpu_ctx, layout, words):
    from pislam_amd import synth
    levels = synth.level_table() if layout == "demo" else packed_levels()
    vstep = 640 if layout == "demo" else 1280
    rows = synth.pyramid_rows(levels)
    stride, B, d = 1000, len(PAIRS), 10
    rng = np.random.default_rng([words, len(levels)])
    s = level_scales(levels)
    pyrs = random_image_pyramids(rng, B, levels, vstep, rows, d)
    lc = np.array([p[0] for p in PAIRS], np.uint32)
    rc = np.array([p[1] for p in PAIRS], np.uint32)
    lkp = np.zeros((B, stride), np.uint32)
    rkp = np.zeros((B, stride), np.uint32)
    ld = np.zeros((B, stride, words), np.uint32)
    rd = np.zeros((B, stride, words), np.uint32)
    for b, (nl, nr) in enumerate(PAIRS):
        lkp[b, :nl] = random_positions(rng, nl, levels, 5)
        ld[b, :nl] = random_descriptors(rng, nl, words)
        rkp[b, :nr] = stereo_positions(rng, lkp[b, :nl], nr, levels, s, row_radii(s), d)
        rd[b, :nr] = random_descriptors(rng, nr, words)
        if nl and nr:                                    # half of the right keypoints carry a left descriptor
            near = rng.random(nr) < 0.5
            rd[b, :nr] = np.where(near[:, None], ld[b, rng.integers(0, nl, nr)], rd[b, :nr])
    dm = [hamming(ld[b, :clamp_count(lc[b], stride)], rd[b, :clamp_count(rc[b], stride)]) for b in range(B)]
    left, right = (lkp, ld, lc), (rkp, rd, rc)
    settings = [dict(), dict(level_span=0, median_filter=False), dict(level_span=2, sad_radius=1, search_radius=1),
                dict(sad_radius=7, search_radius=8, min_disp=5, max_disp=20, max_hamming=words * 8),
                dict(sad_radius=3, search_radius=2, max_hamming=0, median_filter=False),
                dict(min_disp=0, max_disp=65535, max_hamming=1 << 20)]                  # dense bands
    for k, st in enumerate(settings):
        rr = row_radii(s) if k % 2 == 0 else [int(v) for v in rng.choice([0, 1, 3, 40], len(levels))]
        p = {**KW, **st}
        got = run_stereo(gpu_ctx, levels, s, rr, pyrs, left, right, **p)
        check_stereo(got, levels, s, rr, pyrs, left, right, dmats=dm, **p)


@pytest.mark.gpu
def test_gpu_stereo_full_right_stride(gpu_ctx):
    """r_stride = 65535 (the largest index the dist << 16 | index key holds), one pair filled to the stride."""
    from pislam_amd import synth
    rng = np.random.default_rng(65535)
    levels = synth.level_table()
    rows = synth.pyramid_rows(levels)
    s = level_scales(levels)
    rr = row_radii(s)
    rs, ls, words, d = 65535, 70, 4, 10
    pyrs = random_image_pyramids(rng, 2, levels, 640, rows, d)
    rkp = np.zeros((2, rs), np.uint32)
    rd = np.zeros((2, rs, words), np.uint32)
    rkp[0] = pack(rng.integers(0, 640, rs), rng.integers(0, 480, rs))
    rkp[1, :100] = random_positions(rng, 100, levels, 5)
    rd[0] = random_descriptors(rng, rs, words)
    rd[1, :100] = random_descriptors(rng, 100, words)
    lkp = np.zeros((2, ls), np.uint32)
    ld = np.zeros((2, ls, words), np.uint32)
    x, y = (rkp[0, rs - 65:] >> 12) & 0xFFF, rkp[0, rs - 65:] & 0xFFF
    lkp[0, :65] = pack(np.minimum(x + d, 639), y)          # find the last indices
    ld[0, :65] = rd[0, rs - 65:]
    lkp[0, 65:] = pack([0, 639, 0, 639, 320], [0, 0, 479, 479, 240])
    lkp[1] = random_positions(rng, ls, levels, 5)
    ld[1] = random_descriptors(rng, ls, words)
    lc = np.array([ls, ls], np.uint32)
    rc = np.array([rs, 100], np.uint32)
    for mx in (64, 448):
        p = {**KW, "max_disp": mx}
        got = run_stereo(gpu_ctx, levels, s, rr, pyrs, (lkp, ld, lc), (rkp, rd, rc), **p)
        check_stereo(got, levels, s, rr, pyrs, (lkp, ld, lc), (rkp, rd, rc), **p)
        assert (got[0][1][0, :65] == 0).all()


@pytest.mark.gpu
def test_gpu_stereo_shifted_copy_property(gpu_ctx):
    """Left frame and its copy shifted by d = 16 px, no buckets, a keypoint capacity that drops nothing: a level-0
    left keypoint at least d + 32 px from the left and right edges and 32 px from the top and bottom has an identical
    right keypoint at (x - d, y) (blur, FAST, Harris, NMS and ORB are local and commute with the shift).  With the
    filter off all but a tiny fraction of them must find that twin at distance 0 with |disp_q8 - 256 d| <= 128."""
    B, d = 8, 16
    levels, pyrs, left, right = stereo_inputs(B, d, "vga", seed=30, max_kp=8192)
    s = level_scales(levels)
    rr = row_radii(s)
    lkp, ld, lc = left
    rkp, rd, rc = right
    assert (lc < 8192).all() and (rc < 8192).all()
    (gi, gd, gp, gs), _ = run_stereo(gpu_ctx, levels, s, rr, pyrs, left, right, **{**KW, "median_filter": False})
    total = good = 0
    for b in range(B):
        n = int(lc[b])
        x, y = (lkp[b, :n] >> 12) & 0xFFF, lkp[b, :n] & 0xFFF
        inner = np.flatnonzero((y < 480) & (x >= d + 32) & (x < 640 - d - 32) & (y >= 32) & (y < 480 - 32))
        rpos = rkp[b, :int(rc[b])] & 0xFFFFFF
        total += len(inner)
        for i in inner:
            j = int(gi[b, i].view(np.int32))
            twin = pack([x[i] - d], [y[i]])[0]
            ok = (j >= 0 and rpos[j] == twin and gd[b, i] == 0 and (rd[b, j] == ld[b, i]).all()
                  and abs(int(gp[b, i].view(np.int32)) - 256 * d) <= 128)
            good += ok
    assert total > 500
    # observed on an MI355X: 772 of 772 (no miss); the bound leaves 1 % for ties between identical descriptors of two
    # right keypoints inside the band
    assert good >= 0.99 * total, (good, total)


@pytest.mark.gpu
def test_gpu_stereo_invalid_counts_and_untouched_slots(gpu_ctx):
    from pislam_amd import synth
    rng = np.random.default_rng(3)
    levels = synth.level_table()
    rows = synth.pyramid_rows(levels)
    s = level_scales(levels)
    rr = row_radii(s)
    words, n, d = 2, 128, 8
    pyrs = random_image_pyramids(rng, 4, levels, 640, rows, d)
    lkp = np.stack([random_positions(rng, n, levels, 5) for _ in range(4)])
    rkp = np.stack([stereo_positions(rng, lkp[b], n, levels, s, rr, d) for b in range(4)])
    ld = np.stack([random_descriptors(rng, n, words) for _ in range(4)])
    rd = ld.copy()
    lc = np.array([COUNT_INVALID, 100, 100, 50], np.uint32)
    rc = np.array([100, COUNT_INVALID, 100, 0], np.uint32)
    for fill in (SENTINEL, 0xFFFFFFFF, 0):
        got = run_stereo(gpu_ctx, levels, s, rr, pyrs, (lkp, ld, lc), (rkp, rd, rc), fill=fill, **KW)
        check_stereo(got, levels, s, rr, pyrs, (lkp, ld, lc), (rkp, rd, rc), fill=fill)
        (gi, gd, gp, gs), gn = got
        assert all((g[0] == fill).all() for g in (gi, gd, gp, gs)) and gn[0] == 0
        assert (gi[1, :100].view(np.int32) == -1).all() and (gs[1, :100] == NONE_U32).all() and gn[1] == 0
        assert (gi[2, :100].view(np.int32) >= 0).any()


@pytest.mark.gpu
def test_gpu_stereo_rejects_bad_arguments(gpu_ctx):
    """Every invalid argument returns PISLAM_ERR_INVALID and leaves the outputs as they were."""
    import torch
    from pislam_amd import synth
    from pislam_amd.capi import PislamError
    from pislam_amd.frontend import matchStereoBatch, reserveMatchStereo
    dev = torch.device("cuda:0")
    lv = synth.level_table()
    rows = synth.pyramid_rows(lv)
    s = level_scales(lv)
    kp = torch.zeros((2, 16), dtype=torch.int32, device=dev)
    desc = torch.zeros((2, 16, 8), dtype=torch.int32, device=dev)
    cnt = torch.full((2,), 16, dtype=torch.int32, device=dev)
    pyr = torch.zeros((2, rows, 640), dtype=torch.uint8, device=dev)
    outs = [torch.full((2, 16), SENTINEL, dtype=torch.int32, device=dev) for _ in range(4)]
    ns = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)

    def call(ld=desc, rk=kp, rd=desc, levels=lv, scale=s, rr=2, lk=kp, lc=cnt, rc=cnt, lp=pyr, rp=pyr, n=ns, **kw):
        p = {**KW, **kw}
        matchStereoBatch(lk, ld, lc, rk, rd, rc, lp, rp, levels, scale, rr, idx=outs[0], dist=outs[1],
                         disp_q8=outs[2], sad=outs[3], nstereo=n, ctx=gpu_ctx, **p)

    call()
    torch.cuda.synchronize()
    for o in outs + [ns]:
        o.fill_(SENTINEL)
    d3 = torch.zeros((2, 16, 3), dtype=torch.int32, device=dev)
    big_kp = torch.zeros((2, 65536), dtype=torch.int32, device=dev)
    big_desc = torch.zeros((2, 65536, 8), dtype=torch.int32, device=dev)
    short = torch.zeros((2, rows - 1, 640), dtype=torch.uint8, device=dev)
    narrow = torch.zeros((2, rows, 600), dtype=torch.uint8, device=dev)
    bad = [dict(ld=d3, rd=d3), dict(rk=big_kp, rd=big_desc),
           dict(rr=-1), dict(rr=65536), dict(rr=[2] * 7 + [65536]),
           dict(level_span=-1), dict(level_span=8), dict(levels=lv[:1], scale=s[:1], level_span=1),
           dict(levels=[], scale=[], rr=[], level_span=0),
           dict(levels=[(10, 10, 10 * i, 0) for i in range(17)], scale=[65536] * 17, level_span=0),
           dict(levels=[(640, 480, 0, 0), (100, 100, 479, 0)], scale=[65536, 65536]),
           dict(levels=[(4000, 100, 0, 100)], scale=[65536], level_span=0),
           dict(scale=0), dict(scale=(1 << 20) + 1),
           dict(lp=short, rp=short), dict(lp=narrow, rp=narrow),                 # levels outside rows x vstep
           dict(min_disp=-1), dict(min_disp=10, max_disp=9), dict(max_disp=65536), dict(max_hamming=-1),
           dict(sad_radius=0), dict(sad_radius=8), dict(search_radius=0), dict(search_radius=9),
           dict(median_filter=2),
           dict(lk=kp.cpu(), ld=desc.cpu(), lc=cnt.cpu()), dict(rk=kp.cpu(), rd=desc.cpu(), rc=cnt.cpu()),
           dict(lp=pyr.cpu(), rp=pyr.cpu()), dict(n=ns.cpu())]
    for kw in bad:
        with pytest.raises(PislamError):
            call(**kw)
    torch.cuda.synchronize()
    for o in outs + [ns]:
        assert (o == SENTINEL).all()
    for kw in (dict(words=3), dict(r_stride=65536), dict(rr=65536), dict(level_span=8), dict(sad_radius=8),
               dict(median_filter=-1), dict(min_disp=5, max_disp=4)):
        args = dict(levels=lv, scale=s, rr=2, r_stride=16, batch=2, words=8, **KW)
        args.update(kw)
        with pytest.raises(PislamError):
            reserveMatchStereo(args.pop("levels"), args.pop("scale"), args.pop("rr"), args.pop("r_stride"),
                               args.pop("batch"), ctx=gpu_ctx, **args)


@pytest.mark.gpu
def test_gpu_stereo_call_is_hipgraph_capturable(gpu_ctx):
    """After pislam_match_stereo_reserve the call allocates nothing and never synchronises: capture one call (C entry
    point, host tables of this test's own) on a side stream, replay it and compare with the eager call; then change
    the host tables and the inputs, replay and compare with the reference for the tables as captured."""
    import torch
    from pislam_amd.capi import Context, Level, StereoParams
    from pislam_amd.frontend import matchStereoBatch, reserveMatchStereo
    B = 3
    levels, pyrs, left, right = stereo_inputs(B + 1, 16, "vga", seed=40)
    s = level_scales(levels)
    rr = row_radii(s)
    nl, ls, words = len(levels), left[0].shape[1], left[1].shape[2]
    rows, vstep = pyrs[0].shape[1], pyrs[0].shape[2]
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    U = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lk, ld, lc = (T(a[:B]) for a in left)
    rk, rd, rc = (T(a[:B]) for a in right)
    lp, rp = U(pyrs[0][:B]), U(pyrs[1][:B])
    lv_c = (Level * nl)(*[Level(*_lv(t)) for t in levels])
    s_c = (ctypes.c_int32 * nl)(*s)
    r_c = (ctypes.c_int32 * nl)(*rr)
    p_c = StereoParams(1, 0, 64, 74, 5, 5, 1)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        reserveMatchStereo(levels, s, rr, ls, B, words=words, ctx=ctx, **{k: v for k, v in KW.items()})
        outs = [torch.zeros((B, ls), dtype=torch.int32, device=dev) for _ in range(4)]
        ns = torch.zeros((B,), dtype=torch.int32, device=dev)

        def capi_call():
            ctx.check(ctx.lib.pislam_match_stereo_batch(
                ctx.h, words, lv_c, nl, s_c, r_c, ctypes.byref(p_c), lp.data_ptr(), rp.data_ptr(), vstep, rows,
                rows * vstep, lk.data_ptr(), ld.data_ptr(), lc.data_ptr(), ls, rk.data_ptr(), rd.data_ptr(),
                rc.data_ptr(), ls, B, *[o.data_ptr() for o in outs], ns.data_ptr()), "pislam_match_stereo_batch")

        capi_call()
        side.synchronize()
        eager = matchStereoBatch(lk, ld, lc, rk, rd, rc, lp, rp, levels, s, rr, ctx=ctx, **KW)
        side.synchronize()
        for a, b in zip(eager, outs + [ns]):
            assert torch.equal(a, b)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            capi_call()
        for o in outs + [ns]:
            o.zero_()
        g.replay()
        side.synchronize()
        for a, b in zip(eager, outs + [ns]):
            assert torch.equal(a, b)
        for l in range(nl):                               # the graph keeps the tables it was captured with
            s_c[l], r_c[l] = 65536, 0
        p_c.max_disp, p_c.median_filter = 1, 0
        for o in outs + [ns]:
            o.zero_()
        for dst, a in zip((lk, ld, lc, rk, rd, rc), (*left, *right)):
            dst.copy_(T(a[1:]))
        lp.copy_(U(pyrs[0][1:])), rp.copy_(U(pyrs[1][1:]))
        g.replay()
        side.synchronize()
    got = ([o.cpu().numpy().view(np.uint32) for o in outs], ns.cpu().numpy().view(np.uint32))
    sub = lambda t: tuple(a[1:] for a in t)
    check_stereo(got, levels, s, rr, sub(pyrs), sub(left), sub(right), fill=0)
    assert (got[1] > 0).all()
