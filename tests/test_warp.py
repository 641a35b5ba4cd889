"""The mesh warp (pislam_warp_*: lens undistortion / stereo rectification in front of the pyramid build) against the
integer statement of include/pislam_hip.h, bit for bit.

`ref_warp` is that statement in numpy int64.  Every GPU comparison covers the whole destination buffer: it is
pre-filled with a sentinel, so bytes beyond `width` in a row and between frames must come back untouched, and the
source's row padding holds a byte that is neither the border nor likely image content, so a tap that strays into it
shows up in the output."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SENT = 0xEE          # destination pre-fill
PADB = 0x5B          # source padding (rows, gaps between frames, bytes in front of the first frame)
INVALID = -1
WARP_FUNCS = ["pislam_warp_create", "pislam_warp_destroy", "pislam_warp_mesh_dims", "pislam_warp_info", "pislam_warp_batch"]


# ---- the expectation ------------------------------------------------------------------------------------------------
def mesh_dims(W, H, lc):
    return ((W - 1) >> lc) + 2, ((H - 1) >> lc) + 2


def mesh_coords(m, W, H, lc):
    """s_q8 of every output pixel, int64 [H][W]."""
    m = np.asarray(m, np.int64)
    C = 1 << lc
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    i, fx, j, fy = x >> lc, x & (C - 1), y >> lc, y & (C - 1)
    a = (m[j, i] * (C - fx) + m[j, i + 1] * fx + (C >> 1)) >> lc
    b = (m[j + 1, i] * (C - fx) + m[j + 1, i + 1] * fx + (C >> 1)) >> lc
    return (a * (C - fy) + b * fy + (C >> 1)) >> lc


def ref_warp(mesh_x, mesh_y, lc, W, H, src, SW, SH, border):
    """src: uint8 [B][>= SH][>= SW] (only [:, :SH, :SW] is looked at) -> uint8 [B][H][W]."""
    s5x, s5y = (mesh_coords(mesh_x, W, H, lc) + 4) >> 3, (mesh_coords(mesh_y, W, H, lc) + 4) >> 3
    x0, ax, y0, ay = s5x >> 5, s5x & 31, s5y >> 5, s5y & 31
    img = np.asarray(src)[:, :SH, :SW].astype(np.int64)

    def S(u, v):
        inside = (u >= 0) & (u < SW) & (v >= 0) & (v < SH)
        return np.where(inside[None], img[:, np.clip(v, 0, SH - 1), np.clip(u, 0, SW - 1)], border)

    out = ((32 - ax) * (32 - ay) * S(x0, y0) + ax * (32 - ay) * S(x0 + 1, y0) + (32 - ax) * ay * S(x0, y0 + 1)
           + ax * ay * S(x0 + 1, y0 + 1) + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def affine_mesh(W, H, lc, cx, cy, jitter=0, seed=0):
    """Nodes cx[0] * X + cx[1] * Y + cx[2] (likewise y) at X = i << lc, Y = j << lc, plus a per-node jitter of up
    to +-jitter (Q8) from a fixed seed."""
    mw, mh = mesh_dims(W, H, lc)
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) << lc, np.arange(mh, dtype=np.int64) << lc)
    rng = np.random.default_rng(seed)
    jx = rng.integers(-jitter, jitter + 1, X.shape) if jitter else 0
    jy = rng.integers(-jitter, jitter + 1, X.shape) if jitter else 0
    return ((cx[0] * X + cx[1] * Y + cx[2] + jx).astype(np.int32), (cy[0] * X + cy[1] * Y + cy[2] + jy).astype(np.int32))


def identity_mesh(W, H, lc, dx=0, dy=0):
    return affine_mesh(W, H, lc, (256, 0, dx), (0, 256, dy))


def frames_of(B, SH, SW, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, SH, SW), dtype=np.uint8)


# ---- CPU: declarations, the expectation's anchors, rectify_mesh ----------------------------------------------------------
def test_warp_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "pislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in WARP_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, code), f"{f} is not declared in include/pislam_hip.h"
    assert "typedef struct pislam_warp pislam_warp;" in code
    from pislam_amd import capi, frontend, rectify
    for f in WARP_FUNCS:
        assert f in capi.SYMBOLS
    assert callable(frontend.Warp) and callable(frontend.warpMeshDims) and callable(rectify.rectify_mesh)
    assert callable(frontend.Warp.from_calibration)
    for m in ("info", "close", "__call__", "__del__"):
        assert hasattr(frontend.Warp, m)
    lib = capi.load()
    mw, mh = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.pislam_warp_mesh_dims(752, 480, 3, ctypes.byref(mw), ctypes.byref(mh)) == 0 and (mw.value, mh.value) == (95, 61)
    assert lib.pislam_warp_mesh_dims(1, 1, 6, ctypes.byref(mw), ctypes.byref(mh)) == 0 and (mw.value, mh.value) == (2, 2)
    assert frontend.warpMeshDims(640, 480, 0) == (641, 481)
    for bad in ((0, 1, 0), (1, 0, 0), (4097, 1, 0), (1, 4097, 0), (8, 8, -1), (8, 8, 7)):
        assert lib.pislam_warp_mesh_dims(*bad, ctypes.byref(mw), ctypes.byref(mh)) == INVALID, bad


def test_ref_warp_anchors():
    """The expectation itself, independent of the library."""
    W, H, SW, SH = 37, 23, 50, 41
    src = frames_of(2, SH, SW, 1)
    for lc in (0, 3, 6):
        assert (ref_warp(*identity_mesh(W, H, lc), lc, W, H, src, SW, SH, 7) == src[:, :H, :W]).all()
        assert (ref_warp(*identity_mesh(W, H, lc, 256 * 5, 256 * 9), lc, W, H, src, SW, SH, 7) == src[:, 9:9 + H, 5:5 + W]).all()
        half = ref_warp(*identity_mesh(W, H, lc, 128, 0), lc, W, H, src, SW, SH, 7)
        p = src.astype(np.int64)
        assert (half == ((p[:, :H, :W] + p[:, :H, 1:W + 1] + 1) >> 1)).all()
    # a position of -0.5 px is x0 = -1, ax = 16: half border, half pixel 0
    m = identity_mesh(4, 4, 0, -128, 0)
    assert (ref_warp(*m, 0, 4, 4, src, SW, SH, 200)[:, :, 0] == ((200 + src[:, :4, 0].astype(np.int64) + 1) >> 1)).all()
    # an affine mesh with integer node values is the same function of (x, y) at every cell size
    cx, cy = (300, 20, -700), (-10, 250, -300)
    outs = [ref_warp(*affine_mesh(W, H, lc, cx, cy), lc, W, H, src, SW, SH, 7) for lc in (0, 3, 6)]
    assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all()
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    assert (mesh_coords(affine_mesh(W, H, 3, cx, cy)[0], W, H, 3) == 300 * x + 20 * y - 700).all()


EUROC_K = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]])
EUROC_D = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]


def test_rectify_mesh():
    from pislam_amd import rectify
    K = np.array([[400.0, 0, 320.0], [0, 410.0, 240.0], [0, 0, 1]])
    for lc in (0, 3, 5):
        C = 1 << lc
        mw, mh = mesh_dims(640, 480, lc)
        i, j = np.meshgrid(np.arange(mw), np.arange(mh))
        mx, my = rectify.rectify_mesh(K, [0, 0, 0, 0], None, None, (640, 480), lc)
        assert mx.dtype == np.int32 and mx.shape == (mh, mw) and my.shape == (mh, mw)
        assert (mx == 256 * C * i).all() and (my == 256 * C * j).all()
        P = K.copy()
        P[0, 2] += 3.5
        P[1, 2] -= 2.25
        mx, my = rectify.rectify_mesh(K, np.zeros(5), np.eye(3), P, (640, 480), lc)
        assert (mx == 256 * C * i - 896).all() and (my == 256 * C * j + 576).all()
    # pure k1, closed form at the corner nodes
    k1, lc = -0.2, 4
    mx, my = rectify.rectify_mesh(K, [k1, 0, 0, 0, 0, 0, 0, 0], None, None, (640, 480), lc)
    for (j, i) in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        u, v = (np.arange(mx.shape[1]) * 16)[i], (np.arange(mx.shape[0]) * 16)[j]
        x, y = (u - 320.0) / 400.0, (v - 240.0) / 410.0
        f = 1 + k1 * (x * x + y * y)
        assert abs(int(mx[j, i]) - 256 * (400.0 * x * f + 320.0)) <= 1 and abs(int(my[j, i]) - 256 * (410.0 * y * f + 240.0)) <= 1
    with pytest.raises(ValueError):
        rectify.rectify_mesh(K, [0.1, 0.2, 0.3], None, None, (640, 480), 3)
    # EuRoC cam0: the log_cell 3 mesh against the dense one
    W, H = 752, 480
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    model = [256.0 * s for s in rectify.source_position(EUROC_K, EUROC_D, None, None, x, y)]
    dense = [mesh_coords(m, W, H, 0) for m in rectify.rectify_mesh(EUROC_K, EUROC_D, None, None, (W, H), 0)]
    coarse = [mesh_coords(m, W, H, 3) for m in rectify.rectify_mesh(EUROC_K, EUROC_D, None, None, (W, H), 3)]
    dev0 = max(np.abs(d - m).max() for d, m in zip(dense, model)) / 256.0
    dev3 = max(np.abs(c - d).max() for c, d in zip(coarse, dense)) / 256.0
    print(f"EuRoC: dense mesh {dev0:.4f} px from the model, log_cell 3 mesh {dev3:.4f} px from the dense mesh")
    assert dev0 <= 0.5 / 256 + 1e-9 and dev3 <= dev0 + 0.03
    assert abs(model[0][0, 0] / 256.0 - 0.0) > 30            # (the corner does move by tens of pixels)
    # clipping: a model that throws nodes far out stays inside the node range
    mx, my = rectify.rectify_mesh(K, [5000.0, 0, 0, 0], None, None, (640, 480), 3)
    for m in (mx, my):
        assert m.min() >= -(1 << 23) and m.max() <= (1 << 23) - 1
    assert mx.min() == -(1 << 23) and mx.max() == (1 << 23) - 1


# ---- GPU -------------------------------------------------------------------------------------------------------------
class Device:
    """Flat device buffers around a warp call: frames at an odd offset, padded rows, a gap between frames."""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx, self.lib = torch, ctx, ctx.lib

    def warp(self, mesh, W, H, SW, SH, lc, border):
        from pislam_amd.frontend import Warp
        return Warp(mesh[0], mesh[1], W, H, SW, SH, lc, border, ctx=self.ctx)

    def source(self, frames, pad, gap, off):
        """-> (tensor, numpy view [B][SH][vstep] of the same bytes, vstep, stride)"""
        B, SH, SW = frames.shape
        vs = SW + pad
        stride = SH * vs + gap
        host = np.full(off + B * stride, PADB, np.uint8)
        view = np.lib.stride_tricks.as_strided(host[off:], (B, SH, vs), (stride, vs, 1))
        view[:, :, :SW] = frames
        return self.torch.from_numpy(host).cuda(), vs, stride

    def run(self, warp, frames, pad=0, gap=0, off=0, direct=0, expect=None):
        """One pislam_warp_batch call; asserts the whole destination buffer (sentinel included) equals `expect`."""
        torch = self.torch
        B = frames.shape[0]
        src, svs, sstride = self.source(frames, pad, gap, off)
        dvs = warp.width + pad
        dstride = warp.height * dvs + gap
        dst = torch.full((off + B * dstride,), SENT, dtype=torch.uint8, device="cuda")
        self.ctx.set_option("warp_direct", direct)
        try:
            rc = self.lib.pislam_warp_batch(self.ctx.h, warp.h, src.data_ptr() + off, svs, sstride, dst.data_ptr() + off, dvs,
                                            dstride, B)
        finally:
            self.ctx.set_option("warp_direct", 0)
        assert rc == 0, self.lib.pislam_last_error(self.ctx.h)
        self.ctx.synchronize()
        want = np.full(off + B * dstride, SENT, np.uint8)
        np.lib.stride_tricks.as_strided(want[off:], (B, warp.height, dvs), (dstride, dvs, 1))[:, :, :warp.width] = expect
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{bad.size} bytes differ (direct={direct}), first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}")

    def both(self, warp, frames, expect, **kw):
        for direct in (0, 1):
            self.run(warp, frames, direct=direct, expect=expect, **kw)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    return Device(gpu_ctx)


MATRIX = [(1, 1, 1, 1), (64, 32, 64, 32), (65, 33, 70, 40), (70, 37, 90, 50), (200, 90, 211, 97)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MATRIX + [(33, 20, 50, 30)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_matrix_against_ref_warp(dev, shape):
    """Affine meshes (a slight zoom and shear that overhangs the source) with +-2 px of per-node jitter, borders 0 and
    0xA5, log_cell 0, 3 and 6 (on the small shapes one cell is larger than the whole image; (33, 20) is there for
    that alone), batch 3 with padded strides at an odd address and batch 1 plain, staged and direct."""
    W, H, SW, SH = shape
    for lc in (0, 3, 6):
        mesh = affine_mesh(W, H, lc, (300, 20, -700), (-10, 250, -300), jitter=512, seed=lc + W)
        for border in (0, 0xA5):
            warp = dev.warp(mesh, W, H, SW, SH, lc, border)
            for B, pad, gap, off in ((3, 5, 7, 3), (1, 0, 0, 0)):
                frames = frames_of(B, SH, SW, 10 * lc + B)
                dev.both(warp, frames, ref_warp(*mesh, lc, W, H, frames, SW, SH, border), pad=pad, gap=gap, off=off)
            warp.close()


@pytest.mark.gpu
def test_gpu_borders_and_signs(dev):
    W, H, SW, SH = 81, 49, 80, 48
    frames = frames_of(2, SH, SW, 3)
    for lc in (0, 3):
        cases = {
            "overhang": affine_mesh(W, H, lc, (290, 0, -1300), (0, 300, -1111)),        # -5.08 .. 85.5 px, -4.34 .. 51.9 px
            "half": identity_mesh(W, H, lc, -128, -128),                               # -0.5 px .. SW - 0.5 / SH - 0.5
            "outside_right": identity_mesh(W, H, lc, 256 * (SW + 1), 0),
            "outside_above": identity_mesh(W, H, lc, 0, -256 * (H + 1)),
        }
        for name, mesh in cases.items():
            want = ref_warp(*mesh, lc, W, H, frames, SW, SH, 0xA5)
            if name.startswith("outside"):
                assert (want == 0xA5).all()
            if name == "half":
                p = frames.astype(np.int64)
                assert (want[:, 1:SH, 0] == ((2 * 0xA5 + p[:, :-1, 0] + p[:, 1:, 0] + 2) >> 2)).all()
                assert (want[:, H - 1, W - 1] == ((3 * 0xA5 + p[:, SH - 1, SW - 1] + 2) >> 2)).all()
            warp = dev.warp(mesh, W, H, SW, SH, lc, 0xA5)
            dev.both(warp, frames, want, pad=9, gap=5, off=1)
            warp.close()


@pytest.mark.gpu
def test_gpu_extremes(dev):
    lo, hi = -(1 << 23), (1 << 23) - 1
    frames = frames_of(2, 50, 90, 4)
    for lc in (0, 3, 6):
        mw, mh = mesh_dims(70, 37, lc)
        for vx, vy in ((lo, lo), (hi, hi), (lo, hi)):
            mesh = (np.full((mh, mw), vx, np.int32), np.full((mh, mw), vy, np.int32))
            warp = dev.warp(mesh, 70, 37, 90, 50, lc, 0x33)
            dev.both(warp, frames, np.full((2, 37, 70), 0x33, np.uint8), pad=3)
            warp.close()
    # nodes alternating between the two ends of the range: every product of the statement at its largest
    mw, mh = mesh_dims(70, 37, 6)
    chk = np.indices((mh, mw)).sum(0) & 1
    mesh = (np.where(chk, lo, hi).astype(np.int32), np.where(chk, hi, lo).astype(np.int32))
    warp = dev.warp(mesh, 70, 37, 90, 50, 6, 0x33)
    dev.both(warp, frames, ref_warp(*mesh, 6, 70, 37, frames, 90, 50, 0x33), pad=3)
    warp.close()
    # a 16384 x 2 source sampled near its right end, past it on the last columns
    W, H, SW, SH = 130, 2, 16384, 2
    wide = frames_of(1, SH, SW, 5)
    mesh = identity_mesh(W, H, 3, 256 * (SW - W) + 900, 37)
    warp = dev.warp(mesh, W, H, SW, SH, 3, 9)
    dev.both(warp, wide, ref_warp(*mesh, 3, W, H, wide, SW, SH, 9), pad=1, off=1)
    warp.close()
    # a 4096 x 1 and a 1 x 4096 output
    for (W, H, SW, SH) in ((4096, 1, 300, 7), (1, 4096, 7, 300)):
        src = frames_of(1, SH, SW, 6)
        mesh = affine_mesh(W, H, 5, (18, 3, -200), (2, 18, -150), jitter=300, seed=W)
        warp = dev.warp(mesh, W, H, SW, SH, 5, 0)
        dev.both(warp, src, ref_warp(*mesh, 5, W, H, src, SW, SH, 0), pad=3, off=2)
        warp.close()


@pytest.mark.gpu
def test_gpu_paths(dev):
    W, H = 200, 90
    ident = dev.warp(identity_mesh(W, H, 3), W, H, W + 1, H + 1, 3, 0)
    info = ident.info()
    assert info["tiles"] == 4 * 3 and info["staged"] == info["tiles"] and info["direct"] == 0, info
    assert 0 < info["lds_bytes"] <= 160 * 1024 // 4, info                              # several workgroups per CU
    frames = frames_of(2, H + 1, W + 1, 7)
    dev.both(ident, frames, frames[:, :H, :W], pad=2)
    ident.close()
    # 8x minification: 640 x 400 -> 80 x 50
    big = frames_of(2, 400, 640, 8)
    for lc in (0, 3):
        mesh = affine_mesh(80, 50, lc, (2048, 0, 0), (0, 2048, 0))
        mini = dev.warp(mesh, 80, 50, 640, 400, lc, 0)
        info = mini.info()
        assert info["direct"] >= 1 and info["staged"] + info["direct"] == info["tiles"] == 4, info
        dev.both(mini, big, ref_warp(*mesh, lc, 80, 50, big, 640, 400, 0), pad=4, off=1)
        mini.close()
    # one call with both kinds of tile: the left 64 columns 1:1, the rest minified 8x horizontally and 2x vertically
    W, H, SW, SH, lc = 200, 40, 1200, 90, 3
    mw, mh = mesh_dims(W, H, lc)
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) << lc, np.arange(mh, dtype=np.int64) << lc)
    mesh = (np.where(X <= 64, 256 * X, 256 * 64 + 2048 * (X - 64)).astype(np.int32),
            np.where(X <= 64, 256 * Y, 512 * Y).astype(np.int32))
    mixed = dev.warp(mesh, W, H, SW, SH, lc, 0x11)
    info = mixed.info()
    assert info["staged"] >= 1 and info["direct"] >= 1, info
    src = frames_of(2, SH, SW, 9)
    dev.both(mixed, src, ref_warp(*mesh, lc, W, H, src, SW, SH, 0x11), pad=1, gap=3, off=3)
    mixed.close()


@pytest.mark.gpu
def test_gpu_anchors(dev):
    W, H, SW, SH = 150, 70, 170, 95
    src = frames_of(2, SH, SW, 11)
    p = src.astype(np.int64)
    for lc in (0, 3, 6):
        for mesh, want in ((identity_mesh(W, H, lc), src[:, :H, :W]),
                           (identity_mesh(W, H, lc, 256 * 13, 256 * 21), src[:, 21:21 + H, 13:13 + W]),
                           (identity_mesh(W, H, lc, 128, 0), ((p[:, :H, :W] + p[:, :H, 1:W + 1] + 1) >> 1).astype(np.uint8))):
            warp = dev.warp(mesh, W, H, SW, SH, lc, 0)
            dev.both(warp, src, want, pad=6, off=2)
            warp.close()
    one = frames_of(3, 1, 1, 12)
    for lc in (0, 6):
        warp = dev.warp(identity_mesh(1, 1, lc), 1, 1, 1, 1, lc, 0)
        dev.both(warp, one, one, pad=2, gap=1, off=1)
        warp.close()
    cx, cy = (300, 20, -700), (-10, 250, -300)
    want = ref_warp(*affine_mesh(W, H, 0, cx, cy), 0, W, H, src, SW, SH, 0x77)
    for lc in (0, 3, 6):
        warp = dev.warp(affine_mesh(W, H, lc, cx, cy), W, H, SW, SH, lc, 0x77)
        dev.both(warp, src, want, pad=3)
        warp.close()


@pytest.mark.gpu
def test_gpu_dense_mesh_ignores_its_last_row_and_column(dev):
    W, H, SW, SH = 70, 37, 90, 50
    mesh = [m.copy() for m in affine_mesh(W, H, 0, (300, 20, -700), (-10, 250, -300), jitter=512, seed=2)]
    src = frames_of(1, SH, SW, 12)
    want = ref_warp(*mesh, 0, W, H, src, SW, SH, 1)
    for m in mesh:
        m[-1, :] = np.iinfo(np.int32).max
        m[:, -1] = np.iinfo(np.int32).min
    warp = dev.warp(mesh, W, H, SW, SH, 0, 1)
    dev.both(warp, src, want, pad=1)
    warp.close()


@pytest.mark.gpu
def test_gpu_validation(dev):
    import torch
    from pislam_amd.frontend import Warp
    lib, ctx = dev.lib, dev.ctx
    W, H, SW, SH, lc = 70, 37, 90, 50, 3
    mesh = identity_mesh(W, H, lc)

    def create(W=W, H=H, SW=SW, SH=SH, lc=lc, mx=mesh[0], my=mesh[1], border=0):
        h = ctypes.c_void_p()
        px = mx.ctypes.data if mx is not None else None
        py = my.ctypes.data if my is not None else None
        rc = lib.pislam_warp_create(ctx.h, W, H, SW, SH, lc, px, py, border, ctypes.byref(h))
        if rc == 0:
            lib.pislam_warp_destroy(h)
        else:
            assert not h.value
        return rc

    assert create() == 0
    big = np.zeros((70, 4100), np.int32)                      # enough nodes for whatever shape is refused below
    for kw in (dict(W=0), dict(W=4097), dict(H=0), dict(H=4097), dict(SW=0), dict(SW=16385), dict(SH=0), dict(SH=16385),
               dict(lc=-1), dict(lc=7), dict(border=-1), dict(border=256), dict(mx=None), dict(my=None)):
        assert create(**dict(dict(mx=big, my=big), **kw)) == INVALID, kw
    for axis in (0, 1):
        for v in (1 << 23, -(1 << 23) - 1):
            m = [mesh[0].copy(), mesh[1].copy()]
            m[axis][2, 3] = v
            assert create(mx=m[0], my=m[1]) == INVALID, (axis, v)
            m[axis][2, 3] = v - 1 if v > 0 else v + 1
            assert create(mx=m[0], my=m[1]) == 0, (axis, v)
    with pytest.raises(ValueError):
        Warp(mesh[0][:-1], mesh[1], W, H, SW, SH, lc, ctx=ctx)

    warp = dev.warp(mesh, W, H, SW, SH, lc, 0)
    src = torch.full((3 * SH * SW + 64,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((3 * H * W + 64,), SENT, dtype=torch.uint8, device="cuda")
    host = np.zeros(3 * SH * SW + 64, np.uint8)

    def batch(s=None, svs=SW, sst=SH * SW, d=None, dvs=W, dst_=H * W, B=2, w=None):
        s = src.data_ptr() if s is None else s
        d = dst.data_ptr() if d is None else d
        return lib.pislam_warp_batch(ctx.h, warp.h if w is None else w, s, svs, sst, d, dvs, dst_, B)

    bad = [dict(svs=SW - 1), dict(dvs=W - 1), dict(B=-1), dict(s=host.ctypes.data), dict(d=host.ctypes.data), dict(s=0), dict(d=0),
           dict(w=0),
           dict(s=dst.data_ptr()),                                                 # the same bytes
           dict(s=dst.data_ptr() + 2 * H * W - 1),                                 # src begins on dst's last byte
           dict(d=src.data_ptr() + 2 * SH * SW - 1)]                               # dst begins on src's last byte
    for kw in bad:
        assert batch(**kw) == INVALID, kw
        assert lib.pislam_last_error(ctx.h)
    assert lib.pislam_ctx_set_option(ctx.h, b"warp_direct", 2) == INVALID
    assert lib.pislam_ctx_set_option(ctx.h, b"warp_direct", -1) == INVALID
    assert batch(B=0) == 0
    assert batch(B=0, s=0, d=0) == 0
    ctx.synchronize()
    assert (dst.cpu().numpy() == SENT).all() and (src.cpu().numpy() == 7).all()
    # src ends where dst begins: allowed
    both = torch.full((2 * SH * SW + 2 * H * W,), 7, dtype=torch.uint8, device="cuda")
    assert batch(s=both.data_ptr(), d=both.data_ptr() + 2 * SH * SW) == 0
    ctx.synchronize()
    assert (both.cpu().numpy() == 7).all()                                          # an identity warp of a constant image
    info = (ctypes.c_int32 * 4)()
    assert lib.pislam_warp_info(None, ctypes.byref(info)) == INVALID and lib.pislam_warp_destroy(None) == INVALID
    warp.close()


@pytest.mark.gpu
def test_gpu_warp_then_pyramid_build(dev):
    """Warp (an integer translation) -> PyramidBuilder == PyramidBuilder on the numpy-shifted frames, on every byte the
    build defines."""
    import torch
    from pislam_amd.frontend import PyramidBuilder, Warp
    from test_prep import build_defined_mask
    W, H, SW, SH, B, steps = 96, 80, 110, 101, 2, (2, 1)
    src = frames_of(B, SH, SW, 13)
    warp = Warp(*identity_mesh(W, H, 3, 256 * 9, 256 * 17), W, H, SW, SH, 3, ctx=dev.ctx)
    pb = PyramidBuilder(W, H, steps, ctx=dev.ctx)
    pyr = [torch.full((B, pb.rows, pb.vstep), 0, dtype=torch.uint8, device="cuda") for _ in range(2)]
    warped = warp(torch.from_numpy(src).cuda())
    assert tuple(warped.shape) == (B, H, W)
    pb(warped, pyr[0])
    shifted = np.ascontiguousarray(src[:, 17:17 + H, 9:9 + W])
    pb(torch.from_numpy(shifted).cuda(), pyr[1])
    dev.ctx.synchronize()
    assert (warped.cpu().numpy() == shifted).all()
    mask = build_defined_mask(pb, steps)
    a, b = pyr[0].cpu().numpy(), pyr[1].cpu().numpy()
    assert mask.any() and (a[:, mask] == b[:, mask]).all()
    warp.close()


@pytest.mark.gpu
def test_gpu_warp_is_hipgraph_capturable(gpu_ctx):
    """No workspace, no host round trip: one kernel captured on a side stream of a fresh context without a warm-up
    call, replayed with changed sources in the same tensor."""
    import torch
    from pislam_amd.capi import Context
    from pislam_amd.frontend import Warp
    W, H, SW, SH, lc, B = 70, 37, 90, 50, 3, 2
    mesh = affine_mesh(W, H, lc, (300, 20, -700), (-10, 250, -300), jitter=512, seed=5)
    side = torch.cuda.Stream(torch.device("cuda:0"))
    with torch.cuda.stream(side):
        ctx = Context(device=0, stream=side.cuda_stream)
        warp = Warp(*mesh, W, H, SW, SH, lc, 0xA5, ctx=ctx)
        src = torch.zeros((B, SH, SW), dtype=torch.uint8, device="cuda")
        dst = torch.full((B, H, W + 3), SENT, dtype=torch.uint8, device="cuda")
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            warp(src, dst[:, :, :W])
        for seed in (20, 21):
            frames = frames_of(B, SH, SW, seed)
            src.copy_(torch.from_numpy(frames).cuda())
            dst.fill_(SENT)
            g.replay()
            side.synchronize()
            got = dst.cpu().numpy()
            assert (got[:, :, :W] == ref_warp(*mesh, lc, W, H, frames, SW, SH, 0xA5)).all() and (got[:, :, W:] == SENT).all()
        warp.close()
        ctx.close()
